"""GPU: on-device multi-sweep merge + collation (csrc/merge.hip) against its exact twin (tests/merge_ref.py: the whole buffer, bit for
bit) and against the numpy restatement of nusc.py:76-121 / waymo.py:49-67 / collate.py:15-22 (oracle.merge_sweeps): row order and kept set exact,
coordinates exact up to the fp64 dot product's summation order (<= 1 ulp of fp32), and the merged buffer drives the reader to the same canvas as the
host path.  The seams of the kernels and the sizes past one level-2 scan pass are in tests/test_gpu_merge_seams.py."""
import merge_ref as M
import numpy as np
import pytest
from merge_ref import sample as _sample  # noqa: F401  (tests/test_gpu_workspace.py imports it from here)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dataset", ["nuscenes", "waymo"])
def test_merge_matches_the_host_path(oracle, dataset):
    from pillarnext_amd.io import SweepMerger

    rng = np.random.default_rng(11)
    sweeps = []
    for b in range(3):
        sweeps += _sample(rng, b, 10 if dataset == "nuscenes" else 3, 3000, radius=1.0 if dataset == "nuscenes" else 0.0)
    ref = oracle.merge_sweeps(sweeps, n_copy=4)
    raw = np.concatenate([s["points"] for s in sweeps])
    segs, o = [], 0
    for s in sweeps:
        segs.append(dict(begin=o, end=o + len(s["points"]), batch=s["batch"], time=s["time"], radius=s["radius"], transform=s["transform"]))
        o += len(s["points"])
    out, n_out = SweepMerger()(torch.from_numpy(raw).cuda(), segs, n_copy=4)
    n = int(n_out.item())
    twin, n_twin = M.merge(raw, segs, 4)
    assert n == n_twin
    M.assert_same_bits(out.cpu().numpy(), twin, dataset)                                             # every row, the tail included, bit for bit
    assert n == len(ref) and n < len(raw) or dataset == "waymo"
    got = out[:n].cpu().numpy()
    assert np.array_equal(got[:, 0], ref[:, 0]) and np.array_equal(got[:, 4:], ref[:, 4:])       # batch, intensity, time: exact, same order
    np.testing.assert_allclose(got[:, 1:4], ref[:, 1:4], rtol=0, atol=4e-6)                          # <= 1 ulp at |x| <= 40
    assert float(np.mean(got[:, 1:4] == ref[:, 1:4])) > 0.999


def test_merged_buffer_feeds_the_reader(oracle):
    from pillarnext_amd import synth
    from pillarnext_amd.io import SweepMerger
    from test_gpu_reader import make_net

    cfg = synth.CONFIGS["C1"]
    rng = np.random.default_rng(12)
    sweeps = _sample(rng, 0, 5, 4000) + _sample(rng, 1, 5, 3500)
    host = oracle.merge_sweeps(sweeps, n_copy=4)
    raw = np.concatenate([s["points"] for s in sweeps])
    segs, o = [], 0
    for s in sweeps:
        segs.append(dict(begin=o, end=o + len(s["points"]), batch=s["batch"], time=s["time"], radius=s["radius"], transform=s["transform"]))
        o += len(s["points"])
    out, n_out = SweepMerger()(torch.from_numpy(raw).cuda(), segs, n_copy=4)
    net = make_net(cfg["pc_range"], cfg["voxel_size"], synth.pfn_params())
    a = net.forward_dense(out[: int(n_out.item())].contiguous(), 2)
    b = net.forward_dense(torch.from_numpy(host).cuda(), 2)
    # a coordinate that differs in its last bit can move a point across a pillar edge: compare the occupied sets, allow a handful
    diff = int(((a != 0).any(1) != (b != 0).any(1)).sum())
    assert diff <= 4, diff
