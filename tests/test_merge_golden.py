"""The multi-sweep merge pinned to the REFERENCE: tests/golden/merge_sweeps.npz holds raw sweep files and the output of the reference's own
NuScenesDataset.load_pointcloud (nusc.py:76-121: fp64 4x4 transform stored back as fp32, remove_close on past sweeps, time-lag column) and
WaymoDataset.load_pointcloud (waymo.py:49-67: nlz filter, inv(pose) @ sweep_pose, timestamp column), made by oracle/gen_golden.py merge.
CPU: the numpy restatement oracle.merge_sweeps; GPU: the device merge (csrc/merge.hip behind io.SweepMerger), also bit for bit against its exact twin
(tests/merge_ref.py, which tests/test_merge_ref_cpu.py holds to this same golden file)."""
import merge_ref
import numpy as np
import pytest

from conftest import load_golden


def _nusc_sweeps(g, batch=0):
    sw = []
    for k in range(4):
        sw.append(dict(points=g[f"nusc_raw{k}"], batch=batch, time=float(g["nusc_time_lag"][k]), radius=1.0 if k > 0 else 0.0,
                       transform=g[f"nusc_T{k}"] if k > 0 else None))
    return sw


def _waymo_sweeps(g, batch=0):
    sw = []
    p0 = g["waymo_pose0"]
    for k in range(3):
        raw = g[f"waymo_raw{k}"]
        raw = raw[raw[:, -1] == -1, :4]                                       # read_file: no-label-zone rows out, elongation dropped (waymo.py:44)
        rel = np.linalg.inv(p0) @ g[f"waymo_pose{k}"] if k > 0 else None     # waymo.py:60-61
        sw.append(dict(points=raw, batch=batch, time=float(g["waymo_timestamp"][k]), radius=0.0, transform=rel))
    return sw


@pytest.mark.parametrize("ds", ["nusc", "waymo"])
def test_oracle_merge_equals_the_reference(oracle, ds):
    g = load_golden("merge_sweeps")
    ref = g[f"{ds}_points"]
    got = oracle.merge_sweeps(_nusc_sweeps(g) if ds == "nusc" else _waymo_sweeps(g), n_copy=4)
    assert got.shape == (len(ref), 6) and ref.dtype == np.float32
    assert np.array_equal(got[:, 4:], ref[:, 3:])                            # intensity and time columns, same rows in the same order
    if ds == "nusc":
        assert np.array_equal(got[:, 1:4], ref[:, :3])                        # T.dot(vstack(xyz, 1)): the same expression, bit for bit
    else:                                                                     # (xyz1 @ rel_pose.T): the other summation order of the fp64 dot
        np.testing.assert_allclose(got[:, 1:4], ref[:, :3], rtol=0, atol=8e-6)
        assert float(np.mean(got[:, 1:4] == ref[:, :3])) > 0.999


@pytest.mark.gpu
@pytest.mark.parametrize("ds", ["nusc", "waymo"])
def test_device_merge_equals_the_reference(ds):
    torch = pytest.importorskip("torch")
    from pillarnext_amd.io import SweepMerger

    g = load_golden("merge_sweeps")
    ref = g[f"{ds}_points"]
    sweeps = _nusc_sweeps(g, batch=1) if ds == "nusc" else _waymo_sweeps(g, batch=1)
    ncol = max(s["points"].shape[1] for s in sweeps)
    raw = np.concatenate([np.pad(s["points"], ((0, 0), (0, ncol - s["points"].shape[1]))) for s in sweeps]).astype(np.float32)
    segs, o = [], 0
    for s in sweeps:
        segs.append(dict(begin=o, end=o + len(s["points"]), batch=s["batch"], time=s["time"], radius=s["radius"], transform=s["transform"]))
        o += len(s["points"])
    out, n_out = SweepMerger()(torch.from_numpy(raw).cuda(), segs, n_copy=4)
    n = int(n_out.item())
    got = out[:n].cpu().numpy()
    twin, n_twin = merge_ref.merge(raw, segs, 4)                              # the exact twin of the kernel: the whole buffer, bit for bit
    assert n == n_twin
    merge_ref.assert_same_bits(out.cpu().numpy(), twin, ds)
    assert n == len(ref) and bool((got[:, 0] == 1).all())
    assert np.array_equal(got[:, 4:], ref[:, 3:])
    np.testing.assert_allclose(got[:, 1:4], ref[:, :3], rtol=0, atol=8e-6)    # <= 1 ulp of fp32 at |x| <= 75 m
    assert float(np.mean(got[:, 1:4] == ref[:, :3])) > 0.999
    assert bool((out[n:, 0] == -1).all())
