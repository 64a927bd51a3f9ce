"""GPU: the sparse 3-D kernels of csrc/sparse3d.hip and SparseResNet3D.
  - every layer kind (SparseConv3d s1 / s2 / (3,1,1)-(2,1,1) p0, SubM k3, SubM k1, with and without residual) against the fp64 numpy
    rulebook of tests/sparse_conv3d_ref.py on the operands the kernel saw: output coords exact, |err| <= 1e-6 * sum|terms| + 1e-30
  - full size: a C2 sweep cloud (2 frames, nuScenes voxel18 geometry) through VoxelFeatureNet + SparseResNet3D against a torch statement
    on the GPU whose neighbours come from torch.unique / searchsorted over int64 keys: identical active sets at every stage, the output
    within 1e-5 relative Frobenius of fp64; the Waymo geometry once
  - edge cases: an empty sample in the middle, zero voxels, sites on every grid face, bit-identical repeats
  - the detector of configs/voxel18_aspp_nusc.yaml end to end in eval."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import sparse_conv3d_ref as R  # noqa: E402
from conftest import ROOT  # noqa: E402

NUSC = dict(voxel_size=[0.075, 0.075, 0.2], pc_range=[-50.4, -50.4, -5.0, 50.4, 50.4, 3.0])
WAYMO = dict(voxel_size=[0.075, 0.075, 0.15], pc_range=[-76.8, -76.8, -2.0, 76.8, 76.8, 4.0])
VOXEL18 = dict(layer_nums=[2, 2, 2, 2], ds_layer_strides=[1, 2, 2, 2], num_input_features=5)


# ------------------------------------------------------------------------------------------------ single layers vs the numpy rulebook
def _case(rng, B, grid, n, cin, positive=False):
    D, H, W = grid
    keys = rng.choice(B * D * H * W, size=n, replace=False)
    c, _ = R.sort_rows(np.stack(np.unravel_index(keys, (B, D, H, W)), 1))
    x = rng.standard_normal((n, cin)).astype(np.float32)
    return c, (np.abs(x) if positive else x)


LAYERS = [  # (kind, kernel, stride, pad, cin, cout, residual)
    ("sparse", 3, 1, 1, 5, 18, False),
    ("sparse", 3, 2, 1, 18, 36, False),
    ("sparse", 3, 2, 1, 36, 72, False),
    ("sparse", (3, 1, 1), (2, 1, 1), 0, 144, 144, False),
    ("sparse", (3, 1, 1), (2, 1, 1), 0, 16, 16, False),
    ("subm", 3, 1, 1, 18, 18, False),
    ("subm", 3, 1, 1, 18, 18, True),
    ("subm", 3, 1, 1, 144, 144, True),
    ("subm", 3, 1, 1, 16, 32, False),
    ("subm", 3, 1, 1, 72, 72, True),
    ("subm", 1, 1, 0, 144, 128, False),
    ("subm", 1, 1, 0, 36, 72, True),
]


@pytest.mark.parametrize("kind,kernel,stride,pad,cin,cout,res", LAYERS)
def test_layer_against_fp64_rulebook(kind, kernel, stride, pad, cin, cout, res):
    from pillarnext_amd import ops

    rng = np.random.default_rng(cin * 1000 + cout + (7 if res else 0))
    B, grid = 2, (9, 10, 11)
    c, x = _case(rng, B, grid, 500, cin, positive=True)
    perm = rng.permutation(len(c))  # rows in any order: the index's row_of_rank undoes it
    k, s, p = R.triple(kernel), R.triple(stride), R.triple(pad)
    w = (rng.standard_normal((cout, *k, cin)) / np.sqrt(cin * np.prod(k))).astype(np.float32)
    shift = rng.standard_normal(cout).astype(np.float32)
    dev = "cuda"
    tc = torch.from_numpy(c[perm]).int().to(dev).contiguous()
    tx = torch.from_numpy(x[perm]).to(dev).contiguous()
    ix, rows, cnt = ops.sp3_index_build(tc, B, grid, want_rows=True)
    assert int(cnt.item()) == len(c)
    if kind == "sparse":
        oix, ocnt = ops.sp3_out_index(tc, B, grid, k, s, p)
        oc = ops.sp3_index_coords(oix, int(ocnt.item()))
        ref_c, og = R.output_set(c, grid, k, s, p)
        assert oix.grid == og
    else:
        oc, ref_c = tc, c[perm]
    assert np.array_equal(oc.cpu().numpy(), ref_c), "output coords differ"
    m = ops.sp3_neighbor_map(oc, ix, rows, k, s, p)
    ref_m = R.neighbor_map(ref_c, c[perm], k, s, p)
    assert np.array_equal(m.cpu().numpy(), ref_m), "neighbour map differs"
    resid = torch.from_numpy(rng.standard_normal((len(ref_c), cout)).astype(np.float32)).to(dev) if res else None
    y = ops.sp3_conv(tx, m, ops.sp3_pack_weight(torch.from_numpy(w).to(dev)), torch.from_numpy(shift).to(dev), cout, residual=resid, relu=False)
    acc, mag = R.gather_conv(x[perm].astype(np.float64), ref_m, w.astype(np.float64))
    ref = acc + shift.astype(np.float64)
    mag = mag + np.abs(shift.astype(np.float64))
    if res:
        r64 = resid.cpu().numpy().astype(np.float64)
        ref, mag = ref + r64, mag + np.abs(r64)
    err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
    assert (err <= 1e-6 * mag + 1e-30).all(), f"worst {np.max(err / (mag + 1e-30)):.3g} of sum|terms|"
    yr = ops.sp3_conv(tx, m, ops.sp3_pack_weight(torch.from_numpy(w).to(dev)), torch.from_numpy(shift).to(dev), cout, residual=resid, relu=True)
    assert torch.equal(yr, torch.clamp(y, min=0))


# ------------------------------------------------------------------------------------------------ torch statement of the backbone
def _keys(c, grid):
    D, H, W = grid
    c = c.long()
    return ((c[:, 0] * D + c[:, 1]) * H + c[:, 2]) * W + c[:, 3]


def _coords(keys, grid):
    D, H, W = grid
    return torch.stack([keys // (D * H * W), keys // (H * W) % D, keys // W % H, keys % W], 1).int()


def _ref_layer(coords, x, grid, conv, subm):
    """One conv in fp64: output set from torch.unique over candidate keys, neighbours from searchsorted over the sorted input keys."""
    k, s, p = conv.kernel_size, conv.stride, conv.padding
    og = R.out_grid(grid, k, s, p)
    c = coords.long()
    taps = [(a, b, d) for a in range(k[0]) for b in range(k[1]) for d in range(k[2])]
    if subm:
        oc = coords
    else:
        cand = []
        for o in taps:
            t = c[:, 1:] + torch.tensor(p, device=c.device) - torch.tensor(o, device=c.device)
            sv = torch.tensor(s, device=c.device)
            ok = (t >= 0).all(1) & (t % sv == 0).all(1) & (t // sv < torch.tensor(og, device=c.device)).all(1)
            cand.append(_keys(torch.cat([c[ok, :1], t[ok] // sv], 1), og))
        oc = _coords(torch.unique(torch.cat(cand)), og)
    kin = _keys(coords, grid)
    skey, order = torch.sort(kin)
    w = conv.weight.detach().double()
    out = torch.zeros((oc.shape[0], w.shape[0]), dtype=torch.float64, device=x.device)
    q = oc.long()
    for ti, o in enumerate(taps):
        pin = q[:, 1:] * torch.tensor(s, device=q.device) - torch.tensor(p, device=q.device) + torch.tensor(o, device=q.device)
        inside = (pin >= 0).all(1) & (pin < torch.tensor(grid, device=q.device)).all(1)
        key = _keys(torch.cat([q[:, :1], pin.clamp(min=0)], 1), grid)
        pos = torch.searchsorted(skey, key).clamp(max=max(len(skey) - 1, 0))
        hit = inside & (skey[pos] == key) if len(skey) else inside & False
        sel = hit.nonzero()[:, 0]
        out.index_add_(0, sel, x[order[pos[sel]]] @ w[:, o[0], o[1], o[2], :].T)
    return oc, out, og


def _bn(x, bn):
    return (x - bn.running_mean.double()) / torch.sqrt(bn.running_var.double() + bn.eps) * bn.weight.double() + bn.bias.double()


def ref_backbone(bb, feats, coords, grid, B):
    """fp64 torch statement of SparseResNet3D.forward: (sets [(coords, x)] per stage / extra / mapping, dense output)."""
    x = feats.double()
    sets = []
    with torch.no_grad():
        for seq in bb.blocks:
            coords, x, grid = _ref_layer(coords, x, grid, seq[0].conv, False)
            x = torch.relu(_bn(x, seq[0].norm))
            for blk in seq[1:]:
                y = torch.relu(_bn(_ref_layer(coords, x, grid, blk.block1.conv, True)[1], blk.block1.norm))
                x = torch.relu(_bn(_ref_layer(coords, y, grid, blk.conv2, True)[1], blk.norm2) + x)
            sets.append((coords, x))
        coords, x, grid = _ref_layer(coords, x, grid, bb.extra_conv[0], False)
        x = torch.relu(_bn(x, bb.extra_conv[1]))
        sets.append((coords, x))
        x = torch.relu(_bn(_ref_layer(coords, x, grid, bb.mapping.conv, True)[1], bb.mapping.norm))
        sets.append((coords, x))
        D, H, W = grid
        dense = torch.zeros((B, x.shape[1], D, H, W), dtype=torch.float64, device=x.device)
        c = coords.long()
        dense[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]] = x
    return sets, dense.view(B, -1, H, W)


def make_backbone(ch, seed=0):
    from pillarnext_amd.sparse3d import SparseResNet3D

    torch.manual_seed(seed)
    bb = SparseResNet3D(ds_num_filters=ch, **VOXEL18)
    with torch.no_grad():
        for m in bb.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.uniform_(0.5, 1.5), m.bias.uniform_(-0.2, 0.2), m.running_mean.uniform_(-0.2, 0.2), m.running_var.uniform_(0.5, 2.0)
    return bb.cuda().eval()


def _rel(a, b):
    return float(torch.linalg.norm((a.double() - b).flatten()) / torch.linalg.norm(b.flatten()).clamp(min=1e-300))


def _voxels(config, geom, frames):
    from pillarnext_amd import synth
    from pillarnext_amd.voxel_encoder import VoxelFeatureNet

    pts = torch.from_numpy(synth.make_batch(config, frames, "sweep")).cuda()
    return VoxelFeatureNet(**geom).cuda()(pts, frames)


@pytest.mark.parametrize("name,config,geom,ch,frames", [("nusc", "C2", NUSC, [18, 36, 72, 144], 2), ("waymo", "C5ref", WAYMO, [16, 32, 64, 128], 1)])
def test_full_size_backbone_against_torch_statement(name, config, geom, ch, frames):
    feats, coords, grid = _voxels(config, geom, frames)
    assert tuple(int(g) for g in grid)[0] == 40 and feats.shape[1] == 5
    bb = make_backbone(ch)
    with torch.no_grad():
        sets = bb.forward_sparse(feats, coords, grid, frames)
        out = bb(feats, coords, grid, frames)
    ref_sets, ref = ref_backbone(bb, feats, coords, tuple(int(g) for g in grid), frames)
    assert len(sets) == len(ref_sets) == 6
    for i, ((c, x, _), (rc, rx)) in enumerate(zip(sets, ref_sets)):
        assert torch.equal(c, rc), f"active set {i} differs ({c.shape[0]} vs {rc.shape[0]} sites)"
        assert _rel(x, rx) <= 1e-5, f"set {i}: {_rel(x, rx):.3g}"
    print(f"[{name}] sites per stage:", [int(s[0].shape[0]) for s in sets], "out", tuple(out.shape), f"rel {_rel(out, ref):.3g}")
    assert out.shape == ref.shape == (frames, 256, *[int(g) // 8 for g in grid[1:]])
    assert _rel(out, ref) <= 1e-5


# ------------------------------------------------------------------------------------------------ edge cases
def test_empty_sample_zero_voxels_grid_faces_and_repeats():
    bb = make_backbone([16, 32, 64, 128], seed=3)
    grid = (40, 20, 24)  # -> (20, 10, 12), (10, 5, 6), (5, 3, 3), extra_conv (2, 3, 3)
    D, H, W = grid
    rng = np.random.default_rng(5)
    faces = [(z, y, x) for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)] + [(0, 7, 9), (D - 1, 3, 4), (5, 0, 11), (6, H - 1, 2), (4, 8, 0),
                                                                                      (7, 13, W - 1)]
    inner = [tuple(v) for v in np.stack(np.unravel_index(rng.choice(D * H * W, 150, replace=False), grid), 1)]
    rows = sorted({(b, *v) for b in (0, 2) for v in faces + inner})  # sample 1 of 3 is empty
    coords = torch.tensor(rows, dtype=torch.int32, device="cuda")
    feats = torch.randn((len(rows), 5), device="cuda")
    with torch.no_grad():
        out = bb(feats, coords, grid, batch_size=3)
        again = bb(feats, coords, grid, batch_size=3)
        _, ref = ref_backbone(bb, feats, coords, grid, 3)
        assert out.shape == (3, 256, 3, 3)
        assert torch.equal(out, again)
        assert _rel(out, ref) <= 1e-5
        assert not bool(out[1].any()) and bool(out[0].any()) and bool(out[2].any())
        empty = bb(feats[:0], coords[:0], grid, batch_size=2)
        assert empty.shape == (2, 256, 3, 3) and not bool(empty.any())
        assert bb(feats[:0], coords[:0], grid).shape == (0, 256, 3, 3)  # the reference's batch rule: no voxels, no samples
        from pillarnext_amd._lib import PnxError

        with pytest.raises(PnxError, match="outside"):
            bb(feats, coords, grid, batch_size=2)
        with pytest.raises(PnxError, match="outside"):
            bb(feats, coords, (D, H, W - 1), batch_size=3)


# ------------------------------------------------------------------------------------------------ detector end to end
def test_voxel18_nusc_detector_end_to_end():
    from pillarnext_amd import config, synth

    cfg = config.load(os.path.join(ROOT, "configs", "voxel18_aspp_nusc.yaml"))["model"]
    cfg["post_processing"]["score_threshold"] = 0.0
    torch.manual_seed(0)
    det = config.instantiate(cfg).cuda().eval()
    pts = torch.from_numpy(synth.make_batch("C2ref", 2, "sweep", n=60_000)).cuda()
    ex = {"points": pts, "token": ["a", "b"], "batch_size": 2}
    out = det(ex)
    out2 = det(ex)
    assert set(out) == {"a", "b"} and out["a"]["box3d_lidar"].shape[0] > 0
    for t in out:
        for k, v in out[t].items():
            assert torch.equal(v, out2[t][k]) if torch.is_tensor(v) else v == out2[t][k], (t, k)
    with torch.no_grad():
        feats, coords, grid = det.reader(pts, 2)
        x = det.backbone(feats, coords, grid)
        _, ref = ref_backbone(det.backbone, feats, coords, tuple(int(g) for g in grid), 2)
        assert x.shape == (2, 256, 168, 168)
        preds = det.head(det.neck(x))
        ref_preds = det.head(det.neck(ref.float()))
    for p, q in zip(preds, ref_preds):
        for k in p:
            assert _rel(p[k], q[k].double()) <= 1e-4, k
