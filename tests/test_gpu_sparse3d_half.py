"""GPU: SparseResNet3D inference on bf16 / fp16 rows and the 16-bit matrix cores (csrc/sparse3d_half.h, SparseResNet3D.use_half_precision).
  - every layer kind of test_gpu_sparse3d.LAYERS, both element types, with and without ReLU, against the fp64 rulebook of
    tests/sparse_conv3d_ref.py run on the operands ROUNDED to the element type (what the kernel saw):
        |y - ref| <= u |ref| + c sum|terms| + floor      u = 2^-8 (bf16), 2^-11 (fp16): the single output rounding
                                                         c = 1e-6: fp32 accumulation of products that are exact in fp32
                                                         floor = 1e-30 (bf16), 6e-8 (fp16, the spacing of its subnormals)
    and the pad columns of the output are exactly zero
  - row counts at the tile seams (1, 15, 16, 17, 33, 64, 65), a tap no row has, only the centre tap, map entries outside [0, n_in), no rows
  - a small whole backbone, one sample of two empty: the active sets of the fp32 path, and its distance to un-rounded fp64 within 1.5 E,
    E = the distance of the fp64 statement with weights, input and every layer's output rounded to the element type
  - nothing else changes: use_half_precision(None) is the never-switched module bit for bit, repeats are bit-identical, zero voxels and grid
    faces run, a call that wants gradients takes the fp32 autograd path
  - the configs/voxel18_aspp_nusc.yaml detector with backbone.use_half_precision() end to end."""
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import sparse3d_half_ref as HR  # noqa: E402
import sparse_conv3d_ref as R  # noqa: E402
import test_gpu_sparse3d as T3  # noqa: E402
from conftest import ROOT  # noqa: E402

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
C_ACC = 1e-6  # fp32 accumulation, the project's bar for pnx_sp3_conv; measured worst ratio of the 16-bit kernel: 1.86e-08 (test_layer_... below)


def _r(a, dtype):
    """fp32 numpy -> the values the element type holds, fp32 numpy (exact: every bf16 / fp16 value is an fp32 value)."""
    return HR.round_to(a.astype(np.float64), dtype).astype(np.float32)


def _rows(a, dtype, dev="cuda"):
    """numpy (N, C) values already representable in dtype -> padded device rows."""
    from pillarnext_amd import ops

    return ops.sp3_rows_h(torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev), dtype)


def _check_conv(y, cout, x, m, w, shift, resid, relu, dtype, what):
    """y (N_out, cpad) device rows against the fp64 rulebook on the (rounded) operands; returns the worst accumulation ratio."""
    yn = y.double().cpu().numpy()
    assert y.dtype == dtype and yn.shape == (m.shape[0], (cout + 7) // 8 * 8)
    assert not yn[:, cout:].any(), f"{what}: pad columns are not zero"
    acc, mag = R.gather_conv(x.astype(np.float64), m, w.astype(np.float64))
    ref = acc + shift.astype(np.float64)
    mag = mag + np.abs(shift.astype(np.float64))
    if resid is not None:
        ref, mag = ref + resid.astype(np.float64), mag + np.abs(resid.astype(np.float64))
    if relu:
        ref = np.maximum(ref, 0.0)
    err = np.abs(yn[:, :cout] - ref)
    # what is left of the error once the output rounding and the floor are taken off, in units of sum|terms|
    ratio = float(np.max(np.maximum(err - HR.U[dtype] * np.abs(ref) - HR.FLOOR[dtype], 0.0) / (mag + 1e-300))) if err.size else 0.0
    print(f"{what}: worst accumulation ratio {ratio:.3g} of sum|terms|, worst |err| {float(err.max()) if err.size else 0.0:.3g}")
    assert (err <= HR.U[dtype] * np.abs(ref) + C_ACC * mag + HR.FLOOR[dtype]).all(), f"{what}: worst ratio {ratio:.3g} of sum|terms|"
    return ratio


# ------------------------------------------------------------------------------------------------ single layers vs the numpy rulebook
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind,kernel,stride,pad,cin,cout,res", T3.LAYERS)
def test_layer_against_fp64_rulebook_on_rounded_operands(kind, kernel, stride, pad, cin, cout, res, dtype):
    """Measured on MI355X over all 24 cases x ReLU on / off: what is left of |err| after the output rounding is at worst 1.86e-08 of sum|terms|
    (subm 72 -> 72 with residual, fp16), so the bar stays at c = 1e-6."""
    from pillarnext_amd import ops

    rng = np.random.default_rng(cin * 1000 + cout + (7 if res else 0))
    B, grid = 2, (9, 10, 11)
    c, x = T3._case(rng, B, grid, 500, cin, positive=True)
    perm = rng.permutation(len(c))
    k, s, p = R.triple(kernel), R.triple(stride), R.triple(pad)
    w = _r((rng.standard_normal((cout, *k, cin)) / np.sqrt(cin * np.prod(k))).astype(np.float32), dtype)
    x = _r(x[perm], dtype)
    shift = rng.standard_normal(cout).astype(np.float32)  # the shift is an fp32 operand of the kernel
    dev = "cuda"
    tc = torch.from_numpy(c[perm]).int().to(dev).contiguous()
    ix, rows, cnt = ops.sp3_index_build(tc, B, grid, want_rows=True)
    if kind == "sparse":
        oix, ocnt = ops.sp3_out_index(tc, B, grid, k, s, p)
        oc = ops.sp3_index_coords(oix, int(ocnt.item()))
        ref_c, _ = R.output_set(c, grid, k, s, p)
    else:
        oc, ref_c = tc, c[perm]
    assert np.array_equal(oc.cpu().numpy(), ref_c), "output coords differ"
    m = ops.sp3_neighbor_map(oc, ix, rows, k, s, p)
    ref_m = R.neighbor_map(ref_c, c[perm], k, s, p)
    assert np.array_equal(m.cpu().numpy(), ref_m), "neighbour map differs"
    resid = _r(rng.standard_normal((len(ref_c), cout)).astype(np.float32), dtype) if res else None
    tx, tr = _rows(x, dtype), (_rows(resid, dtype) if res else None)
    wp = ops.sp3_pack_weight_h(torch.from_numpy(w).to(dev), dtype)
    tshift = torch.from_numpy(shift).to(dev)
    for relu in (False, True):
        y = ops.sp3_conv_h(tx, m, wp, tshift, cin, cout, residual=tr, relu=relu)
        _check_conv(y, cout, x, ref_m, w, shift, resid, relu, dtype, f"{kind} {cin}->{cout} relu={relu}")


# ------------------------------------------------------------------------------------------------ tile seams, skipped taps, bad map entries
def _plane(rng, n):
    """n sites of one z plane of a (5, 9, 9) grid: the 18 taps with od != 1 have no row."""
    yx = rng.choice(81, size=n, replace=False)
    return np.stack([np.zeros(n, np.int64), np.full(n, 2), yx // 9, yx % 9], 1), (5, 9, 9)


def _isolated(rng, n):
    """n sites on the even lattice of a (5, 9, 9) grid: no two are neighbours, only the centre tap exists."""
    idx = rng.choice(3 * 5 * 5, size=n, replace=False)
    return np.stack([np.zeros(n, np.int64), 2 * (idx // 25), 2 * (idx // 5 % 5), 2 * (idx % 5)], 1), (5, 9, 9)


def _random(rng, n):
    idx = rng.choice(4 * 5 * 6, size=n, replace=False)  # dense enough for every tap to occur once n is not tiny
    return np.stack([np.zeros(n, np.int64), idx // 30, idx // 6 % 5, idx % 6], 1), (4, 5, 6)


SEAMS = [("random", _random, n) for n in (1, 15, 16, 17, 33, 64, 65)] + [("plane", _plane, 33), ("isolated", _isolated, 17)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cin,cout", [(16, 16), (5, 18), (72, 72)])  # two taps per K step in LDS; four taps per step, 24 padded columns; streamed weights
@pytest.mark.parametrize("name,make,n", SEAMS, ids=[f"{a}{n}" for a, _, n in SEAMS])
def test_row_counts_at_the_tile_seams(name, make, n, cin, cout, dtype):
    from pillarnext_amd import ops

    rng = np.random.default_rng(n * 31 + cin)
    c, grid = make(rng, n)
    c, _ = R.sort_rows(c)
    m = R.neighbor_map(c, c, 3, 1, 1)
    if name == "plane":
        assert (m[:, :9] < 0).all() and (m[:, 18:] < 0).all() and (m[:, 9:18] >= 0).sum() > n
    if name == "isolated":
        assert (np.delete(m, 13, 1) < 0).all() and np.array_equal(m[:, 13], np.arange(n))
    x = _r(rng.standard_normal((n, cin)).astype(np.float32), dtype)
    w = _r((rng.standard_normal((cout, 3, 3, 3, cin)) / np.sqrt(cin * 27)).astype(np.float32), dtype)
    shift = rng.standard_normal(cout).astype(np.float32)
    resid = _r(rng.standard_normal((n, cout)).astype(np.float32), dtype)
    tc = torch.from_numpy(c).int().cuda().contiguous()
    ix, _, _ = ops.sp3_index_build(tc, 1, grid)
    tm = ops.sp3_neighbor_map(tc, ix, None, (3, 3, 3), (1, 1, 1), (1, 1, 1))
    assert np.array_equal(tm.cpu().numpy(), m)
    y = ops.sp3_conv_h(_rows(x, dtype), tm, ops.sp3_pack_weight_h(torch.from_numpy(w).cuda(), dtype), torch.from_numpy(shift).cuda(), cin, cout,
                       residual=_rows(resid, dtype), relu=False)
    _check_conv(y, cout, x, m, w, shift, resid, False, dtype, f"{name} n={n} {cin}->{cout}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_map_entries_outside_the_input_contribute_zero_and_no_rows_launch_nothing(dtype):
    from pillarnext_amd import ops

    rng = np.random.default_rng(11)
    n_in, n_out, cin, cout, T = 40, 37, 18, 36, 27
    m = rng.integers(-1, n_in, size=(n_out, T)).astype(np.int32)
    bad = m.copy()
    bad[rng.random(m.shape) < 0.2] = -7          # any negative entry is "no neighbour"
    bad[rng.random(m.shape) < 0.2] = n_in + 5    # and so is one past the input rows (the kernel never forms an address from it)
    bad[0, :] = n_in                             # a row without any neighbour
    ref_m = np.where((bad < 0) | (bad >= n_in), -1, bad)
    x = _r(rng.standard_normal((n_in, cin)).astype(np.float32), dtype)
    w = _r((rng.standard_normal((cout, 3, 3, 3, cin)) / np.sqrt(cin * T)).astype(np.float32), dtype)
    shift = rng.standard_normal(cout).astype(np.float32)
    wp, ts = ops.sp3_pack_weight_h(torch.from_numpy(w).cuda(), dtype), torch.from_numpy(shift).cuda()
    y = ops.sp3_conv_h(_rows(x, dtype), torch.from_numpy(bad).cuda(), wp, ts, cin, cout, relu=False)
    _check_conv(y, cout, x, ref_m, w, shift, None, False, dtype, "bad map entries")
    assert np.array_equal(y[0, :cout].double().cpu().numpy(), HR.round_to(shift.astype(np.float64), dtype))
    # no input rows: every output is the shift; no output rows: an empty result, nothing launched
    y0 = ops.sp3_conv_h(_rows(x[:0], dtype), torch.from_numpy(m).cuda(), wp, ts, cin, cout, relu=False)
    assert torch.equal(y0, y[:1].expand(n_out, -1))
    e = ops.sp3_conv_h(_rows(x, dtype), torch.zeros((0, T), dtype=torch.int32, device="cuda"), wp, ts, cin, cout)
    assert tuple(e.shape) == (0, 40) and e.dtype == dtype
    d = ops.sp3_dense_h(e, torch.zeros((0, 4), dtype=torch.int32, device="cuda"), 2, (2, 3, 3), cout)
    assert tuple(d.shape) == (2, cout * 2, 3, 3) and d.dtype == torch.float32 and not bool(d.any())


# ------------------------------------------------------------------------------------------------ a small whole backbone
def _fold_rounded(conv, bn, dtype):
    """The layer as the 16-bit path states it: BN scale folded into the weight in fp32, the product rounded once; the shift stays fp32."""
    a = bn.weight.detach().float() * torch.rsqrt(bn.running_var.detach().float() + bn.eps)
    w = HR.round_to(conv.weight.detach().float() * a.view(-1, 1, 1, 1, 1), dtype)
    shift = (bn.bias.detach().float() - bn.running_mean.detach().float() * a).double()
    return types.SimpleNamespace(weight=w, kernel_size=conv.kernel_size, stride=conv.stride, padding=conv.padding), shift


def ref_backbone_rounded(bb, feats, coords, grid, B, dtype):
    """test_gpu_sparse3d.ref_backbone in fp64 with the weights, the input and every layer's output rounded to `dtype`."""
    rd = lambda t: HR.round_to(t, dtype)  # noqa: E731

    def layer(coords, x, grid, conv, bn, subm, residual=None):
        cv, shift = _fold_rounded(conv, bn, dtype)
        oc, y, og = T3._ref_layer(coords, x, grid, cv, subm)
        y = y + shift
        return oc, rd(torch.relu(y if residual is None else y + residual)), og

    x = rd(feats.double())
    with torch.no_grad():
        for seq in bb.blocks:
            coords, x, grid = layer(coords, x, grid, seq[0].conv, seq[0].norm, False)
            for blk in seq[1:]:
                y = layer(coords, x, grid, blk.block1.conv, blk.block1.norm, True)[1]
                x = layer(coords, y, grid, blk.conv2, blk.norm2, True, residual=x)[1]
        coords, x, grid = layer(coords, x, grid, bb.extra_conv[0], bb.extra_conv[1], False)
        x = layer(coords, x, grid, bb.mapping.conv, bb.mapping.norm, True)[1]
        D, H, W = grid
        dense = torch.zeros((B, x.shape[1], D, H, W), dtype=torch.float64, device=x.device)
        c = coords.long()
        dense[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]] = x
    return dense.view(B, -1, H, W)


def _small_cloud(seed, grid, n, batch_index=0):
    rng = np.random.default_rng(seed)
    D, H, W = grid
    idx = np.sort(rng.choice(D * H * W, n, replace=False))
    c = np.stack([np.full(n, batch_index), idx // (H * W), idx // W % H, idx % W], 1)
    coords = torch.from_numpy(c).int().cuda().contiguous()
    return torch.randn((n, 5), device="cuda", generator=torch.Generator("cuda").manual_seed(seed)), coords


_SMALL = {}


def _small_backbone(ch):
    """Backbone, cloud and the three references of the whole-backbone tests, computed once per width."""
    key = tuple(ch)
    if key not in _SMALL:
        grid = (17, 24, 24)  # -> (17, 24, 24), (9, 12, 12), (5, 6, 6), (3, 3, 3), extra_conv (1, 3, 3)
        bb = T3.make_backbone(ch, seed=1)
        feats, coords = _small_cloud(2, grid, 400)  # sample 0 of 2; sample 1 is empty
        with torch.no_grad():
            sets32 = bb.forward_sparse(feats, coords, grid, 2)
            out32 = bb(feats, coords, grid, 2)
        _, ref = T3.ref_backbone(bb, feats, coords, grid, 2)
        _SMALL[key] = (bb, feats, coords, grid, sets32, out32, ref)
    return _SMALL[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ch", [[16, 32, 64, 128], [18, 36, 72, 144]], ids=["w16", "w18"])
def test_small_backbone_within_the_rounded_fp64_statement(ch, dtype):
    """Measured on MI355X (E = rounded fp64 statement vs fp64, d = 16-bit path vs fp64; bar d <= 1.5 E):
      16/32/64/128  bf16: E 0.002211, d 0.00228  (1.031 E)    fp16: E 0.0002784, d 0.0002837 (1.019 E)
      18/36/72/144  bf16: E 0.00216,  d 0.002102 (0.973 E)    fp16: E 0.0002771, d 0.000276  (0.996 E)"""
    bb, feats, coords, grid, sets32, out32, ref = _small_backbone(ch)
    bb.use_half_precision(dtype)
    try:
        with torch.no_grad():
            sets = bb.forward_sparse(feats, coords, grid, 2)
            out = bb(feats, coords, grid, 2)
    finally:
        bb.use_half_precision(None)
    assert len(sets) == len(sets32) == 6
    true_ch = [*ch, ch[-1], 128]
    for i, ((c, x, g), (c32, x32, g32)) in enumerate(zip(sets, sets32)):
        assert torch.equal(c, c32) and g == g32, f"active set {i} differs"
        assert x.dtype == dtype and tuple(x.shape) == tuple(x32.shape) == (c.shape[0], true_ch[i])
    assert out.dtype == torch.float32 and out.shape == out32.shape == ref.shape == (2, 128, 3, 3)
    assert bool(out[0].any()) and not bool(out[1].any())  # the empty sample stays empty
    E = T3._rel(ref_backbone_rounded(bb, feats, coords, grid, 2, dtype), ref)
    d = T3._rel(out, ref)
    print(f"[{'x'.join(map(str, ch))} {str(dtype)[6:]}] sites per stage {[int(s[0].shape[0]) for s in sets]}: E {E:.4g}, 16-bit path {d:.4g}, "
          f"ratio {d / E:.3f}, fp32 path {T3._rel(out32, ref):.3g}")
    assert torch.isfinite(out).all() and E > 0
    assert d <= 1.5 * E, f"16-bit path {d:.4g} from fp64, the rounded fp64 statement {E:.4g}"


# ------------------------------------------------------------------------------------------------ nothing else changes
def test_switching_back_repeats_faces_zero_voxels_and_gradients():
    ch = [16, 32, 64, 128]
    never = T3.make_backbone(ch, seed=3)
    bb = T3.make_backbone(ch, seed=3)
    grid = (40, 20, 24)
    D, H, W = grid
    rng = np.random.default_rng(5)
    faces = [(z, y, x) for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)] + [(0, 7, 9), (D - 1, 3, 4), (5, 0, 11), (6, H - 1, 2), (4, 8, 0),
                                                                                      (7, 13, W - 1)]
    inner = [tuple(v) for v in np.stack(np.unravel_index(rng.choice(D * H * W, 150, replace=False), grid), 1)]
    rows = sorted({(b, *v) for b in (0, 2) for v in faces + inner})  # sample 1 of 3 is empty
    coords = torch.tensor(rows, dtype=torch.int32, device="cuda")
    feats = torch.randn((len(rows), 5), device="cuda")
    with torch.no_grad():
        want = never(feats, coords, grid, batch_size=3)
        for dtype in DTYPES:
            bb.use_half_precision(dtype)
            out = bb(feats, coords, grid, batch_size=3)
            again = bb(feats, coords, grid, batch_size=3)
            assert out.dtype == torch.float32 and out.shape == (3, 256, 3, 3)
            assert torch.equal(out, again), "two 16-bit runs differ"
            assert not torch.equal(out, want)  # it did run in 16 bits (how close it must be: the test above)
            assert not bool(out[1].any()) and bool(out[0].any()) and bool(out[2].any())
            empty = bb(feats[:0], coords[:0], grid, batch_size=2)
            assert empty.shape == (2, 256, 3, 3) and empty.dtype == torch.float32 and not bool(empty.any())
            assert bb(feats[:0], coords[:0], grid).shape == (0, 256, 3, 3)
            assert all(x.dtype == dtype and x.shape[0] == 0 for _, x, _ in bb.forward_sparse(feats[:0], coords[:0], grid, 2))
        bb.use_half_precision(None)
        assert torch.equal(bb(feats, coords, grid, batch_size=3), want), "use_half_precision(None) is not the fp32 path"
    # gradients enabled and parameters that require one: the fp32 autograd path, whatever use_half_precision says
    bb.use_half_precision()
    sets = bb.forward_sparse(feats, coords, grid, 3)
    assert all(x.dtype == torch.float32 for _, x, _ in sets) and sets[-1][1].requires_grad
    out = bb(feats, coords, grid, batch_size=3)
    ref_out = never(feats, coords, grid, batch_size=3)
    assert out.requires_grad and torch.equal(out, ref_out)
    out.sum().backward()
    assert bb.mapping.conv.weight.grad is not None and bool(bb.mapping.conv.weight.grad.any())


# ------------------------------------------------------------------------------------------------ detector end to end
def test_voxel18_nusc_detector_in_bf16_end_to_end():
    from pillarnext_amd import config, synth

    cfg = config.load(os.path.join(ROOT, "configs", "voxel18_aspp_nusc.yaml"))["model"]
    cfg["post_processing"]["score_threshold"] = 0.0
    torch.manual_seed(0)
    det = config.instantiate(cfg).cuda().eval()
    assert det.backbone.use_half_precision() is det.backbone and det.backbone.half_dtype == torch.bfloat16
    pts = torch.from_numpy(synth.make_batch("C2ref", 2, "sweep", n=60_000)).cuda()
    ex = {"points": pts, "token": ["a", "b"], "batch_size": 2}
    det.backbone.profile = []
    out = det(ex)
    assert "input.rows" in [name for name, _ in det.backbone.profile], "the detector's forward did not take the 16-bit path"
    det.backbone.profile = None
    assert set(out) == {"a", "b"} and out["a"]["box3d_lidar"].shape[0] > 0 and out["b"]["box3d_lidar"].shape[0] > 0
    for t in out:
        for k, v in out[t].items():
            if torch.is_tensor(v) and v.dtype.is_floating_point:
                assert bool(torch.isfinite(v).all()), (t, k)
    with torch.no_grad():
        feats, coords, grid = det.reader(pts, 2)
        x = det.backbone(feats, coords, grid)
        assert x.shape == (2, 256, 168, 168) and x.dtype == torch.float32 and bool(torch.isfinite(x).all())
        x32 = det.backbone.use_half_precision(None)(feats, coords, grid)
        assert x32.shape == x.shape and not torch.equal(x, x32)
