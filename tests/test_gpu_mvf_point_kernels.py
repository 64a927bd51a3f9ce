"""GPU: the three point kernels of the multi-view reader's eval path -- pnx_pfn_layer_eval and the forward of pnx_bilinear_gather (csrc/group.hip),
pnx_scatter_max and pnx_scatter_max_backward (csrc/scatter.hip) -- against the twins of tests/mvf_point_ref.py at the seams of the kernels: the second
input register of k_pfn_layer (cin 65 .. 128), cin = 64, the xa / gb[inv] seam inside a register, the 64 KiB weight, empty and 5 000-point cells, the
wave-stride loops, the lane loops past 64 channels in all three map types, image indices -1 and B, ties and -inf in the per-pillar maximum, a scan-block
seam without rows.  The bounds are derived in that module's docstring; tests/test_mvf_point_ref_cpu.py shows that the references alone meet them on
these very inputs."""
import mvf_bilinear_ref as R
import mvf_point_ref as P
import numpy as np
import pytest
import torch
from test_gpu_mvf_train import CELLS4, _edge_points

pytestmark = pytest.mark.gpu


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ pnx_pfn_layer_eval
def _raw_pfn(xa, gb, inv, wt, shift, G, y, gmax):
    """The C entry point with the caller's output tensors (ops.pfn_layer_eval allocates its own)."""
    from pillarnext_amd._lib import check, lib, ptr, stream_ptr

    n, ca = xa.shape
    cb, cout = 0 if gb is None else gb.shape[1], wt.shape[1]
    check(lib().pnx_pfn_layer_eval(ptr(xa), xa.stride(0) if n > 1 else max(ca, 1), ca, ptr(gb), cb, ptr(inv), ptr(wt), ptr(shift), cout, n, G, ptr(y), cout,
                                   ptr(gmax), stream_ptr()), "pnx_pfn_layer_eval")


def _pfn_layer(what, xa, gb, inv, wt, shift, G, store):
    """One layer against its twin; returns (y or None, gmax, worst |err| / bound)."""
    from pillarnext_amd import ops

    n, cout, cin = xa.shape[0], wt.shape[1], wt.shape[0]
    inv_h = inv.cpu().numpy()
    S, A = P.pfn_layer(xa.cpu().numpy(), None if gb is None else gb.cpu().numpy(), inv_h, wt.cpu().numpy(), shift.cpu().numpy(), G)
    # the caller's buffers hold 0xFF bytes: every element of y and every cell of gmax, the empty ones included, is written
    y = torch.empty((n, cout), device="cuda") if store else None
    gmax = torch.empty((G, cout), device="cuda")
    for t in (y, gmax):
        if t is not None:
            t.view(torch.uint8).fill_(0xFF)
    _raw_pfn(xa, gb, inv, wt, shift, G, y, gmax)
    ratio = P.pfn_check(None if y is None else y.cpu().numpy(), gmax.cpu().numpy(), S, A, inv_h, G, cin, what)
    # without the maximum (and, where no gb needs it, without inv): the same y
    y_only, none = ops.pfn_layer_eval(xa, gb, None if gb is None else inv, wt, shift, G, store=True, want_max=False)
    assert none is None and y_only.shape == (n, cout)
    if store:
        assert torch.equal(_bits(y_only), _bits(y)), what
    else:
        P.pfn_check(y_only.cpu().numpy(), None, S, A, inv_h, G, cin, what + ", y alone")
    # the maximum is the maximum of the kernel's own outputs, bit for bit
    assert np.array_equal(gmax.cpu().numpy().view(np.uint32), P.cell_max_of(y_only.cpu().numpy(), inv_h, G).view(np.uint32)), what
    # repeated calls give the same bits
    for _ in range(2):
        y2, g2 = ops.pfn_layer_eval(xa, gb, inv, wt, shift, G, store=store, want_max=True)
        assert torch.equal(_bits(g2), _bits(gmax)) and (y2 is None) == (not store) and (y2 is None or torch.equal(_bits(y2), _bits(y))), what
    return y, gmax, ratio


@pytest.mark.parametrize("name,n", P.pfn_cases())
def test_pfn_layer_eval_against_fp64(name, n):
    d = P.pfn_case(name, n)
    ca = d["xa"].shape[1]
    wide = torch.from_numpy(d["wide"]).cuda()
    xa = wide[:, P.PFN_XA_OFFSET:P.PFN_XA_OFFSET + ca]                      # a column slice of a wider buffer at an odd offset
    assert xa.shape == (n, ca) and (n < 2 or (xa.stride(0) == ca + P.PFN_XA_PAD and xa.storage_offset() == P.PFN_XA_OFFSET))
    gb, inv, wt, shift = _dev(d["gb"]), _dev(d["inv"]), _dev(d["wt"]), _dev(d["shift"])
    y0, gm0, _ = _pfn_layer(f"pfn {name} n={n}", xa, gb, inv, wt, shift, d["G"], store=True)
    if len(d["zero_rows"]):                                                    # a pre-activation of -0.0 is stored as +0
        assert not bool(y0[_dev(d["zero_rows"]), 0].view(torch.int32).any())
    if name == "config":                                                       # the second layer reads the kernel's own [y | max[inv]] in place
        wt1, shift1 = (_dev(a) for a in P.pfn_layer1_params())
        _pfn_layer(f"pfn {name} n={n}, layer 1", y0, gm0, inv, wt1, shift1, d["G"], store=False)


@pytest.mark.parametrize("ca,cb,cout,why", [(129, 0, 8, "at most 128"), (8, 0, 257, "at most 256"), (100, 0, 200, "64 KiB")])
def test_pfn_layer_eval_refuses_what_it_cannot_hold(ca, cb, cout, why):
    """129 inputs, 257 outputs, a weight of 80 000 bytes: PnxError, and nothing is written."""
    from pillarnext_amd import ops
    from pillarnext_amd._lib import PnxError

    n, G = 10, 3
    xa, wt, shift = torch.zeros((n, ca), device="cuda"), torch.zeros((ca + cb, cout), device="cuda"), torch.zeros((cout,), device="cuda")
    inv = torch.zeros((n,), dtype=torch.int64, device="cuda")
    y, gmax = torch.full((n, cout), 7.0, device="cuda"), torch.full((G, cout), 7.0, device="cuda")
    with pytest.raises(PnxError, match=why):
        _raw_pfn(xa, None, inv, wt, shift, G, y, gmax)
    with pytest.raises(PnxError, match=why):
        ops.pfn_layer_eval(xa, None, inv, wt, shift, G)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((gmax == 7.0).all())


# ------------------------------------------------------------------------------------------------ pnx_bilinear_gather, forward
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}


def _gather(what, img32, dtype, pos, mn, vs, cells, inv, ds):
    """The kernel on the map cast to dtype against the twin on that map's exact values; returns the worst |out - S| / bound."""
    from pillarnext_amd import ops

    img = img32.to(dtype).contiguous(memory_format=torch.channels_last)
    got = ops.bilinear_gather(img, pos, mn, vs, cells, inv, ds)
    b = cells.cpu().numpy()[inv.cpu().numpy(), 0]
    out, S, A = P.gather(img.float().cpu().numpy(), pos.cpu().numpy(), mn, vs, b, ds)
    return P.gather_check(got.cpu().numpy(), out, S, A, b, img.shape[0], what)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("ds", [1, 8])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (5, 1), (9, 11)])
def test_bilinear_gather_smallest_shapes(H, W, ds, dtype):
    gen = torch.Generator(device="cuda").manual_seed(100 * H + W + ds)
    B = 2
    pos, mn, vs, cells, inv = _edge_points(H, W, B, ds, gen)                   # every image index, -1 and B included, at every kind of position
    assert pos.stride(0) == 5 and set(cells.cpu()[inv.cpu(), 0].tolist()) == {-1, 0, 1, 2}
    for C in (1, 48, 64, 65, 192, 200):                                        # lanes are channels: one pass, exactly one, one element past, three, a remainder
        img = torch.randn((B, C, H, W), device="cuda", generator=gen)
        _gather(f"gather {H} x {W} map, {C} channels, ds {ds}, {dtype}", img, DTYPES[dtype], pos, mn, vs, cells, inv, ds)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_bilinear_gather_without_points(dtype):
    """n = 0 (a batch whose points all fell outside the range): no launch, an empty result."""
    from pillarnext_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(1)
    pos, mn, vs, cells, inv = _edge_points(9, 11, 2, 2, gen)
    img = torch.randn((2, 65, 9, 11), device="cuda", generator=gen).to(DTYPES[dtype]).contiguous(memory_format=torch.channels_last)
    z = ops.bilinear_gather(img, pos[:0], mn, vs, cells, inv[:0], 2)
    assert z.shape == (0, 65) and z.dtype == torch.float32


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_bilinear_gather_past_the_largest_grid(dtype):
    """70 001 points: more than the 32 768 waves of the largest grid, so the wave-stride loop iterates; half of the points outside the batch."""
    gen = torch.Generator(device="cuda").manual_seed(11)
    n = 70_001
    pos = torch.rand((n, 2), device="cuda", generator=gen) * 18.0 - 1.0
    cells = torch.tensor(CELLS4, dtype=torch.int32, device="cuda")
    inv = torch.randint(0, 4, (n,), device="cuda", generator=gen)
    img = torch.randn((2, 48, 16, 16), device="cuda", generator=gen)
    _gather(f"gather 70001 points, 2 x 16 x 16, {dtype}", img, DTYPES[dtype], pos, [0.0, 0.0], [1.0, 1.0], cells, inv, 1)


def test_positions_beyond_32_bit_cell_coordinates():
    """+-3e9 cells from the map.  The reference floors to int64 and adds 1 there, so both corners of such a point clamp to the same border column (row);
    a 32-bit conversion saturates at 2^31 - 1 and the + 1 wraps to the other side of the map.  Forward and backward share the corner computation."""
    from pillarnext_amd import ops

    H, W, C, big = 9, 11, 65, 3e9
    pts = [[big, 4.25], [-big, 4.25], [5.5, big], [5.5, -big], [big, big], [-big, -big], [big, -big], [-big, big], [W - 1.5, H - 1.5], [0.25, 0.25], [W - 0.5, 3.0]]
    pos = torch.tensor(pts, dtype=torch.float32, device="cuda")
    cells = torch.tensor(CELLS4[:2], dtype=torch.int32, device="cuda")
    inv = (torch.arange(len(pts), device="cuda") % 2).long()
    gen = torch.Generator(device="cuda").manual_seed(4)
    img = torch.randn((2, C, H, W), device="cuda", generator=gen)
    mn, vs = [0.0, 0.0], [1.0, 1.0]
    x0, x1, y0, y1, *_ = R.corners_and_weights(pos.cpu().numpy(), mn, vs, 1, H, W)
    assert x0[:2].tolist() == x1[:2].tolist() == [W - 1, 0] and y0[2:4].tolist() == y1[2:4].tolist() == [H - 1, 0]
    for dtype in ("float32", "bfloat16"):
        _gather(f"gather +-3e9 cells, {dtype}", img, DTYPES[dtype], pos, mn, vs, cells, inv, 1)
    go = torch.randn((len(pts), C), device="cuda", generator=gen)
    b = cells.cpu().numpy()[inv.cpu().numpy(), 0]
    S, A, k = R.grad_image(go.cpu().numpy(), (2, C, H, W), pos.cpu().numpy(), mn, vs, b, 1)
    R.check(ops.bilinear_gather_backward(go, (2, C, H, W), pos, mn, vs, cells, inv, 1).cpu().numpy(), S, A, k, "backward +-3e9 cells")


# ------------------------------------------------------------------------------------------------ pnx_scatter_max and its backward
@pytest.mark.parametrize("C", P.SM_CHANNELS)
@pytest.mark.parametrize("pillars", P.SM_PILLARS)
def test_scatter_max_and_its_backward_are_exact(pillars, C):
    from pillarnext_amd import ops
    from pillarnext_amd._lib import check, lib, ptr, stream_ptr

    for n in P.SM_ROWS:
        what = f"scatter_max n={n}, {C} channels, {pillars} pillars"
        x, index = P.scatter_inputs(n, C, pillars, seed=7 * C + pillars + n)
        want, warg = P.scatter_max(x, index, pillars)
        xt, it = torch.from_numpy(x).cuda(), torch.from_numpy(index).cuda()
        out, arg = ops.scatter_max(xt, it, pillars)
        assert out.shape == arg.shape == (pillars, C) and arg.dtype == torch.int64
        assert np.array_equal(arg.cpu().numpy(), warg), what                                   # the lowest row among the maxima; n for a pillar without rows
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), what   # that row's value, -inf and the sign of a zero included
        for _ in range(2):                                                                     # the same bits again, also over a workspace of 0xFF bytes
            ops._SM_WS.buf.fill_(0xFF)
            out2, arg2 = ops.scatter_max(xt, it, pillars)
            assert torch.equal(_bits(out2), _bits(out)) and torch.equal(arg2, arg), what
        # backward: g routed through the argmax, every other element +0 although the output held NaN
        g = torch.from_numpy(np.random.default_rng(n + C).standard_normal((pillars, C)).astype(np.float32)).cuda()
        wgx = P.scatter_max_backward(g.cpu().numpy(), warg, n)
        gx = torch.full((n, C), float("nan"), device="cuda")
        check(lib().pnx_scatter_max_backward(ptr(g), ptr(arg), n, C, pillars, ptr(gx), stream_ptr()), "pnx_scatter_max_backward")
        assert np.array_equal(gx.cpu().numpy().view(np.uint32), wgx.view(np.uint32)), what
        xr = xt.clone().requires_grad_(True)                                                   # and through the autograd node
        ops.scatter_max(xr, it, pillars)[0].backward(g)
        assert np.array_equal(xr.grad.cpu().numpy().view(np.uint32), wgx.view(np.uint32)), what
        dropped = (index < 0) | (index >= pillars)
        assert not np.any(wgx[dropped].view(np.uint32)) and (n < 2 or int(dropped.sum()) == n // 16)
    print(f"[scatter_max {C} channels, {pillars} pillars] forward, argmax and backward equal the twin exactly at n = {P.SM_ROWS}")


def test_scatter_max_past_one_pass_of_the_block_scan():
    """526 500 pillars are 258 scan blocks of 2048: the level-2 scan of the pillar offsets (SCAN_IDENT, as in the sweep merge) takes a second pass through its
    carry loop.  Rows on both sides of that seam (pillars 524 287 and 524 288) and on the last pillar; most pillars are empty."""
    from pillarnext_amd import ops
    from pillarnext_amd._lib import check, lib, ptr, stream_ptr

    pillars, n, C = 526_500, 20_000, 4
    assert -(-pillars // 2048) > 256
    rng = np.random.default_rng(526)
    x = np.clip(np.round(rng.standard_normal((n, C)) * 4.0) / 4.0, -2.0, 2.0).astype(np.float32)
    index = rng.integers(0, pillars, n).astype(np.int64)
    index[:3000] = rng.integers(524_000, 524_600, 3000)                                        # a crowd around the seam of the two passes
    index[3000:3040] = np.repeat([524_287, 524_288, pillars - 1, 0], 10)
    index[3040:3100] = np.array([-1, pillars, 1 << 40], np.int64)[np.arange(60) % 3]
    rng.shuffle(index)
    x[index == 524_288] = -np.abs(x[index == 524_288]) - np.float32(0.25)                      # an all-negative pillar right behind the seam
    want, warg = P.scatter_max(x, index, pillars)
    assert all((warg[p] < n).all() for p in (0, 524_287, 524_288, pillars - 1)) and int((warg[:, 0] < n).sum()) < pillars // 20
    xt, it = torch.from_numpy(x).cuda(), torch.from_numpy(index).cuda()
    out, arg = ops.scatter_max(xt, it, pillars)
    assert np.array_equal(arg.cpu().numpy(), warg) and np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    ops._SM_WS.buf.fill_(0xFF)
    out2, arg2 = ops.scatter_max(xt, it, pillars)
    assert torch.equal(_bits(out2), _bits(out)) and torch.equal(arg2, arg)
    g = torch.from_numpy(rng.standard_normal((pillars, C)).astype(np.float32)).cuda()
    wgx = P.scatter_max_backward(g.cpu().numpy(), warg, n)
    gx = torch.full((n, C), float("nan"), device="cuda")
    check(lib().pnx_scatter_max_backward(ptr(g), ptr(arg), n, C, pillars, ptr(gx), stream_ptr()), "pnx_scatter_max_backward")
    assert np.array_equal(gx.cpu().numpy().view(np.uint32), wgx.view(np.uint32))
    xr = xt.clone().requires_grad_(True)
    ops.scatter_max(xr, it, pillars)[0].backward(g)
    assert np.array_equal(xr.grad.cpu().numpy().view(np.uint32), wgx.view(np.uint32))
