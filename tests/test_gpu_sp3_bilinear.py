"""GPU: pnx_sp3_bilinear_gather / pnx_sp3_bilinear_gather_backward (csrc/group.hip) -- the view's map sampled at the points from the ROWS of an
active set -- against the dense pair they restate, exactly:
  - forward == pnx_bilinear_gather on the channels-last map scattered from the same rows (==, so -0 equals +0);
  - backward bit-identical to pnx_bilinear_gather_backward's map read at the active cells;
over maps down to one cell, ds_rate 1 and 8, channel counts around the 64-lane and 256-channel passes, every / one / no / checkerboard active cells,
points left of and above the first cell centre (negative weights), in the last column and row (coincident corners), with an image index outside
the batch, n = 0 / 1 / 70 and 5 000 points in one cell; the same bits on a repeat and over a workspace filled with 0xFF; the autograd node."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

B = 2
MN, VS = [-3.0, -3.0], [0.25, 0.5]


def _active(kind, H, W, gen):
    """coords (n_rows, 4) int32 [b, 0, y, x] in rank order."""
    b, y, x = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), indexing="ij")
    c = torch.stack([b, torch.zeros_like(b), y, x], -1).reshape(-1, 4)
    if kind == "one":
        c = c[int(torch.randint(len(c), (1,), generator=gen)):][:1]
    elif kind == "none":
        c = c[:0]
    elif kind == "checkerboard":
        c = c[(c[:, 0] + c[:, 2] + c[:, 3]) % 2 == 0]
    return c.int().cuda().contiguous()


def _points(n, H, W, ds, gen):
    """n points: sample positions from 1.5 cells left of / above the first centre to half a cell past the last, the first few pinned to the seams;
    cells (K, 3) whose image indices include -1 and B; inv (n,)."""
    u = torch.rand((n, 2), generator=gen) * torch.tensor([W + 2.0, H + 2.0]) - 1.5
    seams = torch.tensor([[-1.25, -0.5], [-0.25, H - 0.5], [W - 1.0, H - 1.0], [W - 0.75, 0.25], [W + 0.25, H + 0.25], [0.0, 0.0]])
    k = min(n, len(seams))
    u[:k] = seams[:k]
    pos = torch.tensor(MN) + u * torch.tensor(VS) * ds
    pos = torch.cat([pos, torch.rand((n, 1), generator=gen)], 1)[:, :2]          # rows of a wider buffer: row stride 3
    cells = torch.tensor([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [B, 0, 0], [1, 0, 0]], dtype=torch.int32)
    inv = torch.randint(len(cells), (n,), generator=gen)
    if n > 6:
        inv[:6] = torch.tensor([0, 1, 0, 1, 0, 1])                                # the seam points stay inside the batch
    return pos.cuda(), cells.cuda(), inv.cuda()


def _dense(rows, coords, H, W):
    C = rows.shape[1]
    img = torch.zeros((B, H, W, C), device="cuda")
    c = coords.long()
    img[c[:, 0], c[:, 2], c[:, 3]] = rows
    return img.permute(0, 3, 1, 2)


def _both(rows, coords, H, W, pos, cells, inv, ds, go):
    from pillarnext_amd import ops

    ix, _, _ = ops.sp3_index_build(coords, B, (1, H, W))
    C = rows.shape[1]
    out = ops.sp3_bilinear_gather(rows, ix, pos, MN, VS, cells, inv, ds)
    ref = ops.bilinear_gather(_dense(rows, coords, H, W), pos, MN, VS, cells, inv, ds)
    gr = ops.sp3_bilinear_gather_backward(go, coords, ix, pos, MN, VS, cells, inv, ds)
    gi = ops.bilinear_gather_backward(go, (B, C, H, W), pos, MN, VS, cells, inv, ds)
    c = coords.long()
    return ix, out, ref, gr, gi.permute(0, 2, 3, 1)[c[:, 0], c[:, 2], c[:, 3]]


@pytest.mark.parametrize("ds", [1, 8])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (5, 1), (9, 11)])
def test_rows_equal_the_dense_pair(H, W, ds):
    gen = torch.Generator().manual_seed(H * 100 + W * 10 + ds)
    checked = 0
    for C in (1, 48, 192, 257):
        for kind in ("every", "one", "none", "checkerboard"):
            coords = _active(kind, H, W, gen)
            rows = torch.randn((coords.shape[0], C), generator=gen).cuda()
            for n in (0, 1, 70):
                pos, cells, inv = _points(n, H, W, ds, gen)
                go = torch.randn((n, C + 3), generator=gen).cuda()[:, 1:C + 1]      # a column slice, read in place
                _, out, ref, gr, gref = _both(rows, coords, H, W, pos, cells, inv, ds, go)
                what = f"{H} x {W}, ds {ds}, {C} channels, {kind} active, n {n}"
                assert out.shape == (n, C) and gr.shape == (coords.shape[0], C), what
                assert bool((out == ref).all()), f"forward differs: {what}"
                assert torch.equal(gr.view(torch.int32), gref.contiguous().view(torch.int32)), f"backward differs: {what}"
                if n:
                    outside = (cells[inv, 0] < 0) | (cells[inv, 0] >= B)
                    assert not bool(out[outside].any()) and not bool(torch.signbit(out[outside]).any()), "a point outside the batch gets +0"
                checked += 1
    assert checked == 48


def test_negative_weights_and_coincident_corners_are_reached():
    """The seam points of _points do what they are there for, by the fp64 statement of the corners (tests/mvf_bilinear_ref.py)."""
    import mvf_bilinear_ref as R

    H, W, ds = 9, 11, 8
    pos, _, _ = _points(70, H, W, ds, torch.Generator().manual_seed(1))
    x0, x1, y0, y1, wa, wb, wc, wd = R.corners_and_weights(pos.cpu().numpy(), MN, VS, ds, H, W)
    assert (np.minimum(np.minimum(wa, wb), np.minimum(wc, wd)) < 0).any(), "no negative weight"
    assert (x0 == x1).any() and (y0 == y1).any() and ((x0 == x1) & (y0 == y1)).any(), "no coincident corners"


def test_many_points_in_one_cell_and_equal_bits_over_a_dirty_workspace():
    from pillarnext_amd import ops

    gen = torch.Generator().manual_seed(5)
    H, W, ds, C, n = 9, 11, 8, 48, 5000
    coords = _active("checkerboard", H, W, gen)
    rows = torch.randn((coords.shape[0], C), generator=gen).cuda()
    u = torch.tensor([4.0, 3.0]) + torch.rand((n, 2), generator=gen) * 0.999     # base cell (y 3, x 4) of image 1 for every point
    pos = (torch.tensor(MN) + u * torch.tensor(VS) * ds).cuda()
    cells = torch.tensor([[1, 0, 0]], dtype=torch.int32).cuda()
    inv = torch.zeros((n,), dtype=torch.int64).cuda()
    go = torch.randn((n, C), generator=gen).cuda()
    ix, out, ref, gr, gref = _both(rows, coords, H, W, pos, cells, inv, ds, go)
    assert bool((out == ref).all())
    assert torch.equal(gr.view(torch.int32), gref.contiguous().view(torch.int32))
    assert int((gr != 0).any(1).sum()) == 2, "the four corners around one base cell, two of them on the checkerboard"
    again = ops.sp3_bilinear_gather_backward(go, coords, ix, pos, MN, VS, cells, inv, ds)
    assert torch.equal(gr.view(torch.int32), again.view(torch.int32))
    assert ops._BILGRAD_WS.buf is not None
    ops._BILGRAD_WS.buf.fill_(0xFF)
    third = ops.sp3_bilinear_gather_backward(go, coords, ix, pos, MN, VS, cells, inv, ds)
    assert torch.equal(gr.view(torch.int32), third.view(torch.int32))


def test_empty_inputs_write_what_they_own():
    """n = 0 zero-fills grad_rows (although it held NaN) and launches no gather; n_rows = 0 samples an empty map."""
    import ctypes

    from pillarnext_amd import ops
    from pillarnext_amd._lib import check, lib, ptr, stream_ptr

    gen = torch.Generator().manual_seed(2)
    H, W, ds, C = 5, 6, 2, 7
    coords = _active("checkerboard", H, W, gen)
    ix, _, _ = ops.sp3_index_build(coords, B, (1, H, W))
    f2 = lambda v: (ctypes.c_float * 2)(float(v[0]), float(v[1]))  # noqa: E731
    gr = torch.full((coords.shape[0], C), float("nan"), device="cuda")
    nbytes = lib().pnx_sp3_bilinear_gather_backward_scratch_bytes(0, coords.shape[0])
    assert nbytes >= 256
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    check(lib().pnx_sp3_bilinear_gather_backward(None, C, ptr(coords), coords.shape[0], B, H, W, C, None, 2, f2(MN), f2(VS), None, None, ds, 0, ptr(gr), ptr(ws),
                                                 nbytes, stream_ptr()), "pnx_sp3_bilinear_gather_backward")
    assert not bool(gr.any()) and not bool(torch.signbit(gr).any())
    pos, cells, inv = _points(20, H, W, ds, gen)
    none = _active("none", H, W, gen)
    eix, _, _ = ops.sp3_index_build(none, B, (1, H, W))
    out = ops.sp3_bilinear_gather(torch.zeros((0, C), device="cuda"), eix, pos, MN, VS, cells, inv, ds)
    assert out.shape == (20, C) and not bool(out.any())
    assert ops.sp3_bilinear_gather_backward(torch.ones((20, C), device="cuda"), none, eix, pos, MN, VS, cells, inv, ds).shape == (0, C)
    assert lib().pnx_sp3_bilinear_gather_backward_scratch_bytes(1 << 31, 1) == 0 and lib().pnx_sp3_bilinear_gather_backward_scratch_bytes(1, -1) == 0


def test_autograd_node_gives_the_backward_kernel():
    from pillarnext_amd import ops

    gen = torch.Generator().manual_seed(3)
    H, W, ds, C = 9, 11, 8, 65
    coords = _active("checkerboard", H, W, gen)
    ix, _, _ = ops.sp3_index_build(coords, B, (1, H, W))
    rows = torch.randn((coords.shape[0], C), generator=gen).cuda().requires_grad_(True)
    pos, cells, inv = _points(70, H, W, ds, gen)
    out = ops.SparseBilinearGather.apply(rows, coords, ix, pos, MN, VS, cells, inv, ds)
    assert torch.equal(out, ops.sp3_bilinear_gather(rows.detach(), ix, pos, MN, VS, cells, inv, ds))
    go = torch.randn((70, C), generator=gen).cuda()
    (g,) = torch.autograd.grad(out, rows, go)
    assert torch.equal(g.view(torch.int32), ops.sp3_bilinear_gather_backward(go, coords, ix, pos, MN, VS, cells, inv, ds).view(torch.int32))
    # a gradient that arrives expanded (the backward of a sum) is made contiguous first
    (g1,) = torch.autograd.grad(ops.SparseBilinearGather.apply(rows, coords, ix, pos, MN, VS, cells, inv, ds).sum(), rows)
    ones = torch.ones((70, C), device="cuda")
    assert torch.equal(g1, ops.sp3_bilinear_gather_backward(ones, coords, ix, pos, MN, VS, cells, inv, ds))
    with pytest.raises(ops.PnxError):
        ops.sp3_bilinear_gather(rows.detach().cpu(), ix, pos, MN, VS, cells, inv, ds)
