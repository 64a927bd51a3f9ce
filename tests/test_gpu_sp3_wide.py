"""GPU: the sparse convolution kernels of csrc/sparse3d.hip above 144 channels -- what the MVF view nets (48 / 96 / 192 / 192) need.
  - pnx_sp3_conv and pnx_sp3_conv_train (both summation forms) at cout up to 192 (accumulator tiles NT = 10, 11, 12) against the fp64 rulebook of
    tests/sparse_conv3d_ref.py on the operands the kernel saw: |err| <= 1e-6 * sum|terms| + 1e-30 per element, the bar of test_gpu_sparse3d.py;
    9 taps (kernel (1, 3, 3): submanifold and stride (1, 2, 2)) and 27 taps, with and without residual and ReLU, row counts around the 16-row tile
    and the 64-row workgroup, and a map without a single neighbour
  - ops.sp3_wgrad above 144 channels, served by column blocks: h * 2^-24 * sum|terms| + 1e-30 with h the height of the summation tree of the call
    that wrote the element (test_gpu_sparse3d_grad.py's bar, per block), one and several partials, equal bits on a repeat
  - the data gradient through sparse_conv_dgrad at 192 channels."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import sparse_conv3d_grad_ref as G  # noqa: E402
import sparse_conv3d_ref as R  # noqa: E402

EPS32 = 2.0 ** -24
PAIRS = [(96, 192), (192, 192), (150, 176), (192, 145)]
GEOMS = {  # name -> (grid, kernel, stride, pad, submanifold, cells)
    "subm9": ((1, 40, 41), (1, 3, 3), (1, 1, 1), (0, 1, 1), True, 900),
    "s2x9": ((1, 61, 62), (1, 3, 3), (1, 2, 2), (0, 1, 1), False, 900),
    "subm27": ((7, 12, 13), (3, 3, 3), (1, 1, 1), (1, 1, 1), True, 900),
}
_maps = {}


def _map(geom):
    """(input coords, kernel, map (N_out, T) on the device, the same map from the numpy rulebook) of one geometry, built once."""
    if geom not in _maps:
        from pillarnext_amd import ops

        grid, k, s, p, subm, n = GEOMS[geom]
        rng = np.random.default_rng(len(geom) + 11)
        B = 2
        keys = rng.choice(B * int(np.prod(grid)), size=n, replace=False)
        c, _ = R.sort_rows(np.stack(np.unravel_index(keys, (B, *grid)), 1))
        tc = torch.from_numpy(c).int().cuda().contiguous()
        ix, rows, _ = ops.sp3_index_build(tc, B, grid, want_rows=True)
        if subm:
            oc = tc
        else:
            oix, cnt = ops.sp3_out_index(tc, B, grid, k, s, p)
            oc = ops.sp3_index_coords(oix, int(cnt.item()))
            assert np.array_equal(oc.cpu().numpy(), R.output_set(c, grid, k, s, p)[0])
        m = ops.sp3_neighbor_map(oc, ix, rows, k, s, p)
        ref_m = R.neighbor_map(oc.cpu().numpy(), c, k, s, p)
        assert np.array_equal(m.cpu().numpy(), ref_m), "neighbour map differs"
        assert m.shape[0] >= 807
        _maps[geom] = (len(c), k, m, ref_m)
    return _maps[geom]


def _operands(rng, n_in, k, cin, cout):
    x = rng.standard_normal((n_in, cin)).astype(np.float32)
    w = (rng.standard_normal((cout, *k, cin)) / np.sqrt(cin * np.prod(k))).astype(np.float32)
    return x, w


@pytest.mark.parametrize("cin,cout", PAIRS)
@pytest.mark.parametrize("n_out", [1, 15, 16, 17, 65, 807])
def test_wide_conv_against_fp64_rulebook(n_out, cin, cout):
    from pillarnext_amd import ops

    for geom in GEOMS:
        n_in, k, m_all, ref_all = _map(geom)
        m, ref_m = m_all[:n_out].contiguous(), ref_all[:n_out]      # the first n_out output rows: a map is valid row by row
        rng = np.random.default_rng(cin * 1000 + cout + n_out)
        x, w = _operands(rng, n_in, k, cin, cout)
        shift = rng.standard_normal(cout).astype(np.float32)
        res = rng.standard_normal((n_out, cout)).astype(np.float32)
        tx, tw, ts, tr = (torch.from_numpy(a).cuda() for a in (x, w, shift, res))
        wp = ops.sp3_pack_weight(tw)
        acc, mag = R.gather_conv(x.astype(np.float64), ref_m, w.astype(np.float64))
        for with_res in (False, True):
            ref = acc + shift.astype(np.float64) + (res.astype(np.float64) if with_res else 0.0)
            bar = 1e-6 * (mag + np.abs(shift.astype(np.float64)) + (np.abs(res.astype(np.float64)) if with_res else 0.0)) + 1e-30
            for per_tap in (False, True):
                y = ops.sp3_conv(tx, m, wp, ts, cout, residual=tr if with_res else None, relu=False, per_tap=per_tap)
                assert y.shape == (n_out, cout)
                err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
                worst = float(np.max(err / bar))
                print(f"[{geom} {cin}->{cout} n_out {n_out} res {with_res} per_tap {per_tap}] worst {worst * 1e-6:.3g} of sum|terms| (bar 1e-6)")
                assert (err <= bar).all(), f"{geom} res {with_res} per_tap {per_tap}: worst {worst * 1e-6:.3g} of sum|terms|"
                yr = ops.sp3_conv(tx, m, wp, ts, cout, residual=tr if with_res else None, relu=True, per_tap=per_tap)
                assert torch.equal(yr, torch.clamp(y, min=0)), "ReLU epilogue"


@pytest.mark.parametrize("cin,cout", PAIRS)
@pytest.mark.parametrize("per_tap", [False, True])
def test_wide_conv_of_a_map_without_neighbours(cin, cout, per_tap):
    """Every entry -1: no tap runs, y is the shift (+ residual), exactly."""
    from pillarnext_amd import ops

    rng = np.random.default_rng(cin + cout)
    n_out, T = 70, 9
    x, w = _operands(rng, 33, (1, 3, 3), cin, cout)
    shift = torch.from_numpy(rng.standard_normal(cout).astype(np.float32)).cuda()
    res = torch.from_numpy(rng.standard_normal((n_out, cout)).astype(np.float32)).cuda()
    m = torch.full((n_out, T), -1, dtype=torch.int32, device="cuda")
    wp = ops.sp3_pack_weight(torch.from_numpy(w).cuda())
    tx = torch.from_numpy(x).cuda()
    assert torch.equal(ops.sp3_conv(tx, m, wp, shift, cout, relu=False, per_tap=per_tap), shift.expand(n_out, cout))
    assert torch.equal(ops.sp3_conv(tx, m, wp, shift, cout, residual=res, relu=True, per_tap=per_tap), torch.clamp(shift + res, min=0))


def test_conv_refuses_more_than_192_output_channels():
    from pillarnext_amd import ops

    m = torch.full((4, 9), -1, dtype=torch.int32, device="cuda")
    x = torch.zeros((4, 16), device="cuda")
    wp = ops.sp3_pack_weight(torch.zeros((193, 1, 3, 3, 16), device="cuda"))
    with pytest.raises(ops.PnxError, match="cout 1..192"):
        ops.sp3_conv(x, m, wp, torch.zeros(193, device="cuda"), 193)


@pytest.mark.parametrize("cin,cout", PAIRS + [(192, 96)])
@pytest.mark.parametrize("n_out", [1, 300, 4100])
def test_wide_wgrad_by_column_blocks(n_out, cin, cout):
    from pillarnext_amd import ops

    rng = np.random.default_rng(cin * 1000 + cout + n_out + 5)
    B, grid, k = 1, (1, 80, 81), (1, 3, 3)
    keys = rng.choice(B * int(np.prod(grid)), size=max(n_out, 2), replace=False)
    c, _ = R.sort_rows(np.stack(np.unravel_index(keys, (B, *grid)), 1))
    tc = torch.from_numpy(c).int().cuda().contiguous()
    ix, _, _ = ops.sp3_index_build(tc, B, grid)
    m = ops.sp3_neighbor_map(tc, ix, None, k, (1, 1, 1), (0, 1, 1))[:n_out].contiguous()
    ref_m = m.cpu().numpy().astype(np.int64)
    x = rng.standard_normal((len(c), cin)).astype(np.float32)
    dy = rng.standard_normal((n_out, cout)).astype(np.float32)
    tx, tdy = torch.from_numpy(x).cuda(), torch.from_numpy(dy).cuda()
    dw = ops.sp3_wgrad(tx, m, tdy)
    assert dw.shape == (cout, 9, cin)
    ref, mag = G.grad_weight(ref_m, x.astype(np.float64), dy.astype(np.float64))
    err = np.abs(dw.cpu().numpy().astype(np.float64) - ref)
    parts = []
    for so, ko in ops.sp3_wgrad_blocks(cout):
        assert ko <= 144
        h = G.wgrad_tree_height(n_out, ko)       # the call that wrote dw[so : so + ko] saw ko output channels
        parts.append(G.wgrad_split(n_out, ko)[1])
        e, g = err[so:so + ko], mag[so:so + ko]
        print(f"[{cin}->{cout} n_out {n_out}] dw[{so}:{so + ko}] worst {np.max(e / (g + 1e-30)):.3g} of sum|terms| (bar {h * EPS32:.3g}, h = {h})")
        assert (e <= h * EPS32 * g + 1e-30).all(), f"dw[{so}:{so + ko}] worst {np.max(e / (g + 1e-30)):.3g} of sum|terms|, bar {h * EPS32:.3g}"
    assert min(parts) > 1 if n_out == 4100 else max(parts) == 1 if n_out == 1 else True, f"{parts} partials"
    assert not dw[torch.from_numpy(mag == 0).cuda()].any(), "an element without a term must be exactly 0"
    assert torch.equal(dw, ops.sp3_wgrad(tx, m, tdy)), "dw differs between two runs"


@pytest.mark.parametrize("cin,cout", [(192, 192), (96, 192)])
@pytest.mark.parametrize("geom", ["subm9", "s2x9"])
def test_wide_data_gradient(geom, cin, cout):
    from pillarnext_amd.sparse3d import sparse_conv_dgrad

    n_in, k, m, ref_m = _map(geom)
    rng = np.random.default_rng(cin + cout + len(geom))
    _, w = _operands(rng, 1, k, cin, cout)
    dy = rng.standard_normal((m.shape[0], cout)).astype(np.float32)
    tw, tdy = torch.from_numpy(w).cuda(), torch.from_numpy(dy).cuda()
    subm = GEOMS[geom][4]
    dx = sparse_conv_dgrad(tdy, tw, m, n_in, subm=subm)
    assert dx.shape == (n_in, cin)
    ref, mag = G.grad_input(ref_m, w.astype(np.float64), dy.astype(np.float64), n_in)
    err = np.abs(dx.cpu().numpy().astype(np.float64) - ref)
    print(f"[{geom} {cin}->{cout}] dx worst {np.max(err / (mag + 1e-30)):.3g} of sum|terms| (bar 1e-6)")
    assert (err <= 1e-6 * mag + 1e-30).all(), f"dx worst {np.max(err / (mag + 1e-30)):.3g} of sum|terms|"
    assert torch.equal(dx, sparse_conv_dgrad(tdy, tw, m, n_in, subm=subm)), "dx differs between two runs"
