"""CPU: the fp64 gradient rulebook of tests/sparse_conv3d_grad_ref.py against torch.autograd through dense fp64 F.conv3d on masked grids
(the construction of tests/test_sparse3d_cpu.py: dense conv x output mask) for every geometry SparseResNet3D has, transpose_map against a
brute-force dictionary, the submanifold mirror identity, and the restated launch split of pnx_sp3_wgrad against the library's workspace query."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

import sparse_conv3d_grad_ref as G  # noqa: E402
import sparse_conv3d_ref as R  # noqa: E402

GEOMETRIES = [  # (subm, kernel, stride, pad)
    (False, 3, 1, 1),
    (False, 3, 2, 1),
    (False, (3, 1, 1), (2, 1, 1), 0),
    (True, 3, 1, 1),
    (True, 1, 1, 0),
]


def _case(rng, B, grid, n, cin):
    D, H, W = grid
    c, _ = R.sort_rows(np.stack(np.unravel_index(rng.choice(B * D * H * W, size=n, replace=False), (B, D, H, W)), 1))
    return c, rng.standard_normal((n, cin))


def _layer(c, grid, subm, k, s, p):
    if subm:
        return c, grid, R.neighbor_map(c, c, k, s, p)
    oc, og = R.output_set(c, grid, k, s, p)
    return oc, og, R.neighbor_map(oc, c, k, s, p)


@pytest.mark.parametrize("subm,kernel,stride,pad", GEOMETRIES)
def test_gradient_rulebook_equals_autograd_of_masked_dense_conv(subm, kernel, stride, pad):
    rng = np.random.default_rng(11)
    B, grid, cin, cout = 2, (7, 6, 9), 3, 5
    D, H, W = grid
    c, x = _case(rng, B, grid, 45, cin)
    k, s, p = R.triple(kernel), R.triple(stride), R.triple(pad)
    w = rng.standard_normal((cout, *k, cin))
    oc, og, m = _layer(c, grid, subm, k, s, p)
    dy = rng.standard_normal((len(oc), cout))
    dy[len(oc) // 3] = 0.0
    # dense statement: rows -> grid, conv, output mask, loss = <Y, dY on the grid>
    ci, co = torch.from_numpy(c), torch.from_numpy(oc)
    tx = torch.from_numpy(x).requires_grad_(True)
    tw = torch.from_numpy(w).requires_grad_(True)
    X = torch.zeros((B, D, H, W, cin), dtype=torch.float64).index_put((ci[:, 0], ci[:, 1], ci[:, 2], ci[:, 3]), tx).permute(0, 4, 1, 2, 3)
    Mo = torch.zeros((B, 1, *og), dtype=torch.float64)
    Mo[co[:, 0], 0, co[:, 1], co[:, 2], co[:, 3]] = 1
    Y = F.conv3d(X, tw.permute(0, 4, 1, 2, 3), stride=s, padding=p) * Mo
    rows = Y.permute(0, 2, 3, 4, 1)[co[:, 0], co[:, 1], co[:, 2], co[:, 3]]
    np.testing.assert_allclose(R.gather_conv(x, m, w)[0], rows.detach().numpy(), rtol=1e-12, atol=1e-12)
    (rows * torch.from_numpy(dy)).sum().backward()
    dx, dx_mag = G.grad_input(m, w, dy, len(c))
    dw, dw_mag = G.grad_weight(m, x, dy)
    np.testing.assert_allclose(dx, tx.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dw.reshape(cout, *k, cin), tw.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert (dx_mag >= np.abs(dx) - 1e-12).all() and (dw_mag >= np.abs(dw) - 1e-12).all()
    # the data gradient as the forward rule on the transposed map and the transposed weights
    tm = G.transpose_map(m, len(c))
    wt = w.reshape(cout, -1, cin).transpose(2, 1, 0).reshape(cin, *k, cout)
    via, via_mag = R.gather_conv(dy, tm, wt)
    np.testing.assert_allclose(via, dx, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(via_mag, dx_mag, rtol=1e-12, atol=1e-12)
    # rows and taps without a neighbour: exactly zero
    T = m.shape[1]
    for t in range(T):
        if not (m[:, t] >= 0).any():
            assert not dw[:, t].any() and not dw_mag[:, t].any()
    unreached = np.setdiff1d(np.arange(len(c)), m[m >= 0])
    assert not dx[unreached].any()


@pytest.mark.parametrize("subm,kernel,stride,pad", GEOMETRIES)
def test_transpose_map_against_a_dictionary(subm, kernel, stride, pad):
    rng = np.random.default_rng(12)
    grid = (9, 10, 11)
    c, _ = _case(rng, 2, grid, 300, 1)
    k, s, p = R.triple(kernel), R.triple(stride), R.triple(pad)
    oc, og, m = _layer(c, grid, subm, k, s, p)
    where = {}
    for o in range(m.shape[0]):
        for t in range(m.shape[1]):
            if m[o, t] >= 0:
                assert (int(m[o, t]), t) not in where
                where[(int(m[o, t]), t)] = o
    tm = G.transpose_map(m, len(c))
    assert tm.shape == (len(c), m.shape[1])
    for i in range(tm.shape[0]):
        for t in range(tm.shape[1]):
            assert tm[i, t] == where.get((i, t), -1)
    assert (tm >= 0).sum() == (m >= 0).sum() > 0
    if subm:
        assert np.array_equal(tm, m[:, ::-1]), "submanifold mirror identity tmap[i][t] == map[i][T - 1 - t]"
        perm = rng.permutation(len(c))  # rows in any order, the same for inputs and outputs
        mp = R.neighbor_map(c[perm], c[perm], k, s, p)
        assert np.array_equal(G.transpose_map(mp, len(c)), mp[:, ::-1])


def test_restated_wgrad_split_matches_the_workspace_query():
    from pillarnext_amd import _lib

    L = _lib.lib()
    for n_out in (1, 15, 16, 255, 256, 257, 500, 4097, 131_072, 1_000_003, 8_900_000):
        for cout in (5, 16, 18, 36, 64, 72, 128, 144):
            R_, P, mt, groups = G.wgrad_split(n_out, cout)
            assert R_ % 16 == 0 and 256 <= R_ <= 4096 and (P - 1) * R_ < n_out <= P * R_ and groups * mt * 16 >= cout
            for T, cin in ((27, 18), (3, 144), (1, 5)):
                assert L.pnx_sp3_wgrad_workspace_bytes(n_out, T, cin, cout) == max(256, P * T * cin * cout * 4), (n_out, cout, T, cin)
    assert L.pnx_sp3_wgrad_workspace_bytes(100, 27, 145, 16) == 0 and L.pnx_sp3_wgrad_workspace_bytes(100, 28, 16, 16) == 0
    assert G.wgrad_tree_height(500, 18) == 256 + 2 and G.wgrad_tree_height(100, 18) == 100 + 1


def test_gradient_entry_points_validate_before_launching():
    import ctypes

    from pillarnext_amd import _lib

    L = _lib.lib()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.pnx_sp3_wgrad(p, 10, 200, p, 16, p, 10, 27, p, p, 1 << 20, None) < 0 and b"channels" in L.pnx_last_error()
    assert L.pnx_sp3_wgrad(p, 10, 16, p, 16, p, 10, 27, None, p, 1 << 20, None) < 0 and b"dw" in L.pnx_last_error()
    assert L.pnx_sp3_wgrad(p, 10, 16, p, 16, p, 10, 27, p, p, 8, None) < 0 and b"workspace" in L.pnx_last_error()
    assert L.pnx_sp3_transpose_map(p, 10, 28, 10, p, None) < 0 and b"taps" in L.pnx_last_error()
    assert L.pnx_sp3_transpose_map(p, 10, 27, 10, None, None) < 0 and b"null" in L.pnx_last_error()
    g = (ctypes.c_int32 * 3)(2, 3, 4)
    assert L.pnx_sp3_dense_backward(None, p, 10, 4, 1, g, p, None) < 0 and b"null" in L.pnx_last_error()
