"""Test helper (not a test): the fp64 gradient rulebook of the sparse 3-D convolution of tests/sparse_conv3d_ref.py,
    y[o] = sum_t w[:, t, :] . x[map[o][t]]          (map[o][t] = input row or -1, taps (od*kh + oh)*kw + ow)
    dx[i] = sum over (o, t) with map[o][t] = i of w[:, t, :]^T . dy[o]
    dw[co][t][ci] = sum_o dy[o][co] * x[map[o][t]][ci]
each with the sum of |terms| of every element (the scale of the GPU tests' error bars), the transposed map the data gradient runs on, and
the launch split of pnx_sp3_wgrad as include/pnx.h documents it."""
import numpy as np


def transpose_map(nbmap, n_in):
    """tmap (n_in, T): tmap[map[o][t]][t] = o, -1 elsewhere.  An input row and tap reach at most one output row; a second one is an error."""
    nbmap = np.asarray(nbmap, np.int64)
    t = np.full((n_in, nbmap.shape[1]), -1, np.int64)
    o, tap = np.nonzero(nbmap >= 0)
    rows = nbmap[o, tap]
    assert len(np.unique(rows * nbmap.shape[1] + tap)) == len(rows), "two output rows reach one input row through the same tap"
    t[rows, tap] = o
    return t


def grad_input(nbmap, weight, dy, n_in):
    """-> (dx (n_in, Cin) fp64, sum of |terms|)."""
    w = np.asarray(weight, np.float64)
    co, ci = w.shape[0], w.shape[-1]
    wt = w.reshape(co, -1, ci)
    dy = np.asarray(dy, np.float64)
    dx, mag = np.zeros((n_in, ci)), np.zeros((n_in, ci))
    for t in range(nbmap.shape[1]):
        o = np.nonzero(nbmap[:, t] >= 0)[0]
        np.add.at(dx, nbmap[o, t], dy[o] @ wt[:, t])
        np.add.at(mag, nbmap[o, t], np.abs(dy[o]) @ np.abs(wt[:, t]))
    return dx, mag


def grad_weight(nbmap, feats, dy):
    """-> (dw (Cout, T, Cin) fp64, sum of |terms|); an entry -1 contributes nothing."""
    x, dy = np.asarray(feats, np.float64), np.asarray(dy, np.float64)
    T = nbmap.shape[1]
    dw, mag = np.zeros((dy.shape[1], T, x.shape[1])), np.zeros((dy.shape[1], T, x.shape[1]))
    for t in range(T):
        o = np.nonzero(nbmap[:, t] >= 0)[0]
        dw[:, t] = dy[o].T @ x[nbmap[o, t]]
        mag[:, t] = np.abs(dy[o]).T @ np.abs(x[nbmap[o, t]])
    return dw, mag


def wgrad_split(n_out, cout):
    """pnx_sp3_wgrad's static split (include/pnx.h): (rows per workgroup R, partials P, output-channel tiles per wave, channel groups)."""
    tiles = (cout + 15) // 16
    mt = tiles if tiles <= 3 else (3 if tiles % 3 == 0 else (2 if tiles % 2 == 0 else 3))
    groups = (tiles + mt - 1) // mt
    p0 = max(1, 256 // groups)
    R = min(max(((n_out + p0 - 1) // p0 + 15) // 16 * 16, 256), 4096)
    return R, (n_out + R - 1) // R, mt, groups


def wgrad_tree_height(n_out, cout):
    """Height of the summation tree of one dw element: the longest FMA chain inside a workgroup (one FMA per row of its chunk, in row
    order) plus the number of partials the second kernel adds."""
    R, P, _, _ = wgrad_split(n_out, cout)
    return min(R, n_out) + P
