"""Test helper (not a test): a numpy rulebook restatement of spconv's SubMConv3d / SparseConv3d, BatchNorm1d in eval mode, SparseBasicBlock3d
and `dense().view(B, C*D, H, W)` for small cases -- oracle/sparse_conv_ref.py's 2-D conventions on three axes (z, y, x):

    SubMConv3d      out[p] = sum_o W[o] . in[p + o - k//2] over ACTIVE neighbours; the output set is the input set
    SparseConv3d    an output q exists iff some active input lies at q*s - pad + o; out[q] = sum_o W[o] . in[q*s - pad + o]
    output extent   (n + 2 pad - k) // s + 1 per axis

Weights are spconv >= 2.2's (Cout, kD, kH, kW, Cin); taps run (od*kh + oh)*kw + ow.  Everything is fp64; every conv also returns the sum of
|terms| of each output element, the scale of the per-element error bars the GPU tests use."""
import numpy as np


def triple(v):
    return tuple(int(a) for a in v) if isinstance(v, (list, tuple)) else (int(v),) * 3


def out_grid(grid, kernel, stride, pad):
    return tuple((n + 2 * p - k) // s + 1 for n, k, s, p in zip(grid, triple(kernel), triple(stride), triple(pad)))


def sort_rows(coords):
    coords = np.asarray(coords, np.int64).reshape(-1, 4)
    order = np.lexsort(coords.T[::-1])
    return coords[order], order


def output_set(coords, grid, kernel, stride, pad):
    """SparseConv3d's output set, sorted [b, z, y, x]."""
    k, s, p = triple(kernel), triple(stride), triple(pad)
    og = out_grid(grid, k, s, p)
    out = set()
    for b, *c in np.asarray(coords, np.int64).tolist():
        for od in range(k[0]):
            for oh in range(k[1]):
                for ow in range(k[2]):
                    t = [c[0] + p[0] - od, c[1] + p[1] - oh, c[2] + p[2] - ow]
                    if all(t[a] >= 0 and t[a] % s[a] == 0 and t[a] // s[a] < og[a] for a in range(3)):
                        out.add((b, t[0] // s[0], t[1] // s[1], t[2] // s[2]))
    return sort_rows(sorted(out))[0], og


def neighbor_map(coords_out, coords_in, kernel, stride, pad):
    """(N_out, T) row of coords_in at q*s - pad + o, -1 where inactive."""
    k, s, p = triple(kernel), triple(stride), triple(pad)
    where = {tuple(r): i for i, r in enumerate(np.asarray(coords_in, np.int64).tolist())}
    T = k[0] * k[1] * k[2]
    m = np.full((len(coords_out), T), -1, np.int64)
    for i, (b, z, y, x) in enumerate(np.asarray(coords_out, np.int64).tolist()):
        for t in range(T):
            o = (t // (k[1] * k[2]), (t // k[2]) % k[1], t % k[2])
            m[i, t] = where.get((b, z * s[0] - p[0] + o[0], y * s[1] - p[1] + o[1], x * s[2] - p[2] + o[2]), -1)
    return m


def gather_conv(feats, nbmap, weight):
    """sum over taps of W[:, t] . x[nbmap[:, t]] -> (out (N_out, Cout) fp64, sum of |terms| (N_out, Cout))."""
    w = np.asarray(weight, np.float64)
    co, ci = w.shape[0], w.shape[-1]
    wt = w.reshape(co, -1, ci)
    x = np.asarray(feats, np.float64)
    out = np.zeros((nbmap.shape[0], co))
    mag = np.zeros_like(out)
    for t in range(nbmap.shape[1]):
        ok = nbmap[:, t] >= 0
        xs = np.where(ok[:, None], x[np.maximum(nbmap[:, t], 0)] if len(x) else 0.0, 0.0)
        out += xs @ wt[:, t].T
        mag += np.abs(xs) @ np.abs(wt[:, t]).T
    return out, mag


def subm_conv3d(coords, feats, weight, kernel):
    k = triple(kernel)
    m = neighbor_map(coords, coords, k, 1, tuple(a // 2 for a in k))
    return gather_conv(feats, m, weight)


def sparse_conv3d(coords, feats, weight, grid, kernel, stride, pad):
    """-> (coords_out sorted, out, |terms|, grid_out)."""
    oc, og = output_set(coords, grid, kernel, stride, pad)
    out, mag = gather_conv(feats, neighbor_map(oc, coords, kernel, stride, pad), weight)
    return oc, out, mag, og


def bn_eval(x, gamma, beta, mean, var, eps=1e-3):
    return (x - mean) / np.sqrt(var + eps) * gamma + beta


def relu(x):
    return np.maximum(x, 0.0)


def basic_block(coords, x, w1, bn1, w2, bn2, kernel=3):
    """SparseBasicBlock3d: relu(bn2(subm(relu(bn1(subm(x))))) + x)."""
    y = relu(bn_eval(subm_conv3d(coords, x, w1, kernel)[0], *bn1))
    return relu(bn_eval(subm_conv3d(coords, y, w2, kernel)[0], *bn2) + x)


def dense_view(coords, feats, batch, grid):
    """x.dense() (B, C, D, H, W) then view(B, C*D, H, W): channel c*D + d."""
    D, H, W = grid
    C = feats.shape[1]
    out = np.zeros((batch, C, D, H, W))
    c = np.asarray(coords, np.int64)
    out[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]] = feats
    return out.reshape(batch, C * D, H, W)
