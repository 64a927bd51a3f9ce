"""fp64 reference of the inference reader (pillar_encoder.py:95-125 dynamic pillarisation, :35-50 x2 PFNLayer in eval mode,
:174-182 PillarFeatureNet.forward) -- test helper next to sparse_conv3d_ref.py: plain numpy on the CPU, no kernel code.

What is fp32 in the reference module stays fp32 here, step by step as csrc/pfn_spans.hip documents it, so that the decorated features
are the SAME fp32 numbers the kernels see and everything measured against this reference is the error of the PFN alone:
  * cell index: (x - min) / voxel, fp32 subtract and fp32 IEEE divide, truncated (pe:95-96, :106-107);
  * range mask: fp32 compares against the integer grid size (pe:98-101);
  * cluster mean: the fp64 sum of the fp32 coordinates of the pillar, rounded to fp32, divided in fp32 by the fp32 count (pe:113);
  * x - mean and x - centre in fp32, the centre as idx*voxel + voxel/2 + min with every step rounded to fp32 (pe:114-120).
Everything behind the decorated features is fp64 from the RAW layer parameters: BatchNorm (eps 1e-3) folded in fp64, Linear, shift, ReLU,
per-pillar max, the concat with the pillar max, layer 1, ReLU, per-pillar max.

Besides the values it returns the magnitudes an error bar is built from (all fp64, all computed from the fp64 run):
  t1     (P, 64)  max over the pillar's points of  sum_k |W1'[c,k] x[k]| + |beta1[c]| + |mean1[c] a1[c]|      (layer 1's sum of |terms|)
  t01    (P, 64)  max over the pillar's points of  sum_k |W1'[c,k]| T0x[k], with T0x[k] = layer 0's sum of |terms| of input channel k:
                  sum_j |W0'[k,j] f[j]| + |beta0[k]| + |mean0[k] a0[k]| of the point for k < 32, its maximum over the pillar for k >= 32
  w1_l1  (64,)    sum_k |W1'[c,k]|;   x_l1 (P,)  max over the pillar's points of sum_k x[k]                    (absolute floors)
  h0max  (P, 32)  the layer-0 pillar maxima (post-ReLU): which pillars lie beyond the fp16 range of layer 1's split
(the max over the points is the right envelope for an output that is itself a max over the points: |max a' - max a| <= max |a' - a|)."""
import numpy as np

EPS = 1e-3


def _seg_max(x_sorted, starts):
    return np.maximum.reduceat(x_sorted, starts, axis=0)


def voxelize(points, pc_range, voxel_size, B=None):
    """The pillar set: kept (row indices of the points inside the range, original order), coords (P, 3) int32 [b, y, x] in torch.unique
    order (rows of [b, xi, yi] sorted), unq_inv (N',) int64, grid [ny, nx], and the integer cell of every kept point."""
    pts = np.ascontiguousarray(points, np.float32)
    pr, vs64 = np.asarray(pc_range, np.float64), np.asarray(voxel_size, np.float64)
    g = np.rint((pr[3:] - pr[:3]) / vs64).astype(np.int64)
    gx, gy = int(g[0]), int(g[1])
    pc_min, vs = pr[:3].astype(np.float32), vs64.astype(np.float32)
    with np.errstate(invalid="ignore"):
        cx = (pts[:, 1] - pc_min[0]) / vs[0]
        cy = (pts[:, 2] - pc_min[1]) / vs[1]
        keep = (cx >= 0) & (cx < np.float32(gx)) & (cy >= 0) & (cy < np.float32(gy))
    kept = np.flatnonzero(keep)
    xi, yi, bi = cx[kept].astype(np.int64), cy[kept].astype(np.int64), pts[kept, 0].astype(np.int64)
    key = (bi * gx + xi) * gy + yi
    unq, inv = np.unique(key, return_inverse=True)
    coords = np.stack([unq // (gx * gy), unq % gy, (unq // gy) % gx], axis=1).astype(np.int32)
    return dict(kept=kept, coords=coords, unq_inv=inv.astype(np.int64).reshape(-1), grid=np.array([gy, gx], np.int64), xi=xi, yi=yi, P=len(unq),
                pc_min=pc_min, vs=vs)


def decorate(points, v):
    """(N', F + 5) fp32: raw columns | x - cluster mean | x - pillar centre."""
    pts = np.ascontiguousarray(points, np.float32)[v["kept"]]
    inv, P = v["unq_inv"], v["P"]
    cnt = np.bincount(inv, minlength=P)
    mean = np.empty((P, 3), np.float32)
    for k in range(3):
        s = np.bincount(inv, weights=pts[:, 1 + k].astype(np.float64), minlength=P)   # fp64 sum of the fp32 coordinates
        mean[:, k] = s.astype(np.float32) / cnt.astype(np.float32)                     # rounded to fp32, fp32 divide
    vs, pc_min = v["vs"], v["pc_min"]
    ctr_x = (v["xi"].astype(np.float32) * vs[0] + vs[0] / np.float32(2)) + pc_min[0]    # numpy rounds every fp32 step, no FMA
    ctr_y = (v["yi"].astype(np.float32) * vs[1] + vs[1] / np.float32(2)) + pc_min[1]
    f = np.concatenate([pts[:, 1:], pts[:, 1:4] - mean[inv], (pts[:, 1] - ctr_x)[:, None], (pts[:, 2] - ctr_y)[:, None]], axis=1)
    assert f.dtype == np.float32
    return f, cnt


def fold64(L, eps=EPS):
    """BatchNorm(eval) folded in fp64: W' = W a, shift = beta - mean a, a = gamma / sqrt(var + eps); |beta| + |mean a| for the bars."""
    W, gamma, beta, mean, var = (np.asarray(L[k], np.float64) for k in ("W", "gamma", "beta", "mean", "var"))
    a = gamma / np.sqrt(var + eps)
    return W * a[:, None], beta - mean * a, np.abs(beta) + np.abs(mean * a)


def reader_forward(points, pc_range, voxel_size, layers, B=None, eps=EPS):
    assert len(layers) == 2
    v = voxelize(points, pc_range, voxel_size, B)
    feat, cnt = decorate(points, v)
    inv, P = v["unq_inv"], v["P"]
    out = dict(coords=v["coords"], unq_inv=inv, grid=v["grid"], kept=v["kept"], features=feat, counts=cnt, P=P)
    if P == 0:
        z = np.zeros((0, 64))
        out.update(feat_max=z, t1=z, t01=z, h0max=np.zeros((0, 32)), x_l1=np.zeros(0), w1_l1=np.zeros(64))
        return out
    order = np.argsort(inv, kind="stable")
    starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    inv_s = inv[order]
    f = feat[order].astype(np.float64)                       # pillar-sorted from here on
    W0, s0, a0 = fold64(layers[0], eps)
    W1, s1, a1 = fold64(layers[1], eps)
    h0 = np.maximum(f @ W0.T + s0, 0.0)                       # (N', 32)
    t0 = np.abs(f) @ np.abs(W0).T + a0                        # layer 0's sum of |terms|
    h0max = _seg_max(h0, starts)
    t0max = _seg_max(t0, starts)
    x = np.concatenate([h0, h0max[inv_s]], axis=1)            # (N', 64): the concat of pe:49
    t0x = np.concatenate([t0, t0max[inv_s]], axis=1)
    y = np.maximum(x @ W1.T + s1, 0.0)
    aW1 = np.abs(W1)
    out.update(feat_max=_seg_max(y, starts), h0max=h0max,
               t1=_seg_max(x @ aW1.T + a1, starts),          # x >= 0: |W1' x| = |W1'| x
               t01=_seg_max(t0x @ aW1.T, starts),
               x_l1=_seg_max(x.sum(1), starts), w1_l1=aW1.sum(1))
    return out
