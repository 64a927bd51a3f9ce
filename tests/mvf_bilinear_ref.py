"""The yardstick of the bilinear sampling's gradient (pnx_bilinear_gather_backward): an fp64 numpy twin and the bound it is compared under.

Corners and weights are computed in np.float32 with the forward kernel's operation order (k_bilinear / SingleView.bilinear_interpolate,
det3d/models/readers/mvf_encoder.py:208-246): subtract, IEEE divide, multiply by 1 / ds, floor, clamp, subtract, multiply -- every fp32 operation
rounded once, so the weights are the kernel's bit for bit.  The sum of weight * grad_out per cell is then taken in fp64.

Bound (derived, not measured).  A cell's value is a sum of k terms w * g, each an fp32 product (one rounding, relative error <= u = 2^-24)
summed in fp32 in some fixed order (k - 1 additions; a term passes through at most k - 1 of them).  By the standard analysis of recursive
summation the computed value differs from the exact sum S by at most gamma(k) * A for ANY order, A = the sum of the terms' absolute values and
gamma(m) = m u / (1 - m u); the test allows gamma(k + 1) * A.  The fp64 twin's own error (2^-53 relative per term) is 2^-29 of that and is ignored."""
import numpy as np

U = 2.0 ** -24


def gamma(m):
    m = np.asarray(m, np.float64)
    return m * U / (1.0 - m * U)


def corners_and_weights(pos, pos_min, pos_voxel, ds_rate, H, W):
    """pos (N, 2) fp32 [x-like, y-like] -> (x0, x1, y0, y1 int64 clamped corners; wa, wb, wc, wd fp32) with the forward's fp32 operation order."""
    f = np.float32
    pos = np.asarray(pos, f)
    inv_ds = f(1.0) / f(ds_rate)
    with np.errstate(all="ignore"):
        x = ((pos[:, 0] - f(pos_min[0])) / f(pos_voxel[0])) * inv_ds
        y = ((pos[:, 1] - f(pos_min[1])) / f(pos_voxel[1])) * inv_ds
    assert x.dtype == f and y.dtype == f
    fx, fy = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    x0, x1 = np.clip(fx, 0, W - 1), np.clip(fx + 1, 0, W - 1)
    y0, y1 = np.clip(fy, 0, H - 1), np.clip(fy + 1, 0, H - 1)
    wa = (x1.astype(f) - x) * (y1.astype(f) - y)
    wb = (x1.astype(f) - x) * (y - y0.astype(f))
    wc = (x - x0.astype(f)) * (y1.astype(f) - y)
    wd = (x - x0.astype(f)) * (y - y0.astype(f))
    assert wa.dtype == f
    return x0, x1, y0, y1, wa, wb, wc, wd


def grad_image(grad_out, image_shape, pos, pos_min, pos_voxel, image_index, ds_rate):
    """grad_out (N, C); image_shape (B, C, H, W); image_index (N) = cell_coords[unq_inv][:, 0] -> (S, A, k): the fp64 sum per cell and channel
    (B, C, H, W), the sum of the absolute terms (B, C, H, W) and the number of terms per cell (B, H, W)."""
    B, C, H, W = image_shape
    g = np.asarray(grad_out, np.float64)
    b = np.asarray(image_index, np.int64)
    x0, x1, y0, y1, wa, wb, wc, wd = corners_and_weights(pos, pos_min, pos_voxel, ds_rate, H, W)
    ok = (b >= 0) & (b < B)
    S = np.zeros((B * H * W, C), np.float64)
    A = np.zeros((B * H * W, C), np.float64)
    k = np.zeros((B * H * W,), np.int64)
    for yy, xx, w in ((y0, x0, wa), (y1, x0, wb), (y0, x1, wc), (y1, x1, wd)):
        cell = ((b * H + yy) * W + xx)[ok]
        t = w.astype(np.float64)[ok, None] * g[ok]
        np.add.at(S, cell, t)
        np.add.at(A, cell, np.abs(t))
        np.add.at(k, cell, 1)
    to = lambda a: np.ascontiguousarray(a.reshape(B, H, W, C).transpose(0, 3, 1, 2))  # noqa: E731
    return to(S), to(A), k.reshape(B, H, W)


def check(got, S, A, k, what=""):
    """Asserts |got - S| <= gamma(k + 1) * A everywhere and exact +0 where a cell has no term; returns the worst ratio to the bound."""
    got = np.asarray(got)
    assert got.shape == S.shape, (got.shape, S.shape)
    kk = np.broadcast_to(k[:, None], S.shape)
    empty = kk == 0
    assert not np.any(got[empty] != 0) and not np.any(np.signbit(got[empty])), f"{what}: a cell without a term is not +0"
    bound = gamma(kk + 1) * A
    err = np.abs(got.astype(np.float64) - S)
    assert np.all(np.isfinite(got)), f"{what}: non-finite gradient"
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)))) if got.size else 0.0
    print(f"[{what}] worst |got - S| / bound = {ratio:.3f} over {int((k > 0).sum())} cells with terms, at most {int(k.max()) if k.size else 0} terms per cell")
    assert ratio <= 1.0, f"{what}: {ratio:.3f} of the bound gamma(k + 1) * sum|terms|"
    return ratio
