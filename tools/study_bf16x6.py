#!/usr/bin/env python3
"""Numerical study (CPU, numpy; no GPU): the fp32 training graph's 3x3 convolution on three bf16 pieces per operand (PNX_TRAIN_F32_PIECES=3,
pnx_conv3x3_x6) against fp64.  Emulates the split (hi = RNE(x), mid = RNE(x - hi), lo = RNE(x - hi - mid)), the six products of piece orders 0..2 and
the kernel's fp32 accumulation in its order -- per 64-channel slab the pieces x_lo (W_hi), x_mid (W_mid, W_hi), x_hi (W_lo, W_mid, W_hi), each pass
a 9-tap x 4-k-step walk of 16-channel MFMA blocks whose 16 products are summed exactly and added to the fp32 accumulator -- beside the three-product
node (pnx_conv3x3_x3) and a plain fp32 dot product, on random operands of the test shapes (tests/test_gpu_fp32_six_products.py).  Prints the relative
Frobenius error and the largest error over 2^-19 of the sum of |terms| (the test's elementwise bar: <= 1 passes).

  python tools/study_bf16x6.py [n_outputs]"""
import sys

import numpy as np


def bf16(x):
    """round-to-nearest-even fp32 -> bf16 -> fp32 (finite values)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split(x, n):
    x = np.asarray(x, np.float32)
    out, r = [], x
    for _ in range(n):
        p = bf16(r)
        out.append(p)
        r = (r - p).astype(np.float32)
    return out


def accumulate(x, w, plan, acc0=None):
    """x (N, K), w (K,) as pieces; plan: list of (x piece, w piece) per slab in kernel order.  K = 9 taps x cin; a slab = 64 channels x 9 taps,
    walked as 36 k-steps of 16 products (summed exactly in fp64, then one fp32 add -- the MFMA's inner sum is exact for bf16 inputs)."""
    N, K = x[0].shape
    cin = K // 9
    acc = np.zeros(N, np.float32) if acc0 is None else acc0
    for slab in range(cin // 64):
        for xi, wi in plan:
            for tap in range(9):
                for kk in range(4):
                    c0 = tap * cin + slab * 64 + kk * 16
                    part = x[xi][:, c0:c0 + 16].astype(np.float64) @ w[wi][c0:c0 + 16].astype(np.float64)
                    acc = (acc + part.astype(np.float32)).astype(np.float32)
    return acc


PLAN6 = [(2, 0), (1, 1), (1, 0), (0, 2), (0, 1), (0, 0)]   # (x piece, W piece): 0 hi, 1 mid, 2 lo -- x_lo W_hi first, x_hi W_hi last
PLAN3 = [(0, 0), (0, 1), (1, 0)]                           # pnx_conv3x3_x3: x_hi (W_hi, W_lo), then x_lo W_hi


def study(cin, n, rng, x_scale=1.0):
    K = 9 * cin
    x = (rng.standard_normal((n, K)) * x_scale).astype(np.float32)
    w = (rng.standard_normal(K) * np.sqrt(2.0 / K)).astype(np.float32)
    ref = x.astype(np.float64) @ w.astype(np.float64)
    absum = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64))
    res = {}
    # the slab order of the kernels: slabs outer, pieces inner, as accumulate() walks them
    res["bf16 x6 (pnx_conv3x3_x6)"] = accumulate(split(x, 3), split(w, 3), PLAN6)
    res["bf16 x3 (pnx_conv3x3_x3)"] = accumulate(split(x, 2), split(w, 2), PLAN3)
    fp32 = np.zeros(n, np.float32)
    for k in range(K):   # a sequential fp32 dot product (what a direct fp32 kernel does, up to order)
        fp32 = (fp32 + (x[:, k] * w[k]).astype(np.float32)).astype(np.float32)
    res["fp32 sequential"] = fp32
    out = []
    for name, y in res.items():
        err = np.abs(y.astype(np.float64) - ref)
        out.append((name, float(np.linalg.norm(err) / np.linalg.norm(ref)), float((err / (2.0 ** -19 * absum)).max())))
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    rng = np.random.default_rng(0)
    print(f"{n} outputs per case; bars of the GPU test: relative Frobenius <= 1e-6, elementwise err / (2^-19 sum|terms|) <= 1")
    for cin in (64, 128, 256):
        for xs in (1.0, 2.0 ** -60, 2.0 ** 40):
            for name, fro, elt in study(cin, n, rng, xs):
                print(f"  K = 9 x {cin:3d}, |x| ~ 2^{int(np.log2(xs)):+d}  {name:26s} relative Frobenius {fro:.2e}   max err / (2^-19 sum|terms|) {elt:.3f}")


if __name__ == "__main__":
    main()
