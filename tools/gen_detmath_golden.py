#!/usr/bin/env python3
"""gen_detmath_golden.py -- writes tests/golden/detmath_cases.npz: arguments for csrc/pnx_detmath.h's sin / cos / atan2 and the CORRECTLY ROUNDED fp32
value of each, from mpmath at 256 bits.  Only this generator needs mpmath; the tests read the fixture (and re-derive a sample where mpmath is there).

The list is fixed (seeded numpy), so are the expectations.  `hard_*` name the results that lie within HARD_ULP of the midpoint of two fp32 neighbours:
a routine that rounds an fp64 value (abs err < 1e-15) once more to fp32 may legitimately land on the other neighbour there, with an error of
0.5 + that distance ulp, and nowhere else.

    python tools/gen_detmath_golden.py            # writes the fixture
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "detmath_cases.npz")
LIMIT = 1.0e9          # pnx_detmath.h: |a| >= LIMIT (or non-finite) gives NaN; below it sin / cos are correctly rounded.  float32(1e9) is exact.
HARD_ULP = 1.0e-7      # a result this close (in ulp) to a rounding boundary is a hard rounding case
PREC = 256
f32 = np.float32


def _neighbours(v, n=2):
    """v and its n fp32 neighbours on either side."""
    out = [f32(v)]
    lo = hi = f32(v)
    for _ in range(n):
        lo, hi = np.nextafter(lo, f32(-np.inf)), np.nextafter(hi, f32(np.inf))
        out += [lo, hi]
    return out


def sincos_args():
    """fp32 arguments of sin / cos (numpy only, deterministic)."""
    rng = np.random.default_rng(20250)
    a = []
    for d in range(-45, 9):                                   # dense per decade, 1e-45 .. LIMIT, both signs
        v = 10.0 ** (d + rng.uniform(0, 1, 100))
        a.append((v * rng.choice([-1.0, 1.0], 100)).astype(f32))
    for lo, hi, n in ((1e6, 1e7, 1000), (1e7, 1e8, 1000), (1e8, 9.9e8, 1500), (1.6e6, 1.7e6, 500)):  # where the 3-term reduction was inexact; its seam
        a.append((rng.uniform(lo, hi, n) * rng.choice([-1.0, 1.0], n)).astype(f32))
    half_pi = math.pi / 2
    ks = list(range(-2000, 2001)) + [s * ((1 << 20) + j) for s in (-1, 1) for j in range(-8, 9)] + \
        [s * k for s in (-1, 1) for k in (1 << 22, 1 << 25, 1 << 28, 636619000)]
    a.append(np.asarray([x for k in ks for x in _neighbours(f32(k * half_pi))], f32))       # every fp32 within 2 ulp of k pi/2
    tiny, sub_max, norm_min = f32(1e-45), np.nextafter(f32(1.17549435e-38), f32(0)), f32(1.17549435e-38)
    edge = [0.0, -0.0, tiny, -tiny, sub_max, -sub_max, norm_min, -norm_min, f32(3e-42), f32(-7e-40), np.inf, -np.inf, np.nan]
    edge += _neighbours(f32(LIMIT)) + [-x for x in _neighbours(f32(LIMIT))] + [f32(2e9), f32(-3e38)]
    a.append(np.asarray(edge, f32))
    return np.concatenate(a)


def atan2_args():
    """fp32 (y, x) pairs of atan2 (numpy only, deterministic)."""
    rng = np.random.default_rng(20251)
    sp = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 1e-45, -1e-45, 1e-40, -1e-40, 1e20, -1e20, 3.4e38, -3.4e38, 0.5, -2.0]
    y = [p for p in sp for _ in sp]                            # every signed-zero / inf / NaN / denormal / axis combination
    x = [q for _ in sp for q in sp]
    n = 4000                                                   # exponents across +-20 decades
    y += list(10.0 ** rng.uniform(-20, 20, n) * rng.choice([-1.0, 1.0], n))
    x += list(10.0 ** rng.uniform(-20, 20, n) * rng.choice([-1.0, 1.0], n))
    n = 2000                                                   # ordinary ratios: the polygon's vertex angles
    y += list(rng.normal(0, 3, n))
    x += list(rng.normal(0, 3, n))
    for ratio in (math.tan(math.pi / 8), 1.0):                 # the branch at 0.41421356..., and mx == mn
        for _ in range(150):
            big = f32(10.0 ** rng.uniform(-3, 3))
            for small in _neighbours(f32(float(big) * ratio), 4):
                sy, sx = rng.choice([-1.0, 1.0], 2)
                if rng.uniform() < 0.5:
                    y.append(sy * small), x.append(sx * big)
                else:
                    y.append(sy * big), x.append(sx * small)
    for v in (1e-45, 1e-30, 1e-7, 1.0, 1e10, 3e38):            # y = +-0 and y tiny against x < 0: +-pi
        for yy in (0.0, -0.0, 1e-45, -1e-45, 1e-38, -1e-38):
            y.append(yy), x.append(-v)
    return np.asarray(y, f32), np.asarray(x, f32)


def round32(v):
    """(correctly rounded fp32 of the mpmath value v, distance of v from the nearest rounding boundary in ulp)."""
    import mpmath as mp

    c = f32(float(v))
    cands = [c, np.nextafter(c, f32(-np.inf)), np.nextafter(c, f32(np.inf))]
    cands = [k for k in cands if np.isfinite(k)]
    d = sorted((abs(mp.mpf(float(k)) - v), i) for i, k in enumerate(cands))
    best, second = cands[d[0][1]], cands[d[1][1]]
    ulp = abs(mp.mpf(float(best)) - mp.mpf(float(second)))
    return best, float((d[1][0] - d[0][0]) / (2 * ulp))


def expect_sincos(a):
    import mpmath as mp

    mp.mp.prec = PREC
    s, c, ds, dc = np.empty_like(a), np.empty_like(a), np.full(a.shape, 0.5), np.full(a.shape, 0.5)
    for i, v in enumerate(a):
        if not np.isfinite(v) or abs(float(v)) >= LIMIT:
            s[i] = c[i] = np.nan
        elif v == 0:
            s[i], c[i] = v, 1.0                                # sin keeps the zero's sign, as IEEE / libm
        else:
            s[i], ds[i] = round32(mp.sin(mp.mpf(float(v))))
            c[i], dc[i] = round32(mp.cos(mp.mpf(float(v))))
    return s, c, ds, dc


def expect_atan2(y, x):
    import mpmath as mp

    mp.mp.prec = PREC
    r, dr = np.empty_like(y), np.full(y.shape, 0.5)
    for i, (p, q) in enumerate(zip(y, x)):
        if np.isnan(p) or np.isnan(q):
            r[i] = np.nan
        elif p == 0 or q == 0 or np.isinf(p) or np.isinf(q):   # IEEE 754 atan2's table: 0, +-pi/4, +-pi/2, +-3pi/4, +-pi with the zero's sign
            r[i] = f32(math.atan2(float(p), float(q)))
        else:
            r[i], dr[i] = round32(mp.atan2(mp.mpf(float(p)), mp.mpf(float(q))))
    return r, dr


def main():
    a = sincos_args()
    y, x = atan2_args()
    s, c, ds, dc = expect_sincos(a)
    r, dr = expect_atan2(y, x)
    kind, index, err = [], [], []
    for k, d in enumerate((ds, dc, dr)):                       # kind 0 = sin, 1 = cos, 2 = atan2
        for i in np.nonzero(d < HARD_ULP)[0]:
            kind.append(k), index.append(i), err.append(0.5 + d[i])
    np.savez_compressed(OUT, limit=np.float64(LIMIT), sc_a=a, sc_sin=s, sc_cos=c, at_y=y, at_x=x, at_r=r, hard_kind=np.asarray(kind, np.int32),
                        hard_index=np.asarray(index, np.int64), hard_err_ulp=np.asarray(err, np.float64))
    print(f"[detmath] {len(a)} sin/cos arguments, {len(y)} atan2 pairs, {len(kind)} hard rounding cases {list(zip(kind, index, err))}; "
          f"closest to a boundary: sin {ds.min():.3g} cos {dc.min():.3g} atan2 {dr.min():.3g} ulp; {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    sys.exit(main())
