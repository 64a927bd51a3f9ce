"""Yardsticks of the multi-view reader's point kernels: numpy twins of pnx_pfn_layer_eval, the forward of pnx_bilinear_gather and pnx_scatter_max /
pnx_scatter_max_backward, the bounds they are compared under, and the seeded inputs that tests/test_mvf_point_ref_cpu.py (no GPU) and
tests/test_gpu_mvf_point_kernels.py share.  numpy only; gamma and the corners / weights come from tests/mvf_bilinear_ref.py.

pfn_layer -- bound (derived, not measured).  k_pfn_layer evaluates, per point and output channel, acc = shift; acc = fma(x_k, w_k, acc) for k = 0 .. cin - 1
in that order: cin fused multiply-adds, one rounding each (relative error <= u = 2^-24).  With s_0 = shift and s_k = fl(s_(k-1) + x_k w_k) =
(s_(k-1) + x_k w_k)(1 + d_k), |d_k| <= u, the start value passes through cin roundings and term k through cin - k + 1 <= cin of them, so
    |acc - S| <= gamma(cin) A <= gamma(cin + 1) A,       S = shift + sum_k x_k w_k,   A = |shift| + sum_k |x_k w_k|,   gamma(m) = m u / (1 - m u).
The extra unit covers an evaluation that rounds the product and the sum separately (multiply, then add: cin + 1 roundings on a term), in ANY order of
the terms -- which is what test_mvf_point_ref_cpu.py runs in fp32 numpy, forward and reversed, to show that the bound is met by a plain fp32 chain.
relu is 1-Lipschitz, so |y - relu(S)| <= the same bound; where S < -bound the accumulator is negative and y is exactly +0.  max is 1-Lipschitz in the
maximum norm, so |gmax[g] - max_p relu(S_p)| <= the largest bound among the points p of cell g; a cell without a point is exactly +0 (the kernel's memset:
below every ReLU output, and the unsigned atomicMax on bit patterns orders non-negative floats as their values).  The fp64 evaluation's own error
(2^-53 per operation) is 2^-29 of the bound and is ignored.

gather -- k_bilinear's result bit for bit: four products image[corner] * weight, each rounded once (__fmul_rn), added as a, + b, + c, + d (__fadd_rn; nothing
contracts), on the corners and fp32 weights of mvf_bilinear_ref.corners_and_weights.  A bf16 / fp16 map enters as its exact values in fp32 (the kernel's
loads widen exactly).  Rows whose image index is outside [0, B) are +0.  Beside it the fp64 sum S of the four exact products and A = sum |terms|: four
roundings of the products and three additions give |out - S| <= gamma(4) A <= gamma(5) A in any order.

scatter_max -- exact: the maximum per pillar and channel and the LOWEST row that attains it (k_sm_max's tie rule, which is what makes the argmax
independent of the order in which the rows reached the pillar's list); the value is the one stored in that row, so a tie between +0 and -0 is decided
too.  Rows whose index is outside [0, P) take no part; a pillar without a row gives 0 and argmax n.  Inputs are finite or -inf (NaN is unspecified)."""
import numpy as np
from mvf_bilinear_ref import corners_and_weights, gamma

F32 = np.float32


# ------------------------------------------------------------------------------------------------ pnx_pfn_layer_eval
def pfn_layer(xa, gb, inv, wt, shift, num_groups):
    """xa (N, ca) fp32, gb (G, cb) fp32 or None, inv (N) cell of each point (None: no gb, no maximum), wt (ca + cb, cout), shift (cout) -> (S, A), fp64
    (N, cout): the pre-activation and the sum of the absolute values of its terms."""
    x = np.asarray(xa, np.float64)
    if gb is not None and np.asarray(gb).shape[1] > 0:
        g = np.asarray(gb, np.float64)
        assert g.shape[0] == num_groups
        x = np.concatenate([x, g[np.asarray(inv, np.int64)]], axis=1)
    w, s = np.asarray(wt, np.float64), np.asarray(shift, np.float64)
    assert x.shape[1] == w.shape[0] and s.shape == (w.shape[1],)
    return s[None, :] + x @ w, np.abs(s)[None, :] + np.abs(x) @ np.abs(w)


def pfn_bound(A, cin):
    return gamma(cin + 1) * A


def _ratio(err, bound):
    if err.size == 0:
        return 0.0
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))


def pfn_check(y, gmax, S, A, inv, num_groups, cin, what=""):
    """Asserts the bounds of the module docstring on y (N, cout) or None and gmax (G, cout) or None; returns the worst |err| / bound of (y, gmax)."""
    bound = pfn_bound(A, cin)
    want = np.maximum(S, 0.0)
    ry = rg = 0.0
    if y is not None:
        y = np.asarray(y)
        assert y.shape == S.shape and y.dtype == F32 and np.all(np.isfinite(y)), what
        assert not np.any(np.signbit(y)), f"{what}: a sign bit in y"
        ry = _ratio(np.abs(y.astype(np.float64) - want), bound)
        assert ry <= 1.0, f"{what}: y at {ry:.3f} of gamma(cin + 1) * A"
        assert not np.any(y[S < -bound] != 0), f"{what}: y is not 0 where the pre-activation is negative beyond the bound"
    if gmax is not None:
        gmax = np.asarray(gmax)
        assert gmax.shape == (num_groups, S.shape[1]) and gmax.dtype == F32 and np.all(np.isfinite(gmax)), what
        assert not np.any(np.signbit(gmax)), f"{what}: a sign bit in gmax"
        inv = np.asarray(inv, np.int64)
        wmax, bmax = np.zeros(gmax.shape), np.zeros(gmax.shape)
        np.maximum.at(wmax, inv, want)
        np.maximum.at(bmax, inv, bound)
        empty = np.bincount(inv, minlength=num_groups) == 0
        assert not np.any(gmax[empty].view(np.uint32)), f"{what}: a cell without a point is not +0"
        rg = _ratio(np.abs(gmax.astype(np.float64) - wmax), bmax)
        assert rg <= 1.0, f"{what}: gmax at {rg:.3f} of the largest bound among the cell's points"
    print(f"[{what}] worst |err| / bound: y {ry:.3f}, gmax {rg:.3f} ({S.shape[0]} points, {num_groups} cells, {cin} -> {S.shape[1]})")
    return max(ry, rg)


def cell_max_of(y, inv, num_groups):
    """The per-cell maximum of stored (non-negative) outputs, exactly: what gmax must equal bit for bit."""
    m = np.zeros((num_groups, y.shape[1]), F32)
    np.maximum.at(m, np.asarray(inv, np.int64), y)
    return m


def pfn_chain_f32(xa, gb, inv, wt, shift, reverse=False):
    """A plain fp32 evaluation of the layer: the product and the sum rounded separately, the terms in forward or reversed order -> (y, pre-activation)."""
    x = np.asarray(xa, F32)
    if gb is not None and np.asarray(gb).shape[1] > 0:
        x = np.concatenate([x, np.asarray(gb, F32)[np.asarray(inv, np.int64)]], axis=1)
    w = np.asarray(wt, F32)
    acc = np.broadcast_to(np.asarray(shift, F32)[None, :], (x.shape[0], w.shape[1])).copy()
    for k in (range(x.shape[1] - 1, -1, -1) if reverse else range(x.shape[1])):
        acc = acc + x[:, k:k + 1] * w[k][None, :]
    assert acc.dtype == F32
    return np.where(acc > 0, acc, F32(0)), acc


# (ca, cb, cout) beside the config's two layers ("config": 20 -> 24, then [24 | 24] -> 48 without the per-point store)
PFN_WIDTHS = {"1_out": (10, 0, 1), "cin_64": (64, 0, 64), "cin_65": (65, 0, 65), "seam": (40, 60, 130), "lds_64k": (128, 0, 128)}
PFN_CONFIG = (20, 0, 24)
PFN_SIZES = (0, 1, 63, 7001)
PFN_STRIDE_LOOP = 32_773          # more points than the 16 384 waves of the largest grid: the wave-stride loop iterates
PFN_XA_OFFSET, PFN_XA_PAD = 3, 7  # xa = columns [3, 3 + ca) of a (N, ca + 7) buffer


def pfn_layout(n, rng):
    """(inv (n) unsorted, G, cells that stay empty, the cell of the planted rows or None).  From 63 points on the first, a middle and the last cell are
    empty; from 7001 points on one cell holds 5 000 of them."""
    if n <= 1:
        return np.full((n,), 2, np.int64), 5, [g for g in range(5) if n == 0 or g != 2], None
    G = 40 if n < 5000 else 301 + n // 40
    empty = [0, G // 2, G - 1]
    gz, big = 9, 7
    nbig = 5000 if n >= 7001 else 0
    free = np.setdiff1d(np.arange(G), empty + [gz] + ([big] if nbig else []))
    planted = 4                                                           # rows 0 .. 3 go to cell gz, which holds nothing else
    rest = n - planted - nbig
    inv = np.concatenate([np.full((nbig,), big), free[np.arange(min(rest, len(free)))], rng.choice(free, max(rest - len(free), 0))]).astype(np.int64)
    rng.shuffle(inv)
    return np.concatenate([np.full((planted,), gz, np.int64), inv]), G, empty, gz


def pfn_params(cin, cout, rng):
    """(wt (cin, cout) = the folded weight transposed, shift (cout)); with two channels or more the last one has shift -1000."""
    wt = (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(F32)
    shift = (rng.standard_normal((cout,)) * 0.3).astype(F32)
    if cout >= 2:
        shift[cout - 1] = -1000.0
    return wt, shift


def pfn_inputs(ca, cb, cout, n, seed, planted=True):
    """Seeded inputs of one layer: dict(wide, xa (a column slice of wide), gb, inv, wt, shift, G, empty, zero_rows).  Planted, when the widths allow:
      channel cout - 1 (cout >= 2): shift -1000, so every pre-activation is negative;
      channel 0: shift -0.0 and only negative weights, rows 0 and 1 all zero in a cell whose gb row is zero: every product is -0, the pre-activation is -0.0;
      channel 1 (cout >= 3): shift = -wt[0, 1], row 2 = the first unit vector: fma(1, w, -w) is exactly 0 although A = 2 |w|."""
    rng = np.random.default_rng(seed)
    cin = ca + cb
    inv, G, empty, gz = pfn_layout(n, rng)
    wide = rng.standard_normal((n, ca + PFN_XA_PAD)).astype(F32)
    gb = rng.standard_normal((G, cb)).astype(F32) if cb else None
    wt, shift = pfn_params(cin, cout, rng)
    zero_rows = np.zeros((0,), np.int64)
    if planted and gz is not None:
        wt[:, 0] = -np.abs(wt[:, 0]) - F32(1e-3)
        shift[0] = -0.0
        wide[:3, PFN_XA_OFFSET:PFN_XA_OFFSET + ca] = 0.0
        wide[2, PFN_XA_OFFSET] = 1.0
        if cout >= 3:
            shift[1] = -wt[0, 1]
        if gb is not None:
            gb[gz] = 0.0
        zero_rows = np.array([0, 1], np.int64)
    xa = wide[:, PFN_XA_OFFSET:PFN_XA_OFFSET + ca]
    return dict(wide=wide, xa=xa, gb=gb, inv=inv, wt=wt, shift=shift, G=G, empty=empty, zero_rows=zero_rows, cin=cin)


def pfn_case(name, n):
    """The inputs of case (name, n) of both test files: name in PFN_WIDTHS, or "config" (layer 0; layer 1 takes pfn_layer1_params())."""
    ca, cb, cout = PFN_CONFIG if name == "config" else PFN_WIDTHS[name]
    return pfn_inputs(ca, cb, cout, n, seed=1000 * (1 + sorted(PFN_WIDTHS).index(name) if name != "config" else 0) + n)


def pfn_layer1_params():
    return pfn_params(48, 48, np.random.default_rng(77))


def pfn_cases():
    """(name, n): every width at 0, 1, 63 and 7001 points; the config's widths also past the largest grid."""
    return [(name, n) for name in PFN_WIDTHS for n in PFN_SIZES] + [("config", n) for n in PFN_SIZES + (PFN_STRIDE_LOOP,)]


# ------------------------------------------------------------------------------------------------ pnx_bilinear_gather, forward
def gather(image, pos, pos_min, pos_voxel, image_index, ds_rate):
    """image (B, C, H, W) fp32 (a 16-bit map: its exact values); pos (N, 2) fp32; image_index (N) = cell_coords[unq_inv][:, 0] -> (out fp32 (N, C): the
    kernel's bits; S, A fp64 (N, C): the exact sum of the four products and the sum of their absolute values)."""
    img = np.asarray(image)
    assert img.dtype == F32 and img.ndim == 4
    B, C, H, W = img.shape
    hwc = img.transpose(0, 2, 3, 1)
    x0, x1, y0, y1, wa, wb, wc, wd = corners_and_weights(pos, pos_min, pos_voxel, ds_rate, H, W)
    b = np.asarray(image_index, np.int64)
    ok = (b >= 0) & (b < B)
    bb = np.where(ok, b, 0)
    n = len(b)
    out, S, A = None, np.zeros((n, C)), np.zeros((n, C))
    for yy, xx, w in ((y0, x0, wa), (y1, x0, wb), (y0, x1, wc), (y1, x1, wd)):
        v = hwc[bb, yy, xx]
        t = v * w[:, None]                                # fp32, rounded once
        out = t if out is None else out + t               # a, + b, + c, + d
        t64 = v.astype(np.float64) * w.astype(np.float64)[:, None]
        S += t64
        A += np.abs(t64)
    assert out.dtype == F32
    out[~ok], S[~ok], A[~ok] = F32(0), 0.0, 0.0
    return out, S, A


def gather_check(got, out, S, A, image_index, B, what=""):
    """got equals the twin bit for bit, lies within gamma(5) * A of S, and is +0 in the rows outside the batch; returns the worst |err| / bound."""
    got = np.asarray(got)
    assert got.shape == out.shape and got.dtype == F32, (what, got.shape, out.shape)
    b = np.asarray(image_index, np.int64)
    outside = (b < 0) | (b >= B)
    assert not np.any(got[outside].view(np.uint32)), f"{what}: a row outside the batch is not +0"
    r = _ratio(np.abs(got.astype(np.float64) - S), gamma(5) * A)
    print(f"[{what}] worst |out - S| / (gamma(5) * sum|terms|) = {r:.3f}; {int(outside.sum())} of {len(b)} rows outside the batch")
    assert r <= 1.0, f"{what}: {r:.3f} of gamma(5) * sum|terms|"
    diff = got.view(np.uint32) != out.view(np.uint32)
    assert not np.any(diff), f"{what}: {int(diff.sum())} of {diff.size} elements differ from the twin's bits, first at {np.argwhere(diff)[0]}"
    return r


# ------------------------------------------------------------------------------------------------ pnx_scatter_max and its backward
def scatter_max(x, index, P):
    """x (n, C) fp32, index (n) int64 -> (out (P, C) fp32, argmax (P, C) int64)."""
    x = np.asarray(x)
    assert x.dtype == F32 and x.ndim == 2
    n, C = x.shape
    index = np.asarray(index, np.int64)
    out, arg = np.zeros((P, C), F32), np.full((P, C), n, np.int64)
    rows = np.nonzero((index >= 0) & (index < P))[0]
    if len(rows) == 0:
        return out, arg
    order = rows[np.argsort(index[rows], kind="stable")]              # grouped by pillar, ascending row inside a pillar
    key = index[order]
    starts = np.nonzero(np.r_[True, key[1:] != key[:-1]])[0]
    seg = np.cumsum(np.r_[False, key[1:] != key[:-1]])
    xs = x[order]
    with np.errstate(invalid="ignore"):
        mx = np.maximum.reduceat(xs, starts, axis=0)
    first = np.minimum.reduceat(np.where(xs == mx[seg], np.arange(len(order))[:, None], len(order)), starts, axis=0)   # first = lowest row at the maximum
    assert first.max() < len(order)
    pillars = key[starts]
    arg[pillars] = order[first]
    out[pillars] = np.take_along_axis(x, arg[pillars], axis=0)
    return out, arg


def scatter_max_backward(g, arg, n):
    """g (P, C) routed to the argmax rows; every other element +0."""
    g = np.asarray(g, F32)
    P, C = g.shape
    gx = np.zeros((n, C), F32)
    has = arg < n
    gx[arg[has], np.broadcast_to(np.arange(C)[None, :], arg.shape)[has]] = g[has]
    return gx


SM_CHANNELS, SM_PILLARS, SM_ROWS = (1, 48, 64, 65, 256), (1, 2049, 4100), (0, 1, 20_000)


def scatter_inputs(n, C, P, seed):
    """Values on multiples of 0.25 in [-2, 2] (ties in most pillars, +0 and -0 among them), unsorted indices; with more than one pillar: 2047 and 2048 (the seam of
    two scan blocks) without a row, one pillar of 5 000 rows, pillars 3 .. 40 all negative and 41 .. 60 all -inf, and a sixteenth of the rows with an
    index of -1, P or 2^40."""
    rng = np.random.default_rng(seed)
    x = np.clip(np.round(rng.standard_normal((n, C)) * 4.0) / 4.0, -2.0, 2.0).astype(F32)
    if P == 1:
        index = np.zeros((n,), np.int64)
    else:
        free = np.setdiff1d(np.arange(P), [2047, 2048, 5])
        nbig = 5000 if n >= 20_000 else 0
        index = np.concatenate([np.full((nbig,), 5), rng.choice(free, n - nbig)]).astype(np.int64)
        rng.shuffle(index)
        x[(index >= 3) & (index <= 40) & (index != 5)] = -np.abs(x[(index >= 3) & (index <= 40) & (index != 5)]) - F32(0.25)
        x[(index >= 41) & (index <= 60)] = -np.inf
    if n > 1:
        bad = rng.choice(n, n // 16, replace=False)
        index[bad] = np.array([-1, P, 1 << 40], np.int64)[np.arange(len(bad)) % 3]
    return x, index
