"""The exact twin of csrc/merge.hip (numpy only).  It restates the KERNEL, not the reference: the library is built with -ffp-contract=off, so
k_merge_flags / k_merge_write evaluate one fixed IEEE expression per coordinate,

    x' = fp32(((t[4r] * x + t[4r+1] * y) + t[4r+2] * z) + t[4r+3])        every product and sum rounded to fp64, in that order,

and elementwise numpy in fp64 performs the same roundings: the twin is held to bit equality with the device (tests/test_gpu_merge_seams.py) and to
<= 1 ulp of fp32 with the reference's BLAS dot, whose summation order is not fixed (tests/test_merge_ref_cpu.py).  Shared helpers of the two test
modules (inputs, planted cases, comparisons) live here as well, so that the CPU test shows the twin alone meets what the GPU test asks."""
import numpy as np

F32 = np.float32
SCAN_ITEMS = 2048          # PNX_SCAN_ITEMS: rows per level-1 scan block
SCAN_BLOCK = 256           # kBlock: block totals handled per pass of the level-2 carry loop


def transform_rows(T, xyz):
    """(n, 3) fp32 -> (n, 3) fp32 through the rows of the 3x4 [R | t] in fp64, in the kernel's order of operations."""
    T = np.asarray(T, np.float64)[:3, :4]
    x, y, z = (xyz[:, k].astype(np.float64) for k in range(3))
    out = np.empty((len(xyz), 3), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            out[:, r] = (((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(F32)
    return out


def merge(raw, segments, n_copy):
    """raw (n_raw, C >= n_copy) fp32, segments as io.pack_segments takes them -> (out (n_raw, n_copy + 2) fp32, n_out)."""
    raw = np.asarray(raw)
    assert raw.dtype == F32 and raw.ndim == 2 and 3 <= n_copy <= raw.shape[1]
    n = len(raw)
    out = np.zeros((n, n_copy + 2), F32)
    rows = []
    for s in segments:
        p = raw[int(s["begin"]):int(s["end"])]
        T = s.get("transform")
        xyz = p[:, :3].copy() if T is None else transform_rows(T, p[:, :3])
        r = F32(s.get("radius", 0.0))
        keep = np.ones(len(p), bool)
        if r > 0:
            with np.errstate(invalid="ignore"):
                keep = ~((np.abs(xyz[:, 0]) < r) & (np.abs(xyz[:, 1]) < r))         # NaN fails the comparison: kept
        m = np.empty((int(keep.sum()), n_copy + 2), F32)
        m[:, 0] = F32(int(s["batch"]))
        m[:, 1:4] = xyz[keep]
        m[:, 4:1 + n_copy] = p[keep, 3:n_copy]
        m[:, 1 + n_copy] = F32(s["time"])
        rows.append(m)
    n_out = sum(len(m) for m in rows)
    if rows:
        out[:n_out] = np.concatenate(rows)
    out[n_out:, 0] = -1.0
    return out, n_out


def segments_of(sweeps):
    """oracle.merge_sweeps' list of sweeps -> (raw, segments) of the device form; narrower sweeps are padded with zero columns."""
    ncol = max(s["points"].shape[1] for s in sweeps)
    raw = np.concatenate([np.pad(s["points"], ((0, 0), (0, ncol - s["points"].shape[1]))) for s in sweeps]).astype(F32)
    segs, o = [], 0
    for s in sweeps:
        segs.append(dict(begin=o, end=o + len(s["points"]), batch=s["batch"], time=s["time"], radius=s["radius"], transform=s["transform"]))
        o += len(s["points"])
    return raw, segs


def ulp_distance(a, b):
    """Distance in units of the last place between two finite fp32 arrays (monotone integer mapping of the bit patterns)."""
    def key(v):
        i = np.ascontiguousarray(v, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def near_radius(raw, segments, ulps=2):
    """Number of transformed |x'| or |y'| of radius-filtered segments within `ulps` fp32 ulp of the radius: where the kept sets of two
    implementations that differ by 1 ulp in a coordinate may differ."""
    k = 0
    for s in segments:
        r = F32(s.get("radius", 0.0))
        if r > 0:
            p = raw[int(s["begin"]):int(s["end"]), :3]
            xyz = p if s.get("transform") is None else transform_rows(s["transform"], p)
            a = np.abs(xyz[:, :2])
            a = a[np.isfinite(a)]
            k += int((ulp_distance(a, np.full(a.shape, r, F32)) <= ulps).sum())
    return k


def assert_same_bits(got, want, what=""):
    """Whole-buffer comparison as uint32; where the twin holds a NaN in a transformed column (1 .. 3), the kernel need only hold a NaN there."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = got.view(np.uint32) == want.view(np.uint32)
    nan_ok = np.zeros(want.shape, bool)
    nan_ok[:, 1:4] = np.isnan(want[:, 1:4]) & np.isnan(got[:, 1:4])
    bad = ~(same | nan_ok)
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} words differ, first at row {r} column {c}: got {got[r]!r}, twin {want[r]!r}")


# ------------------------------------------------------------------------------------------------ the seeded nuScenes-like batch
def sample(rng, b, nsweeps, n_per, with_tf=True, radius=1.0):
    """One sample of `nsweeps` sweeps: a twentieth of the points near the ego vehicle, past sweeps rotated about z and translated."""
    sweeps = []
    for s in range(nsweeps):
        pts = np.empty((n_per + 17 * s, 5), F32)
        pts[:, :2] = rng.uniform(-40, 40, (len(pts), 2))
        pts[: len(pts) // 20, :2] = rng.uniform(-1.5, 1.5, (len(pts) // 20, 2))
        pts[:, 2] = rng.uniform(-3, 1, len(pts))
        pts[:, 3] = rng.uniform(0, 255, len(pts))
        pts[:, 4] = rng.integers(0, 32, len(pts))
        T = None
        if s > 0 and with_tf:
            a = 0.01 * s
            T = np.eye(4)
            T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
            T[:3, 3] = [0.4 * s, -0.1 * s, 0.02 * s]
        sweeps.append(dict(points=pts, batch=b, time=0.05 * s, radius=radius if s > 0 else 0.0, transform=T))
    return sweeps


def nuscenes_batch(seed=11, B=4, nsweeps=10, n_per=13_200):
    """4 x 10 sweeps, 531 060 rows: past 256 scan blocks."""
    rng = np.random.default_rng(seed)
    sweeps = []
    for b in range(B):
        sweeps += sample(rng, b, nsweeps, n_per)
    return sweeps


def contract_batch(seed=12):
    """Two samples of 5 sweeps each with the close-point radius on: the batch whose whole merged buffer, tail included, is fed to the readers."""
    rng = np.random.default_rng(seed)
    return sample(rng, 0, 5, 4000) + sample(rng, 1, 5, 3500)


# ------------------------------------------------------------------------------------------------ keep patterns over a buffer
def blocks_and_passes(n):
    """(level-1 scan blocks, passes of the level-2 carry loop) that an n-row merge takes."""
    nblk = -(-n // SCAN_ITEMS)
    return nblk, -(-nblk // SCAN_BLOCK)


def pattern_keep(n, seed=0):
    """A keep flag per row that varies across the buffer, repeating with a period of 7 scan blocks: seeded random, all dropped, all kept,
    alternating, only the first and last row kept, all dropped but row 1000, kept in runs of 8 (the vector width of k_scan_local)."""
    i = np.arange(n, dtype=np.int64)
    blk, j = i // SCAN_ITEMS, i % SCAN_ITEMS
    kind = blk % 7
    rnd = np.random.default_rng(seed).random(n) < 0.5
    keep = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5],
                     [rnd, np.zeros(n, bool), np.ones(n, bool), j % 2 == 1, (j == 0) | (j == SCAN_ITEMS - 1), j == 1000], (j // 8) % 2 == 0)
    return keep


def pattern_case(n, seed=0, shift=0):
    """Two segments over n rows (the first with radius 1 and a transform, the second with radius 2 and none), rows placed inside or outside the
    radius box after pattern_keep (rolled by `shift` rows).  Column 3 carries the row number, column 4 is not copied."""
    rng = np.random.default_rng(seed + 1)
    keep = np.roll(pattern_keep(n, seed), shift)
    cut = (2 * n) // 3 if n > 1 else 1
    T = np.eye(4)
    a = 0.3
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = [0.25, -0.125, 0.5]
    raw = np.empty((n, 5), F32)
    inside = rng.uniform(-0.6, 0.6, (n, 2))
    far = rng.uniform(3.0, 40.0, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
    target = np.where(keep[:, None], far, inside)                                 # where the row must land AFTER the transform
    back = (target[:cut] - T[:2, 3]) @ T[:2, :2]                                  # inverse rotation: rows of (R^T v)^T = v^T R
    raw[:cut, :2] = back
    raw[cut:, :2] = target[cut:]
    raw[:, 2] = rng.uniform(-3, 1, n)
    raw[:, 3] = np.arange(n) % 16_777_216
    raw[:, 4] = 12345.0
    segs = [dict(begin=0, end=cut, batch=0, time=0.25, radius=1.0, transform=T), dict(begin=cut, end=n, batch=1, time=0.5, radius=2.0, transform=None)]
    return raw, segs, keep


ROW_COUNTS = (1, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 524_287, 524_288, 524_289, 2 * 524_288 + 2049 + 5)


# ------------------------------------------------------------------------------------------------ planted radius cases
def prev32(r):
    return np.nextafter(F32(r), F32(0))


def radius_rows(r):
    """Planted (x, y) pairs and whether each row is KEPT under radius r: only rows with both |x| < r and |y| < r are dropped; NaN is kept."""
    r, p = F32(r), prev32(r)
    nan, inf = F32("nan"), F32("inf")
    rows = [((r, 0), True), ((-r, 0), True), ((0, r), True), ((0, -r), True),
            ((p, p), False), ((-p, p), False), ((p, -p), False), ((-p, -p), False),
            ((p, r), True), ((-0.0, 0.0), False), ((nan, 0), True), ((0, nan), True), ((inf, 0), True),
            ((0, 0), False), ((r, r), True)]
    xy = np.array([v for v, _ in rows], F32)
    return xy, np.array([k for _, k in rows], bool)


def radius_case(r):
    """An identity segment and a no-transform segment, both with radius r, over the planted rows.  Returns (raw (2m, 4), segments, kept (2m))."""
    xy, kept = radius_rows(r)
    m = len(xy)
    raw = np.zeros((2 * m, 4), F32)
    raw[:, :2] = np.concatenate([xy, xy])
    raw[:, 2] = 0.5
    raw[:, 3] = np.arange(2 * m)
    segs = [dict(begin=0, end=m, batch=0, time=0.0, radius=float(r), transform=np.eye(4)), dict(begin=m, end=2 * m, batch=1, time=1.0, radius=float(r), transform=None)]
    return raw, segs, np.concatenate([kept, kept])


def rounds_up_to_radius_case():
    """One translated segment: x = 0.5, t = 0.5 - 2^-26.  The fp64 sum 1 - 2^-26 is exact and lies under r = 1, but rounds to fp32(1.0) (the
    neighbours are 1 - 2^-24 and 1, and 1 - 2^-26 is nearer to 1): the row is kept, as in the reference, which compares the stored fp32 value.  A
    second row at x = 0.5 - 2^-24 gives 1 - 2^-24 - 2^-26, which rounds to 1 - 2^-24 (a quarter of the gap above it): dropped."""
    T = np.eye(4)
    T[0, 3] = 0.5 - 2.0 ** -26
    raw = np.zeros((2, 4), F32)
    raw[0, 0], raw[1, 0] = 0.5, F32(0.5) - F32(2.0 ** -24)
    raw[:, 3] = [7, 8]
    return raw, [dict(begin=0, end=2, batch=3, time=0.5, radius=1.0, transform=T)], np.array([True, False])


# ------------------------------------------------------------------------------------------------ segment layouts
def tagged_raw(n, seed, stride=5):
    rng = np.random.default_rng(seed)
    raw = np.empty((n, stride), F32)
    raw[:, :3] = rng.uniform(-40, 40, (n, 3))
    raw[:, 3:] = np.arange(n)[:, None] % 16_777_216
    return raw


def segments_from_lengths(lengths, seed=0, every_radius=3):
    """Contiguous segments of the given lengths, distinct (batch, time) per segment -- batch = s % 7 is not monotone, time = s / 4 is exact in fp32 --
    every third with radius 1, every second with a small rotation + translation."""
    segs, o = [], 0
    for s, ln in enumerate(lengths):
        T = None
        if s % 2 == 1:
            a = 0.001 * (s % 50)
            T = np.eye(4)
            T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
            T[:3, 3] = [0.01 * (s % 13), -0.02 * (s % 7), 0.0]
        segs.append(dict(begin=o, end=o + int(ln), batch=s % 7, time=0.25 * s, radius=1.0 if s % every_radius == 0 else 0.0, transform=T))
        o += int(ln)
    return segs, o


def segment_layouts():
    """name -> segment lengths.  'every residue': 2048 one-row segments put a boundary on every residue of 256 and of 2048 (and a find_seg that is off
    by one stamps every row wrongly), followed by segments that straddle scan blocks."""
    seeded = np.random.default_rng(1000).integers(0, 301, 1000)
    seeded[[0, 500, 501, 999]] = 0
    seeded[10] = 300
    return {"single": [5000],
            "empty first, last, middle, two in a row": [0, 300, 0, 0, 257, 0, 2048, 1, 0],
            "1000 seeded": [int(v) for v in seeded],
            "every residue": [1] * 2048 + [2049, 255, 257, 1, 2047]}


def close_rows(raw, frac=8):
    """Moves every `frac`-th row next to the origin so that radius segments drop some."""
    raw[::frac, :2] *= F32(0.01)
    return raw


def waymo_like_transforms():
    """inv(pose0) @ pose_k with rotations about all three axes and translations of the order of 1e4 m that cancel to tens of metres."""
    def rot(ax, a):
        c, s = np.cos(a), np.sin(a)
        R = np.eye(4)
        i, j = [(1, 2), (0, 2), (0, 1)][ax]
        R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
        return R
    def pose(yaw, pitch, roll, t):
        P = rot(2, yaw) @ rot(1, pitch) @ rot(0, roll)
        P[:3, 3] = t
        return P
    p0 = pose(1.1, 0.02, -0.015, [12_345.678, -9_876.543, 31.25])
    out = []
    for k in range(1, 5):
        pk = pose(1.1 + 0.03 * k, 0.02 - 0.004 * k, -0.015 + 0.006 * k, [12_345.678 + 7.5 * k, -9_876.543 - 4.25 * k, 31.25 + 0.125 * k])
        out.append(np.linalg.inv(p0) @ pk)
    return out
