"""Inputs shared by tests/test_paste_augment_cpu.py and tests/test_gpu_paste_augment.py: the planted collision cases, the seeded selection
batch and the seeded point-pass batch.  The CPU file checks that every seeded decision is far from its threshold (so that the GPU's own
sin / cos cannot change it); the GPU file holds the kernels to the fp64 statement on the same arrays."""
import numpy as np

D = 9


def box(x, y, dx, dy, yaw, z=0.0, dz=2.0):
    b = np.zeros(D, np.float32)
    b[[0, 1, 2, 3, 4, 5, 8]] = [x, y, z, dx, dy, dz, yaw]
    return b


def planted():
    """(gt (3, 9), cand (9, 9), group (9), expected accept (9)); every number of the degenerate cases is dyadic, every yaw there 0.
       A   inside gt 0 (containment, no edge crosses)                                    -> rejected
       B   same y-extent as gt 1, overlapping in x: edges collinear or touching at ends  -> no collision, accepted
       C   touches gt 2 along an edge: the stand-up overlap is 0, not > 0                -> accepted
       E1  overlaps E2 of its own group, visited first                                   -> rejected
       E2  E1 no longer counts                                                           -> accepted
       D1, D2  the same pair pattern in group 1                                          -> rejected, accepted
       F   group 2, overlaps only E1 (rejected earlier: blocks nothing)                  -> accepted
       G   group 2, overlaps E2 (accepted earlier)                                       -> rejected"""
    gt = np.stack([box(0, 0, 6, 6, 0), box(20, 0, 4, 2, 0), box(40, 0, 2, 2, 0)])
    cand = np.stack([box(0.3, 0.2, 1, 1, 0.3), box(22, 0, 4, 2, 0), box(42, 0, 2, 2, 0), box(80, 0, 3, 2, 0), box(82, 0, 3, 2, 0.3),
                     box(60, 0, 3, 2, 0.2), box(61, 0.5, 3, 2, -0.4), box(78, 0, 3, 2, 0.3), box(84, 0, 3, 2, -0.3)])
    group = np.array([0, 0, 0, 0, 0, 1, 1, 2, 2], np.int32)
    expect = np.array([0, 1, 1, 0, 1, 0, 1, 1, 0], bool)
    return gt, cand, group, expect


def _random_boxes(rng, n, lo, hi):
    b = np.zeros((n, D), np.float32)
    b[:, 0] = rng.uniform(lo[0], hi[0], n)
    b[:, 1] = rng.uniform(lo[1], hi[1], n)
    b[:, 2] = rng.uniform(-1.0, 1.0, n)
    b[:, 3:6] = rng.uniform([2.0, 1.0, 1.0], [6.0, 3.0, 3.0], (n, 3))
    b[:, 6:8] = rng.normal(0, 2.0, (n, 2))
    b[:, 8] = rng.uniform(-np.pi, np.pi, n)
    return b


def selection_batch(seed=7):
    """B = 3, K = 20, S = 24 in 4 groups.  Frame 0: the planted cases (y near 0) plus random boxes (y in [10, 50]); frame 1: 0 gt; frame 2: 0
    candidates.  Returns dict(gt (3, 20, 9), cls (3, 20), num_gt (3), cand: {bank, boxes, cls, group}, n_groups)."""
    rng = np.random.default_rng(seed)
    B, K, S = 3, 20, 24
    gt = np.zeros((B, K, D), np.float32)
    cls = np.full((B, K), -1, np.int32)
    num_gt = np.array([17, 0, 20], np.int32)
    cand = dict(bank=np.full((B, S), -1, np.int32), boxes=np.zeros((B, S, D), np.float32), cls=np.full((B, S), -1, np.int32), group=np.full((B, S), -1, np.int32))
    pg, pc, pgroup, _ = planted()
    gt[0, :3], gt[0, 3:17] = pg, _random_boxes(rng, 14, (0, 10), (40, 50))
    gt[0, 17:] = _random_boxes(rng, 3, (0, 10), (40, 50))   # beyond num_gt: must be ignored
    gt[2] = _random_boxes(rng, 20, (0, 10), (40, 50))
    for b in range(B):
        cls[b, :num_gt[b]] = rng.integers(0, 6, num_gt[b])
    extra = _random_boxes(rng, S - len(pc), (0, 10), (40, 50))
    egroup = np.sort(rng.integers(0, 4, len(extra))).astype(np.int32)
    boxes0 = np.concatenate([pc, extra])
    group0 = np.concatenate([pgroup, egroup])
    order = np.argsort(group0, kind="stable")
    cand["boxes"][0], cand["group"][0] = boxes0[order], group0[order]
    n1 = 21   # frame 1: 21 candidates, 3 padded slots
    cand["boxes"][1, :n1] = _random_boxes(rng, n1, (0, 10), (30, 40))
    cand["group"][1, :n1] = np.sort(rng.integers(0, 4, n1))
    for b, n in ((0, S), (1, n1)):
        cand["bank"][b, :n] = rng.integers(0, 12, n)
        cand["cls"][b, :n] = cand["group"][b, :n] + 1
    return dict(gt=gt, cls=cls, num_gt=num_gt, cand=cand, n_groups=4, planted_index=np.argsort(order, kind="stable")[:len(pc)])


def object_bank(seed=3, n_obj=12, F=5, tag0=1.0e6):
    """(points (P, F) fp32, offsets (n_obj + 1) int64): 5 .. 300 rows per object, xyz within +-1.5 m; column 3 carries a unique tag."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(5, 301, n_obj)
    off = np.zeros(n_obj + 1, np.int64)
    off[1:] = np.cumsum(rows)
    pts = rng.uniform(-1.5, 1.5, (int(off[-1]), F)).astype(np.float32)
    pts[:, 3] = tag0 + np.arange(len(pts))
    return pts, off


FACE_BOX = box(8, 4, 4, 2, 0, z=0.5, dz=2)                                       # yaw 0, dyadic: faces at x = 6, 10; y = 3, 5; z = -0.5, 1.5
FACE_POINTS = np.array([[10, 4.5, 0.25], [7, 5, 1.0], [8, 4, 1.5], [10, 5, 1.5], [6, 3, -0.5], [8, 4, 0.5]], np.float32)   # faces, edges, corners, centre


def points_batch(total, seed=5):
    """B = 3, F = 5.  Frame 0: ONE scene row, inside a candidate that is accepted (the frame loses all its points); frame 1: no scene row, but
    candidates; frame 2: the rest of the rows, uniform over 40 m x 40 m, with FACE_POINTS planted; about one row in six carries batch index -1 or
    3 (dropped), and the last 1100 rows are a -1 tail.  `total` rows in all.  Column 4 of a row (the first after xyz) is its tag = its index.
    Returns dict(points (total, 6), gt, cls, num_gt, cand, n_groups, bank_points, bank_offsets, planted_tags)."""
    rng = np.random.default_rng(seed)
    B, K, S, F = 3, 4, 8, 5
    pts = np.zeros((total, 1 + F), np.float32)
    pts[:, 1:3] = rng.uniform(0, 40, (total, 2))
    pts[:, 3] = rng.uniform(-1.5, 2.5, total)
    pts[:, 5:] = rng.random((total, F - 4))
    pts[:, 4] = np.arange(total)
    bi = np.full(total, 2.0, np.float32)
    drop = rng.random(total) < 1 / 6
    bi[drop] = rng.choice([-1.0, 3.0], int(drop.sum()))
    bi[total - 1100:] = -1.0
    bi[0] = 0.0
    pts[0, 1:4] = [50.25, 50.5, 0.0]
    pts[:, 0] = bi
    where = 100 + 7 * np.arange(len(FACE_POINTS))
    pts[where, 0], pts[where, 1:4] = 2.0, FACE_POINTS
    bank_points, bank_offsets = object_bank()
    gt = np.zeros((B, K, D), np.float32)
    gt[2] = np.stack([box(30, 30, 5, 2, 0.7), box(12, 30, 4, 2, -1.0), box(30, 8, 4.5, 2, 2.0), box(20, 20, 4, 4, 0.1)])
    cls = np.tile(np.arange(K, dtype=np.int32), (B, 1))
    num_gt = np.array([0, 0, 4], np.int32)
    cand = dict(bank=np.full((B, S), -1, np.int32), boxes=np.zeros((B, S, D), np.float32), cls=np.full((B, S), -1, np.int32), group=np.full((B, S), -1, np.int32))
    cand["boxes"][0, 0], cand["bank"][0, 0], cand["group"][0, 0] = box(50, 50, 3, 3, 0.4), 0, 0
    cand["boxes"][1, :2], cand["bank"][1, :2], cand["group"][1, :2] = np.stack([box(5, 5, 3, 2, 1.0), box(15, 5, 3, 2, 2.0)]), [3, 4], [0, 1]
    c2 = np.stack([FACE_BOX, box(30.5, 30.2, 4, 2, 0.2), box(25, 12, 6, 3, 0.9, z=0.3, dz=3), box(26, 13, 5, 2, -0.5), box(5, 35, 5, 2.5, 2.5, z=0.2, dz=2.5),
                   box(35, 5, 6, 3, -2.0, z=0.8, dz=3), box(14, 22, 3.5, 2, 1.3), box(36, 36, 4, 4, 0.0)])
    cand["boxes"][2], cand["bank"][2], cand["group"][2] = c2, [1, 2, 5, 6, 7, 8, 9, 10], [0, 0, 1, 1, 2, 2, 3, 3]
    cand["cls"] = np.where(cand["bank"] >= 0, cand["group"] + 4, -1).astype(np.int32)
    return dict(points=pts, gt=gt, cls=cls, num_gt=num_gt, cand=cand, n_groups=4, bank_points=bank_points, bank_offsets=bank_offsets, planted_tags=where)


def xform_combos(rng):
    """32 frames: every on/off combination of rotation, scaling, translation, flip x, flip y.  Returns (32, 6) fp64 rows."""
    import paste_augment_ref as R

    rows = []
    for m in range(32):
        rows.append(R.xform_row(angle=rng.uniform(-0.8, 0.8) if m & 1 else None, scale=rng.uniform(0.9, 1.1) if m & 2 else None,
                                translate=rng.normal(0, 0.5) if m & 4 else None, flip_x=bool(m & 8), flip_y=bool(m & 16)))
    return np.stack(rows)


def transform_boxes(cols):
    """48 boxes from the fixture layout plus yaws at and next to +-fp32(pi); a NaN vx and a NaN (vx, vy) row when there are 9 columns."""
    rng = np.random.default_rng(77)
    b = _random_boxes(rng, 48, (-9, -8), (9, 8))
    pi32 = np.float32(np.pi)
    b[:8, 8] = [pi32, -pi32, np.nextafter(pi32, np.float32(4)), np.nextafter(-pi32, np.float32(-4)), np.nextafter(pi32, np.float32(0)), 3.1, -3.1, 0.0]
    b[8:12, 8] = [2.4, -2.4, 3.0, -3.0]   # +-a next to these crosses +-pi
    b[5, 6] = np.nan
    b[11, 6:8] = np.nan
    return b if cols == 9 else np.ascontiguousarray(b[:, [0, 1, 2, 3, 4, 5, 8]])
