"""fp64 numpy statement of the GT paste and the four global augmentations (pnx_paste_select, pnx_paste_augment_points, pnx_augment_boxes,
csrc/augment.hip), written from their specification: the yardstick of tests/test_paste_augment_cpu.py (against the recorded run of the
reference's augmentation.py and BatchSampler, tests/golden/paste_augment_small.npz) and of tests/test_gpu_paste_augment.py.

Selection.  BEV corners of [x, y, dx, dy, yaw] in fp64 from the fp32 values, clockwise (-,-) (-,+) (+,+) (+,-), turned counter-clockwise by
yaw and moved to the centre.  Box a collides with box q when their stand-up rectangles overlap strictly in x and in y and either an edge of
a and an edge of q cross properly (four strict orientation tests) or all corners of one lie strictly inside the other.  Candidates are
visited group by group, in candidate order inside a group; a candidate is rejected when it collides with a gt box, an accepted candidate of
an earlier group, or any candidate of its own group that has not been rejected so far (the unvisited ones included).

Points.  A scene point is removed when for some accepted box |z - cz| <= dz/2, |lx| <= dx/2 and |ly| <= dy/2 (lx = sx cos + sy sin,
ly = -sx sin + sy cos).  A frame's result is [pasted rows in acceptance order (bank row + fp32 box centre, fp32 adds), survivors in input
order]; the boxes are [gt, accepted].

Transforms, each rounding to fp32 before the next: rotation (separate fp64 products and sum), scaling (fp32 multiply of xyz and of every box
column but the yaw), translation (ONE scalar on x, y, z; fp64 add), flip x (y, yaw, vy negated), flip y (x, vx negated, yaw = -yaw + fp32(pi)),
the yaw wrapped once after each flip.  A NaN box element enters every stage as 0 and is NaN again after it."""
import numpy as np

ROTATE, SCALE, TRANSLATE, FLIP_X, FLIP_Y = 1, 2, 4, 8, 16
PI32 = np.float32(np.pi)
TWO_PI32 = np.float32(2 * np.pi)


# ------------------------------------------------------------------------------------------------------------------------------ selection
def corners(boxes):
    """(n, D) fp32 boxes -> (n, 4, 2) fp64 BEV corners.  (fp64 boxes are taken as they are: the robustness checks move them by less than an fp32 ulp.)"""
    b = np.asarray(boxes)
    b = b if b.dtype == np.float64 else b.astype(np.float32).astype(np.float64)
    hx, hy = b[:, 3] * 0.5, b[:, 4] * 0.5
    lx = np.stack([-hx, -hx, hx, hx], 1)
    ly = np.stack([-hy, hy, hy, -hy], 1)
    c, s = np.cos(b[:, -1])[:, None], np.sin(b[:, -1])[:, None]
    return np.stack([(lx * c - ly * s) + b[:, 0:1], (lx * s + ly * c) + b[:, 1:2]], 2)


def _inside(a, q):
    """every corner of q strictly inside the clockwise box a"""
    for l in range(4):
        for k in range(4):
            vx, vy = -(a[k, 0] - a[(k + 1) % 4, 0]), -(a[k, 1] - a[(k + 1) % 4, 1])
            cross = vy * (a[k, 0] - q[l, 0])
            cross -= vx * (a[k, 1] - q[l, 1])
            if cross >= 0:
                return False
    return True


def collide(a, q):
    """a, q: (4, 2) fp64 corners.  The directed test: a plays `boxes[i]`, q plays `qboxes[j]`."""
    if not min(a[:, 0].max(), q[:, 0].max()) - max(a[:, 0].min(), q[:, 0].min()) > 0:
        return False
    if not min(a[:, 1].max(), q[:, 1].max()) - max(a[:, 1].min(), q[:, 1].min()) > 0:
        return False
    for k in range(4):
        A, B = a[k], a[(k + 1) % 4]
        for l in range(4):
            C, D = q[l], q[(l + 1) % 4]
            acd = (D[1] - A[1]) * (C[0] - A[0]) > (C[1] - A[1]) * (D[0] - A[0])
            bcd = (D[1] - B[1]) * (C[0] - B[0]) > (C[1] - B[1]) * (D[0] - B[0])
            if acd != bcd:
                abc = (C[1] - A[1]) * (B[0] - A[0]) > (B[1] - A[1]) * (C[0] - A[0])
                abd = (D[1] - A[1]) * (B[0] - A[0]) > (B[1] - A[1]) * (D[0] - A[0])
                if abc != abd:
                    return True
    return _inside(a, q) or _inside(q, a)


def select(gt_boxes, cand_boxes, cand_group, n_groups, cand_valid=None):
    """One frame.  gt_boxes (ng, D), cand_boxes (S, D), cand_group (S) ints, cand_valid (S) bools or None.  Returns (accept (S) bool, order):
    `order` lists the accepted candidates in acceptance order."""
    gt = corners(gt_boxes) if len(gt_boxes) else np.zeros((0, 4, 2))
    S = len(cand_boxes)
    cc = corners(cand_boxes) if S else np.zeros((0, 4, 2))
    valid = np.ones(S, bool) if cand_valid is None else np.asarray(cand_valid, bool)
    group = np.asarray(cand_group, np.int64)
    accept = np.zeros(S, bool)
    order = []
    for g in range(n_groups):
        mine = [i for i in range(S) if valid[i] and group[i] == g]
        alive = set(mine)
        for i in mine:
            hit = any(collide(cc[i], gt[j]) for j in range(len(gt)))
            hit = hit or any(collide(cc[i], cc[j]) for j in order)
            hit = hit or any(collide(cc[i], cc[j]) for j in alive if j != i)
            if hit:
                alive.discard(i)
            else:
                accept[i] = True
        order += [i for i in mine if accept[i]]
    return accept, order


def merge_boxes(gt_boxes, gt_classes, cand_boxes, cand_classes, order, rows_total):
    """[gt, accepted] padded with zeros / -1 to rows_total."""
    D = gt_boxes.shape[1] if len(gt_boxes) else cand_boxes.shape[1]
    boxes = np.zeros((rows_total, D), np.float32)
    classes = np.full(rows_total, -1, np.int32)
    n = len(gt_boxes)
    boxes[:n], classes[:n] = gt_boxes, gt_classes
    for i in order:
        boxes[n], classes[n] = cand_boxes[i], cand_classes[i]
        n += 1
    return boxes, classes, n


# --------------------------------------------------------------------------------------------------------------------------------- points
def face_distance(xyz, boxes):
    """xyz (n, 3) fp32, boxes (m, D) fp32 -> (inside (n, m) bool, margin (n, m) fp64): margin = the smallest |distance to a face plane| in the
    box's frame, the quantity the tests use to leave near-face points out of a comparison."""
    p = np.asarray(xyz, np.float32).astype(np.float64)
    b = np.asarray(boxes, np.float32).astype(np.float64)
    c, s = np.cos(b[:, -1])[None], np.sin(b[:, -1])[None]
    sx, sy = p[:, 0:1] - b[None, :, 0], p[:, 1:2] - b[None, :, 1]
    lx, ly = sx * c + sy * s, -sx * s + sy * c
    dz = np.abs(p[:, 2:3] - b[None, :, 2])
    hx, hy, hz = b[None, :, 3] / 2.0, b[None, :, 4] / 2.0, b[None, :, 5] / 2.0
    inside = (dz <= hz) & (np.abs(lx) <= hx) & (np.abs(ly) <= hy)
    margin = np.minimum(np.abs(dz - hz), np.minimum(np.abs(np.abs(lx) - hx), np.abs(np.abs(ly) - hy)))
    return inside, margin


def paste_frame(scene, accepted_boxes, objects):
    """scene (n, F) fp32 rows of one frame, accepted_boxes (m, D) fp32 in acceptance order, objects: their (r_i, F) fp32 bank rows.  Returns
    (rows (n', F) fp32 = [pasted, survivors], n_pasted, keep (n) bool, near (n) fp64 = the smallest face margin of each scene row)."""
    scene = np.asarray(scene, np.float32)
    keep = np.ones(len(scene), bool)
    near = np.full(len(scene), np.inf)
    if len(accepted_boxes) and len(scene):
        inside, margin = face_distance(scene[:, :3], accepted_boxes)
        keep = ~inside.any(1)
        near = margin.min(1)
    pasted = []
    for bx, rows in zip(accepted_boxes, objects):
        r = np.array(rows, np.float32)
        r[:, :3] = r[:, :3] + np.asarray(bx[:3], np.float32)[None]   # fp32 + fp32
        pasted.append(r)
    parts = pasted + [scene[keep]]
    out = np.concatenate(parts, 0) if parts else scene
    return out.astype(np.float32), int(sum(len(r) for r in pasted)), keep, near


# ----------------------------------------------------------------------------------------------------------------------------- transforms
def xform_row(angle=None, scale=None, translate=None, flip_x=False, flip_y=False):
    """The six doubles per frame the device reads: cos a, sin a, a, fp32(scale), t, flags."""
    flags = (ROTATE if angle is not None else 0) | (SCALE if scale is not None else 0) | (TRANSLATE if translate is not None else 0) | \
        (FLIP_X if flip_x else 0) | (FLIP_Y if flip_y else 0)
    a = 0.0 if angle is None else float(angle)
    return np.array([np.cos(a), np.sin(a), a, float(np.float32(1.0 if scale is None else scale)), 0.0 if translate is None else float(translate),
                     float(flags)], np.float64)


def _rot(x, y, c, s):
    x, y = x.astype(np.float64), y.astype(np.float64)
    return ((x * c) - (y * s)).astype(np.float32), ((x * s) + (y * c)).astype(np.float32)


def points_stages(xyz, xf):
    """xyz (n, 3) fp32, xf = xform_row(..).  Returns the fp32 array after each of the five stages [rotation, scaling, translation, flip x, flip y]
    (a disabled stage repeats its input)."""
    c, s, _, scale, t, flags = xf
    flags = int(flags)
    p = np.array(xyz, np.float32)
    out = []
    if flags & ROTATE:
        p = p.copy()
        p[:, 0], p[:, 1] = _rot(p[:, 0], p[:, 1], c, s)
    out.append(p)
    if flags & SCALE:
        p = p * np.float32(scale)
    out.append(p)
    if flags & TRANSLATE:
        p = (p.astype(np.float64) + t).astype(np.float32)
    out.append(p)
    if flags & FLIP_X:
        p = p.copy()
        p[:, 1] = -p[:, 1]
    out.append(p)
    if flags & FLIP_Y:
        p = p.copy()
        p[:, 0] = -p[:, 0]
    out.append(p)
    return out


def augment_points(xyz, xf):
    return points_stages(xyz, xf)[-1]


def _wrap(yaw):
    yaw = np.where(yaw > PI32, yaw - TWO_PI32, yaw).astype(np.float32)
    return np.where(yaw < -PI32, yaw + TWO_PI32, yaw).astype(np.float32)


def boxes_stages(boxes, xf):
    """boxes (m, 7 or 9) fp32.  The fp32 array after each of the five stages."""
    c, s, a, scale, t, flags = xf
    flags = int(flags)
    b = np.array(boxes, np.float32)
    vel = b.shape[1] == 9
    out = []

    def stage(fn):
        nonlocal b
        m = np.isnan(b)
        b = b.copy()
        b[m] = 0
        fn(b)
        b[m] = np.nan

    def rotate(b):
        b[:, 0], b[:, 1] = _rot(b[:, 0], b[:, 1], c, s)
        if vel:
            b[:, 6], b[:, 7] = _rot(b[:, 6], b[:, 7], c, s)
        b[:, -1] = b[:, -1] + np.float32(a)

    def scaling(b):
        b[:, :-1] = b[:, :-1] * np.float32(scale)

    def translate(b):
        b[:, :3] = (b[:, :3].astype(np.float64) + t).astype(np.float32)

    def flip_x(b):
        b[:, 1] = -b[:, 1]
        b[:, -1] = -b[:, -1]
        if vel:
            b[:, 7] = -b[:, 7]
        b[:, -1] = _wrap(b[:, -1])

    def flip_y(b):
        b[:, 0] = -b[:, 0]
        b[:, -1] = -b[:, -1] + PI32
        if vel:
            b[:, 6] = -b[:, 6]
        b[:, -1] = _wrap(b[:, -1])

    for bit, fn in ((ROTATE, rotate), (SCALE, scaling), (TRANSLATE, translate), (FLIP_X, flip_x), (FLIP_Y, flip_y)):
        if flags & bit:
            stage(fn)
        out.append(b)
    return out


def augment_boxes(boxes, xf):
    return boxes_stages(boxes, xf)[-1]


# ------------------------------------------------------------------------------------------------------------------------------ whole call
def paste_and_augment(points, gt_boxes, gt_classes, num_gt, cand=None, bank_points=None, bank_offsets=None, n_groups=0, xforms=None):
    """The whole stage on numpy arrays.  points (N, 1 + F) fp32; gt_boxes (B, K, D); gt_classes (B, K); num_gt (B) or None; cand: None or
    {bank, boxes, cls, group} (B, S, ..) with bank < 0 = padding; xforms (B, 6) or None.
    Returns dict(points (n_out, 1 + F), frame_rows (B), boxes (B, K + S, D), classes (B, K + S), num (B), accept (B, S), near (n_out) fp64:
    for a surviving scene row its smallest face margin, inf for pasted rows, removed_near: margins of the removed rows, ambiguous: the input
    scene rows (F columns), kept or removed, whose margin is below 1e-5)."""
    points = np.asarray(points, np.float32)
    B, K, D = gt_boxes.shape
    S = 0 if cand is None else cand["bank"].shape[1]
    bi = points[:, 0]
    rows_out, near_out, frame_rows = [], [], []
    boxes = np.zeros((B, K + S, D), np.float32)
    classes = np.full((B, K + S), -1, np.int32)
    num = np.zeros(B, np.int32)
    accept = np.zeros((B, S), bool)
    removed_near, ambiguous = [], [points[:0, 1:]]
    for b in range(B):
        ng = K if num_gt is None else int(num_gt[b])
        order = []
        if S:
            valid = cand["bank"][b] >= 0
            accept[b], order = select(gt_boxes[b, :ng], cand["boxes"][b], cand["group"][b], n_groups, valid)
            boxes[b], classes[b], num[b] = merge_boxes(gt_boxes[b, :ng], gt_classes[b, :ng], cand["boxes"][b], cand["cls"][b], order, K + S)
        else:
            boxes[b, :ng], classes[b, :ng], num[b] = gt_boxes[b, :ng], gt_classes[b, :ng], ng
        scene = points[(bi >= 0) & (bi < B) & (bi.astype(np.int64) == b)][:, 1:] if len(points) else points[:0, 1:]
        objs = [bank_points[bank_offsets[cand["bank"][b, i]]:bank_offsets[cand["bank"][b, i] + 1]] for i in order]
        acc_boxes = cand["boxes"][b][order] if S else np.zeros((0, D), np.float32)
        rows, n_pasted, keep, near = paste_frame(scene, acc_boxes, objs)
        removed_near.append(near[~keep])
        ambiguous.append(scene[near < 1e-5])
        near = np.concatenate([np.full(n_pasted, np.inf), near[keep]])
        if xforms is not None:
            rows = rows.copy()
            rows[:, :3] = augment_points(rows[:, :3], xforms[b])
            boxes[b, :num[b]] = augment_boxes(boxes[b, :num[b]], xforms[b])
        rows_out.append(np.concatenate([np.full((len(rows), 1), b, np.float32), rows], 1))
        near_out.append(near)
        frame_rows.append(len(rows))
    return dict(points=np.concatenate(rows_out, 0), frame_rows=np.asarray(frame_rows, np.int32), boxes=boxes, classes=classes, num=num, accept=accept,
                near=np.concatenate(near_out), removed_near=np.concatenate(removed_near), ambiguous=np.concatenate(ambiguous, 0))
