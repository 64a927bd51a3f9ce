"""True rotated-rectangle overlap in fp64: Sutherland-Hodgman clipping of one rectangle by the other's four edges.  No margin, no transcription of the
reference's algorithm (collect crossings and contained corners, sort by angle, fan): this is what the overlap IS, to about 1e-15 of the boxes' area.
numpy only.  A pair with a non-finite field gives NaN; a box of zero area overlaps nothing."""
import numpy as np


def corners(box):
    """(4, 2) fp64 corners, counter-clockwise, of one [x, y, z, dx, dy, dz, heading] box."""
    x, y, dx, dy, h = (float(box[k]) for k in (0, 1, 3, 4, 6))
    c, s = np.cos(h), np.sin(h)
    local = np.array([[-dx, -dy], [dx, -dy], [dx, dy], [-dx, dy]]) / 2
    return local @ np.array([[c, s], [-s, c]]) + (x, y)


def clip(poly, q):
    """poly clipped by the convex counter-clockwise polygon q: list of points."""
    for i in range(len(q)):
        e0, e = q[i], q[(i + 1) % len(q)] - q[i]
        side = [e[0] * (p[1] - e0[1]) - e[1] * (p[0] - e0[0]) for p in poly]           # > 0: left of the edge = inside
        out = []
        for j, p in enumerate(poly):
            k = (j + 1) % len(poly)
            if side[j] >= 0:
                out.append(p)
            if (side[j] > 0 and side[k] < 0) or (side[j] < 0 and side[k] > 0):
                out.append(p + (poly[k] - p) * (side[j] / (side[j] - side[k])))
        poly = out
        if not poly:
            break
    return poly


def area(poly):
    if len(poly) < 3:
        return 0.0
    p = np.asarray(poly)
    x, y = p[:, 0], p[:, 1]
    return 0.5 * abs(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))


def deviations(ref, host, exact):
    """One row of DESIGN section 3's table, over the pairs where all three are finite: (max |ref - exact|, share of pairs with ref > 1, max |host - ref|)."""
    ref, host = np.asarray(ref, np.float64), np.asarray(host, np.float64)
    ok = np.isfinite(ref) & np.isfinite(host) & np.isfinite(exact)
    if not ok.any():
        return 0.0, 0.0, 0.0
    return float(np.abs(ref - exact)[ok].max()), float((ref[ok] > 1).mean()), float(np.abs(host - ref)[ok].max())


def aligned(a, b):
    """Per pair i: (overlap area, IoU, number of vertices of the intersection polygon), fp64 / fp64 / int."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ov, iou, nv = np.zeros(len(a)), np.zeros(len(a)), np.zeros(len(a), np.int64)
    for i, (p, q) in enumerate(zip(a, b)):
        if not (np.isfinite(p[[0, 1, 3, 4, 6]]).all() and np.isfinite(q[[0, 1, 3, 4, 6]]).all()):
            ov[i] = iou[i] = np.nan
            continue
        sa, sb = p[3] * p[4], q[3] * q[4]
        if sa > 0 and sb > 0:
            poly = clip(list(corners(p)), corners(q))
            ov[i], nv[i] = area(poly), len(poly)
        union = sa + sb - ov[i]
        iou[i] = ov[i] / union if union > 0 else 0.0
    return ov, iou, nv
