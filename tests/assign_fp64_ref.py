"""fp64 numpy statement of the label assignment (pnx_assign_labels, csrc/assign.hip), written from its specification: the yardstick of
tests/test_assign_cpu.py (against the reference's own output, tests/golden/assign_small.npz) and of tests/test_gpu_assign.py.

Per object: sizes in cells by two fp64 divisions, the CenterNet radius (three roots, the third not divided by its leading coefficient,
truncated, at least min_radius), the centre in cells rounded to fp32 and truncated toward zero, the range test on the integer cell.  The
survivors of a task take slots in input order; those beyond max_objs are dropped from the lists and the heat map, `counts` keeps the
un-clamped number.  The heat map is the per-cell maximum over the objects of exp(-(dx^2 + dy^2) / (2 sigma^2)), sigma = (2r + 1) / 6, over the
|dx|, |dy| <= r window around the integer cell, in fp64, rounded to fp32 once.  log / sin / cos of anno_box are the fp64 values of the fp32
inputs (`anno64`), `anno_box` their fp32 rounding."""
import numpy as np


def make_cfg(tasks_ncls, pc_range, voxel_size, out_size_factor, gaussian_overlap, min_radius, max_objs):
    """tasks_ncls: classes per task.  Plain values only (what the fixture stores)."""
    pr, vs = np.asarray(pc_range, np.float64), np.asarray(voxel_size, np.float64)
    grid = np.round((pr[3:] - pr[:3]) / vs).astype(np.int64)
    osf = [int(v) for v in out_size_factor]
    return dict(lo=pr[:2].copy(), voxel=vs[:2].copy(), overlap=float(gaussian_overlap), min_radius=int(min_radius), max_objs=int(max_objs), osf=osf,
                hw=[(int(grid[1] // f), int(grid[0] // f)) for f in osf], ncls=[int(n) for n in tasks_ncls],
                class_task=[t for t, n in enumerate(tasks_ncls) for _ in range(n)], class_cls=[c for n in tasks_ncls for c in range(n)])


def _radius(h, w, o):
    b1 = h + w
    c1 = w * h * (1 - o) / (1 + o)
    r1 = (b1 + np.sqrt(b1 * b1 - 4 * c1)) / 2
    b2 = 2 * (h + w)
    c2 = (1 - o) * w * h
    r2 = (b2 + np.sqrt(b2 * b2 - 16 * c2)) / 2
    b3 = -2 * o * (h + w)
    c3 = (o - 1) * w * h
    r3 = (b3 + np.sqrt(b3 * b3 - 16 * o * c3)) / 2
    return np.minimum(r1, np.minimum(r2, r3))


def assign(boxes, classes, cfg, num_gt=None):
    """boxes (B, K, 9) fp32, classes (B, K) int, num_gt (B) or None.  Returns {hm, hm64, anno_box, anno64, ind, mask, cat, gt_boxes: lists per
    task, counts (B, T) int32, windows: per task a bool (B, ncls, H, W) map of the cells inside at least one drawn window}."""
    boxes = np.asarray(boxes, np.float32)
    classes = np.asarray(classes, np.int64)
    B, K = classes.shape
    T, M = len(cfg["osf"]), cfg["max_objs"]
    ctask, ccls = np.asarray(cfg["class_task"], np.int64), np.asarray(cfg["class_cls"], np.int64)
    out = {k: [] for k in ("hm", "hm64", "anno_box", "anno64", "ind", "mask", "cat", "gt_boxes", "windows")}
    for t in range(T):
        H, W = cfg["hw"][t]
        out["hm64"].append(np.zeros((B, cfg["ncls"][t], H, W), np.float64))
        out["windows"].append(np.zeros((B, cfg["ncls"][t], H, W), bool))
        out["anno64"].append(np.zeros((B, M, 10), np.float64))
        out["ind"].append(np.zeros((B, M), np.int64))
        out["mask"].append(np.zeros((B, M), np.uint8))
        out["cat"].append(np.zeros((B, M), np.int64))
        out["gt_boxes"].append(np.zeros((B, M, 7), np.float32))
    counts = np.zeros((B, T), np.int32)
    for b in range(B):
        n = K if num_gt is None else int(min(max(int(num_gt[b]), 0), K))
        bx, g = boxes[b, :n], classes[b, :n]
        known = (g >= 0) & (g < len(ctask))
        gi = np.where(known, g, 0)
        task, cls = np.where(known, ctask[gi], -1), ccls[gi]
        for t in range(T):
            H, W = cfg["hw"][t]
            f = float(cfg["osf"][t])
            with np.errstate(all="ignore"):
                sx = bx[:, 3].astype(np.float64) / cfg["voxel"][0] / f
                sy = bx[:, 4].astype(np.float64) / cfg["voxel"][1] / f
                ok = (task == t) & (sx > 0) & (sy > 0) & np.isfinite(bx[:, 0]) & np.isfinite(bx[:, 1])
                sxs, sys_ = np.where(ok, sx, 1.0), np.where(ok, sy, 1.0)
                rad = np.maximum(cfg["min_radius"], np.trunc(_radius(sys_, sxs, cfg["overlap"])).astype(np.int64))
                ctx = ((bx[:, 0].astype(np.float64) - cfg["lo"][0]) / cfg["voxel"][0] / f).astype(np.float32)
                cty = ((bx[:, 1].astype(np.float64) - cfg["lo"][1]) / cfg["voxel"][1] / f).astype(np.float32)
                ix = np.trunc(np.where(ok, ctx, -9.0).astype(np.float64))
                iy = np.trunc(np.where(ok, cty, -9.0).astype(np.float64))
            ok &= (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
            idx = np.nonzero(ok)[0]
            counts[b, t] = len(idx)
            idx = idx[:M]
            m = len(idx)
            if m == 0:
                continue
            x, y, r, c = ix[idx].astype(np.int64), iy[idx].astype(np.int64), rad[idx], cls[idx]
            o = bx[idx]
            out["ind"][t][b, :m] = y * W + x
            out["mask"][t][b, :m] = 1
            out["cat"][t][b, :m] = c
            out["gt_boxes"][t][b, :m] = o[:, [0, 1, 2, 3, 4, 5, 8]]
            a = out["anno64"][t][b]
            a[:m, 0] = (ctx[idx] - x.astype(np.float32)).astype(np.float64)
            a[:m, 1] = (cty[idx] - y.astype(np.float32)).astype(np.float64)
            a[:m, 2] = o[:, 2]
            with np.errstate(all="ignore"):
                a[:m, 3:6] = np.log(o[:, 3:6].astype(np.float64))
            a[:m, 6:8] = o[:, 6:8]
            a[:m, 8] = np.sin(o[:, 8].astype(np.float64))
            a[:m, 9] = np.cos(o[:, 8].astype(np.float64))
            # heat map: all objects against all cells at once, per class
            dy = np.arange(H, dtype=np.float64)[None, :, None] - y[:, None, None]
            dx = np.arange(W, dtype=np.float64)[None, None, :] - x[:, None, None]
            rr = r.astype(np.float64)[:, None, None]
            sigma = (2.0 * rr + 1.0) / 6.0
            inside = (np.abs(dx) <= rr) & (np.abs(dy) <= rr)
            val = np.where(inside, np.exp(-(dx * dx + dy * dy) / (2.0 * sigma * sigma)), 0.0)
            for k in range(cfg["ncls"][t]):
                sel = c == k
                if sel.any():
                    out["hm64"][t][b, k] = val[sel].max(axis=0)
                    out["windows"][t][b, k] = inside[sel].any(axis=0)
    out["hm"] = [h.astype(np.float32) for h in out["hm64"]]
    out["anno_box"] = [a.astype(np.float32) for a in out["anno64"]]
    out["counts"] = counts
    return out


def ulp_distance(a32, truth64):
    """|a - truth| in units of the fp32 spacing at the truth (elementwise; a is fp32, truth fp64)."""
    t32 = np.asarray(truth64, np.float64).astype(np.float32)
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(a32, np.float64) - np.asarray(truth64, np.float64)) / np.spacing(np.abs(t32)).astype(np.float64)
