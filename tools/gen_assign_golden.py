#!/usr/bin/env python3
"""Writes tests/golden/assign_small.npz by RUNNING THE REFERENCE's AssignLabel (det3d/datasets/pipelines/assign.py with center_utils.py) on
a fixed input.  Build machine only (needs the reference tree, numpy; no GPU, no torch):

    python tools/gen_assign_golden.py --reference <reference tree>

The two files are loaded by path under a stand-in package name: the reference's det3d.datasets package __init__ pulls in its whole data
pipeline.  Nothing of their text is stored; the fixture holds the inputs, the config as plain arrays and the six outputs per task.

Case: 3 tasks [[a], [b, c], [d, e]], pc_range [-9.6, -8, -5, 9.6, 8, 3], voxel 0.1, out_size_factor [2, 4, 4] (maps 80 x 96 and 40 x 48: not
square, two strides), gaussian_overlap 0.1, min_radius 2, max_objs 64; 96 fp32 boxes, centres uniform slightly beyond the range, sizes
exp(U(-1.5, 1.8)), yaw in +-7, classes -1 .. 4 (-1 = a name no task lists), plus planted cases (see PLANTED)."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["a", "b", "c", "d", "e"]
TASKS = [["a"], ["b", "c"], ["d", "e"]]
PC_RANGE = [-9.6, -8.0, -5.0, 9.6, 8.0, 3.0]
VOXEL = [0.1, 0.1, 8.0]
OSF = [2, 4, 4]
OVERLAP, MIN_RADIUS, MAX_OBJS = 0.1, 2, 64


def load_reference(ref):
    pkg = types.ModuleType("pnx_ref_pipelines")
    pkg.__path__ = []
    sys.modules[pkg.__name__] = pkg
    mods = {}
    for name in ("center_utils", "assign"):
        spec = importlib.util.spec_from_file_location(f"{pkg.__name__}.{name}", os.path.join(ref, "det3d", "datasets", "pipelines", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = m
        spec.loader.exec_module(m)
        mods[name] = m
    return mods["assign"].AssignLabel


def make_inputs():
    rng = np.random.default_rng(20240)
    n = 96
    b = np.zeros((n, 9), np.float32)
    b[:, 0] = rng.uniform(-10.2, 10.2, n)
    b[:, 1] = rng.uniform(-8.6, 8.6, n)
    b[:, 2] = rng.uniform(-2.0, 1.0, n)
    b[:, 3:6] = np.exp(rng.uniform(-1.5, 1.8, (n, 3)))
    b[:, 6:8] = rng.normal(0, 2.0, (n, 2))
    b[:, 8] = rng.uniform(-7.0, 7.0, n)
    cls = rng.integers(-1, 5, n).astype(np.int32)
    # PLANTED cases (rows 0..8); sizes of the planted rows are ordinary unless they are the point
    b[0, 3], cls[0] = 0.0, 1                                   # a zero size: skipped
    b[1, 4], cls[1] = -1.3, 3                                  # a negative size: skipped
    b[2, 0], b[2, 1], cls[2] = -9.6 - 0.15, 1.0, 0             # stride 2: coor x = -0.75 in (-1, 0): truncates to cell 0, KEPT, negative offset
    b[3, 0], b[3, 1], cls[3] = 2.0, -8.0 - 0.15, 2             # the same in y on a stride-4 task (coor y = -0.375)
    b[4, 0], b[4, 1], cls[4] = 9.6, 0.5, 4                     # exactly on the upper edge: cell 48 of 48, dropped
    b[5, 0], b[5, 1], cls[5] = 9.6 - 0.05, 8.0 - 0.05, 3       # the last cell (47, 39)
    b[6, 0], b[6, 1], cls[6] = 3.21, -2.33, 1                  # two boxes of one class on one centre, different radii
    b[7, 0], b[7, 1], cls[7] = 3.21, -2.33, 1
    b[6, 3:5], b[7, 3:5] = (4.5, 2.0), (0.6, 0.5)
    return b, cls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "assign_small.npz"))
    a = ap.parse_args()
    AssignLabel = load_reference(a.reference)
    boxes, cls = make_inputs()
    names = np.array([NAMES[c] if c >= 0 else "unlisted" for c in cls])
    stage = AssignLabel(TASKS, OVERLAP, MAX_OBJS, MIN_RADIUS, PC_RANGE, VOXEL, OSF)
    res = stage({"annotations": {"gt_boxes": boxes, "gt_names": names}})
    out = dict(in_boxes=boxes, in_classes=cls, cfg_pc_range=np.asarray(PC_RANGE, np.float64), cfg_voxel_size=np.asarray(VOXEL, np.float64),
               cfg_out_size_factor=np.asarray(OSF, np.int64), cfg_tasks_ncls=np.asarray([len(t) for t in TASKS], np.int64),
               cfg_gaussian_overlap=np.float64(OVERLAP), cfg_min_radius=np.int64(MIN_RADIUS), cfg_max_objs=np.int64(MAX_OBJS))
    worst = 0.0
    for t in range(len(TASKS)):
        for k in ("hm", "anno_box", "ind", "mask", "cat", "gt_boxes"):
            out[f"t{t}_{k}"] = np.asarray(res[k][t])
        # distance of the reference's fp32 log / sin / cos from the fp64 values of the same fp32 inputs, in fp32 ulps
        m = res["mask"][t].astype(bool)
        gb, an = res["gt_boxes"][t][m].astype(np.float64), res["anno_box"][t][m]
        truth = np.concatenate([np.log(gb[:, 3:6]), np.sin(gb[:, 6:7]), np.cos(gb[:, 6:7])], axis=1)
        got = an[:, [3, 4, 5, 8, 9]]
        if len(got):
            worst = max(worst, float((np.abs(got.astype(np.float64) - truth) / np.spacing(np.abs(truth.astype(np.float32))).astype(np.float64)).max()))
    out["ref_ulp"] = np.float64(worst)
    np.savez_compressed(a.out, **out)
    n1 = sum(int((out[f"t{t}_hm"] == 1.0).sum()) for t in range(len(TASKS)))
    nobj = sum(int(out[f"t{t}_mask"].sum()) for t in range(len(TASKS)))
    print(f"{a.out}: {os.path.getsize(a.out)} bytes, {nobj} objects kept, {n1} cells equal to 1, ref_ulp {worst:.2f} (numpy {np.__version__})")


if __name__ == "__main__":
    main()
