#!/usr/bin/env python3
"""Times AssignLabel.assign (csrc/assign.hip) with device events at the nuScenes geometry: 6 tasks, 10 classes, 336 x 336 maps (C2ref),
B frames of up to K boxes from synth.make_gt_boxes, and prints the time beside its floor = bytes written (heat maps + label lists) / 8 TB/s.

    python tools/bench_assign.py [--batch 4] [--max-gt 200] [--iters 200]
    python tools/bench_assign.py --reference <reference tree>     # no GPU: wall time of the reference's host AssignLabel on the same boxes"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pillarnext_amd import synth  # noqa: E402

TASKS = [["car"], ["truck", "construction_vehicle"], ["bus", "trailer"], ["barrier"], ["motorcycle", "bicycle"], ["pedestrian", "traffic_cone"]]
ARGS = dict(gaussian_overlap=0.1, max_objs=500, min_radius=2, out_size_factor=[4] * 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2ref")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--max-gt", type=int, default=200)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reference", default="", help="time the reference's AssignLabel from this tree on the host instead (build machine)")
    a = ap.parse_args()
    cfg = synth.CONFIGS[a.config]
    boxes, classes, num_gt = synth.make_gt_boxes(a.config, a.batch, 0, max_gt=a.max_gt)
    what = f"{a.config}: 6 tasks, 10 classes, B = {a.batch}, K = {a.max_gt}, {int(num_gt.sum())} boxes ({num_gt.tolist()} per frame)"
    if a.reference:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from gen_assign_golden import load_reference

        stage = load_reference(a.reference)(TASKS, ARGS["gaussian_overlap"], ARGS["max_objs"], ARGS["min_radius"], list(cfg["pc_range"]), list(cfg["voxel_size"]),
                                            ARGS["out_size_factor"])
        flat = [n for t in TASKS for n in t]
        frames = [{"annotations": {"gt_boxes": boxes[b, : num_gt[b]], "gt_names": np.array([flat[c] if c >= 0 else "unlisted" for c in classes[b, : num_gt[b]]])}}
                  for b in range(a.batch)]
        best = []
        for _ in range(5):
            t0 = time.perf_counter()
            for f in frames:
                stage(dict(f))
            best.append(time.perf_counter() - t0)
        print(f"reference AssignLabel on the host, {what}: {min(best) * 1e3:.1f} ms per batch (best of 5, one thread; numpy {np.__version__}), "
              f"before the upload of {a.batch * 10 * 336 * 336 * 4 / 1e6:.1f} MB of heat maps")
        return
    import torch

    from pillarnext_amd.assign import AssignLabel

    assert torch.cuda.is_available(), "bench_assign.py measures on the GPU"
    stage = AssignLabel(TASKS, pc_range=list(cfg["pc_range"]), voxel_size=list(cfg["voxel_size"]), **ARGS)
    gb, gc, gn = (torch.from_numpy(v).cuda() for v in (boxes, classes, num_gt))
    for _ in range(a.warmup):
        res = stage.assign(gb, gc, gn)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        res = stage.assign(gb, gc, gn)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / a.iters
    written = sum(t.numel() * t.element_size() for k in ("hm", "anno_box", "ind", "mask", "cat", "gt_boxes") for t in res[k])
    hm = sum(t.numel() * t.element_size() for t in res["hm"])
    floor = written / 8e12 * 1e6
    print(f"AssignLabel.assign, {what}, maps {tuple(res['hm'][1].shape)}: {us:.1f} us per call (two launches, {a.iters} calls between two device events)")
    print(f"bytes written {written / 1e6:.2f} MB (heat maps {hm / 1e6:.2f} MB + label lists {(written - hm) / 1e6:.2f} MB); floor at 8 TB/s {floor:.2f} us; "
          f"{written / us / 1e6:.2f} TB/s = {floor / us * 100:.0f} % of the floor rate; kept per task {res['counts'].sum(0).tolist()}")


if __name__ == "__main__":
    main()
