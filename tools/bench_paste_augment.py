#!/usr/bin/env python3
"""Times the GT paste + global augmentation stage (csrc/augment.hip, pillarnext_amd.augment.PasteAugment) with device events at C2 x 4 frames:
300 k points and up to 200 gt boxes per frame, 40 candidates per frame from a synthetic bank whose objects hold 5 .. 2000 points, all four
transforms.  Prints the time per call, the bytes the pass has to move (from the shapes: every scene row read once and every output row written
once, the accepted objects' bank rows read once) over that time as a share of the 8 TB/s HBM peak, and -- for scale -- the wall time of the
numpy statement of the same work (tests/paste_augment_ref.py, the vectorised point test and transforms; its collision loop is plain Python).

    python tools/bench_paste_augment.py [--batch 4] [--points 300000] [--iters 100] [--no-host]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pillarnext_amd import synth  # noqa: E402

CLASSES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone"]
GROUPS = [{"car": 2}, {"truck": 3}, {"construction_vehicle": 7}, {"bus": 4}, {"trailer": 6}, {"barrier": 2}, {"motorcycle": 6}, {"bicycle": 6}, {"pedestrian": 2},
          {"traffic_cone": 2}]   # the nuScenes recipe's maxima: 40 in all


def setup(a):
    from pillarnext_amd import augment as A

    bank = synth.make_object_bank(CLASSES, 60, seed=1, point_dim=5, min_points=5, max_points=2000, config=a.config)
    np.random.seed(0)
    sampler = A.DataBaseSamplerV2(groups=GROUPS, rate=1.0, db_infos=bank, class_names=CLASSES)
    aug = {"rotation": A.Rotation([-0.78539816, 0.78539816]), "scaling": A.Scaling([0.9, 1.1]), "translation": A.Translation(0.5), "flip": A.Flip([0.5, 0.5])}
    pts = synth.make_batch(a.config, a.batch, "sweep", n=a.points)
    boxes, classes, num_gt = synth.make_gt_boxes(a.config, a.batch, 0, max_gt=200)
    # 40 candidates per frame whatever the frame holds: the sampler is asked as if no object of a sampled class were present
    host_classes = [np.zeros(0, np.int32) for _ in range(a.batch)]
    return sampler, aug, pts, boxes, classes, num_gt, host_classes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--points", type=int, default=300000, help="scene points per frame")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy statement")
    a = ap.parse_args()
    import torch

    from pillarnext_amd import augment as A

    assert torch.cuda.is_available(), "bench_paste_augment.py measures on the GPU"
    sampler, aug, pts, boxes, classes, num_gt, host_classes = setup(a)
    stage = A.PasteAugment(sampler, aug)
    dp, db, dc, dn = (torch.from_numpy(v).cuda() for v in (pts, boxes, classes, num_gt))
    for _ in range(a.warmup):
        out = stage(dp, db, dc, dn, host_classes=host_classes)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(a.iters):
        out = stage(dp, db, dc, dn, host_classes=host_classes)
    e1.record()
    host_issue = (time.perf_counter() - t0) / a.iters
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / a.iters
    buf = stage.last
    n_out, rows_pasted, n_acc = int(out[1].item()), int(buf["pasted_rows"].sum().item()), int(buf["accept"].sum().item())
    n_pts, width = pts.shape
    moved = (n_pts + out[0].shape[0]) * width * 4 + rows_pasted * (width - 1) * 4       # read every scene row, write every output row, read the pasted bank rows
    print(f"paste_and_augment, {a.config} x {a.batch} frames: {n_pts} scene rows of {width} floats, gt per frame {num_gt.tolist()}, {buf['accept'].shape[1]} candidate "
          f"slots per frame; last call: {n_acc} objects accepted bringing {rows_pasted} rows, n_out {n_out} of capacity {out[0].shape[0]}")
    print(f"  {us:.1f} us per call between two device events ({a.iters} calls; the host issues a call in {host_issue * 1e6:.0f} us: sampler, draws, three uploads, "
          f"ten launches)")
    print(f"  bytes the pass must move {moved / 1e6:.2f} MB -> {moved / us / 1e6:.3f} TB/s = {moved / us / 1e6 / 8.0 * 100:.1f} % of the 8 TB/s HBM peak "
          f"(floor {moved / 8e12 * 1e6:.1f} us)")
    if a.no_host:
        return
    import paste_augment_ref as R

    frames = [sampler.sample_frame(h) for h in host_classes]
    xf = np.stack([A.draw_xform(aug) for _ in range(a.batch)])
    S = max(len(f) for f in frames)
    cand = dict(bank=np.full((a.batch, S), -1, np.int32), boxes=np.zeros((a.batch, S, 9), np.float32), cls=np.full((a.batch, S), -1, np.int32),
                group=np.full((a.batch, S), -1, np.int32))
    for b, f in enumerate(frames):
        for i, (bank_id, box, c, g) in enumerate(f):
            cand["bank"][b, i], cand["boxes"][b, i], cand["cls"][b, i], cand["group"][b, i] = bank_id, box, c, g
    bp, bo = sampler.bank_host()
    t0 = time.perf_counter()
    R.paste_and_augment(pts, boxes, classes, num_gt, cand, bp, bo, sampler.n_groups, xf)
    print(f"  the numpy statement of the same work on this host, one thread: {(time.perf_counter() - t0) * 1e3:.0f} ms per batch (numpy {np.__version__})")


if __name__ == "__main__":
    main()
