#!/usr/bin/env python3
"""Timing of the voxel and multi-view readers on one GPU, synthetic clouds, HIP events: the grouping calls (pnx_group_points: all of
its kernels + the one host sync for the two counts), the eval PFN stack and bilinear gather of a view, and MVFFeatureNet end to end at the
reference's Waymo MVF geometry (configs/models/reader/mvf_encoder.yaml: 0.075 m pillars over +-76.8 m = 2048 x 2048, cylinder cells 0.140625 deg x 0.2 m =
2560 x 100) with the per-view sparse ResNets as fp32 torch modules and on the masked HIP convolution kernels (use_hip_convs).
Algorithmic bytes of a grouping call = read every 24-byte row once + write the feature rows, unq_inv and coords once (no credit for the key /
bitmap / scan scratch).  usage: python tools/bench_readers.py [--points 180000] [--batch 2]
--train runs the training leg instead: sampling a view's map at the points, forward + backward, through SingleView.sample -- the autograd node on
pnx_bilinear_gather / pnx_bilinear_gather_backward against the torch statement (PNX_TRAIN_BILINEAR_HIP=0: four advanced-index gathers, four
index_put(accumulate) scatters on float atomics) -- at the YAML's geometry, 192 channels, both views' map sizes; the two alternate in one run,
medians of device-event times after warm-up, torch.cuda.max_memory_allocated above the resident inputs for each."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pillarnext_amd import ops, synth  # noqa: E402
from pillarnext_amd._lib import PNX_GROUP_CYLINDER_CLAMP, PNX_GROUP_PILLAR_CLAMP, PNX_GROUP_VOXEL  # noqa: E402
from pillarnext_amd.mvf_encoder import MVFFeatureNet  # noqa: E402


def timed(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def train_leg(a):
    B = a.batch
    t = torch.from_numpy(synth.make_batch("C4", B, "sweep", n=a.points)).cuda()
    pr, vs = [-76.8, -76.8, -10.0, 76.8, 76.8, 10.0], [0.075, 0.075, 20]
    cr, cs = [-180, -10.0, 0, 180, 10.0, 107], [0.140625, 0.2, 107]
    m = MVFFeatureNet(in_channels=5, voxel_size=vs, pc_range=pr, cylinder_size=cs, cylinder_range=cr, num_filters=[48, 48], layer_nums=[0, 0, 0, 0],
                      ds_layer_strides=[1, 2, 2, 2], ds_num_filters=[48, 96, 192, 192], kernel_size=[3, 3, 3, 3], out_channels=256).cuda().train()
    with torch.no_grad():
        feat, rp, rc, _ = m.group_views(t, B)
    n, C = feat.shape[0], 192
    print(f"# sampling a view's map at the points, forward + backward (SingleView.sample, training): {n} points in {B} frames, {C} channels, MI355X")
    print("# node = pnx_bilinear_gather + pnx_bilinear_gather_backward (deterministic); torch = PNX_TRAIN_BILINEAR_HIP=0, the parent's path")
    gen = torch.Generator(device="cuda").manual_seed(0)
    wide = torch.randn((n, 3 * C), device="cuda", generator=gen)                   # the gradient of torch.cat((pointnet1, pv, cv)): the views get column slices
    total = {"node": 0.0, "torch": 0.0}
    for view, r, (H, W), col in ((m.pillarview, rp, (256, 256), 1), (m.cylinderview, rc, (13, 320), 2)):   # 2048 / 8; 100 -> 50 -> 25 -> 13, 2560 / 8
        x = torch.randn((B, H, W, C), device="cuda", generator=gen).permute(0, 3, 1, 2).requires_grad_(True)
        pos, go = view._pos_columns(feat), wide[:, col * C:(col + 1) * C]

        def step():
            x.grad = None
            view.sample(x, pos, r["coords"], r["unq_inv"]).backward(go)

        times, peak, grads = {"node": [], "torch": []}, {}, {}
        for it in range(a.warm + a.iters):
            for leg, switch in (("node", "1"), ("torch", "0")):                    # alternating, so that both see the same machine
                os.environ["PNX_TRAIN_BILINEAR_HIP"] = switch
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step()
                e1.record()
                torch.cuda.synchronize()
                if it >= a.warm:
                    times[leg].append(e0.elapsed_time(e1) * 1e3)
                    peak[leg] = max(peak.get(leg, 0), torch.cuda.max_memory_allocated() - base)
                grads[leg] = x.grad.detach().clone()
        diff = float((grads["node"] - grads["torch"]).abs().max() / grads["torch"].abs().max())
        for leg in ("node", "torch"):
            us = np.sort(np.asarray(times[leg]))
            total[leg] += float(np.median(us))
            print(f"{view.mode:8s} view, map {B} x {H} x {W} x {C}, {leg:5s}: median {np.median(us):8.1f} us  (min {us[0]:8.1f}, max {us[-1]:8.1f}, {len(us)} runs), "
                  f"peak above the inputs {peak[leg] / 2**20:7.1f} MiB")
        print(f"{view.mode:8s} view: max |grad(node) - grad(torch)| / max |grad| = {diff:.2e}; node / torch time = {np.median(times['node']) / np.median(times['torch']):.3f}")
    print(f"both views: node {total['node']:.1f} us, torch {total['torch']:.1f} us, node / torch = {total['node'] / total['torch']:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=180_000)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--train", action="store_true", help="the training leg: sampling forward + backward, node against the torch statement")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5)
    a = ap.parse_args()
    if a.train:
        return train_leg(a)
    B = a.batch
    pts = synth.make_batch("C4", B, "sweep", n=a.points)                    # Waymo-shaped sweep cloud, +-75.2 m
    t = torch.from_numpy(pts).cuda()
    n = t.shape[0]
    pr, vs = [-76.8, -76.8, -10.0, 76.8, 76.8, 10.0], [0.075, 0.075, 20]
    cr, cs = [-180, -10.0, 0, 180, 10.0, 107], [0.140625, 0.2, 107]
    print(f"# {n} points in {B} frames ({a.points} per frame), MI355X; wall time per call incl. the host sync for the counts")
    for name, g, cols in (("voxel 0.075 x 0.075 x 0.2 (drop)", ops.group_geom([-76.8, -76.8, -4.0, 76.8, 76.8, 4.0], [0.075, 0.075, 0.2], PNX_GROUP_VOXEL), 5),
                          ("pillar view 2048 x 2048 (clamp)", ops.group_geom(pr, vs, PNX_GROUP_PILLAR_CLAMP, pr), 10),
                          ("cylinder view 2560 x 100 (clamp)", ops.group_geom(cr, cs, PNX_GROUP_CYLINDER_CLAMP, pr), 10)):
        r = ops.group_points(t, B, g, want_mean=True)
        us = timed(lambda: ops.group_points(t, B, g, want_mean=True))
        by = 24 * n + r["Nk"] * (cols * 4 + 8) + r["G"] * (r["coords"].shape[1] * 4 + r["mean"].shape[1] * 4)
        print(f"pnx_group_points {name}: {us:7.1f} us   cells {r['G']}, kept {r['Nk']}, algorithmic {by / 1e6:.1f} MB -> {by / us / 1e3:.1f} GB/s")
    torch.manual_seed(0)
    m = MVFFeatureNet(in_channels=5, voxel_size=vs, pc_range=pr, cylinder_size=cs, cylinder_range=cr, num_filters=[48, 48], layer_nums=[2, 2, 2, 2],
                      ds_layer_strides=[1, 2, 2, 2], ds_num_filters=[48, 96, 192, 192], kernel_size=[3, 3, 3, 3], out_channels=256).cuda().eval()
    with torch.no_grad():
        feat, rp, rc, _ = m.group_views(t, B)
        us = timed(lambda: m.group_views(t, B))
        print(f"MVFFeatureNet.group_views (both groupings into one (N', 20) buffer): {us:7.1f} us")
        us = timed(lambda: m.pillarview.cell_features(feat, rp["unq_inv"], rp["G"]))
        print(f"SingleView PFN stack, eval (2 x pnx_pfn_layer_eval: 20 -> 24 (+) 24, 48 -> 48 + cell max): {us:7.1f} us  ({feat.shape[0]} points, {rp['G']} cells)")
        for label, dt in (("fp32 torch modules", None), ("HIP conv kernels bf16", torch.bfloat16), ("HIP conv kernels fp16", torch.float16)):
            m.use_hip_convs(dt)
            torch.cuda.reset_peak_memory_stats()
            ms = timed(lambda: m(t, batch_size=B), iters=5, warm=2) / 1e3
            print(f"MVFFeatureNet.forward, per-view sparse ResNets on {label}: {ms:8.2f} ms per {B} frames = {B / ms * 1e3:6.1f} frames/s, peak {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")


if __name__ == "__main__":
    main()
