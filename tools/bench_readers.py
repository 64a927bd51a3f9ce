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
medians of device-event times after warm-up, torch.cuda.max_memory_allocated above the resident inputs for each.  Its second leg (--leg points
runs it alone) times the reader's six per-point layers at the same geometry -- the PFN layers of both views (20 -> 24, 48 -> 48), pointnet1
(20 -> 192) and pointnet2 (576 -> 256 + per-pillar max) -- forward + backward, the fused node of csrc/point_layer_train.hip (PNX_TRAIN_POINT_HIP=1)
against the torch modules (=0, the parent's path), alternating in one run: median / min / max of device-event times and peak memory above the
inputs per layer and in total, the weight-gradient difference, and the verdict the switch's default follows; it writes --points-out.
--train --sparse-rows runs the view nets' leg instead: each view's sparse ResNet (configs/mvf18_aspp_waymo.yaml: 48 / 96 / 192 / 192, two basic blocks
per stage) + its sampling, forward + backward from the cell features, masked dense (the (B, H, W, C) canvas through models.py's blocks) against
SingleView.use_sparse_rows (rows of the active cells on csrc/sparse3d.hip), alternating in one run: device-event times, peak memory above the inputs,
the rows per stage; then the sampler alone, pnx_sp3_bilinear_gather + backward against the dense pair; it writes --views-out."""
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


def view_nets_leg(a):
    """The two view nets in training at full size, masked dense against sparse rows."""
    B = a.batch
    t = torch.from_numpy(synth.make_batch("C4", B, "sweep", n=a.points)).cuda()
    pr, vs = [-76.8, -76.8, -10.0, 76.8, 76.8, 10.0], [0.075, 0.075, 20]
    cr, cs = [-180, -10.0, 0, 180, 10.0, 107], [0.140625, 0.2, 107]
    torch.manual_seed(0)
    m = MVFFeatureNet(in_channels=5, voxel_size=vs, pc_range=pr, cylinder_size=cs, cylinder_range=cr, num_filters=[48, 48], layer_nums=[2, 2, 2, 2],
                      ds_layer_strides=[1, 2, 2, 2], ds_num_filters=[48, 96, 192, 192], kernel_size=[3, 3, 3, 3], out_channels=256).cuda().train()
    with torch.no_grad():
        feat, rp, rc, _ = m.group_views(t, B)
    n = feat.shape[0]
    gen = torch.Generator(device="cuda").manual_seed(0)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# the multi-view reader's view nets in training, forward + backward from the cell features (blocks + sampling): {n} points in {B} frames, MI355X")
    say("# rows = SingleView.use_sparse_rows (csrc/sparse3d.hip, pnx_sp3_bilinear_gather); dense = the (B, H, W, C) canvas through the masked-dense blocks, the parent's path")
    total = {"rows": 0.0, "dense": 0.0}
    for view, r, (H, W) in ((m.pillarview, rp, (2048, 2048)), (m.cylinderview, rc, (100, 2560))):
        P = r["coords"].shape[0]
        fv = torch.randn((P, 48), device="cuda", generator=gen).requires_grad_(True)
        go = torch.randn((n, 192), device="cuda", generator=gen)
        view.cell_features = lambda features, unq_inv, num_cells, fv=fv: fv
        with torch.no_grad():
            sets = view.use_sparse_rows().sparse_sets(fv.detach(), r["coords"], B, H, W, differentiable=False)
        say(f"{view.mode:8s} view, grid {B} x {H} x {W}: {P} active cells ({100.0 * P / (B * H * W):.2f} %); rows per stage "
            + ", ".join(f"{c.shape[0]} of {B * ix.grid[1] * ix.grid[2]}" for c, _, ix in sets))
        del sets

        def step():
            fv.grad = None
            view.zero_grad(set_to_none=True)
            view(feat, r["coords"], r["unq_inv"], np.array([H, W]), B).backward(go)

        times, peak, grads = {"rows": [], "dense": []}, {}, {}
        for it in range(a.warm + a.iters):
            for leg in ("rows", "dense"):                                          # alternating, so that both see the same machine
                view.use_sparse_rows(leg == "rows")
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step()
                e1.record()
                torch.cuda.synchronize()
                if it >= a.warm:
                    times[leg].append(e0.elapsed_time(e1))
                    peak[leg] = max(peak.get(leg, 0), torch.cuda.max_memory_allocated() - base)
                grads[leg] = (fv.grad.detach().clone(), view.blocks[0][0].conv.weight.grad.detach().clone())
        del view.cell_features
        for leg in ("rows", "dense"):
            ms = np.sort(np.asarray(times[leg]))
            total[leg] += float(np.median(ms))
            say(f"{view.mode:8s} view, {leg:5s}: median {np.median(ms):9.2f} ms  (min {ms[0]:9.2f}, max {ms[-1]:9.2f}, {len(ms)} runs), peak above the inputs {peak[leg] / 2**20:9.1f} MiB")
        d = [float((a_ - b_).abs().max() / b_.abs().max()) for a_, b_ in zip(grads["rows"], grads["dense"])]
        say(f"{view.mode:8s} view: max |d fv(rows) - d fv(dense)| / max = {d[0]:.2e}, first conv's dW {d[1]:.2e}; rows / dense time = "
            f"{np.median(times['rows']) / np.median(times['dense']):.3f}, peak memory = {peak['rows'] / peak['dense']:.4f}")
        # the sampler alone: the rows of the last stage against the dense map scattered from them
        with torch.no_grad():
            coords, x, ix = view.use_sparse_rows().sparse_sets(fv.detach(), r["coords"], B, H, W, differentiable=False)[-1]
        pos, ds = view._pos_columns(feat), int(view.ds_rate)
        img = torch.zeros((B, ix.grid[1], ix.grid[2], 192), device="cuda")
        cl = coords.long()
        img[cl[:, 0], cl[:, 2], cl[:, 3]] = x
        img = img.permute(0, 3, 1, 2)
        for name, fn in (("pnx_sp3_bilinear_gather          ", lambda: ops.sp3_bilinear_gather(x, ix, pos, view.bias, view.voxel_size, r["coords"], r["unq_inv"], ds)),
                         ("pnx_bilinear_gather              ", lambda: ops.bilinear_gather(img, pos, view.bias, view.voxel_size, r["coords"], r["unq_inv"], ds)),
                         ("pnx_sp3_bilinear_gather_backward ", lambda: ops.sp3_bilinear_gather_backward(go, coords, ix, pos, view.bias, view.voxel_size, r["coords"], r["unq_inv"], ds)),
                         ("pnx_bilinear_gather_backward     ", lambda: ops.bilinear_gather_backward(go, tuple(img.shape), pos, view.bias, view.voxel_size, r["coords"], r["unq_inv"], ds))):
            say(f"{view.mode:8s} view, {name} {x.shape[0]} rows / map {B} x {ix.grid[1]} x {ix.grid[2]} x 192, {n} points: {timed(fn):8.1f} us per call (wall, 20 calls)")
        del img
    say(f"both views: rows {total['rows']:.2f} ms, dense {total['dense']:.2f} ms, rows / dense = {total['rows'] / total['dense']:.3f}")
    if a.views_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.views_out)), exist_ok=True)
        with open(a.views_out, "w") as f:
            f.write("\n".join(lines) + "\n")


def point_layers_leg(a):
    """The six per-point layers of the mvf18 reader in training, node against torch, one layer at a time."""
    from torch.nn import functional as F

    B = a.batch
    t = torch.from_numpy(synth.make_batch("C4", B, "sweep", n=a.points)).cuda()
    pr, vs = [-76.8, -76.8, -10.0, 76.8, 76.8, 10.0], [0.075, 0.075, 20]
    cr, cs = [-180, -10.0, 0, 180, 10.0, 107], [0.140625, 0.2, 107]
    torch.manual_seed(0)
    m = MVFFeatureNet(in_channels=5, voxel_size=vs, pc_range=pr, cylinder_size=cs, cylinder_range=cr, num_filters=[48, 48], layer_nums=[0, 0, 0, 0],
                      ds_layer_strides=[1, 2, 2, 2], ds_num_filters=[48, 96, 192, 192], kernel_size=[3, 3, 3, 3], out_channels=256).cuda().train()
    with torch.no_grad():
        feat, rp, rc, _ = m.group_views(t, B)
    n = feat.shape[0]
    gen = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *shape: torch.randn(shape, device="cuda", generator=gen)  # noqa: E731
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# the multi-view reader's per-point layers in training, forward + backward: {n} points in {B} frames, {rp['G']} pillars, {rc['G']} cylinder cells, MI355X")
    say("# node = ops.PointLayer on csrc/point_layer_train.hip (fp32 MFMA, deterministic); torch = PNX_TRAIN_POINT_HIP=0, the parent's path "
        "(rocBLAS GEMM + BatchNorm1d + ReLU kernels + pnx_scatter_max)")

    def pfn_first(pfn, x, inv, G, node):          # -> cat [y, max[inv]] (n, 2 c), as SingleView.cell_features / PFNLayer.forward hand it on
        if node:
            y, g = ops.point_layer(x, pfn.linear, pfn.norm, inv, G, want_y=True, want_max=True)
            return torch.cat([y, g[inv]], dim=1)
        return pfn(x, inv, G)

    def pfn_last(pfn, x, inv, G, node):           # -> the cell feature (G, c)
        if node:
            return ops.point_layer(x, pfn.linear, pfn.norm, inv, G, want_y=False, want_max=True)[1]
        return ops.scatter_max(pfn(x, inv, G), inv, G)[0]

    def pn_plain(pn, x, inv, G, node):
        return ops.point_layer(x, pn.linear, pn.norm)[0] if node else F.relu(pn.norm(pn.linear(x)))

    def pn_max(pn, x, inv, G, node):
        if node:
            return ops.point_layer(x, pn.linear, pn.norm, inv, G, want_y=False, want_max=True)[1]
        return ops.scatter_max(F.relu(pn.norm(pn.linear(x))), inv, G)[0]

    pi, ci, PG, CG = rp["unq_inv"], rc["unq_inv"], rp["G"], rc["G"]
    layers = [("pillar pfn0   20 ->  24 (+max, cat)", pfn_first, m.pillarview.pfn_layers[0], feat, pi, PG, (n, 48)),
              ("pillar pfn1   48 ->  48 (cell max) ", pfn_last, m.pillarview.pfn_layers[1], rnd(n, 48).requires_grad_(True), pi, PG, (PG, 48)),
              ("cyl    pfn0   20 ->  24 (+max, cat)", pfn_first, m.cylinderview.pfn_layers[0], feat, ci, CG, (n, 48)),
              ("cyl    pfn1   48 ->  48 (cell max) ", pfn_last, m.cylinderview.pfn_layers[1], rnd(n, 48).requires_grad_(True), ci, CG, (CG, 48)),
              ("pointnet1     20 -> 192            ", pn_plain, m.pointnet1, feat, None, 0, (n, 192)),
              ("pointnet2    576 -> 256 (cell max) ", pn_max, m.pointnet2, rnd(n, 576).requires_grad_(True), pi, PG, (PG, 256))]
    runs = a.iters
    tot = {"node": np.zeros(runs), "torch": np.zeros(runs)}
    tot_peak = {"node": 0, "torch": 0}
    slower = []
    for name, fn, mod, x, inv, G, gshape in layers:
        go = rnd(*gshape)
        times, peak, grads = {"node": [], "torch": []}, {}, {}
        for it in range(a.warm + runs):
            for leg in ("node", "torch"):                                          # alternating, so that both see the same machine
                mod.zero_grad(set_to_none=True)
                if x.requires_grad:
                    x.grad = None
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(mod, x, inv, G, leg == "node").backward(go)
                e1.record()
                torch.cuda.synchronize()
                if it >= a.warm:
                    times[leg].append(e0.elapsed_time(e1) * 1e3)
                    peak[leg] = max(peak.get(leg, 0), torch.cuda.max_memory_allocated() - base)
                grads[leg] = mod.linear.weight.grad.detach().clone()
        diff = float((grads["node"] - grads["torch"]).abs().max() / grads["torch"].abs().max())
        for leg in ("node", "torch"):
            us = np.asarray(times[leg])
            tot[leg] += us
            tot_peak[leg] = max(tot_peak[leg], peak[leg])
            say(f"{name} {leg:5s}: median {np.median(us):9.1f} us  (min {us.min():9.1f}, max {us.max():9.1f}, {len(us)} runs), peak above the inputs {peak[leg] / 2**20:8.1f} MiB")
        ratio = float(np.median(times["node"]) / np.median(times["torch"]))
        if ratio > 1.0:
            slower.append(name.strip())
        say(f"{name} max |dW(node) - dW(torch)| / max |dW| = {diff:.2e}; node / torch time = {ratio:.3f}")
    for leg in ("node", "torch"):
        say(f"six layers, {leg:5s}: median {np.median(tot[leg]):9.1f} us  (min {tot[leg].min():9.1f}, max {tot[leg].max():9.1f}), largest peak above the inputs {tot_peak[leg] / 2**20:8.1f} MiB")
    gain = float(np.median(tot["torch"]) - np.median(tot["node"]))
    spread = float((tot["node"].max() - tot["node"].min()) + (tot["torch"].max() - tot["torch"].min()))
    on = gain > spread and tot_peak["node"] < tot_peak["torch"]
    say(f"torch - node = {gain:.1f} us against the two legs' max - min spread of {spread:.1f} us, node / torch = {np.median(tot['node']) / np.median(tot['torch']):.3f}; "
        f"peak memory {'lower' if tot_peak['node'] < tot_peak['torch'] else 'not lower'} on the node -> PNX_TRAIN_POINT_HIP defaults to {'on' if on else 'off'}")
    say("layers on which the node is slower than torch: " + (", ".join(slower) if slower else "none"))
    if a.points_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.points_out)), exist_ok=True)
        with open(a.points_out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=180_000)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--train", action="store_true", help="the training leg: sampling forward + backward, node against the torch statement")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--leg", choices=["all", "sampling", "points"], default="all", help="--train: the sampling leg, the per-point layers, or both")
    ap.add_argument("--points-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mvf_point_layers_train.txt"),
                    help="--train: where the per-point layers' leg writes its report ('' = nowhere)")
    ap.add_argument("--sparse-rows", action="store_true", help="--train: the view nets' leg, masked dense against SingleView.use_sparse_rows")
    ap.add_argument("--views-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mvf_view_nets_sparse.txt"),
                    help="--train --sparse-rows: where the view nets' leg writes its report ('' = nowhere)")
    a = ap.parse_args()
    if a.train and a.sparse_rows:
        view_nets_leg(a)
        return
    if a.train:
        if a.leg in ("all", "sampling"):
            train_leg(a)
        if a.leg in ("all", "points"):
            point_layers_leg(a)
        return
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
