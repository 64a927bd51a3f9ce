"""Voxel18 backbone on one MI355X: nuScenes-shaped sweep clouds (synth C2, 4 frames) through VoxelFeatureNet + SparseResNet3D
(channels 18/36/72/144, the geometry of configs/voxel18_aspp_nusc.yaml), random weights and BN statistics.

Prints the active sites per stage, ms per layer from HIP events (index, neighbour map and convolution separately), backbone ms per frame,
peak memory, and -- for context -- the same backbone as a torch statement on the GPU (fp32 gather + matmul + index_add_ per tap, neighbours
from torch.unique / searchsorted).  Usage: python tools/bench_voxel18.py [--frames 4] [--iters 5] [--dtype fp32|bf16|fp16]

--dtype bf16 / fp16 adds an arm that runs the backbone under use_half_precision(dtype): the two arms alternate forward by forward in one process,
each prints its own per-layer table, and the convolution phases are compared by the A/B rule (difference against three times the larger spread).

--train times forward + backward of the backbone in training mode instead (loss = sum of the dense output x a fixed random tensor): ms per step,
the split into forward convolutions / data gradients / weight gradients / everything else (index, maps, BatchNorm, ReLU, residual, dense: torch
glue included) from HIP events, peak memory, the weight-gradient workspace per stage, and the same torch statement under autograd, alternating
with the HIP step in one process (--torch-frames: fewer frames for the statement if it does not fit; its time is then also given per frame).

--train --dtype bf16 / fp16 times the training step under use_half_precision(dtype, training=True) against the fp32 training step instead of
the torch statement: the two arms alternate step by step in one process and each reports the same phases with its spread (min .. max over the
iterations), its wall time and the peak memory of one step of its own; the phases are compared by the A/B rule.

--train [--dtype bf16 / fp16] --fused-norm adds one more arm to that run: the last arm's step again under use_fused_norm (BatchNorm + residual +
ReLU as one HIP node).  The arm in front of it -- the same step without the option -- is its yardstick.  Every arm splits "everything else"
into the norm / residual / ReLU passes, forward (the name.rest phases) and backward (what runs in front of each convolution's backward), and
what remains (index, maps, dense scatter)."""
import argparse
import collections
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pillarnext_amd import synth  # noqa: E402
from pillarnext_amd.sparse3d import SparseResNet3D  # noqa: E402
from pillarnext_amd.voxel_encoder import VoxelFeatureNet  # noqa: E402

HALF = {"bf16": torch.bfloat16, "fp16": torch.float16}
NUSC = dict(voxel_size=[0.075, 0.075, 0.2], pc_range=[-50.4, -50.4, -5.0, 50.4, 50.4, 3.0])


def _keys(c, grid):
    D, H, W = grid
    c = c.long()
    return ((c[:, 0] * D + c[:, 1]) * H + c[:, 2]) * W + c[:, 3]


def torch_layer(coords, x, grid, w, k, s, p, subm, shift, residual=None):
    """fp32 torch statement of one layer (folded BN): the context number, not a reference."""
    og = tuple((n + 2 * pp - kk) // ss + 1 for n, kk, ss, pp in zip(grid, k, s, p))
    dev = x.device
    taps = [(a, b, d) for a in range(k[0]) for b in range(k[1]) for d in range(k[2])]
    c = coords.long()
    sv, pv = torch.tensor(s, device=dev), torch.tensor(p, device=dev)
    if subm:
        oc = coords
    else:
        cand = []
        for o in taps:
            t = c[:, 1:] + pv - torch.tensor(o, device=dev)
            ok = (t >= 0).all(1) & (t % sv == 0).all(1) & (t // sv < torch.tensor(og, device=dev)).all(1)
            cand.append(_keys(torch.cat([c[ok, :1], t[ok] // sv], 1), og))
        u = torch.unique(torch.cat(cand))
        D, H, W = og
        oc = torch.stack([u // (D * H * W), u // (H * W) % D, u // W % H, u % W], 1).int()
    skey, order = torch.sort(_keys(coords, grid))
    q = oc.long()
    out = torch.zeros((oc.shape[0], w.shape[0]), dtype=torch.float32, device=dev)
    for o in taps:
        pin = q[:, 1:] * sv - pv + torch.tensor(o, device=dev)
        inside = (pin >= 0).all(1) & (pin < torch.tensor(grid, device=dev)).all(1)
        key = _keys(torch.cat([q[:, :1], pin.clamp(min=0)], 1), grid)
        pos = torch.searchsorted(skey, key).clamp(max=skey.numel() - 1)
        sel = (inside & (skey[pos] == key)).nonzero()[:, 0]
        out.index_add_(0, sel, x[order[pos[sel]]] @ w[:, o[0], o[1], o[2], :].T)
    out = out + shift
    if residual is not None:
        out = out + residual
    return oc, torch.relu(out), og


def torch_backbone(bb, feats, coords, grid):
    def fold(conv, bn):
        a = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
        return conv.weight * a.view(-1, 1, 1, 1, 1), bn.bias - bn.running_mean * a

    x = feats
    for seq in bb.blocks:
        cv = seq[0].conv
        w0, b0 = fold(cv, seq[0].norm)
        coords, x, grid = torch_layer(coords, x, grid, w0, cv.kernel_size, cv.stride, cv.padding, False, b0)
        for blk in seq[1:]:
            w1, b1 = fold(blk.block1.conv, blk.block1.norm)
            w2, b2 = fold(blk.conv2, blk.norm2)
            k = blk.conv2.kernel_size
            _, y, _ = torch_layer(coords, x, grid, w1, k, (1, 1, 1), (1, 1, 1), True, b1)
            _, x, _ = torch_layer(coords, y, grid, w2, k, (1, 1, 1), (1, 1, 1), True, b2, residual=x)
    cv = bb.extra_conv[0]
    w, b = fold(cv, bb.extra_conv[1])
    coords, x, grid = torch_layer(coords, x, grid, w, cv.kernel_size, cv.stride, cv.padding, False, b)
    w, b = fold(bb.mapping.conv, bb.mapping.norm)
    _, x, _ = torch_layer(coords, x, grid, w, (1, 1, 1), (1, 1, 1), (0, 0, 0), True, b)
    return x


def _inputs(reader, B):
    pts = torch.from_numpy(synth.make_batch("C2", B, "sweep")).cuda()
    with torch.no_grad():
        feats, coords, grid = reader(pts, B)
    return pts, feats, coords, grid


def train(a, reader, bb):
    from pillarnext_amd import ops

    B = a.frames
    pts, feats, coords, grid = _inputs(reader, B)
    bb.train()
    print(f"# voxel18 backbone TRAINING step, synth C2 sweep x {B} frames ({pts.shape[0]} points), grid {tuple(int(g) for g in grid)}, {feats.shape[0]} voxels")
    with torch.no_grad():
        sets = bb.eval().forward_sparse(feats, coords, grid, B)
    bb.train()
    names = ["stage0", "stage1", "stage2", "stage3", "extra_conv", "mapping"]
    convs = [bb.blocks[0][1].conv2, bb.blocks[1][1].conv2, bb.blocks[2][1].conv2, bb.blocks[3][1].conv2, bb.extra_conv[0], bb.mapping.conv]
    print("active sites / weight-gradient workspace of one layer:", ", ".join(
        f"{n} {int(s[0].shape[0])} / {ops.sp3_wgrad_workspace_bytes(int(s[0].shape[0]), cv.weight[0, ..., 0].numel(), cv.in_channels, cv.out_channels) / 2**20:.1f} MiB"
        for n, s, cv in zip(names, sets, convs)))
    del sets
    proj = None

    def hip_step(profile):
        nonlocal proj
        bb.zero_grad(set_to_none=True)
        bb.profile = [] if profile else None
        out = bb(feats, coords, grid, B)
        if proj is None:
            proj = torch.randn(out.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        (out * proj).sum().backward()
        bb._tick("end")
        ev, bb.profile = bb.profile, None
        return ev

    if a.dtype != "fp32" or a.fused_norm:
        return train_arms(a, bb, hip_step, B)
    tb, tf_, tc, tg = (a.torch_frames or B), None, None, None
    if tb != B:
        _, tf_, tc, tg = _inputs(reader, tb)
    else:
        tf_, tc, tg = feats, coords, grid
    tproj = None

    def torch_step():
        nonlocal tproj
        bb.zero_grad(set_to_none=True)
        bb.eval()  # the statement the tool carries folds the running statistics; same convolutions, same graph shape
        x = torch_backbone(bb, tf_, tc, tuple(int(g) for g in tg))
        bb.train()
        if tproj is None:
            tproj = torch.randn(x.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        (x * tproj).sum().backward()

    def wall(fn, *args):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn(*args)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    hip_step(False), torch_step(), hip_step(False)  # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    hw, tw = [], []
    per = collections.defaultdict(float)
    for _ in range(a.iters):  # alternate: both see the same clocks and the same allocator state
        ms, ev = wall(hip_step, True)
        hw.append(ms)
        for (_, e0), (name, e1) in zip(ev[:-1], ev[1:]):
            per[name.rsplit(".", 1)[-1]] += e0.elapsed_time(e1) / a.iters
        tw.append(wall(torch_step)[0])
    peak = torch.cuda.max_memory_allocated() - base
    hw.sort(), tw.sort()
    phases = {"forward conv": per["conv"], "dgrad": per["dgrad"], "wgrad": per["wgrad"]}
    rest = sum(per.values()) - sum(phases.values())
    print("HIP step by phase (HIP events, mean of %d): " % a.iters + ", ".join(f"{k} {v:.2f} ms" for k, v in phases.items())
          + f", the rest (index, maps, BatchNorm / ReLU / residual, dense, autograd glue) {rest:.2f} ms")
    print(f"HIP forward + backward: {hw[len(hw) // 2]:.2f} ms per batch of {B} (median wall of {a.iters}; min {hw[0]:.2f}, max {hw[-1]:.2f}), "
          f"{hw[len(hw) // 2] / B:.2f} ms per frame")
    print(f"torch statement forward + backward (fp32 gather + matmul + index_add_ per tap under autograd, {tb} frames): {tw[len(tw) // 2]:.2f} ms per batch "
          f"(min {tw[0]:.2f}, max {tw[-1]:.2f}), {tw[len(tw) // 2] / tb:.2f} ms per frame")
    print(f"peak memory above inputs (both steps in the process): {peak / 2**30:.2f} GiB")


def train_arms(a, bb, hip_step, B):
    """The training steps of the arms alternating in one process: fp32, the 16-bit type of --dtype, and with --fused-norm the last of them again
    under use_fused_norm -- the arm in front of it, the same step without the option, is its yardstick."""
    arms = [("fp32", None, False)] + ([(a.dtype, HALF[a.dtype], False)] if a.dtype != "fp32" else [])
    if a.fused_norm:
        arms.append((arms[-1][0] + " + fused norm", arms[-1][1], True))

    def switch(dt, fused):
        if dt is None:
            bb.use_half_precision(None)
        else:
            bb.use_half_precision(dt, training=True)
        bb.use_fused_norm(fused)

    for _, dt, fused in arms:  # warm-up
        switch(dt, fused)
        hip_step(False), hip_step(False)
    torch.cuda.synchronize()
    # "the rest" = norm forward (the name.rest phases: BatchNorm + residual + ReLU; the 16-bit row conversions are inside the convolution phases) + norm
    # backward (what runs in front of each convolution's backward: the BatchNorm / ReLU / residual backward and autograd's glue; before the last
    # layer's also the dense gather and the loss) + everything else (index, maps, dense scatter)
    keys = ("forward conv", "dgrad", "wgrad", "the rest", "  norm forward", "  norm backward", "  everything else", "step (events)")
    runs = {n: {k: [] for k in keys} for n, _, _ in arms}
    walls = {n: [] for n, _, _ in arms}
    for _ in range(a.iters):  # the arms alternate: all see the same clocks and the same allocator state
        for arm, dt, fused in arms:
            switch(dt, fused)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev = hip_step(True)
            torch.cuda.synchronize()
            walls[arm].append((time.perf_counter() - t0) * 1e3)
            per = collections.defaultdict(float)
            for (_, e0), (name, e1) in zip(ev[:-1], ev[1:]):
                per[name.rsplit(".", 1)[-1]] += e0.elapsed_time(e1)
            total = sum(per.values())
            for k, v in (("forward conv", per["conv"]), ("dgrad", per["dgrad"]), ("wgrad", per["wgrad"])):
                runs[arm][k].append(v)
            rest = total - per["conv"] - per["dgrad"] - per["wgrad"]
            runs[arm]["the rest"].append(rest)
            runs[arm]["  norm forward"].append(per["rest"])
            runs[arm]["  norm backward"].append(per["bwd"])
            runs[arm]["  everything else"].append(rest - per["rest"] - per["bwd"])
            runs[arm]["step (events)"].append(total)
    peaks = {}
    for arm, dt, fused in arms:  # one step of each arm alone
        switch(dt, fused)
        bb.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        hip_step(False)
        torch.cuda.synchronize()
        peaks[arm] = torch.cuda.max_memory_allocated() - base
    switch(None, False)
    mean = {n: {k: sum(v) / len(v) for k, v in runs[n].items()} for n, _, _ in arms}
    for arm, _, _ in arms:
        w = sorted(walls[arm])
        print(f"## arm {arm}: HIP step by phase (HIP events, mean of {a.iters} [min .. max]; the rest = index, maps, BatchNorm / ReLU / residual, dense, "
              "autograd glue, 16-bit row conversions outside the gradients)")
        for k in keys:
            v = runs[arm][k]
            print(f"  {k:18s} {mean[arm][k]:8.2f} ms  [{min(v):.2f} .. {max(v):.2f}]")
        print(f"  forward + backward: {w[len(w) // 2]:.2f} ms per batch of {B} (median wall; min {w[0]:.2f}, max {w[-1]:.2f}), {w[len(w) // 2] / B:.2f} ms per frame; "
              f"peak memory of one step above inputs {peaks[arm] / 2**30:.2f} GiB")
    for (n0, _, _), (n1, _, _) in zip(arms[:-1], arms[1:]):
        print(f"# {n0} vs {n1}")
        for k in keys:
            spread = max(max(runs[n][k]) - min(runs[n][k]) for n in (n0, n1))
            d = mean[n0][k] - mean[n1][k]
            print(f"{k.strip()}: {n0} {mean[n0][k]:.2f} ms vs {n1} {mean[n1][k]:.2f} ms: difference {d:.2f} ms = {d / max(spread, 1e-9):.1f} x the larger spread "
                  f"({spread:.2f} ms; the A/B rule asks for more than 3 x), ratio {mean[n0][k] / max(mean[n1][k], 1e-9):.2f}")
        print(f"peak memory of one step: {n0} {peaks[n0] / 2**30:.2f} GiB vs {n1} {peaks[n1] / 2**30:.2f} GiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--dtype", choices=["fp32", "bf16", "fp16"], default="fp32",
                    help="bf16 / fp16: time SparseResNet3D.use_half_precision as well, its forwards (--train: training steps) alternating with the fp32 ones in this run")
    ap.add_argument("--train", action="store_true", help="time forward + backward in training mode")
    ap.add_argument("--torch-frames", type=int, default=0, help="--train: frames of the torch statement (default: --frames)")
    ap.add_argument("--fused-norm", action="store_true",
                    help="--train: one more arm, the last one again under SparseResNet3D.use_fused_norm, alternating with the others in this run")
    a = ap.parse_args()
    torch.manual_seed(0)
    B = a.frames
    pts = torch.from_numpy(synth.make_batch("C2", B, "sweep")).cuda()
    reader = VoxelFeatureNet(**NUSC).cuda()
    bb = SparseResNet3D([2, 2, 2, 2], [1, 2, 2, 2], [18, 36, 72, 144], 5).cuda().eval()
    with torch.no_grad():
        for m in bb.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.uniform_(0.5, 1.5), m.bias.uniform_(-0.2, 0.2), m.running_mean.uniform_(-0.2, 0.2), m.running_var.uniform_(0.5, 2.0)
    if a.train:
        return train(a, reader, bb)
    with torch.no_grad():
        feats, coords, grid = reader(pts, B)
        torch.cuda.synchronize()
        print(f"# voxel18 backbone, synth C2 sweep x {B} frames ({pts.shape[0]} points), grid {tuple(int(g) for g in grid)}, {feats.shape[0]} voxels")
        sets = bb.forward_sparse(feats, coords, grid, B)
        names = ["stage0", "stage1", "stage2", "stage3", "extra_conv", "mapping"]
        print("active sites:", ", ".join(f"{n} {int(s[0].shape[0])} (grid {s[2]})" for n, s in zip(names, sets)))
        arms = [("fp32", None)] + ([(a.dtype, HALF[a.dtype])] if a.dtype != "fp32" else [])
        for _, dt in arms:
            bb.use_half_precision(dt)
            for _ in range(2):
                bb(feats, coords, grid, B)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        per = {n: collections.defaultdict(float) for n, _ in arms}
        walls, convs = {n: [] for n, _ in arms}, {n: [] for n, _ in arms}
        for _ in range(a.iters):  # the arms alternate: both see the same clocks and the same allocator state
            for arm, dt in arms:
                bb.use_half_precision(dt)
                bb.profile = []
                t0 = time.perf_counter()
                bb(feats, coords, grid, B)
                torch.cuda.synchronize()
                walls[arm].append((time.perf_counter() - t0) * 1e3)
                ev = bb.profile
                conv = 0.0
                for (_, e0), (name, e1) in zip(ev[:-1], ev[1:]):
                    ms = e0.elapsed_time(e1)
                    per[arm][name] += ms / a.iters
                    conv += ms if name.endswith(".conv") else 0.0
                convs[arm].append(conv)
                bb.profile = None
        bb.use_half_precision(None)
        peak = torch.cuda.max_memory_allocated() - base
        for arm, _ in arms:
            w = sorted(walls[arm])
            if len(arms) > 1:
                print(f"## arm {arm}")
            print("ms per layer (HIP events, mean of %d):" % a.iters)
            kinds = collections.defaultdict(float)
            for name, ms in per[arm].items():
                print(f"  {name:28s} {ms:8.3f}")
                kinds[name.rsplit(".", 1)[-1]] += ms
            print("by phase:", ", ".join(f"{k} {v:.3f} ms" for k, v in kinds.items()))
            print(f"conv phase per iteration: min {min(convs[arm]):.3f}, max {max(convs[arm]):.3f} ms (spread {max(convs[arm]) - min(convs[arm]):.3f})")
            print(f"backbone: {w[len(w) // 2]:.2f} ms per batch (median wall; min {w[0]:.2f}, max {w[-1]:.2f}), {w[len(w) // 2] / B:.2f} ms per frame; "
                  f"event sum {sum(per[arm].values()):.2f} ms")
        if len(arms) > 1:
            (n0, _), (n1, _) = arms
            m0, m1 = sum(convs[n0]) / a.iters, sum(convs[n1]) / a.iters
            spread = max(max(convs[n]) - min(convs[n]) for n in (n0, n1))
            print(f"conv phase {n0} {m0:.3f} ms vs {n1} {m1:.3f} ms: difference {m0 - m1:.3f} ms = {(m0 - m1) / max(spread, 1e-9):.1f} x the larger spread "
                  f"({spread:.3f} ms; the A/B rule asks for more than 3 x), ratio {m0 / m1:.2f}")
        print(f"peak memory above inputs{' (all arms in the process)' if len(arms) > 1 else ''}: {peak / 2**30:.2f} GiB")
        torch_backbone(bb, feats, coords, tuple(int(g) for g in grid))
        torch.cuda.synchronize()
        tw = []
        for _ in range(max(1, a.iters // 2)):
            t0 = time.perf_counter()
            torch_backbone(bb, feats, coords, tuple(int(g) for g in grid))
            torch.cuda.synchronize()
            tw.append((time.perf_counter() - t0) * 1e3)
        tw.sort()
        print(f"torch statement (fp32 gather + matmul + index_add_ per tap): {tw[len(tw) // 2]:.2f} ms per batch, {tw[len(tw) // 2] / B:.2f} ms per frame")


if __name__ == "__main__":
    main()
