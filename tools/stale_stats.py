#!/usr/bin/env python3
"""CPU: how many zero lines the packed masked convolutions store per active line, from the benchmark's own clouds.

Two consecutive frame batches A, B of synth.make_batch("C2", batch, "sweep"); per backbone stage the active set is the model's: occupancy -> 3x3
dilation (stage 0's entry convolution) -> one 3x3 stride-2 pool per further stage.  A "line" is one pixel of one output buffer (128 B per 64
channels).  Per active line of the launch, the zero lines stored
  same mask, before   a launch that rewrites a buffer written with the same mask (launches 4 and 5 of a stage) and re-zeroes every inactive pixel of
                      every flagged 32-pixel row segment -- what the kernels did before the written masks (PNX_CONV_STALE=0)
  next batch, before  the same rule for a launch of batch B into a buffer that batch A wrote (launches 1 to 3): the inactive pixels of B's active
                      segments that A had flagged, plus the whole of A's segments that B leaves empty
  stale               the pixels active in A and not in B: all that has to be zeroed.  With the written masks launches 1 to 3 store these and
                      launches 4 and 5 store none.
and the bytes per 12-frame step they stand for (five stride-1-or-entry launches per stage, 2 bytes x channels per line)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pillarnext_amd import synth  # noqa: E402

CHANNELS = (64, 128, 256, 256)


def pool3(m, stride):
    """3x3 max pool, pad 1, of a (B, H, W) 0/1 map"""
    B, H, W = m.shape
    p = np.zeros((B, H + 2, W + 2), dtype=m.dtype)
    p[:, 1:-1, 1:-1] = m
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= p[:, dy:dy + H, dx:dx + W]
    return out[:, ::stride, ::stride]


def stage_masks(batch, frame0):
    cfg = synth.CONFIGS["C2"]
    r, v = cfg["pc_range"], cfg["voxel_size"]
    pts = synth.make_batch("C2", batch, "sweep", frame0=frame0)
    nx, ny = int(round((r[3] - r[0]) / v[0])), int(round((r[4] - r[1]) / v[1]))
    bi, xi, yi = pts[:, 0].astype(np.int64), np.floor((pts[:, 1] - r[0]) / v[0]).astype(np.int64), np.floor((pts[:, 2] - r[1]) / v[1]).astype(np.int64)
    ok = (xi >= 0) & (xi < nx) & (yi >= 0) & (yi < ny)
    occ = np.zeros((batch, ny, nx), dtype=np.uint8)
    occ[bi[ok], yi[ok], xi[ok]] = 1
    masks = [pool3(occ, 1)]
    for _ in range(3):
        masks.append(pool3(masks[-1], 2))
    return masks


def segments(m):
    """(B, H, segs, 32) view of the mask padded to whole segments, and the number of in-image pixels of every segment column"""
    B, H, W = m.shape
    segs = (W + 31) // 32
    p = np.zeros((B, H, segs * 32), dtype=np.int64)
    p[:, :, :W] = m
    width = np.minimum(32, W - 32 * np.arange(segs))
    return p.reshape(B, H, segs, 32), width


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--step-frames", type=int, default=12, help="frames per benchmark step the byte columns are scaled to")
    a = ap.parse_args()
    A, Bm = stage_masks(a.batch, 0), stage_masks(a.batch, a.batch)
    print("stage  size  channels  active px  active segs | zero lines per active line: same mask, before | next batch, before | stale || GB per step: before | after")
    tot = [0.0, 0.0]
    for s, (ma, mb, ch) in enumerate(zip(A, Bm, CHANNELS)):
        sa, width = segments(ma)
        sb, _ = segments(mb)
        na, nb_ = sa.sum(-1), sb.sum(-1)                      # active pixels per segment
        act = float(nb_.sum())
        same = float((width - nb_)[nb_ > 0].sum()) / act
        w3 = np.broadcast_to(width, nb_.shape)
        nxt = float((w3 - nb_)[(nb_ > 0) & (na > 0)].sum() + w3[(nb_ == 0) & (na > 0)].sum()) / act
        stale = float(((sa == 1) & (sb == 0)).sum()) / act
        line = 2 * ch
        per_step = act / a.batch * a.step_frames * line       # bytes of the active lines of one launch of a step
        n_packed = 5 if s == 0 else 4                         # stage 0: five packed launches; later stages: the entry convolution is a row form
        before = per_step * (2 * same + (n_packed - 2) * nxt) / 1e9
        after = per_step * (n_packed - 2) * stale / 1e9
        tot[0] += before
        tot[1] += after
        print(f"{s:5d} {ma.shape[-1]:5d} {ch:9d} {mb.mean():10.3f} {(nb_ > 0).mean():12.3f} | {same:45.2f} | {nxt:18.2f} | {stale:5.2f} || {before:19.2f} | {after:5.2f}")
    print(f"all stages: {tot[0]:.2f} GB of zero stores per step before, {tot[1]:.2f} GB after")


if __name__ == "__main__":
    main()
