"""GPU: the masked convolutions zero only the pixels that went stale (the written masks behind the row_dirty flags, include/pnx.h).

One persistent workspace per case goes through the mask sequence M1, M1, M2 (pixels removed inside rows that stay active), M3 (whole rows emptied,
others newly active), M1, with new input data at every call.  After every call
  * the whole buffer is bit-equal to the same call into a fresh workspace (same kernels) and exactly zero at every inactive site,
  * the flags are the row segments that hold an active site, the written masks behind them the current row masks.
That the zero stores are really skipped is shown without a timer: after the first M1 call a value is written from torch into a pixel that is
inactive in every mask but lies in an active segment.  The second M1 call must leave it alone (nothing went stale); with PNX_CONV_STALE=0, which
restores "zero every inactive pixel of a flagged segment", it must be gone.  The switch is read once per process, so that arm runs in a child (this
file as a script) and reports its digests: both arms must agree bit for bit.

Cases (bf16 and fp16, with and without residual, with and without a tile list), the smallest shapes that cross every seam:
  pc64     64 -> 64   k_conv3x3_pc packed,    2 x 37 x 70: 16-row tiles, a partial tile row of 5, a last tile of 6 columns
  ldsx128  128 -> 128 k_conv3x3_ldsx packed,  2 x 19 x 70: 8-row tiles, a partial tile row of 3, a last tile of 6 columns
  ldsx256  256 -> 256 k_conv3x3_ldsx packed,  2 x 19 x 70: two passes per tile.  A work unit is (tile, pass) and the grid is one workgroup per unit
           up to 512, so the 18 tiles' 36 units run on 36 different workgroups: the two passes of every tile meet in either order
  s2chain  64 -> 128 stride 2 (row form, 38 x 70 -> 19 x 35), then 128 -> 128 packed into the SAME workspace with the same mask: what launches 1 and 4
           of a backbone stage do.  The value is poked after the stride-2 call: the packed rewrite must find nothing to zero."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"pc64": (64, 64, 37, 70), "ldsx128": (128, 128, 19, 70), "ldsx256": (256, 256, 19, 70), "s2chain": (64, 128, 19, 35)}
POKE = 3.0


def masks(H, W):
    """M1, M2, M3 (B = 2, uint8, CPU) and the poked pixel (b, row, col): inactive in all three, in a segment that M1 and M2 keep active."""
    import torch

    g = torch.Generator().manual_seed(11)
    rows = torch.arange(H)
    m1 = (torch.rand((2, H, W), generator=g) < 0.4).to(torch.uint8)
    m1[:, rows % 5 == 4] = 0                                   # rows without a site
    m2 = m1 * (torch.rand((2, H, W), generator=g) < 0.5).to(torch.uint8)
    m2[:, :, 1::8] = m1[:, :, 1::8]                            # every segment of M1 keeps what it has in these columns: the rows stay active
    m3 = (torch.rand((2, H, W), generator=g) < 0.4).to(torch.uint8)
    m3[:, rows % 3 == 0] = 0                                   # whole rows emptied ...
    m3[:, rows % 5 == 4] = 1                                   # ... and the empty rows of M1 newly active, every pixel
    pr, pc = 1, W - 2                                          # in the ragged last segment
    for m in (m1, m2, m3):
        m[:, pr, pc] = 0
    m1[:, pr, pc - 1] = 1
    m2[:, pr, pc - 1] = 1
    assert bool((m1[:, rows % 3 == 0].sum() > 0)) and bool(((m1 == 1) & (m2 == 0)).any()) and bool((m2 <= m1).all())
    return [m1, m2, m3], (0, pr, pc)


def row_words(mask):
    """(B, H, segs) int32: bit p of a word = pixel p of the 32-pixel row segment is active -- what the written masks must be after a call."""
    import torch

    B, H, W = mask.shape
    segs = (W + 31) // 32
    m = torch.zeros((B, H, segs * 32), dtype=torch.int64, device=mask.device)
    m[:, :, :W] = mask
    v = (m.view(B, H, segs, 32) << torch.arange(32, device=mask.device)).sum(-1)
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)


def run_case(name, dtype, stale_on, digests=None):
    import torch

    from pillarnext_amd import ops

    dev = "cuda"
    cin, cout, H, W = CASES[name]
    chain = name == "s2chain"
    M, poke = masks(H, W)
    M = [m.to(dev) for m in M]
    seq = [0, 0, 1, 2, 0]
    g = torch.Generator(device=dev).manual_seed(7)

    def nhwc(c, h, w):
        return torch.randn((2, c, h, w), device=dev, generator=g).to(dtype).contiguous(memory_format=torch.channels_last)

    wf = ops.conv3x3_pack_weights((torch.randn((cout, cout if chain else cin, 3, 3), device=dev, generator=g) / 24).to(dtype), dtype=dtype)
    bias = torch.randn((cout,), device=dev, generator=g)
    if chain:
        wf_s2 = ops.conv3x3_pack_weights((torch.randn((cout, cin, 3, 3), device=dev, generator=g) / 24).to(dtype), dtype=dtype)
        xs_s2 = [nhwc(cin, 2 * H, 2 * W) for _ in seq]
    xs = [nhwc(cout if chain else cin, H, W) for _ in seq]
    res = nhwc(cout, H, W)
    th = ops.conv_tile_rows(cout, cout, 1)
    assert th == (16 if name == "pc64" else 8)

    def state(ws, mask, what):
        y, flags = ws
        assert not bool((y * (1 - mask).unsqueeze(1).to(dtype)).any()), (what, "a non-zero value at an inactive site")
        segs = (W + 31) // 32
        want = torch.zeros((2, H, segs * 32), dtype=torch.uint8, device=dev)
        want[:, :, :W] = mask
        assert torch.equal(flags, want.view(2, H, segs, 32).amax(-1)), (what, "flags differ from the active row segments")
        assert torch.equal(ops.row_dirty_written(flags, W), row_words(mask)), (what, "written masks differ from the row masks")

    def poked(y):
        b, r, c = poke
        return y[b, :, r, c].float()

    for use_res in (False, True):
        for use_tiles in (False, True):
            tag = f"{name} {str(dtype)[6:]} res={use_res} tiles={use_tiles}"
            r = res if use_res else None
            ws = ops.conv3x3_workspace(2, cout, H, W, dev, dtype)

            def packed(out, k, mask):
                tiles = ops.conv_tile_list(mask, [out[1]], th) if use_tiles else None
                return ops.conv3x3_masked(xs[k], wf, bias, cout, 1, mask, r, True, out=out, tiles=tiles)

            for k, mi in enumerate(seq):
                mask, what = M[mi], f"{tag} call {k} (M{mi + 1})"
                if chain:   # launch 1 of a stage: the stride-2 row form writes the buffer ...
                    y = ops.conv3x3_masked(xs_s2[k], wf_s2, bias, cout, 2, mask, None, True, out=ws)
                    fresh = ops.conv3x3_workspace(2, cout, H, W, dev, dtype)
                    assert torch.equal(y, ops.conv3x3_masked(xs_s2[k], wf_s2, bias, cout, 2, mask, None, True, out=fresh)), (what, "stride 2")
                    state(ws, mask, what + " stride 2")
                    if k == 0:
                        y[poke[0], :, poke[1], poke[2]] = POKE
                if not chain and k == 1:
                    ws[0][poke[0], :, poke[1], poke[2]] = POKE      # after the first M1 call, before the second
                if (chain and k == 0) or (not chain and k == 1):    # ... and the packed launch rewrites it with the same mask
                    y = packed(ws, k, mask)
                    got = poked(y)
                    if stale_on:
                        assert bool((got == POKE).all()), (what, "a pixel that did not go stale was zeroed", got.tolist()[:4])
                        y[poke[0], :, poke[1], poke[2]] = 0
                    else:
                        assert bool((got == 0).all()), (what, "PNX_CONV_STALE=0 must zero every inactive pixel of a flagged segment", got.tolist()[:4])
                else:
                    y = packed(ws, k, mask)
                fresh = ops.conv3x3_workspace(2, cout, H, W, dev, dtype)
                assert torch.equal(y, packed(fresh, k, mask)), (what, "differs from the same call into a fresh workspace")
                state(ws, mask, what)
                if mi == 1:
                    gone = ((M[0] == 1) & (mask == 0)).nonzero()[0].tolist()    # a pixel of M1 \ M2: written two calls ago, stale now
                    assert not bool(y[gone[0], :, gone[1], gone[2]].any()), (what, "a pixel of M1 \\ M2 kept its value", gone)
                if digests is not None:
                    digests[f"{tag} call {k}"] = hashlib.sha256(y.contiguous().cpu().view(torch.int16).numpy().tobytes()).hexdigest()
    torch.cuda.synchronize()


def _dtypes():
    import torch

    return {"bf16": torch.bfloat16, "f16": torch.float16}


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("name", list(CASES))
def test_only_stale_pixels_are_zeroed(name, dt):
    pytest.importorskip("torch")
    assert os.environ.get("PNX_CONV_STALE", "1") != "0" and os.environ.get("PNX_CONV_PACK") in (None, "3"), "the default forms are under test"
    run_case(name, _dtypes()[dt], True)


def _all(stale_on):
    digests = {}
    for name in CASES:
        for dtype in _dtypes().values():
            run_case(name, dtype, stale_on, digests)
    return digests


@pytest.mark.gpu
def test_switch_off_zeroes_every_idle_pixel_and_agrees_bit_for_bit():
    pytest.importorskip("torch")
    env = dict(os.environ, PNX_CONV_STALE="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    off, on = json.loads(p.stdout.strip().splitlines()[-1]), _all(True)
    assert len(off) == len(on) == len(CASES) * 2 * 4 * 5
    diff = [k for k in on if off.get(k) != on[k]]
    assert not diff, f"PNX_CONV_STALE=0 and the default differ: {diff[:8]}"


# ---------------------------------------------------------------------------------------------------------------- model level
@pytest.mark.gpu
def test_fused_model_frames_a_b_a_c_equal_fresh_models():
    """The 72 x 64 detector of tests/test_fused_schedule_cpu.py on the launch-plan path: frame batches A, B, A, C through ONE model; every step's stage
    outputs and detections are bit-equal to a fresh model's (same kernels, same schedule: nothing of an earlier frame may show)."""
    torch = pytest.importorskip("torch")
    import numpy as np

    from pillarnext_amd import ops
    from pillarnext_amd.models import FusedPillarNeXt, build_pillarnext_b

    pc_range, voxel = (-6.4, -7.2, -5.0, 6.4, 7.2, 3.0), (0.2, 0.2, 8.0)
    torch.manual_seed(5)
    torch.backends.cudnn.deterministic = True  # MIOpen (the neck's dilated convolutions): deterministic algorithms; the HIP path is deterministic by construction
    det = build_pillarnext_b(pc_range, voxel, tasks=[["car"], ["truck", "bus"]], with_iou_head=True).cuda().eval()

    def frame(seed, n):
        rng = np.random.default_rng(seed)
        centres = rng.uniform([-5.5, -6.3], [5.5, 6.3], size=(6, 2))                       # clusters: a sparse, frame-dependent occupancy
        xy = centres[rng.integers(0, 6, size=n)] + rng.normal(0, 0.5, size=(n, 2))
        pts = np.concatenate([rng.integers(0, 2, size=(n, 1)), xy, rng.uniform(-3, 1, size=(n, 1)), rng.uniform(0, 1, size=(n, 2))], axis=1)
        pts = pts[(np.abs(pts[:, 1]) < 6.39) & (np.abs(pts[:, 2]) < 7.19)]
        return torch.from_numpy(pts[np.argsort(pts[:, 0], kind="stable")].astype(np.float32)).cuda()

    A, Bf, C = frame(1, 900), frame(2, 500), frame(3, 1300)

    def step(fused, pts):
        with torch.no_grad():
            dets = fused({"points": pts, "token": ["a", "b"], "batch_size": 2})
        torch.cuda.synchronize()
        assert any(isinstance(k, tuple) and k[0] == "plan_bb" for k in fused._ws), "the launch-plan path was not taken"
        return {k: v for k, v in fused._ws.items() if isinstance(k, tuple) and isinstance(k[0], int)}, dets   # (stage, B, H, W, device): its 3 buffers

    def make():
        fused = FusedPillarNeXt(det, hip_conv=True).cuda().eval()
        assert fused.sparse_ws and fused._plan_ok()
        return fused

    seq = make()
    for i, pts in enumerate((A, Bf, A, C)):
        stages, dets = step(seq, pts)
        ref_stages, ref_dets = step(make(), pts)
        assert sorted(k[0] for k in stages) == [0, 1, 2, 3] and set(stages) == set(ref_stages)
        for key in stages:
            for j, ((y, fl), (ry, rfl)) in enumerate(zip(stages[key], ref_stages[key])):   # buffer 1 holds the stage's output, 0 and 2 its last block's inputs
                assert bool(y.any()) and torch.equal(y, ry), (i, key[0], j, "workspace state leaked into a stage buffer")
                assert torch.equal(fl, rfl) and torch.equal(ops.row_dirty_written(fl, key[3]), ops.row_dirty_written(rfl, key[3])), (i, key[0], j)
        assert set(dets) == set(ref_dets) == {"a", "b"}
        for tok in dets:
            for k, v in dets[tok].items():
                if torch.is_tensor(v):
                    r = ref_dets[tok][k]
                    same = v.shape == r.shape and v.dtype == r.dtype and torch.equal(v.contiguous().view(torch.uint8), r.contiguous().view(torch.uint8))
                    if not same:
                        print(f"[stale-model] step {i} {tok} {k}: shapes {tuple(v.shape)} / {tuple(r.shape)}"
                              + (f", {int((v != r).sum())} values differ, max |diff| {float((v.float() - r.float()).abs().max()):.3g}" if v.shape == r.shape else ""))
                    assert same, (i, tok, k, "detections differ from a fresh model's")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    print(json.dumps(_all(os.environ.get("PNX_CONV_STALE", "1") != "0")))
