"""The packed-pixel form of the masked 128 -> 128 and 256 -> 256 convolutions (k_conv3x3_ldsx<..., PACK>, PNX_CONV_PACK=1, the default) against
the row form (PNX_CONV_PACK=0).  The library reads the switch once per process, so each setting runs in a child (this file as a script) that writes
a digest of every output; the digests must be equal -- per output element both forms run the same k-steps and MFMAs, so the results are
bit-identical -- and each child checks its outputs against fp32 F.conv2d.

Cases: the C2 sweep stage masks (stage 0's dilated set pooled to stages 1, 2, 3), tiles with exactly 32 / 33 / 1 active pixels, fully active tiles,
ragged right edges (180 and 360 are not multiples of 32), with and without residual, bf16 and f16, and a persistent output buffer written with two
different masks (no stale values may remain)."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child():
    import torch

    sys.path.insert(0, ROOT)
    from pillarnext_amd import ops, synth

    dev = "cuda"
    digests = {}

    def digest(t):
        return hashlib.sha256(t.contiguous().cpu().view(torch.int16).numpy().tobytes()).hexdigest()

    def check(name, x, w, bias, mask, res, y):
        ref = torch.nn.functional.conv2d(x.float(), w.float(), bias, 1, 1)
        if res is not None:
            ref = ref + res.float()
        ref = torch.relu(ref) * mask.unsqueeze(1)
        torch.testing.assert_close(y.float(), ref, rtol=1.6e-2, atol=2e-2, msg=lambda m: f"{name}: {m}")
        digests[name] = digest(y)

    def operands(c, B, H, W, dtype, seed, mask):
        g = torch.Generator(device=dev).manual_seed(seed)
        x = (torch.randn((B, c, H, W), device=dev, generator=g) * mask.unsqueeze(1)).to(dtype).contiguous(memory_format=torch.channels_last)
        w = (torch.randn((c, c, 3, 3), device=dev, generator=g) / 24).to(dtype)
        bias = torch.randn((c,), device=dev, generator=g)
        res = torch.randn((B, c, H, W), device=dev, generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
        return x, w, ops.conv3x3_pack_weights(w, dtype=dtype), bias, res

    def run(name, c, mask, dtype, seed):
        B, H, W = mask.shape
        x, w, wf, bias, res = operands(c, B, H, W, dtype, seed, mask)
        for r in (None, res):
            tag = f"{name} {c} {str(dtype)[6:]} res={r is not None}"
            check(tag, x, w, bias, mask, r, ops.conv3x3_masked(x, wf, bias, c, 1, mask, r, True))
            ws = ops.conv3x3_workspace(B, c, H, W, dev, dtype)  # persistent buffer + tile list, as the backbone runs them
            tiles = ops.conv_tile_list(mask, [ws[1]], ops.conv_tile_rows(c, c, 1))
            check(tag + " ws", x, w, bias, mask, r, ops.conv3x3_masked(x, wf, bias, c, 1, mask, r, True, out=ws, tiles=tiles))

    # C2 sweep masks of the stages
    cfg = synth.CONFIGS["C2"]
    rng, vox = cfg["pc_range"], cfg["voxel_size"]
    B = 2
    pts = torch.from_numpy(synth.make_batch("C2", B, "sweep")).to(dev)
    nx, ny = int(round((rng[3] - rng[0]) / vox[0])), int(round((rng[4] - rng[1]) / vox[1]))
    bi, xi, yi = pts[:, 0].long(), ((pts[:, 1] - rng[0]) / vox[0]).floor().long(), ((pts[:, 2] - rng[1]) / vox[1]).floor().long()
    ok = (xi >= 0) & (xi < nx) & (yi >= 0) & (yi < ny)
    occ = torch.zeros((B, ny, nx), dtype=torch.uint8, device=dev)
    occ[bi[ok], yi[ok], xi[ok]] = 1
    stage = [ops.mask_pool3(occ, 1)]
    for _ in range(3):
        stage.append(ops.mask_pool3(stage[-1], 2))
    assert [m.shape[-1] for m in stage[1:]] == [720, 360, 180]

    # edge cases on 24 x 180: 8 x 32 tiles (0, 0..5) with 32 / 33 / 1 / 256 active pixels, a half-active tile, a fully active ragged tile (20 columns);
    # row 8 onwards: a checkerboard (every group spans several rows) and a single pixel in the ragged corner
    edge = torch.zeros((2, 24, 180), dtype=torch.uint8, device=dev)
    edge[:, 0, 0:32] = 1
    edge[:, 0, 32:64] = 1
    edge[:, 5, 40] = 1
    edge[:, 3, 77] = 1
    edge[:, 0:8, 96:128] = 1
    edge[:, 0:8:2, 128:160] = 1
    edge[:, 0:8, 160:180] = 1
    edge[:, 8:16] = ((torch.arange(8, device=dev).view(8, 1) + torch.arange(180, device=dev).view(1, 180)) % 2).to(torch.uint8)
    edge[1, 23, 179] = 1

    for dtype in (torch.bfloat16, torch.float16):
        run("stage1", 128, stage[1], dtype, 1)
        run("stage2", 256, stage[2], dtype, 2)
        run("stage3", 256, stage[3], dtype, 3)
        for c in (128, 256):
            run("edge", c, edge, dtype, 4)
            # ragged 360-wide map, random half-density mask
            g = torch.Generator(device=dev).manual_seed(5)
            run("ragged360", c, (torch.rand((1, 40, 360), device=dev, generator=g) < 0.5).to(torch.uint8), dtype, 5)

        # one persistent buffer, two different masks: whatever frame 0 left must not survive frame 1
        for c in (128, 256):
            H = W = 180
            ws = ops.conv3x3_workspace(2, c, H, W, dev, dtype)
            for frame, m in enumerate((stage[3], stage[3].flip(2))):
                x, w, wf, bias, res = operands(c, 2, H, W, dtype, 10 + frame, m)
                tiles = ops.conv_tile_list(m, [ws[1]], ops.conv_tile_rows(c, c, 1))
                y = ops.conv3x3_masked(x, wf, bias, c, 1, m, res, True, out=ws, tiles=tiles)
                check(f"twice {c} {str(dtype)[6:]} frame {frame}", x, w, bias, m, res, y)
                digests[f"twice {c} {str(dtype)[6:]} frame {frame} dirty"] = digest(ws[1])
    torch.cuda.synchronize()
    print(json.dumps(digests))


def _run_child(pack):
    env = dict(os.environ, PNX_CONV_PACK=str(pack), PNX_CONV_PC="1")  # PNX_CONV_PC bit 1 would take these shapes to the producer / consumer kernel
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (pack, p.stdout[-1500:], p.stderr[-3000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_packed_pixel_convolution_is_bit_identical_to_row_form():
    pytest.importorskip("torch")
    packed, rows = _run_child(1), _run_child(0)
    assert len(packed) == len(rows) == 72
    diff = [k for k in rows if packed.get(k) != rows[k]]
    assert not diff, f"packed and row forms differ: {diff}"


if __name__ == "__main__":
    _child()
