"""The packed-pixel form of the masked 64 -> 64 convolution (k_conv3x3_pc<64, 64, ..., PACK>, PNX_CONV_PACK bit 1, on by default) against the row form
(PNX_CONV_PACK=1: bit 0 only, what the library did before the 64-channel form existed).  The library reads the switch once per process, so each setting
runs in a child (this file as a script) that writes a digest of every output; the digests must be equal -- per output element both forms run the same
k-steps and MFMAs, so the results are bit-identical -- and each child checks its outputs against fp32 F.conv2d.

Cases, bf16 and f16, with and without residual, direct (a fresh uninitialised output) and through a persistent workspace + tile list:
  edge       2 x 32 x 180: two tile rows of 16, ragged right edge of 20 columns; 16 x 32 tiles with exactly 32, 33, 1 and 512 active pixels, a half-active
             tile, a fully active ragged tile, a checkerboard (every group of 32 spans several rows), a single pixel in the last row and column
  ragged360  1 x 40 x 360, random half density; 40 is not a multiple of 16
  stage0     the C2 sweep's dilated stage-0 mask, 2 frames at 1440^2 (the tile-ticket and list paths go past one tile per workgroup only at that size)
  twice      one persistent buffer written with a mask and then its flip: nothing of frame 0 may survive frame 1
Where a workspace is used its row_dirty array is digested as well."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 64


def _child():
    import torch

    sys.path.insert(0, ROOT)
    from pillarnext_amd import ops, synth

    dev = "cuda"
    digests = {}

    def digest(t):
        t = t.contiguous().cpu()
        return hashlib.sha256((t if t.dtype == torch.uint8 else t.view(torch.int16)).numpy().tobytes()).hexdigest()

    def reference(x, w, bias):  # fp32, before residual / ReLU / mask: computed once per set of operands
        return torch.nn.functional.conv2d(x.float(), w.float(), bias, 1, 1)

    def check(name, base, mask, res, y):
        ref = base if res is None else base + res.float()
        ref = torch.relu(ref) * mask.unsqueeze(1)
        torch.testing.assert_close(y.float(), ref, rtol=1.6e-2, atol=2e-2, msg=lambda m: f"{name}: {m}")
        digests[name] = digest(y)

    def operands(B, H, W, dtype, seed, mask):
        g = torch.Generator(device=dev).manual_seed(seed)
        x = (torch.randn((B, C, H, W), device=dev, generator=g) * mask.unsqueeze(1)).to(dtype).contiguous(memory_format=torch.channels_last)
        w = (torch.randn((C, C, 3, 3), device=dev, generator=g) / 24).to(dtype)
        bias = torch.randn((C,), device=dev, generator=g)
        res = torch.randn((B, C, H, W), device=dev, generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
        return x, w, ops.conv3x3_pack_weights(w, dtype=dtype), bias, res

    def run(name, mask, dtype, seed):
        B, H, W = mask.shape
        x, w, wf, bias, res = operands(B, H, W, dtype, seed, mask)
        base = reference(x, w, bias)
        for r in (None, res):
            tag = f"{name} {str(dtype)[6:]} res={r is not None}"
            check(tag, base, mask, r, ops.conv3x3_masked(x, wf, bias, C, 1, mask, r, True))
            ws = ops.conv3x3_workspace(B, C, H, W, dev, dtype)  # persistent buffer + tile list, as the backbone runs them
            tiles = ops.conv_tile_list(mask, [ws[1]], ops.conv_tile_rows(C, C, 1))
            check(tag + " ws", base, mask, r, ops.conv3x3_masked(x, wf, bias, C, 1, mask, r, True, out=ws, tiles=tiles))
            digests[tag + " ws dirty"] = digest(ws[1])

    assert ops.conv_tile_rows(C, C, 1) == 16

    # the C2 sweep's dilated stage-0 mask
    cfg = synth.CONFIGS["C2"]
    rng, vox = cfg["pc_range"], cfg["voxel_size"]
    B = 2
    pts = torch.from_numpy(synth.make_batch("C2", B, "sweep")).to(dev)
    nx, ny = int(round((rng[3] - rng[0]) / vox[0])), int(round((rng[4] - rng[1]) / vox[1]))
    bi, xi, yi = pts[:, 0].long(), ((pts[:, 1] - rng[0]) / vox[0]).floor().long(), ((pts[:, 2] - rng[1]) / vox[1]).floor().long()
    ok = (xi >= 0) & (xi < nx) & (yi >= 0) & (yi < ny)
    occ = torch.zeros((B, ny, nx), dtype=torch.uint8, device=dev)
    occ[bi[ok], yi[ok], xi[ok]] = 1
    stage0 = ops.mask_pool3(occ, 1)
    assert tuple(stage0.shape) == (2, 1440, 1440)

    # edge cases on 32 x 180: 16 x 32 tiles (0, 0..5) with 32 / 33 / 1 / 512 active pixels, a half-active tile, a fully active ragged tile (20 columns);
    # rows 16..23: a checkerboard (every group spans several rows); image 1: a single pixel in the ragged corner, alone in its row
    edge = torch.zeros((2, 32, 180), dtype=torch.uint8, device=dev)
    edge[:, 0, 0:32] = 1
    edge[:, 0, 32:64] = 1
    edge[:, 5, 40] = 1
    edge[:, 3, 77] = 1
    edge[:, 0:16, 96:128] = 1
    edge[:, 0:16:2, 128:160] = 1
    edge[:, 0:16, 160:180] = 1
    edge[:, 16:24] = ((torch.arange(8, device=dev).view(8, 1) + torch.arange(180, device=dev).view(1, 180)) % 2).to(torch.uint8)
    edge[1, 31, 179] = 1
    per_tile = edge[0, 0:16, 0:160].reshape(16, 5, 32).sum((0, 2)).tolist()
    assert per_tile == [32, 33, 1, 512, 256] and int(edge[0, 0:16, 160:].sum()) == 16 * 20

    g = torch.Generator(device=dev).manual_seed(5)
    ragged = (torch.rand((1, 40, 360), device=dev, generator=g) < 0.5).to(torch.uint8)
    crop = stage0[:, 540:900, 540:900].contiguous()  # the dense middle of the sweep, 360 = 22.5 tile rows

    for dtype in (torch.bfloat16, torch.float16):
        run("edge", edge, dtype, 4)
        run("ragged360", ragged, dtype, 5)
        run("stage0", stage0, dtype, 1)
        # one persistent buffer, two different masks: whatever frame 0 left must not survive frame 1
        H = W = 360
        ws = ops.conv3x3_workspace(2, C, H, W, dev, dtype)
        for frame, m in enumerate((crop, crop.flip(2).contiguous())):
            x, w, wf, bias, res = operands(2, H, W, dtype, 10 + frame, m)
            tiles = ops.conv_tile_list(m, [ws[1]], ops.conv_tile_rows(C, C, 1))
            y = ops.conv3x3_masked(x, wf, bias, C, 1, m, res, True, out=ws, tiles=tiles)
            check(f"twice {str(dtype)[6:]} frame {frame}", reference(x, w, bias), m, res, y)
            digests[f"twice {str(dtype)[6:]} frame {frame} dirty"] = digest(ws[1])
    torch.cuda.synchronize()
    print(json.dumps(digests))


def _run_child(pack):
    env = dict(os.environ, PNX_CONV_PC="1")  # bit 0: 64 -> 64 on the producer / consumer kernel, which holds the packed form
    env.pop("PNX_CONV_PACK", None)
    if pack is not None:
        env["PNX_CONV_PACK"] = str(pack)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (pack, p.stdout[-1500:], p.stderr[-3000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_packed_pixel_convolution_64_is_bit_identical_to_row_form():
    pytest.importorskip("torch")
    packed, rows = _run_child(None), _run_child(1)
    assert len(packed) == len(rows) == 44  # per dtype: 3 masks x 2 (residual) x 3 (direct, workspace, its row_dirty) + 2 frames x 2
    diff = [k for k in rows if packed.get(k) != rows[k]]
    assert not diff, f"packed and row forms differ: {diff}"


if __name__ == "__main__":
    _child()
