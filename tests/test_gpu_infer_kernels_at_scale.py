"""GPU: the inference convolution kernels (csrc/conv3x3.hip and the headers it includes: conv_rows.h, conv_s2.h, sephead.h, conv_pc.h) at the shapes
bench.py runs them at, one layer at a time, against fp64 on the SAME bf16 / f16 operands the kernel read.

The other inference tests use maps of 18 to 140 tiles per launch: every persistent workgroup takes one tile and exits, no ticket of the 64-slot g_tile_ctr
ring is drawn, the depth-2 tile pipeline never iterates and the LDS words double-buffered by iteration parity are never reused; the tests that do reach many
tiles per workgroup compare with fp32 F.conv2d at rtol 1.6e-2 / atol 2e-2, which passes an output that lost a tap on a few tiles.  Every case below first
restates its launch's work split in Python (launch_lds, launch_ldsx, launch_pc, launch_s2, launch_direct, launch_deconv, launch_sephead: each names the
constants of the source it mirrors) and asserts (_reach) that its shape and mask reach the path it is there for: a case that does not reach it fails.

References: fp64 on the GPU, gathered at the active sites and chunked (_gconv_half: _gconv of tests/test_gpu_train_kernels_at_scale.py gathering from the
half-precision map, so that a 12 x 64 x 1440^2 map never exists in fp64); bias, residual, ReLU and mask in fp64 too.  Bars (_check):
  per element   |got - ref| <= BF_REL * sum|terms| + out_round * |ref| + TINY, sum|terms| including |bias| and |residual|, out_round = 2^-8 (bf16) / 2^-11
                (f16): one output rounding;
  Frobenius     over the active set, at most 1.25 x that of the reference rounded ONCE to the output type (measured in the test, no kernel involved);
  signed mean   |mean(got - ref)| <= BF_REL * mean(sum|terms|) + |mean(round(ref) - ref)|: what the per-element bar implies, nothing looser.
Inactive sites are compared with zero (bit pattern), over the whole buffer; no element is left out.  -rP prints the measured figures per case."""
import os
import subprocess
import sys
from collections import namedtuple

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_train_kernels_at_scale import BF_REL, CHUNK, TINY, _pad1, _taps  # noqa: E402  (the training module's bars and gather helpers, unchanged)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_ROUND = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}      # one rounding of an 8- / 11-bit significand
FRO_MARGIN = 1.25                                                       # fp32 accumulation on top of the one output rounding (bounded by BF_REL per element)


# ---------------------------------------------------------------------------------------------------- work splits of the launches

Split = namedtuple("Split", "units grid static nh th")
"""units: work units when every tile is walked; grid: workgroups (gridDim.x = G); static: indices dealt without a ticket under a mask (None: the launch never
draws one); nh: units per tile; th: rows of a tile"""


def _ntiles(B, H, W, th):
    return B * -(-H // th) * -(-W // 32)


def launch_lds(B, H, W):
    """conv3x3.hip launch_lds<COUT> / conv_rows.h k_conv3x3_lds: tiles of LDS_TH (16) rows x 32 pixels, grid = min(tiles, 256 * 2); sched_next2: indices 0..2G-1 static"""
    n = _ntiles(B, H, W, 16)
    g = min(n, 512)
    return Split(n, g, 2 * g, 1, 16)


def launch_ldsx(B, H, W, cout):
    """conv_rows.h launch_ldsx<CIN, COUT> / k_conv3x3_ldsx: tiles of L128_TH (8) rows, units = tiles x NH, NH = ceil(COUT / 128) passes, unit = tile * NH +
    pass, grid = min(units, 512); sched_next2: indices 0..2G-1 static"""
    nh = -(-cout // 128)
    n = _ntiles(B, H, W, 8) * nh
    g = min(n, 512)
    return Split(n, g, 2 * g, nh, 8)


def launch_pc(B, H, W, cin):
    """conv_pc.h launch_pc<CIN, COUT> / k_conv3x3_pc: tiles of TH = 16 (CIN 64) / 8 rows, grid = min(tiles, 256); tile_index: n < 3 static, tickets from 3G"""
    th = 16 if cin == 64 else 8
    n = _ntiles(B, H, W, th)
    g = min(n, 256)
    return Split(n, g, 3 * g, 1, th)


def launch_s2(B, Ho, Wo):
    """conv_s2.h launch_s2 / k_conv3x3_s2: OUTPUT tiles of S2_TH (4) rows, grid = min(tiles, 512); sched_next: the first tile static, tickets from G"""
    n = _ntiles(B, Ho, Wo, 4)
    g = min(n, 512)
    return Split(n, g, g, 1, 4)


def launch_direct(B, Ho, Wo, cout):
    """conv3x3.hip launch<CIN, COUT, STRIDE> / k_conv3x3: one tile of NT rows (4 if COUT / 32 <= 2 else 2) per WAVE, 4 tiles per workgroup,
    grid = min(ceil(tiles / 4), 512), static stride 4 G; no ticket.  units / grid here are tiles and waves"""
    nt = 4 if cout // 32 <= 2 else 2
    n = _ntiles(B, Ho, Wo, nt)
    return Split(n, 4 * min(-(-n // 4), 512), None, 1, nt)


def launch_deconv(B, H, W):
    """conv3x3.hip pnx_deconv2x2 / sephead.h k_deconv2x2_64: one 32-pixel input row segment per WAVE, grid = min(ceil(segments / 4), 512); units / grid: segments, waves"""
    n = B * H * -(-W // 32)
    return Split(n, 4 * min(-(-n // 4), 512), None, 1, 1)


def launch_sephead(B, H, W):
    """sephead.h launch_sephead<NBR> / k_sephead_out<NBR, 8>: tiles of 8 rows x 32 pixels, grid = min(tiles, 768), static round-robin"""
    n = _ntiles(B, H, W, 8)
    return Split(n, min(n, 768), None, 1, 8)


def _split_of(cin, cout, stride, B, Ho, Wo, sel="default"):
    """the launch pnx_conv3x3 picks: stride 1 -- 64 -> 64 on the producer / consumer kernel (PNX_CONV_PC bit 0, the default; "pc0": launch_lds<64>),
    128 -> 128 / 256 -> 256 / 256 -> 64 on launch_ldsx; stride 2 without residual -- launch_s2; sel "direct" (PNX_CONV_DIRECT) -- k_conv3x3"""
    if sel == "direct":
        return launch_direct(B, Ho, Wo, cout)
    if stride == 2:
        return launch_s2(B, Ho, Wo)
    if cin == 64 and cout == 64:
        return launch_lds(B, Ho, Wo) if sel == "pc0" else launch_pc(B, Ho, Wo, 64)
    if cin == 64:
        return launch_lds(B, Ho, Wo)
    return launch_ldsx(B, Ho, Wo, cout)


def _tile_nonempty(mask_u8, th):
    """per th x 32 tile in (b, ty, tx) order: does it hold an active site"""
    B, H, W = mask_u8.shape
    ty, tx = -(-H // th), -(-W // 32)
    m = torch.zeros((B, ty * th, tx * 32), dtype=torch.uint8, device=mask_u8.device)
    m[:, :H, :W] = mask_u8
    return (m.view(B, ty, th, tx, 32) != 0).any(dim=4).any(dim=2).reshape(-1)


def _reach(tag, sp, units, want):
    """`units` work units go to sp.grid workgroups (waves).  iterate: some workgroup takes a second unit (the pipeline's index B); tickets: units past the
    static deal; reuse: >= 4 units per workgroup, so both parities of every double-buffered word (and all four s_tile slots of conv_pc.h) are reused"""
    print(f"{tag}: {units} units on {sp.grid} workgroups ({units / sp.grid:.1f} each), static deal {sp.static}: {want}")
    assert want and set(want.split("+")) <= {"iterate", "tickets", "reuse"}, want
    assert units > sp.grid, (tag, "no workgroup takes a second unit", units, sp.grid)
    if "tickets" in want:
        assert sp.static is not None and units > sp.static, (tag, "no ticket is drawn", units, sp.static)
    if "reuse" in want:
        assert units >= 4 * sp.grid, (tag, "fewer than 4 units per workgroup", units, sp.grid)


# ---------------------------------------------------------------------------------------------------- operands

def _c2_masks(B):
    """uint8 active sets of the four backbone stages at the C2 geometry, sweep occupancy, built as tests/test_gpu_conv_pack.py builds them: the pillars of
    synth.make_batch("C2", B, "sweep"), dilated by stage 0's 3x3 and pooled 3x3 / stride 2 per later stage"""
    from pillarnext_amd import ops, synth

    cfg = synth.CONFIGS["C2"]
    rng, vox = cfg["pc_range"], cfg["voxel_size"]
    pts = torch.from_numpy(synth.make_batch("C2", B, "sweep")).cuda()
    nx, ny = int(round((rng[3] - rng[0]) / vox[0])), int(round((rng[4] - rng[1]) / vox[1]))
    bi, xi, yi = pts[:, 0].long(), ((pts[:, 1] - rng[0]) / vox[0]).floor().long(), ((pts[:, 2] - rng[1]) / vox[1]).floor().long()
    ok = (xi >= 0) & (xi < nx) & (yi >= 0) & (yi < ny)
    occ = torch.zeros((B, ny, nx), dtype=torch.uint8, device="cuda")
    occ[bi[ok], yi[ok], xi[ok]] = 1
    stage = [ops.mask_pool3(occ, 1)]
    for _ in range(3):
        stage.append(ops.mask_pool3(stage[-1], 2))
    assert [m.shape[-1] for m in stage] == [nx, nx // 2, nx // 4, nx // 8]
    for s, m in enumerate(stage):      # every frame of every stage has active sites, and empty tiles
        assert int(m.flatten(1).any(dim=1).sum()) == B, ("a frame without an active site at stage", s)
        assert not bool(_tile_nonempty(m, 16).all()), ("no empty tile at stage", s)
    return stage


_MASKS = {}


def _masks(B):
    if B not in _MASKS:
        _MASKS.clear()      # one batch size alive at a time
        _MASKS[B] = _c2_masks(B)
    return _MASKS[B]


def _rand_map(B, C, H, W, gen, dtype, mask_u8=None):
    """randn (x mask) as a channels_last (B,C,H,W) map of dtype, generated in its memory order"""
    t = torch.randn((B, H, W, C), device="cuda", generator=gen)
    if mask_u8 is not None:
        t = t * mask_u8.unsqueeze(3)
    return t.to(dtype).permute(0, 3, 1, 2)


def _weights(cin, cout, gen, dtype):
    """He-scaled weights rounded to dtype (the values the kernel multiplies), their packed form, an fp32 bias"""
    from pillarnext_amd import ops

    w = (torch.randn((cout, cin, 3, 3), device="cuda", generator=gen) * (2.0 / (9 * cin)) ** 0.5).to(dtype)
    bias = torch.randn((cout,), device="cuda", generator=gen) * 0.5
    return w, ops.conv3x3_pack_weights(w, dtype=dtype), bias


# ---------------------------------------------------------------------------------------------------- gathered fp64 reference and the bars

def _gconv_half(xp, w9, sites, stride):
    """_gconv of the training module on a HALF-precision padded map xp (B,H+2,W+2,C): each gathered chunk is widened to fp64, the map never is.
    -> sum over the nine taps of xp[b, s oy + ky, s ox + kx] @ w9[tap] at the sites, and the same sum of |terms|"""
    b, oy, ox = sites
    out, outa = [], []
    wa = w9.abs()
    for i in range(0, b.numel(), CHUNK):
        bb, yy, xx = b[i:i + CHUNK], oy[i:i + CHUNK] * stride, ox[i:i + CHUNK] * stride
        acc = acca = None
        for t in range(9):
            v = xp[bb, yy + t // 3, xx + t % 3].double()
            a, aa = v @ w9[t], v.abs() @ wa[t]
            acc, acca = (a, aa) if acc is None else (acc + a, acca + aa)
        out.append(acc)
        outa.append(acca)
    return torch.cat(out), torch.cat(outa)


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1)


def _conv_ref(x, w, sites, stride):
    return _gconv_half(_pad1(_nhwc(x)), _taps(w), sites, stride)


def _finish_ref(conv, conva, bias, res, sites, relu):
    """bias, residual and ReLU in fp64 on the gathered convolution; -> (ref, sum|terms|)"""
    ref, refa = conv + bias.double(), conva + bias.double().abs()
    if res is not None:
        r = _nhwc(res)[sites].double()
        ref, refa = ref + r, refa + r.abs()
    return (ref.clamp(min=0) if relu else ref), refa


def _check(tag, got, ref, refa, dtype):
    """the three bars of the module docstring on (n, C) fp64 tensors; prints the figures, then asserts"""
    got = got.double()
    d = got - ref
    worst = float((d.abs() / (BF_REL * refa + OUT_ROUND[dtype] * ref.abs() + TINY)).max())
    once = ref.to(dtype).double() - ref                                  # the reference rounded once: no kernel involved
    nref = float(ref.norm())
    fro, fro1 = float(d.norm()) / nref, float(once.norm()) / nref
    mean, mean1, mabs, mterms = float(d.mean()), float(once.mean()), float(ref.abs().mean()), float(refa.mean())
    print(f"{tag}: worst |error| / bar {worst:.3f}; relative Frobenius {fro:.3e} (reference rounded once {fro1:.3e}, ratio {fro / fro1:.4f}); "
          f"signed mean error / mean|ref| {mean / mabs:+.2e} (rounded once {mean1 / mabs:+.2e}, bar {(BF_REL * mterms + abs(mean1)) / mabs:.2e})")
    assert worst <= 1.0, (tag, "per-element bar", worst)
    assert fro <= FRO_MARGIN * fro1, (tag, "relative Frobenius", fro, fro1)
    assert abs(mean) <= BF_REL * mterms + abs(mean1), (tag, "signed mean", mean, BF_REL * mterms, mean1)
    return worst


def _check_map(tag, y, mask_u8, sites, ref, refa, dtype):
    """the WHOLE output map: the active sites against fp64, every other element exactly zero (no non-zero bit pattern outside the active sites)"""
    got = _nhwc(y)[sites]
    n_all, n_act = int(torch.count_nonzero(y.view(torch.int16))), int(torch.count_nonzero(got.view(torch.int16)))
    assert n_all == n_act, (tag, "non-zero values at inactive sites", n_all - n_act)
    return _check(tag, got, ref, refa, dtype)


def _row_segments(mask_u8):
    """(B, H, ceil(W / 32)) uint8: row segments of 32 pixels that hold an active site = what row_dirty must be after a launch"""
    B, H, W = mask_u8.shape
    tx = -(-W // 32)
    m = torch.zeros((B, H, tx * 32), dtype=torch.uint8, device=mask_u8.device)
    m[:, :, :W] = mask_u8
    return (m.view(B, H, tx, 32) != 0).any(dim=3).to(torch.uint8)


# ---------------------------------------------------------------------------------------------------- a. backbone layers at the C2 geometry

# name, cin, cout, stride, stage of the OUTPUT map, residual taken, what walking all tiles at B = 4 must reach, what the tile list at B = 4 must reach.
# Tile counts of the sweep occupancy (non-empty 8 x 32 tiles at B = 4: 3175 / 961 / 289 at stages 1 / 2 / 3, 5629 of 16 x 32 at stage 0): at stage 3 a B = 4
# launch has 2 units per workgroup and a tile list 578 units for 512 workgroups, so those cases only claim what they reach; the B = 12 pass below
# brings stage 3 to the ticket range with a list and to >= 4 units per workgroup without.  256 -> 64 runs on the stage-2 map (on the 180^2 map it is one
# unit per workgroup at B = 4).
LAYERS = [
    ("stage0 64->64", 64, 64, 1, 0, True, "tickets+reuse", "tickets+reuse"),
    ("stage1 entry 64->128 s2", 64, 128, 2, 1, False, "tickets+reuse", None),
    ("stage1 128->128", 128, 128, 1, 1, True, "tickets+reuse", "tickets+reuse"),
    ("stage2 entry 128->256 s2", 128, 256, 2, 2, False, "tickets+reuse", None),
    ("stage2 256->256", 256, 256, 1, 2, True, "tickets+reuse", "tickets"),
    ("stage3 entry 256->256 s2", 256, 256, 2, 3, False, "tickets", None),
    ("stage3 256->256", 256, 256, 1, 3, True, "tickets", "iterate"),
    ("256->64 on the stage-2 map", 256, 64, 1, 2, True, "tickets+reuse", "iterate"),
]
LAYERS_B12 = {"stage0 64->64": ("tickets+reuse", "tickets+reuse"), "stage3 entry 256->256 s2": ("tickets+reuse", None),
              "stage3 256->256": ("tickets+reuse", "tickets")}


def _layer_case(layer, dtype, B, sel="default", want=None, ways=("stateless", "workspace", "tile list"), seed=0):
    """one layer, every way the backbone runs it, with and without residual, ReLU on: each output map against one gathered fp64 convolution"""
    from pillarnext_amd import ops

    name, cin, cout, stride, so, takes_res, want_all, want_list = layer
    if want is not None:
        want_all, want_list = want
    stage = _masks(B)
    mo = stage[so]
    mi = stage[so - 1] if stride == 2 else mo
    Ho, Wo = mo.shape[1:]
    H, W = mi.shape[1:]
    assert (Ho, Wo) == ((H - 1) // stride + 1, (W - 1) // stride + 1)
    tag = f"{name} {str(dtype)[6:]} B={B}" + ("" if sel == "default" else f" [{sel}]")
    sp = _split_of(cin, cout, stride, B, Ho, Wo, sel)
    nonempty = _tile_nonempty(mo, sp.th)
    assert nonempty.numel() * sp.nh == sp.units
    _reach(tag + " all tiles", sp, sp.units, want_all)
    if sp.static is not None:
        assert not bool(nonempty[sp.static // sp.nh:].all()), (tag, "no empty tile in the ticket range")
    listed = int(nonempty.sum()) * sp.nh
    if "tile list" in ways and want_list is not None:
        _reach(tag + " tile list", sp, listed, want_list)
    gen = torch.Generator(device="cuda").manual_seed(1000 * seed + 7 * cin + cout + stride + B)
    x = _rand_map(B, cin, H, W, gen, dtype, mi)
    w, wf, bias = _weights(cin, cout, gen, dtype)
    res = _rand_map(B, cout, Ho, Wo, gen, dtype) if takes_res else None     # NOT masked: the kernel must mask it
    sites = tuple(mo.nonzero(as_tuple=True))
    conv, conva = _conv_ref(x, w, sites, stride)
    segs = _row_segments(mo)
    worst = 0.0
    for r in ((None, res) if takes_res else (None,)):
        ref, refa = _finish_ref(conv, conva, bias, r, sites, True)
        for way in ways:
            if way == "tile list" and want_list is None:
                continue        # the stride-2 kernel walks all tiles (ops.conv_tile_rows == 0)
            t = f"{tag} res={r is not None} {way}"
            if way == "stateless":
                y = ops.conv3x3_masked(x, wf, bias, cout, stride, mo, r, True)
            else:
                ws = ops.conv3x3_workspace(B, cout, Ho, Wo, "cuda", dtype)
                tiles = None
                if way == "tile list":
                    rows = ops.conv_tile_rows(cin, cout, stride)
                    assert rows == sp.th, (rows, sp.th)
                    tiles = ops.conv_tile_list(mo, [ws[1]], rows)
                    assert int(tiles[1]) * sp.nh == listed, (t, int(tiles[1]), listed)
                y = ops.conv3x3_masked(x, wf, bias, cout, stride, mo, r, True, out=ws, tiles=tiles)
                assert y.data_ptr() == ws[0].data_ptr()
                assert torch.equal(ws[1], segs), (t, "row_dirty differs from the active row segments")
            worst = max(worst, _check_map(t, y, mo, sites, ref, refa, dtype))
            del y
    return worst


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("layer", LAYERS, ids=[la[0].replace(" ", "_") for la in LAYERS])
def test_backbone_layers_at_the_c2_geometry(layer, dtype):
    """Every backbone layer of SparseResNet at 4 frames of the C2 sweep occupancy, bf16 and f16 (the PNX_CONV_F16 object): stateless, through a fresh
    persistent workspace (row_dirty must come out as the active row segments) and with the tile list of ops.conv_tile_list, with and without residual."""
    _layer_case(layer, dtype, 4)


@pytest.mark.parametrize("name", list(LAYERS_B12), ids=[n.replace(" ", "_") for n in LAYERS_B12])
def test_backbone_layers_at_the_benchmark_batch(name):
    """bench.py's own batch of 12: stage 0 (a 3.19 GB map: active sites at byte offsets past 2^31, which no other test touches) and stage 3 (the only
    batch at which a stage-3 tile list reaches the ticket range, and a stage-3 launch 4 units per workgroup)."""
    layer = next(la for la in LAYERS if la[0] == name)
    B = 12
    if layer[4] == 0:
        mo = _masks(B)[0]
        H, W = mo.shape[1:]
        assert B * H * W * layer[2] * 2 > 2 ** 31
        b, y, x = (t[-1] for t in mo.nonzero(as_tuple=True))
        assert ((int(b) * H + int(y)) * W + int(x)) * layer[2] * 2 > 2 ** 31, "no active site past 2^31 bytes"
    _layer_case(layer, torch.bfloat16, B, want=LAYERS_B12[name])


# ---------------------------------------------------------------------------------------------------- b. two frames through one workspace

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("layer", [LAYERS[0], LAYERS[1], LAYERS[2], LAYERS[4], LAYERS[6]], ids=["stage0", "stage1_entry", "stage1", "stage2", "stage3"])
def test_two_frames_through_one_workspace_with_the_occupancy_flipped(layer, dtype):
    """Frame 0 on the sweep occupancy, frame 1 on its mirror image through the same (output, row_dirty) pair, tile list where the kernel takes one: the
    list of frame 1 names tiles that hold only stale rows (empty tiles, drawn by ticket at stages 0 - 2), those rows must be zeroed, and after each frame
    the whole buffer is the fp64 result at the active sites and exactly zero elsewhere, row_dirty the active row segments."""
    from pillarnext_amd import ops

    name, cin, cout, stride, so, takes_res, _, want_list = layer
    B = 4
    stage = _masks(B)
    Ho, Wo = stage[so].shape[1:]
    sp = _split_of(cin, cout, stride, B, Ho, Wo)
    gen = torch.Generator(device="cuda").manual_seed(3 * cin + cout + stride)
    w, wf, bias = _weights(cin, cout, gen, dtype)
    ws = ops.conv3x3_workspace(B, cout, Ho, Wo, "cuda", dtype)
    rows = ops.conv_tile_rows(cin, cout, stride)
    prev = None
    for frame in range(2):
        flip = (lambda m: m.flip(2).contiguous()) if frame else (lambda m: m)
        mo = flip(stage[so])
        mi = flip(stage[so - 1]) if stride == 2 else mo
        if stride == 2 and frame:        # the mirror image of the pooled set is the pooled mirror image only for odd widths: pool the mirrored input
            mo = ops.mask_pool3(mi, 2)
        tag = f"two frames {name} {str(dtype)[6:]} frame {frame}"
        nonempty = _tile_nonempty(mo, sp.th)
        tiles = None
        if rows:
            stale = _tile_nonempty(prev, sp.th) & ~nonempty if prev is not None else torch.zeros_like(nonempty)
            listed = int((nonempty | stale).sum()) * sp.nh
            _reach(tag + " tile list", sp, listed, want_list)
            if frame:
                assert int(stale.sum()) > 0, (tag, "no tile with stale rows only")
            tiles = ops.conv_tile_list(mo, [ws[1]], rows)
            assert int(tiles[1]) * sp.nh == listed, (tag, int(tiles[1]), listed)
        else:
            _reach(tag + " all tiles", sp, sp.units, "tickets+reuse")
        x = _rand_map(B, cin, mi.shape[1], mi.shape[2], gen, dtype, mi)
        res = _rand_map(B, cout, Ho, Wo, gen, dtype) if takes_res else None
        y = ops.conv3x3_masked(x, wf, bias, cout, stride, mo, res, True, out=ws, tiles=tiles)
        sites = tuple(mo.nonzero(as_tuple=True))
        ref, refa = _finish_ref(*_conv_ref(x, w, sites, stride), bias, res, sites, True)
        _check_map(tag, y, mo, sites, ref, refa, dtype)
        assert torch.equal(ws[1], _row_segments(mo)), (tag, "row_dirty differs from the active row segments")
        prev = mo


# ---------------------------------------------------------------------------------------------------- c. dense calls

def _detector_maps(config):
    """(neck map, head map) sides of the detector of BASELINE config `config`: the reader's grid (synth.CONFIGS) over the backbone's strides
    (configs/*.yaml: ds_layer_strides), the head's deblock upsampling by its `strides`"""
    from pillarnext_amd import config as C
    from pillarnext_amd import synth

    g = synth.CONFIGS[config]
    cfg = C.load(os.path.join(ROOT, "configs", "pillarnext_b_nusc.yaml" if config == "C2" else "pillarnext_b_waymo.yaml"))["model"]
    grid = int(round((g["pc_range"][3] - g["pc_range"][0]) / g["voxel_size"][0]))
    ds = 1
    for s in cfg["backbone"]["ds_layer_strides"]:
        ds *= int(s)
    up = int(cfg["head"]["strides"][0])
    assert grid % ds == 0
    return grid // ds, grid // ds * up


def _all_sites(B, H, W):
    b, y, x = torch.meshgrid(torch.arange(B, device="cuda"), torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    return b.reshape(-1), y.reshape(-1), x.reshape(-1)


DENSE = [("neck 256->256", "C2", 256, 256, 8), ("neck 256->256", "C4", 256, 256, 8), ("head 64->64", "C2", 64, 64, 4), ("head 64->64", "C4", 64, 64, 4),
         ("head 64->320", "C2", 64, 320, 8), ("head 64->384", "C2", 64, 384, 8), ("head 64->448", "C4", 64, 448, 8)]


@pytest.mark.parametrize("name,config,cin,cout,B", DENSE, ids=[f"{d[0].replace(' ', '_')}_{d[1]}" for d in DENSE])
def test_dense_convolutions_on_the_detector_maps(name, config, cin, cout, B):
    """mask = None (static round-robin, slot < 0) with at least 4 units per workgroup on the neck / head maps of the C2 and C4 detectors: the neck's
    256 -> 256 (launch_ldsx), the head's shared 64 -> 64 (launch_pc) and the merged first SepHead convolutions 64 -> 320 / 384 / 448 (launch_lds)."""
    from pillarnext_amd import ops

    neck, head = _detector_maps(config)
    H = W = neck if cin == 256 else head
    sp = _split_of(cin, cout, 1, B, H, W)
    tag = f"dense {name} {config} {B}x{H}x{W}"
    _reach(tag, sp, sp.units, "reuse")
    gen = torch.Generator(device="cuda").manual_seed(cin + cout + H)
    x = _rand_map(B, cin, H, W, gen, torch.bfloat16)
    w, wf, bias = _weights(cin, cout, gen, torch.bfloat16)
    sites = _all_sites(B, H, W)
    y = ops.conv3x3_masked(x, wf, bias, cout, 1, None, None, True)
    ref, refa = _finish_ref(*_conv_ref(x, w, sites, 1), bias, None, sites, True)
    _check(tag, _nhwc(y)[sites], ref, refa, torch.bfloat16)


@pytest.mark.parametrize("config", ["C2", "C4"])
def test_deconv2x2_on_the_detector_maps(config):
    """k_deconv2x2_64 (the SepHead deblock, neck map -> head map) with at least 4 row segments per wave"""
    from pillarnext_amd import ops

    H = W = _detector_maps(config)[0]
    B = 8
    sp = launch_deconv(B, H, W)
    tag = f"deconv2x2 64->64 {config} {B}x{H}x{W}"
    _reach(tag, sp, sp.units, "reuse")
    gen = torch.Generator(device="cuda").manual_seed(H)
    x = _rand_map(B, 64, H, W, gen, torch.bfloat16)
    w = (torch.randn((64, 64, 2, 2), device="cuda", generator=gen) / 8).to(torch.bfloat16)
    bias = torch.randn((64,), device="cuda", generator=gen) * 0.5
    y = ops.deconv2x2(x, ops.deconv2x2_pack_weights(w), bias, 64, True)
    assert tuple(y.shape) == (B, 64, 2 * H, 2 * W)
    x64, w64 = _nhwc(x).double(), w.double()
    ref = torch.empty((B, 2 * H, 2 * W, 64), dtype=torch.float64, device="cuda")
    refa = torch.empty_like(ref)
    for ky in range(2):
        for kx in range(2):
            ref[:, ky::2, kx::2] = x64 @ w64[:, :, ky, kx] + bias.double()
            refa[:, ky::2, kx::2] = x64.abs() @ w64[:, :, ky, kx].abs() + bias.double().abs()
    _check(tag, _nhwc(y).reshape(-1, 64), ref.clamp(min=0).reshape(-1, 64), refa.reshape(-1, 64), torch.bfloat16)


@pytest.mark.parametrize("nb,config", [(5, "C2"), (6, "C2"), (7, "C4"), (1, "C2"), (2, "C4")])
def test_sephead_output_convolution_on_the_detector_maps(nb, config):
    """k_sephead_out<NBR> (block-diagonal nb x 64 -> 16; 5 / 6 / 7 branches, and the lazy head's 1 and 2) on the head map with at least 4 tiles per workgroup"""
    from pillarnext_amd import ops

    H = W = _detector_maps(config)[1]
    B = 12
    sp = launch_sephead(B, H, W)
    tag = f"sephead_out {nb} branches {config} {B}x{H}x{W}"
    _reach(tag, sp, sp.units, "reuse")
    gen = torch.Generator(device="cuda").manual_seed(10 * nb + H)
    outs = [2, 1, 3, 2, 2, 1, 2][:nb]
    x = torch.relu(_rand_map(B, nb * 64, H, W, gen, torch.bfloat16))
    w2 = torch.zeros((16, nb * 64, 3, 3), device="cuda")
    o = 0
    for j, k in enumerate(outs):
        w2[o:o + k, 64 * j:64 * (j + 1)] = torch.randn((k, 64, 3, 3), device="cuda", generator=gen) / 24
        o += k
    w2 = w2.to(torch.bfloat16)
    bias = torch.randn((16,), device="cuda", generator=gen) * 0.5
    bias[o:] = 0.0
    y = ops.sephead_out(x, ops.sephead_pack_weights(w2), bias)
    sites = _all_sites(B, H, W)
    ref, refa = _finish_ref(*_conv_ref(x, w2, sites, 1), bias, None, sites, False)
    got = _nhwc(y)[sites]
    assert int(torch.count_nonzero(got[:, o:])) == 0, (tag, "outputs past the last branch")
    _check(tag, got[:, :o], ref[:, :o], refa[:, :o], torch.bfloat16)


# ---------------------------------------------------------------------------------------------------- d. non-default kernel selections

@pytest.mark.parametrize("layer", [LAYERS[0], LAYERS[2]], ids=["stage0", "stage1"])
def test_direct_kernel_at_the_c2_geometry(layer, monkeypatch):
    """PNX_CONV_DIRECT (read per call): k_conv3x3, one tile per wave, at least 4 tiles per wave, stateless and through a workspace"""
    monkeypatch.setenv("PNX_CONV_DIRECT", "1")
    _layer_case(layer, torch.bfloat16, 4, sel="direct", want=("reuse", None), ways=("stateless", "workspace"))


CHILD_CASES = {
    # PNX_CONV_PC=0: 64 -> 64 on launch_lds<64> (k_conv3x3_lds, sched_next2) instead of the producer / consumer kernel
    "pc0": dict(env={"PNX_CONV_PC": "0"}, layers=[0], sel="pc0"),
    # PNX_CONV_PACK=0: the row form of k_conv3x3_ldsx at stages 1 - 3 (same launch, same work split)
    "pack0": dict(env={"PNX_CONV_PACK": "0"}, layers=[2, 4, 6], sel="default"),
}


def _child(which):
    case = CHILD_CASES[which]
    for k, v in case["env"].items():
        assert os.environ.get(k) == v, (k, os.environ.get(k))
    for i in case["layers"]:
        for dtype in (torch.bfloat16, torch.float16):
            _layer_case(LAYERS[i], dtype, 4, sel=case["sel"])
    torch.cuda.synchronize()
    print(f"child {which}: ok")


@pytest.mark.parametrize("which", list(CHILD_CASES))
def test_non_default_kernel_selections_in_a_child_process(which):
    """The library reads PNX_CONV_PC / PNX_CONV_PACK once per process: the same layer cases, reference and bars in a child (this file as a script).  One
    child per test, with a timeout; nothing runs after it."""
    env = dict(os.environ, **CHILD_CASES[which]["env"])
    p = subprocess.run([sys.executable, os.path.abspath(__file__), which], env=env, capture_output=True, text=True, timeout=600)
    print(p.stdout[-20000:])
    assert p.returncode == 0, (which, p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    assert p.stdout.strip().endswith(f"child {which}: ok")


# ---------------------------------------------------------------------------------------------------- e. ticket ring wrap

def test_inference_launches_wrap_the_ticket_ring():
    """132 masked launches back to back on one stream -- the producer / consumer 64 -> 64, the stride-2 256 -> 256 entry and the packed 256 -> 256, in turn,
    each drawing tickets -- take every g_tile_ctr slot at least twice: the first launch of each kernel is held to the fp64 bars, every later one must be
    bit-equal to it, so sched_done re-armed every slot."""
    from pillarnext_amd import ops

    B = 4
    stage = _masks(B)
    gen = torch.Generator(device="cuda").manual_seed(64)
    runs = []
    for cin, cout, stride, so in ((64, 64, 1, 1), (256, 256, 2, 3), (256, 256, 1, 3)):
        mo = stage[so]
        mi = stage[so - 1] if stride == 2 else mo
        sp = _split_of(cin, cout, stride, B, mo.shape[1], mo.shape[2])
        _reach(f"ring wrap {cin}->{cout} s{stride}", sp, sp.units, "tickets")
        x = _rand_map(B, cin, mi.shape[1], mi.shape[2], gen, torch.bfloat16, mi)
        w, wf, bias = _weights(cin, cout, gen, torch.bfloat16)
        runs.append((cin, cout, stride, mo, x, w, wf, bias))
    first = [None] * len(runs)
    n = 0
    for i in range(44):
        for k, (cin, cout, stride, mo, x, w, wf, bias) in enumerate(runs):
            y = ops.conv3x3_masked(x, wf, bias, cout, stride, mo, None, True)
            n += 1
            if first[k] is None:
                first[k] = y
                sites = tuple(mo.nonzero(as_tuple=True))
                ref, refa = _finish_ref(*_conv_ref(x, w, sites, stride), bias, None, sites, True)
                _check_map(f"ring wrap {cin}->{cout} s{stride}", y, mo, sites, ref, refa, torch.bfloat16)
            else:
                assert torch.equal(y, first[k]), (f"{cin}->{cout} s{stride} differs at launch", n)
    assert n > 2 * 64


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    _child(sys.argv[1])
