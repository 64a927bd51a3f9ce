"""GPU: the training kernels at shapes where their tile / site loops run many times per workgroup or wave, against fp64 on the SAME operands the kernels saw.

The other training tests use shapes at which every workgroup of csrc/conv_wgrad.hip, csrc/conv_pc.h, csrc/conv_dgrad_s2.h, csrc/masked_bn.hip and
csrc/head_train.hip handles one tile or one site and exits: the software-pipelined prefetch of tile k + 1, the row-mask sets indexed by tile parity, the
tile tickets of the 64-slot g_tile_ctr ring and the 2-4 sites / vectors in flight never run there.  Every case below first restates the launch's work split
in Python (_wgrad_split, _pc_grid, _dgrad_s2_grid, _mbn_strides, _smallk_units: each names the constants of the .hip source it mirrors) and asserts that
its shape reaches the path it is there for.

References: fp64 on the GPU, gathered at the active sites and chunked (_gconv, _gwgrad), on the bf16 maps themselves for the bf16 node and on the fp32
operand (x6: = the exact sum of its pieces; x3: the halves' sum) for the fp32 nodes.  Bars per element against the sum of |terms| (as
tests/test_gpu_fp32_six_products.py) plus relative Frobenius; bf16 outputs get one output rounding on top.  -rP prints the measured numbers."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

X6_REL, X6_FRO = 2.0 ** -19, 1e-6       # tests/test_gpu_fp32_six_products.py
X3_REL, X3_FRO = 2.0 ** -14, 3e-5       # tests/test_gpu_masked_conv_train.py::test_fp32_node_on_three_bf16_products_against_fp64
BF_REL, BF_OUT = 1e-5, 2.0 ** -8        # bf16 operands, fp32 accumulation (test_sephead_output_convolution_kernels); one bf16 output rounding
TINY = 2.0 ** -126
CHUNK = 1 << 18                         # gathered sites per reference step: 2^18 x 256 channels x 8 bytes = 512 MiB per operand


# ---------------------------------------------------------------------------------------------------- work splits of the launches

def _wgrad_split(mask_u8, cin, cout, stride):
    """conv_wgrad.hip launch_wgrad / k_wgrad64: G = max(1, WG_GROUPS (512) / n_pairs) workgroups per 64x64 channel pair; output tiles of WgGeo<S>::TH rows
    (4 at S=1, 2 at S=2) x 32 pixels in (b, ty, tx) order; workgroup g lists tiles g, g + G, ... that hold an active output (empty ones are compacted away).
    -> (G, non-empty tiles per workgroup, all tiles per workgroup)"""
    TH = 4 if stride == 1 else 2
    G = max(1, 512 // ((cin // 64) * (cout // 64)))
    B, Ho, Wo = mask_u8.shape
    ty, tx = -(-Ho // TH), -(-Wo // 32)
    m = torch.zeros((B, ty * TH, tx * 32), dtype=torch.uint8, device=mask_u8.device)
    m[:, :Ho, :Wo] = mask_u8
    nonempty = (m.view(B, ty, TH, tx, 32) != 0).any(dim=4).any(dim=2).reshape(-1)
    idx = torch.arange(nonempty.numel(), device=m.device) % G
    return G, torch.bincount(idx[nonempty], minlength=G), torch.bincount(idx, minlength=G)


def _pc_grid(B, H, W, cin):
    """conv_pc.h launch_pc*: tiles of TH = 16 (64 channels) / 8 rows x 32 pixels, grid = min(tiles, 256); with a mask, indices >= 3 x grid are tickets"""
    TH = 16 if cin == 64 else 8
    n = B * -(-H // TH) * -(-W // 32)
    return n, min(n, 256)


def _dgrad_s2_grid(B, H, W, cin, cout):
    """conv_dgrad_s2.h Dg2Geo<CO, CI> / launch_dgrad_s2: TG = 2 * (8 / (CI / 32)) g rows x 32 g columns per tile, LDS = CO/64 slabs x (TG + 1) rows x LDS_HW (34)
    x 8 x 16 bytes, per_cu = 2 if LDS <= 75 KiB else 1, grid = min(tiles, 256 * per_cu); tiles past the first grid come from tickets"""
    TG = 2 * (8 // (cin // 32))
    lds = (cout // 64) * (TG + 1) * 34 * 8 * 16
    per_cu = 2 if lds <= 75 * 1024 else 1
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    n = B * -(-Ho // TG) * -(-Wo // 32)
    return n, min(n, 256 * per_cu)


def _mbn_strides(n, C):
    """masked_bn.hip: the statistics passes (kMbnBlocks = 1024 blocks of 256 threads, 256 * 8 / C sites per block and step) walk sites with stride
    1024 * rows, four (k_mbn_stats) / two (k_mbn_bwd_stats) per iteration; the apply passes (min(8192, ceil(n * C/8 / 256)) blocks) walk 8-channel vectors
    with stride blocks * 256, two per iteration"""
    cvec = C // 8
    s_sites = 1024 * (256 // cvec)
    nvec = n * cvec
    s_vec = min(8192, -(-nvec // 256)) * 256
    return s_sites, nvec, s_vec


def _smallk_units(B, H, W):
    """head_train.hip ht_blocks: units of 4 rows x HT_STRIP (16) sites, min(ceil(units / 4), HT_WAVES (2048) / 4) blocks of 4 waves"""
    units = B * -(-H // 4) * -(-W // 16)
    return units, 4 * min(-(-units // 4), 2048 // 4)


# ---------------------------------------------------------------------------------------------------- operands

def _lidar_mask(B, H, W, gen, p=0.12):
    """clustered occupancy: a few dense blobs + scattered cells, ~p of the cells (as tests/test_gpu_masked_conv_train.py)"""
    m = torch.rand((B, 1, H, W), device="cuda", generator=gen) < p * 0.3
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    for b in range(B):
        for _ in range(6):
            cy, cx = (torch.rand(2, device="cuda", generator=gen) * torch.tensor([H, W], device="cuda")).tolist()
            r = 3 + 0.12 * min(H, W) * float(torch.rand(1, device="cuda", generator=gen))
            m[b, 0] |= ((yy - cy) ** 2 + (xx - cx) ** 2 < r * r) & (torch.rand((H, W), device="cuda", generator=gen) < 0.6)
    return m.float()


def _dense_mask(B, H, W, gen):
    """every cell active with p = 0.5, except rows [H/3, H/2) x columns [W/3, W) of each frame (so that some workgroups list empty tiles too)"""
    m = torch.rand((B, 1, H, W), device="cuda", generator=gen) < 0.5
    m[:, :, H // 3:H // 2, W // 3:] = False
    return m.float()


def _mask(kind, B, H, W, gen):
    """lidar: _lidar_mask with the empty sector of _dense_mask (an occluded region: the pooled stride-2 output sets have no empty tile without it)"""
    if kind == "dense":
        return _dense_mask(B, H, W, gen)
    m = _lidar_mask(B, H, W, gen)
    m[:, :, H // 3:H // 2, W // 3:] = 0.0
    return m


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _u8(mask):
    return (mask[:, 0] != 0).to(torch.uint8).contiguous()


def _fro(a, r):
    return float((a.double() - r).norm() / r.norm())


# ---------------------------------------------------------------------------------------------------- gathered fp64 references

def _nhwc64(t):
    return t.detach().permute(0, 2, 3, 1).double()


def _pad1(x):
    """(B,H,W,C) -> (B,H+2,W+2,C), zeros around: index i + 1 is site i"""
    return torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))


def _taps(w):
    """forward taps: (Cout,Cin,3,3) -> (9, Cin, Cout) fp64, tap = 3 ky + kx"""
    return w.detach().double().permute(2, 3, 1, 0).reshape(9, w.shape[1], w.shape[0]).contiguous()


def _taps_t(w):
    """data-gradient taps: tap (ky, kx) of the flipped, transposed weights, (9, Cout, Cin)"""
    return w.detach().double().flip(2, 3).permute(2, 3, 0, 1).reshape(9, w.shape[0], w.shape[1]).contiguous()


def _gconv(xp, w9, sites, stride):
    """sum over the nine taps of xp[b, s oy + ky, s ox + kx] @ w9[tap] at the sites (b, oy, ox), xp padded by one (_pad1); and the same sum of |terms|"""
    b, oy, ox = sites
    out, outa = [], []
    wa = w9.abs()
    for i in range(0, b.numel(), CHUNK):
        bb, yy, xx = b[i:i + CHUNK], oy[i:i + CHUNK] * stride, ox[i:i + CHUNK] * stride
        acc = acca = None
        for t in range(9):
            v = xp[bb, yy + t // 3, xx + t % 3]
            a, aa = v @ w9[t], v.abs() @ wa[t]
            acc, acca = (a, aa) if acc is None else (acc + a, acca + aa)
        out.append(acc)
        outa.append(acca)
    return torch.cat(out), torch.cat(outa)


def _gwgrad(xp, g, sites, stride):
    """dW[co, ci, ky, kx] = sum over the output sites p of g[p, co] x[s p + tap - 1, ci] (xp padded, g (B,Ho,Wo,Cout)); and the sum of |terms|"""
    b, oy, ox = sites
    co, ci = g.shape[-1], xp.shape[-1]
    dw = torch.zeros((9, co, ci), dtype=torch.float64, device=xp.device)
    dwa = torch.zeros_like(dw)
    for i in range(0, b.numel(), CHUNK):
        bb, yy, xx = b[i:i + CHUNK], oy[i:i + CHUNK], ox[i:i + CHUNK]
        gv = g[bb, yy, xx]
        gt, gta = gv.t(), gv.abs().t()
        for t in range(9):
            v = xp[bb, stride * yy + t // 3, stride * xx + t % 3]
            dw[t] += gt @ v
            dwa[t] += gta @ v.abs()
    return dw.view(3, 3, co, ci).permute(2, 3, 0, 1), dwa.view(3, 3, co, ci).permute(2, 3, 0, 1)


def _dilate(g, H, W):
    """stride-2 data gradient as a stride-1 one: g (B,Ho,Wo,C) at the even sites of an (B,H,W,C) map of zeros"""
    gd = torch.zeros((g.shape[0], H, W, g.shape[3]), dtype=g.dtype, device=g.device)
    gd[:, 0::2, 0::2] = g
    return gd


def _sites(mask):
    return tuple(mask[:, 0].nonzero(as_tuple=True))


def _gather(t, sites):
    """kernel output (B,C,H,W) at the sites -> (n, C) fp64"""
    b, y, x = sites
    return t.detach().permute(0, 2, 3, 1)[b, y, x].double()


def _conv_refs(x, w, g, mask_in, mask_out, stride, want_w=True):
    """fp64 y (at mask_out), dx (at mask_in), dW of mask_out * conv3x3(x, w) with upstream gradient g, each with its sum of |terms|"""
    so, si = _sites(mask_out), _sites(mask_in)
    xp = _pad1(_nhwc64(x))
    y = _gconv(xp, _taps(w), so, stride)
    g64 = _nhwc64(g) * _nhwc64(mask_out)
    gsrc = g64 if stride == 1 else _dilate(g64, x.shape[2], x.shape[3])
    dx = _gconv(_pad1(gsrc), _taps_t(w), si, 1)
    del gsrc
    dw = _gwgrad(xp, g64, so, stride) if want_w else None
    return dict(y=y, dx=dx, dw=dw, so=so, si=si)


def _check(tag, name, got, ref, refa, rel, fro=None, out_ulp=0.0):
    """|got - ref| <= rel * (sum of |terms|) [+ out_ulp * |ref|: one output rounding] per element; relative Frobenius <= fro; both printed"""
    got = got.double()
    err = (got - ref).abs()
    ok = bool((err <= rel * refa + out_ulp * ref.abs() + TINY).all())
    worst = float(((err - out_ulp * ref.abs()).clamp(min=0) / (refa + TINY)).max())
    e = _fro(got, ref)
    print(f"{tag} {name}: relative Frobenius {e:.2e}, worst |error| / sum|terms| {worst:.2e} (bar {rel:.1e})")
    assert ok, (tag, name, worst, rel)
    if fro is not None:
        assert e <= fro, (tag, name, e, fro)
    return e


def _bars(prec):
    return {"bf16": (BF_REL, None, BF_OUT), "x3": (X3_REL, X3_FRO, 0.0), "x6": (X6_REL, X6_FRO, 0.0)}[prec]


# ---------------------------------------------------------------------------------------------------- a. weight gradient

WGRAD = [(64, 64, 1, (2, 801, 417)), (128, 128, 1, (2, 230, 190)), (256, 256, 1, (2, 202, 200)),
         (64, 128, 2, (2, 342, 420)), (128, 256, 2, (2, 190, 190)), (256, 256, 2, (2, 202, 260))]


@pytest.mark.parametrize("kind", ["lidar", "dense"])
@pytest.mark.parametrize("cin,cout,stride,shape", WGRAD)
def test_wgrad_kernels_over_many_tiles_per_workgroup(cin, cout, stride, shape, kind):
    """ops.conv3x3_wgrad on 1, 2 and 3 pieces (csrc/conv_wgrad.hip) with >= 3 non-empty tiles in every workgroup's list (the k + 1 prefetch and the s_rm[k & 1] row
    masks run), partial bottom and right tiles, an upstream gradient that is NOT zero outside the mask: against fp64, bit-identical on a second call,
    exactly zero on an empty mask."""
    import torch.nn.functional as F

    from pillarnext_amd import ops

    B, H, W = shape
    gen = torch.Generator(device="cuda").manual_seed(7 * cin + cout + H + (kind == "dense"))
    m_in = _mask(kind, B, H, W, gen)
    m = m_in if stride == 1 else F.max_pool2d(m_in, 3, stride, 1)
    mu8 = _u8(m)
    Ho, Wo = mu8.shape[1:]
    TH = 4 if stride == 1 else 2
    assert Ho % TH and Wo % 32, "partial bottom and right tiles"
    G, mine, tiles = _wgrad_split(mu8, cin, cout, stride)
    assert int(mine.min()) >= 3, (G, int(mine.min()))
    assert bool(((mine > 0) & (mine < tiles)).any()), "no workgroup lists a subset of its tiles"
    assert int(tiles.max()) <= 2040                                             # WG_LIST_MAX
    x0 = _cl(torch.randn((B, cin, H, W), device="cuda", generator=gen) * m_in)
    g_all = _cl(torch.randn((B, cout, Ho, Wo), device="cuda", generator=gen))
    so = _sites(m)
    empty = torch.zeros_like(mu8)
    tag = f"wgrad {cin}->{cout} s{stride} {kind} (min {int(mine.min())} tiles / workgroup)"
    for prec in ("bf16", "x3", "x6"):
        if prec == "bf16":
            xs, gs = (x0.to(torch.bfloat16),), (g_all.to(torch.bfloat16),)
            run = lambda mk: ops.conv3x3_wgrad(xs[0], gs[0], mk, stride=stride)  # noqa: E731
        elif prec == "x3":
            xs, gs = ops.split_f32(x0), ops.split_f32(g_all)
            run = lambda mk: ops.conv3x3_wgrad(xs, gs, mk, stride=stride)  # noqa: E731
        else:
            xs, gs = ops.split_f32(x0, pieces=3), ops.split_f32(g_all, pieces=3)
            run = lambda mk: ops.conv3x3_wgrad(xs, gs, mk, stride=stride)  # noqa: E731
        dw = run(mu8)
        assert torch.equal(dw, run(mu8)), (tag, prec, "not bit-identical on a second call")
        assert float(run(empty).abs().max()) == 0.0, (tag, prec, "an empty mask")
        xr = sum(p.double() for p in xs)          # the operands the kernel saw: the bf16 map / the exact sum of the pieces
        gr = sum(p.double() for p in gs)
        ref, refa = _gwgrad(_pad1(_nhwc64(xr)), _nhwc64(gr), so, stride)
        rel, fro, _ = _bars(prec)
        _check(f"{tag} {prec}", "dw", dw, ref, refa, rel, fro)


def test_fp32_wgrad_forms_have_no_systematic_offset():
    """pnx_conv3x3_wgrad_x3 / _x6 at 32 tiles per workgroup (every site active): an MFMA rounds a much smaller addend to its accumulator toward -inf,
    and the low-order visits add products 2^-8 .. 2^-16 of the running sum -- before conv_wgrad.hip alternated the sign of the sum per tile, every
    element of dW came out low by about the same amount (x6: mean error -0.98 x its rms, 4.7e-6 relative Frobenius).  The mean error must be small
    against its rms, and the six-product form within its 1e-6 bar."""
    from pillarnext_amd import ops

    B, C, H, W = 2, 64, 1024, 1024
    G, mine, _ = _wgrad_split(torch.ones((B, H, W), dtype=torch.uint8, device="cuda"), C, C, 1)
    assert int(mine.min()) == 32
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = _cl(torch.randn((B, C, H, W), device="cuda", generator=gen))
    g = _cl(torch.randn((B, C, H, W), device="cuda", generator=gen))
    ones = torch.ones((B, H, W), dtype=torch.uint8, device="cuda")
    xp = _pad1(_nhwc64(x))
    g2 = _nhwc64(g).reshape(-1, C)
    ref = torch.empty((C, C, 3, 3), dtype=torch.float64, device="cuda")
    for t in range(9):
        ref[:, :, t // 3, t % 3] = g2.t() @ xp[:, t // 3:t // 3 + H, t % 3:t % 3 + W].reshape(-1, C)
    for prec, dw in (("x3", ops.conv3x3_wgrad(ops.split_f32(x), ops.split_f32(g), ones)),
                     ("x6", ops.conv3x3_wgrad(ops.split_f32(x, pieces=3), ops.split_f32(g, pieces=3), ones))):
        e = dw.double() - ref
        mean, rms, fro = float(e.mean()), float(e.pow(2).mean().sqrt()), _fro(dw, ref)
        print(f"wgrad {prec} 64->64 {B}x{H}x{W} (32 tiles / workgroup): mean error {mean:.2e}, rms {rms:.2e}, relative Frobenius {fro:.2e}")
        assert abs(mean) <= 0.1 * rms, (prec, mean, rms)
        assert fro <= (X6_FRO if prec == "x6" else X3_FRO), (prec, fro)


# ---------------------------------------------------------------------------------------------------- b. forward and data gradient

def _run_node(prec, conv, x0, g0, mask_out, mask_in, monkeypatch, dense=False):
    """the training node of `prec` (bf16: _MaskedConv3x3Fn under autocast; x3 / x6: _MaskedConv3x3F32Fn, PNX_TRAIN_F32_PIECES = 2 / 3): y, dx, dW"""
    from pillarnext_amd.models import masked_conv, x3_conv

    conv.weight.grad = None
    if conv.bias is not None:
        conv.bias.grad = None
    x = x0.clone().requires_grad_(True)
    if prec != "bf16":
        monkeypatch.setenv("PNX_TRAIN_F32_PIECES", "2" if prec == "x3" else "3")
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec == "bf16"):
        y = x3_conv(conv, x) if dense else masked_conv(conv, x, mask_out, mask_in)
    want = "_MaskedConv3x3Fn" if prec == "bf16" else "_MaskedConv3x3F32Fn"
    assert type(y.grad_fn).__name__ == want + "Backward", type(y.grad_fn).__name__
    y.backward(g0.to(y.dtype))
    return y.detach(), x.grad, conv.weight.grad.clone()


def _operands(prec, x0, w, g0):
    """what the node's kernels multiply: bf16-rounded maps and weights for the bf16 node, the fp32 operands for the fp32 node"""
    if prec == "bf16":
        return x0.to(torch.bfloat16), w.detach().to(torch.bfloat16), g0.to(torch.bfloat16)
    return x0, w.detach(), g0


FWD = [(64, 64, 1, (2, 512, 512)), (128, 128, 1, (2, 400, 400)), (256, 256, 1, (2, 400, 400)),
       (64, 128, 2, (2, 600, 800)), (128, 256, 2, (2, 480, 480)), (256, 256, 2, (2, 480, 480))]


@pytest.mark.parametrize("cin,cout,stride,shape", FWD)
def test_conv_nodes_forward_and_data_gradient_on_tickets(cin, cout, stride, shape, monkeypatch):
    """train_nodes._MaskedConv3x3Fn (bf16) and _MaskedConv3x3F32Fn (x3, x6) with more than 3 x grid tiles: the stride-1 producer / consumer kernel (forward and
    data gradient, csrc/conv_pc.h) and the stride-2 data gradient (csrc/conv_dgrad_s2.h) take most of their tiles from tickets.  y and dx against fp64,
    bit-identical on repeat, exact zeros at inactive sites."""
    import torch.nn.functional as F

    from pillarnext_amd.models import _SpConv2d

    B, H, W = shape
    if stride == 1:
        n, grid = _pc_grid(B, H, W, cin)
    else:
        n, grid = _dgrad_s2_grid(B, H, W, cin, cout)
    assert n > 3 * grid, (n, grid)
    gen = torch.Generator(device="cuda").manual_seed(5 * cin + cout + H)
    mask_in = _lidar_mask(B, H, W, gen)
    mask_out = mask_in if stride == 1 else F.max_pool2d(mask_in, 3, stride, 1)
    conv = _SpConv2d(cin, cout, 3, stride=stride, padding=1, bias=False).cuda().train()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, device="cuda", generator=gen) * (2.0 / (9 * cin)) ** 0.5)
    x0 = _cl(torch.randn((B, cin, H, W), device="cuda", generator=gen) * mask_in)
    Ho, Wo = mask_out.shape[2:]
    g0 = _cl(torch.randn((B, cout, Ho, Wo), device="cuda", generator=gen) * mask_out)
    tag = f"node {cin}->{cout} s{stride} ({n} tiles, grid {grid})"
    refs = {}
    for prec in ("bf16", "x3", "x6"):
        y, dx, dw = _run_node(prec, conv, x0, g0, mask_out, mask_in, monkeypatch)
        y2, dx2, dw2 = _run_node(prec, conv, x0, g0, mask_out, mask_in, monkeypatch)
        assert torch.equal(y, y2) and torch.equal(dx, dx2) and torch.equal(dw, dw2), (tag, prec, "not bit-identical on repeat")
        assert bool((y[(mask_out == 0).expand_as(y)] == 0).all()), (tag, prec, "y at inactive outputs")
        assert bool((dx[(mask_in == 0).expand_as(dx)] == 0).all()), (tag, prec, "dx at inactive inputs")
        key = "bf16" if prec == "bf16" else "f32"
        if key not in refs:
            refs[key] = _conv_refs(*_operands(prec, x0, conv.weight, g0), mask_in, mask_out, stride, want_w=False)
        r = refs[key]
        rel, fro, ulp = _bars(prec)
        _check(f"{tag} {prec}", "y", _gather(y, r["so"]), *r["y"], rel, fro, ulp)
        _check(f"{tag} {prec}", "dx", _gather(dx, r["si"]), *r["dx"], rel, fro, ulp)


@pytest.mark.parametrize("c", [64, 256])
def test_dense_conv_nodes_over_many_tiles(c, monkeypatch):
    """models.x3_conv (the neck's / head's dense 3x3 layers, bias; mask = None: the static round-robin deal of conv_pc.h) at more than 2 x grid tiles:
    y, dx, dW, db against fp64 for bf16 / x3 / x6, bit-identical on repeat."""
    B, H, W = (2, 288, 512) if c == 64 else (1, 288, 512)
    n, grid = _pc_grid(B, H, W, c)
    assert n > 2 * grid, (n, grid)
    gen = torch.Generator(device="cuda").manual_seed(c + 1)
    conv = torch.nn.Conv2d(c, c, 3, padding=1, bias=True).cuda().train()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, device="cuda", generator=gen) * (2.0 / (9 * c)) ** 0.5)
        conv.bias.copy_(torch.randn(c, device="cuda", generator=gen))
    x0 = _cl(torch.randn((B, c, H, W), device="cuda", generator=gen))
    g0 = _cl(torch.randn((B, c, H, W), device="cuda", generator=gen))
    ones = torch.ones((B, 1, H, W), device="cuda")
    tag = f"dense {c} ({n} tiles, grid {grid})"
    refs = {}
    for prec in ("bf16", "x3", "x6"):
        y, dx, dw = _run_node(prec, conv, x0, g0, None, None, monkeypatch, dense=True)
        db = conv.bias.grad.clone()
        y2, dx2, dw2 = _run_node(prec, conv, x0, g0, None, None, monkeypatch, dense=True)
        assert torch.equal(y, y2) and torch.equal(dx, dx2) and torch.equal(dw, dw2), (tag, prec, "not bit-identical on repeat")
        key = "bf16" if prec == "bf16" else "f32"
        if key not in refs:
            xr, wr, gr = _operands(prec, x0, conv.weight, g0)
            refs[key] = _conv_refs(xr, wr, gr, ones, ones, 1)
            refs[key]["g"] = gr
        r = refs[key]
        rel, fro, ulp = _bars(prec)
        yr, ya = r["y"]
        bias = conv.bias.detach().double()
        _check(f"{tag} {prec}", "y", _gather(y, r["so"]), yr + bias, ya + bias.abs(), rel, fro, ulp)
        _check(f"{tag} {prec}", "dx", _gather(dx, r["si"]), *r["dx"], rel, fro, ulp)
        if prec == "bf16":
            fro_bf16_dw = _check(f"{tag} {prec}", "dw", dw, *r["dw"], rel, fro)
        elif prec == "x6":
            # The dense 256 -> 256 layer: every site active, 18 tiles per workgroup; its weight gradient's Frobenius error is the fp32 rounding of the
            # running sums, and the six-product form rounds six times per tile where the bf16 kernel rounds once (the visits' products are otherwise
            # exact): sqrt(6) x the bf16 kernel's figure on the same tiles (measured 1.02e-6 = 2.4 x 4.26e-7), 1.25 x that as the bar, never looser
            # than 1e-6 where that holds.  (Before the sign alternation of conv_wgrad.hip it was 1.66e-6, 3.9 x.)
            _check(f"{tag} {prec}", "dw", dw, *r["dw"], rel, max(fro, 1.25 * 6 ** 0.5 * fro_bf16_dw))
        else:
            _check(f"{tag} {prec}", "dw", dw, *r["dw"], rel, fro)
        gsum = r["g"].double()
        _check(f"{tag} {prec}", "db", db, gsum.sum(dim=(0, 2, 3)), gsum.abs().sum(dim=(0, 2, 3)), rel if prec != "bf16" else BF_REL)


# ---------------------------------------------------------------------------------------------------- c. ticket ring wrap

def test_ticket_ring_wraps_without_losing_tiles():
    """264 masked launches that draw tickets (the x3 forward on conv_pc.h and the bf16 stride-2 data gradient, alternating two shapes each) go round the 64
    g_tile_ctr slots four times: every result is bit-equal to the first result of its shape, so sched_done re-armed every slot."""
    import torch.nn.functional as F

    from pillarnext_amd import ops
    from pillarnext_amd.train_nodes import _split_pack

    gen = torch.Generator(device="cuda").manual_seed(21)
    w64 = torch.randn((64, 64, 3, 3), device="cuda", generator=gen) * 0.06
    wh, wl = _split_pack(w64)
    w128 = torch.randn((128, 64, 3, 3), device="cuda", generator=gen) * 0.06
    wt = ops.conv3x3_pack_weights(w128, transposed=True)
    pc, dg = [], []
    for H, W in ((800, 512), (784, 544)):
        n, grid = _pc_grid(1, H, W, 64)
        assert n > 3 * grid, (n, grid)
        m = _lidar_mask(1, H, W, gen)
        xh, xl = ops.split_f32(_cl(torch.randn((1, 64, H, W), device="cuda", generator=gen) * m))
        pc.append((xh, xl, _u8(m)))
    for H, W in ((1040, 1040), (1000, 1100)):
        n, grid = _dgrad_s2_grid(1, H, W, 64, 128)
        assert n > 3 * grid, (n, grid)
        m = _lidar_mask(1, H, W, gen)
        mo = F.max_pool2d(m, 3, 2, 1)
        g = _cl(torch.randn((1, 128) + tuple(mo.shape[2:]), device="cuda", generator=gen) * mo).to(torch.bfloat16)
        dg.append((g, (H, W), _u8(m)))
    first_pc, first_dg = [None, None], [None, None]
    for i in range(132):
        s = i & 1
        xh, xl, mu = pc[s]
        y = ops.conv3x3_f32((xh, xl), (wh, wl), 64, 1, mu)
        g, hw, mi = dg[s]
        dx = ops.conv3x3_dgrad_s2(g, wt, 64, hw, mi)
        if first_pc[s] is None:
            first_pc[s], first_dg[s] = y, dx
            assert float(y.abs().sum()) > 0 and float(dx.float().abs().sum()) > 0
        else:
            assert torch.equal(y, first_pc[s]), ("conv_pc x3 forward differs at launch", 2 * i)
            assert torch.equal(dx, first_dg[s]), ("dgrad_s2 differs at launch", 2 * i + 1)


# ---------------------------------------------------------------------------------------------------- d. production shapes (C3)

@pytest.fixture(scope="module")
def c3_masks():
    """stage-0 / stage-1 active sets of a C3 step: the reader's occupancy of synth.make_batch("C2", 4, "sweep") on the 1440^2 grid, max-pooled the way
    SparseResNet does (stage 0's entry SparseConvBlock: 3x3 stride 1; stage 1's: 3x3 stride 2)"""
    import torch.nn.functional as F

    from pillarnext_amd import synth
    from pillarnext_amd.reader import PillarFeatureNet

    cfg = synth.CONFIGS["C2"]
    pts = torch.from_numpy(synth.make_batch("C2", 4, "sweep")).cuda()
    net = PillarFeatureNet(5, [64, 64], list(cfg["voxel_size"]), list(cfg["pc_range"])).cuda().eval()
    with torch.no_grad():
        _, coords, _ = net(pts, 4)
    occ = torch.zeros((4, 1, 1440, 1440), device="cuda")
    c = coords.long()
    occ[c[:, 0], 0, c[:, 1], c[:, 2]] = 1.0
    m0 = F.max_pool2d(occ, 3, 1, 1)
    return m0, F.max_pool2d(m0, 3, 2, 1)


@pytest.mark.parametrize("cin,cout,stride", [(64, 64, 1), (64, 128, 2)])
def test_conv_nodes_at_the_c3_training_shape(cin, cout, stride, c3_masks, monkeypatch):
    """stage 0's 64 -> 64 and stage 1's 64 -> 128 stride-2 entry at 4 x 1440^2 on the C3 occupancy: y, dx, dW of the bf16, three- and six-product nodes
    against fp64 on one set of operands; the six-product node to the CHANGELOG's figure (<= 1e-6 relative Frobenius, measured 3.9e-7 at C2 x 4 frames).
    The six-product weight gradient failed this at 3.6e-6 (every element low by the same amount: k_wgrad64's MFMAs round the small low-order products
    they add to a large running sum toward -inf, ~130 tiles per workgroup here); conv_wgrad.hip now alternates the sign of the sum from tile to tile."""
    from pillarnext_amd.models import _SpConv2d

    m0, m1 = c3_masks
    mask_in = m0
    mask_out = m0 if stride == 1 else m1
    B, H, W = 4, 1440, 1440
    G, mine, _ = _wgrad_split(_u8(mask_out), cin, cout, stride)
    n, grid = _pc_grid(B, H, W, cin) if stride == 1 else _dgrad_s2_grid(B, H, W, cin, cout)
    assert int(mine.min()) >= 3 and n > 3 * grid
    gen = torch.Generator(device="cuda").manual_seed(cout + stride)
    conv = _SpConv2d(cin, cout, 3, stride=stride, padding=1, bias=False).cuda().train()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, device="cuda", generator=gen) * (2.0 / (9 * cin)) ** 0.5)
    x0 = _cl(torch.randn((B, cin, H, W), device="cuda", generator=gen) * mask_in)
    g0 = _cl(torch.randn((B, cout) + tuple(mask_out.shape[2:]), device="cuda", generator=gen) * mask_out)
    tag = f"C3 {cin}->{cout} s{stride} ({int(mask_in.sum())} active inputs)"
    refs = {}
    for prec in ("bf16", "x3", "x6"):
        y, dx, dw = _run_node(prec, conv, x0, g0, mask_out, mask_in, monkeypatch)
        assert bool((y[(mask_out == 0).expand_as(y)] == 0).all()) and bool((dx[(mask_in == 0).expand_as(dx)] == 0).all())
        key = "bf16" if prec == "bf16" else "f32"
        if key not in refs:
            refs.clear()     # one reference alive at a time
            refs[key] = _conv_refs(*_operands(prec, x0, conv.weight, g0), mask_in, mask_out, stride)
        r = refs[key]
        rel, fro, ulp = _bars(prec)
        _check(f"{tag} {prec}", "y", _gather(y, r["so"]), *r["y"], rel, fro, ulp)
        _check(f"{tag} {prec}", "dx", _gather(dx, r["si"]), *r["dx"], rel, fro, ulp)
        _check(f"{tag} {prec}", "dw", dw, *r["dw"], rel, fro)
        del y, dx, dw


# ---------------------------------------------------------------------------------------------------- e. masked BatchNorm + residual + ReLU

# Bars.  fp32 sums of the statistics passes: a thread adds its ~n / (1024 rows) sites, a block its rows (256 * 8 / C of them, 128 at C = 16), both in
# fp32, the blocks in fp64: at most ~160 fp32 additions deep at the shapes below, 160 * 2^-24 < 2^-16 of the sum of |terms|.  Every quantity is held to
# 2^-16 of its own sum of |terms| (y: (|x| + |mean|) invstd |gamma| + |beta| + |residual|; dx: |gamma| invstd (|g| + mean |g| + (|x| + |mean|) invstd
# mean |g xhat|)); bf16 maps (fp32 inside the kernels) get one bf16 rounding of the output on top.  The upstream gradient is zero where the fp64
# pre-activation is within 2^-12 of its sum of |terms| from zero, so a ReLU gate never flips between kernel and reference.
BN_REL = 2.0 ** -16
BN_SHAPES = {16: (2, 1500, 1500), 64: (2, 800, 700), 128: (2, 600, 500), 256: (2, 300, 500)}


def _bn_guard(n, C):
    s_sites, nvec, s_vec = _mbn_strides(n, C)
    assert n > 2 * 4 * s_sites and n % s_sites, (n, s_sites)          # k_mbn_stats: u = 1..3 loads, two iterations, a tail
    assert nvec > 2 * 2 * s_vec and nvec % s_vec, (nvec, s_vec)       # apply passes: the second vector in flight, two iterations, a tail
    return s_sites, s_vec


def _bn_ref(x, mask, gamma, beta, res, relu, rm, rv, eps, mom):
    """fp64 statement: BatchNorm1d over the gathered active sites, scattered back, + residual, ReLU, mask"""
    m = mask.double()
    x64 = x.double()
    cnt = m.sum().clamp(min=1.0)
    mean = (x64 * m).sum(dim=(0, 2, 3)) / cnt
    var = (((x64 - mean.view(1, -1, 1, 1)) ** 2) * m).sum(dim=(0, 2, 3)) / cnt
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x64 - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
    g64, b64 = gamma.double().view(1, -1, 1, 1), beta.double().view(1, -1, 1, 1)
    pre = xhat * g64 + b64
    prea = (x64.abs() + mean.abs().view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1) * g64.abs() + b64.abs()
    if res is not None:
        pre = pre + res.double()
        prea = prea + res.double().abs()
    y = (pre.clamp(min=0) if relu else pre) * m
    r = dict(m=m, cnt=cnt, mean=mean, var=var, invstd=invstd, xhat=xhat, x64=x64, pre=pre, prea=prea, y=y, relu=relu, gamma=gamma.double())
    r["rm"] = (1 - mom) * rm.double() + mom * mean
    r["rv"] = (1 - mom) * rv.double() + mom * var * cnt / (cnt - 1).clamp(min=1.0)
    return r


def _bn_ref_backward(r, gy):
    m, cnt, invstd, xhat = r["m"], r["cnt"], r["invstd"], r["xhat"]
    g = gy.double() * m
    if r["relu"]:
        g = g * (r["pre"] > 0)
    dbeta, dgamma = g.sum(dim=(0, 2, 3)), (g * xhat).sum(dim=(0, 2, 3))
    a = (r["gamma"] * invstd).view(1, -1, 1, 1)
    dx = a * (g - (dbeta / cnt).view(1, -1, 1, 1) - xhat * (dgamma / cnt).view(1, -1, 1, 1)) * m
    mg = (g.abs().sum(dim=(0, 2, 3)) / cnt).view(1, -1, 1, 1)
    mgx = ((g * xhat).abs().sum(dim=(0, 2, 3)) / cnt).view(1, -1, 1, 1)
    xa = (r["x64"].abs() + r["mean"].abs().view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
    dxa = a.abs() * (g.abs() + mg + xa * mgx) * m
    return dict(g=g, dbeta=dbeta, dgamma=dgamma, dbeta_a=g.abs().sum(dim=(0, 2, 3)), dgamma_a=(g.abs() * xa).sum(dim=(0, 2, 3)), dx=dx, dxa=dxa)


def _bn_case(C, shape, dtype, with_res, relu, first_step, gen):
    from pillarnext_amd.models import MaskedBatchNorm

    B, H, W = shape
    mask = (torch.rand((B, 1, H, W), device="cuda", generator=gen) < 0.3).float()
    ch_std = torch.rand(C, device="cuda", generator=gen) + 0.5
    ch_mean = (2 * torch.rand(C, device="cuda", generator=gen) - 1) * ch_std * (30.0 if first_step else 2.0)
    if first_step:
        ch_mean[0] = 30.0 * ch_std[0]                                   # channel 0 at mean / std = 30 exactly
    x = _cl((torch.randn((B, C, H, W), device="cuda", generator=gen) * ch_std.view(1, -1, 1, 1) + ch_mean.view(1, -1, 1, 1)).to(dtype))
    res = _cl(torch.randn((B, C, H, W), device="cuda", generator=gen).to(dtype)) if with_res else None
    n = MaskedBatchNorm(C, eps=1e-3, momentum=0.01).cuda().train()
    with torch.no_grad():
        n.weight.copy_(torch.rand(C, device="cuda", generator=gen) + 0.5)
        n.bias.copy_(torch.randn(C, device="cuda", generator=gen) * 0.3)
        if not first_step:     # steady state: the running mean within a tenth of a std of the batch mean
            n.running_mean.copy_(ch_mean + 0.1 * ch_std * torch.randn(C, device="cuda", generator=gen))
            n.running_var.copy_(ch_std ** 2)
    return mask, x, res, n


def _bn_run(x, mask, n, res, relu, gy):
    from pillarnext_amd.models import masked_bn_act

    xa = x.clone().requires_grad_(True)
    ra = res.clone().requires_grad_(True) if res is not None else None
    y = masked_bn_act(xa, mask, n, residual=ra, relu=relu)
    assert type(y.grad_fn).__name__ == "_MaskedBNActFnBackward"
    y.backward(gy)
    return y.detach(), xa.grad, None if ra is None else ra.grad


def _bn_check(tag, C, dtype, mask, x, res, n, relu, gen):
    rm0, rv0 = n.running_mean.clone(), n.running_var.clone()
    r = _bn_ref(x, mask, n.weight.detach(), n.bias.detach(), res, relu, rm0, rv0, n.eps, n.momentum)
    gy = torch.randn(x.shape, device="cuda", generator=gen)
    if relu:
        gy = gy * ((r["pre"].abs() > 2.0 ** -12 * r["prea"]) | (mask == 0))
    gy = _cl(gy.to(dtype))
    y, dx, dres = _bn_run(x, mask, n, res, relu, gy)
    rb = _bn_ref_backward(r, gy)
    ulp = BF_OUT if dtype == torch.bfloat16 else 0.0
    act = (mask != 0).expand_as(x)
    assert bool((y[~act] == 0).all()) and bool((dx[~act] == 0).all()), (tag, "inactive sites")
    ya = (r["prea"] * r["m"])[act]
    _check(tag, "y", y[act], r["y"][act], ya, BN_REL, None, ulp)
    _check(tag, "dx", dx[act], rb["dx"][act], rb["dxa"][act], BN_REL, None, ulp)
    if res is not None:
        assert torch.equal(dres.double(), rb["g"]), (tag, "dresidual is the gated upstream gradient, exactly")
    _check(tag, "dgamma", n.weight.grad, rb["dgamma"], rb["dgamma_a"], BN_REL)
    _check(tag, "dbeta", n.bias.grad, rb["dbeta"], rb["dbeta_a"], BN_REL)
    sd = r["var"].sqrt()
    _check(tag, "running_mean", n.running_mean, r["rm"], rm0.double().abs() + n.momentum * (r["mean"].abs() + sd), BN_REL)
    _check(tag, "running_var", n.running_var, r["rv"], rv0.double().abs() + n.momentum * r["var"] * 2, BN_REL)
    assert int(n.num_batches_tracked) == 1


@pytest.mark.parametrize("with_res,relu", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [16, 64, 128, 256])
def test_masked_bn_over_many_sites_per_thread(monkeypatch, C, dtype, with_res, relu):
    """models.masked_bn_act on csrc/masked_bn.hip (steady state: running mean near the batch mean) with every site / vector slot of the unrolled walks
    in use and a tail: y, dx, dresidual, dgamma, dbeta, running statistics against the fp64 statement of BatchNorm1d over the gathered active sites."""
    monkeypatch.setenv("PNX_MASKED_BN_HIP", "1")
    shape = BN_SHAPES[C]
    _bn_guard(shape[0] * shape[1] * shape[2], C)
    gen = torch.Generator(device="cuda").manual_seed(C + 2 * with_res + relu + (dtype == torch.bfloat16) * 10)
    mask, x, res, n = _bn_case(C, shape, dtype, with_res, relu, False, gen)
    _bn_check(f"masked BN C={C} {str(dtype)[6:]} res={with_res} relu={relu}", C, dtype, mask, x, res, n, relu, gen)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [64, 256])
def test_masked_bn_first_step_far_from_the_running_mean(monkeypatch, C, dtype):
    """The first training step: running_mean = 0 while the channel means reach 30 x the std.  The statistics pass sums around the running mean; the
    variance must not lose its leading digits to E[d^2] - E[d]^2 (held to the same bars as the steady state)."""
    monkeypatch.setenv("PNX_MASKED_BN_HIP", "1")
    shape = BN_SHAPES[C]
    _bn_guard(shape[0] * shape[1] * shape[2], C)
    gen = torch.Generator(device="cuda").manual_seed(3 * C + (dtype == torch.bfloat16))
    mask, x, res, n = _bn_case(C, shape, dtype, True, True, True, gen)
    _bn_check(f"masked BN first step C={C} {str(dtype)[6:]}", C, dtype, mask, x, res, n, True, gen)


@pytest.mark.parametrize("case", ["none", "one", "all"])
def test_masked_bn_edge_counts_match_the_torch_statement(monkeypatch, case):
    """zero active sites in the whole batch, exactly one, every one (at the C = 64 multi-iteration shape): the HIP node against the torch statement
    (PNX_MASKED_BN_HIP=0, the same count clamp to 1): outputs, gradients, running statistics, at the tolerances of tests/test_gpu_masked_bn.py.
    With no active site the batch mean is 0 in the torch statement; k_mbn_finalize reported the running mean (its centre) instead, which moved the
    running mean by momentum x running_mean less than the statement did (fixed in csrc/masked_bn.hip)."""
    C, shape = 64, BN_SHAPES[64]
    B, H, W = shape
    gen = torch.Generator(device="cuda").manual_seed(99)
    _, x, res, _ = _bn_case(C, shape, torch.float32, True, True, False, gen)
    mask = torch.zeros((B, 1, H, W), device="cuda")
    if case == "one":
        mask[1, 0, H - 1, W - 3] = 1.0          # in the tail of the walks
    elif case == "all":
        mask.fill_(1.0)
    _, _, _, n = _bn_case(C, (1, 1, 8), torch.float32, True, True, False, torch.Generator(device="cuda").manual_seed(5))
    r = _bn_ref(x, mask, n.weight.detach(), n.bias.detach(), res, True, n.running_mean, n.running_var, n.eps, n.momentum)
    gy = torch.randn(x.shape, device="cuda", generator=gen)
    gy = _cl(gy * ((r["pre"].abs() > 2.0 ** -12 * r["prea"]) | (mask == 0)))      # no ReLU gate within rounding of zero (see BN_REL)
    del r
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("PNX_MASKED_BN_HIP", mode)
        _, _, _, n = _bn_case(C, (1, 1, 8), torch.float32, True, True, False, torch.Generator(device="cuda").manual_seed(5))
        y, dx, dres = _bn_run(x, mask, n, res, True, gy)
        out[mode] = (y, dx, dres, n.weight.grad, n.bias.grad, n.running_mean, n.running_var, int(n.num_batches_tracked))
    a, b = out["1"], out["0"]
    tols = (1e-4, 2e-4, 1e-5, 1e-3, 1e-3, None, None)
    for i, name in enumerate(("y", "dx", "dresidual", "dgamma", "dbeta", "running_mean", "running_var")):
        if tols[i] is None:
            tol = dict(rtol=1e-4, atol=1e-5)
        else:
            tol = dict(rtol=tols[i], atol=tols[i] * (max(1.0, float(b[i].abs().max())) if name in ("dgamma", "dbeta") else 1.0))
        torch.testing.assert_close(a[i], b[i], **tol, msg=lambda s, name=name: f"{case} {name}: {s}")
    assert a[7] == b[7] == 1
    if case == "none":
        assert float(a[0].abs().max()) == 0.0 and float(a[1].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- f. SepHead output convolution

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_sephead_output_convolution_on_the_c2_head_map(k, dtype):
    """_SmallKConv3x3Fn (csrc/head_train.hip: forward and weight / bias gradient) on the C2 head map, B = 4, 64 -> k at 360^2: several units per wave.
    fp64 bars of test_sephead_output_convolution_kernels."""
    from pillarnext_amd.models import smallk_conv

    B, H, W = 4, 360, 360
    units, waves = _smallk_units(B, H, W)
    assert units > 3 * waves, (units, waves)
    gen = torch.Generator(device="cuda").manual_seed(31 * k + (dtype == torch.bfloat16))
    conv = torch.nn.Conv2d(64, k, 3, padding=1, bias=True).cuda().train()
    with torch.no_grad():
        conv.bias.copy_(torch.randn(k, device="cuda", generator=gen))
    x0 = _cl(torch.randn((B, 64, H, W), device="cuda", generator=gen).to(dtype))
    g0 = torch.randn((B, k, H, W), device="cuda", generator=gen).to(dtype)
    x = x0.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        y = smallk_conv(conv, x)
    assert y.dtype == dtype and type(y.grad_fn).__name__ == "_SmallKConv3x3FnBackward"
    y.backward(g0)
    ones = torch.ones((B, 1, H, W), device="cuda")
    r = _conv_refs(x0, conv.weight, g0, ones, ones, 1)
    bias = conv.bias.detach().double()
    tag = f"smallk 64->{k} {str(dtype)[6:]} ({units} units, {waves} waves)"
    yr, ya = r["y"]
    _check(tag, "y", _gather(y, r["so"]), yr + bias, ya + bias.abs(), BF_REL, None, BF_OUT if dtype == torch.bfloat16 else 0.0)
    _check(tag, "dw", conv.weight.grad, *r["dw"], BF_REL)
    g64 = g0.double()
    _check(tag, "db", conv.bias.grad, g64.sum(dim=(0, 2, 3)), g64.abs().sum(dim=(0, 2, 3)), BF_REL)
