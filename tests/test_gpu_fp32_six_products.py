"""GPU: the six-product form of the fp32 training graph's 3x3 layers (PNX_TRAIN_F32_PIECES=3): every fp32 operand split into three bf16 pieces
(pnx_split3_f32), the six products of piece orders 0..2 accumulated in fp32 (pnx_conv3x3_x6, pnx_conv3x3_dgrad_s2_x6, pnx_conv3x3_wgrad_x6), against
the fp64 autograd of the same convolution on the same fp32 operands.  Bars: 2^-19 of the sum of |terms| per element, 1e-6 relative Frobenius (the
three-product node is at ~4e-6); MIOpen's fp32 error on the same operands is printed beside each result (-rP)."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

REL = 2.0 ** -19
FRO = 1e-6

BACKBONE = [(64, 64, 1, True, (2, 70, 97)), (64, 64, 1, False, (2, 48, 64)), (128, 128, 1, True, (2, 41, 70)), (256, 256, 1, True, (2, 23, 33)),
            (64, 128, 2, False, (2, 50, 66)), (128, 256, 2, False, (1, 37, 41)), (256, 256, 2, False, (2, 24, 64)), (64, 64, 1, True, (1, 16, 32)),
            (128, 128, 1, True, (1, 8, 33))]


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


def _fro(a, r):
    return float((a.double() - r).norm() / r.norm())


def _wide_values(shape, gen):
    """random fp32 values of both signs with |x| spread over [2^-100, 2^120], some zeros"""
    e = torch.randint(-100, 120, shape, device="cuda", generator=gen).float()
    m = 1.0 + torch.rand(shape, device="cuda", generator=gen)
    s = torch.where(torch.rand(shape, device="cuda", generator=gen) < 0.5, -1.0, 1.0)
    x = s * m * torch.exp2(e)
    return torch.where(torch.rand(shape, device="cuda", generator=gen) < 0.02, torch.zeros_like(x), x)


def _bits(t):
    return t.view(torch.int16)


def test_split3_pieces_are_exact():
    from pillarnext_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(11)
    x = _wide_values((3, 64, 17, 8), gen).contiguous(memory_format=torch.channels_last)
    x[0, 0, 0, :2] = torch.tensor([0.0, -0.0], device="cuda")
    hi, mid, lo = ops.split_f32(x, pieces=3)
    for p in (hi, mid, lo):
        assert p.dtype == torch.bfloat16 and p.is_contiguous(memory_format=torch.channels_last) and p.shape == x.shape
    assert torch.equal(_bits(hi), _bits(x.to(torch.bfloat16)))                          # hi = RNE(x), like torch's cast
    assert torch.equal((hi.double() + mid.double() + lo.double()), x.double())         # exact in fp64
    r = x - hi.float()
    assert torch.equal(_bits(mid), _bits(r.to(torch.bfloat16))) and torch.equal(lo.float(), r - mid.float())
    # with a mask: inactive sites are not read (NaN there), zeros are written
    m = (torch.rand((3, 17, 8), device="cuda", generator=gen) < 0.4).to(torch.uint8)
    keep = m[:, None].bool().expand_as(x)
    xm = torch.where(keep, x, torch.full_like(x, float("nan")))
    for got, want in zip(ops.split_f32(xm, m, pieces=3), (hi, mid, lo)):
        assert torch.equal(_bits(got)[keep], _bits(want)[keep]) and bool((_bits(got)[~keep] == 0).all())
    # non-finite values: the convention of pnx_split_f32 (hi = the bf16 cast; the lower pieces of an inf / nan are nan)
    xn = x.clone()
    xn[1, :3, 2, 3] = torch.tensor([float("inf"), -float("inf"), float("nan")], device="cuda")
    h3, m3, l3 = ops.split_f32(xn, pieces=3)
    h2, l2 = ops.split_f32(xn)
    bad = ~torch.isfinite(xn)
    assert torch.equal(_bits(h3), _bits(h2))
    assert bool(torch.isnan(m3[bad]).all()) and bool(torch.isnan(l3[bad]).all()) and bool(torch.isnan(l2[bad]).all())
    with pytest.raises(Exception):
        ops.split_f32(x.contiguous(), m, pieces=3)           # the mask form is for channels_last maps


def _run_backbone(cin, cout, stride, subm, shape, monkeypatch, pieces="3", x_scale=None, g_scale=1.0):
    import torch.nn.functional as F

    from pillarnext_amd.models import _SpConv2d, masked_conv

    if pieces is None:
        monkeypatch.delenv("PNX_TRAIN_F32_PIECES", raising=False)
    else:
        monkeypatch.setenv("PNX_TRAIN_F32_PIECES", pieces)
    B, H, W = shape
    gen = torch.Generator(device="cuda").manual_seed(3 * cin + cout + H)
    mask_in = _lidar_mask(B, H, W, gen)
    mask_out = mask_in if subm else F.max_pool2d(mask_in, 3, stride, 1)
    conv = _SpConv2d(cin, cout, 3, stride=stride, padding=1, bias=False).cuda().train()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, device="cuda", generator=gen) * (2.0 / (9 * cin)) ** 0.5)
    x0 = torch.randn((B, cin, H, W), device="cuda", generator=gen) * mask_in
    if x_scale is not None:
        x0 = x0 * x_scale.view(1, cin, 1, 1)
    x0 = x0.contiguous(memory_format=torch.channels_last)
    Ho, Wo = mask_out.shape[2:]
    g0 = (torch.randn((B, cout, Ho, Wo), device="cuda", generator=gen) * mask_out * g_scale).contiguous(memory_format=torch.channels_last)
    x = x0.clone().requires_grad_(True)
    y = masked_conv(conv, x, mask_out, mask_in)
    y.backward(g0)
    return dict(conv=conv, x0=x0, g0=g0, mask_in=mask_in, mask_out=mask_out, y=y, dx=x.grad, dw=conv.weight.grad, stride=stride)


def _check_against_fp64(r, tag):
    """elementwise 2^-19 of the sum of |terms|, relative Frobenius 1e-6, zeros at inactive sites; MIOpen's fp32 error printed beside"""
    import torch.nn.functional as F

    conv, x0, g0, mask_in, mask_out, s = r["conv"], r["x0"], r["g0"], r["mask_in"], r["mask_out"], r["stride"]
    y, dx, dw = r["y"], r["dx"], r["dw"]
    assert y.dtype == torch.float32 and type(y.grad_fn).__name__.startswith("_MaskedConv3x3F32Fn")
    xr = x0.double().contiguous().requires_grad_(True)
    wr = conv.weight.detach().double().requires_grad_(True)
    yr = F.conv2d(xr, wr, None, s, 1) * mask_out.double()
    yr.backward(g0.double())
    # MIOpen fp32 on the same operands
    xm = x0.clone().requires_grad_(True)
    wm = conv.weight.detach().clone().requires_grad_(True)
    ym = F.conv2d(xm, wm, None, s, 1) * mask_out
    ym.backward(g0)
    ya = F.conv2d(x0.double().abs(), wr.detach().abs(), None, s, 1)
    dxa = torch.nn.grad.conv2d_input(xr.shape, wr.detach().abs(), g0.double().abs(), stride=s, padding=1)
    dwa = torch.nn.grad.conv2d_weight(x0.double().abs(), wr.shape, g0.double().abs(), stride=s, padding=1)
    dxr = xr.grad * mask_in
    tiny = 2.0 ** -126
    assert bool(((y.double() - yr.detach()).abs() <= REL * ya + tiny).all()), (tag, "y", float(((y.double() - yr.detach()).abs() / (ya + tiny)).max()))
    assert bool((y[(mask_out == 0).expand_as(y)] == 0).all())
    dxm = dx.double() * mask_in
    assert bool(((dxm - dxr).abs() <= REL * dxa + tiny).all()), (tag, "dx", float(((dxm - dxr).abs() / (dxa + tiny)).max()))
    assert bool((dx[(mask_in == 0).expand_as(dx)] == 0).all())
    assert bool(((dw.double() - wr.grad).abs() <= REL * dwa + tiny).all()), (tag, "dw", float(((dw.double() - wr.grad).abs() / (dwa + tiny)).max()))
    for name, a, ref, mio in (("y", y, yr.detach(), ym), ("dx", dxm, dxr, xm.grad * mask_in), ("dw", dw, wr.grad, wm.grad)):
        e, em = _fro(a, ref), _fro(mio, ref)
        print(f"six-product {tag} {name}: relative error {e:.2e}   (MIOpen fp32 on the same operands: {em:.2e})")
        assert e <= FRO, (tag, name, e, em)


@pytest.mark.parametrize("cin,cout,stride,subm,shape", BACKBONE)
def test_six_product_node_against_fp64(cin, cout, stride, subm, shape, monkeypatch):
    """train_nodes._MaskedConv3x3F32Fn under PNX_TRAIN_F32_PIECES=3 on the nine cases of the three-product test (which holds that node to 2^-14 / 3e-5)."""
    r = _run_backbone(cin, cout, stride, subm, shape, monkeypatch)
    _check_against_fp64(r, f"{cin}->{cout} s{stride}")


@pytest.mark.parametrize("case,x_range,g_scale", [(0, None, 2.0 ** -60), (0, None, 2.0 ** 40), (0, 30, 1.0), (4, None, 2.0 ** -60), (4, 30, 2.0 ** 40),
                                                  (6, 30, 1.0)])
def test_six_product_node_on_wide_range_operands(case, x_range, g_scale, monkeypatch):
    """Gradient maps scaled by 2^-60 / 2^40 and input channels scaled by 2^-30 .. 2^30: bf16 pieces carry fp32's exponent range, the bars stay."""
    cin, cout, stride, subm, shape = BACKBONE[case]
    x_scale = None
    if x_range is not None:
        x_scale = torch.exp2(torch.linspace(-x_range, x_range, cin, device="cuda"))[torch.randperm(cin, device="cuda", generator=torch.Generator(device="cuda").manual_seed(cin))]
    r = _run_backbone(cin, cout, stride, subm, shape, monkeypatch, x_scale=x_scale, g_scale=g_scale)
    _check_against_fp64(r, f"{cin}->{cout} s{stride} x 2^+-{x_range} g {g_scale:.0e}")


@pytest.mark.parametrize("c,shape,shared", [(64, (2, 40, 72), True), (64, (1, 17, 40), False), (128, (1, 9, 31), True), (128, (2, 20, 24), False),
                                            (256, (1, 20, 33), False), (256, (1, 12, 16), True)])
def test_dense_layers_on_six_products(c, shape, shared, monkeypatch):
    """models.x3_conv (the neck's / head's dense 3x3 nn.Conv2d with bias) under PNX_TRAIN_F32_PIECES=3: y, dx, dw, db to 1e-6 of fp64; `shared`: x split
    once by the caller (models.split_f32_pieces, as SepHead.forward does)."""
    import torch.nn.functional as F

    from pillarnext_amd.models import split_f32_pieces, x3_conv

    monkeypatch.setenv("PNX_TRAIN_F32_PIECES", "3")
    B, H, W = shape
    gen = torch.Generator(device="cuda").manual_seed(c + H)
    conv = torch.nn.Conv2d(c, c, 3, padding=1, bias=True).cuda().train()
    with torch.no_grad():
        conv.bias.copy_(torch.randn(c, device="cuda", generator=gen))
    x0 = torch.randn((B, c, H, W), device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    g0 = torch.randn((B, c, H, W), device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    x = x0.clone().requires_grad_(True)
    pieces = split_f32_pieces(x.detach()) if shared else None
    assert pieces is None or len(pieces) == 3
    y = x3_conv(conv, x, pieces)
    assert type(y.grad_fn).__name__.startswith("_MaskedConv3x3F32Fn")
    y.backward(g0)
    xr, wr, br = x0.double().requires_grad_(True), conv.weight.detach().double().requires_grad_(True), conv.bias.detach().double().requires_grad_(True)
    yr = F.conv2d(xr, wr, br, 1, 1)
    yr.backward(g0.double())
    for name, a, r in (("y", y, yr.detach()), ("dx", x.grad, xr.grad), ("dw", conv.weight.grad, wr.grad), ("db", conv.bias.grad, br.grad)):
        e = _fro(a, r)
        print(f"six-product dense {c} {name}: relative error {e:.2e}")
        assert e <= FRO, (name, e)


def test_default_is_the_three_product_node(monkeypatch):
    """With PNX_TRAIN_F32_PIECES unset the node is today's: outputs and gradients bit for bit those of PNX_TRAIN_F32_PIECES=2 and of the three-product
    kernels called directly, on one backbone layer and one dense layer; the same autograd node."""
    import torch.nn.functional as F

    from pillarnext_amd import ops
    from pillarnext_amd.models import x3_conv
    from pillarnext_amd.train_nodes import _split_pack

    for case in (0, 4):
        runs = [_run_backbone(*BACKBONE[case], monkeypatch, pieces=p) for p in (None, "2")]
        for k in ("y", "dx", "dw"):
            assert torch.equal(runs[0][k], runs[1][k]), (case, k)
        assert type(runs[0]["y"].grad_fn) is type(runs[1]["y"].grad_fn)
        r = runs[0]
        mi, mo = r["mask_in"][:, 0].to(torch.uint8).contiguous(), r["mask_out"][:, 0].to(torch.uint8).contiguous()
        w = r["conv"].weight
        xh, xl = ops.split_f32(r["x0"], mi)
        wh, wl = _split_pack(w)
        assert torch.equal(r["y"], ops.conv3x3_f32((xh, xl), (wh, wl), w.shape[0], r["stride"], mo))
        gh, gl = ops.split_f32(r["g0"], mo)
        assert torch.equal(r["dw"], ops.conv3x3_wgrad((xh, xl), (gh, gl), mo, stride=r["stride"]))
        wth, wtl = _split_pack(w, transposed=True)
        if r["stride"] == 1:
            dx = ops.conv3x3_f32((gh, gl), (wth, wtl), w.shape[1], 1, mi)
        else:
            dx = ops.conv3x3_dgrad_s2((gh, gl), (wth, wtl), w.shape[1], r["x0"].shape[2:], mi)
        assert torch.equal(r["dx"], dx)
    # a dense layer (bias)
    gen = torch.Generator(device="cuda").manual_seed(7)
    conv = torch.nn.Conv2d(128, 128, 3, padding=1, bias=True).cuda().train()
    x0 = torch.randn((1, 128, 19, 40), device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    g0 = torch.randn((1, 128, 19, 40), device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    outs = []
    for p in (None, "2"):
        if p is None:
            monkeypatch.delenv("PNX_TRAIN_F32_PIECES", raising=False)
        else:
            monkeypatch.setenv("PNX_TRAIN_F32_PIECES", p)
        conv.weight.grad = conv.bias.grad = None
        x = x0.clone().requires_grad_(True)
        y = x3_conv(conv, x)
        y.backward(g0)
        outs.append((y, x.grad, conv.weight.grad.clone(), conv.bias.grad.clone(), type(y.grad_fn)))
    for a, b in zip(outs[0], outs[1]):
        assert a is b if isinstance(a, type) else torch.equal(a, b)
    xh, xl = ops.split_f32(x0)
    wh, wl = _split_pack(conv.weight)
    assert torch.equal(outs[0][0], ops.conv3x3_f32((xh, xl), (wh, wl), 128, 1, None, bias=conv.bias.detach()))
    # the six-product form is another computation (closer to fp64)
    monkeypatch.setenv("PNX_TRAIN_F32_PIECES", "3")
    y6 = x3_conv(conv, x0.clone().requires_grad_(True))
    yr = F.conv2d(x0.double(), conv.weight.detach().double(), conv.bias.detach().double(), 1, 1)
    assert _fro(y6, yr) < _fro(outs[0][0], yr)


def test_bad_piece_count_raises(monkeypatch):
    from pillarnext_amd import ops
    from pillarnext_amd.models import _SpConv2d, masked_conv

    conv = _SpConv2d(64, 64, 3, stride=1, padding=1, bias=False).cuda().train()
    x = torch.randn((1, 64, 16, 32), device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
    m = torch.ones((1, 1, 16, 32), device="cuda")
    monkeypatch.setenv("PNX_TRAIN_F32_PIECES", "4")
    with pytest.raises(ops.PnxError):
        masked_conv(conv, x, m, m)
    monkeypatch.setenv("PNX_TRAIN_F32_HIP", "0")    # MIOpen: the switch is not read
    assert not type(masked_conv(conv, x, m, m).grad_fn).__name__.startswith("_MaskedConv3x3")


def test_sephead_training_path_on_six_products(monkeypatch):
    """SepHead.forward in training under PNX_TRAIN_F32_PIECES=3 (as test_sephead_training_path_against_its_modules): every parameter gradient no further
    from the fp64 modules than the MIOpen fp32 graph's (PNX_TRAIN_F32_HIP=0) is, x 2 + 1e-6.  Distances: Frobenius norm of the difference over
    max(|reference|, 1e-3 of the largest gradient) -- the biases in front of a BatchNorm have an exact gradient of zero."""
    import copy

    from pillarnext_amd.models import SepHead

    torch.manual_seed(4)
    heads = {"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2), "hm": (2, 2)}
    head = SepHead(64, heads, stride=1, head_conv=64, final_kernel=3, bn=True).cuda().train().to(memory_format=torch.channels_last)
    mio = copy.deepcopy(head)
    ref = copy.deepcopy(head)
    x0 = torch.randn((2, 64, 40, 56), device="cuda").contiguous(memory_format=torch.channels_last)
    gs = {h: torch.randn((2, heads[h][0], 40, 56), device="cuda") for h in heads}

    def run(m, x):
        out = m(x)
        sum((out[h] * gs[h].to(out[h].dtype)).sum() for h in heads).backward()
        return out

    monkeypatch.setenv("PNX_TRAIN_F32_PIECES", "3")
    xa = x0.clone().requires_grad_(True)
    run(head, xa)
    monkeypatch.setenv("PNX_TRAIN_F32_HIP", "0")
    xm = x0.clone().requires_grad_(True)
    run(mio, xm)
    for k in ("PNX_TRAIN_DENSE_HIP", "PNX_TRAIN_HEAD_HIP", "PNX_TRAIN_DENSE_BN_HIP"):
        monkeypatch.setenv(k, "0")
    ref = ref.double().to(memory_format=torch.contiguous_format)
    xb = x0.double().contiguous().requires_grad_(True)
    run(ref, xb)
    big = max(float(r.grad.norm()) for r in ref.parameters())

    def dist(a, r):
        return float((a.double() - r).norm()) / max(float(r.norm()), 1e-3 * big)

    grads = [("input", xa.grad, xm.grad, xb.grad)] + [(n, p.grad, q.grad, r.grad) for (n, p), (_, q), (_, r) in
                                                      zip(head.named_parameters(), mio.named_parameters(), ref.named_parameters())]
    worst = []
    for n, a, m, r in grads:
        e, em = dist(a, r), dist(m, r)
        worst.append((e - 2 * em, n, e, em))
        print(f"sephead {n}: six-product {e:.2e}  MIOpen fp32 {em:.2e}")
    bad = [w for w in worst if w[2] > 2 * w[3] + 1e-6]
    assert not bad, bad
