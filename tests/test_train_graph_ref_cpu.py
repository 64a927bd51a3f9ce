"""CPU: tests/train_graph_ref.py (what tests/test_gpu_train_graph_vs_fp64.py holds the HIP training graph to) proven without a GPU.

  statements   every fp64 statement against torch.autograd of the plain modules / functions in fp64, 1e-10 of sum|terms|;
  harness      the recorder plus every wiring, fork and value check on the plain fp32 module graph (the helpers fall back to the modules on the CPU)
               from a synthetic canvas: fork accounting, the checkpoint's second call, the two-update running statistics.  fp32 bars: 2^-20 of
               sum|terms| per convolution node, BN_REL per BatchNorm node;
  gate cap     the fp64 plain-module graph at the GPU test's own geometry, clouds' occupancy and initialisation: ambiguous ReLU gates <= 2^-9 per node
               (the GPU test allows 2^-8);
  seeded mistakes   six wiring / scaling mistakes applied to the CPU graph by monkeypatch: the harness flags each one."""
import copy
import types

import pytest

torch = pytest.importorskip("torch")

import torch.nn.functional as F  # noqa: E402

import train_graph_ref as T  # noqa: E402

RTOL = 1e-10
SMALL_RANGE = (-4.0, -2.4, -5.0, 4.0, 2.4, 3.0)      # 24 x 40 cells of 0.2 m


def _close(tag, got, ref, terms):
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert bool((terms * (1 + 1e-12) + 1e-300 >= ref.abs()).all()), (tag, "sum|terms| does not bound the statement")
    assert float(terms.max()) > 0, tag
    assert bool(((got - ref).abs() <= RTOL * terms + 1e-300).all()), (tag, float(((got - ref).abs() / (terms + 1e-300)).max()))


def _masks(gen, B, H, W, p=0.2):
    m = (torch.rand((B, 1, H, W), generator=gen) < p).float()
    m[-1] = 0          # an empty sample
    return m


# ---------------------------------------------------------------------------------------------------- statements against autograd
@pytest.mark.parametrize("stride,dense,bias", [(1, False, False), (2, False, False), (1, True, True)])
def test_conv3x3_statement_is_autograd_of_the_masked_convolution(stride, dense, bias):
    gen = torch.Generator().manual_seed(3 + stride + dense)
    B, ci, co, H, W = 2, 8, 12, 24, 40
    m_in = torch.ones((B, 1, H, W)) if dense else _masks(gen, B, H, W)
    m_out = m_in if stride == 1 else F.max_pool2d(m_in, 3, 2, 1)
    x = (torch.randn((B, ci, H, W), generator=gen, dtype=torch.float64) * m_in).requires_grad_(True)
    w = torch.randn((co, ci, 3, 3), generator=gen, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(co, generator=gen, dtype=torch.float64).requires_grad_(True) if bias else None
    y = F.conv2d(x, w, b, stride, 1) * m_out
    g = torch.randn(y.shape, generator=gen, dtype=torch.float64) * m_out
    grads = torch.autograd.grad(y, (x, w) + ((b,) if bias else ()), g)
    r = T.conv3x3_statement(x, w, b, g, m_in, m_out, stride)
    _close("y", r["y"][0], T._gather(y, r["so"]), r["y"][1])
    _close("dx", r["dx"][0], T._gather(grads[0], r["si"]), r["dx"][1])
    _close("dw", r["dw"][0], grads[1], r["dw"][1])
    if bias:
        _close("db", r["db"][0], grads[2], r["db"][1])
    assert r["y"][0].shape[0] == int(m_out.sum()) and r["dx"][0].shape[0] == int(m_in.sum())


@pytest.mark.parametrize("case", ["1x1", "3x3 bias", "dilated 6", "transposed 2x2"])
def test_library_statement_is_autograd_of_the_torch_convolution(case):
    gen = torch.Generator().manual_seed(len(case))
    x = torch.randn((2, 6, 9, 13), generator=gen, dtype=torch.float64).requires_grad_(True)
    k, pad, dil, tr = {"1x1": (1, 0, 1, False), "3x3 bias": (3, 1, 1, False), "dilated 6": (3, 6, 6, False), "transposed 2x2": (2, 0, 1, True)}[case]
    w = torch.randn((6, 5, k, k) if tr else (5, 6, k, k), generator=gen, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(5, generator=gen, dtype=torch.float64).requires_grad_(True) if "bias" in case else None
    y = F.conv_transpose2d(x, w, None, 2) if tr else F.conv2d(x, w, b, 1, pad, dil)
    g = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    grads = torch.autograd.grad(y, (x, w) + ((b,) if b is not None else ()), g)
    r = T.lib_conv_statement(x, w, b, g, 1, pad, dil, tr)
    for name, want in zip(("y", "dx", "dw", "db"), (y.detach(),) + grads):
        _close(f"{case} {name}", r[name][0], want, r[name][1])


@pytest.mark.parametrize("dense,with_res", [(False, False), (False, True), (True, False)])
def test_bn_statement_is_autograd_of_the_modules(dense, with_res):
    """BatchNorm over the active sites (nn.BatchNorm1d on the gathered sites, scattered back: what sparse_conv.py applies to a sparse tensor's features;
    models.MaskedBatchNorm computes in fp32 whatever it is given; nn.BatchNorm2d for the dense layers) + residual + ReLU + mask, in fp64: y, dx, dresidual,
    dgamma, dbeta, and the running statistics after the call"""
    gen = torch.Generator().manual_seed(17 + dense + 2 * with_res)
    B, C, H, W = 2, 8, 24, 40
    mask = None if dense else _masks(gen, B, H, W)
    norm = (torch.nn.BatchNorm2d(C) if dense else torch.nn.BatchNorm1d(C, eps=1e-3, momentum=0.01)).double().train()
    with torch.no_grad():
        for t in (norm.weight, norm.bias, norm.running_mean, norm.running_var):
            t.copy_(torch.rand(C, generator=gen, dtype=torch.float64) + 0.5)
    x = (torch.randn((B, C, H, W), generator=gen, dtype=torch.float64) * 1.5 + 0.3).requires_grad_(True)
    res = torch.randn((B, C, H, W), generator=gen, dtype=torch.float64).requires_grad_(True) if with_res else None
    call = dict(x=x.detach(), mask=mask, residual=None if res is None else res.detach(), gamma=norm.weight.detach().clone(), beta=norm.bias.detach().clone(),
                rm=norm.running_mean.clone(), rv=norm.running_var.clone())
    if dense:
        pre = norm(x)
    else:
        sites = mask[:, 0].nonzero(as_tuple=True)
        pre = torch.zeros((B, H, W, C), dtype=torch.float64).index_put(sites, norm(x.permute(0, 2, 3, 1)[sites])).permute(0, 3, 1, 2)
    if with_res:
        pre = pre + res
    y = torch.relu(pre) if dense else torch.relu(pre) * mask
    gy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    grads = torch.autograd.grad(y, (x, norm.weight, norm.bias) + ((res,) if with_res else ()), gy)
    r, rb = T.bn_statement(call, norm, True, gy)
    assert r["share"] <= T.GATE_CAP
    _close("y", r["y"], y.detach(), r["prea"] * r["m"] + 1e-300)
    _close("dx", rb["dx"], grads[0], rb["dxa"] + 1e-300)
    _close("dgamma", rb["dgamma"], grads[1], rb["dgamma_a"])
    _close("dbeta", rb["dbeta"], grads[2], rb["dbeta_a"])
    if with_res:
        assert torch.equal(rb["g"], grads[3])
    rm1, rv1 = T.running_update(norm, r["mean"], r["var"], r["cnt"], call["rm"], call["rv"])
    torch.testing.assert_close(norm.running_mean, rm1, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(norm.running_var, rv1, rtol=1e-12, atol=1e-14)
    # the widened bars vanish without an ambiguous gate and grow with one
    assert float(rb["dx_x"].abs().max()) == 0.0 or bool(r["amb"].any())


# ---------------------------------------------------------------------------------------------------- the harness on the plain fp32 modules
@pytest.fixture(scope="module")
def base():
    model = T.build_model(seed=31, bn_seed=32, pc_range=SMALL_RANGE)
    gen = torch.Generator().manual_seed(33)
    occ = (torch.rand((2, 1, 24, 40), generator=gen) < 0.25).float()
    occ[1] = 0
    canvas = torch.randn((2, 64, 24, 40), generator=gen).abs() * occ
    hg = {(ti, k): torch.randn((2, task.heads[k][0], 6, 10), generator=gen) for ti, task in enumerate(model.head.tasks) for k in task.heads}
    return model, canvas, occ, hg


def _run(base, mp, prepare=None, verbose=False):
    model, canvas, occ, hg = base
    model = copy.deepcopy(model)
    canvas = canvas.clone().requires_grad_(True)
    if prepare is not None:
        prepare(model, mp)
    rec = T.Recorder(model).install(mp)
    try:
        T.run_dense_chain(model, canvas, occ, hg)
    finally:
        rec.remove()
    mode = T.Mode("cpu")
    ck = T.Checker(mode)
    ck.verbose = verbose
    rec.after_backward(ck)
    first_dx = T.check_graph(ck, model, rec, mode, canvas.detach(), occ)
    ck.need(first_dx is not None and T.biteq(canvas.grad, first_dx), "canvas", "its gradient is not what the first backbone node returned")
    return ck, rec, model


def test_harness_passes_on_the_plain_module_graph(base, monkeypatch):
    ck, rec, model = _run(base, monkeypatch, verbose=True)
    ck.done("cpu")
    kinds = {}
    for (name, helper), n in rec.nodes.items():
        kinds[helper] = kinds.get(helper, 0) + 1
        assert len(n.calls) == (2 if name.startswith("neck.") else 1), (name, helper)
    # 20 backbone convolutions, 21 masked + 18 dense BatchNorm nodes, pre_conv 2 + post_conv 1 + deblock 2 + 12 first convolutions, 12 output convolutions,
    # the four module-hooked layers and the ASPP's four F.conv2d branches
    assert kinds == {"masked_conv": 20, "masked_bn_act": 21, "dense_bn_act": 18, "x3_conv": 17, "smallk_conv": 12, "module": 4,
                     "conv_d1": 1, "conv_d6": 1, "conv_d12": 1, "conv_d18": 1}, kinds
    nb = model.neck.post_conv.norm
    assert int(nb.num_batches_tracked) == 2 and int(model.head.shared_conv[1].num_batches_tracked) == 1


def test_ambiguous_gates_stay_under_the_cap_at_the_gpu_geometry(monkeypatch):
    """the fp64 plain-module graph at 136 x 208, B = 3 with the middle sample empty, the GPU test's clouds' occupancy and initialisation (forward only):
    per BatchNorm node, (site, channel) pairs with |pre| <= 2^-12 prea are <= 2^-9 of the active pairs"""
    model = T.build_model().double()
    occ = T.cloud_occupancy(T.cloud_points()).double()
    assert float(occ[1].sum()) == 0 and float(occ[0].sum()) > 1000 and float(occ[2].sum()) > 1000
    gen = torch.Generator().manual_seed(5)
    canvas = torch.randn((T.B, 64, T.NY, T.NX), generator=gen, dtype=torch.float64).abs() * occ
    rec = T.Recorder(model).install(monkeypatch)
    try:
        with torch.no_grad():
            T.run_dense_chain(model, canvas, occ)
    finally:
        rec.remove()
    worst, n = 0.0, 0
    for (name, helper), node in rec.nodes.items():
        if node.kind != "bn":
            continue
        r, _ = T.bn_statement(node.calls[0], model.get_submodule(name), True, None)
        worst, n = max(worst, r["share"]), n + 1
        assert r["share"] <= 2.0 ** -9, (name, r["share"])
    assert n == 39
    print(f"largest ambiguous-gate share of the fp64 reference graph: {worst:.3e}")


# ---------------------------------------------------------------------------------------------------- seeded mistakes
def _bad_bn_backward(what):
    def prepare(model, mp):
        from pillarnext_amd import train_nodes as tn

        orig = tn._MaskedBNActFn.backward

        def backward(ctx, gy):
            out = list(orig(ctx, gy))
            if what == "residual before the gate" and out[4] is not None:
                out[4] = (gy.float() * ctx.saved_tensors[1]).to(out[4].dtype)
            if what == "dgamma / count":
                out[2] = out[2] / ctx.saved_tensors[7]
            return tuple(out)

        mp.setattr(tn._MaskedBNActFn, "backward", staticmethod(backward))
    return prepare


class _BadConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride, mask_out, what):
        ctx.save_for_backward(x, w, mask_out)
        ctx.stride, ctx.what = stride, what
        return F.conv2d(x, w, None, stride, 1)

    @staticmethod
    def backward(ctx, g):
        x, w, mask_out = ctx.saved_tensors
        dx = torch.nn.grad.conv2d_input(x.shape, w, g, stride=ctx.stride, padding=1)
        dw = torch.nn.grad.conv2d_weight(x, w.shape, g, stride=ctx.stride, padding=1)
        if ctx.what == "masks swapped":        # the OUTPUT's active set read with the input's indices
            wrong = torch.zeros_like(dx[:, :1])
            wrong[:, :, :mask_out.shape[2], :mask_out.shape[3]] = mask_out
            dx = dx * wrong
        else:
            dw = dw * (1 + 2.0 ** -10)
        return dx, dw, None, None, None


def _bad_conv(pick, what):
    def prepare(model, mp):
        from pillarnext_amd import models

        target, orig = pick(model), models.masked_conv

        def masked_conv(conv, x, mask_out, mask_in):
            if conv is target:
                return _BadConv.apply(x, conv.weight, conv.stride[0], mask_out, what)
            return orig(conv, x, mask_out, mask_in)

        mp.setattr(models, "masked_conv", masked_conv)
    return prepare


def _bad_block(what):
    def prepare(model, mp):
        from pillarnext_amd import models as M

        def forward(self, x, mask):
            out, _ = self.block1(x, mask)
            if what == "fork contribution dropped":
                return M.masked_bn_act(M.masked_conv(self.conv2, out, mask, mask), mask, self.norm2, residual=x.detach()), mask
            return M.masked_bn_act(M.masked_conv(self.conv2, x, mask, mask), mask, self.norm2, residual=x), mask      # the stage's previous buffer

        blk = model.backbone.blocks[1][2]
        mp.setattr(blk, "forward", types.MethodType(forward, blk), raising=False)
    return prepare


SEEDED = {
    "residual gradient taken before the gate": (_bad_bn_backward("residual before the gate"), "dresidual is not the gated upstream gradient"),
    "mask_in / mask_out swapped in a stride-2 dx": (_bad_conv(lambda m: m.backbone.blocks[1][0].conv, "masks swapped"), "backbone.blocks.1.0.conv dx"),
    "one block's dW scaled by 1 + 2^-10": (_bad_conv(lambda m: m.backbone.blocks[2][1].block1.conv, "dw scaled"), "backbone.blocks.2.1.block1.conv dw"),
    "dgamma divided by the count": (_bad_bn_backward("dgamma / count"), "dgamma"),
    "a fork contribution dropped": (_bad_block("fork contribution dropped"), "fork: a contribution is missing"),
    "a layer's input replaced by the stage's previous buffer": (_bad_block("previous buffer"), "input is not the recorded output of the node before it"),
}


@pytest.mark.parametrize("mistake", list(SEEDED))
def test_harness_flags_a_seeded_mistake(base, monkeypatch, mistake):
    prepare, expect = SEEDED[mistake]
    ck, _, _ = _run(base, monkeypatch, prepare)
    hits = [f for f in ck.fails if any(expect in str(part) for part in f)]
    print(mistake, "->", len(ck.fails), "failed checks, e.g.", ck.fails[:3])
    assert hits, (mistake, "was not flagged", ck.fails[:5])
