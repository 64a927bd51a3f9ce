"""GPU: the fused training node BatchNorm1d + residual + ReLU of SparseResNet3D -- the kernels pnx_sp3_bn_stats / _apply / _bwd_stats / _bwd_apply
(csrc/sparse3d_bn.h), sparse3d.SparseBNActFunction and SparseResNet3D.use_fused_norm -- against the fp64 statement of tests/sparse3d_bn_ref.py
ON THE OPERANDS THE KERNELS SAW.
  - the default did not change: with the option off, the fp32 module and the 16-bit training module give the same bits before, while and after
    another module has it on
  - the four kernels at C in {16, 18, 36, 72, 128, 144}, n in {2, 33, 500, workgroups x rows per pass + 7}, residual none / fp32 / bf16 rows /
    fp16 rows, ReLU on and off, inputs with |mean| ~ 30 std in every third channel.  Bars from the arithmetic (no contraction):
      stats, bwd_stats  each sum within h 2^-24 sum|terms|, h = the longest fp32 chain of the documented split (sparse3d_bn_ref.chain)
      apply             |out - ref| <= 3 2^-24 (|y scale| + |shift| + |res|); out_h bit-equal to ops.sp3_rows_h(out); gate agrees where decided
      bwd_apply         |dy - ref| <= 8 2^-24 |scale| (|g| + |mean_g| + (|y| + |mean|) invstd |mean_gx|) where the gate is decided (<= 1 % is
                        not); dresidual bit-equal to g
    running statistics at rtol 1e-6 of the fp64 values, num_batches_tracked + 1, bit-identical repeats, n = 0, n = 1
  - the whole small backbone: fp32 + fused norm against the fp64 statement at 2 x the error of the option-off module; bf16 / fp16 + fused norm
    against (a) fp64, (b) fp64 with the rounding node at every convolution and on the residual operand, bars 1.5 (output) and 2 (gradients);
    ops.sp3_rows_h runs for the input features and for dy only; SyncBatchNorm over two replayed ranks against the joint batch
  - the voxel18 detector: one training step with both options on."""
import copy
import functools
import os

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import sparse3d_bn_ref as BR  # noqa: E402
import sparse3d_half_train_ref as TR  # noqa: E402
from conftest import ROOT  # noqa: E402
from sync_replay import Replay  # noqa: E402
from test_gpu_sparse3d_grad import _geometry, _labels, _small_scene, _train_backbone  # noqa: E402

EPS32 = 2.0 ** -24
EPS, MOM = 1e-3, 0.01
HALF = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _module_run(bb, feats, coords, grid, B=3):
    bb.zero_grad(set_to_none=True)
    f = feats.clone().requires_grad_(True)
    out = bb(f, coords, grid, B)
    out.sum().backward()
    return [out.detach(), f.grad] + [p.grad.clone() for p in bb.parameters()] + [v.clone() for v in bb.state_dict().values()]


# ------------------------------------------------------------------------------------------------ 1. the default did not change
def test_default_paths_are_unchanged_by_the_option():
    """First in the file: the fp32 training module and the 16-bit training module (option off) before any module of this process has the option
    on, then again while another module runs with it and after this one had it switched on and off."""
    feats, coords, grid = _small_scene()

    def fresh(half):
        bb = _train_backbone([16, 32, 64, 128], seed=6)
        return bb.use_half_precision(torch.bfloat16, training=True) if half else bb

    start = {k: v.detach().clone() for k, v in fresh(False).state_dict().items()}

    def run(bb):
        bb.load_state_dict(start)
        return _module_run(bb, feats, coords, grid)

    b32, b16 = fresh(False), fresh(True)
    assert b32.fused_norm is False and b16.fused_norm is False
    before32, before16 = run(b32), run(b16)
    other32, other16 = fresh(False).use_fused_norm(), fresh(True).use_fused_norm()
    on32, on16 = run(other32), run(other16)
    assert not torch.equal(on32[0], before32[0]) and not torch.equal(on16[0], before16[0]), "the option changes nothing: the node is not reached"
    for bb, before in ((b32, before32), (b16, before16)):
        for a, b in zip(run(bb), before):
            assert torch.equal(a, b), "the default path changed while the option is on in another module"
        bb.use_fused_norm()
        for a, b in zip(run(bb), on32 if bb is b32 else on16):
            assert torch.equal(a, b), "the option is not the same computation in two modules"
        bb.use_fused_norm(False)
        for a, b in zip(run(bb), before):
            assert torch.equal(a, b), "the default path changed after the option was switched on and off"
    # eval mode with gradients: fixed statistics, torch's ops with or without the option
    e_off, e_on = fresh(False).eval(), fresh(False).eval().use_fused_norm()
    for a, b in zip(_module_run(e_on, feats, coords, grid), _module_run(e_off, feats, coords, grid)):
        assert torch.equal(a, b), "a norm in eval mode must keep torch's ops"


# ------------------------------------------------------------------------------------------------ 2. the kernels
CHANNELS = [16, 18, 36, 72, 128, 144]
ROWS = [2, 33, 500, "passes"]
WORST = {}


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


def _two_pass_rows(C):
    """The kernel's own workgroups x rows per pass + 7: every workgroup makes more than one pass and the last pass ends inside a tile."""
    from pillarnext_amd import ops

    blocks, rpp, _ = ops.sp3_bn_split((1 << 31) - 1, C)
    n = blocks * rpp + 7
    assert ops.sp3_bn_split(n, C) == (blocks, rpp, 2) and 7 < rpp
    return n


def _sum_check(tag, got, ref, mag, h):
    err = (got - ref).abs()
    worst = float((err / (mag + 1e-30)).max())
    _note(tag, worst)
    print(f"[{tag}] worst {worst:.3g} of sum|terms| (bar h 2^-24 = {h * EPS32:.3g}, h = {h})")
    assert bool((err <= h * EPS32 * mag + 1e-30).all()), f"{tag}: worst {worst:.3g} of sum|terms|, bar {h * EPS32:.3g}"


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("C", CHANNELS)
def test_kernels_against_fp64_statement(C, n):
    from pillarnext_amd import ops

    n = _two_pass_rows(C) if n == "passes" else n
    y, res, gout, gamma, beta, rm, rv = BR.inputs(n, C, 2, device="cuda")
    split = ops.sp3_bn_split(n, C)
    h = BR.chain(split)
    cp = (C + 7) // 8 * 8
    y64, g64 = y.double(), gout.double()
    tag = f"C {C} n {n}"
    # ---- stats: [sum d | sum d^2 | rows] around the running mean, and around 0
    for center in (rm, None):
        part = ops.sp3_bn_stats(y, center)
        assert tuple(part.shape) == (split[0], 2 * C + 1) and ops.sp3_bn_partials_bytes(n, C) >= part.numel() * 4
        s = ops.sp3_bn_reduce(part)
        d = y64 - (0 if center is None else center.double())
        assert float(s[2 * C]) == n
        _sum_check(f"stats {tag}", s[:C], d.sum(0), d.abs().sum(0), h)
        _sum_check(f"stats {tag}", s[C:2 * C], (d * d).sum(0), (d * d).sum(0), h)
        assert torch.equal(part, ops.sp3_bn_stats(y, center)), "stats differ between two runs"
    s = ops.sp3_bn_reduce(ops.sp3_bn_stats(y, rm))
    # ---- finalize: the running statistics as torch's training-mode BatchNorm1d moves them
    rm2, rv2, nbt = rm.clone(), rv.clone(), torch.tensor(4, device="cuda")
    mean, invstd, scale, shift, cnt = ops.sp3_bn_finalize(s, rm2, gamma, beta, EPS, MOM, rm2, rv2, nbt)
    _, cache = BR.forward(y64, gamma.double(), beta.double(), None, False, EPS)
    want_m, want_v = BR.running(rm.double(), rv.double(), cache["mean"], cache["var"], n, MOM)
    assert int(nbt) == 5 and float(cnt) == n
    for got, want, name in ((rm2, want_m, "running_mean"), (rv2, want_v, "running_var")):
        _note("running statistics", ((got.double() - want).abs() / (1e-6 * want.abs() + 1e-7)).max())
        assert torch.allclose(got.double(), want, rtol=1e-6, atol=1e-7), f"{tag}: {name}"
    # the batch mean: the sum's bar over n, plus its own rounding to fp32
    d = y64 - rm.double()
    assert bool(((mean.double() - cache["mean"]).abs() <= h * EPS32 * d.abs().mean(0) + EPS32 * cache["mean"].abs() + 1e-30).all()), f"{tag}: mean"
    sc, sh, mu, isd = scale.double(), shift.double(), mean.double(), invstd.double()
    xhat = (y64 - mu) * isd
    for kind in ("none", "fp32", "bf16", "fp16"):
        r_op = None if kind == "none" else (res if kind == "fp32" else ops.sp3_rows_h(res, HALF[kind]))
        r64 = None if r_op is None else r_op.double()[:, :C]
        for relu in (True, False):
            t2 = f"{tag} res {kind} relu {relu}"
            # ---- apply
            ref, z = BR.apply_ref(y64, sc, sh, r64, relu)
            bar = BR.apply_bar(y64, sc, sh, r64)
            decided = (z.abs() > bar) if relu else torch.ones_like(z, dtype=torch.bool)
            _note("undecided share", 1.0 - float(decided.double().mean()))
            assert float(decided.double().mean()) >= 0.99, f"{t2}: more than 1 % of the gates are undecided"
            outs = {}
            for hk in ([kind] if kind in HALF else [None, "bf16", "fp16"]):
                out, out_h = ops.sp3_bn_apply(y, r_op, scale, shift, relu, None if hk is None else HALF[hk])
                assert out.dtype == torch.float32 and out.shape == y.shape
                err = (out.double() - ref).abs()
                _note("apply", (err / (bar + 1e-30)).max())
                assert bool((err <= bar).all()), f"{t2}: out worst {float((err / (bar + 1e-30)).max()):.3g} of the bar"
                if relu:
                    assert torch.equal((out > 0)[decided], (z > 0)[decided]), f"{t2}: a decided gate differs"
                if hk is None:
                    assert out_h is None
                else:
                    want_h = ops.sp3_rows_h(out, HALF[hk])
                    assert out_h.dtype == HALF[hk] and tuple(out_h.shape) == (n, cp) and not bool(out_h[:, C:].any())
                    assert torch.equal(out_h.view(torch.int16), want_h.view(torch.int16)), f"{t2}: out_h is not sp3_rows_h(out, {hk})"
                outs[hk] = out
            first = next(iter(outs.values()))
            assert all(torch.equal(o, first) for o in outs.values()), "out depends on out_h"
            assert torch.equal(first, ops.sp3_bn_apply(y, r_op, scale, shift, relu, None)[0]), "out differs between two runs"
            # ---- bwd_stats: the gate is the forward's own (the same operations in the same order), which dresidual confirms bit for bit below
            gate = (first > 0) if relu else torch.ones_like(first, dtype=torch.bool)
            g = g64 * gate
            part = ops.sp3_bn_bwd_stats(gout, y, r_op, scale, shift, mean, invstd, relu)
            assert tuple(part.shape) == (split[0], 2 * C)
            sg = ops.sp3_bn_reduce(part)
            _sum_check(f"bwd_stats {tag}", sg[:C], g.sum(0), g.abs().sum(0), h)
            _sum_check(f"bwd_stats {tag}", sg[C:], (g * xhat).sum(0), (g * xhat).abs().sum(0), h)
            assert torch.equal(part, ops.sp3_bn_bwd_stats(gout, y, r_op, scale, shift, mean, invstd, relu)), "bwd_stats differ between two runs"
            dgamma, dbeta, mg, mgx = ops.sp3_bn_bwd_finalize(sg, None, cnt)
            assert torch.allclose(dbeta.double(), sg[:C], rtol=1e-6, atol=1e-30) and torch.allclose(dgamma.double(), sg[C:], rtol=1e-6, atol=1e-30)
            assert torch.allclose(mg.double(), sg[:C] / n, rtol=1e-6, atol=1e-30) and torch.allclose(mgx.double(), sg[C:] / n, rtol=1e-6, atol=1e-30)
            # ---- bwd_apply
            dy, dres = ops.sp3_bn_bwd_apply(gout, y, r_op, scale, shift, mean, invstd, relu, mg, mgx, want_residual_grad=True)
            assert torch.equal(dres, torch.where(gate, gout, torch.zeros_like(gout))), f"{t2}: dresidual is not g"
            gd = g64 * (z > 0) if relu else g64  # the statement's own gate, compared where it is decided
            ref_dy = BR.bwd_apply_ref(gd, y64, sc, mu, isd, mg.double(), mgx.double())
            bar_dy = BR.bwd_apply_bar(gd, y64, sc, mu, isd, mg.double(), mgx.double())
            err = (dy.double() - ref_dy).abs()
            _note("bwd_apply", (err / (bar_dy + 1e-30))[decided].max())
            assert bool((err <= bar_dy)[decided].all()), f"{t2}: dy worst {float((err / (bar_dy + 1e-30))[decided].max()):.3g} of the bar"
            dy2, none = ops.sp3_bn_bwd_apply(gout, y, r_op, scale, shift, mean, invstd, relu, mg, mgx)
            assert none is None and torch.equal(dy, dy2), "dy differs between two runs"
    print(f"[{tag}] worst so far: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


def test_wrappers_refuse_what_the_kernels_do_not_take():
    from pillarnext_amd import ops
    from pillarnext_amd._lib import PnxError

    y = torch.zeros((4, 18), device="cuda")
    v = torch.zeros((18,), device="cuda")
    with pytest.raises(PnxError, match="one dtype"):
        ops.sp3_bn_apply(y, torch.zeros((4, 24), dtype=torch.bfloat16, device="cuda"), v, v, True, torch.float16)
    with pytest.raises(PnxError, match="16-bit residual"):
        ops.sp3_bn_apply(y, torch.zeros((4, 18), dtype=torch.bfloat16, device="cuda"), v, v, True)
    with pytest.raises(PnxError, match="fp32 rows"):
        ops.sp3_bn_stats(torch.zeros((4, 300), device="cuda"), None)
    with pytest.raises(PnxError):
        ops.masked_bn_reduce(torch.zeros((4, 37), device="cuda"))  # the 2-D wrappers keep their channel counts


# ------------------------------------------------------------------------------------------------ 3. the node
def _node(y, gamma, beta, res, res_h, norm, relu, dtype):
    from pillarnext_amd.sparse3d import SparseBNActFunction

    return SparseBNActFunction.apply(y, gamma, beta, res, res_h, norm, relu, dtype)


def _norm_module(C, rm, rv, sync=None):
    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=MOM).cuda().train()
    with torch.no_grad():
        bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    return bn if sync is None else torch.nn.SyncBatchNorm.convert_sync_batchnorm(bn, sync)


def test_node_without_rows_and_with_one_row():
    C = 18
    y, res, gout, gamma, beta, rm, rv = BR.inputs(4, C, 3, device="cuda")
    bn = _norm_module(C, rm, rv)
    before = {k: v.clone() for k, v in bn.state_dict().items()}
    ga, be = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y0 = y[:0].clone().requires_grad_(True)
    out, out_h = _node(y0, ga, be, None, None, bn, True, torch.bfloat16)
    assert tuple(out.shape) == (0, C) and out.dtype == torch.float32 and tuple(out_h.shape) == (0, 24) and out_h.dtype == torch.bfloat16
    out.sum().backward()
    assert tuple(y0.grad.shape) == (0, C)
    for k, v in bn.state_dict().items():
        assert torch.equal(v, before[k]), f"an empty set moved {k}"
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        _node(y[:1].clone(), ga, be, None, None, bn, True, None)
    for k, v in bn.state_dict().items():
        assert torch.equal(v, before[k]), f"a refused call moved {k}"


@pytest.mark.parametrize("kind", ["none", "fp32", "bf16", "fp16"])
def test_node_against_fp64_statement(kind):
    """Autograd plumbing of one node: outputs, every gradient, the saved tensors, the non-differentiable out_h."""
    from pillarnext_amd import ops

    n, C = 333, 36
    y, res, gout, gamma, beta, rm, rv = BR.inputs(n, C, 4, device="cuda")
    dtype = HALF.get(kind)
    bn = _norm_module(C, rm, rv)
    leaves = [t.clone().requires_grad_(True) for t in (y, gamma, beta, res)]
    r = None if kind == "none" else leaves[3]
    r_h = ops.sp3_rows_h(res, dtype) if dtype is not None else None
    out, out_h = _node(leaves[0], leaves[1], leaves[2], r, r_h, bn, True, dtype)
    assert out.requires_grad and (out_h is None) == (dtype is None) and (out_h is None or not out_h.requires_grad)
    saved = [tuple(t.shape) for t in out.grad_fn.saved_tensors if t is not None and t.dim() == 2]
    assert sorted(saved) == sorted([(n, C)] + ([] if kind == "none" else [tuple((r_h if r_h is not None else res).shape)])), "the node keeps y and the residual only"
    out.backward(gout)
    want, cache = BR.forward(y.double(), gamma.double(), beta.double(), None if kind == "none" else res.double(), True, EPS, dtype)
    dy, dgamma, dbeta, dres = BR.backward(gout.double(), cache)
    decided = cache["z"].abs() > 1e-4
    assert torch.allclose(out.double(), want, rtol=1e-5, atol=1e-5)
    assert torch.allclose(leaves[0].grad.double()[decided], dy[decided], rtol=1e-4, atol=1e-5)
    assert torch.allclose(leaves[1].grad.double(), dgamma, rtol=1e-4, atol=1e-4) and torch.allclose(leaves[2].grad.double(), dbeta, rtol=1e-4, atol=1e-4)
    if kind == "none":
        assert leaves[3].grad is None
    else:
        assert torch.equal(leaves[3].grad, torch.where(out > 0, gout, torch.zeros_like(gout))), "dresidual = g, straight through the rounding"
    want_m, want_v = BR.running(rm.double(), rv.double(), cache["mean"], cache["var"], n, MOM)
    assert torch.allclose(bn.running_mean.double(), want_m, rtol=1e-6, atol=1e-7) and torch.allclose(bn.running_var.double(), want_v, rtol=1e-6, atol=1e-7)
    assert int(bn.num_batches_tracked) == 1


def test_synchronised_node_with_a_rank_without_rows():
    """Two replayed ranks, the second without a row: both issue the forward and the backward collective, and rank 0 computes what it computes alone."""
    n, C = 77, 18
    y, res, gout, gamma, beta, rm, rv = BR.inputs(n, C, 5, device="cuda")

    def run(rows, norm):
        leaves = [t.clone().requires_grad_(True) for t in (y[:rows], gamma, beta)]
        out, _ = _node(leaves[0], leaves[1], leaves[2], None, None, norm, True, None)
        out.backward(gout[:rows])
        return [out.detach()] + [t.grad for t in leaves] + [norm.running_mean.clone(), norm.running_var.clone()]

    alone = run(n, _norm_module(C, rm, rv))
    rp = Replay(2)
    got = rp.run(lambda rank, token: run(n if rank == 0 else 0, _norm_module(C, rm + rank, rv, sync=token)))
    assert rp.passes == 3, "one collective forward, one backward"
    for a, b in zip(got[0], alone):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)
    assert tuple(got[1][0].shape) == (0, C) and not bool(got[1][2].any()) and not bool(got[1][3].any())  # no rows: zero parameter gradients
    want = 0.99 * (rm.double() + 1) + 0.01 * y.double().mean(0)  # its own running mean moved by the global batch mean
    assert torch.allclose(got[1][4].double(), want, rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------------------------------------------ 4. the whole small backbone
def _statement(bb, params, feats, coords, grid, B, dtype):
    """SparseResNet3D.forward in training mode in fp64 under autograd.  dtype None: plain; bf16 / fp16: every convolution through TR.RoundedConv and
    the residual operand through the rounding with a straight-through gradient (sparse3d_bn_ref.bn_act)."""
    def conv(x, name, coords, grid, mod, subm):
        oc, og, pairs = _geometry(coords, grid, mod, subm)
        return oc, TR.RoundedConv.apply(x, params[name + ".weight"], pairs, oc.shape[0], dtype), og

    def bn(x, name, res=None):
        return BR.bn_act(x, params[name + ".weight"], params[name + ".bias"], res, True, EPS, dtype)

    x = feats
    for i, seq in enumerate(bb.blocks):
        coords, x, grid = conv(x, f"blocks.{i}.0.conv", coords, grid, seq[0].conv, False)
        x = bn(x, f"blocks.{i}.0.norm")
        for j, blk in enumerate(seq[1:], 1):
            y = bn(conv(x, f"blocks.{i}.{j}.block1.conv", coords, grid, blk.block1.conv, True)[1], f"blocks.{i}.{j}.block1.norm")
            x = bn(conv(y, f"blocks.{i}.{j}.conv2", coords, grid, blk.conv2, True)[1], f"blocks.{i}.{j}.norm2", x)
    coords, x, grid = conv(x, "extra_conv.0", coords, grid, bb.extra_conv[0], False)
    x = bn(x, "extra_conv.1")
    x = bn(conv(x, "mapping.conv", coords, grid, bb.mapping.conv, True)[1], "mapping.norm")
    D, H, W = grid
    c = coords.long()
    dense = torch.zeros((B, D, H, W, x.shape[1]), dtype=x.dtype, device=x.device).index_put((c[:, 0], c[:, 1], c[:, 2], c[:, 3]), x)
    return dense.permute(0, 4, 1, 2, 3).reshape(B, -1, H, W)


def _norm(t):
    return float(torch.linalg.vector_norm(t.double()))


def _proj(B=3):
    return torch.randn((B, 256, 3, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))


@functools.lru_cache(maxsize=None)
def _fp64(dtype):
    """(dense output, gradients) of the fp64 statement from _train_backbone(seed 3)'s start; computed once per rounding, never changed."""
    bb = _train_backbone([16, 32, 64, 128], seed=3)
    feats, coords, grid = _small_scene()
    params = {k: v.detach().double().clone().requires_grad_(True) for k, v in bb.named_parameters()}
    f = feats.detach().double().clone().requires_grad_(True)
    dense = _statement(bb, params, f, coords, grid, 3, dtype)
    (dense * _proj().double()).sum().backward()
    return dense.detach(), {**{k: p.grad for k, p in params.items()}, "input features": f.grad}


def _module(bb, feats, coords, grid, B, proj):
    bb.zero_grad(set_to_none=True)
    f = feats.detach().clone().requires_grad_(True)
    out = bb(f, coords, grid, B)
    assert out.dtype == torch.float32
    (out * proj).sum().backward()
    return out.detach(), {**{k: p.grad for k, p in bb.named_parameters()}, "input features": f.grad}


@functools.lru_cache(maxsize=None)
def _option_off():
    """The fp32 module with the option off (the path before this option), from the same start."""
    feats, coords, grid = _small_scene()
    return _module(_train_backbone([16, 32, 64, 128], seed=3), feats, coords, grid, 3, _proj())


def _ratios(tag, got, ref_a, ref_b, bars):
    """rows of (name, |c - a|, |b - a|, bar); asserts |c - a| <= bar |b - a| for each."""
    (out_c, g_c), (out_a, g_a), (out_b, g_b) = got, ref_a, ref_b
    rows = [("dense output", _norm(out_c.double() - out_a), _norm(out_b.double() - out_a), bars[0])]
    for k, r in g_a.items():
        assert g_c[k] is not None and g_c[k].dtype == torch.float32 and bool(torch.isfinite(g_c[k]).all()), k
        rows.append((k, _norm(g_c[k].double() - r), _norm(g_b[k].double() - r), bars[1]))
    worst = [0.0, 0.0]
    for i, (k, e_c, e_b, bar) in enumerate(rows):
        print(f"[{tag}] {k:34s} |c - a| {e_c:.3g}  |b - a| {e_b:.3g}  ratio {e_c / max(e_b, 1e-300):.3f} (bar {bar})")
        worst[min(i, 1)] = max(worst[min(i, 1)], e_c / max(e_b, 1e-300))
    print(f"[{tag}] worst ratio: output {worst[0]:.3f} (bar {bars[0]}), gradients {worst[1]:.3f} (bar {bars[1]})")
    for k, e_c, e_b, bar in rows:
        assert e_c <= bar * e_b, f"{k}: |c - a| {e_c:.3g} > {bar} x |b - a| {e_b:.3g}"


def _moved_once(bb, start):
    for name, m in bb.named_modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            assert int(m.num_batches_tracked) == int(start[name + ".num_batches_tracked"]) + 1
            assert not torch.equal(m.running_mean, start[name + ".running_mean"]) and not torch.equal(m.running_var, start[name + ".running_var"]), name


def test_whole_graph_fp32_with_fused_norm():
    """(a) the fp64 statement, (b) the module with the option off, (c) the module with the option on: |c - a| <= 2 |b - a| for the dense output
    and every gradient -- both are fp32 roundings of the same expressions in another order."""
    bb = _train_backbone([16, 32, 64, 128], seed=3).use_fused_norm()
    feats, coords, grid = _small_scene()
    start = {k: v.detach().clone() for k, v in bb.state_dict().items()}
    got = _module(bb, feats, coords, grid, 3, _proj())
    _ratios("whole graph fp32 + fused norm", got, _fp64(None), _option_off(), (2.0, 2.0))
    _moved_once(bb, start)
    off = _train_backbone([16, 32, 64, 128], seed=3)
    _module(off, feats, coords, grid, 3, _proj())
    for k, v in bb.state_dict().items():  # the running statistics are the ones torch's BatchNorm1d keeps
        assert torch.allclose(v.double(), off.state_dict()[k].double(), rtol=1e-5, atol=1e-6), k


@pytest.mark.parametrize("name", list(HALF))
def test_whole_graph_half_with_fused_norm(name, monkeypatch):
    """(a) fp64, (b) fp64 with the rounding node at every convolution and on the residual operand, (c) the module with both options on."""
    from pillarnext_amd import ops

    dtype = HALF[name]
    bb = _train_backbone([16, 32, 64, 128], seed=3).use_half_precision(dtype, training=True).use_fused_norm()
    feats, coords, grid = _small_scene()
    start = {k: v.detach().clone() for k, v in bb.state_dict().items()}
    calls, real = [], ops.sp3_rows_h

    def counting(x, dt):
        calls.append(tuple(x.shape))
        return real(x, dt)

    monkeypatch.setattr(ops, "sp3_rows_h", counting)
    f = feats.detach().clone().requires_grad_(True)
    out = bb(f, coords, grid, 3)
    assert calls == [tuple(feats.shape)], f"sp3_rows_h between layers: {calls}"  # the input features only
    (out * _proj()).sum().backward()
    assert len(calls) == 1 + 22, "sp3_rows_h runs once per layer in the backward, for dy"
    monkeypatch.undo()
    got = (out.detach(), {**{k: p.grad for k, p in bb.named_parameters()}, "input features": f.grad})
    _ratios(f"whole graph {name} + fused norm", got, _fp64(None), _fp64(dtype), (1.5, 2.0))
    _moved_once(bb, start)
    first = {k: v.clone() for k, v in got[1].items()}
    bb.load_state_dict(start)
    out2, again = _module(bb, feats, coords, grid, 3, _proj())
    assert torch.equal(out2, got[0])
    for k in first:
        assert torch.equal(first[k], again[k]), f"{k}: gradient differs between two runs"


def test_whole_graph_synchronised_over_two_ranks():
    """The scene's two occupied frames on two replayed ranks, every norm a SyncBatchNorm that carries the rank's token: outputs, dL/dx and the
    parameter gradients summed over the ranks against the fp64 statement of the joint batch, at the single-rank bar."""
    feats, coords, grid = _small_scene()
    proj = _proj()
    frames = [0, 2]
    base = _train_backbone([16, 32, 64, 128], seed=3).use_fused_norm()

    def rank_run(rank, token):
        bb = torch.nn.SyncBatchNorm.convert_sync_batchnorm(copy.deepcopy(base), token)
        assert all(m.process_group is token for m in bb.modules() if isinstance(m, torch.nn.SyncBatchNorm)) and bb.fused_norm
        sel = coords[:, 0] == frames[rank]
        c = coords[sel].clone()
        c[:, 0] = 0
        out, g = _module(bb, feats[sel], c, grid, 1, proj[frames[rank]:frames[rank] + 1])
        return out, {k: v.clone() for k, v in g.items()}, {k: v.clone() for k, v in bb.state_dict().items()}

    rp = Replay(2)
    res = rp.run(rank_run, max_passes=64)
    assert rp.passes == 2 * 22 + 1, "one collective per norm layer forward, one backward, on both ranks"
    out = torch.zeros((3, 256, 3, 3), device="cuda")
    gin = torch.zeros_like(feats)
    for rank, (o, g, _) in enumerate(res):
        out[frames[rank]] = o[0]
        gin[coords[:, 0] == frames[rank]] = g["input features"]
    grads = {k: res[0][1][k] + res[1][1][k] for k in res[0][1] if k != "input features"}  # the loss is a sum over the frames
    grads["input features"] = gin
    _ratios("two synchronised ranks", (out, grads), _fp64(None), _option_off(), (2.0, 2.0))
    off = _train_backbone([16, 32, 64, 128], seed=3)
    _module(off, feats, coords, grid, 3, proj)
    for k, v in res[0][2].items():  # every rank keeps the joint batch's running statistics
        assert torch.allclose(v.double(), off.state_dict()[k].double(), rtol=1e-5, atol=1e-6), k
        assert torch.equal(v, res[1][2][k]), f"the ranks' {k} differ"


# ------------------------------------------------------------------------------------------------ 5. detector: a training step
def test_voxel18_nusc_detector_training_step_fused_norm():
    from pillarnext_amd import config, synth

    cfg = config.load(os.path.join(ROOT, "configs", "voxel18_aspp_nusc.yaml"))
    torch.manual_seed(0)
    det = config.instantiate(cfg["model"]).cuda().train()
    assert det.backbone.use_half_precision(torch.bfloat16, training=True).use_fused_norm() is det.backbone
    B, M = 2, 16
    H = W = 1344 // cfg["_out_size_factor"][0]
    pts = torch.from_numpy(synth.make_batch("C2ref", B, "sweep", n=60_000)).cuda()
    ex = {"points": pts, "batch_size": B, **_labels([list(t) for t in cfg["_tasks"]], B, M, H, W)}
    opt = torch.optim.SGD(det.parameters(), lr=1e-3)
    loss, _ = det(ex)
    assert bool(torch.isfinite(loss))
    opt.zero_grad()
    loss.backward()
    for k, p in det.backbone.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), f"backbone.{k}"
    opt.step()
    loss2, _ = det(ex)
    print(f"[voxel18 training step bf16 + fused norm] loss {float(loss):.6f} -> {float(loss2):.6f}")
    assert bool(torch.isfinite(loss2)) and float(loss2) < float(loss)
