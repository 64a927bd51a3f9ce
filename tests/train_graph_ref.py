"""The 2-D TRAINING graph held to fp64 node by node, with teacher forcing: a recorder that keeps what every node of the real graph received and
produced, forward and backward; one plain fp64 statement per node kind, run on exactly those recorded operands; and the checks (wiring, forks,
values) that tests/test_gpu_train_graph_vs_fp64.py runs on the HIP graph and tests/test_train_graph_ref_cpu.py on the plain modules on the CPU.
No error is carried from node to node, so the per-element bars of tests/test_gpu_train_kernels_at_scale.py apply unchanged to every node of the
COMPOSED graph, and a wiring mistake is an O(1) error at the sites it touches.

Recorder (no kernel knowledge).  models.py binds its routing helpers by name (masked_conv, masked_bn_act, dense_bn_act, x3_conv, smallk_conv,
dense_conv3x3, split_f32_pieces): those names are replaced, in pillarnext_amd.models only, by wrappers that call the original and record detached
clones of every tensor input (x, residual, masks, weight, bias, gamma, beta, the running statistics BEFORE the call) and of the output, the
output's grad_fn type and the owning module's qualified name (identity of conv / norm against model.named_modules()).  The layers that run outside
the helpers (the 1x1 mapping convolution, conv1x1, shared_conv[0], BasicBlock's add + ReLU: module hooks; the ASPP's F.conv2d calls: a proxy for
the name `F` of models.py) are recorded the same way, so the chain "output of k = input of k + 1" has no hole.
Backward: every differentiable input goes through an identity view (same shape, strides and storage) in front of the node, with a tensor hook on
the view: what the hook sees is the gradient THIS node returned for that input, not the sum over a fork.  Parameters get the same treatment (the
view replaces the module's parameter for the duration of the call).  A hook on the output records the upstream gradient.
The checkpointed neck runs its nodes a second time during the backward: records are keyed by (module name, helper); on the second call of a key
the inputs and the output must equal the first call's bit for bit, and the running statistics before the second call are kept as well.  Any other
repeated key is an error.  The backward flows through the graph the first call built, so the first call's hooks fire.

Statements.  Masked / dense 3x3 convolutions and the SepHead output convolution: _conv_refs of the at-scale module (gathered fp64 sums at the
active sites, each with its sum|terms|); BatchNorm + residual + ReLU + mask: _bn_ref / _bn_ref_backward of the same module (BatchNorm1d over the
gathered active sites, as sparse_conv.py applies it; every site for the dense layers); the library layers: the tap-by-tap fp64 convolution of
tests/fused_graph_ref.py (written from the modules' definition) and its fp64 gradients.  Operands: the bf16 graph's nodes multiply bf16 maps and
bf16-rounded weights, so those ARE the reference operands; the fp32 graphs' references take the fp32 operands.

A BatchNorm node inside the checkpointed region ran its forward twice, so its running statistics are held to TWO updates, the second from the
recorded "before" of the second call, and num_batches_tracked to + 2.  That is the reference's behaviour too: det3d/models/necks/aspp.py
checkpoints the same region around nn.BatchNorm2d.

ReLU gates within rounding of zero.  The isolated tests zero the upstream gradient where |pre| <= 2^-12 prea; inside a composed graph that is
impossible, so the bars absorb it (bn_statement, bn_node_values): dx at an ambiguous (site, channel) gets |gamma invstd| |g| on its bar, dgamma sum_amb |g| xa, dbeta
sum_amb |g|, every dx of that channel |gamma invstd| (dmg + xa dmgx); dresidual equals the gated upstream gradient exactly elsewhere and is g or 0
at an ambiguous pair.  Condition, per node: ambiguous pairs <= GATE_CAP = 2^-8 of the active pairs (expected ~2 * 2^-12 * prea * pdf(0) ~ 2^-11
with pre ~ unit normal and prea of 1..3; the cap leaves ~8x headroom and keeps the widened sums negligible)."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as TF
import torch.utils.checkpoint

import fused_graph_ref as R
from test_gpu_infer_kernels_at_scale import FRO_MARGIN  # noqa: F401  (the at-scale modules' bars, unchanged)
from test_gpu_train_kernels_at_scale import (BF_OUT, BF_REL, BN_REL, TINY, X3_FRO, X3_REL, X6_FRO, X6_REL, _bn_ref, _bn_ref_backward, _conv_refs,
                                             _gather)

GATE_CAP = 2.0 ** -8
GATE_REL = 2.0 ** -12
HALF_ULP = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float64: 2.0 ** -53}
HELPERS = ("masked_conv", "masked_bn_act", "dense_bn_act", "x3_conv", "smallk_conv", "dense_conv3x3", "split_f32_pieces")
CL = torch.channels_last


# ---------------------------------------------------------------------------------------------------- bits
def biteq(a, b):
    if a is None or b is None or a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {4: torch.int32, 2: torch.int16, 8: torch.int64}.get(a.element_size()) if a.is_floating_point() else None
    a, b = a.contiguous(), b.contiguous()
    return torch.equal(a, b) if it is None else torch.equal(a.view(it), b.view(it))


def zero_bits(t, strict=True):
    """every element +0.0 (strict=False: -0.0 too, what a torch statement's `* mask` leaves)"""
    return int(torch.count_nonzero(t)) == 0 and not (strict and bool(torch.signbit(t).any()))


# ---------------------------------------------------------------------------------------------------- modes
class Mode:
    """what a parametrisation expects of its nodes: bars (the at-scale modules', unchanged), operand rounding, grad_fn types"""

    def __init__(self, name):
        self.name, self.hip = name, name != "cpu"
        self.amp = name == "bf16"
        if name == "bf16":
            self.conv, self.lib = (BF_REL, None, BF_OUT), (BF_REL, BF_OUT)
        elif name == "x3":
            self.conv, self.lib = (X3_REL, X3_FRO, 0.0), (X3_REL, 0.0)
        elif name == "x6":
            self.conv, self.lib = (X6_REL, X6_FRO, 0.0), (X3_REL, 0.0)
        else:   # the plain fp32 modules on the CPU: 2^-20 of sum|terms| per convolution node
            self.conv, self.lib = (2.0 ** -20, None, 0.0), (2.0 ** -20, 0.0)
        self.smallk = (BF_REL, None, BF_OUT if self.amp else 0.0) if self.hip else self.conv
        self.bn_ulp = BF_OUT if self.amp else 0.0
        self.conv_fn = {"bf16": "_MaskedConv3x3FnBackward", "x3": "_MaskedConv3x3F32FnBackward", "x6": "_MaskedConv3x3F32FnBackward"}.get(name)

    def op(self, t):
        """the operand the node's kernel multiplies"""
        return t.to(torch.bfloat16) if self.amp else t


# ---------------------------------------------------------------------------------------------------- the recorder
class Node:
    def __init__(self, key, kind):
        self.key, self.kind, self.calls, self.grads, self.expect, self.gfn, self.extra = key, kind, [], {}, [], None, {}

    def __getattr__(self, name):            # first call's tensors: n.x, n.out, ...
        calls = self.__dict__.get("calls")
        if calls and name in calls[0]:
            return calls[0][name]
        raise AttributeError(name)

    def grad(self, name):
        g = self.grads.get(name)
        return None if not g else g[0]


def _c(t):
    return None if t is None else t.detach().clone()


class Recorder:
    """install(mp) patches pillarnext_amd.models through a pytest MonkeyPatch (undone with it); hooks are removed by remove()."""

    def __init__(self, model, twice=("neck.",)):
        self.model, self.nodes, self.twice, self.handles, self.splits, self.errors = model, {}, tuple(twice), [], [], []
        self.names = {id(m): n for n, m in model.named_modules()}
        self.canvas = self.occ = None
        self.canvas_grad = []

    # ---- one call of one node
    def _tap(self, node, name, t, first):
        v = t.view_as(t)
        same_strides = all(a == b for a, b, n in zip(v.stride(), t.stride(), t.shape) if n > 1)       # the stride of a size-1 dimension addresses nothing
        assert v.shape == t.shape and same_strides and v.data_ptr() == t.data_ptr(), (node.key, name, "the identity view moved the tensor")
        if t.dim() == 4 and t.is_contiguous(memory_format=CL):
            assert v.is_contiguous(memory_format=CL), (node.key, name, "the identity view lost channels_last")
        if first and v.requires_grad:
            node.expect.append(name)
            v.register_hook(lambda g, n=name: node.grads.setdefault(n, []).append(g.detach().clone()))
        return v

    @contextlib.contextmanager
    def call(self, key, kind, tensors, diff=(), module=None, params=(), buffers=()):
        """tensors: name -> tensor or None (cloned); diff: the names among them that get an identity view + hook; params: (record name, attribute) of
        `module` swapped for a view during the call; buffers: (record name, attribute) cloned before the call.  Yields (node, views, finish)."""
        node = self.nodes.get(key)
        first = node is None
        if first:
            node = self.nodes[key] = Node(key, kind)
        elif not (key[0].startswith(self.twice) and len(node.calls) == 1):
            self.errors.append((key, "called again outside the checkpointed region", len(node.calls) + 1))
        rec = {k: _c(t) for k, t in tensors.items()}
        views = {k: (self._tap(node, k, tensors[k], first) if tensors[k] is not None else None) for k in diff}
        saved = {}
        for rname, attr in params:
            p = module._parameters.get(attr)
            if p is None:
                rec[rname] = None
                continue
            rec[rname] = _c(p)
            saved[attr] = p
            module._parameters[attr] = self._tap(node, rname, p, first)
            node.extra.setdefault("params", {})[rname] = p
        for rname, attr in buffers:
            rec[rname] = _c(getattr(module, attr))

        def finish(out):
            rec["out"] = _c(out)
            if first:
                node.gfn = type(out.grad_fn).__name__ if out.grad_fn is not None else None
                if out.requires_grad:
                    node.expect.append("out")
                    out.register_hook(lambda g: node.grads.setdefault("out", []).append(g.detach().clone()))
            else:
                a = node.calls[0]
                for k in rec:
                    if k in ("rm", "rv", "nbt"):
                        continue
                    if not (rec[k] is None and a.get(k) is None) and not biteq(rec[k], a.get(k)):
                        self.errors.append((key, k, "the recomputation differs from the first call"))
            node.calls.append(rec)
            return out

        try:
            yield node, views, finish
        finally:
            for attr, p in saved.items():
                module._parameters[attr] = p
            if "out" not in rec and first and key in self.nodes and not node.calls:
                del self.nodes[key]

    def name(self, module):
        return self.names[id(module)]

    # ---- the helpers of models.py
    def install(self, mp):
        from pillarnext_amd import models

        o = {h: getattr(models, h) for h in HELPERS}
        rec = self
        conv_p, bn_p, bn_b = (("w", "weight"), ("b", "bias")), (("gamma", "weight"), ("beta", "bias")), (("rm", "running_mean"), ("rv", "running_var"), ("nbt", "num_batches_tracked"))

        def masked_conv(conv, x, mask_out, mask_in):
            with rec.call((rec.name(conv), "masked_conv"), "conv", dict(x=x, mask_out=mask_out, mask_in=mask_in), ("x",), conv, conv_p) as (n, v, fin):
                return fin(o["masked_conv"](conv, v["x"], mask_out, mask_in))

        def masked_bn_act(x, mask, norm, residual=None, relu=True):
            with rec.call((rec.name(norm), "masked_bn_act"), "bn", dict(x=x, mask=mask, residual=residual), ("x", "residual"), norm, bn_p, bn_b) as (n, v, fin):
                n.extra["relu"] = relu
                return fin(o["masked_bn_act"](v["x"], mask, norm, residual=v["residual"], relu=relu))

        def dense_bn_act(norm, x, relu=True):
            with rec.call((rec.name(norm), "dense_bn_act"), "bn", dict(x=x, mask=None, residual=None), ("x",), norm, bn_p, bn_b) as (n, v, fin):
                n.extra["relu"] = relu
                return fin(o["dense_bn_act"](norm, v["x"], relu=relu))

        def x3_conv(conv, x, pieces=None):
            with rec.call((rec.name(conv), "x3_conv"), "conv", dict(x=x), ("x",), conv, conv_p) as (n, v, fin):
                if pieces is not None:
                    n.extra["pieces"] = (pieces, [_c(p) for p in pieces])
                return fin(o["x3_conv"](conv, v["x"], pieces))

        def smallk_conv(conv, x):
            with rec.call((rec.name(conv), "smallk_conv"), "conv", dict(x=x), ("x",), conv, conv_p) as (n, v, fin):
                return fin(o["smallk_conv"](conv, v["x"]))

        def dense_conv3x3(x, weight, bias=None, pieces=None, **kw):
            with rec.call(("neck.weight", "conv_d1"), "conv", dict(x=x, w=weight, b=bias), ("x", "w", "b")) as (n, v, fin):
                y = o["dense_conv3x3"](v["x"], v["w"], v["b"], pieces, **kw)
                return y if y is None else fin(y)      # None: the caller's own convolution runs (and is recorded there)

        def split_f32_pieces(x, mask=None, pieces=None):
            out = o["split_f32_pieces"](x, mask, pieces)
            rec.splits.append((_c(x), out, [_c(p) for p in out]))
            return out

        for h, f in (("masked_conv", masked_conv), ("masked_bn_act", masked_bn_act), ("dense_bn_act", dense_bn_act), ("x3_conv", x3_conv),
                     ("smallk_conv", smallk_conv), ("dense_conv3x3", dense_conv3x3), ("split_f32_pieces", split_f32_pieces)):
            mp.setattr(models, h, f)

        class _F:       # models.py's `F`: conv2d (the ASPP's dilated branches) recorded, every other name torch's own
            def __getattr__(self, name):
                return getattr(TF, name)

            @staticmethod
            def conv2d(x, w, bias=None, stride=1, padding=0, dilation=1, groups=1):
                assert bias is None and stride == 1 and groups == 1 and padding == dilation, "only the ASPP's branches call F.conv2d in models.py"
                with rec.call(("neck.weight", f"conv_d{dilation}"), "conv", dict(x=x, w=w, b=None), ("x", "w")) as (n, v, fin):
                    return fin(TF.conv2d(v["x"], v["w"], None, 1, padding, dilation))

        mp.setattr(models, "F", _F())
        m = self.model
        for mod, kind, params in ((m.backbone.mapping[0], "conv", conv_p), (m.neck.conv1x1, "conv", conv_p), (m.head.shared_conv[0], "conv", conv_p),
                                  (m.neck.pre_conv.act, "act", ())):
            self._hook_module(mod, kind, params)
        if not next(m.parameters()).is_cuda:
            # SepHead.forward leaves its branches to their nn.Sequential off the GPU: the same records, under the keys the helpers would have used
            for task in m.head.tasks:
                for h in task.heads:
                    fc = getattr(task, h)
                    self._hook_module(fc[0], "conv", conv_p, "x3_conv")
                    self._hook_module(fc[1], "bn", bn_p, "dense_bn_act", bn_b, end=fc[2], extra=dict(mask=None, residual=None))
                    self._hook_module(fc[3], "conv", conv_p, "smallk_conv")
        if hasattr(m.reader, "forward_dense"):
            inner = m.reader.forward_dense

            def forward_dense(points, batch_size, **kw):
                x = inner(points, batch_size, **kw)
                rec.canvas, rec.occ = _c(x), _c(kw["occupancy"])
                if x.requires_grad:
                    x.register_hook(lambda g: rec.canvas_grad.append(g.detach().clone()))
                return x

            mp.setattr(m.reader, "forward_dense", forward_dense, raising=False)
        return self

    def _hook_module(self, mod, kind, params, helper="module", buffers=(), end=None, extra=None):
        """record a layer that runs outside the helpers: a forward_pre_hook on `mod` opens the call (identity view of the input, parameter views), a forward
        hook on `end` (default: mod itself; the ReLU behind a BatchNorm for a BN + ReLU pair) closes it"""
        key, stack = (self.name(mod), helper), []

        def pre(module, args):
            cm = self.call(key, kind, dict(x=args[0], **(extra or {})), ("x",), module, params, buffers)
            n, v, fin = cm.__enter__()
            if kind == "bn":
                n.extra["relu"] = True
            stack.append((cm, fin))
            return (v["x"],) + tuple(args[1:])

        def post(module, args, out):
            cm, fin = stack.pop()
            try:
                fin(out)
            finally:
                cm.__exit__(None, None, None)

        self.handles += [mod.register_forward_pre_hook(pre), (end or mod).register_forward_hook(post)]

    def remove(self):
        for h in self.handles:
            h.remove()
        self.handles = []

    def after_backward(self, ck):
        """every record has its upstream gradient and all the input gradients it expects, each exactly once; the checkpointed nodes ran twice"""
        for e in self.errors:
            ck.need(False, "recorder", *e)
        for key, n in self.nodes.items():
            for name in n.expect:
                ck.need(len(n.grads.get(name, ())) == 1, key, f"gradient '{name}' recorded {len(n.grads.get(name, ()))} times")
            want = 2 if key[0].startswith(self.twice) else 1
            ck.need(len(n.calls) == want, key, "calls", len(n.calls), "expected", want)


# ---------------------------------------------------------------------------------------------------- the checker
class Checker:
    """collects every failed check (so that one run names them all) and the worst figures per node kind; done() asserts"""

    def __init__(self, mode):
        self.mode, self.fails, self.worst, self.gate, self.verbose = mode, [], {}, 0.0, True

    def need(self, ok, *what):
        if not ok:
            self.fails.append(what)
            if self.verbose:
                print("FAILED:", *what)

    def values(self, tag, kind, got, ref, terms, rel, fro=None, ulp=0.0, extra=None, once=None, keep=None):
        """|got - ref| <= rel sum|terms| + ulp |ref| + TINY [+ extra] per element; relative Frobenius <= fro; with once (a dtype: the statement rounded
        once to it): signed mean within rel mean(sum|terms|) + |mean(once - ref)|, and, where the output rounding is the node's error budget
        (bf16 maps), Frobenius error within FRO_MARGIN of the once-rounded statement's own; keep: the elements these two are taken over (a ReLU gate
        within rounding of zero may flip, which the per-element bar absorbs and a norm cannot)"""
        if got is None or got.shape != ref.shape:
            self.need(False, tag, "missing or misshapen", None if got is None else tuple(got.shape), tuple(ref.shape))
            return
        got = got.double()
        self.need(bool(torch.isfinite(got).all()), tag, "not finite")
        d = got - ref
        bar = rel * terms + ulp * ref.abs() + TINY
        if extra is not None:
            bar = bar + extra
        worst = float((d.abs() / bar).max()) if d.numel() else 0.0
        nref = float(ref.norm())
        e = float(d.norm()) / nref if nref > 0 else float(d.norm())
        msg = f"[{tag}] worst |error| / bar {worst:.3f}; relative Frobenius {e:.3e}"
        w = self.worst.setdefault(kind, [0.0, 0.0, 0.0])
        w[0] = max(w[0], worst)
        self.need(worst <= 1.0, tag, "per-element bar", worst)
        if fro is not None:
            w[1] = max(w[1], e / fro)
            self.need(e <= fro, tag, "relative Frobenius", e, fro)
        if once is not None and d.numel():
            o = ref.to(once).double() - ref
            if keep is not None:
                d, o, terms = d[keep], o[keep], terms[keep]
            mean, mean1, mterms = float(d.mean()), float(o.mean()), float(terms.mean())
            msg += f"; signed mean {mean:+.2e} (once rounded {mean1:+.2e}, bar {rel * mterms + abs(mean1):.2e})"
            self.need(abs(mean) <= rel * mterms + abs(mean1) + TINY, tag, "signed mean", mean, rel * mterms, mean1)
            if once == torch.bfloat16 and float(o.norm()) > 0:
                ratio = float(d.norm()) / float(o.norm())
                w[2] = max(w[2], ratio)
                msg += f"; Frobenius ratio to the once-rounded statement {ratio:.4f}"
                self.need(ratio <= FRO_MARGIN, tag, "Frobenius against the once-rounded statement", ratio)
        if self.verbose:
            print(msg)

    def done(self, tag):
        for kind, (w, f, r) in sorted(self.worst.items()):
            print(f"[{tag}] {kind}: worst |error| / bar {w:.3f}, worst Frobenius / bar {f:.3f}, worst ratio to the once-rounded statement {r:.4f}")
        print(f"[{tag}] largest ambiguous-gate share {self.gate:.3e} (cap {GATE_CAP:.3e})")
        assert not self.fails, (tag, len(self.fails), self.fails[:20])


# ---------------------------------------------------------------------------------------------------- fp64 statements
def ones_mask(t):
    return torch.ones((t.shape[0], 1, t.shape[2], t.shape[3]), dtype=torch.float32, device=t.device)


def conv3x3_statement(x, w, b, g, mask_in, mask_out, stride):
    """mask_out * (conv3x3(x, W) + b) at the active outputs, dx at the active inputs, dW over the active outputs, db: each (value, sum|terms|),
    gathered (n, C) for y at `so` and dx at `si`"""
    r = _conv_refs(x, w, g, mask_in, mask_out, stride)
    if b is not None:
        b64 = b.detach().double()
        r["y"] = (r["y"][0] + b64, r["y"][1] + b64.abs())
    g64 = g.detach().double() * mask_out.double()
    r["db"] = (g64.sum(dim=(0, 2, 3)), g64.abs().sum(dim=(0, 2, 3)))
    return r


def lib_conv_statement(x, w, b, g, stride=1, padding=0, dilation=1, transposed=False):
    """a dense convolution (or the 2x2 / stride-2 transposed one) as fused_graph_ref states it tap by tap, and its gradients, in fp64; the sums of
    |terms| are the same bilinear form on |x|, |W|, |g|"""
    f = (lambda a, c: R.deconv2x2(a, c)) if transposed else (lambda a, c: R.conv2d(a, c, stride, padding, dilation))
    g64 = g.detach().double()
    out = []
    with torch.enable_grad():
        for xx, ww, gg in ((x.detach().double(), w.detach().double(), g64), (x.detach().double().abs(), w.detach().double().abs(), g64.abs())):
            xx, ww = xx.requires_grad_(True), ww.requires_grad_(True)
            y = f(xx, ww)
            dx, dw = torch.autograd.grad(y, (xx, ww), gg)
            out.append((y.detach(), dx, dw))
    (y, dx, dw), (ya, dxa, dwa) = out
    if b is not None:
        b64 = b.detach().double().view(1, -1, 1, 1)
        y, ya = y + b64, ya + b64.abs()
    return dict(y=(y, ya), dx=(dx, dxa), dw=(dw, dwa), db=(g64.sum(dim=(0, 2, 3)), g64.abs().sum(dim=(0, 2, 3))))


TILE_REACH = 7


def tile_terms(w, g, sites):
    """sum|terms| of a 3x3 data gradient computed in a TRANSFORM domain (the vendor library's fp32 Winograd kernels): a tile's upstream gradients and a
    channel's nine taps are mixed before they are multiplied, so an element's round-off scales with sum_k (sum of |g_k| over its tile) (sum_taps |W_k,ci|),
    not with its own nine products -- with ONE output channel and an upstream gradient that is zero except at a few positives, an element whose only tap
    is a small weight carries 1e-4 .. 1e-3 of its own sum|terms| while the map's relative Frobenius error is 9e-8 (CHANGELOG).  Tiles are at most 8 x 8
    inputs (F(6,3)): the box reaches TILE_REACH = 7 cells each way.  Where no upstream gradient lies within reach the bar is still TINY: exact zero."""
    ga = TF.avg_pool2d(g.detach().double().abs(), 2 * TILE_REACH + 1, 1, TILE_REACH, divisor_override=1)
    wa = w.detach().double().abs().sum(dim=(2, 3))                                         # (k, ci)
    b, y, x = sites
    return ga.permute(0, 2, 3, 1)[b, y, x] @ wa


def bn_statement(call, norm, relu, gy):
    """BatchNorm over the active sites + residual + ReLU + mask on the recorded operands (every site where the record has no mask), its backward for
    the recorded upstream gradient, the ambiguous gates and what they add to the bars"""
    x = call["x"]
    mask = call["mask"] if call["mask"] is not None else ones_mask(x)
    r = _bn_ref(x, mask, call["gamma"], call["beta"], call["residual"], relu, call["rm"], call["rv"], norm.eps, norm.momentum)
    act = (mask != 0).expand_as(x)
    amb = act & (r["pre"].abs() <= GATE_REL * r["prea"]) if relu else torch.zeros_like(act)
    r.update(act=act, amb=amb, share=float(amb.sum()) / max(float(act.sum()), 1.0), mask=mask)
    if gy is None:
        return r, None
    rb = _bn_ref_backward(r, gy)
    gu = gy.double() * r["m"]                                           # the upstream gradient before the gate
    ga = gu.abs() * amb
    cs = (1, -1, 1, 1)
    a = (r["gamma"] * r["invstd"]).abs().view(cs)
    xa = (r["x64"].abs() + r["mean"].abs().view(cs)) * r["invstd"].view(cs)
    db_x, dg_x = ga.sum(dim=(0, 2, 3)), (ga * xa).sum(dim=(0, 2, 3))
    rb.update(gu=gu, dbeta_x=db_x, dgamma_x=dg_x, dx_x=a * (ga + (db_x / r["cnt"]).view(cs) + xa * (dg_x / r["cnt"]).view(cs)) * r["m"])
    return r, rb


def running_update(norm, mean, var, cnt, rm, rv):
    mom = norm.momentum
    return (1 - mom) * rm.double() + mom * mean, (1 - mom) * rv.double() + mom * var * cnt / (cnt - 1).clamp(min=1.0)


# ---------------------------------------------------------------------------------------------------- value checks per node kind
def conv_node_values(ck, tag, kind, n, mode, bars, mask_in=None, mask_out=None, stride=1, lib_dx=False):
    """a 3x3 / pad-1 node (masked, dense or the SepHead output convolution) against conv3x3_statement on its recorded operands"""
    rel, fro, ulp = bars
    g = n.grad("out")
    if g is None:
        ck.need(False, tag, "no upstream gradient")
        return
    dense = mask_out is None
    mo = ones_mask(n.out) if dense else mask_out
    mi = ones_mask(n.x) if dense else mask_in
    w = n.w if lib_dx and mode.hip else mode.op(n.w)     # the SepHead output kernels read the fp32 master weights, under autocast too
    r = conv3x3_statement(mode.op(n.x), w, n.b, mode.op(g), mi, mo, stride)
    once = n.out.dtype if mode.hip else None
    ck.values(f"{tag} y", kind, _gather(n.out, r["so"]), *r["y"], rel, fro, ulp, once=once)
    if mode.hip and not dense:
        ck.need(zero_bits(n.out[(mo == 0).expand_as(n.out)]), tag, "y is not bit-zero at the inactive outputs")
    dx = n.grad("x")
    if "x" in n.expect:
        if lib_dx:     # the SepHead output convolution's data gradient runs on the library, on the weights in the map's dtype
            rl = _conv_refs(mode.op(n.x), mode.op(n.w), mode.op(g), mi, mo, 1, want_w=False)
            got = None if dx is None else _gather(dx, rl["si"])
            ref, terms = rl["dx"]
            if got is not None:
                print(f"[{tag} dx (library)] against the element's own sum|terms|: worst |error| / bar "
                      f"{float(((got.double() - ref).abs() / (mode.lib[0] * terms + mode.lib[1] * ref.abs() + TINY)).max()):.3f}")
            ck.values(f"{tag} dx (library)", "library", got, ref, tile_terms(mode.op(n.w), mode.op(g), rl["si"]), mode.lib[0], X3_FRO if not mode.amp else None, mode.lib[1])
        else:
            ck.values(f"{tag} dx", kind, None if dx is None else _gather(dx, r["si"]), *r["dx"], rel, fro, ulp, once=dx.dtype if mode.hip and dx is not None else None)
            if mode.hip and not dense and dx is not None:
                ck.need(zero_bits(dx[(mi == 0).expand_as(dx)]), tag, "dx is not bit-zero at the inactive inputs")
    dw = n.grad("w")
    ck.values(f"{tag} dw", kind, dw, *r["dw"], rel, fro, BF_OUT if dw is not None and dw.dtype == torch.bfloat16 else 0.0)   # a gradient held in bf16: one output rounding
    if n.b is not None:
        ck.values(f"{tag} db", kind, n.grad("b"), *r["db"], BF_REL if mode.amp else rel)


def lib_node_values(ck, tag, n, mode, conv=None, padding=0, dilation=1, transposed=False):
    g = n.grad("out")
    if g is None:
        ck.need(False, tag, "no upstream gradient")
        return
    if conv is not None:
        transposed = isinstance(conv, torch.nn.ConvTranspose2d)
        padding, dilation = conv.padding[0], conv.dilation[0]
        ck.need(conv.groups == 1 and (transposed or conv.stride == (1, 1)), tag, "an unexpected library layer")
    r = lib_conv_statement(mode.op(n.x), mode.op(n.w), None if n.b is None else mode.op(n.b), mode.op(g), 1, padding, dilation, transposed)
    rel, ulp = mode.lib
    worst = []
    for name, got in (("y", n.out), ("dx", n.grad("x")), ("dw", n.grad("w"))) + ((("db", n.grad("b")),) if n.b is not None else ()):
        if name == "dx" and "x" not in n.expect:
            continue
        # under autocast a convolution with a bias is TWO library operations, each of which rounds its result to bf16: the convolution, then the addition
        # of the bias; the bar of y carries one output rounding for each (|conv| and |conv + b|)
        extra = ulp * (r["y"][0] - n.b.double().view(1, -1, 1, 1)).abs() if name == "y" and n.b is not None and mode.amp else None
        ck.values(f"{tag} {name}", "library", got, *r[name], rel, None, ulp, extra=extra)
        if got is not None and got.shape == r[name][0].shape:
            worst.append(float(((got.double() - r[name][0]).abs() / (rel * r[name][1] + ulp * r[name][0].abs() + TINY + (0 if extra is None else extra))).max()))
    print(f"[{tag}] library layer: worst |error| / bar {max(worst):.3f}")


def bn_node_values(ck, tag, kind, n, norm, mode, final=True):
    """a BatchNorm + residual + ReLU + mask node: y, dx, dresidual, dgamma, dbeta, and the running statistics after ALL its calls"""
    relu, c, ulp = n.extra["relu"], n.calls[0], mode.bn_ulp
    gy = n.grad("out")
    r, rb = bn_statement(c, norm, relu, gy)
    ck.gate = max(ck.gate, r["share"])
    ck.need(r["share"] <= GATE_CAP, tag, "ambiguous ReLU gates above the cap", r["share"])
    act, y = r["act"], n.out
    once = y.dtype if mode.hip else None
    ck.values(f"{tag} y", kind, y[act], r["y"][act], (r["prea"] * r["m"])[act], BN_REL, None, ulp, once=once)
    ck.need(zero_bits(y[~act], mode.hip), tag, "y is not bit-zero at the inactive sites")
    if rb is None:
        ck.need(False, tag, "no upstream gradient")
    else:
        dx = n.grad("x")
        if "x" in n.expect and dx is not None:
            ck.values(f"{tag} dx", kind, dx[act], rb["dx"][act], rb["dxa"][act], BN_REL, None, ulp, extra=rb["dx_x"][act], once=dx.dtype if mode.hip else None,
                      keep=~r["amb"][act])
            ck.need(zero_bits(dx[~act], mode.hip), tag, "dx is not bit-zero at the inactive sites")
        if c["residual"] is not None:
            dres = n.grad("residual")
            ck.need(dres is not None, tag, "no residual gradient")
            if dres is not None:
                dres, amb = dres.double(), r["amb"]
                ck.need(torch.equal(dres[~amb], rb["g"][~amb]), tag, "dresidual is not the gated upstream gradient, exactly",
                        int((dres[~amb] != rb["g"][~amb]).sum()))
                ck.need(bool(((dres[amb] == rb["gu"][amb]) | (dres[amb] == 0)).all()), tag, "dresidual at an ambiguous gate is neither g nor 0")
        ck.values(f"{tag} dgamma", kind, n.grad("gamma"), rb["dgamma"], rb["dgamma_a"], BN_REL, extra=rb["dgamma_x"])
        ck.values(f"{tag} dbeta", kind, n.grad("beta"), rb["dbeta"], rb["dbeta_a"], BN_REL, extra=rb["dbeta_x"])
    if not final:
        return r
    # running statistics: one update per call, each from the recorded "before" of that call
    sd, mom = r["var"].sqrt(), norm.momentum
    after = [(cc["rm"], cc["rv"]) for cc in n.calls[1:]] + [(norm.running_mean.detach(), norm.running_var.detach())]
    for i, (cc, (rm1, rv1)) in enumerate(zip(n.calls, after)):
        rm, rv = running_update(norm, r["mean"], r["var"], r["cnt"], cc["rm"], cc["rv"])
        ck.values(f"{tag} running_mean (update {i + 1})", kind, rm1, rm, cc["rm"].double().abs() + mom * (r["mean"].abs() + sd), BN_REL)
        ck.values(f"{tag} running_var (update {i + 1})", kind, rv1, rv, cc["rv"].double().abs() + mom * r["var"] * 2, BN_REL)
    ck.need(int(norm.num_batches_tracked) == int(c["nbt"]) + len(n.calls), tag, "num_batches_tracked", int(norm.num_batches_tracked), int(c["nbt"]), len(n.calls))
    return r


# ---------------------------------------------------------------------------------------------------- wiring
def same(ck, tag, a, b, what):
    ck.need(biteq(a, b), tag, what)


def fork(ck, tag, total, parts):
    """the gradient a producer receives = the sum of what its consumers returned: exact for two, (n - 1) roundings of the dtype against sum|parts| for n"""
    if total is None or any(p is None for p in parts):
        ck.need(False, tag, "fork: a contribution is missing", [p is None for p in parts], total is None)
        return
    if len(parts) == 1:
        ck.need(biteq(total, parts[0]), tag, "the upstream gradient is not what the single consumer returned")
    elif len(parts) == 2:
        ck.need(biteq(total, parts[0] + parts[1]), tag, "fork of two: the total is not the sum of the two contributions")
    else:
        s, sa = sum(p.double() for p in parts), sum(p.double().abs() for p in parts)
        ck.need(bool(((total.double() - s).abs() <= (len(parts) - 1) * HALF_ULP[total.dtype] * sa + TINY).all()), tag, f"fork of {len(parts)}",
                float(((total.double() - s).abs() / (sa + TINY)).max()))


def check_graph(ck, model, rec, mode, canvas, occ, counts=None):
    """wiring, forks and values of every recorded node of model(ex) / the CPU chain; occ (B,1,H,W) 0/1 float, canvas the backbone's input"""
    N, bb, nk, hd = rec.nodes, model.backbone, model.neck, model.head
    seen = set()

    def node(name, helper):
        n = N.get((name, helper))
        ck.need(n is not None and n.calls, name, helper, "was not recorded")
        seen.add((name, helper))
        return n if n is not None and n.calls else None

    def gfn(n, want, tag):
        if mode.hip and n is not None:
            ck.need(n.gfn == want, tag, "grad_fn", n.gfn, "expected", want)
            kinds[want] = kinds.get(want, 0) + 1

    kinds = {}
    bnfn, skfn = "_MaskedBNActFnBackward", "_SmallKConv3x3FnBackward"

    def bn(name, helper, x_from, mask, residual, tag, kind):
        n = node(name, helper)
        if n is None:
            return None
        gfn(n, bnfn, tag)
        same(ck, tag, n.x, x_from.out, "input is not the recorded output of the node before it")
        fork(ck, tag + " <- its BatchNorm", x_from.grad("out"), [n.grad("x")])
        ck.need((n.mask is None and mask is None) or biteq(n.mask, mask), tag, "mask is not the stage's")
        ck.need((n.residual is None) == (residual is None) and (residual is None or biteq(n.residual, residual)), tag, "residual is not the block's recorded input")
        bn_node_values(ck, tag, kind, n, model.get_submodule(name), mode)
        return n

    # ---- backbone
    prev_out, prev_consumers, mask = canvas, None, occ
    first_dx = None
    for si, blk in enumerate(bb.blocks):
        ch = blk[0].conv.out_channels
        m_in, mask = mask, TF.max_pool2d(mask, 3, blk[0].stride, 1)
        for j, m in enumerate(blk):
            entry = j == 0
            pre = f"backbone.blocks.{si}.{j}"
            convs = [(pre + ".conv", pre + ".norm", False)] if entry else [(pre + ".block1.conv", pre + ".block1.norm", False), (pre + ".conv2", pre + ".norm2", True)]
            block_in, block_grads = prev_out, []
            for cname, nname, with_res in convs:
                tag = f"{mode.name} {cname}"
                n = node(cname, "masked_conv")
                if n is None:
                    return
                gfn(n, mode.conv_fn, tag)
                mi = m_in if entry else mask
                same(ck, tag, n.x, prev_out, "input is not the recorded output of the node before it")
                same(ck, tag, n.mask_out, mask, "mask_out is not max_pool2d of the recorded occupancy chain")
                same(ck, tag, n.mask_in, mi, "mask_in is not the input's active set")
                conv_node_values(ck, tag, f"masked conv {ch}ch s{m.stride if entry else 1}", n, mode, mode.conv, mi, mask, blk[0].stride if entry else 1)
                if first_dx is None:
                    first_dx = (n.grad("x"),)
                if not with_res:
                    block_grads.append(n.grad("x"))
                b = bn(nname, "masked_bn_act", n, mask, block_in if with_res else None, f"{mode.name} {nname}", f"masked bn {ch}ch")
                if b is None:
                    return
                if with_res:
                    block_grads.append(b.grad("residual"))
                prev_out = b.out
                if with_res:
                    fork(ck, f"{mode.name} {pre}.block1.norm -> conv2", mid.grad("out"), [n.grad("x")])
                mid = b
            # the block's input is consumed by its first convolution (and, in a residual block, by the second BatchNorm node's residual)
            if prev_consumers is not None:
                fork(ck, f"{mode.name} {pre}: gradient of the block's input", prev_consumers.grad("out"), block_grads)
            prev_consumers = b
    # ---- mapping
    tag = f"{mode.name} backbone.mapping"
    n = node("backbone.mapping.0", "module")
    if n is None:
        return
    same(ck, tag, n.x, prev_out, "input is not the last stage's output")
    fork(ck, tag, prev_consumers.grad("out"), [n.grad("x")])
    lib_node_values(ck, tag + ".0", n, mode, bb.mapping[0])
    xm = bn("backbone.mapping.1", "masked_bn_act", n, mask, None, tag + ".1", "masked bn 256ch")
    # ---- neck (checkpointed: every node below ran twice)
    p = "neck.pre_conv."
    c1 = node(p + "block1.conv.conv", "x3_conv")
    if c1 is None or xm is None:
        return
    gfn(c1, mode.conv_fn, p + "block1")
    same(ck, p + "block1", c1.x, xm.out, "input is not the mapping's output")
    conv_node_values(ck, f"{mode.name} {p}block1.conv", "dense conv 256ch", c1, mode, mode.conv)
    b1 = bn(p + "block1.norm", "dense_bn_act", c1, None, None, f"{mode.name} {p}block1.norm", "dense bn")
    c2 = node(p + "block2.conv.conv", "x3_conv")
    if c2 is None or b1 is None:
        return
    gfn(c2, mode.conv_fn, p + "block2")
    same(ck, p + "block2", c2.x, b1.out, "input is not block1's output")
    fork(ck, p + "block1.norm", b1.grad("out"), [c2.grad("x")])
    conv_node_values(ck, f"{mode.name} {p}block2.conv", "dense conv 256ch", c2, mode, mode.conv)
    b2 = bn(p + "block2.norm", "dense_bn_act", c2, None, None, f"{mode.name} {p}block2.norm", "dense bn")
    act = node(p + "act", "module")
    if act is None or b2 is None:
        return
    tag = f"{mode.name} {p}act"
    s64 = b2.out.double() + xm.out.double()
    ck.need(bool(((act.x.double() - s64).abs() <= HALF_ULP[act.x.dtype] * s64.abs() + TINY).all()), tag, "input is not block2's output + the block's input")
    ck.need(torch.equal(act.out.double(), act.x.double().clamp(min=0)), tag, "output is not relu(input)")
    ga = act.grad("out")
    ck.need(ga is not None and act.grad("x") is not None and torch.equal(act.grad("x").double(), ga.double() * (act.x > 0)), tag, "dx is not the gated upstream gradient")
    fork(ck, tag + " -> block2.norm", b2.grad("out"), [act.grad("x")])
    fork(ck, f"{mode.name} mapping output -> block1 + residual", xm.grad("out"), [c1.grad("x"), act.grad("x")])
    x = act.out
    one = node("neck.conv1x1", "module")
    branches = [one] + [node("neck.weight", f"conv_d{d}") for d in R.ASPP_DILATIONS]
    post = node("neck.post_conv.conv.conv", "x3_conv")
    if post is None or any(b is None for b in branches):
        return
    for b, d in zip(branches, (0,) + R.ASPP_DILATIONS):
        tag = f"{mode.name} neck " + ("conv1x1" if d == 0 else f"aspp d{d}")
        same(ck, tag, b.x, x, "input is not pre_conv's output")
        if d:
            same(ck, tag, b.w, nk.weight.detach().to(x.dtype), "weight is not the neck's shared weight")
        if d == 1 and mode.hip:
            gfn(b, mode.conv_fn, tag)
            conv_node_values(ck, tag, "dense conv 256ch", b, mode, mode.conv)
        else:
            lib_node_values(ck, tag, b, mode, padding=d, dilation=max(d, 1))
    same(ck, "neck.post_conv", post.x, torch.cat([x] + [b.out for b in branches], dim=1), "input is not cat(x, conv1x1, d1, d6, d12, d18)")
    gp = post.grad("x")
    C = x.shape[1]
    if gp is None:
        ck.need(False, "neck.post_conv", "no input gradient")
        return
    for k, b in enumerate(branches):
        ck.need(biteq(b.grad("out"), gp[:, (k + 1) * C:(k + 2) * C]), b.key, "upstream gradient is not its slice of post_conv's input gradient")
    fork(ck, f"{mode.name} neck x -> identity / 1x1 / four dilations", act.grad("out"), [gp[:, :C]] + [b.grad("x") for b in branches])
    lib_node_values(ck, f"{mode.name} neck.post_conv.conv", post, mode, nk.post_conv.conv.conv)
    nout = bn("neck.post_conv.norm", "dense_bn_act", post, None, None, f"{mode.name} neck.post_conv.norm", "dense bn")
    # the shared weight: four uses
    wg = [b.grad("w") for b in branches[1:]]
    if all(g is not None for g in wg) and nk.weight.grad is not None:
        s, sa = sum(g.double() for g in wg), sum(g.double().abs() for g in wg)
        ck.need(bool(((nk.weight.grad.double() - s).abs() <= 3 * HALF_ULP[wg[0].dtype] * sa + TINY).all()), "neck.weight", ".grad is not the sum over its four uses")
    else:
        ck.need(False, "neck.weight", "a use of the shared weight has no gradient")
    # ---- head
    sc = node("head.shared_conv.0", "module")
    if sc is None or nout is None:
        return
    same(ck, "head.shared_conv.0", sc.x, nout.out, "input is not the neck's output")
    fork(ck, "neck output", nout.grad("out"), [sc.grad("x")])
    lib_node_values(ck, f"{mode.name} head.shared_conv.0", sc, mode, hd.shared_conv[0])
    sh = bn("head.shared_conv.1", "dense_bn_act", sc, None, None, f"{mode.name} head.shared_conv.1", "dense bn")
    if sh is None:
        return
    task_dx = []
    for ti, task in enumerate(hd.tasks):
        p = f"head.tasks.{ti}."
        dc = node(p + "deblock.conv.conv", "x3_conv")
        if dc is None:
            return
        same(ck, p + "deblock", dc.x, sh.out, "input is not the shared convolution's output")
        task_dx.append(dc.grad("x"))
        lib_node_values(ck, f"{mode.name} {p}deblock.conv", dc, mode, task.deblock.conv.conv)
        up = bn(p + "deblock.norm", "dense_bn_act", dc, None, None, f"{mode.name} {p}deblock.norm", "dense bn")
        if up is None:
            return
        dxs = []
        for h in task.heads:
            q = f"{p}{h}."
            f0, f3 = node(q + "0", "x3_conv"), node(q + "3", "smallk_conv")
            if f0 is None or f3 is None:
                return
            gfn(f0, mode.conv_fn, q + "0")
            same(ck, q + "0", f0.x, up.out, "input is not the deblock's output")
            if "pieces" in f0.extra:
                ck.need(len(rec.splits) > ti and f0.extra["pieces"][0] is rec.splits[ti][1] and biteq(rec.splits[ti][0], up.out)
                        and all(biteq(a, b) for a, b in zip(f0.extra["pieces"][1], rec.splits[ti][2])), q + "0", "the shared pieces are not this task's split of the deblock output")
                ps = sum(t.double() for t in f0.extra["pieces"][1])
                tol = 0.0 if len(f0.extra["pieces"][1]) == 3 else 2.0 ** -16
                ck.need(bool(((ps - up.out.double()).abs() <= tol * up.out.double().abs()).all()), q + "0", "the pieces do not add up to the deblock output")
            elif mode.name in ("x3", "x6"):
                ck.need(False, q + "0", "the fp32 graph did not share the pieces of the deblock output")
            dxs.append(f0.grad("x"))
            conv_node_values(ck, f"{mode.name} {q}0", "dense conv 64ch", f0, mode, mode.conv)
            f1 = bn(q + "1", "dense_bn_act", f0, None, None, f"{mode.name} {q}1", "dense bn")
            if f1 is None:
                return
            gfn(f3, skfn, q + "3")
            same(ck, q + "3", f3.x, f1.out, "input is not the branch's BatchNorm output")
            fork(ck, q + "1", f1.grad("out"), [f3.grad("x")])
            conv_node_values(ck, f"{mode.name} {q}3", "smallk conv", f3, mode, mode.smallk, lib_dx=mode.hip)
        fork(ck, f"{mode.name} {p}deblock output -> {len(dxs)} branches", up.grad("out"), dxs)
    fork(ck, f"{mode.name} shared -> tasks", sh.grad("out"), task_dx)
    # ---- nothing recorded that the walk did not visit; parameters
    for key in N:
        ck.need(key in seen, key, "recorded, but not part of the expected graph")
    for key, n in N.items():
        for rname, prm in n.extra.get("params", {}).items():
            g = n.grad(rname)
            if prm.requires_grad:
                ck.need(g is not None and prm.grad is not None and biteq(prm.grad, g), key, rname, ".grad is not the gradient its node returned")
    for name, prm in model.named_parameters():
        if prm.requires_grad and not (name.startswith("reader.") and rec.canvas is None):
            ck.need(prm.grad is not None and bool(torch.isfinite(prm.grad).all()), name, "no finite gradient")
    if mode.hip and counts is not None:
        print(f"[{mode.name}] nodes per kind: {kinds}")
        ck.need(kinds == counts, mode.name, "node counts", kinds, "expected", counts)
    return first_dx[0] if first_dx else None


# ---------------------------------------------------------------------------------------------------- geometry shared by the GPU test and the CPU gate test
PC_RANGE, VOXEL = (-20.8, -13.6, -5.0, 20.8, 13.6, 3.0), (0.2, 0.2, 8.0)
NY, NX, B = 136, 208, 3
CLOUDS = (1000, (("sweep", 8000), ("empty", 500), ("sweep", 8000)))        # FRAMES[0] of tests/test_gpu_fused_graph_vs_fp64.py
TASKS = [["car"], ["pedestrian", "cyclist"]]


def cloud_points():
    """the three clouds of CLOUDS as one (n, 6) float32 array; the GPU test holds it equal to test_gpu_fused_graph_vs_fp64._frame(*FRAMES[0])"""
    from pillarnext_amd import synth

    seed0, kinds = CLOUDS
    out = []
    for b, (kind, n) in enumerate(kinds):
        p = (synth.sweep_cloud if kind == "sweep" else synth.uniform_cloud)(n, PC_RANGE, seed0 + b, batch_idx=b)
        out.append(synth.push_outside(p, PC_RANGE, 1.0, 77000 + seed0 + b) if kind == "empty" else p)
    return np.concatenate(out)


def cloud_occupancy(pts):
    """(B,1,NY,NX) float occupancy of the points' cells (the reader's rule: floor((p - range min) / voxel), points outside the range dropped)"""
    p = pts.astype(np.float64)
    ix, iy = np.floor((p[:, 1] - PC_RANGE[0]) / VOXEL[0]).astype(np.int64), np.floor((p[:, 2] - PC_RANGE[1]) / VOXEL[1]).astype(np.int64)
    ok = (ix >= 0) & (ix < NX) & (iy >= 0) & (iy < NY) & (p[:, 3] >= PC_RANGE[2]) & (p[:, 3] < PC_RANGE[5])
    occ = np.zeros((B, 1, NY, NX), np.float32)
    occ[p[ok, 0].astype(np.int64), 0, iy[ok], ix[ok]] = 1.0
    return torch.from_numpy(occ)


def build_model(seed=21, bn_seed=22, pc_range=PC_RANGE):
    from pillarnext_amd.models import build_pillarnext_b
    from test_fused_graph_ref_cpu import random_bn_

    torch.manual_seed(seed)
    model = build_pillarnext_b(pc_range, VOXEL, tasks=TASKS).train()
    random_bn_(model, bn_seed)
    return model


def run_dense_chain(model, canvas, occ, head_grads=None):
    """the graph behind the reader on a given canvas: backbone.forward_dense -> neck -> head; with head_grads ({(task, branch): tensor}) a synthetic
    loss sum(pred * head_grads) is backpropagated (the loss kernels' own values are held elsewhere)"""
    with torch.utils.checkpoint.set_checkpoint_early_stop(False):     # read when the checkpoint is entered: the recomputation runs to its end, so its last node is recorded whole
        x = model.backbone.forward_dense(canvas, occ)
        preds = model.head(model.neck(x))
        if head_grads is not None:
            loss = sum((preds[ti][k].float() * g).sum() for (ti, k), g in head_grads.items())
            loss.backward()
    return preds
