"""GPU: every layer of the fused inference graph (models.FusedPillarNeXt) against fp64, layer by layer, with TEACHER FORCING: the graph's own stored input
of layer k goes through layer k as tests/fused_graph_ref.py states it from the ORIGINAL detector's parameters, and the graph's output of layer k is held to
that.  No error carries from layer to layer, so the per-element bars of the at-scale kernel tests apply to every layer of the COMPOSED graph, and a wiring
mistake (a BatchNorm folded into the wrong weight, a stage given the wrong mask, a residual read from the wrong one of the three rotating stage buffers or
added on the wrong side of the ReLU, a branch of the ASPP or of the merged SepHead in the wrong place) is an O(1) error at the sites it touches.

Capture: forward hooks on every module of the graph clone input, mask, residual and output when the module is called (the stage outputs live in three
rotating persistent buffers); the reader's call is wrapped to clone the canvas and the occupancy it wrote; models.py is used as it is.  forward_preds(...,
taps={}) runs launch by launch, so the hooks fire; test_launch_plans_equal_the_python_launch_loop and the last part of this test tie the planned path to
it bit for bit.  While the fp64 statement runs, every `lib` of the package raises: the reference cannot reach a HIP kernel.

Geometry: the smallest at which the composition can still go wrong.  136 x 208 cells of 0.2 m: not square, both sides multiples of 8 (three stride-2
stages, the 2x deblock), the width no multiple of 32 and the height no multiple of 16 or 8 at any stage (208/104/52/26 wide, 136/68/34/17 high), so every
stage has a ragged last tile column and row; the neck runs on 17 x 26, where at dilation 12 and 18 whole rings of taps fall into the padding.  B = 3
with one sample that has no point inside the range.

Bars, per recorded layer, every element compared (`ref`: the UNROUNDED statement on the recorded input):
  wiring, exact   masks = max_pool2d of the recorded occupancy chain; canvas zero off the occupancy; every layer's input = the recorded output of the layer
                  before it; the residual of a block's second convolution = the recorded output two layers before; pre2 gets post_residual; bit-zero at
                  every inactive site and in the padded channels of the packed head maps;
  per element     |got - ref| <= (W_REL + BF_REL) sum|terms| + OUT_ROUND |ref| + TINY   (+ OUT_ROUND sum_d |part_d| for the neck's four stored partial
                  maps).  BF_REL, TINY, OUT_ROUND: the at-scale modules', unchanged.  W_REL: half an ulp of the element type -- the reference holds the
                  folded weights unrounded, the graph rounds them once;
  Frobenius       over the active set, ||got - ref|| <= FRO_MARGIN (1.25) ||once-rounded statement - ref||, the second norm measured here, no kernel involved;
  signed mean     |mean(got - ref)| <= BF_REL mean(sum|terms|) + |mean(once-rounded statement - ref)|, as in the at-scale modules.
-rP prints worst |error| / bar, the Frobenius ratio and the signed means per layer."""
import sys
from collections import namedtuple

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import fused_graph_ref as R  # noqa: E402
from test_fused_graph_ref_cpu import TASKS, random_bn_  # noqa: E402
from test_gpu_infer_kernels_at_scale import BF_REL, FRO_MARGIN, OUT_ROUND, TINY  # noqa: E402  (the at-scale modules' bars, unchanged)

W_REL = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}     # one rounding of a weight to an 8- / 11-bit significand
PC_RANGE, VOXEL = (-20.8, -13.6, -5.0, 20.8, 13.6, 3.0), (0.2, 0.2, 8.0)
NY, NX, B = 136, 208, 3
TILE_W, TILE_H = 32, {64: 16, 128: 8, 256: 8}                       # conv_taps.h LDS_TH, conv_rows.h L128_TH; every tile is 32 pixels wide
# per frame, per sample: (cloud, points); "empty": every point pushed outside the x/y range
FRAMES = ((1000, (("sweep", 8000), ("empty", 500), ("sweep", 8000))),
          (1007, (("empty", 500), ("uniform", 1500), ("uniform", 750))))

Rec = namedtuple("Rec", "x mask residual post_residual out")
Run = namedtuple("Run", "recs canvas occ neck packed")


def _frame(seed0, kinds):
    from pillarnext_amd import synth

    out = []
    for b, (kind, n) in enumerate(kinds):
        p = (synth.sweep_cloud if kind == "sweep" else synth.uniform_cloud)(n, PC_RANGE, seed0 + b, batch_idx=b)
        out.append(synth.push_outside(p, PC_RANGE, 1.0, 77000 + seed0 + b) if kind == "empty" else p)
    return torch.from_numpy(np.concatenate(out)).cuda()


def _bits(t):
    return t.contiguous(memory_format=torch.channels_last).view(torch.int16) if t.dim() == 4 else t.contiguous()


def biteq(a, b):
    return a is not None and b is not None and a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _nonzero_bits(t):
    return int(torch.count_nonzero(t.contiguous().view(torch.int16)))


# ---------------------------------------------------------------------------------------------------- capture
def _modules(fused):
    """name -> module of everything forward_preds calls as a module"""
    mods = {f"stage{si}.{j}": m for si, st in enumerate(fused.stages) for j, m in enumerate(st)}
    mods.update(mapping=fused.mapping, pre1=fused.pre1, pre2=fused.pre2, shared=fused.shared)
    for ti in range(len(fused.task_deblock)):
        mods.update({f"deblock{ti}": fused.task_deblock[ti], f"conv1_{ti}": fused.task_conv1[ti], f"conv2_{ti}": fused.task_conv2[ti],
                     f"lazy1_{ti}": fused.lazy_conv1[ti], f"lazy2_{ti}": fused.lazy_conv2[ti]})
    return mods


class Recorder:
    def __init__(self, fused):
        self.recs, self.handles = {}, []
        for name, m in _modules(fused).items():
            self.handles.append(m.register_forward_hook(self._hook(name), with_kwargs=True))

    def _hook(self, name):
        def hook(module, args, kwargs, output):
            assert name not in self.recs, (name, "called twice in one frame")

            def c(t):
                return None if t is None else t.clone()
            self.recs[name] = Rec(c(args[0]), c(args[1] if len(args) > 1 else kwargs.get("mask")), c(kwargs.get("residual")), c(kwargs.get("post_residual")),
                                  c(output))
        return hook

    def remove(self):
        for h in self.handles:
            h.remove()


def _run(fused, rec, pts, lazy, monkeypatch):
    """one frame batch launch by launch -> Run; the reader's canvas and occupancy are cloned as it returns"""
    seen = {}
    inner = fused.reader.forward_dense

    def forward_dense(points, batch_size, **kw):
        x = inner(points, batch_size, **kw)
        seen.update(canvas=x.clone(), occ=kw["occupancy"].clone())
        return x

    rec.recs = {}
    taps, packed = {}, []
    with monkeypatch.context() as mp:
        mp.setattr(fused.reader, "forward_dense", forward_dense, raising=False)
        fused.forward_preds(pts, B, taps=taps, packed_out=packed, lazy=lazy)
    torch.cuda.synchronize()
    return Run(rec.recs, seen["canvas"], seen["occ"], taps["neck"], packed)


def _block_kernels(mp):
    def boom(*a, **k):
        raise AssertionError("the fp64 statement reached the HIP library")

    n = 0
    for name, mod in list(sys.modules.items()):
        if name.startswith("pillarnext_amd") and callable(getattr(mod, "lib", None)):
            mp.setattr(mod, "lib", boom)
            n += 1
    assert n >= 2    # _lib itself and the modules that imported the name


# ---------------------------------------------------------------------------------------------------- the bars
class Checker:
    """collects every failed check of a test (so that one run names them all) and the worst figures per layer kind; done() asserts"""

    def __init__(self, dtype):
        self.dtype, self.fails, self.worst = dtype, [], {}

    def need(self, ok, *what):
        if not ok:
            self.fails.append(what)
            print("FAILED:", *what)

    def values(self, tag, kind, got, L, Lr, mask=None, Lc=None):
        """got (B,C,H,W) of the element type against Layer L (unrounded), Lr (once rounded); mask (B,1,H,W) fp64 or None = every site active"""
        dt = self.dtype
        got = got.double()
        self.need(got.shape == L.ref.shape, tag, "shape", tuple(got.shape), tuple(L.ref.shape))
        if got.shape != L.ref.shape:
            return
        d = got - L.ref
        bar = (W_REL[dt] + BF_REL) * L.terms + OUT_ROUND[dt] * L.ref.abs() + TINY
        if L.parts is not None:
            bar = bar + OUT_ROUND[dt] * L.parts
        worst = float((d.abs() / bar).max())
        if mask is not None:
            off = (mask == 0).expand_as(got)
            self.need(int(torch.count_nonzero(got[off])) == 0 and not bool(torch.signbit(got[off]).any()), tag, "non-zero bits at inactive sites")
            act = ~off
            d, once, ref, terms = d[act], (Lr.ref - L.ref)[act], L.ref[act], L.terms[act]
        else:
            once, ref, terms = Lr.ref - L.ref, L.ref, L.terms
        nref = float(ref.norm())
        fro, fro1 = float(d.norm()) / nref, float(once.norm()) / nref
        mean, mean1, mterms, mabs = float(d.mean()), float(once.mean()), float(terms.mean()), float(ref.abs().mean())
        extra = ""
        if Lc is not None:   # the statement that also rounds the convolution's own result
            oc = (Lc.ref - L.ref) if mask is None else (Lc.ref - L.ref)[act]
            extra = f" [conv result rounded too: ratio {fro / (float(oc.norm()) / nref):.4f}]"
        print(f"[{tag}] worst |error| / bar {worst:.3f}; relative Frobenius {fro:.3e} (once rounded {fro1:.3e}, ratio {fro / fro1:.4f}){extra}; "
              f"signed mean / mean|ref| {mean / mabs:+.2e} (once rounded {mean1 / mabs:+.2e}, bar {(BF_REL * mterms + abs(mean1)) / mabs:.2e})")
        w = self.worst.setdefault(kind, [0.0, 0.0])
        w[0], w[1] = max(w[0], worst), max(w[1], fro / fro1)
        self.need(worst <= 1.0, tag, "per-element bar", worst)
        self.need(fro <= FRO_MARGIN * fro1, tag, "Frobenius", fro, fro1, fro / fro1)
        self.need(abs(mean) <= BF_REL * mterms + abs(mean1), tag, "signed mean", mean, BF_REL * mterms, mean1)

    def done(self, tag):
        for kind, (w, f) in self.worst.items():
            print(f"[{tag}] {kind}: worst |error| / bar {w:.3f}, worst Frobenius ratio {f:.4f}")
        assert not self.fails, (tag, len(self.fails), self.fails)


def _d(t):
    return t.double()


def _mask64(m):
    return m.unsqueeze(1).double()


def _check_trunk(ck, tag, det, fused, run):
    """reader output -> neck: wiring + values of every recorded layer; -> the reach figures"""
    dt, recs, bb = ck.dtype, run.recs, det.backbone
    occ = run.occ
    ck.need(occ.dtype == torch.uint8 and tuple(occ.shape) == (B, NY, NX) and int(occ.max()) == 1, tag, "occupancy")
    ck.need(tuple(run.canvas.shape) == (B, 64, NY, NX) and run.canvas.dtype == dt, tag, "canvas", tuple(run.canvas.shape))
    ck.need(_nonzero_bits(run.canvas.permute(0, 2, 3, 1)[occ == 0]) == 0, tag, "canvas not zero off the occupancy")
    m64, prev, reach = _mask64(occ), run.canvas, []
    for si, blk in enumerate(bb.blocks):
        n = len(fused.stages[si])
        rs = [recs.get(f"stage{si}.{j}") for j in range(n)]
        ck.need(all(r is not None for r in rs) and n == 2 * (len(blk) - 1) + 1, tag, f"stage {si}: not every module was called")
        m_in, m64 = m64, R.pooled_mask(m64, blk[0].stride)
        mu8 = m64.squeeze(1).to(torch.uint8)
        H, W = mu8.shape[1:]
        th = TILE_H[blk[0].conv.out_channels]
        lc, lr = (W - 1) // TILE_W * TILE_W, (H - 1) // th * th
        reach.append(dict(share=float(m64.mean()), per_sample=[float(m64[b].mean()) for b in range(B)], last_col=int(mu8[:, :, lc:].sum()),
                          last_row=int(mu8[:, lr:].sum()), ragged=(W % TILE_W, H % th)))
        outs = []
        for j, r in enumerate(rs):
            name = f"{tag} stage{si}.{j}"
            ck.need(biteq(r.mask, mu8), name, "mask is not max_pool2d of the occupancy chain")
            ck.need(biteq(r.x, prev), name, "input is not the recorded output of the layer before")
            ck.need(r.post_residual is None, name, "post_residual")
            if j == 0:
                ck.need(r.residual is None, name, "an entry convolution with a residual")
                L, Lr = (R.sparse_conv_block(blk[0], _d(r.x), m_in, rounded=q) for q in (None, dt))
                ck.need(torch.equal(L.mask, m64), name, "statement mask")
            elif j % 2 == 1:
                ck.need(r.residual is None, name, "the first convolution of a block with a residual")
                L, Lr = (R.sparse_conv_block(blk[(j + 1) // 2].block1, _d(r.x), m64, rounded=q) for q in (None, dt))
            else:
                ck.need(biteq(r.residual, outs[j - 2]), name, "residual is not the recorded block input")
                L, Lr = (R.sparse_block_tail(blk[j // 2], _d(r.x), _d(outs[j - 2]), m64, rounded=q) for q in (None, dt))
            ck.values(name, f"backbone {blk[0].conv.out_channels}ch" + (" entry" if j == 0 else ""), r.out, L, Lr, m64)
            outs.append(r.out)
            prev = r.out
    r = recs["mapping"]
    ck.need(biteq(r.mask, m64.squeeze(1).to(torch.uint8)) and biteq(r.x, prev) and r.residual is None and r.post_residual is None, tag, "mapping wiring")
    L, Lr, Lc = (R.mapping(bb, _d(r.x), m64, rounded=q, conv_out=c) for q, c in ((None, False), (dt, False), (dt, True)))
    ck.values(f"{tag} mapping", "mapping", r.out, L, Lr, m64, Lc)
    x_map = r.out
    r = recs["pre1"]
    ck.need(r.mask is None and biteq(r.x, x_map) and r.residual is None and r.post_residual is None, tag, "pre1 wiring")
    L, Lr, Lc = (R.conv_block(det.neck.pre_conv.block1, _d(r.x), rounded=q, conv_out=c) for q, c in ((None, False), (dt, False), (dt, True)))
    ck.values(f"{tag} pre1", "neck pre_conv", r.out, L, Lr, None, Lc)
    y = r.out
    r = recs["pre2"]
    ck.need(r.mask is None and biteq(r.x, y), tag, "pre2 wiring")
    ck.need(r.residual is None and biteq(r.post_residual, x_map), tag, "pre2 must get the block input as post_residual (behind its ReLU)")
    L, Lr, Lc = (R.pre_conv_tail(det.neck.pre_conv, _d(r.x), _d(x_map), rounded=q, conv_out=c) for q, c in ((None, False), (dt, False), (dt, True)))
    ck.values(f"{tag} pre2", "neck pre_conv", r.out, L, Lr, None, Lc)
    L, Lr = (R.aspp(det.neck, _d(r.out), rounded=q) for q in (None, dt))
    ck.values(f"{tag} aspp", "neck aspp", run.neck, L, Lr)
    return reach


def _check_head(ck, tag, det, fused, run, lazy):
    dt, recs, hd = ck.dtype, run.recs, det.head
    r = recs["shared"]
    ck.need(biteq(r.x, run.neck) and r.mask is None and r.residual is None, tag, "shared wiring")
    L, Lr = (R.shared_conv(hd, _d(r.x), rounded=q) for q in (None, dt))
    ck.values(f"{tag} shared", "head shared", r.out, L, Lr)
    sh = r.out
    n1, n2, off = ("lazy1_", "lazy2_", ("conv1_", "conv2_")) if lazy else ("conv1_", "conv2_", ("lazy1_", "lazy2_"))
    ck.need(not any(k.startswith(off) for k in recs), tag, "the other head's modules were called")
    ck.need(len(run.packed) == len(hd.tasks), tag, "packed_out")
    for ti, task in enumerate(hd.tasks):
        names = list(task.heads)
        ck.need(names == ["reg", "height", "dim", "rot", "vel", "iou", "hm"] and (names, [task.heads[k][0] for k in names]) == tuple(fused.task_split[ti]),
                tag, ti, "branch order")
        if lazy:
            names = names[5:]           # the lazy layout: [iou] hm
        r = recs[f"deblock{ti}"]
        ck.need(biteq(r.x, sh), tag, ti, "deblock wiring")
        L, Lr = (R.deblock(task, _d(r.x), rounded=q) for q in (None, dt))
        ck.values(f"{tag} deblock{ti}", "head deblock", r.out, L, Lr)
        up = r.out
        r1, r2 = recs[n1 + str(ti)], recs[n2 + str(ti)]
        ck.need(biteq(r1.x, up) and biteq(r2.x, r1.out), tag, ti, "branch wiring")
        ck.need(tuple(r1.out.shape[:2]) == (B, 64 * len(names)) and tuple(r2.out.shape[:2]) == (B, 16), tag, ti, "merged widths", tuple(r1.out.shape), tuple(r2.out.shape))
        o = 0
        for j, name in enumerate(names):
            k = task.heads[name][0]
            L, Lr = (R.branch_first(task, name, _d(up), rounded=q) for q in (None, dt))
            ck.values(f"{tag} task{ti}.{name} conv1", "head conv1", r1.out[:, 64 * j:64 * (j + 1)], L, Lr)
            L, Lr = (R.branch_last(task, name, _d(r1.out[:, 64 * j:64 * (j + 1)]), rounded=q) for q in (None, dt))
            ck.values(f"{tag} task{ti}.{name} conv2", "head conv2", r2.out[:, o:o + k], L, Lr)
            o += k
        ck.need(o < 16 and _nonzero_bits(r2.out[:, o:]) == 0, tag, ti, "padded channels of the packed map are not zero")
        if lazy:
            ck.need(biteq(run.packed[ti].dense, r2.out) and biteq(run.packed[ti].up, up), tag, ti, "LazyTask")
        else:
            ck.need(biteq(run.packed[ti], r2.out), tag, ti, "packed map")


def _check_reach(ck, tag, reach, empty):
    for si, s in enumerate(reach):
        print(f"[{tag}] stage {si}: active share {s['share']:.3f} (per sample {[round(v, 3) for v in s['per_sample']]}), sites in the ragged last tile column "
              f"{s['last_col']}, row {s['last_row']} (remainders {s['ragged']})")
        ck.need(s["per_sample"][empty] == 0.0 and all(v > 0 for b, v in enumerate(s["per_sample"]) if b != empty), tag, si, "empty sample")
        ck.need(s["ragged"][0] > 0 and s["ragged"][1] > 0 and s["last_col"] > 0 and s["last_row"] > 0, tag, si, "ragged tiles not reached")
    ck.need(0.05 <= reach[0]["share"] <= 0.60, tag, "stage-0 active share", reach[0]["share"])


def _same_recordings(ck, tag, a, b, names=None):
    keys = [k for k in a.recs if names is None or k.startswith(names)]
    ck.need(len(keys) > 0 and all(k in b.recs for k in keys), tag, "recorded modules differ")
    for k in keys:
        if k in b.recs:
            ck.need(biteq(a.recs[k].out, b.recs[k].out) and biteq(a.recs[k].x, b.recs[k].x), tag, k, "recordings differ")
    ck.need(biteq(a.neck, b.neck) and biteq(a.occ, b.occ) and biteq(a.canvas, b.canvas), tag, "neck / reader recordings differ")


# ---------------------------------------------------------------------------------------------------- the test
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_every_layer_of_the_fused_graph_against_fp64(dtype, monkeypatch):
    """Two frame batches through ONE FusedPillarNeXt, every recorded layer held to the fp64 statement on its own recorded input: the first frame with
    the dense and with the lazy head, then a smaller active set with the empty sample moved (a row left over from the first frame has to pass the fp64
    bar and the bit-zero check), again without the stage workspaces (bit-equal recordings); last, the planned path on a second instance against the
    verified launch-by-launch path, detections bit for bit."""
    from pillarnext_amd import models, ops
    from pillarnext_amd.fused import _HipConv3x3, _HipDeconv2x2, _HipSepHeadOut

    torch.manual_seed(21)
    torch.backends.cudnn.deterministic = True
    det = models.build_pillarnext_b(PC_RANGE, VOXEL, tasks=TASKS, with_iou_head=True).cuda().eval()
    random_bn_(det, 22)
    assert [int(v) for v in det.reader.grid_size] == [NY, NX]
    fused = models.FusedPillarNeXt(det, dtype=dtype).cuda().eval()
    assert all(isinstance(m, _HipConv3x3) for mods in fused.stages for m in mods) and fused.sparse_ws and fused.tile_lists
    assert isinstance(fused.shared, _HipConv3x3) and all(isinstance(m, _HipDeconv2x2) for m in fused.task_deblock)
    assert all(isinstance(m, _HipSepHeadOut) for m in list(fused.task_conv2) + list(fused.lazy_conv2)) and fused.lazy_head
    for blk in det.backbone.blocks:
        c = blk[0].conv.out_channels
        assert ops.conv_tile_rows(c, c, 1) == TILE_H[c]
    frames = [_frame(*f) for f in FRAMES]
    empties = [next(b for b, (kind, _) in enumerate(kinds) if kind == "empty") for _, kinds in FRAMES]
    ck, rec = Checker(dtype), Recorder(fused)
    name = {torch.bfloat16: "bf16", torch.float16: "f16"}[dtype]
    with torch.no_grad():
        runs = []
        for fi, pts in enumerate(frames):
            tag = f"{name} frame {fi}"
            dense, lazy = _run(fused, rec, pts, False, monkeypatch), _run(fused, rec, pts, True, monkeypatch)
            runs.append(dense)
            with monkeypatch.context() as mp:
                _block_kernels(mp)
                reach = _check_trunk(ck, tag, det, fused, dense)
                _check_reach(ck, tag, reach, empties[fi])
                _check_head(ck, tag + " dense head", det, fused, dense, False)
                _check_head(ck, tag + " lazy head", det, fused, lazy, True)
                _same_recordings(ck, tag + " lazy run == dense run up to the head", dense, lazy, ("stage", "mapping", "pre", "shared", "deblock"))
            if fi == 0:
                ws = [k for k in fused._ws if isinstance(k[0], int)]
                tl = [k for k in fused._ws if k[0] == "tiles"]
                ck.need(len(ws) == 4 and len(tl) == 4 and all(len(fused._ws[k]) == 3 for k in ws), tag, "stage workspaces / tile lists", list(fused._ws))
        a0, a1 = (int(r.occ.sum()) for r in runs)
        ck.need(0 < a1 < a0, "the second frame's active set is not the smaller one", a0, a1)
        fused.sparse_ws = False
        plainws = _run(fused, rec, frames[1], False, monkeypatch)
        fused.sparse_ws = True
        _same_recordings(ck, f"{name} frame 1 without the stage workspaces", runs[1], plainws)
        ck.need(all(biteq(a, b) for a, b in zip(runs[1].packed, plainws.packed)), name, "packed maps without the stage workspaces")
        # the path bench.py runs (launch plans, a second instance, no hook, no tap) against the one just verified
        rec.remove()
        fused.use_plan = False
        planned = models.FusedPillarNeXt(det, dtype=dtype).cuda().eval()
        assert planned.use_plan and planned._plan_ok() and planned._head_plan_ok() and planned.lazy_head
        total = 0
        for fi, pts in enumerate(frames):
            ex = {"points": pts, "batch_size": B, "token": [f"f{fi}s{b}" for b in range(B)]}
            want, got = fused(dict(ex)), planned(dict(ex))
            ck.need(set(want) == set(got) == set(ex["token"]), name, "tokens")
            for k in want:
                total += len(want[k]["scores"])
                ck.need(all(torch.equal(want[k][f], got[k][f]) for f in ("scores", "box3d_lidar", "label_preds")), name, k, "planned detections differ")
        ck.need(("plan_bb", B, frames[0].device) in planned._ws and any(k[0] == "plan_head" for k in planned._ws), name, "no launch plan was built")
        ck.need(total > 0, name, "no detection to compare")
        print(f"[{name}] planned path == verified path on {total} detections")
    ck.done(name)
