"""The fused inference graph: FusedPillarNeXt re-expresses a built SingleStageDetector for eval (BatchNorm folded into the convolutions, epilogues
fused, the branches of a SepHead merged into two convolutions, the regression branches evaluated lazily at the decoder's candidates) and walks its
launch schedule launch by launch or through launch plans (plan.py).  It duck-types the detector it is given and names no module class of models.py.
Every kernel call is an attribute lookup on the ops module at call time (ops.conv3x3_masked(...)): tests replace those attributes with recording fakes."""
import weakref

import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from .plan import Dyn, LaunchPlan
from .switches import on


def _params_version(module):
    """Changes whenever a parameter or buffer of the module is replaced or written in place: the key of every cache of folded / packed weights."""
    return tuple((p.data_ptr(), p._version) for p in list(module.parameters()) + list(module.buffers()))


def _fold_bn(weight, bn, conv_bias=None, transposed=False):
    """Fold an eval-mode BatchNorm into the preceding conv: returns (weight', bias') in fp32."""
    w = weight.detach().float()
    a = bn.weight.detach().float() * torch.rsqrt(bn.running_var.detach().float() + bn.eps)
    shape = (1, -1, 1, 1) if transposed else (-1, 1, 1, 1)
    b0 = conv_bias.detach().float() if conv_bias is not None else torch.zeros_like(a)
    return w * a.view(shape), (b0 - bn.running_mean.detach().float()) * a + bn.bias.detach().float()


def fold_aspp(nk):
    """ASPPNeck (eval) after pre_conv as ONE sum of four dilated convolutions of x: returns ([w_d (O,C,3,3) for d in 1,6,12,18], shift (O,))
    with  relu(sum_d conv_d(x, w_d) + shift) == post_conv(cat(x, conv1x1(x), conv_d(x, W)...))  (aspp.py:19-32).  The identity and
    1x1 branches are 1x1 convolutions of x, i.e. centre taps: they are added to the centre tap of the dilation-1 kernel."""
    wp, bp = _fold_bn(nk.post_conv.conv.conv.weight, nk.post_conv.norm)
    C = nk.weight.shape[0]
    P = wp.detach().float().reshape(wp.shape[0], 6, C)                       # (out, branch, mid): column blocks of the post weight
    w1 = nk.conv1x1.weight.detach().float().reshape(C, C)
    ws = nk.weight.detach().float()
    wds = [torch.einsum("om,mikl->oikl", P[:, 2 + k], ws) for k in range(4)]
    wds[0][:, :, 1, 1] += P[:, 0] + P[:, 1] @ w1
    return wds, bp.float()


class _FusedConv(nn.Module):
    """conv (BN folded, no bias inside MIOpen) + ONE HIP epilogue pass: [relu](y + b [+ res]) * mask."""

    def __init__(self, weight, bias, stride=1, padding=0, dilation=1, relu=True, transposed=False, dtype=torch.bfloat16):
        super().__init__()
        self.register_buffer("weight", weight.to(dtype).contiguous(memory_format=torch.channels_last) if weight.dim() == 4 else weight.to(dtype))
        self.register_buffer("bias", bias.float().contiguous())
        self.stride, self.padding, self.dilation, self.relu, self.transposed = stride, padding, dilation, relu, transposed

    def forward(self, x, mask=None, residual=None, post_residual=None):
        """post_residual: added AFTER this layer's ReLU (relu mode 2 of the epilogue) instead of before it."""
        if self.transposed:
            y = F.conv_transpose2d(x, self.weight, None, self.stride, self.padding)
        else:
            y = F.conv2d(x, self.weight, None, self.stride, self.padding, self.dilation)
        if not y.is_contiguous(memory_format=torch.channels_last):
            y = y.contiguous(memory_format=torch.channels_last)
        if post_residual is not None:
            return ops.bias_act_mask_(y, self.bias, mask, post_residual, 2 if self.relu else 0)
        return ops.bias_act_mask_(y, self.bias, mask, residual, self.relu)


class _HipConv3x3(nn.Module):
    """3x3 masked conv + folded BN + [residual] + ReLU + mask in ONE HIP kernel (csrc/conv3x3.hip) -- no MIOpen, no epilogue pass."""

    def __init__(self, weight, bias, stride=1, dtype=torch.bfloat16):
        super().__init__()
        self.cout, self.cin, self.stride = weight.shape[0], weight.shape[1], int(stride)
        self.register_buffer("wfrag", ops.conv3x3_pack_weights(weight, dtype=dtype))
        self.register_buffer("bias", bias.float().contiguous())

    def forward(self, x, mask=None, residual=None, out=None, tiles=None, plan=None):
        """plan: a LaunchPlan that records the call instead of issuing it (the same arguments; `out` says where it will write)."""
        call = ops.conv3x3_masked if plan is None else plan.conv3x3
        return call(x, self.wfrag, self.bias, self.cout, self.stride, mask, residual, True, out=out, tiles=tiles if self.stride == 1 else None)


class _HipDeconv2x2(nn.Module):
    """ConvTranspose2d(k=2, s=2) + folded BN + ReLU in ONE HIP kernel (csrc/sephead.h::k_deconv2x2_64): the SepHead deblock."""

    def __init__(self, weight, bias, relu=True, dtype=torch.bfloat16):
        super().__init__()
        self.cout, self.relu = weight.shape[1], relu
        self.register_buffer("wfrag", ops.deconv2x2_pack_weights(weight, dtype=dtype))
        self.register_buffer("bias", bias.float().contiguous())

    def forward(self, x, mask=None, residual=None, out=None, plan=None):
        if plan is None:
            return ops.deconv2x2(x, self.wfrag, self.bias, self.cout, self.relu)
        return plan.deconv2x2(x, self.wfrag, self.bias, self.cout, out, self.relu)


class _HipSepHeadOut(nn.Module):
    """Last 3x3 conv of all SepHead branches of a task as ONE HIP kernel over the block-diagonal weight (csrc/sephead.h::k_sephead_out)."""

    def __init__(self, weight, bias, dtype=torch.bfloat16):
        super().__init__()
        self.cout = weight.shape[0]
        self.register_buffer("wfrag", ops.sephead_pack_weights(weight, dtype=dtype))
        self.register_buffer("bias", bias.float().contiguous())

    def forward(self, x, mask=None, residual=None, out=None, plan=None):
        if plan is None:
            return ops.sephead_out(x, self.wfrag, self.bias)
        return plan.sephead_out(x, self.wfrag, self.bias, out)


def _backbone_conv(weight, bias, stride, padding, dtype, hip_conv):
    co, ci, kh, kw = weight.shape
    shapes = ops.CONV3X3_SHAPES_S1 if stride == 1 else ops.CONV3X3_SHAPES_S2
    if hip_conv and dtype in ops._HALF and (kh, kw) == (3, 3) and padding == 1 and (ci, co) in shapes and stride in (1, 2):
        return _HipConv3x3(weight, bias, stride, dtype=dtype)
    return _FusedConv(weight, bias, stride, padding, dtype=dtype)


# ---------------------------------------------------------------------------------------------- one task's head weights
def _fold_branches(task, names):
    """The branches `names` of a SepHead (conv-bn-relu-conv each), the BatchNorm folded into the first convolution: per branch
    (w1s (hc,64,3,3), b1s (hc), w2s (k,hc,3,3), b2s (k), outs k), fp32."""
    w1s, b1s, w2s, b2s, outs = [], [], [], [], []
    for nme in names:
        fc = getattr(task, nme)
        assert len(fc) == 4, "merged head expects conv-bn-relu-conv branches"
        w1, b1 = _fold_bn(fc[0].weight, fc[1], fc[0].bias)
        w1s.append(w1)
        b1s.append(b1)
        w2s.append(fc[3].weight.detach().float())
        b2s.append(fc[3].bias.detach().float())
        outs.append(fc[3].weight.shape[0])
    return w1s, b1s, w2s, b2s, outs


def _block_diag(w2s, b2s, branches, rows):
    """The second convolutions of `branches` as ONE 3x3 convolution over their concatenated hidden channels, zero-padded to `rows` outputs:
    (W (rows, hc * len(branches), 3, 3), B (rows)), block-diagonal -- a branch only sees its own hc channels."""
    hc = w2s[0].shape[1]
    W = torch.zeros((rows, hc * len(branches), 3, 3), dtype=torch.float32, device=w2s[0].device)
    B = torch.zeros((rows,), dtype=torch.float32, device=w2s[0].device)
    o = 0
    for q, j in enumerate(branches):
        k = w2s[j].shape[0]
        W[o:o + k, q * hc:(q + 1) * hc] = w2s[j]
        B[o:o + k] = b2s[j]
        o += k
    return W, B


def _lazy_matrices(w1s, b1s, w2s, b2s, outs, dtype):
    """The five regression branches as matrices over (tap, channel) -- conv1 (576 -> 320), conv2 (9 positions x 320 -> 10, block-diagonal) -- and as the
    packed weights of the lazy kernels: the buffers (suffix, tensor) of one task in registration order, w1, b1, w2, b2, wf1, w2c."""
    hc, dev = w1s[0].shape[0], w1s[0].device
    W1z = torch.cat(w1s[:5], 0)                               # (320, 64, 3, 3)
    w1m = W1z.permute(2, 3, 1, 0).reshape(9 * hc, 5 * hc)     # rows (ky, kx, cin)
    w2m = torch.zeros((9 * 5 * hc, 10), dtype=torch.float32, device=dev)
    b2z = torch.zeros((10,), dtype=torch.float32, device=dev)
    o = 0
    for j in range(5):
        w2 = w2s[j]                                          # (k, 64, 3, 3)
        for pos in range(9):
            w2m[pos * 5 * hc + j * hc: pos * 5 * hc + (j + 1) * hc, o:o + outs[j]] = w2[:, :, pos // 3, pos % 3].t()
        b2z[o:o + outs[j]] = b2s[j]
        o += outs[j]
    w2 = w2m.to(dtype).float().contiguous()                   # the dense kernels hold W2 in the element type
    return [("w1", w1m.to(dtype).contiguous()), ("b1", torch.cat(b1s[:5]).float().contiguous()), ("w2", w2), ("b2", b2z),
            ("wf1", ops.conv3x3_pack_weights(W1z, dtype=dtype)), ("w2c", ops.sephead_lazy_pack_w2(w2))]


class LazyTask:
    """What the lazy head hands the decoder for one task: the dense [iou] hm map and the deblocked features the regression branches
    are evaluated on at the selected candidates."""

    def __init__(self, dense, up):
        self.dense, self.up = dense, up


class _DeferredDecode:
    """The decoder launch of one frame batch, held back until the next batch's reader has been enqueued (FusedPillarNeXt.forward_async with
    decode_on_side_stream) or until somebody asks for the result.  Behaves like the decode.PendingDetections it turns into."""

    def __init__(self, model, packed, tokens):
        self.model, self.packed, self.tokens = model, packed, tokens
        self.head_done = torch.cuda.Event()
        self.head_done.record()                       # the head of this batch, on the caller's stream
        self.launched, self.pend = False, None

    def launch(self, behind_reader=False):
        if self.launched:
            return
        self.launched = True
        m = self.model
        main = torch.cuda.current_stream()
        side = m.__dict__.get("_decode_stream")
        if side is None or side.device != main.device:
            side = m.__dict__["_decode_stream"] = torch.cuda.Stream(device=main.device)
        side.wait_event(self.head_done)
        if behind_reader:                             # called right after the next batch's reader was enqueued on `main`
            ev = torch.cuda.Event()
            ev.record(main)
            side.wait_event(ev)
        with torch.cuda.stream(side):
            self.pend = m.launch_decode(self.packed, self.tokens)
        for p in self.packed:   # allocated on the main stream, consumed on the side stream: the caching allocator must not hand them out before that work ran
            p.dense.record_stream(side), p.up.record_stream(side)
        self.packed = None
        ref = m.__dict__.get("_deferred")
        if ref is not None and ref() is self:
            m.__dict__["_deferred"] = None

    def result(self):
        self.launch()
        return self.pend.result()

    def __getattr__(self, name):                      # flag_h, event, done, ... of the PendingDetections
        if name in ("pend", "launched", "packed", "model", "tokens", "head_done"):
            raise AttributeError(name)
        self.launch()
        return getattr(self.pend, name)


class FusedPillarNeXt(nn.Module):
    """Inference-only re-expression of SingleStageDetector (eval BN folded, epilogues fused, the 6-7 SepHead branches of a
    task merged into two convolutions).  Mathematically the same network; weights come from the trained modules.
    One instance drives ONE stream: the stage workspaces, the launch plans' canvas and the decoder's scratch are persistent and reused
    from call to call in stream order (a second stream needs a second instance).  forward_async additionally owns one internal side stream
    for the decoder (decode_on_side_stream); everything it returns is ordered for the caller by PendingDetections.result()."""

    def __init__(self, det, dtype=torch.bfloat16, hip_conv=None):
        super().__init__()
        if hip_conv is None:
            hip_conv = on("PNX_HIP_CONV")
        hip = bool(hip_conv) and dtype in ops._HALF
        self._ws = {}
        # launch plans (plan.py / pnx_enqueue): the backbone and the head as one C call each; PNX_PLAN=0 issues every launch from Python
        self.use_plan = on("PNX_PLAN")
        self.sparse_ws = on("PNX_SPARSE_WS")
        self.tile_lists = on("PNX_TILE_LISTS")
        # the decoder on its own stream, launched behind the NEXT batch's reader (forward_async / _DeferredDecode): +4.8 % frames/s in bench.py's
        # serving loop with the reader's in-loop time unchanged (round 5); PNX_DECODE_STREAM=0: everything on one stream
        self.decode_on_side_stream = on("PNX_DECODE_STREAM")
        self.reader = det.reader
        self.post_processing = det.post_processing
        self.head_ref = det.head  # predict() / rectifier / class bookkeeping
        self.dtype = dtype
        self._decoder = None
        bb = det.backbone
        self.stages = nn.ModuleList()
        self.stage_meta = []
        for blk in bb.blocks:
            mods = nn.ModuleList()
            first = blk[0]
            w, b = _fold_bn(first.conv.weight, first.norm)
            mods.append(_backbone_conv(w, b, first.stride, first.kernel_size // 2, dtype, hip_conv))
            for rb in list(blk)[1:]:
                w1, b1 = _fold_bn(rb.block1.conv.weight, rb.block1.norm)
                w2, b2 = _fold_bn(rb.conv2.weight, rb.norm2)
                mods.append(_backbone_conv(w1, b1, 1, rb.block1.kernel_size // 2, dtype, hip_conv))
                mods.append(_backbone_conv(w2, b2, 1, rb.conv2.kernel_size[0] // 2, dtype, hip_conv))
            self.stages.append(mods)
            self.stage_meta.append((first.stride, first.subm))
        w, b = _fold_bn(bb.mapping[0].weight, bb.mapping[1])
        self.mapping = _FusedConv(w, b, 1, 0, dtype=dtype)
        nk = det.neck
        self.pre1 = _FusedConv(*_fold_bn(nk.pre_conv.block1.conv.conv.weight, nk.pre_conv.block1.norm), 1, 1, dtype=dtype)
        self.pre2 = _FusedConv(*_fold_bn(nk.pre_conv.block2.conv.conv.weight, nk.pre_conv.block2.norm), 1, 1, dtype=dtype)
        # ASPP (aspp.py:19-32): the identity, the 1x1 branch and the four dilated branches have no BN/activation of their own and
        # post_conv is a 1x1 over their concat, so it distributes over the branches:
        #     post(cat(x, conv1x1(x), conv_d(x, Ws)...)) = conv1x1(x, P0 + P1.W1) + sum_d conv_d(x, P_d.Ws)
        # (P_k = the k-th 256-column block of the BN-folded post weight), and the 1x1 term is a centre tap, added to the dilation-1
        # kernel.  The 1536-channel concat, the 1536 -> 256 GEMM and the 1x1 branch disappear; the four partial results are summed
        # in fp32 by one pass (pnx_sum_bias_act) that also applies the folded-BN shift + ReLU.
        wds, bp = fold_aspp(nk)
        for k, wd in enumerate(wds):
            self.register_buffer(f"aspp_w{k}", wd.to(dtype).contiguous(memory_format=torch.channels_last))
        self.register_buffer("aspp_bias", bp.float().contiguous())
        hd = det.head
        sc = hd.shared_conv[0]
        self.shared = _backbone_conv(*_fold_bn(sc.weight, hd.shared_conv[1], sc.bias), sc.stride[0], sc.padding[0], dtype, hip_conv)
        self.task_deblock, self.task_conv1, self.task_conv2 = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        self.task_split, self.task_chans = [], []
        # Lazy head (PNX_HEAD_LAZY, default on): per task only the class (and iou) branches run over the whole map; the five regression
        # branches (reg, height, dim, rot, vel = 5/6 of the head's convolution work and its 9.6 GB/step intermediate) are evaluated
        # at the <= pre_max candidates per (sample, class) that the decoder selects -- what CenterHead.predict does after the fact
        # (centerhead.py:341-363) done before the fact.
        self.lazy_head = hip and on("PNX_HEAD_LAZY")
        self.lazy_conv1, self.lazy_conv2 = nn.ModuleList(), nn.ModuleList()
        self._lazy_ok = []
        for ti, task in enumerate(hd.tasks):
            db = task.deblock
            w, b = _fold_bn(db.conv.conv.weight, db.norm, transposed=True)
            dc = db.conv.conv
            if hip and tuple(w.shape) == (64, 64, 2, 2) and tuple(dc.stride) == (2, 2) and tuple(dc.padding) == (0, 0):
                self.task_deblock.append(_HipDeconv2x2(w, b, dtype=dtype))
            else:
                self.task_deblock.append(_FusedConv(w, b, dc.stride, 0, transposed=True, dtype=dtype))
            names = list(task.heads.keys())
            w1s, b1s, w2s, b2s, outs = _fold_branches(task, names)
            hc, tot = w1s[0].shape[0], sum(outs)
            W1 = torch.cat(w1s, 0)                                   # (nh*hc, 64, 3, 3)
            hip_out = hip and hc == 64 and tot <= 16 and len(names) in (5, 6, 7)
            # k_sephead_out: 16 output channels (one MFMA M tile); the epilogue kernel wants channels % 8 == 0
            tot_p = 16 if hip_out else (tot + 7) // 8 * 8
            W2, B2 = _block_diag(w2s, b2s, range(len(names)), tot_p)
            if hip and (W1.shape[1], W1.shape[0]) in ops.CONV3X3_SHAPES_S1:
                self.task_conv1.append(_HipConv3x3(W1, torch.cat(b1s), 1, dtype=dtype))   # input tile staged once, reused for all 64-channel passes
            else:
                self.task_conv1.append(_FusedConv(W1, torch.cat(b1s), 1, 1, dtype=dtype))
            self.task_conv2.append(_HipSepHeadOut(W2, B2, dtype=dtype) if hip_out else _FusedConv(W2, B2, 1, 1, relu=False, dtype=dtype))
            self.task_chans.append(tot_p)
            self.task_split.append((names, outs))
            ok = (self.lazy_head and hip_out and names[:5] == ["reg", "height", "dim", "rot", "vel"] and outs[:5] == [2, 1, 3, 2, 2]
                  and names[5:] in (["hm"], ["iou", "hm"]))
            self._lazy_ok.append(ok)
            if ok:
                dn = range(5, len(names))                               # dense branches: [iou] hm
                self.lazy_conv1.append(_HipConv3x3(torch.cat([w1s[j] for j in dn], 0), torch.cat([b1s[j] for j in dn]), 1, dtype=dtype))
                self.lazy_conv2.append(_HipSepHeadOut(*_block_diag(w2s, b2s, dn, 16), dtype=dtype))
                for suffix, t in _lazy_matrices(w1s, b1s, w2s, b2s, outs, dtype):
                    self.register_buffer(f"lazy_{suffix}_{ti}", t)
            else:
                self.lazy_conv1.append(nn.Identity())
                self.lazy_conv2.append(nn.Identity())
        self.lazy_head = self.lazy_head and all(self._lazy_ok)

    @torch.no_grad()
    def forward_preds(self, points, batch_size, marks=None, packed_out=None, taps=None, lazy=None, after_reader=None):
        """packed_out: a list that receives, per task, the packed NHWC head output -- or, with the lazy head (lazy=None: the model's
        setting), a LazyTask (dense [iou] hm map + deblocked features) for launch_decode()."""
        def mark(name):
            if marks is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                marks.append((name, e))

        mark("start")
        planned = marks is None and taps is None and self._plan_ok()
        if planned:   # the reader writes the plan's persistent canvas / occupancy
            bb = self._backbone_plan(batch_size, points.device)
            canvas, occ = bb["canvas"], bb["occ"]
        else:
            ny, nx = (int(v) for v in self.reader.grid_size)
            canvas, occ = None, torch.empty((batch_size, ny, nx), dtype=torch.uint8, device=points.device)
        x = self.reader.forward_dense(points, batch_size, dtype=self.dtype, out=canvas, occupancy=occ)
        if after_reader is not None:
            after_reader()
        mark("reader")
        if planned:
            bb["plan"].run()
            x, mask = bb["out"], bb["mask"]
        else:
            x, mask = self._backbone(x, occ, mark=mark, taps=taps)
        x = self.mapping(x, mask)
        # BasicBlock (utils/conv.py): act(block2(block1(x)) + x) where block2 already ends in a ReLU, so the residual is added
        # AFTER that ReLU; both terms are >= 0, which makes the trailing act() the identity.
        x = self.pre2(self.pre1(x), post_residual=x)
        parts = [F.conv2d(x, getattr(self, f"aspp_w{k}"), None, 1, d, d) for k, d in enumerate((1, 6, 12, 18))]
        parts = [p if p.is_contiguous(memory_format=torch.channels_last) else p.contiguous(memory_format=torch.channels_last) for p in parts]
        x = ops.sum_bias_act(parts, self.aspp_bias, relu=True)
        mark("mapping+neck")
        if taps is not None:
            taps["neck"] = x
        lazy = packed_out is not None and self.lazy_head and (lazy is None or lazy)
        if planned and lazy and self._head_plan_ok():
            packed_out.extend(self._run_head_plan(x))
            return []
        preds = []
        for (t, up), (names, outs_n) in zip(self._head(x, lazy), self.task_split):
            if lazy:
                packed_out.append(LazyTask(t, up))
            elif packed_out is not None:
                packed_out.append(t)
            else:
                d, o = {}, 0
                for nme, k in zip(names, outs_n):
                    d[nme] = t[:, o:o + k]
                    o += k
                preds.append(d)
        mark("head")
        return preds

    # ------------------------------------------------------------------ the launch schedule: each section written once, issued launch by
    # launch (plan=None) or recorded into a plan.LaunchPlan (include/pnx.h: pnx_enqueue) that replays it with one C call per frame batch
    def _backbone(self, x, mask, plan=None, mark=lambda name: None, taps=None):
        """Canvas + occupancy -> (last stage's activation, its mask): per stage [mask_pool3,] tile list, entry convolution, residual blocks.
        Recorded into a plan, every mask, tile list and activation is a persistent buffer (the plan is only built when _plan_ok() holds)."""
        for si, (mods, (stride, subm)) in enumerate(zip(self.stages, self.stage_meta)):
            if not subm:
                mask = ops.mask_pool3(mask, stride) if plan is None else plan.mask_pool3(mask, ops.mask_pool3_out(mask, stride), stride)
            ws, k = self._stage_workspace(si, mods, mask), 0
            tiles = self._stage_tiles(si, mods, mask, ws, plan)

            def run(m, inp, res=None):
                nonlocal k
                if ws is None or not isinstance(m, _HipConv3x3):   # launch by launch only: MIOpen + epilogue, or HIP kernels into fresh tensors
                    assert plan is None
                    return m(inp, mask, residual=res)
                k += 1                                  # x, y, out of a block sit in three different buffers
                return m(inp, mask, residual=res, out=ws[(k - 1) % 3], tiles=tiles, plan=plan)

            x = run(mods[0], x)
            for j in range(1, len(mods), 2):
                y = run(mods[j], x)
                x = run(mods[j + 1], y, x)
            mark(f"backbone.stage{si}")
            if taps is not None:
                taps[f"stage{si}"] = x
        return x, mask

    def _head(self, x, lazy, plan=None):
        """Neck output -> per task (map, deblocked features): shared conv, then deblock -> conv1 -> conv2 of the dense [iou] hm branches (lazy) or
        of all branches.  Recorded into a plan (lazy, and only when _head_plan_ok() holds), x, the deblocked and the dense maps are the slots "x",
        "up{ti}", "dense{ti}" bound per step; the intermediates are persistent, one per width: the tasks run one after the other on the stream."""
        c1s, c2s = (self.lazy_conv1, self.lazy_conv2) if lazy else (self.task_conv1, self.task_conv2)

        def run(m, inp, out):
            return m(inp) if plan is None else m(inp, out=out, plan=plan)

        o_sh, outs = None, [(None, None, None)] * len(c1s)
        if plan is not None:   # where the recorded launches write; issued at once, every launch allocates its own output
            def new(c, s):
                return torch.empty((x.shape[0], c, s * x.shape[2], s * x.shape[3]), dtype=self.dtype, device=x.device, memory_format=torch.channels_last)

            o_sh, mids = (new(self.shared.cout, 1), None), {c1.cout: new(c1.cout, 2) for c1 in c1s}
            outs = [(Dyn(f"up{ti}", new(64, 2)), (mids[c1.cout], None), Dyn(f"dense{ti}", new(16, 2))) for ti, c1 in enumerate(c1s)]
            x = Dyn("x", x)
        sh = run(self.shared, x, o_sh)
        for db, c1, c2, (o_up, o_mid, o_map) in zip(self.task_deblock, c1s, c2s, outs):
            up = run(db, sh, o_up)
            yield run(c2, run(c1, up, o_mid), o_map), up

    def _plan_ok(self):
        return (self.use_plan and self.sparse_ws and self.tile_lists and self.dtype in ops._HALF and not self.reader.training
                and self.reader._fused_supported() and all(isinstance(m, _HipConv3x3) for mods in self.stages for m in mods))

    def _head_plan_ok(self):
        return isinstance(self.shared, _HipConv3x3) and all(isinstance(d, _HipDeconv2x2) for d in self.task_deblock)

    def _backbone_plan(self, B, dev):
        """The backbone of a B-frame batch as ONE pnx_enqueue call, from the persistent canvas / occupancy the reader is to write."""
        key = ("plan_bb", B, dev)
        st = self._ws.get(key)
        wkey = tuple(t.data_ptr() for mods in self.stages for m in mods for t in (m.wfrag, m.bias))   # .to() / a reload / a re-fold moves or replaces them
        if st is not None and st["weights_at"] == wkey:
            return st
        ny, nx = (int(v) for v in self.reader.grid_size)
        canvas = torch.empty((B, 64, ny, nx), dtype=self.dtype, device=dev, memory_format=torch.channels_last)
        occ = torch.empty((B, ny, nx), dtype=torch.uint8, device=dev)
        plan = LaunchPlan()
        x, mask = self._backbone(canvas, occ, plan)
        st = self._ws[key] = {"canvas": canvas, "occ": occ, "plan": plan.freeze(), "out": x, "mask": mask, "weights_at": wkey}
        return st

    def _head_plan(self, x):
        """The lazy head for maps like x as ONE pnx_enqueue call: built once per shape (no launch, no GPU needed), bound and run by _run_head_plan."""
        key = ("plan_head", *x.shape[:1], *x.shape[2:], x.device, self.shared.wfrag.data_ptr())   # the weights' address: .to() after the plan was built moves them
        if key not in self._ws:
            plan = LaunchPlan()
            list(self._head(x, True, plan))
            self._ws[key] = plan.freeze()
        return self._ws[key]

    def _run_head_plan(self, x):
        """The deblocked maps and the dense maps are fresh tensors per step (the decoder's fallback may read them after later steps were enqueued)."""
        st = self._head_plan(x)
        B, _, H, W = x.shape
        st.bind("x", x)
        tasks = []
        for ti in range(len(self.task_deblock)):
            up, dense = (torch.empty((B, c, 2 * H, 2 * W), dtype=self.dtype, device=x.device, memory_format=torch.channels_last) for c in (64, 16))
            st.bind(f"up{ti}", up)
            st.bind(f"dense{ti}", dense)
            tasks.append(LazyTask(dense, up))
        st.run()
        return tasks

    def _stage_workspace(self, si, mods, mask):
        """Three persistent (activation, row_dirty) pairs per backbone stage for its HIP convolutions: they then touch only the row
        segments that hold (or held, one frame ago) active sites -- ops.conv3x3_workspace / pnx.h row_dirty."""
        if not self.sparse_ws or not any(isinstance(m, _HipConv3x3) for m in mods):
            return None
        B, H, W = mask.shape
        key = (si, B, H, W, mask.device)
        if key not in self._ws:
            cout = next(m.cout for m in mods if isinstance(m, _HipConv3x3))
            self._ws[key] = [ops.conv3x3_workspace(B, cout, H, W, mask.device, self.dtype) for _ in range(3)]
        return self._ws[key]

    def _stage_tiles(self, si, mods, mask, ws, plan=None):
        """Tile list of a stage (ops.conv_tile_list): the submanifold blocks share the stage's mask, so the tiles with an active site
        or a stale row in one of the stage's three buffers are listed once and every stride-1 convolution walks the list."""
        if ws is None or not self.tile_lists:
            return None
        m = next((m for m in mods if isinstance(m, _HipConv3x3) and m.stride == 1), None)
        rows = ops.conv_tile_rows(m.cin, m.cout, 1) if m is not None else 0
        if rows <= 0:
            return None
        key = ("tiles", si) + tuple(mask.shape) + (mask.device,)
        buf, dirties = self._ws.get(key), [w[1] for w in ws]
        list_tiles = ops.conv_tile_list if plan is None else plan.tile_list
        buf = self._ws[key] = list_tiles(mask, dirties, rows, buf if plan is None else ops.conv_tile_buffers(mask, rows, buf))
        return buf

    def _lazy_tasks(self, ups):
        """What ops.sephead_lazy / the fused lazy decoder take: per task (deblocked map, packed regression-branch weights), and the task of every class."""
        tasks = [(up, *(getattr(self, f"lazy_{n}_{ti}") for n in ("wf1", "b1", "w2c", "b2"))) for ti, up in enumerate(ups)]
        return tasks, [ti for ti, (names, outs) in enumerate(self.task_split) for _ in range(outs[-1])]

    def decoder(self):
        if self._decoder is None:
            from .decode import PackedDecoder

            hd = self.head_ref
            chans = list(self.task_chans)
            # decode.hip reads the packed channels as reg(2) height(1) dim(3) rot(2) vel(2) [iou(1)] hm(ncls): the order of the
            # YAML's common_heads dict decides the packing, so check it instead of decoding the wrong channels silently
            want = ["reg", "height", "dim", "rot", "vel"] + (["iou"] if hd.with_iou else []) + ["hm"]
            sizes = {"reg": 2, "height": 1, "dim": 3, "rot": 2, "vel": 2, "iou": 1}
            for (names, outs), ncls in zip(self.task_split, hd.num_classes):
                if list(names) != want or any(o != sizes.get(n, ncls) for n, o in zip(names, outs)) or ncls > 4:
                    raise ops.PnxError(f"fused decoder needs head branches {want} with sizes 2,1,3,2,2[,1],ncls<=4; got {list(zip(names, outs))} -- "
                                       "use SingleStageDetector (CenterHead.predict) for this head layout")
            self._decoder = PackedDecoder(hd.num_classes, hd.rectifier, self.post_processing, hd.with_iou, chans)
        return self._decoder

    @staticmethod
    def _lazy_eval_in_torch():   # read on every call: tests flip it between two runs of one model
        return on("PNX_HEAD_LAZY_TORCH")

    @torch.no_grad()
    def lazy_eval(self, ups, local, seg_len, valid, segs):
        """The five regression branches of every task at the candidate cells (local (S, pre_max) = b*H*W + cell inside the list's task map,
        lists s = sample * nc_total + class) of the deblocked maps ups[t] (B,64,H,W channels_last bf16): conv3x3 (64 -> 5*64) + folded BN +
        ReLU at the 3 x 3 neighbours of every cell, rounded to bf16 like the dense kernel's intermediate, then the block-diagonal 3x3 conv
        (-> 10) at the cell; zero padding at the map border.  Returns (S, pre_max, 10) fp32 in the order reg 2, height 1, dim 3, rot 2,
        vel 2, rounded to bf16 like the dense output.  One HIP launch (ops.sephead_lazy); PNX_HEAD_LAZY_TORCH=1 runs the torch statement
        of the same arithmetic below instead (tests compare the two)."""
        if not self._lazy_eval_in_torch():
            tasks, class_task = self._lazy_tasks(ups)
            return ops.sephead_lazy(tasks, class_task, ups[0].shape[0], local, seg_len, local.shape[1])
        cand = torch.zeros((*local.shape, 10), dtype=torch.float32, device=local.device)
        for ti, st in enumerate(segs):
            cand[st] = self._lazy_eval_torch(ti, ups[ti], local[st].reshape(-1), valid[st].reshape(-1)).reshape(len(st), local.shape[1], 10)
        return cand

    def _lazy_eval_torch(self, ti, up, local, valid):
        B, C, H, W = up.shape
        n = local.shape[0]
        upf = up.permute(0, 2, 3, 1).reshape(B * H * W, C)
        local = torch.where(valid, local, torch.zeros_like(local))
        b, cell = local // (H * W), local % (H * W)
        y, x = cell // W, cell % W
        d = torch.arange(-2, 3, device=up.device)
        yy, xx = y[:, None] + d[None, :], x[:, None] + d[None, :]
        vy, vx = (yy >= 0) & (yy < H), (xx >= 0) & (xx < W)
        idx = (b[:, None, None] * H + yy.clamp(0, H - 1)[:, :, None]) * W + xx.clamp(0, W - 1)[:, None, :]
        patch = upf[idx.reshape(-1)].reshape(n, 5, 5, C) * (vy[:, :, None] & vx[:, None, :])[..., None].to(up.dtype)
        cols = patch.unfold(1, 3, 1).unfold(2, 3, 1).permute(0, 1, 2, 4, 5, 3).reshape(n * 9, 9 * C)
        t1 = torch.relu(cols.float() @ getattr(self, f"lazy_w1_{ti}").float() + getattr(self, f"lazy_b1_{ti}"))
        inside = (vy[:, 1:4, None] & vx[:, None, 1:4]).reshape(n * 9, 1)
        t1 = (t1 * inside).to(up.dtype).float().reshape(n, -1)
        out = t1 @ getattr(self, f"lazy_w2_{ti}") + getattr(self, f"lazy_b2_{ti}")
        return out.to(up.dtype).float() * valid[:, None]

    @torch.no_grad()
    def forward_async(self, example):
        """Enqueue the whole frame batch (reader -> ... -> NMS -> D2H copy) and return a decode.PendingDetections."""
        ref = self.__dict__.get("_deferred")    # the previous batch's decoder, if nobody asked for its result yet -- held by WEAK reference: a handle the
        prev = ref() if ref is not None else None  # caller dropped is not launched at all, and its ~1.2 GB of deblocked maps go back to the allocator at once
        packed = []
        self.forward_preds(example["points"], example["batch_size"], packed_out=packed,
                           after_reader=(lambda: prev.launch(behind_reader=True)) if prev is not None and not prev.launched else None)
        if not (self.decode_on_side_stream and packed and isinstance(packed[0], LazyTask)):
            return self.launch_decode(packed, example.get("token"))
        # The decoder (keys, radix select, candidate evaluation, boxes, NMS, gather, D2H) is a chain of small latency-bound launches.  On its own
        # stream, and started only once the NEXT batch's reader is through (so that the HBM-bound reader keeps the GPU to itself), it runs beside
        # that batch's convolutions instead of in front of them.  It reads only this step's fresh tensors (dense [iou] hm maps, deblocked maps) and
        # constants; its scratch is per stream (decode.PackedDecoder).  Nobody enqueues a next batch: result() launches it at once.
        d = _DeferredDecode(self, packed, example.get("token"))
        self.__dict__["_deferred"] = weakref.ref(d)
        return d

    def __getstate__(self):   # copy.deepcopy / torch.save of the module: the side stream and the pending decoder are per-process launch state, not model state
        st = dict(self.__dict__)
        for k in ("_decode_stream", "_deferred"):
            st.pop(k, None)
        st["_decoder"] = None
        st["_ws"] = {}
        return st

    def launch_decode(self, packed, tokens=None):
        if not (packed and isinstance(packed[0], LazyTask)):
            return self.decoder().launch(packed, tokens)
        ups = [p.up for p in packed]

        def dense_path():  # the exact fallback (decode.PendingDetections.result): every branch over the whole map
            return self.decoder().launch([c2(c1(u)) for u, c1, c2 in zip(ups, self.task_conv1, self.task_conv2)], tokens)

        dec = self.decoder()
        if self.use_plan and dec.selection == "topk" and not self._lazy_eval_in_torch():
            tasks, class_task = self._lazy_tasks(ups)
            return dec.launch_lazy_fused([p.dense for p in packed], tasks, class_task, tokens, dense_path)
        return dec.launch_lazy([p.dense for p in packed], lambda *a: self.lazy_eval(ups, *a), tokens, dense_path)

    @staticmethod
    def detections(outputs):
        det = {}
        for o in outputs:
            tok = o.pop("token")
            det[tok] = o  # already on the host
        return det

    @torch.no_grad()
    def forward(self, example):
        return self.detections(self.forward_async(example).result())
