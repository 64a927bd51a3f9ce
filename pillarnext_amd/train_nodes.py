"""The training graph's HIP autograd nodes and the helpers that route a layer to them.  The modules of models.py (and the multi-view reader's
blocks) call masked_conv / masked_bn_act in the backbone, x3_conv / dense_bn_act / smallk_conv in the neck and the head; each helper decides from
the layer, the tensors and the switches (switches.py, read on every call) whether the product's kernel serves the call, and hands the module
itself (MIOpen) the rest.  Every kernel is reached through its checked wrapper in ops.py."""
import contextlib
import threading

import torch
import torch.nn.functional as F
from torch import nn

from . import dist_utils, ops
from .switches import on, train_f32_pieces


_CKPT = threading.local()


@contextlib.contextmanager
def _ckpt_phase(phase):
    prev = getattr(_CKPT, "phase", None)
    _CKPT.phase = phase
    try:
        yield
    finally:
        _CKPT.phase = prev


def checkpoint_contexts():
    """context_fn of torch.utils.checkpoint.checkpoint(..., use_reentrant=False) for a region that holds _MaskedBNActFn nodes: tells the node whether it
    runs in the region's forward or in its recomputation (which happens on the autograd engine's thread: the flag is per thread)."""
    return _ckpt_phase("forward"), _ckpt_phase("recompute")


class _MaskedBNActFn(torch.autograd.Function):
    """y = relu(BN_active_sites(x) [+ residual]) * mask in ONE autograd node (train mode).  The module-by-module form keeps ~6 full-size
    fp32 tensors per layer alive for the backward (x.float(), the masked products, the normalised map, the ReLU output ...); this node
    keeps x (in its own dtype), the residual (the block's input, alive anyway) and two per-channel vectors, and recomputes the rest:
    the C2 x 4-frame training step went from 106 to 50.5 GiB (profiles/r03_train_step_c2_b4_fp32.log).  SyncBatchNorm mode all-reduces [sum x, count], [sum (x-mu)^2]
    forward (the HIP path: [sum x | sum x^2 | count] in fp64, once) and [sum g, sum g*xhat] backward over the ACTIVE sites of the global batch
    (dist_utils.all_reduce_sum, looked up at call time); dgamma / dbeta stay the local sums."""

    @staticmethod
    def _hip_ok(x, residual, weight=None, bias=None, norm=None):
        """The fused HIP kernels (csrc/masked_bn.hip) take channels_last bf16 / fp32 CUDA maps with 8..256 channels (fp32 parameters and buffers)."""
        C = x.shape[1]
        f32 = all(t is None or (t.dtype == torch.float32 and t.is_contiguous()) for t in (weight, bias))
        if norm is not None:
            f32 = f32 and norm.momentum is not None and norm.running_mean is not None and norm.running_mean.dtype == torch.float32 \
                and norm.running_var.dtype == torch.float32
        return (x.is_cuda and x.dim() == 4 and x.dtype in (torch.bfloat16, torch.float32) and C in ops.MASKED_BN_CHANNELS and f32
                and x.is_contiguous(memory_format=torch.channels_last) and on("PNX_MASKED_BN_HIP")
                and (residual is None or (residual.dtype == x.dtype and residual.shape == x.shape
                                          and residual.is_contiguous(memory_format=torch.channels_last))))

    @staticmethod
    def _forward_hip(ctx, x, m, weight, bias, residual, norm, relu):
        """stats -> reduce -> [all-reduce] -> finalize -> apply: five launches (round 6: the per-channel arithmetic between the passes was ~20 host tensor
        statements per layer, 800 tiny launches per training step)."""
        C = x.shape[1]
        mflat = None if m is None else m.reshape(-1)
        # statistics around THIS rank's running mean: sum d, sum d^2 with d = x - centre, so that the fp32 partial sums carry deviations, not E[x^2]
        rm, rv = norm.running_mean, norm.running_var
        # Inside a checkpointed region (ASPPNeck) the forward runs again during the backward, AFTER the first call moved the running mean: sums taken
        # around the moved mean round differently, so mean / invstd / scale / shift, and with them the recomputed y that the backward of every later
        # layer saves, would differ in their last bits from what the forward handed on.  The first call keeps its centre, the recomputation sums
        # around that one (checkpoint_contexts below); the running statistics still move once per call, from their current values.
        center, phase = rm, getattr(_CKPT, "phase", None)
        if phase == "forward":
            norm._pnx_ckpt_center = rm.clone()
        elif phase == "recompute" and getattr(norm, "_pnx_ckpt_center", None) is not None:
            center, norm._pnx_ckpt_center = norm._pnx_ckpt_center, None
        s = ops.masked_bn_reduce(ops.masked_bn_stats(x, mflat, center))    # [sum d | sum d^2 | count], fp64
        group = norm.sync_group if getattr(norm, "sync", False) else False
        if group is not False:
            # the batch statistics must not depend on the buffers, and nothing makes the ranks' running means equal (broadcast_buffers=False, a
            # per-rank warm-up, a hand-rolled loop): re-centre this rank's sums to centre 0 in fp64 before they are added to the others',
            # sum x = S1 + n c, sum x^2 = S2 + 2 c S1 + n c^2, and finalize around 0
            c = center.double()
            s[C:2 * C] += 2.0 * c * s[:C] + s[2 * C] * c * c
            s[:C] += s[2 * C] * c
            dist_utils.all_reduce_sum(s, group)
            center = None
        mean32, invstd32, scale, shift, cnt32 = ops.masked_bn_finalize(s, center, weight, bias, norm.eps, norm.momentum, rm, rv, norm.num_batches_tracked)
        y = ops.masked_bn_apply(x, residual, mflat, scale, shift, relu)
        ctx.save_for_backward(x, m, weight, bias, residual, mean32, invstd32, cnt32, scale, shift)
        ctx.group, ctx.relu, ctx.hip = group, relu, True
        return y

    @staticmethod
    def _backward_hip(ctx, gy):
        x, m, weight, bias, residual, mean, invstd, cnt, scale, shift = ctx.saved_tensors
        gy = gy.to(x.dtype)
        if not gy.is_contiguous(memory_format=torch.channels_last):
            gy = gy.contiguous(memory_format=torch.channels_last)
        mflat = None if m is None else m.reshape(-1)
        sg = ops.masked_bn_reduce(ops.masked_bn_bwd_stats(gy, x, residual, mflat, scale, shift, mean, invstd, ctx.relu))
        sg_all = None                                                       # parameter gradients: local sums (DDP averages them)
        if ctx.group is not False:
            sg_all = sg.clone()
            dist_utils.all_reduce_sum(sg_all, ctx.group)
        dgamma, dbeta, mg, mgx = ops.masked_bn_bwd_finalize(sg, sg_all, cnt)
        dx, gres = ops.masked_bn_bwd_apply(gy, x, residual, mflat, scale, shift, mean, invstd, ctx.relu, mg, mgx,
                                           want_residual_grad=ctx.needs_input_grad[4])
        return dx, None, dgamma.to(weight.dtype), dbeta.to(bias.dtype), gres, None, None

    @staticmethod
    def forward(ctx, x, mask, weight, bias, residual, norm, relu):
        if mask is None:   # every site active (dense_bn_act): the HIP kernels only -- no mask word in front of a site's loads
            return _MaskedBNActFn._forward_hip(ctx, x, None, weight, bias, residual, norm, relu)
        m = mask if mask.dtype == torch.float32 else mask.float()
        if _MaskedBNActFn._hip_ok(x, residual, weight, bias, norm):
            return _MaskedBNActFn._forward_hip(ctx, x, m.contiguous(), weight, bias, residual, norm, relu)
        ctx.hip = False
        xf = x.float()
        s1 = torch.cat([(xf * m).sum(dim=(0, 2, 3)), m.sum().view(1)])
        group = norm.sync_group if getattr(norm, "sync", False) else False
        if group is not False:
            dist_utils.all_reduce_sum(s1, group)
        cnt = s1[-1].clamp(min=1.0)
        mean = s1[:-1] / cnt
        xf = xf - mean.view(1, -1, 1, 1)
        ssd = (xf * xf * m).sum(dim=(0, 2, 3))
        if group is not False:
            dist_utils.all_reduce_sum(ssd, group)
        var = ssd / cnt
        invstd = torch.rsqrt(var + norm.eps)
        with torch.no_grad():
            mom = norm.momentum
            norm.running_mean.mul_(1 - mom).add_(mean, alpha=mom)
            norm.running_var.mul_(1 - mom).add_(var * cnt / (cnt - 1).clamp(min=1.0), alpha=mom)
            norm.num_batches_tracked += 1
        xf.mul_((invstd * weight.float()).view(1, -1, 1, 1)).add_(bias.float().view(1, -1, 1, 1))
        if residual is not None:
            xf.add_(residual)
        if relu:
            xf.clamp_(min=0)
        xf.mul_(m)
        ctx.save_for_backward(x, m, weight, bias, residual, mean, invstd, cnt)
        ctx.group, ctx.relu = group, relu
        return xf.to(x.dtype)

    @staticmethod
    def backward(ctx, gy):
        if ctx.hip:
            return _MaskedBNActFn._backward_hip(ctx, gy)
        x, m, weight, bias, residual, mean, invstd, cnt = ctx.saved_tensors
        xhat = (x.float() - mean.view(1, -1, 1, 1)).mul_(invstd.view(1, -1, 1, 1))
        g = gy.float() * m
        if ctx.relu:
            pre = xhat * weight.float().view(1, -1, 1, 1) + bias.float().view(1, -1, 1, 1)
            if residual is not None:
                pre = pre + residual
            g = g * (pre > 0)
            del pre
        gres = g.to(residual.dtype) if residual is not None and ctx.needs_input_grad[4] else None
        sg = torch.cat([g.sum(dim=(0, 2, 3)), (g * xhat).sum(dim=(0, 2, 3))])
        C = weight.numel()
        dbeta, dgamma = sg[:C].clone(), sg[C:].clone()          # parameter gradients: local sums (DDP averages them)
        if ctx.group is not False:
            dist_utils.all_reduce_sum(sg, ctx.group)
        mg, mgx = (sg[:C] / cnt).view(1, -1, 1, 1), (sg[C:] / cnt).view(1, -1, 1, 1)
        dx = (g - mg - xhat * mgx).mul_((weight.float() * invstd).view(1, -1, 1, 1)).mul_(m)
        return dx.to(x.dtype), None, dgamma.to(weight.dtype), dbeta.to(bias.dtype), gres, None, None


def _mask_u8(mask):
    """(B,1,H,W) float occupancy -> (B,H,W) uint8 for the HIP convolution kernels; cached on the tensor object (one conversion per stage)."""
    m = getattr(mask, "_pnx_u8", None)
    if m is None:
        m = (mask[:, 0] != 0).to(torch.uint8).contiguous()
        try:
            mask._pnx_u8 = m
        except Exception:
            pass
    return m


_ZERO_BIAS = {}


def _zero_bias(c, device):
    key = (c, str(device))
    if key not in _ZERO_BIAS:
        _ZERO_BIAS[key] = torch.zeros(c, dtype=torch.float32, device=device)
    return _ZERO_BIAS[key]


def _hip_dgrad_s2(weight):
    """(cin, cout) of the stride-2 data-gradient kernels; PNX_TRAIN_HIP_DGRAD_S2=0: MIOpen / CK."""
    return (weight.shape[1], weight.shape[0]) in ops.CONV3X3_X3_SHAPES[2] and on("PNX_TRAIN_HIP_DGRAD_S2")


class _MaskedConv3x3Fn(torch.autograd.Function):
    """y = mask_out * conv3x3(x, W) on the product's masked-convolution kernels (csrc/conv3x3.hip) in TRAINING, bf16 autocast
    (sparse_conv.py:16-63: SubMConv2d / SparseConv2d compute only at the active sites, forward and backward).
      forward   pnx_conv3x3_bf16 (no bias, no ReLU), row segments without an active site are skipped
      dgrad     stride 1: the SAME kernel on the flipped, transposed weights with the INPUT's active set as its mask -- the upstream
                gradient is zero outside mask_out (the BatchNorm node's backward writes zeros there), and what reaches an inactive input
                site would be thrown away by that site's own mask; stride 2: pnx_conv3x3_dgrad_s2_bf16 (four parity planes; csrc/conv_dgrad_s2.h)
      wgrad     stride 1: pnx_conv3x3_wgrad_bf16 (csrc/conv_wgrad.hip) over the 16-pixel row pieces that hold an active output, fp32 accumulation,
                deterministic, stride 1 and 2 (PNX_TRAIN_HIPWGRAD=0: MIOpen's dense wrw on (x, g), exact because g is zero outside the active outputs)
    The fp32 training graph (the reference's precision) has its own node, _MaskedConv3x3F32Fn."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, x, weight, mask_out, mask_in, stride, bias=None):
        # No cast_inputs (round 6): the fp32 master weight goes straight into the packing kernel (which rounds to bf16 exactly like the cast), the bias
        # stays fp32 for the kernel, and the weight gradient comes back in fp32 -- autocast's casts of both and the bf16 round trip of dW were ~240
        # tiny launches per step.
        x = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        co = weight.shape[0]
        b = _zero_bias(co, x.device) if bias is None else bias.detach().float().contiguous()
        y = ops.conv3x3_masked(x, ops.conv3x3_pack_weights(weight), b, co, stride=stride, mask=mask_out, relu=False)
        ctx.save_for_backward(x, weight, mask_in, mask_out)
        ctx.stride = stride
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        x, weight, mask_in, mask_out = ctx.saved_tensors
        g = g.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx = dw = None
        db = g.sum(dim=(0, 2, 3), dtype=torch.float32) if len(ctx.needs_input_grad) > 5 and ctx.needs_input_grad[5] else None
        if mask_out is None:   # a dense layer (dense_conv3x3 below): the weight-gradient kernel wants the output's active set
            mask_out = _ones_mask(g.shape[0], g.shape[2], g.shape[3], g.device)
        if ctx.stride == 1:
            if need_x:
                ci = weight.shape[1]
                # dgrad of a stride-1 'same' convolution = convolution with W^T flipped (packed in one launch)
                dx = ops.conv3x3_masked(g, ops.conv3x3_pack_weights(weight, transposed=True), _zero_bias(ci, g.device), ci, stride=1, mask=mask_in, relu=False)
            if need_w:
                if on("PNX_TRAIN_HIPWGRAD"):
                    dw = ops.conv3x3_wgrad(x, g, mask_out).to(weight.dtype)
                else:
                    dw = torch.nn.grad.conv2d_weight(x, weight.shape, g, stride=1, padding=1).to(weight.dtype)
        else:
            s = ctx.stride
            hip_w = need_w and on("PNX_TRAIN_HIPWGRAD")
            if hip_w:
                dw = ops.conv3x3_wgrad(x, g, mask_out, stride=s).to(weight.dtype)
            if need_x and s == 2 and mask_in is not None and _hip_dgrad_s2(weight):   # round 6: the four parity planes on csrc/conv_dgrad_s2.h
                dx = ops.conv3x3_dgrad_s2(g, ops.conv3x3_pack_weights(weight, transposed=True), weight.shape[1], x.shape[2:], mask_in)
                need_x = False
            if need_x or (need_w and not hip_w):
                dx, dw2, _ = torch.ops.aten.convolution_backward(g, x, weight.to(g.dtype), None, (s, s), (1, 1), (1, 1), False, (0, 0), 1,
                                                                 (need_x, need_w and not hip_w, False))
                dw = dw if hip_w else dw2.to(weight.dtype)
        return dx, dw, None, None, None, db


def _split_pack(weight, transposed=False, pieces=2):
    """fp32 (Cout,Cin,3,3) -> its `pieces` packed bf16 pieces, (W_hi, W_lo) or (W_hi, W_mid, W_lo): what ops.conv3x3_f32 and ops.conv3x3_dgrad_s2 take."""
    return tuple(ops.conv3x3_pack_weights(p, transposed=transposed) for p in ops.split_f32(weight.detach().contiguous(), pieces=pieces))


def split_f32_pieces(x, mask=None, pieces=None):
    """x split into the bf16 pieces the fp32 node uses (train_f32_pieces() unless given): ops.split_f32 into 2 or 3."""
    return ops.split_f32(x, mask, train_f32_pieces() if pieces is None else pieces)


_ONES_MASK = {}


def _ones_mask(b, h, w, device):
    key = (b, h, w, device)
    if key not in _ONES_MASK:
        _ONES_MASK[key] = torch.ones((b, h, w), dtype=torch.uint8, device=device)
    return _ONES_MASK[key]


class _MaskedConv3x3F32Fn(torch.autograd.Function):
    """_MaskedConv3x3Fn for the fp32 training graph (the reference's training precision: tools/train.py runs without autocast): every fp32 operand
    is split into bf16 pieces and the significant products run on the bf16 matrix cores with fp32 accumulation.  PNX_TRAIN_F32_PIECES (read at
    forward time, kept in ctx for the backward) picks the form:
      2 (default)  two halves (16 mantissa bits together), three products x_hi W_hi + x_hi W_lo + x_lo W_hi:
        forward   pnx_conv3x3_x3 on (x_hi, x_lo) x (W_hi, W_lo) [+ bias]: one launch, fp32 out
        dgrad     stride 1: the same kernel on the halves of g and of W^T flipped, masked by the INPUT's active set; stride 2: pnx_conv3x3_dgrad_s2_x3
        wgrad     pnx_conv3x3_wgrad_x3: x_hi g_hi + x_lo g_hi + x_hi g_lo in one pass, accumulated in fp32
        relative error of every product ~ 4e-6 (the dropped low x low term and the halves' rounding, 2^-17 each)
      3            three pieces (pnx_split3_f32: exact for |x| >= 2^-100), the six products of piece orders 0..2, hi x hi last: pnx_conv3x3_x6,
                   pnx_conv3x3_dgrad_s2_x6, pnx_conv3x3_wgrad_x6 in the same places; what is dropped is ~2^-23 of sum |x||W|, i.e. fp32's own rounding
                   (~2e-7 relative, as MIOpen's fp32 kernels) for about twice the MFMA work of those layers
    mask_out = mask_in = None: a dense layer (the neck's and the head's 3x3 convolutions, dense_conv3x3 below).  pieces: the bf16 pieces of x
    (split_f32_pieces) when the caller already split it (the six branches of a SepHead share their input); they are what the backward keeps of x.
    tests/test_gpu_masked_conv_train.py and tests/test_gpu_fp32_six_products.py hold the node against an fp64 convolution.  PNX_TRAIN_F32_HIP=0 keeps
    the fp32 graph on MIOpen."""

    @staticmethod
    def forward(ctx, x, weight, bias, mask_out, mask_in, stride, pieces):
        n = train_f32_pieces()
        if pieces is None:
            pieces = split_f32_pieces(x.contiguous(memory_format=torch.channels_last), mask_in, n)   # x is zero outside its active set (masked_bn_act, the scatter)
        if len(pieces) != n:
            raise ops.PnxError(f"_MaskedConv3x3F32Fn: {len(pieces)} pieces of x given, PNX_TRAIN_F32_PIECES={n}")
        ctx.pieces = n
        b = None if bias is None else bias.detach().contiguous()
        y = ops.conv3x3_f32(pieces, _split_pack(weight, pieces=n), weight.shape[0], stride, mask_out, bias=b)
        ctx.save_for_backward(*pieces, weight, mask_in, mask_out)
        ctx.stride = stride
        return y

    @staticmethod
    def backward(ctx, g):
        n = ctx.pieces
        *xp, weight, mask_in, mask_out = ctx.saved_tensors   # read once: a checkpointed region (ASPPNeck) lets its saved tensors be unpacked one time only
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        g = g.contiguous(memory_format=torch.channels_last)
        s = ctx.stride
        dx = dw = db = None
        if need_w or need_x:
            gp = ops.split_f32(g, mask_out, n)   # the upstream gradient is zero outside mask_out (the BatchNorm node's backward writes zeros there)
        if need_x:
            if s == 1:
                dx = ops.conv3x3_f32(gp, _split_pack(weight, transposed=True, pieces=n), weight.shape[1], 1, mask_in)
            elif mask_in is not None and _hip_dgrad_s2(weight):
                dx = ops.conv3x3_dgrad_s2(gp, _split_pack(weight, transposed=True, pieces=n), weight.shape[1], xp[0].shape[2:], mask_in)
            else:   # a stride-2 layer outside the kernels' shapes: MIOpen
                dx = torch.nn.grad.conv2d_input(xp[0].shape, weight, g, stride=s, padding=1)
        if need_w:
            m = mask_out if mask_out is not None else _ones_mask(g.shape[0], g.shape[2], g.shape[3], g.device)
            dw = ops.conv3x3_wgrad(xp, gp, m, stride=s)
        if need_b:
            db = g.sum(dim=(0, 2, 3))
        return dx, dw, db, None, None, None, None


class _SmallKConv3x3Fn(torch.autograd.Function):
    """nn.Conv2d(64, k <= 4, 3, padding 1, bias) of a SepHead branch in training (centerhead.py:31-41) on csrc/head_train.hip: forward and the weight / bias
    gradient at the map's HBM rate (fp32 FMAs, fp32 accumulation, fp32 master weights also under autocast); the data gradient on MIOpen."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, x, weight, bias):
        x = x.contiguous(memory_format=torch.channels_last)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return ops.conv3x3_smallk(x, weight.detach().contiguous(), None if bias is None else bias.detach().contiguous())

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad
        dx = dw = db = None
        g = g.to(x.dtype)
        if need_x:
            dx = torch.nn.grad.conv2d_input(x.shape, weight.to(x.dtype), g, stride=1, padding=1)
        if need_w or (need_b and ctx.has_bias):
            dw, db = ops.conv3x3_smallk_wgrad(x, g, want_bias=ctx.has_bias)
        return dx, dw, db


def smallk_ok(conv, x):
    """Does the output convolution of a SepHead branch run on _SmallKConv3x3Fn?  (training, a CUDA fp32 graph or bf16 autocast; PNX_TRAIN_HEAD_HIP=0: MIOpen)"""
    if not (type(conv) is nn.Conv2d and conv.training and torch.is_grad_enabled() and x.is_cuda and x.dim() == 4 and conv.in_channels == 64
            and 1 <= conv.out_channels <= 4 and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) and conv.dilation == (1, 1)
            and conv.groups == 1 and conv.padding_mode == "zeros" and conv.weight.dtype == torch.float32
            and on("PNX_TRAIN_HEAD_HIP")):
        return False
    if torch.is_autocast_enabled():
        return torch.get_autocast_dtype("cuda") == torch.bfloat16 and x.dtype in (torch.bfloat16, torch.float32)
    return x.dtype == torch.float32


def smallk_conv(conv, x):
    if smallk_ok(conv, x):
        if torch.is_autocast_enabled() and x.dtype == torch.float32:
            x = x.to(torch.bfloat16)     # what autocast does to a convolution's input
        return _SmallKConv3x3Fn.apply(x, conv.weight, conv.bias)
    return conv(x)


def _dense3x3_ok(x, weight, stride, padding, dilation, groups, training):
    """What x3_ok and bf16_dense_ok share: a training-mode CUDA 3x3 / stride 1 / pad 1 convolution of a shape the masked stride-1 kernels serve."""
    return (training and torch.is_grad_enabled() and x.is_cuda and x.dim() == 4 and tuple(weight.shape[2:]) == (3, 3)
            and (weight.shape[1], weight.shape[0]) in ops.CONV3X3_X3_SHAPES[1] and x.shape[1] == weight.shape[1]
            and tuple(stride) == (1, 1) and tuple(padding) == (1, 1) and tuple(dilation) == (1, 1) and groups == 1)


def x3_ok(x, weight, stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1, training=True):
    """Does a DENSE 3x3 convolution of the fp32 training graph (neck / head: det3d/models/utils/conv.py, centerhead.py:24-41) run on the three-product node?"""
    return (_dense3x3_ok(x, weight, stride, padding, dilation, groups, training) and x.dtype == torch.float32 and weight.dtype == torch.float32
            and not torch.is_autocast_enabled() and on("PNX_TRAIN_F32_HIP"))


def bf16_dense_ok(x, weight, stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1, training=True):
    """x3_ok's twin under bf16 autocast: the same dense layers on the bf16 masked kernels with every site active (_MaskedConv3x3Fn)."""
    return (_dense3x3_ok(x, weight, stride, padding, dilation, groups, training) and x.dtype in (torch.float32, torch.bfloat16)
            and torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16
            and on("PNX_TRAIN_HIPCONV") and on("PNX_TRAIN_DENSE_HIP"))


def dense_conv3x3(x, weight, bias=None, pieces=None, stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1, training=True):
    """The dense 3x3 / stride 1 / pad 1 convolution of (x, weight, bias) in training, with every site active: the fp32 graph on _MaskedConv3x3F32Fn
    where x3_ok says so (pieces: x already split by split_f32_pieces), bf16 autocast on _MaskedConv3x3Fn where bf16_dense_ok does.  None where neither
    node serves the call: the caller's own convolution (MIOpen) runs instead."""
    if x3_ok(x, weight, stride, padding, dilation, groups, training):
        return _MaskedConv3x3F32Fn.apply(x, weight, bias, None, None, 1, pieces)
    if bf16_dense_ok(x, weight, stride, padding, dilation, groups, training):
        return _MaskedConv3x3Fn.apply(x, weight, None, None, 1, bias)
    return None


def x3_conv(conv, x, pieces=None):
    """conv(x) of a dense nn.Conv2d in training: on the product's kernels where dense_conv3x3 serves it, the module itself (MIOpen) otherwise."""
    if type(conv) is nn.Conv2d and conv.padding_mode == "zeros":
        y = dense_conv3x3(x, conv.weight, conv.bias, pieces, conv.stride, conv.padding, conv.dilation, conv.groups, conv.training)
        if y is not None:
            return y
    return conv(x)


def masked_conv(conv, x, mask_out, mask_in):
    """conv(x) of a backbone block; in training the 3x3 layers of ops.CONV3X3_X3_SHAPES (every 3x3 layer of the PillarNeXt-B backbone) run on the
    product's masked kernels: _MaskedConv3x3Fn under bf16 autocast (PNX_TRAIN_HIPCONV=0 keeps every layer on MIOpen), _MaskedConv3x3F32Fn in the fp32
    graph (PNX_TRAIN_F32_HIP=0: MIOpen)."""
    if (conv.training and torch.is_grad_enabled() and x.is_cuda and conv.kernel_size == (3, 3) and conv.bias is None
            and (conv.in_channels, conv.out_channels) in ops.CONV3X3_X3_SHAPES.get(conv.stride[0], ())):
        s = conv.stride[0]
        if torch.is_autocast_enabled():
            if torch.get_autocast_dtype("cuda") == torch.bfloat16 and on("PNX_TRAIN_HIPCONV"):
                return _MaskedConv3x3Fn.apply(x, conv.weight, _mask_u8(mask_out), _mask_u8(mask_in), s)
        elif x.dtype == torch.float32 and conv.weight.dtype == torch.float32 and on("PNX_TRAIN_F32_HIP"):
            return _MaskedConv3x3F32Fn.apply(x, conv.weight, None, _mask_u8(mask_out), _mask_u8(mask_in), s, None)
    return conv(x)


def masked_bn_act(x, mask, norm, residual=None, relu=True):
    """relu(norm(x, mask) [+ residual]) * mask -- one fused autograd node in train mode, the plain modules otherwise."""
    if norm.training and mask is not None and torch.is_grad_enabled():
        return _MaskedBNActFn.apply(x, mask, norm.weight, norm.bias, residual, norm, relu)
    out = norm(x, mask)
    if residual is not None:
        out = out + residual
    return (F.relu(out) if relu else out) * mask


def dense_bn_act(norm, x, relu=True):
    """[relu](norm(x)) of a DENSE nn.BatchNorm2d in training (the head's and the neck's layers: det3d/models/utils/conv.py:21-34, centerhead.py:24-30): the
    masked node with every site active -- statistics, apply + ReLU, and the backward in four passes over the map on csrc/masked_bn.hip instead of MIOpen's
    three + three kernels and a separate ReLU forward and backward.  Anything else (eval, SyncBatchNorm, CPU, other shapes, PNX_TRAIN_DENSE_BN_HIP=0): the modules."""
    if (type(norm) is nn.BatchNorm2d and norm.training and torch.is_grad_enabled() and norm.affine and norm.track_running_stats and x.is_cuda and x.dim() == 4
            and on("PNX_TRAIN_DENSE_BN_HIP")):
        xc = x if x.is_contiguous(memory_format=torch.channels_last) else None
        if xc is not None and _MaskedBNActFn._hip_ok(xc, None, norm.weight, norm.bias, norm):
            return _MaskedBNActFn.apply(xc, None, norm.weight, norm.bias, None, norm, relu)
    y = norm(x)
    return F.relu(y) if relu else y
