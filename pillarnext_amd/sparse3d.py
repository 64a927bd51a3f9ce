"""SparseResNet3D (det3d/models/backbones/sparse_resnet3d.py:9-72, blocks of det3d/models/utils/sparse_conv.py:66-104) on the sparse 3-D HIP
kernels of csrc/sparse3d.hip (include/pnx.h: pnx_sp3_*).

    SparseResNet3D(...).forward(pillar_features (V, C) fp32, coors (V, 4) int32 [b, z, y, x], input_shape [D, H, W]) -> (B, C_out*D', H', W')

Same constructor, state-dict keys and weight layout as the reference (spconv >= 2.2: (Cout, kD, kH, kW, Cin); the older (kD, kH, kW, Cin, Cout)
is accepted on load).  Each layer is a gather-GEMM over its active sites:
  - an active set is indexed by a key-order occupancy bitmap + popcount prefix (a site's row = its rank in [b, z, y, x] order, the voxel
    reader's row order);
  - SparseConv3d marks the outputs every input x tap reaches (one host sync per strided layer reads their count), SubMConv3d keeps the set;
  - a neighbour map (N_out, taps) per set and geometry -- shared by the four SubM layers of a stage -- feeds pnx_sp3_conv, which applies the
    folded BatchNorm, the residual and the ReLU in its epilogue.

That folded path runs in eval mode when no gradient is wanted.  In training mode, or when gradients are enabled and a parameter or the input
features require one, every layer is conv (SparseConvFunction: pnx_sp3_conv_train with the plain weight; backward = the same on the transposed
map for dx, pnx_sp3_wgrad for dw) -> the module's own nn.BatchNorm1d on the (N, C) rows -> ReLU on torch ops, over the same index, output sets
and neighbour maps, which forward and backward share.

use_half_precision(dtype) moves the folded eval path onto bf16 / fp16 rows and the 16-bit matrix cores (pnx_sp3_conv_h): the fp32 input features
are rounded once, every layer reads and writes padded 16-bit rows over the same index, output sets and neighbour maps, and the dense output
stays fp32.  The default, training and any call that wants gradients are untouched.

use_half_precision(dtype, training=True) also moves the autograd path's convolutions onto the 16-bit matrix cores (SparseConvHalfFunction:
pnx_sp3_conv_h_f32 for y and dx, pnx_sp3_wgrad_h for dw): the node's boundary stays fp32, its operands are rounded once, BatchNorm, residual
and ReLU remain the module's fp32 torch ops.

use_fused_norm() replaces those torch ops, in training mode, by one autograd node per layer on the kernels of csrc/sparse3d_bn.h
(SparseBNActFunction: pnx_sp3_bn_stats / _apply / _bwd_stats / _bwd_apply): batch statistics, running-statistics update, residual and ReLU in four
streaming passes; with 16-bit training on it also writes the next convolution's padded 16-bit rows, so no fp32 activation but the convolution
output survives a layer's forward.  Off by default; the default path is untouched.
"""
import math

import torch
from torch import nn

from . import dist_utils, ops
from ._lib import PnxError
from .fused import _params_version


def _triple(v):
    return tuple(int(a) for a in v) if isinstance(v, (list, tuple)) else (int(v),) * 3


def _spconv3d_weight(w, want):
    """spconv >= 2.2 stores (Cout, kD, kH, kW, Cin), older releases (kD, kH, kW, Cin, Cout)."""
    co, kd, kh, kw, ci = want
    if tuple(w.shape) == want:
        return w
    if tuple(w.shape) == (kd, kh, kw, ci, co):
        return w.permute(4, 0, 1, 2, 3).contiguous()
    raise RuntimeError(f"cannot map sparse-conv weight {tuple(w.shape)} onto SparseConv3d {want}")


class SparseConv3d(nn.Module):
    """spconv.pytorch.SparseConv3d / SubMConv3d without bias: holds the weight (Cout, kD, kH, kW, Cin) and the geometry."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, subm=False):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = _triple(kernel_size), _triple(stride), _triple(padding)
        self.subm = subm
        self.weight = nn.Parameter(torch.empty((out_channels, *self.kernel_size, in_channels)))
        bound = 1.0 / math.sqrt(in_channels * math.prod(self.kernel_size))
        nn.init.uniform_(self.weight, -bound, bound)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        k = prefix + "weight"
        if k in state_dict:
            state_dict[k] = _spconv3d_weight(state_dict[k], tuple(self.weight.shape))
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, padding={self.padding}"
                + (", subm=True" if self.subm else ""))


class SparseConv3dBlock(nn.Module):
    """sparse_conv.py:66-82: SubMConv3d (stride 1 and use_subm) or SparseConv3d, padding k // 2, + BatchNorm1d(eps 1e-3) + ReLU."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, use_subm=True):
        super().__init__()
        self.conv = SparseConv3d(in_channels, out_channels, kernel_size, stride, int(kernel_size) // 2, subm=stride == 1 and use_subm)
        self.norm = nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01)
        self.act = nn.ReLU()


class SparseBasicBlock3d(nn.Module):
    """sparse_conv.py:85-104: SubM + BN + ReLU, SubM + BN, + identity, ReLU."""

    def __init__(self, channels, kernel_size):
        super().__init__()
        self.block1 = SparseConv3dBlock(channels, channels, kernel_size, 1)
        self.conv2 = SparseConv3d(channels, channels, kernel_size, 1, int(kernel_size) // 2, subm=True)
        self.norm2 = nn.BatchNorm1d(channels, eps=1e-3, momentum=0.01)
        self.act2 = nn.ReLU()


def sparse_conv_dgrad(dy, weight, nbmap, n_in, subm):
    """dx (n_in, Cin) of y[o] = sum_t w[:, t, :] . x[nbmap[o][t]]: pnx_sp3_conv_train on dy, the transposed map and the weights packed the other way
    round.  subm: the map is a set's own, its transpose is the map with the taps mirrored, so the taps of the weights are mirrored instead."""
    cin = weight.shape[-1]
    tmap = nbmap if subm else ops.sp3_transpose_map(nbmap, n_in)
    return ops.sp3_conv(dy, tmap, ops.sp3_pack_weight_t(weight, mirror=subm), torch.zeros((cin,), dtype=torch.float32, device=dy.device), cin, relu=False,
                       per_tap=True)


class SparseConvFunction(torch.autograd.Function):
    """y[o] = sum_t w[:, t, :] . x[nbmap[o][t]] with both gradients on the HIP kernels, each computed only if it is wanted.
    subm: the layer runs on its set's own map, whose transpose is the map with the taps mirrored (no second map is built)."""

    @staticmethod
    def forward(ctx, x, weight, nbmap, subm, tick):
        x, w = x.contiguous(), weight.detach()
        cout = w.shape[0]
        y = ops.sp3_conv(x, nbmap, ops.sp3_pack_weight(w), torch.zeros((cout,), dtype=torch.float32, device=x.device), cout, relu=False,
                         per_tap=True)
        ctx.save_for_backward(x, w, nbmap)
        ctx.subm, ctx.tick = subm, tick
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, nbmap = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = None
        ctx.tick("bwd")
        if ctx.needs_input_grad[0]:
            dx = sparse_conv_dgrad(dy, w, nbmap, x.shape[0], ctx.subm)
            ctx.tick("dgrad")
        if ctx.needs_input_grad[1]:
            dw = ops.sp3_wgrad(x, nbmap, dy).view(w.shape)
            ctx.tick("wgrad")
        return dx, dw, None, None, None


class SparseConvHalfFunction(torch.autograd.Function):
    """SparseConvFunction on the 16-bit matrix cores.  The boundary is fp32 (x, weight, y, dy, dx, dw); inside, every operand is rounded once to
    `dtype` (nearest even) into padded rows and products are accumulated in fp32: y = the accumulators of pnx_sp3_conv_h_f32 on rows_h(x) and the
    packed weight `wp`; dx = the same kernel on rows_h(dy) and the weights packed the other way round (own map and mirrored taps for a
    submanifold layer, the transposed map otherwise); dw = pnx_sp3_wgrad_h on the saved rows_h(x) and rows_h(dy).  The node saves the 16-bit
    rows, half of what SparseConvFunction keeps -- which does not lower a step's peak memory while the fp32 rows stay alive in the BatchNorm /
    ReLU that produced them.
    torch.float16: gradients below fp16's range (6e-8) underflow to zero when dy is rounded -- scale the loss (torch.amp.GradScaler); bf16
    keeps fp32's range."""

    @staticmethod
    def forward(ctx, x, weight, nbmap, subm, tick, dtype, wp, *rows):
        """rows: nothing, or (xh,) = rows_h(x) as the layer before already wrote it (SparseBNActFunction's out_h); x then only carries the graph."""
        w = weight.detach()
        cout, cin = w.shape[0], w.shape[-1]
        xh = rows[0] if rows and rows[0] is not None else ops.sp3_rows_h(x, dtype)
        if xh.dtype != dtype or xh.shape[0] != x.shape[0]:
            raise PnxError(f"SparseConvHalfFunction: 16-bit rows {tuple(xh.shape)} of {xh.dtype} for x {tuple(x.shape)} in {dtype}")
        y = ops.sp3_conv_h_f32(xh, nbmap, wp, cin, cout)
        ctx.save_for_backward(xh, w, nbmap)
        ctx.subm, ctx.tick, ctx.dtype, ctx.extra = subm, tick, dtype, len(rows)
        return y

    @staticmethod
    def backward(ctx, dy):
        xh, w, nbmap = ctx.saved_tensors
        cout, cin = w.shape[0], w.shape[-1]
        dx = dw = None
        ctx.tick("bwd")
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            dyh = ops.sp3_rows_h(dy.contiguous(), ctx.dtype)  # rounded once, serves both gradients
        if ctx.needs_input_grad[0]:
            dx = sparse_conv_dgrad_h(dyh, w, nbmap, xh.shape[0], ctx.subm)
            ctx.tick("dgrad")
        if ctx.needs_input_grad[1]:
            dw = ops.sp3_wgrad_h(xh, nbmap, dyh, cin, cout).view(w.shape)
            ctx.tick("wgrad")
        return (dx, dw, None, None, None, None, None) + (None,) * ctx.extra


def sparse_conv_dgrad_h(dyh, weight, nbmap, n_in, subm):
    """sparse_conv_dgrad on the 16-bit matrix cores: dyh (n_out, round_up(Cout, 8)) padded 16-bit rows -> dx (n_in, Cin) fp32.  The weights are
    packed the other way round (w.permute(4, 1, 2, 3, 0)) by the forward's own packing; subm: own map, taps mirrored."""
    cout, cin = weight.shape[0], weight.shape[-1]
    wt = weight.permute(4, 1, 2, 3, 0)
    tmap = nbmap if subm else ops.sp3_transpose_map(nbmap, n_in)
    return ops.sp3_conv_h_f32(dyh, tmap, ops.sp3_pack_weight_h(wt.flip(1, 2, 3) if subm else wt, dyh.dtype), cout, cin)


class SparseDenseFunction(torch.autograd.Function):
    """ops.sp3_dense with its gradient, the gather back into rows."""

    @staticmethod
    def forward(ctx, x, coords, batch, grid):
        ctx.save_for_backward(coords)
        ctx.channels = x.shape[1]
        return ops.sp3_dense(x.contiguous(), coords, batch, grid)

    @staticmethod
    def backward(ctx, dout):
        return ops.sp3_dense_backward(dout, ctx.saved_tensors[0], ctx.channels), None, None, None


class SparseBNActFunction(torch.autograd.Function):
    """out = relu?(BatchNorm1d_train(y) [+ residual]) over the (n, C) fp32 rows of an active set in ONE autograd node on the kernels of
    csrc/sparse3d_bn.h: stats -> reduce -> [all-reduce] -> finalize -> apply forward, bwd_stats -> reduce -> [all-reduce] -> bwd_finalize ->
    bwd_apply backward.

        forward(y, gamma, beta, residual, residual_h, norm, relu, dtype) -> (out (n, C) fp32, out_h or None)

    norm (nn.BatchNorm1d, nn.SyncBatchNorm or the view nets' models.MaskedBatchNorm, in training mode) gives eps and momentum and has its running_mean, running_var and
    num_batches_tracked moved exactly as torch's training-mode BatchNorm1d moves them (unbiased variance); n <= 1 without synchronisation raises
    as torch does, n == 0 returns empty outputs and leaves the buffers alone.  The node saves y, the residual operand it read and the per-channel
    vectors -- not out: the backward recomputes the ReLU gate from them.
    dtype (bf16 / fp16, or None): out_h = out rounded once into padded 16-bit rows, written by the same pass and marked non-differentiable --
    what SparseConvHalfFunction takes in place of ops.sp3_rows_h(out, dtype).
    residual_h (16-bit mode): the padded 16-bit rows of `residual`, i.e. the out_h of the block's input.  The node then READS THE ROUNDED ROWS,
    as the 16-bit eval path (pnx_sp3_conv_h) does, so training and inference add the same residual, and keeps only them for the backward
    (the next convolution holds them anyway: no fp32 activation but y survives the forward); the fp32 `residual` only carries the graph, and
    its gradient passes the rounding straight through: dresidual = g.  Without residual_h (fp32 mode) the fp32 residual is read, as before.
    nn.SyncBatchNorm, or a models.MaskedBatchNorm whose enable_sync() was called (convert_sync_batchnorm; the group is its sync_group):
    [sum x | sum x^2 | n] is all-reduced in fp64 once in the forward (this rank's sums re-centred from its running mean to
    0 first), [sum g | sum g xhat] once in the backward, through dist_utils.all_reduce_sum(t, norm.process_group) looked up at call time;
    dgamma and dbeta stay the local sums (DDP averages them).  A rank without rows issues both collectives all the same."""

    @staticmethod
    def forward(ctx, y, gamma, beta, residual, residual_h, norm, relu, dtype):
        if norm.momentum is None or not norm.track_running_stats or norm.running_mean is None:
            raise PnxError("SparseBNActFunction: the norm must track running statistics with a fixed momentum")
        y = y.contiguous()
        n, C = y.shape
        masked_sync = bool(getattr(norm, "sync", False)) and not isinstance(norm, nn.SyncBatchNorm)  # models.MaskedBatchNorm after enable_sync()
        sync = isinstance(norm, nn.SyncBatchNorm) or masked_sync
        group = (norm.sync_group if masked_sync else norm.process_group) if sync else False
        res = residual_h if residual_h is not None else (None if residual is None else residual.contiguous())
        ctx.relu, ctx.group, ctx.empty = bool(relu), group, n == 0 and not sync
        if ctx.empty:
            out_h = None if dtype is None else torch.zeros((0, ops._cpad(C)), dtype=dtype, device=y.device)
            if out_h is not None:
                ctx.mark_non_differentiable(out_h)
            return torch.zeros_like(y), out_h
        if n == 1 and not sync:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(y.shape)}")
        center = norm.running_mean  # sums of deviations from the running mean: E[d^2] - E[d]^2 does not cancel when |mean| >> std
        s = ops.sp3_bn_reduce(ops.sp3_bn_stats(y, center))  # [sum d | sum d^2 | n], fp64
        if sync:
            # the batch statistics must not depend on a rank's buffers: sum x = S1 + n c, sum x^2 = S2 + 2 c S1 + n c^2, then finalize around 0
            c = center.double()
            s[C:2 * C] += 2.0 * c * s[:C] + s[2 * C] * c * c
            s[:C] += s[2 * C] * c
            dist_utils.all_reduce_sum(s, group)
            center = None
        mean, invstd, scale, shift, cnt = ops.sp3_bn_finalize(s, center, gamma.detach(), beta.detach(), norm.eps, norm.momentum, norm.running_mean,
                                                              norm.running_var, norm.num_batches_tracked)
        out, out_h = ops.sp3_bn_apply(y, res, scale, shift, relu, dtype)
        ctx.save_for_backward(y, res, mean, invstd, cnt, scale, shift)
        if out_h is not None:
            ctx.mark_non_differentiable(out_h)
        return out, out_h

    @staticmethod
    def backward(ctx, gout, _gout_h=None):
        if ctx.empty:
            return gout, None, None, (gout if ctx.needs_input_grad[3] else None), None, None, None, None
        y, res, mean, invstd, cnt, scale, shift = ctx.saved_tensors
        gout = gout.contiguous()
        sg = ops.sp3_bn_reduce(ops.sp3_bn_bwd_stats(gout, y, res, scale, shift, mean, invstd, ctx.relu))  # [sum g | sum g xhat], fp64
        sg_all = None
        if ctx.group is not False:
            sg_all = sg.clone()
            dist_utils.all_reduce_sum(sg_all, ctx.group)
        dgamma, dbeta, mg, mgx = ops.sp3_bn_bwd_finalize(sg, sg_all, cnt)
        dy, gres = ops.sp3_bn_bwd_apply(gout, y, res, scale, shift, mean, invstd, ctx.relu, mg, mgx, want_residual_grad=ctx.needs_input_grad[3])
        return dy, dgamma, dbeta, gres, None, None, None, None


def _fold(conv, bn, dtype=None):
    """Eval BatchNorm folded into the conv: packed weight (BN scale baked in) and per-channel shift, fp32.  dtype (bf16 / fp16): the weight in the
    16-bit path's fragment order instead -- the scale is still folded in fp32, the product rounded once; the shift stays fp32."""
    a = bn.weight.detach().float() * torch.rsqrt(bn.running_var.detach().float() + bn.eps)
    w = conv.weight.detach().float() * a.view(-1, 1, 1, 1, 1)
    shift = (bn.bias.detach().float() - bn.running_mean.detach().float() * a).contiguous()
    return (ops.sp3_pack_weight(w) if dtype is None else ops.sp3_pack_weight_h(w, dtype)), shift


class SparseResNet3D(nn.Module):
    """Same constructor and keys as the reference (sparse_resnet3d.py:10-47)."""

    def __init__(self, layer_nums, ds_layer_strides, ds_num_filters, num_input_features, kernel_size=[3, 3, 3, 3], out_channels=128):
        super().__init__()
        assert len(ds_layer_strides) == len(layer_nums) == len(ds_num_filters)
        self._layer_strides, self._num_filters, self._layer_nums = list(ds_layer_strides), list(ds_num_filters), list(layer_nums)
        self._num_input_features = num_input_features
        in_filters = [num_input_features, *ds_num_filters[:-1]]
        blocks = []
        for i, n in enumerate(layer_nums):
            layers = [SparseConv3dBlock(in_filters[i], ds_num_filters[i], kernel_size[i], ds_layer_strides[i], use_subm=False)]
            layers += [SparseBasicBlock3d(ds_num_filters[i], kernel_size[i]) for _ in range(n)]
            blocks.append(nn.Sequential(*layers))
        self.blocks = nn.ModuleList(blocks)
        c = ds_num_filters[-1]
        self.mapping = SparseConv3dBlock(c, out_channels, kernel_size=1, stride=1, use_subm=True)
        self.extra_conv = nn.Sequential(SparseConv3d(c, c, (3, 1, 1), (2, 1, 1), 0), nn.BatchNorm1d(c, eps=1e-3, momentum=0.01), nn.ReLU())
        self.profile = None  # a list: every phase of the next forwards appends (name, end event) -- tools/bench_voxel18.py
        self.half_dtype = None  # None: fp32; torch.bfloat16 / float16: the folded eval path runs in 16 bits (use_half_precision)
        self.half_train_dtype = None  # None: fp32; torch.bfloat16 / float16: the autograd path's convolutions run in 16 bits
        self.fused_norm = False  # True: training-mode BatchNorm1d + residual + ReLU of the autograd path run in SparseBNActFunction (use_fused_norm)

    def use_fused_norm(self, enabled=True):
        """Training: every layer's BatchNorm1d (or SyncBatchNorm) + residual + ReLU of the autograd path runs as ONE node on the HIP kernels of
        csrc/sparse3d_bn.h (SparseBNActFunction) instead of torch's batch_norm, add and relu: the same batch statistics, running-statistics
        update and gradients up to fp32 rounding in another order, fewer passes over the rows, and only y kept per layer for the backward.
        Together with use_half_precision(dtype, training=True) the node also writes the next convolution's padded 16-bit rows in the same pass
        (no ops.sp3_rows_h between layers), and a block's second layer adds the ROUNDED rows of the block input, as the 16-bit eval path does,
        with the gradient passed straight through the rounding.  A norm in eval mode (fixed statistics) keeps torch's ops.  Off by default;
        returns self."""
        self.fused_norm = bool(enabled)
        return self

    def use_half_precision(self, dtype=torch.bfloat16, training=False):
        """Inference on 16-bit rows and the 16-bit matrix cores (pnx_sp3_conv_h), as MVFFeatureNet.use_hip_convs is for the view nets: eval-mode
        forwards that want no gradient round the fp32 input features once, run every layer in `dtype` (fp32 accumulation, BN shift, residual and
        ReLU in fp32, one rounding per layer) and return the fp32 dense map; forward_sparse then returns its features in `dtype`.  Training and any
        call that wants gradients keep the fp32 autograd path.  dtype=None switches back to fp32.
        torch.float16 has 5 exponent bits: activations above 65504 become inf, which real checkpoints can reach -- bf16, the default, keeps fp32's
        range at 8 bits of precision.
        training=True: the autograd path (training mode, or any call that wants gradients) runs its convolutions on the 16-bit matrix cores
        as well (SparseConvHalfFunction): fp32 at every node's boundary, operands rounded once to `dtype`, fp32 accumulation; BatchNorm1d,
        residual and ReLU stay fp32 torch ops and forward_sparse still returns fp32 features there.  training=False leaves (or puts back)
        the autograd path in fp32.  Under torch.float16 gradients below its range underflow when dy is rounded: scale the loss
        (torch.amp.GradScaler); bf16, the default, needs none."""
        if dtype is not None and dtype not in ops._HALF:
            raise PnxError("use_half_precision: torch.bfloat16, torch.float16 or None")
        if training and dtype is None:
            raise PnxError("use_half_precision: training=True needs torch.bfloat16 or torch.float16 (dtype=None switches both paths back to fp32)")
        self.half_dtype = dtype
        self.half_train_dtype = dtype if training else None
        return self

    # ------------------------------------------------------------------------------------------ plan
    def _folded(self, dtype=None):
        """Packed weights and shifts, folded once per parameter version and element type (as mvf_encoder's view nets are)."""
        cache = self.__dict__.setdefault("_folded_cache", {})  # dtype (None: fp32) -> (parameter version, layers)
        f = cache.get(dtype)
        if f is None or f[0] != _params_version(self):
            layers = {}
            for i, seq in enumerate(self.blocks):
                layers[f"blocks.{i}.0"] = _fold(seq[0].conv, seq[0].norm, dtype)
                for j, blk in enumerate(seq[1:], 1):
                    layers[f"blocks.{i}.{j}.block1"] = _fold(blk.block1.conv, blk.block1.norm, dtype)
                    layers[f"blocks.{i}.{j}.conv2"] = _fold(blk.conv2, blk.norm2, dtype)
            layers["extra_conv"] = _fold(self.extra_conv[0], self.extra_conv[1], dtype)
            layers["mapping"] = _fold(self.mapping.conv, self.mapping.norm, dtype)
            f = cache[dtype] = (_params_version(self), layers)
        return f[1]

    def _train_packed(self, dtype):
        """The 16-bit training path's forward weights in fragment order, packed once per version of the convolution weights and element type
        (the BatchNorm buffers, which every training forward moves, do not count)."""
        cache = self.__dict__.setdefault("_train_packed_cache", {})  # dtype -> (weight versions, {conv module: packed weight})
        convs = [m for m in self.modules() if isinstance(m, SparseConv3d)]
        version = tuple((c.weight.data_ptr(), c.weight._version) for c in convs)
        f = cache.get(dtype)
        if f is None or f[0] != version:
            f = cache[dtype] = (version, {c: ops.sp3_pack_weight_h(c.weight.detach(), dtype) for c in convs})
        return f[1]

    def _tick(self, name):
        if self.profile is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.profile.append((name, e))

    def _differentiable(self, pillar_features):
        """Training mode, or a gradient is wanted: the autograd path.  Otherwise the folded eval path."""
        return self.training or (torch.is_grad_enabled() and (pillar_features.requires_grad or any(p.requires_grad for p in self.parameters())))

    def _check(self, pillar_features, coors):
        """Argument checks; returns whether the call takes the autograd path (decided once per forward)."""
        diff = self._differentiable(pillar_features)
        if diff and not (pillar_features.is_cuda and coors.is_cuda):
            if self.training:
                raise PnxError("SparseResNet3D: training needs CUDA (ROCm) tensors; the sparse 3-D layers have no CPU implementation")
            raise PnxError("SparseResNet3D: gradients need CUDA (ROCm) tensors; the sparse 3-D layers have no CPU implementation "
                           "(run under torch.no_grad() or freeze the parameters to reach the device check of the eval path)")
        if pillar_features.dtype != torch.float32:
            raise PnxError(f"SparseResNet3D: features must be fp32, got {pillar_features.dtype} (there is no bf16 / fp16 form)")
        if coors.dtype not in (torch.int32, torch.int64) or coors.dim() != 2 or coors.shape[1] != 4:
            raise PnxError("SparseResNet3D: coors must be (V, 4) integer [b, z, y, x]")
        if pillar_features.dim() != 2 or pillar_features.shape[0] != coors.shape[0]:
            raise PnxError("SparseResNet3D: pillar_features must be (V, C) with one row per coordinate")
        if pillar_features.shape[1] != self._num_input_features:
            raise PnxError(f"SparseResNet3D: {pillar_features.shape[1]} input channels, the model takes {self._num_input_features}")
        if not (pillar_features.is_cuda and coors.is_cuda):
            raise PnxError("SparseResNet3D: features and coords must be CUDA (ROCm) tensors; the sparse 3-D convolution has no CPU implementation")
        return diff

    def _strided(self, x, coords, ix, rows, B, conv, name):
        """SparseConv3d: output set (one host sync for its count), its coords, the neighbour map into the input set."""
        k, s, p = conv.kernel_size, conv.stride, conv.padding
        oix, cnt = ops.sp3_out_index(coords, B, ix.grid, k, s, p)
        n = int(cnt.item())
        oc = ops.sp3_index_coords(oix, n)
        self._tick(name + ".index")
        m = ops.sp3_neighbor_map(oc, ix, rows, k, s, p)
        self._tick(name + ".map")
        return oix, oc, m

    def _conv(self, x, m, conv, norm, folded, name, residual=None, rows=None, residual_rows=None):
        """One layer -> (its output, that output's padded 16-bit rows or None).  folded: the plan of packed weights and shifts (eval), or None:
        conv -> BatchNorm1d -> (+ residual) -> ReLU under autograd.  rows / residual_rows: the 16-bit rows of x / residual where the layer
        before wrote them (use_fused_norm with 16-bit training), else None."""
        if folded is None:
            def tick(phase):
                self._tick(f"{name}.{phase}")

            if self.half_train_dtype is None:
                y = SparseConvFunction.apply(x, conv.weight, m, conv.subm, tick)
            elif rows is None:
                y = SparseConvHalfFunction.apply(x.contiguous(), conv.weight, m, conv.subm, tick, self.half_train_dtype,
                                                 self._train_packed(self.half_train_dtype)[conv])
            else:
                y = SparseConvHalfFunction.apply(x, conv.weight, m, conv.subm, tick, self.half_train_dtype,
                                                 self._train_packed(self.half_train_dtype)[conv], rows)
            self._tick(name + ".conv")
            if self.fused_norm and norm.training:
                y, yh = SparseBNActFunction.apply(y, norm.weight, norm.bias, residual, residual_rows, norm, True, self.half_train_dtype)
                self._tick(name + ".rest")
                return y, yh
            y = norm(y)
            y = torch.relu(y if residual is None else y + residual)
            self._tick(name + ".rest")
            return y, None
        wp, shift = folded[name]
        if wp.dtype != torch.float32:  # the 16-bit plan: padded 16-bit rows in and out
            y = ops.sp3_conv_h(x, m, wp, shift, conv.in_channels, conv.out_channels, residual=residual, relu=True)
        else:
            y = ops.sp3_conv(x, m, wp, shift, conv.out_channels, residual=residual, relu=True)
        self._tick(name + ".conv")
        return y, None

    def forward_sparse(self, pillar_features, coors, input_shape, batch_size=None):
        """The active sets: [(coords (N, 4) int32, features (N, C) fp32, grid (D, H, W))] after stage 0, 1, ..., extra_conv and mapping.
        Under use_half_precision (and no gradient wanted) the features are in the 16-bit type, cut to the true channel count."""
        diff = self._check(pillar_features, coors)
        sets = self._sets(pillar_features, coors, input_shape, batch_size, diff)
        if self._half(diff) is None:
            return sets
        ch = [*self._num_filters, self._num_filters[-1], self.mapping.conv.out_channels]
        return [(c, x[:, :k], g) for (c, x, g), k in zip(sets, ch)]

    def _half(self, diff):
        """The element type of this forward's rows: the 16-bit type set by use_half_precision on the folded eval path, else None (fp32)."""
        return None if diff else self.half_dtype

    def _sets(self, pillar_features, coors, input_shape, batch_size, diff):
        if batch_size is None:
            batch_size = len(torch.unique(coors[:, 0]))  # the reference's own rule (:62)
        B = int(batch_size)
        grid = tuple(int(v) for v in input_shape)
        if len(grid) != 3 or min(grid) < 1:
            raise PnxError(f"SparseResNet3D: input_shape must be [D, H, W], got {list(input_shape)}")
        coords = coors.int().contiguous()
        x = pillar_features.contiguous()
        n = coords.shape[0]
        self._tick("start")
        ix, rows, cnt = ops.sp3_index_build(coords, B, grid, want_rows=True)
        if n:
            lo, hi = coords.min(0).values, coords.max(0).values
            ok, distinct = torch.stack([(lo >= 0).all() & (hi < torch.tensor([B, *grid], device=coords.device)).all(), cnt[0] == n]).tolist()
            if not ok:
                raise PnxError(f"SparseResNet3D: coords [b, z, y, x] outside the batch of {B} / input_shape {list(grid)}")
            if not distinct:
                raise PnxError("SparseResNet3D: coords hold duplicate sites")
        self._tick("input.index")
        half = self._half(diff)
        folded = None if diff else self._folded(half)
        if half is not None:
            x = ops.sp3_rows_h(x, half)  # the one conversion of the input: rounded, channels padded to a multiple of 8
            self._tick("input.rows")
        sets = []
        xh = None  # x's padded 16-bit rows where the layer before wrote them (use_fused_norm with 16-bit training), else None
        for i, seq in enumerate(self.blocks):
            conv = seq[0].conv
            if conv.subm:
                m = ops.sp3_neighbor_map(coords, ix, rows, conv.kernel_size, (1, 1, 1), conv.padding)
                self._tick(f"blocks.{i}.0.map")
            else:
                ix, coords, m = self._strided(x, coords, ix, rows, B, conv, f"blocks.{i}.0")
            rows = None  # a layer's output rows are in rank order
            x, xh = self._conv(x, m, conv, seq[0].norm, folded, f"blocks.{i}.0", rows=xh)
            if len(seq) > 1:
                k = seq[1].conv2.kernel_size
                m = ops.sp3_neighbor_map(coords, ix, None, k, (1, 1, 1), tuple(a // 2 for a in k))  # shared by the stage's SubM layers
                self._tick(f"blocks.{i}.subm.map")
                for j, blk in enumerate(seq[1:], 1):
                    y, yh = self._conv(x, m, blk.block1.conv, blk.block1.norm, folded, f"blocks.{i}.{j}.block1", rows=xh)
                    x, xh = self._conv(y, m, blk.conv2, blk.norm2, folded, f"blocks.{i}.{j}.conv2", residual=x, rows=yh, residual_rows=xh)
            sets.append((coords, x, ix.grid))
        ix, coords, m = self._strided(x, coords, ix, rows, B, self.extra_conv[0], "extra_conv")
        x, xh = self._conv(x, m, self.extra_conv[0], self.extra_conv[1], folded, "extra_conv", rows=xh)
        sets.append((coords, x, ix.grid))
        mc = self.mapping.conv
        m = ops.sp3_neighbor_map(coords, ix, None, mc.kernel_size, (1, 1, 1), mc.padding)
        self._tick("mapping.map")
        x, xh = self._conv(x, m, mc, self.mapping.norm, folded, "mapping", rows=xh)
        sets.append((coords, x, ix.grid))
        return sets

    def forward(self, pillar_features, coors, input_shape, batch_size=None):
        """sparse_resnet3d.py:61-72: x.dense() then view(B, C*D, H, W) -- channel index c*D + d."""
        diff = self._check(pillar_features, coors)
        if batch_size is None:
            batch_size = len(torch.unique(coors[:, 0]))
        coords, x, grid = self._sets(pillar_features, coors, input_shape, batch_size, diff)[-1]
        if diff:
            out = SparseDenseFunction.apply(x, coords, batch_size, grid)
        elif x.dtype != torch.float32:  # padded 16-bit rows (use_half_precision)
            out = ops.sp3_dense_h(x, coords, batch_size, grid, self.mapping.conv.out_channels)
        else:
            out = ops.sp3_dense(x, coords, batch_size, grid)
        self._tick("dense")
        return out
