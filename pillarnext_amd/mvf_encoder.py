"""Host-side mirror of det3d/models/readers/mvf_encoder.py ("mvf:" below): the multi-view (pillar + cylinder) reader of the mvf18_aspp detectors
(configs/models/reader/mvf_encoder.yaml, configs/experiments/waymo_det_mvf18_aspp_iou_car.yaml), on the kernels of csrc/group.hip.

    MVFFeatureNet(in_channels, voxel_size, pc_range, cylinder_size, cylinder_range, num_filters, layer_nums, ds_layer_strides,
                  ds_num_filters, kernel_size, out_channels).forward(points) -> dense (B, out_channels, gy / ds, gx / ds) map    # mvf:257-327

Same class names, constructor arguments and state-dict keys as the reference.  What runs where:
  * the two point -> cell groupings, which CLAMP the cell index instead of dropping points (mvf:57-62, 111-116), the cylinder transform, the
    per-cell means and the 10-column decoration: ONE C call each (pnx_group_points, modes PILLAR_CLAMP / CYLINDER_CLAMP); MVFFeatureNet's range
    mask (mvf:290-297) is the call's prefilter and both views write their columns into one (N', 20) buffer -- the torch.cat of mvf:304 never runs;
  * the PFN layers of a view in eval mode: pnx_pfn_layer_eval (Linear + folded BatchNorm + ReLU + per-cell max; the concat [x, max[inv]] of a
    non-last layer is read in place by the next one); in training each layer is ONE autograd node on csrc/point_layer_train.hip (ops.PointLayer:
    Linear + BatchNorm1d with batch statistics + ReLU + per-cell max, fp32; PNX_TRAIN_POINT_HIP=0 selects reader.PFNLayer on the HIP scatter-max);
  * sampling the view's map back at the points: pnx_bilinear_gather, in eval and as the forward of ops.BilinearGather in training, whose backward is
    pnx_bilinear_gather_backward (deterministic; PNX_TRAIN_BILINEAR_HIP=0 selects the torch statement over flat indices, which also serves when the
    positions need a gradient);
  * the per-view sparse ResNets: in eval mode the masked HIP convolution kernels of the PillarNeXt backbone (csrc/conv3x3.hip; BatchNorm folded,
    bf16, the 48 / 96 / 192 channels zero-padded to the kernels' 64 / 128 / 256: _HipViewNet), in training the masked-dense blocks of models.py
    (spconv is absent from the image; like the backbone that part is unpinned), or, after use_sparse_rows(), the sparse gather-GEMM kernels of
    csrc/sparse3d.hip over the rows of the active cells -- a 2-D sparse convolution is the 3-D one on a grid of depth 1 -- in eval (BatchNorm
    folded, fp32) and in training (sparse3d.SparseConvFunction + SparseBNActFunction per layer), sampled by pnx_sp3_bilinear_gather: no
    (B, H, W, C) map exists at any stage; the two PointNets: in training the same fused node (pointnet2
    hands over its per-pillar maximum and never writes the (N, 256) activation), otherwise torch Linear (rocBLAS) + BatchNorm + ReLU.
CUDA tensors only: there is no CPU path."""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import ops
from ._lib import PNX_GROUP_CYLINDER_CLAMP, PNX_GROUP_PILLAR_CLAMP
from .fused import _fold_bn, _HipConv3x3, _params_version
from .models import SparseBasicBlock, SparseConvBlock, _Seq
from .reader import PFNLayer
from .sparse3d import SparseBNActFunction, SparseConvFunction, SparseDenseFunction
from .switches import on
from .voxel_encoder import _device_points, batch_of, grid_of


class PointNet(nn.Module):
    """Linear(no bias) + BatchNorm1d(eps 1e-3, momentum 0.01) + ReLU per point (mvf:19-37)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.linear = nn.Linear(in_channels, out_channels, bias=False)
        self.norm = nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01)

    def forward(self, points):
        if points.is_cuda and ops.point_layer_serves(self, self.norm):         # training: the fused node of csrc/point_layer_train.hip
            return ops.point_layer(points, self.linear, self.norm)[0]
        return F.relu(self.norm(self.linear(points)))

    def cell_max(self, points, unq_inv, num_cells):
        """scatter_max(forward(points), unq_inv)[0] (mvf:322): on the node the (N, C) activation is never written."""
        if points.is_cuda and ops.point_layer_serves(self, self.norm):
            return ops.point_layer(points, self.linear, self.norm, unq_inv, num_cells, want_y=False, want_max=True)[1]
        return ops.scatter_max(self.forward(points), unq_inv, num_cells)[0]


class _ClampView(nn.Module):
    """Shared body of PillarVoxelNet / CylinderNet: returns (features (N, F + 5), coords (P, 3) int32 [b, c1, c0], unq_inv, grid [g1, g0])."""

    mode = PNX_GROUP_PILLAR_CLAMP

    def __init__(self, voxel_size, pc_range):
        super().__init__()
        self.voxel_size = np.array(voxel_size)
        self.pc_range = np.array(pc_range)
        self._geoms = {}

    def geom(self, keep_range=None):
        key = None if keep_range is None else tuple(float(v) for v in keep_range)
        if key not in self._geoms:
            self._geoms[key] = ops.group_geom(self.pc_range, self.voxel_size, self.mode, keep_range)
        return self._geoms[key]

    def group(self, points, batch_size=None, keep_range=None, features_out=None):
        points = _device_points(points, type(self).__name__)
        return ops.group_points(points, batch_of(points, batch_size), self.geom(keep_range), want_features=True, features_out=features_out)

    def forward(self, points, batch_size=None):
        r = self.group(points, batch_size)
        return r["features"], r["coords"], r["unq_inv"], grid_of(self.pc_range, self.voxel_size)[[1, 0]]


class PillarVoxelNet(_ClampView):
    """mvf:39-86: cells over (x, y)."""


class CylinderNet(_ClampView):
    """mvf:88-141: the same grouping over (phi [deg], z); features [phi z rho f.. | cluster | centre]."""

    mode = PNX_GROUP_CYLINDER_CLAMP


def bilinear_interpolate(image, coords):
    """mvf:208-246 as autograd-capable torch ops over flat indices (the training path; eval runs pnx_bilinear_gather): image (B, C, H, W),
    coords (N, 3) = [b, x, y] in cell units -> (N, C).  Corner (kx, ky) = (floor(x) + kx, floor(y) + ky) clamped to the map; its weight is the product
    of the distances to the OTHER clamped corner along each axis, as the reference computes it after clamping."""
    B, C, H, W = image.shape
    flat = image.permute(0, 2, 3, 1).reshape(B * H * W, C)
    b = coords[:, 0].long()
    px, py = coords[:, 1], coords[:, 2]
    fx, fy = torch.floor(px).long(), torch.floor(py).long()
    xs = torch.stack([fx.clamp(0, W - 1), (fx + 1).clamp(0, W - 1)], 1)
    ys = torch.stack([fy.clamp(0, H - 1), (fy + 1).clamp(0, H - 1)], 1)
    wx = torch.stack([xs[:, 1].to(px.dtype) - px, px - xs[:, 0].to(px.dtype)], 1)
    wy = torch.stack([ys[:, 1].to(py.dtype) - py, py - ys[:, 0].to(py.dtype)], 1)
    out = None
    for kx, ky in ((0, 0), (0, 1), (1, 0), (1, 1)):
        term = flat[(b * H + ys[:, ky]) * W + xs[:, kx]] * (wx[:, kx] * wy[:, ky]).unsqueeze(-1).to(flat.dtype)
        out = term if out is None else out + term
    return out


def _fold_pfn(pfn):
    """(W' transposed (cin, cout), shift (cout)): BatchNorm1d(eval) folded into the Linear, fp32 (pnx_pfn_fold_bn's algebra)."""
    a = pfn.norm.weight.detach().float() / torch.sqrt(pfn.norm.running_var.float() + pfn.norm.eps)
    wt = (pfn.linear.weight.detach().float() * a[:, None]).t().contiguous()
    return wt, (pfn.norm.bias.detach().float() - pfn.norm.running_mean.float() * a).contiguous()


def _pad_to(c):
    """Channel count of the masked HIP convolution kernel that serves c channels (csrc/conv3x3.hip: 64, 128, 256)."""
    for k in (64, 128, 256):
        if c <= k:
            return k
    return 0


class _HipViewNet:
    """The sparse ResNet of one view (mvf:165-185: per stage a SparseConv2d block + n SubM basic blocks, 48 / 96 / 192 / 192 channels in the YAML) in eval
    mode on the masked HIP convolution kernels of the PillarNeXt backbone: BatchNorm folded into the weights, channels zero-padded to the kernels'
    64 / 128 / 256 (padded output channels have zero weights and zero bias, so they stay exactly 0 and cost MFMA lanes, not correctness), bf16
    channels_last, active-site masks as uint8 maps (SparseConv2d: mask_out = the 3x3 / stride pooled mask, SubM: unchanged).  Built from a
    SingleView's `blocks`; rebuilt when its parameters change.  Inference only."""

    def __init__(self, blocks, dtype=torch.bfloat16):
        self.dtype, self.stages = dtype, []
        self.version = _params_version(blocks)
        for seq in blocks:
            mods = []
            for m in seq:
                if isinstance(m, SparseConvBlock):
                    mods.append(("conv", self._conv(m.conv, m.norm), m.stride, m.subm))
                elif isinstance(m, SparseBasicBlock):
                    mods.append(("block", self._conv(m.block1.conv, m.block1.norm), self._conv(m.conv2, m.norm2)))
                else:
                    raise ops.PnxError(f"_HipViewNet: unexpected module {type(m).__name__}")
            self.stages.append(mods)
        self.cin = self.stages[0][0][1].cin
        self.cout_true = blocks[-1][-1].norm2.num_features if hasattr(blocks[-1][-1], "norm2") else blocks[-1][-1].norm.num_features

    def _conv(self, conv, norm):
        if tuple(conv.kernel_size) != (3, 3) or tuple(conv.padding) != (1, 1) or conv.bias is not None:
            raise ops.PnxError("_HipViewNet: 3x3 / pad 1 / bias-free convolutions only")
        w, b = _fold_bn(conv.weight, norm)
        co, ci = w.shape[:2]
        cop, cip = _pad_to(co), _pad_to(ci)
        stride = int(conv.stride[0])
        shapes = ops.CONV3X3_SHAPES_S1 if stride == 1 else ops.CONV3X3_SHAPES_S2
        if not cop or not cip or (cip, cop) not in shapes:
            raise ops.PnxError(f"_HipViewNet: no kernel for {ci} -> {co} channels at stride {stride}")
        wp = torch.zeros((cop, cip, 3, 3), dtype=torch.float32, device=w.device)
        wp[:co, :ci] = w
        bp = torch.zeros((cop,), dtype=torch.float32, device=w.device)
        bp[:co] = b
        return _HipConv3x3(wp, bp, stride, dtype=self.dtype).to(w.device)

    @staticmethod
    def supported(blocks):
        try:
            for seq in blocks:
                for m in seq:
                    if isinstance(m, SparseConvBlock):
                        cs = [(m.conv, m.stride)]
                    elif isinstance(m, SparseBasicBlock):
                        cs = [(m.block1.conv, 1), (m.conv2, 1)]
                    else:
                        return False
                    for c, st in cs:
                        shapes = ops.CONV3X3_SHAPES_S1 if st == 1 else ops.CONV3X3_SHAPES_S2
                        if tuple(c.kernel_size) != (3, 3) or c.bias is not None or (_pad_to(c.in_channels), _pad_to(c.out_channels)) not in shapes:
                            return False
            return True
        except Exception:
            return False

    def __call__(self, cell_features, coords, batch_size, H, W):
        """cell_features (P, C) fp32 at coords (P, 3) int32 [b, h, w] -> (map (B, Cpad, H', W') channels_last in self.dtype, true channel count)."""
        dev = cell_features.device
        canvas = torch.zeros((batch_size, H, W, self.cin), dtype=self.dtype, device=dev)
        occ = torch.zeros((batch_size, H, W), dtype=torch.uint8, device=dev)
        u = coords.long()
        canvas[u[:, 0], u[:, 1], u[:, 2], : cell_features.shape[1]] = cell_features.to(self.dtype)
        occ[u[:, 0], u[:, 1], u[:, 2]] = 1
        x, mask = canvas.permute(0, 3, 1, 2), occ                     # channels_last view of the NHWC canvas
        for mods in self.stages:
            for m in mods:
                if m[0] == "conv":
                    _, conv, stride, subm = m
                    if not subm:
                        mask = ops.mask_pool3(mask, stride)             # active set of a SparseConv2d's output
                    x = conv(x, mask)
                else:
                    _, c1, c2 = m
                    x = c2(c1(x, mask), mask, residual=x)
        return x


def sparse_weight_view(conv):
    """The (Cout, Cin, kH, kW) weight of a view's _SpConv2d as the sparse kernels read it: (Cout, 1, kH, kW, Cin), a VIEW of the parameter (no
    copy, so autograd delivers dW in the parameter's own layout and a checkpoint written either way loads either way)."""
    return conv.weight.permute(0, 2, 3, 1).unsqueeze(1)


def _no_tick(phase):
    pass


def _conv_geom(conv):
    """(kernel, stride, padding) of a view's 2-D convolution as the 3-D geometry over a grid of depth 1."""
    (kh, kw), (sh, sw), (ph, pw) = conv.kernel_size, conv.stride, conv.padding
    if conv.bias is not None or tuple(conv.dilation) != (1, 1) or conv.groups != 1 or (ph, pw) != (kh // 2, kw // 2):
        raise ops.PnxError("SingleView.use_sparse_rows: bias-free, undilated convolutions with padding k // 2 only")
    return (1, int(kh), int(kw)), (1, int(sh), int(sw)), (0, int(ph), int(pw))


class SingleView(nn.Module):
    """PFN layers + a sparse ResNet over one view's cells, sampled back at the points (mvf:143-206).  The sparse blocks are the
    masked-dense stand-ins of models.py (same keys: blocks.{i}.{j}.conv.weight ...)."""

    def __init__(self, in_channels, num_filters, layer_nums, ds_layer_strides, ds_num_filters, kernel_size, mode, voxel_size, pc_range, norm_cfg=None,
                 act_cfg=None):
        super().__init__()
        self.mode = mode
        self.voxel_size = np.array(voxel_size[:2])
        self.bias = np.array(pc_range[:2])
        nf = [in_channels] + list(num_filters)
        self.pfn_layers = nn.ModuleList([PFNLayer(nf[i], nf[i + 1], norm_cfg=norm_cfg, last_layer=i >= len(nf) - 2) for i in range(len(nf) - 1)])
        in_filters = [nf[-1], *ds_num_filters[:-1]]
        self.blocks = nn.ModuleList([_Seq([SparseConvBlock(in_filters[i], ds_num_filters[i], kernel_size[i], ds_layer_strides[i], use_subm=False)]
                                          + [SparseBasicBlock(ds_num_filters[i], kernel_size[i]) for _ in range(n)]) for i, n in enumerate(layer_nums)])
        self.ds_rate = np.prod(np.array(ds_layer_strides))
        self.conv_dtype = None      # None: the blocks run as fp32 torch modules; torch.bfloat16 / float16: eval runs them on the HIP kernels (use_hip_convs)
        self.sparse_rows = False    # True: every call use_hip_convs does not serve runs the blocks on the rows of the active cells (use_sparse_rows)

    def use_hip_convs(self, dtype=torch.bfloat16):
        """Inference in 16-bit activations for the view's sparse ResNet (what FusedPillarNeXt is to the PillarNeXt backbone): eval-mode forwards under
        no_grad run `blocks` on the masked HIP convolution kernels (_HipViewNet).  dtype=None switches back to the fp32 modules."""
        if dtype is not None and dtype not in ops._HALF:
            raise ops.PnxError("use_hip_convs: torch.bfloat16, torch.float16 or None")
        self.conv_dtype = dtype
        return self

    def use_sparse_rows(self, enabled=True):
        """The view's sparse ResNet and its sampling on the ROWS of the active cells (csrc/sparse3d.hip, fp32) instead of a dense (B, H, W, C) map,
        in eval and in training: memory and time follow the number of occupied cells, not the grid.  Same modules, parameters and state-dict keys;
        results equal the masked-dense path's up to fp32 summation order.  Eval under no_grad keeps use_hip_convs where that is set (16-bit);
        every other call takes the rows.  CUDA tensors only.  Off by default; returns self."""
        self.sparse_rows = bool(enabled)
        return self

    def _rows_folded(self):
        """{conv: (packed weight with the eval BatchNorm's scale folded in, shift)} for pnx_sp3_conv, once per parameter version."""
        f = self.__dict__.get("_rows_folded_cache")
        version = _params_version(self.blocks)
        if f is None or f[0] != version:
            layers = {}
            for seq in self.blocks:
                for m in seq:
                    for conv, bn in ((m.conv, m.norm),) if isinstance(m, SparseConvBlock) else ((m.block1.conv, m.block1.norm), (m.conv2, m.norm2)):
                        a = bn.weight.detach().float() * torch.rsqrt(bn.running_var.detach().float() + bn.eps)    # sparse3d._fold's algebra
                        w = sparse_weight_view(conv).detach().float() * a.view(-1, 1, 1, 1, 1)
                        layers[conv] = (ops.sp3_pack_weight(w), (bn.bias.detach().float() - bn.running_mean.detach().float() * a).contiguous())
            f = self.__dict__["_rows_folded_cache"] = (version, layers)
        return f[1]

    def _rows_conv(self, x, m, conv, norm, subm, folded, residual=None):
        """One layer on rows: relu(BatchNorm(conv(x)) [+ residual]).  folded: the eval plan; None: under autograd."""
        if folded is not None:
            wp, shift = folded[conv]
            return ops.sp3_conv(x, m, wp, shift, conv.out_channels, residual=residual, relu=True)
        y = SparseConvFunction.apply(x, sparse_weight_view(conv), m, subm, _no_tick)
        if norm.training:
            return SparseBNActFunction.apply(y, norm.weight, norm.bias, residual, None, norm, True, None)[0]
        y = F.batch_norm(y, norm.running_mean, norm.running_var, norm.weight, norm.bias, False, 0.0, norm.eps)
        return torch.relu(y if residual is None else y + residual)

    def sparse_sets(self, fv, unq, batch_size, H, W, differentiable=None):
        """`blocks` on rows: fv (P, C) fp32 at unq (P, 3) int32 [b, y, x] (distinct cells) -> per stage (coords (N, 4) int32 [b, 0, y, x] in
        rank = [b, y, x] order, features (N, C_stage) fp32, the set's ops.Sp3Index over (1, H_stage, W_stage)).  A SparseConvBlock builds its output
        set (the 3x3 / stride pooled input set; one host sync reads its size), a stage's SparseBasicBlocks share one submanifold map.
        differentiable (default: training mode, or a gradient is wanted): layer by layer under autograd instead of the folded eval kernels."""
        if not (fv.is_cuda and unq.is_cuda):
            raise ops.PnxError("SingleView.use_sparse_rows needs CUDA (ROCm) tensors; the sparse kernels have no CPU implementation")
        if fv.dtype != torch.float32 or fv.dim() != 2 or unq.dim() != 2 or unq.shape[1] != 3 or unq.shape[0] != fv.shape[0]:
            raise ops.PnxError("SingleView.sparse_sets: fv (P, C) fp32 with one row per cell of unq (P, 3) [b, y, x]")
        if differentiable is None:
            differentiable = self.training or torch.is_grad_enabled() and (fv.requires_grad or any(p.requires_grad for p in self.blocks.parameters()))
        B = int(batch_size)
        u = unq.int()
        coords = torch.stack([u[:, 0], torch.zeros_like(u[:, 0]), u[:, 1], u[:, 2]], dim=1).contiguous()
        ix, rows, _ = ops.sp3_index_build(coords, B, (1, H, W), want_rows=True)
        folded = None if differentiable else self._rows_folded()
        x = fv.contiguous()
        sets = []
        for seq in self.blocks:
            for j, m in enumerate(seq):
                if j == 0 and isinstance(m, SparseConvBlock):
                    k, s, p = _conv_geom(m.conv)
                    if m.subm:
                        nb = ops.sp3_neighbor_map(coords, ix, rows, k, (1, 1, 1), p)
                    else:
                        oix, cnt = ops.sp3_out_index(coords, B, ix.grid, k, s, p)
                        oc = ops.sp3_index_coords(oix, int(cnt.item()))
                        nb = ops.sp3_neighbor_map(oc, ix, rows, k, s, p)
                        ix, coords = oix, oc
                    rows = None      # a layer's output rows are in rank order
                    x = self._rows_conv(x, nb, m.conv, m.norm, m.subm, folded)
                    sub = None
                elif isinstance(m, SparseBasicBlock) and j > 0:
                    k, s, p = _conv_geom(m.conv2)
                    if s != (1, 1, 1) or _conv_geom(m.block1.conv) != (k, s, p):
                        raise ops.PnxError("SingleView.use_sparse_rows: a basic block's convolutions must be two equal stride-1 kernels")
                    if sub is None or sub[0] != k:
                        sub = (k, ops.sp3_neighbor_map(coords, ix, None, k, s, p))     # shared by the stage's submanifold layers
                    y = self._rows_conv(x, sub[1], m.block1.conv, m.block1.norm, True, folded)
                    x = self._rows_conv(y, sub[1], m.conv2, m.norm2, True, folded, residual=x)
                else:
                    raise ops.PnxError(f"SingleView.use_sparse_rows: unexpected module {type(m).__name__} at position {j} of a stage")
            sets.append((coords, x, ix))
        return sets

    def _forward_rows(self, fv, pos, unq, unq_inv, batch_size, H, W):
        coords, x, ix = self.sparse_sets(fv, unq, batch_size, H, W)[-1]
        ds = int(self.ds_rate)
        if torch.is_grad_enabled() and pos.requires_grad:
            # the positions need a gradient: the torch statement on the (small, last-stage) dense map, as on the masked-dense path
            return self.sample(SparseDenseFunction.apply(x, coords, ix.batch, ix.grid), pos, unq, unq_inv)
        if torch.is_grad_enabled() and x.requires_grad:
            return ops.SparseBilinearGather.apply(x, coords, ix, pos, self.bias, self.voxel_size, unq, unq_inv, ds)
        return ops.sp3_bilinear_gather(x, ix, pos, self.bias, self.voxel_size, unq, unq_inv, ds)

    def _pos_columns(self, features):
        return features[:, 0:2] if self.mode == "pillar" else features[:, 10:12]

    def cell_features(self, features, unq_inv, num_cells):
        """(P, C) = scatter_max over the cells of the PFN stack's output (mvf:187-188)."""
        if self.training and features.is_cuda and all(ops.point_layer_serves(pfn, pfn.norm) for pfn in self.pfn_layers):
            # training on the fused node (PNX_TRAIN_POINT_HIP): per layer Linear + BatchNorm1d + ReLU + cell max in one autograd node; the last
            # layer's maximum IS the cell feature -- the feat_max[unq_inv] gather and the second scatter_max of the torch path do not run
            x = features
            for k, pfn in enumerate(self.pfn_layers):
                last = k == len(self.pfn_layers) - 1
                if pfn.last_vfe != last:
                    raise ops.PnxError("SingleView: only the final PFN layer may be a last_layer")
                y, g = ops.point_layer(x, pfn.linear, pfn.norm, unq_inv, num_cells, want_y=not last, want_max=True)
                if last:
                    return g
                x = torch.cat([y, g[unq_inv]], dim=1)
        if self.training or torch.is_grad_enabled() and any(p.requires_grad for p in self.pfn_layers.parameters()):
            for pfn in self.pfn_layers:
                features = pfn(features, unq_inv, num_cells)
            return ops.scatter_max(features, unq_inv, num_cells)[0]
        x, g = features, None
        for k, pfn in enumerate(self.pfn_layers):     # eval: one fused launch per layer; [x, max[inv]] is read in place by the next layer
            wt, shift = _fold_pfn(pfn)
            last = k == len(self.pfn_layers) - 1
            if pfn.last_vfe != last:
                raise ops.PnxError("SingleView: only the final PFN layer may be a last_layer")
            x, g = ops.pfn_layer_eval(x, g, unq_inv, wt, shift, num_cells, store=not last, want_max=True)
        return g

    def forward(self, features, unq, unq_inv, grid_size, batch_size=None):
        pos = self._pos_columns(features)
        P = unq.shape[0]
        fv = self.cell_features(features, unq_inv, P)
        if batch_size is None:
            batch_size = len(torch.unique(unq[:, 0]))                          # the reference's rule (mvf:190)
        H, W = int(grid_size[0]), int(grid_size[1])
        if self.conv_dtype is not None and not (self.training or torch.is_grad_enabled()):
            # eval, 16-bit inference requested (use_hip_convs): the view's sparse ResNet on the masked HIP convolution kernels
            net = self.__dict__.get("_hip_net")
            if net is None or net.version != _params_version(self.blocks) or net.dtype != self.conv_dtype:
                net = _HipViewNet(self.blocks, self.conv_dtype) if _HipViewNet.supported(self.blocks) else False
                self.__dict__["_hip_net"] = net
            if net is False:
                raise ops.PnxError("SingleView.use_hip_convs: this view's layer shapes have no masked HIP convolution kernel")
            if net:
                x = net(fv, unq, batch_size, H, W)
                out = ops.bilinear_gather(x, pos, self.bias, self.voxel_size, unq, unq_inv, int(self.ds_rate))
                return out[:, : net.cout_true].contiguous()
        if self.sparse_rows:
            return self._forward_rows(fv, pos, unq, unq_inv, batch_size, H, W)
        canvas = torch.zeros((batch_size, H, W, fv.shape[1]), dtype=fv.dtype, device=fv.device)
        mask = torch.zeros((batch_size, 1, H, W), dtype=fv.dtype, device=fv.device)
        u = unq.long()
        canvas[u[:, 0], u[:, 1], u[:, 2]] = fv
        mask[u[:, 0], 0, u[:, 1], u[:, 2]] = 1
        x = canvas.permute(0, 3, 1, 2)                                         # channels_last view of the NHWC canvas
        for blk in self.blocks:
            x, mask = blk(x, mask)
        return self.sample(x, pos, unq, unq_inv)

    def sample(self, x, pos, unq, unq_inv):
        """The view's map x (B, C, H', W') sampled at the points (mvf:213-216) -> (N, C)."""
        if not (self.training or torch.is_grad_enabled() and x.requires_grad) and x.dtype in ops._DT:
            return ops.bilinear_gather(x.contiguous(memory_format=torch.channels_last), pos, self.bias, self.voxel_size, unq, unq_inv, int(self.ds_rate))
        if (torch.is_grad_enabled() and x.requires_grad and x.is_cuda and x.dtype in ops._DT and not pos.requires_grad
                and on("PNX_TRAIN_BILINEAR_HIP")):
            # training: the eval kernel forward, its gradient w.r.t. the map on pnx_bilinear_gather_backward
            return ops.BilinearGather.apply(x.contiguous(memory_format=torch.channels_last), pos, self.bias, self.voxel_size, unq, unq_inv, int(self.ds_rate))
        vs = torch.from_numpy(self.voxel_size).type_as(pos).to(pos.device)
        bias = torch.from_numpy(self.bias).type_as(pos).to(pos.device)
        cell = (pos - bias) / vs
        cell = torch.cat((unq[unq_inv][:, 0:1].to(cell.dtype), cell / float(self.ds_rate)), dim=-1)
        return bilinear_interpolate(x, cell)

    bilinear_interpolate = staticmethod(bilinear_interpolate)


class MVFFeatureNet(nn.Module):
    """mvf:249-327."""

    def __init__(self, in_channels, voxel_size, pc_range, cylinder_size, cylinder_range, num_filters, layer_nums, ds_layer_strides, ds_num_filters,
                 kernel_size, out_channels):
        super().__init__()
        self.in_channels = in_channels
        self.voxel_size, self.pc_range = voxel_size, pc_range
        self.cylinder_range, self.cylinder_size = cylinder_range, cylinder_size
        self.voxelization = PillarVoxelNet(voxel_size, pc_range)
        self.cylinderlization = CylinderNet(cylinder_size, cylinder_range)
        c = (in_channels + 5) * 2
        self.pillarview = SingleView(c, num_filters, layer_nums, ds_layer_strides, ds_num_filters, kernel_size, "pillar", self.voxel_size, self.pc_range)
        self.cylinderview = SingleView(c, num_filters, layer_nums, ds_layer_strides, ds_num_filters, kernel_size, "cylinder", self.cylinder_size,
                                       self.cylinder_range)
        self.ds_rate = np.prod(np.array(ds_layer_strides))
        self.pointnet1 = PointNet(c, ds_num_filters[-1])
        self.pointnet2 = PointNet(ds_num_filters[-1] * 3, out_channels)

    def use_hip_convs(self, dtype=torch.bfloat16):
        """Both views' sparse ResNets on the masked HIP convolution kernels in eval mode (SingleView.use_hip_convs)."""
        self.pillarview.use_hip_convs(dtype), self.cylinderview.use_hip_convs(dtype)
        return self

    def use_sparse_rows(self, enabled=True, views=("pillar", "cylinder")):
        """SingleView.use_sparse_rows for the named views ("pillar", "cylinder"); a view that is not named is switched off.  The cylinder view's
        grid is small and far denser than the pillar view's: views=("pillar",) keeps it on the masked-dense path.  Returns self."""
        by_name = {"pillar": self.pillarview, "cylinder": self.cylinderview}
        unknown = [v for v in views if v not in by_name]
        if unknown:
            raise ops.PnxError(f"use_sparse_rows: unknown views {unknown} (pillar, cylinder)")
        for name, view in by_name.items():
            view.use_sparse_rows(bool(enabled) and name in views)
        return self

    def group_views(self, points, batch_size=None):
        """Both groupings of the range-masked points (mvf:290-304): (feat (N', 2 (F + 5)), pillar result, cylinder result)."""
        points = _device_points(points, "MVFFeatureNet")
        B = batch_of(points, batch_size)
        c = points.shape[1] + 4
        feat = torch.empty((max(points.shape[0], 1), 2 * c), dtype=torch.float32, device=points.device)
        pr = self.voxelization.group(points, B, keep_range=self.pc_range, features_out=(feat, 0))
        cr = self.cylinderlization.group(points, B, keep_range=self.pc_range, features_out=(feat, c))
        return feat[:pr["Nk"]], pr, cr, B

    def forward(self, points, batch_size=None):
        feat, pr, cr, B = self.group_views(points, batch_size)
        pcoords, pinv, ccoords, cinv = pr["coords"], pr["unq_inv"], cr["coords"], cr["unq_inv"]
        psize = grid_of(self.voxelization.pc_range, self.voxelization.voxel_size)[[1, 0]]
        csize = grid_of(self.cylinderlization.pc_range, self.cylinderlization.voxel_size)[[1, 0]]
        if batch_size is None:
            batch_size = len(torch.unique(pcoords[:, 0]))                      # the reference's rule (mvf:320)
        pv = self.pillarview(feat, pcoords, pinv, psize, batch_size)
        cv = self.cylinderview(feat, ccoords, cinv, csize, batch_size)
        x = torch.cat((self.pointnet1(feat), pv, cv), dim=-1)
        pillar = self.pointnet2.cell_max(x, pinv, pcoords.shape[0])
        ds = int(self.ds_rate)
        u = pcoords.long()
        H, W = int(psize[0]) // ds, int(psize[1]) // ds
        # SparseConvTensor(features, coords // ds, ...).dense() (mvf:322-327): several pillars fall into one coarse cell; spconv's dense() scatters them
        # in index order -- which one stays is unspecified there and here (index_put without accumulate)
        out = torch.zeros((batch_size, H, W, pillar.shape[1]), dtype=pillar.dtype, device=pillar.device)
        out[u[:, 0], u[:, 1] // ds, u[:, 2] // ds] = pillar
        return out.permute(0, 3, 1, 2)
