"""Thin torch-tensor front-ends over the C ABI (include/pnx.h).  PyTorch is used for device memory and the
current stream only; every computation below happens in libpnx_hip.so."""
import ctypes

import torch

from . import _lib
from ._lib import PNX_BF16, PNX_F16, PNX_F32, PNX_NCHW, PNX_NHWC, PnxError, check, lib, ptr, stream_ptr

_DT = {torch.float32: PNX_F32, torch.bfloat16: PNX_BF16, torch.float16: PNX_F16}


def _need_cuda(t, name):
    if not t.is_cuda:
        raise PnxError(f"{name} must be a CUDA (ROCm) tensor; the PillarNeXt hot path has no CPU implementation")
    if not t.is_contiguous():
        raise PnxError(f"{name} must be contiguous")


class Workspace:
    """Grow-only device scratch, one buffer per (device, current stream): the include/pnx.h contract (256-byte aligned, one workspace per stream).
    Scratch that persists between calls uses a Workspace.  Scratch that lives as long as one call or one autograd ctx is a plain
    torch.empty(nbytes, dtype=torch.uint8) of exactly the size the library asks for."""

    def __init__(self, headroom=1.25):
        self._bufs, self._headroom = {}, headroom   # a request that depends on the data (point counts) creeps: over-allocate; one that follows from layer shapes: 1.0

    @staticmethod
    def _key(device=None):
        dev = torch.cuda.current_device() if device is None or device.index is None else device.index
        return dev, torch.cuda.current_stream(dev).cuda_stream

    @property
    def buf(self):
        """The buffer of the current device and stream, or None."""
        return self._bufs.get(self._key())

    def get(self, nbytes, device):
        key = self._key(torch.device(device))
        buf = self._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = self._bufs[key] = torch.empty(max(int(nbytes * self._headroom), 256), dtype=torch.uint8, device=device)  # never empty: a null base is an error
        assert buf.data_ptr() % 256 == 0
        return buf


# --------------------------------------------------------------------------------------------- reader
def fold_bn(F, w0, bn0, w1, bn1, eps, out=None):
    """bn = (gamma, beta, running_mean, running_var) fp32 CUDA tensors -> folded parameter buffer."""
    n = 32 * (F + 5) + 32 + 64 * 64 + 64 + 64 * 121 + 64 * 71  # PNX_PFN_FOLDED_FLOATS(F)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=w0.device)
    ts = [w0, *bn0, w1, *bn1]
    for t in ts:
        _need_cuda(t, "PFN parameter")
        if t.dtype != torch.float32:
            raise PnxError("PFN parameters must be fp32")
    if tuple(w0.shape) != (32, F + 5) or tuple(w1.shape) != (64, 64):
        raise PnxError(f"PFN weights {tuple(w0.shape)}, {tuple(w1.shape)}: kernels are built for num_filters=[64, 64] only")
    check(lib().pnx_pfn_fold_bn(F, *[ptr(t) for t in ts[:5]], *[ptr(t) for t in ts[5:]], ctypes.c_float(eps), ptr(out), stream_ptr()),
          "pnx_pfn_fold_bn")
    return out


def reader_forward(points, batch, geom, folded, ws, canvas=None, canvas_layout=PNX_NHWC, occupancy=None, feat_max=None, coords=None,
                   unq_inv=None, pillar_of_point=None, counts=None):
    _need_cuda(points, "points")
    if points.dtype != torch.float32 or points.dim() != 2:
        raise PnxError("points must be (N, 1+F) fp32")
    n, stride = points.shape
    nbytes = lib().pnx_reader_workspace_bytes(n, batch, ctypes.byref(geom))
    buf = ws.get(nbytes, points.device)
    cap = 0
    if feat_max is not None:
        cap = feat_max.shape[0]
    if coords is not None:
        cap = coords.shape[0] if cap == 0 else min(cap, coords.shape[0])
    cdt = _DT[canvas.dtype] if canvas is not None else PNX_F32
    check(lib().pnx_reader_forward(ptr(points), n, stride, batch, ctypes.byref(geom), ptr(folded), ptr(canvas), cdt, canvas_layout,
                                   ptr(occupancy), ptr(feat_max), ptr(coords), cap, ptr(unq_inv), ptr(pillar_of_point), ptr(counts), ptr(buf),
                                   buf.numel(), stream_ptr()), "pnx_reader_forward")


def voxelize(points, batch, geom, ws, features=None, coords=None, unq_inv=None, pillar_of_point=None, counts=None):
    _need_cuda(points, "points")
    n, stride = points.shape
    nbytes = lib().pnx_reader_workspace_bytes(n, batch, ctypes.byref(geom))
    buf = ws.get(nbytes, points.device)
    cap = coords.shape[0] if coords is not None else 0
    check(lib().pnx_voxelize(ptr(points), n, stride, batch, ctypes.byref(geom), ptr(features), ptr(coords), cap, ptr(unq_inv),
                             ptr(pillar_of_point), ptr(counts), ptr(buf), buf.numel(), stream_ptr()), "pnx_voxelize")


def scatter_canvas(feat_max, coords, num_pillars_dev, batch, gy, gx, canvas, layout=PNX_NHWC):
    _need_cuda(feat_max, "feat_max")
    check(lib().pnx_scatter_canvas(ptr(feat_max), ptr(coords), ptr(num_pillars_dev), feat_max.shape[0], batch, gy, gx, ptr(canvas),
                                   _DT[canvas.dtype], layout, stream_ptr()), "pnx_scatter_canvas")


_SM_WS = Workspace()


class ScatterMax(torch.autograd.Function):
    """torch_scatter.scatter_max(x, index, dim=0)[0] with the argmax-routed gradient (pillar_encoder.py:43,180)."""

    @staticmethod
    def forward(ctx, x, index, num_pillars):
        _need_cuda(x, "x")
        x = x.float()
        n, C = x.shape
        out = torch.empty((num_pillars, C), dtype=torch.float32, device=x.device)
        arg = torch.empty((num_pillars, C), dtype=torch.int64, device=x.device)
        nbytes = lib().pnx_scatter_max_workspace_bytes(n, num_pillars)
        buf = _SM_WS.get(nbytes, x.device)
        check(lib().pnx_scatter_max(ptr(x), ptr(index), n, C, num_pillars, ptr(out), ptr(arg), ptr(buf), buf.numel(), stream_ptr()),
              "pnx_scatter_max")
        ctx.save_for_backward(arg)
        ctx.n = n
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, grad_out, _grad_arg):
        (arg,) = ctx.saved_tensors
        P, C = arg.shape
        g = grad_out.contiguous().float()
        gx = torch.empty((ctx.n, C), dtype=torch.float32, device=g.device)
        check(lib().pnx_scatter_max_backward(ptr(g), ptr(arg), ctx.n, C, P, ptr(gx), stream_ptr()), "pnx_scatter_max_backward")
        return gx, None, None


def scatter_max(x, index, num_pillars):
    return ScatterMax.apply(x.contiguous(), index.contiguous(), int(num_pillars))


# --------------------------------------------------------------------------------------------- voxel / multi-view readers (csrc/group.hip)
def group_geom(pc_range, voxel_size, mode, keep_range=None):
    """pnx_group_geom from the YAML lists: fp32 casts of min / voxel (what the reference applies, voxel_encoder.py:43-45), grid = np.round((max - min) /
    voxel) in fp64 (:40-41); keep_range (6 values) = MVFFeatureNet.forward's range mask on the raw x, y, z (mvf_encoder.py:290-297)."""
    import numpy as np

    pr, vs = np.asarray(pc_range, np.float64), np.asarray(voxel_size, np.float64)
    gs = (pr[3:] - pr[:3]) / vs
    gs = np.round(gs, 0, gs).astype(np.int64)
    g = _lib.PnxGroupGeom()
    for k in range(3):
        g.min[k], g.voxel[k], g.grid[k] = float(np.float32(pr[k])), float(np.float32(vs[k])), int(gs[k])
    g.mode, g.prefilter = int(mode), 0
    if keep_range is not None:
        g.prefilter = 1
        kr = torch.tensor([float(v) for v in keep_range], dtype=torch.float32)   # torch.tensor(self.pc_range, dtype=points.dtype): fp32 casts
        for k in range(3):
            g.keep_min[k], g.keep_max[k] = float(kr[k]), float(kr[3 + k])
    return g


_GROUP_WS = Workspace()


def group_points(points, batch, geom, want_features=True, want_mean=False, features_out=None):
    """pnx_group_points.  points (N, 1+F) fp32 CUDA.  Returns dict(features (N', C) or None, coords (G, 3|4) int32, unq_inv (N') int64,
    mean (G, M) or None, G, Nk) -- ONE host sync for the two counts (the reference's torch.unique syncs as well).  features_out = (buffer (>= N, ld)
    fp32, column offset): write the feature rows into columns [off, off + C) of an existing buffer (the concat of the two MVF views)."""
    _need_cuda(points, "points")
    if points.dtype != torch.float32 or points.dim() != 2:
        raise PnxError("points must be (N, 1+F) fp32")
    n, stride = points.shape
    dev = points.device
    voxel = geom.mode == _lib.PNX_GROUP_VOXEL
    C = stride - 1 if voxel else stride + 4
    M = stride - 1 if voxel else 3
    cells = batch * geom.grid[0] * geom.grid[1] * (geom.grid[2] if voxel else 1)
    cap = max(min(n, cells), 1)
    feats, ld, fptr = None, 0, None
    if features_out is not None:
        buf, off = features_out
        if not (buf.is_cuda and buf.dtype == torch.float32 and buf.dim() == 2 and buf.is_contiguous() and buf.shape[0] >= n and off + C <= buf.shape[1]):
            raise PnxError("group_points: features_out must be a contiguous fp32 (>= N, ld) buffer with room for the columns")
        feats, ld, fptr = buf, buf.shape[1], ctypes.c_void_p(buf.data_ptr() + 4 * off)
    elif want_features:
        feats = torch.empty((max(n, 1), C), dtype=torch.float32, device=dev)
        ld, fptr = C, ptr(feats)
    coords = torch.empty((cap, 4 if voxel else 3), dtype=torch.int32, device=dev)
    inv = torch.empty((max(n, 1),), dtype=torch.int64, device=dev)
    mean = torch.empty((cap, M), dtype=torch.float32, device=dev) if want_mean else None
    counts = torch.zeros((2,), dtype=torch.int32, device=dev)
    nbytes = lib().pnx_group_workspace_bytes(n, stride, batch, ctypes.byref(geom))
    if nbytes == 0:
        raise PnxError("group_points: bad geometry")
    ws = _GROUP_WS.get(nbytes, dev)
    check(lib().pnx_group_points(ptr(points), n, stride, batch, ctypes.byref(geom), fptr, ld, ptr(coords), cap, ptr(inv), ptr(mean), ptr(counts), ptr(ws),
                                 ws.numel(), stream_ptr()), "pnx_group_points")
    G, Nk = (int(v) for v in counts.tolist())
    return {"features": None if feats is None else (feats if features_out is not None else feats[:Nk]), "coords": coords[:G], "unq_inv": inv[:Nk],
            "mean": None if mean is None else mean[:G], "G": G, "Nk": Nk}


def pfn_layer_eval(xa, gb, inv, wt, shift, num_groups, store=True, want_max=True):
    """pnx_pfn_layer_eval: relu(W' [xa | gb[inv]] + shift) per point (returned when store) and its per-cell maximum (num_groups, cout) (when want_max).
    xa (N, ca) fp32 -- may be a column slice of a wider contiguous buffer; gb (G, cb) fp32 or None; wt (ca + cb, cout) = W' transposed."""
    _need_cuda(wt, "wt")
    n = xa.shape[0]
    ca, cb, cout = xa.shape[1], 0 if gb is None else gb.shape[1], wt.shape[1]
    if not (xa.is_cuda and xa.dtype == torch.float32 and (n == 0 or xa.stride(1) == 1) and wt.shape[0] == ca + cb and wt.dtype == torch.float32 and shift.numel() == cout):
        raise PnxError("pfn_layer_eval: xa (N, ca) fp32 with unit column stride, wt (ca + cb, cout) fp32, shift (cout)")
    if gb is not None:
        _need_cuda(gb, "gb")
    y = torch.empty((n, cout), dtype=torch.float32, device=xa.device) if store else None
    gmax = torch.empty((num_groups, cout), dtype=torch.float32, device=xa.device) if want_max else None
    check(lib().pnx_pfn_layer_eval(ptr(xa), xa.stride(0) if n > 1 else max(ca, 1), ca, ptr(gb), cb, ptr(inv), ptr(wt), ptr(shift), cout, n, num_groups, ptr(y), cout,
                                   ptr(gmax), stream_ptr()), "pnx_pfn_layer_eval")
    return y, gmax


def bilinear_gather(image, pos, pos_min, pos_voxel, cell_coords, unq_inv, ds_rate):
    """pnx_bilinear_gather: image (B, C, H, W) channels_last fp32 / bf16 / fp16; pos (N, >= 2) fp32 columns (may be a slice of a wider buffer); -> (N, C) fp32."""
    if not (image.is_cuda and image.dim() == 4 and image.is_contiguous(memory_format=torch.channels_last) and image.dtype in _DT):
        raise PnxError("bilinear_gather needs a channels_last fp32 / bf16 / fp16 CUDA map")
    if not (pos.is_cuda and pos.dtype == torch.float32 and pos.stride(1) == 1 and cell_coords.dtype == torch.int32 and unq_inv.dtype == torch.int64):
        raise PnxError("bilinear_gather: pos fp32 rows, int32 coords, int64 unq_inv")
    B, C, H, W = image.shape
    n = pos.shape[0]
    out = torch.empty((n, C), dtype=torch.float32, device=image.device)
    mn = (ctypes.c_float * 2)(float(pos_min[0]), float(pos_min[1]))
    vs = (ctypes.c_float * 2)(float(pos_voxel[0]), float(pos_voxel[1]))
    check(lib().pnx_bilinear_gather(ptr(image), _DT[image.dtype], B, H, W, C, ptr(pos), pos.stride(0) if n > 1 else 2, mn, vs, ptr(cell_coords.contiguous()),
                                    ptr(unq_inv), int(ds_rate), n, ptr(out), C, stream_ptr()), "pnx_bilinear_gather")
    return out


_BILGRAD_WS = Workspace()


def bilinear_gather_backward(grad_out, image_shape, pos, pos_min, pos_voxel, cell_coords, unq_inv, ds_rate):
    """pnx_bilinear_gather_backward: grad_out (N, C) fp32 with unit column stride (a column slice of a wider buffer is read in place), image_shape
    (B, C, H, W), the other arguments as bilinear_gather's -> the gradient of the map, (B, C, H, W) channels_last fp32, fully written.  Deterministic."""
    B, C, H, W = (int(v) for v in image_shape)
    n = pos.shape[0]
    if not (grad_out.dtype == torch.float32 and grad_out.dim() == 2 and tuple(grad_out.shape) == (n, C) and (n == 0 or grad_out.stride(1) == 1 or C == 1)
            and (n <= 1 or grad_out.stride(0) >= C)):
        raise PnxError("bilinear_gather_backward: grad_out (N, C) fp32 rows with unit column stride and a row stride >= C")
    if not (pos.dtype == torch.float32 and pos.dim() == 2 and pos.shape[1] >= 2 and pos.stride(1) == 1 and cell_coords.dtype == torch.int32
            and unq_inv.dtype == torch.int64 and unq_inv.shape[0] == n):
        raise PnxError("bilinear_gather_backward: pos fp32 rows, int32 coords, int64 unq_inv")
    ds = int(ds_rate)
    if ds < 1 or ds & (ds - 1):
        raise PnxError(f"bilinear_gather_backward: ds_rate {ds_rate} is not a power of two")
    if not (grad_out.is_cuda and pos.is_cuda and cell_coords.is_cuda and unq_inv.is_cuda):
        raise PnxError("bilinear_gather_backward needs CUDA (ROCm) tensors; there is no CPU implementation")
    nbytes = lib().pnx_bilinear_gather_backward_workspace_bytes(n, B, H, W)
    if nbytes == 0:
        raise PnxError("bilinear_gather_backward: point or cell count beyond 32-bit indices")
    out = torch.empty((B, H, W, C), dtype=torch.float32, device=grad_out.device)
    ws = _BILGRAD_WS.get(nbytes, grad_out.device)
    mn = (ctypes.c_float * 2)(float(pos_min[0]), float(pos_min[1]))
    vs = (ctypes.c_float * 2)(float(pos_voxel[0]), float(pos_voxel[1]))
    check(lib().pnx_bilinear_gather_backward(ptr(grad_out), grad_out.stride(0) if n > 1 else C, B, H, W, C, ptr(pos), pos.stride(0) if n > 1 else 2, mn, vs,
                                             ptr(cell_coords.contiguous()), ptr(unq_inv.contiguous()), ds, n, ptr(out), ptr(ws), ws.numel(), stream_ptr()),
          "pnx_bilinear_gather_backward")
    return out.permute(0, 3, 1, 2)


class BilinearGather(torch.autograd.Function):
    """bilinear_gather with a gradient for the map (training): forward = the eval kernel, backward = bilinear_gather_backward, cast to the map's dtype.
    pos and the index tensors get no gradient."""

    @staticmethod
    def forward(ctx, image, pos, pos_min, pos_voxel, cell_coords, unq_inv, ds_rate):
        ctx.save_for_backward(pos, cell_coords, unq_inv)
        ctx.geom = (tuple(image.shape), image.dtype, pos_min, pos_voxel, ds_rate)
        return bilinear_gather(image, pos, pos_min, pos_voxel, cell_coords, unq_inv, ds_rate)

    @staticmethod
    def backward(ctx, grad_out):
        pos, cell_coords, unq_inv = ctx.saved_tensors
        shape, dtype, pos_min, pos_voxel, ds_rate = ctx.geom
        g = grad_out
        if g.dtype != torch.float32 or g.shape[0] > 0 and (g.stride(1) != 1 or g.shape[0] > 1 and g.stride(0) < g.shape[1]):
            g = g.float().contiguous()          # an expanded or transposed gradient; the column slice torch.cat's backward hands over is read in place
        gi = bilinear_gather_backward(g, shape, pos, pos_min, pos_voxel, cell_coords, unq_inv, ds_rate)
        return gi.to(dtype), None, None, None, None, None, None


def _sp3_bilinear_args(what, ix, pos, cell_coords, unq_inv, ds_rate):
    if len(ix.grid) != 3 or ix.grid[0] != 1:
        raise PnxError(f"{what}: the set must lie over a grid (1, H, W), got {ix.grid}")
    if not (pos.dtype == torch.float32 and pos.dim() == 2 and pos.shape[1] >= 2 and pos.stride(1) == 1 and cell_coords.dtype == torch.int32
            and unq_inv.dtype == torch.int64 and unq_inv.shape[0] == pos.shape[0]):
        raise PnxError(f"{what}: pos fp32 rows, int32 coords, int64 unq_inv")
    if not (pos.is_cuda and cell_coords.is_cuda and unq_inv.is_cuda):
        raise PnxError(f"{what} needs CUDA (ROCm) tensors; there is no CPU implementation")
    ds = int(ds_rate)
    if ds < 1 or ds & (ds - 1):
        raise PnxError(f"{what}: ds_rate {ds_rate} is not a power of two")
    return ds


def sp3_bilinear_gather(rows, ix, pos, pos_min, pos_voxel, cell_coords, unq_inv, ds_rate):
    """pnx_sp3_bilinear_gather: bilinear_gather on the rows (n_rows, C) fp32 of the active set indexed by ix (an Sp3Index over grid (1, H, W)) instead
    of a dense map -> (N, C) fp32, equal to bilinear_gather on the map scattered from the rows."""
    _need_cuda(rows, "rows")
    if rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[1] < 1:
        raise PnxError("sp3_bilinear_gather: rows must be (n_rows, C) fp32")
    ds = _sp3_bilinear_args("sp3_bilinear_gather", ix, pos, cell_coords, unq_inv, ds_rate)
    n, C = pos.shape[0], rows.shape[1]
    out = torch.empty((n, C), dtype=torch.float32, device=rows.device)
    mn = (ctypes.c_float * 2)(float(pos_min[0]), float(pos_min[1]))
    vs = (ctypes.c_float * 2)(float(pos_voxel[0]), float(pos_voxel[1]))
    check(lib().pnx_sp3_bilinear_gather(ptr(rows), rows.shape[0], C, ptr(ix.buf), ix.nbytes, ix.batch, ix.grid[1], ix.grid[2], ptr(pos),
                                        pos.stride(0) if n > 1 else 2, mn, vs, ptr(cell_coords.contiguous()), ptr(unq_inv.contiguous()), ds, n, ptr(out), C,
                                        stream_ptr()), "pnx_sp3_bilinear_gather")
    return out


def sp3_bilinear_gather_backward(grad_out, coords, ix, pos, pos_min, pos_voxel, cell_coords, unq_inv, ds_rate):
    """pnx_sp3_bilinear_gather_backward: grad_out (N, C) fp32 with unit column stride (a column slice is read in place), coords (n_rows, 4) int32
    [b, 0, y, x] = the rows of the set ix indexes -> the gradient of the rows (n_rows, C) fp32, fully written: bilinear_gather_backward's map read
    at coords, bit for bit.  Deterministic."""
    _need_coords(coords)
    ds = _sp3_bilinear_args("sp3_bilinear_gather_backward", ix, pos, cell_coords, unq_inv, ds_rate)
    n = pos.shape[0]
    if not (grad_out.is_cuda and grad_out.dtype == torch.float32 and grad_out.dim() == 2 and grad_out.shape[0] == n and grad_out.shape[1] >= 1):
        raise PnxError("sp3_bilinear_gather_backward: grad_out (N, C) fp32 CUDA rows")
    C = grad_out.shape[1]
    if not ((n == 0 or grad_out.stride(1) == 1 or C == 1) and (n <= 1 or grad_out.stride(0) >= C)):
        raise PnxError("sp3_bilinear_gather_backward: grad_out needs unit column stride and a row stride >= C")
    n_rows = coords.shape[0]
    nbytes = lib().pnx_sp3_bilinear_gather_backward_scratch_bytes(n, n_rows)
    if nbytes == 0:
        raise PnxError("sp3_bilinear_gather_backward: point or row count beyond 32-bit indices")
    out = torch.empty((n_rows, C), dtype=torch.float32, device=grad_out.device)
    ws = _BILGRAD_WS.get(nbytes, grad_out.device)
    mn = (ctypes.c_float * 2)(float(pos_min[0]), float(pos_min[1]))
    vs = (ctypes.c_float * 2)(float(pos_voxel[0]), float(pos_voxel[1]))
    check(lib().pnx_sp3_bilinear_gather_backward(ptr(grad_out), grad_out.stride(0) if n > 1 else C, ptr(coords), n_rows, ix.batch, ix.grid[1], ix.grid[2], C,
                                                 ptr(pos), pos.stride(0) if n > 1 else 2, mn, vs, ptr(cell_coords.contiguous()), ptr(unq_inv.contiguous()),
                                                 ds, n, ptr(out), ptr(ws), ws.numel(), stream_ptr()), "pnx_sp3_bilinear_gather_backward")
    return out


class SparseBilinearGather(torch.autograd.Function):
    """sp3_bilinear_gather with a gradient for the rows (sp3_bilinear_gather_backward).  pos and the index tensors get none."""

    @staticmethod
    def forward(ctx, rows, coords, ix, pos, pos_min, pos_voxel, cell_coords, unq_inv, ds_rate):
        ctx.save_for_backward(coords, pos, cell_coords, unq_inv)
        ctx.geom = (ix, pos_min, pos_voxel, ds_rate)
        return sp3_bilinear_gather(rows.contiguous(), ix, pos, pos_min, pos_voxel, cell_coords, unq_inv, ds_rate)

    @staticmethod
    def backward(ctx, grad_out):
        coords, pos, cell_coords, unq_inv = ctx.saved_tensors
        ix, pos_min, pos_voxel, ds_rate = ctx.geom
        g = grad_out
        if g.dtype != torch.float32 or g.shape[0] > 0 and (g.stride(1) != 1 or g.shape[0] > 1 and g.stride(0) < g.shape[1]):
            g = g.float().contiguous()          # an expanded or transposed gradient; the column slice torch.cat's backward hands over is read in place
        return sp3_bilinear_gather_backward(g, coords, ix, pos, pos_min, pos_voxel, cell_coords, unq_inv, ds_rate), None, None, None, None, None, None, None, None


# --------------------------------------------------------------------------------------------- per-point training layer (csrc/point_layer_train.hip)
_PL_WS = Workspace()


def _rows_in_place(t):
    """fp32 rows with unit column stride and a row stride >= the width (a column slice of a wider buffer), else a contiguous copy."""
    if t.dtype != torch.float32:
        t = t.float()
    n, c = t.shape
    if n > 0 and (t.stride(1) != 1 and c > 1 or n > 1 and t.stride(0) < c):
        t = t.contiguous()
    return t


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)


class PointLayer(torch.autograd.Function):
    """Linear(bias=False) + BatchNorm1d with batch statistics + ReLU [+ per-cell maximum] over a list of points, forward and backward on
    csrc/point_layer_train.hip.  forward(x (n, cin), weight (cout, cin), gamma, beta, inv (n) int64 or None, num_groups, want_y, want_max, eps, norm)
    -> (y (n, cout) or None, gmax (num_groups, cout) or None, argmax int64 or None).  `norm` (or None) is the module whose running statistics
    advance by BatchNorm1d's rule.  Saved for the backward: the inputs, the arg-max rows and 2 x cout statistics -- no (n, cout) tensor; the backward
    recomputes x W^T.  Computes in fp32 under autocast."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, weight, gamma, beta, inv, num_groups, want_y, want_max, eps, norm):
        if not (x.is_cuda and weight.is_cuda and x.dim() == 2 and weight.dim() == 2 and x.shape[1] == weight.shape[1]):
            raise PnxError("point_layer: x (n, cin) and weight (cout, cin) CUDA (ROCm) tensors; there is no CPU implementation")
        if not (want_y or want_max):
            raise PnxError("point_layer: neither y nor the per-cell maximum requested")
        n, cin = x.shape
        cout = weight.shape[0]
        if n < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {x.shape}")
        x, w = _rows_in_place(x), weight.detach().float().contiguous()
        ga, be = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        dev = x.device
        G = 0
        if want_max:
            if inv is None or num_groups is None or inv.dtype != torch.int64 or inv.shape[0] != n:
                raise PnxError("point_layer: the per-cell maximum needs inv (n) int64 and num_groups")
            inv, G = inv.contiguous(), int(num_groups)
        nbytes = lib().pnx_point_layer_workspace_bytes(n, cin, cout, 0)
        if nbytes == 0:
            raise PnxError(f"point_layer: {cin} -> {cout} channels over {n} rows is not served (cin <= 576, cout <= 256)")
        ws = _PL_WS.get(nbytes, dev)
        sums = torch.empty((2, cout), dtype=torch.float64, device=dev)
        check(lib().pnx_point_layer_stats(ptr(x), _ld(x), n, cin, ptr(w), cout, ptr(sums), ptr(ws), ws.numel(), stream_ptr()), "pnx_point_layer_stats")
        # the seam: under SyncBatchNorm `sums` (and n) is what the ranks would all-reduce
        mean = sums[0] / n
        var = (sums[1] / n - mean * mean).clamp_(min=0.0)
        invstd = torch.rsqrt(var + eps)
        prm = torch.zeros((6, cout), dtype=torch.float32, device=dev)
        prm[0], prm[1], prm[2], prm[3] = mean, invstd, ga, be
        y = torch.empty((n, cout), dtype=torch.float32, device=dev) if want_y else None
        gmax = torch.empty((G, cout), dtype=torch.float32, device=dev) if want_max else None
        arg = torch.empty((G, cout), dtype=torch.int64, device=dev) if want_max else None
        check(lib().pnx_point_layer_forward(ptr(x), _ld(x), n, cin, ptr(w), cout, ptr(prm), ptr(inv) if want_max else None, G, ptr(y), cout, ptr(gmax), ptr(arg),
                                            stream_ptr()), "pnx_point_layer_forward")
        if norm is not None and norm.training and norm.track_running_stats and norm.running_mean is not None:
            norm.num_batches_tracked.add_(1)
            f = 1.0 / float(norm.num_batches_tracked) if norm.momentum is None else float(norm.momentum)
            norm.running_mean.mul_(1.0 - f).add_((mean * f).to(norm.running_mean.dtype))
            norm.running_var.mul_(1.0 - f).add_((var * (f * n / (n - 1.0))).to(norm.running_var.dtype))
        ctx.save_for_backward(x, w, prm, inv if want_max else None, arg)
        ctx.flags = (bool(want_y), bool(want_max), G)
        if arg is not None:
            ctx.mark_non_differentiable(arg)
        return y, gmax, arg

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dy, dgmax, _darg):
        x, w, prm, inv, arg = ctx.saved_tensors
        want_y, want_max, G = ctx.flags
        n, cin = x.shape
        cout = w.shape[0]
        dev = x.device
        dy = _rows_in_place(dy) if want_y and dy is not None else None
        dgmax = dgmax.float().contiguous() if want_max and dgmax is not None else None
        if dy is None and dgmax is None:
            return (None,) * 10
        nbytes = lib().pnx_point_layer_workspace_bytes(n, cin, cout, 1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)       # holds dxpre (n, cout): a transient of this call, not kept
        sums = torch.empty((2, cout), dtype=torch.float64, device=dev)
        grad = (ptr(dy), _ld(dy) if dy is not None else cout, ptr(inv) if dgmax is not None else None, G, ptr(dgmax), ptr(arg) if dgmax is not None else None)
        check(lib().pnx_point_layer_backward_stats(ptr(x), _ld(x), n, cin, ptr(w), cout, ptr(prm), *grad, ptr(sums), ptr(ws), ws.numel(), stream_ptr()),
              "pnx_point_layer_backward_stats")
        prm = prm.clone()
        prm[4], prm[5] = sums[0] / n, sums[1] / n
        dx = torch.empty((n, cin), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        dw = torch.empty((cout, cin), dtype=torch.float32, device=dev)
        check(lib().pnx_point_layer_backward(ptr(x), _ld(x), n, cin, ptr(w), cout, ptr(prm), *grad, ptr(dx), cin, ptr(dw), ptr(ws), ws.numel(), stream_ptr()),
              "pnx_point_layer_backward")
        return dx, dw, sums[1].float(), sums[0].float(), None, None, None, None, None, None


def point_layer(x, linear, norm, inv=None, num_groups=None, want_y=True, want_max=False):
    """relu(norm(linear(x))) with batch statistics on the fused training node (PointLayer) -> (y or None, gmax or None): y (n, cout) when want_y, the
    per-cell maximum gmax (num_groups, cout) over inv when want_max.  linear: nn.Linear without bias; norm: BatchNorm1d (or a SyncBatchNorm in a world
    of one process), whose running statistics advance.  CUDA tensors only; fewer than two rows raise what BatchNorm1d raises."""
    if linear.bias is not None:
        raise PnxError("point_layer: the Linear must have no bias")
    if norm.weight is None or norm.bias is None:
        raise PnxError("point_layer: the norm must be affine")
    y, gmax, _ = PointLayer.apply(x, linear.weight, norm.weight, norm.bias, inv, num_groups, want_y, want_max, float(norm.eps), norm)
    return y, gmax


def point_layer_serves(module, norm):
    """Does the fused training node stand in for `module`'s Linear + norm + ReLU?  PNX_TRAIN_POINT_HIP on, training mode, and a plain BatchNorm1d --
    or a SyncBatchNorm while the world is one process (with more it needs the collective the node does not issue: torch keeps it)."""
    from torch import nn

    from .switches import on

    if not (on("PNX_TRAIN_POINT_HIP") and module.training and norm.training):
        return False
    if type(norm) is nn.BatchNorm1d:
        return True
    if isinstance(norm, nn.SyncBatchNorm):
        import torch.distributed as dist

        return not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() <= 1
    return False


# --------------------------------------------------------------------------------------------- IoU / NMS
def _boxes(t, name):
    _need_cuda(t, name)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 7:
        raise PnxError(f"{name} must be (N, 7) fp32")


def boxes_overlap_bev(a, b, out):
    _boxes(a, "boxes_a"), _boxes(b, "boxes_b"), _need_cuda(out, "out")
    check(lib().pnx_boxes_overlap_bev(ptr(a), a.shape[0], ptr(b), b.shape[0], ptr(out), stream_ptr()), "pnx_boxes_overlap_bev")


def boxes_iou_bev(a, b, out):
    _boxes(a, "boxes_a"), _boxes(b, "boxes_b"), _need_cuda(out, "out")
    check(lib().pnx_boxes_iou_bev(ptr(a), a.shape[0], ptr(b), b.shape[0], ptr(out), stream_ptr()), "pnx_boxes_iou_bev")


def boxes_aligned_overlap_bev(a, b, out):
    _boxes(a, "boxes_a"), _boxes(b, "boxes_b"), _need_cuda(out, "out")
    if a.shape[0] != b.shape[0]:
        raise PnxError("aligned overlap needs equally many boxes")
    check(lib().pnx_boxes_aligned_overlap_bev(ptr(a), ptr(b), a.shape[0], ptr(out), stream_ptr()), "pnx_boxes_aligned_overlap_bev")


def boxes_aligned_iou3d(a, b):
    _boxes(a, "boxes_a"), _boxes(b, "boxes_b")
    if a.shape[0] != b.shape[0]:
        raise PnxError("aligned IoU needs equally many boxes")
    out = torch.empty((a.shape[0], 1), dtype=torch.float32, device=a.device)
    check(lib().pnx_boxes_aligned_iou3d(ptr(a), ptr(b), a.shape[0], ptr(out), stream_ptr()), "pnx_boxes_aligned_iou3d")
    return out


_NMS_WS = Workspace()


def nms_batched(boxes, seg_offsets, thresh, max_seg_len, post_max=0, rotated=True, seg_len=None):
    """boxes (T,7) score-sorted inside each segment; seg_offsets int32 (S+1) device; thresh fp32 (S) device.
    Returns keep (T) int32 [segment-local indices, ascending, first keep_count[s] valid per segment] and keep_count (S)."""
    _boxes(boxes, "boxes")
    S = seg_offsets.numel() - 1
    T = boxes.shape[0]
    keep = torch.empty((max(T, 1),), dtype=torch.int32, device=boxes.device)
    cnt = (torch.empty if S > 0 and max_seg_len > 0 else torch.zeros)((max(S, 1),), dtype=torch.int32, device=boxes.device)   # the greedy scan writes every segment's count
    nbytes = lib().pnx_nms_workspace_bytes(T, S, max_seg_len)
    buf = _NMS_WS.get(nbytes, boxes.device)
    fn = lib().pnx_nms_rotated_batched if rotated else lib().pnx_nms_normal_batched
    check(fn(ptr(boxes), ptr(seg_offsets), ptr(seg_len), S, int(max_seg_len), ptr(thresh), int(post_max), ptr(keep), ptr(cnt), ptr(buf), buf.numel(),
             stream_ptr()), "pnx_nms_batched")
    return keep, cnt


def nms_single(boxes, thresh, rotated=True, post_max=0):
    """One score-sorted list -> (keep int32 device tensor, count python int). Syncs once, like nms_gpu does."""
    n = boxes.shape[0]
    if n == 0:
        return torch.empty((0,), dtype=torch.int32, device=boxes.device), 0
    off = torch.tensor([0, n], dtype=torch.int32, device=boxes.device)
    thr = torch.tensor([float(thresh)], dtype=torch.float32, device=boxes.device)
    keep, cnt = nms_batched(boxes, off, thr, n, post_max, rotated)
    k = int(cnt[0].item())
    return keep[:k], k


# --------------------------------------------------------------------------------------------- dense epilogue
def bias_act_mask_(x, bias, mask=None, residual=None, relu=True):
    """In place on a channels_last bf16 / fp16 (B,C,H,W) tensor: x = [relu](x + bias[c] [+ residual]) * mask[b,h,w];
    relu=2: (relu(x + bias[c]) + residual) * mask."""
    if not (x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and x.is_contiguous(memory_format=torch.channels_last)):
        raise PnxError("bias_act_mask_ needs a channels_last bf16 / fp16 CUDA tensor")
    B, C, H, W = x.shape
    if residual is not None and not (residual.dtype == x.dtype and residual.shape == x.shape and residual.is_contiguous(memory_format=torch.channels_last)):
        raise PnxError("residual must match x (dtype, channels_last)")
    check(lib().pnx_bias_act_mask(ptr(x), ptr(residual), ptr(bias), ptr(mask), ptr(x), B * H * W, C, _DT[x.dtype], int(relu), stream_ptr()),
          "pnx_bias_act_mask")
    return x


def sum_bias_act(parts, bias, relu=True):
    """[relu](sum(parts) + bias[c]) for channels_last bf16 (B,C,H,W) tensors of one shape, summed in fp32 in one pass."""
    x = parts[0]
    for t in parts:
        if not (t.is_cuda and t.dtype in (torch.bfloat16, torch.float16) and t.dtype == x.dtype and t.shape == x.shape
                and t.is_contiguous(memory_format=torch.channels_last)):
            raise PnxError("sum_bias_act needs channels_last bf16 / fp16 CUDA tensors of one shape and dtype")
    B, C, H, W = x.shape
    out = torch.empty_like(x, memory_format=torch.channels_last)
    arr = (ctypes.c_void_p * len(parts))(*[t.data_ptr() for t in parts])
    check(lib().pnx_sum_bias_act(arr, len(parts), ptr(bias), ptr(out), B * H * W, C, _DT[x.dtype], 1 if relu else 0, stream_ptr()), "pnx_sum_bias_act")
    return out


# The five calls a launch table can hold (plan.py) check their arguments in the helpers below, which the eager wrapper and the table
# builder of a call share.  They read shapes, dtypes and layouts only, so CPU tensors and plan.Dyn slots pass; that a tensor lives on
# the GPU is asked by the wrappers here and by LaunchPlan.run().
def _like(a):
    """The tensor itself, or the tensor a plan.Dyn slot stands for."""
    return getattr(a, "like", a)


def _out_hw(H, W, stride):
    """Extent of a 3x3 / stride / pad-1 window's output."""
    return (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1


def mask_pool3_out(mask, stride, out=None):
    """The uint8 (B,Ho,Wo) tensor mask_pool3(mask, stride) writes: `out` if it is one, a new one without."""
    B, H, W = _like(mask).shape
    if out is None:
        return torch.empty((B, *_out_hw(H, W, stride)), dtype=torch.uint8, device=mask.device)
    if tuple(_like(out).shape) != (B, *_out_hw(H, W, stride)) or _like(out).dtype != torch.uint8:
        raise PnxError("mask_pool3: the output must be uint8 (B, Ho, Wo)")
    return out


def mask_pool3(mask, stride):
    """uint8 (B,H,W) occupancy -> occupancy after a 3x3/stride/pad-1 sparse conv."""
    B, H, W = mask.shape
    out = mask_pool3_out(mask, stride)
    check(lib().pnx_mask_pool3(ptr(mask), B, H, W, stride, ptr(out), stream_ptr()), "pnx_mask_pool3")
    return out


# (Cin, Cout) pairs pnx_conv3x3_bf16 has kernels for.  Stride 1: backbone blocks, + the merged SepHead branches (5/6/7 x 64).
# Stride 2: the entry convolutions of backbone stages 1-3 (no residual).
CONV3X3_SHAPES_S1 = {(64, 64), (64, 128), (128, 128), (256, 256), (256, 64), (64, 320), (64, 384), (64, 448)}
CONV3X3_SHAPES_S2 = {(64, 64), (64, 128), (128, 128), (128, 256), (256, 256)}


_HALF = (torch.bfloat16, torch.float16)   # element types of the convolution kernels (csrc/conv3x3.hip is built for both)


def _half_nhwc(x, what, dtype=None, cuda=False):
    """channels_last bf16 / fp16 (of `dtype`, where given: a convolution call runs in one element type); cuda: and on the GPU."""
    x = _like(x)
    if cuda and not x.is_cuda:
        raise PnxError(f"{what} needs a CUDA (ROCm) tensor; the convolutions have no CPU implementation")
    if not (x.dtype in _HALF and x.dtype == (dtype or x.dtype) and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)):
        raise PnxError(f"{what} needs a channels_last bf16 / fp16 tensor" + (" of the input's dtype" if dtype else ""))
    return x


def _conv_dims(what, x, wfrag, y, cout, scale, cuda=False):
    """deconv2x2 / sephead_out: -> (B, H, W, Cin, PNX_BF16 / PNX_F16); y, where given, is the (B, cout, scale*H, scale*W) output."""
    xs = _half_nhwc(x, what, cuda=cuda)
    B, ci, H, W = xs.shape
    if wfrag.dtype != xs.dtype or (y is not None and tuple(_half_nhwc(y, what + " output", xs.dtype).shape) != (B, cout, scale * H, scale * W)):
        raise PnxError(f"{what}: weights of another dtype than the input / output of the wrong shape")
    return B, H, W, ci, _DT[xs.dtype]


def _conv_fn(name, dtype):
    """The bf16 or IEEE-half entry point of a convolution call (pnx_<name>_bf16 / pnx_<name>_f16)."""
    return getattr(lib(), f"pnx_{name}_{'f16' if dtype == torch.float16 else 'bf16'}")


def conv3x3_pack_weights(w, transposed=False, dtype=torch.bfloat16):
    """(Cout, Cin, 3, 3) -> bf16 (or, dtype=torch.float16, fp16) MFMA-fragment order [tap][cin/16][cout/32][lane = kb*32 + n][8]  (csrc/conv3x3.hip).  transposed: the weights of
    the stride-1 data gradient instead, i.e. pack(w.flip(2, 3).transpose(0, 1)).  CUDA fp32 / bf16 weights take one HIP launch
    (pnx_conv3x3_pack_weights); anything else the torch statement below, which is also what the tests compare the kernel with."""
    co, ci = w.shape[:2]
    if dtype == torch.bfloat16 and w.is_cuda and w.dtype in (torch.float32, torch.bfloat16) and tuple(w.shape[2:]) == (3, 3) and co % 32 == 0 and ci % 32 == 0:
        wc = w.detach().contiguous()
        out = torch.empty((9 * co * ci,), dtype=torch.bfloat16, device=w.device)
        check(lib().pnx_conv3x3_pack_weights(ptr(wc), _DT[wc.dtype], co, ci, 1 if transposed else 0, ptr(out), stream_ptr()), "pnx_conv3x3_pack_weights")
        return out
    if transposed:
        w = w.flip(2, 3).transpose(0, 1)
        co, ci = ci, co
    v = w.detach().float().reshape(co // 32, 32, ci // 16, 2, 8, 3, 3)         # (mt, n, cb, kb, e, ky, kx)
    v = v.permute(5, 6, 2, 0, 3, 1, 4).contiguous()                               # (ky, kx, cb, mt, kb, n, e)
    return v.reshape(-1).to(dtype).contiguous()


def deconv2x2_pack_weights(w, dtype=torch.bfloat16):
    """ConvTranspose2d weight (Cin, Cout, 2, 2) -> bf16 / fp16 MFMA-fragment order [ky*2+kx][cin/16][cout/32][lane = kb*32 + n][8]."""
    ci, co = w.shape[:2]
    v = w.detach().float().permute(1, 0, 2, 3).reshape(co // 32, 32, ci // 16, 2, 8, 2, 2)   # (mt, n, cb, kb, e, ky, kx)
    v = v.permute(5, 6, 2, 0, 3, 1, 4).contiguous()                                          # (ky, kx, cb, mt, kb, n, e)
    return v.reshape(-1).to(dtype).contiguous()


def deconv2x2(x, wfrag, bias, cout, relu=True):
    """x (B,Cin,H,W) channels_last bf16 / fp16 -> [relu](conv_transpose2d(x, W, stride 2) + bias) as (B,Cout,2H,2W) channels_last, same dtype
    (wfrag packed in that dtype)."""
    B, H, W, ci, _ = _conv_dims("deconv2x2", x, wfrag, None, cout, 2, cuda=True)
    y = torch.empty((B, cout, 2 * H, 2 * W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    check(_conv_fn("deconv2x2", x.dtype)(ptr(x), ptr(wfrag), ptr(bias), ptr(y), B, H, W, ci, cout, 1 if relu else 0, stream_ptr()), "pnx_deconv2x2_bf16")
    return y


def sephead_pack_weights(w2, dtype=torch.bfloat16):
    """Block-diagonal (16, nb*64, 3, 3) -> bf16 / fp16 fragment order [branch][tap][kc][lane = q*16 + o][8]  (csrc/sephead.h::k_sephead_out)."""
    co, ci = w2.shape[:2]
    if co != 16 or ci % 64:
        raise PnxError("sephead_pack_weights wants a (16, nb*64, 3, 3) weight")
    v = w2.detach().float().reshape(16, ci // 64, 2, 4, 8, 3, 3)                # (o, j, kc, q, e, ky, kx)
    v = v.permute(1, 5, 6, 2, 3, 0, 4).contiguous()                               # (j, ky, kx, kc, q, o, e)
    return v.reshape(-1).to(dtype).contiguous()


def sephead_out(x, wfrag, bias):
    """x (B, nb*64, H, W) channels_last bf16 / fp16 -> (B, 16, H, W) channels_last, same dtype: the last 3x3 conv of every SepHead branch of a task."""
    B, H, W, ci, _ = _conv_dims("sephead_out", x, wfrag, None, 16, 1, cuda=True)
    y = torch.empty((B, 16, H, W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    check(_conv_fn("sephead_out", x.dtype)(ptr(x), ptr(wfrag), ptr(bias), ptr(y), B, H, W, ci // 64, stream_ptr()), "pnx_sephead_out_bf16")
    return y


def sephead_lazy_pack_w2(w2m):
    """(9*320, 10) matrix of the five regression branches' second convolutions (rows (pos, channel), block diagonal over the branches
    reg 2 | height 1 | dim 3 | rot 2 | vel 2) -> fp32 [M tile 10][pos 9][channel 32][3]: per 32-channel tile the <= 3 outputs of its branch."""
    off, k = [0, 2, 3, 6, 8], [2, 1, 3, 2, 2]
    v = w2m.detach().float().reshape(9, 10, 32, 10)                               # (pos, mt, cl, o)
    out = torch.zeros((10, 9, 32, 3), dtype=torch.float32, device=w2m.device)
    for mt in range(10):
        j = mt // 2
        out[mt, :, :, :k[j]] = v[:, mt, :, off[j]:off[j] + k[j]]
    return out.contiguous()


class _PnxLazyTask(ctypes.Structure):
    _fields_ = [("up", ctypes.c_void_p), ("wfrag1", ctypes.c_void_p), ("bias1", ctypes.c_void_p), ("w2c", ctypes.c_void_p), ("bias2", ctypes.c_void_p),
                ("h", ctypes.c_int32), ("w", ctypes.c_int32)]


def lazy_task_table(tasks, batch, dtype, shapes=None, arr=None):
    """The _PnxLazyTask row of every task (up, wfrag1, bias1, w2c, bias2), written into `arr` (a caller's persistent table) or a new one.
    Checks what k_sephead_lazy relies on: 64-channel channels_last CUDA maps of `batch` samples in ONE 16-bit dtype (the packed weights
    included) and, where shapes[t] = the tuple (H, W) is given, of the task's map shape."""
    if arr is None:
        arr = (_PnxLazyTask * len(tasks))()
    for t, (up, wf, b1, w2c, b2) in enumerate(tasks):
        if not (up.is_cuda and dtype in _HALF and up.dtype == dtype and wf.dtype == dtype and up.shape[1] == 64 and up.shape[0] == batch
                and up.is_contiguous(memory_format=torch.channels_last) and (shapes is None or tuple(up.shape[2:]) == shapes[t])):
            raise PnxError("sephead_lazy needs 64-channel channels_last bf16 / fp16 CUDA maps of one dtype (packed weights included), of the "
                           "batch and of the task's map shape")
        arr[t] = _PnxLazyTask(up.data_ptr(), wf.data_ptr(), b1.data_ptr(), w2c.data_ptr(), b2.data_ptr(), up.shape[2], up.shape[3])
    return arr


def sephead_lazy(tasks, class_task, batch, local, seg_len, pre_max):
    """The regression branches of every task at the candidate cells (csrc/sephead_lazy.h::k_sephead_lazy, one launch).
    tasks: list of (up (B,64,H,W) channels_last bf16 / fp16 (one dtype for all tasks), wfrag1 in that dtype, bias1, w2c, bias2); class_task: task index of every class (host list);
    local int64 (batch*len(class_task), pre_max) = b*H*W + cell per slot; seg_len int32 (batch*len(class_task),).  -> (lists, pre_max, 10) fp32,
    rows behind seg_len zero."""
    dt = tasks[0][0].dtype
    arr = lazy_task_table(tasks, batch, dt)
    nc = len(class_task)
    ct = (ctypes.c_int32 * nc)(*[int(v) for v in class_task])
    S = batch * nc
    if not (local.is_cuda and local.dtype == torch.int64 and local.numel() == S * pre_max and seg_len.dtype == torch.int32 and seg_len.numel() == S):
        raise PnxError("sephead_lazy: local must be int64 (lists*pre_max), seg_len int32 (lists)")
    local, seg_len = local.contiguous(), seg_len.contiguous()
    out = torch.empty((S, pre_max, 10), dtype=torch.float32, device=local.device)
    check(_conv_fn("sephead_lazy", dt)(arr, len(tasks), ct, nc, batch, ptr(local), ptr(seg_len), pre_max, ptr(out), stream_ptr()), "pnx_sephead_lazy_bf16")
    return out


# The weight-gradient kernels' partial sums: written and reduced inside one C call on one stream, so one buffer per stream serves every layer.  75 MB for
# every 3x3 layer whatever its channels: no headroom, or the step's peak memory grows by a quarter of that.
_PARTIALS_WS = Workspace(headroom=1.0)


# The training convolutions run on 1, 2 or 3 bf16 pieces per operand: one bf16 tensor (bf16 autocast), or the (hi, lo) / (hi, mid, lo) pieces of an fp32
# tensor (split_f32), most significant first.  The number of pieces picks the entry point; pieces give fp32 results.
_PIECES_TAG = {1: "bf16", 2: "x3", 3: "x6"}   # suffix of the entry points by pieces per operand (x3 / x6: the number of bf16 products)


def _pieces(t):
    return (t,) if isinstance(t, torch.Tensor) else tuple(t)


def _bf16_maps(tensors, what):
    """Validator: channels_last bf16 CUDA pieces of one shape."""
    for tns in tensors:
        if not (tns.is_cuda and tns.dtype == torch.bfloat16 and tns.dim() == 4 and tns.is_contiguous(memory_format=torch.channels_last)
                and tns.shape == tensors[0].shape):
            raise PnxError(f"{what} needs channels_last bf16 CUDA pieces of one shape")


def _bf16_packs(wfrags, n, what):
    """Validator: n packed bf16 weight pieces (conv3x3_pack_weights) of one size."""
    if len(wfrags) != n or any(w.dtype != torch.bfloat16 or w.numel() != wfrags[0].numel() for w in wfrags):
        raise PnxError(f"{what}: the weights must be {n} packed bf16 piece(s) of one size, one per piece of the other operand")


def split_f32(x, mask=None, pieces=2):
    """fp32 tensor -> `pieces` bf16 tensors of the same shape and memory layout, most significant first.  2: (hi, lo), hi = RNE(x), lo = RNE(x - hi)
    (pnx_split_f32).  3: (hi, mid, lo), mid = RNE(x - hi), lo = RNE(x - hi - mid) (pnx_split3_f32; hi + mid + lo == x exactly for finite |x| >= 2^-100).
    mask: uint8 (B,H,W) for a channels_last (B,C,H,W) x that is zero where mask is 0 -- those sites are not read."""
    if pieces not in (2, 3):
        raise PnxError(f"split_f32: 2 or 3 pieces, got {pieces!r}")
    if not (x.is_cuda and x.dtype == torch.float32 and x.numel() % 8 == 0):
        raise PnxError("split_f32 needs an fp32 CUDA tensor with a multiple of 8 elements")
    if not (x.is_contiguous() or (x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last))):
        raise PnxError("split_f32 needs a dense tensor (contiguous or channels_last)")
    c = 0
    if mask is not None:
        if not (x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) and mask.dtype == torch.uint8 and mask.is_contiguous()
                and tuple(mask.shape) == (x.shape[0], x.shape[2], x.shape[3]) and x.shape[1] % 8 == 0):
            raise PnxError("split_f32: mask needs a channels_last (B,C,H,W) tensor with C % 8 == 0 and a contiguous uint8 (B,H,W) mask")
        c = x.shape[1]
    out = tuple(torch.empty_like(x, dtype=torch.bfloat16) for _ in range(pieces))
    name = "pnx_split_f32" if pieces == 2 else "pnx_split3_f32"
    check(getattr(lib(), name)(ptr(x), *map(ptr, out), x.numel(), ptr(mask), c, stream_ptr()), name)
    return out


# stride -> (Cin, Cout) of the masked training kernels, the ONE statement of what they serve: pnx_conv3x3_x3 / _x6 (the fp32 graph) and, for bf16
# autocast, the LDS-staged kernels of pnx_conv3x3_bf16; stride 2 is also the set of pnx_conv3x3_dgrad_s2_*.  models.py derives its tables from this.
CONV3X3_X3_SHAPES = {1: {(64, 64), (128, 128), (256, 256)}, 2: {(64, 128), (128, 256), (256, 256)}}


def conv3x3_f32(x_pieces, wfrag_pieces, cout, stride, mask, bias=None):
    """fp32 (B,Cout,Ho,Wo) channels_last = masked 3x3 convolution of an fp32 x with an fp32 W, each given as 2 or 3 bf16 pieces (split_f32; the weight
    pieces packed by conv3x3_pack_weights), accumulated in fp32 in one launch [+ bias, fp32 (Cout,)].  2 pieces: the three products hi.hi + hi.lo + lo.hi
    (pnx_conv3x3_x3); 3 pieces: the six products of piece orders 0..2 (pnx_conv3x3_x6).  mask uint8 (B,Ho,Wo) of the OUTPUT sites or None (dense);
    zeros at inactive sites."""
    xs, ws = tuple(x_pieces), tuple(wfrag_pieces)
    if len(xs) not in (2, 3):
        raise PnxError(f"conv3x3_f32: 2 or 3 pieces per operand, got {len(xs)}")
    if bias is not None and not (bias.is_cuda and bias.dtype == torch.float32 and bias.numel() == cout and bias.is_contiguous()):
        raise PnxError("conv3x3_f32: bias must be a contiguous fp32 CUDA vector of Cout values")
    _bf16_maps(xs, "conv3x3_f32")
    _bf16_packs(ws, len(xs), "conv3x3_f32")
    B, ci, H, W = xs[0].shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if mask is not None and (tuple(mask.shape) != (B, Ho, Wo) or mask.dtype != torch.uint8):
        raise PnxError("conv3x3_f32: mask must be uint8 (B,Ho,Wo)")
    y = torch.empty((B, cout, Ho, Wo), dtype=torch.float32, device=xs[0].device, memory_format=torch.channels_last)
    name = "pnx_conv3x3_" + _PIECES_TAG[len(xs)]
    check(getattr(lib(), name)(*map(ptr, xs), *map(ptr, ws), ptr(bias), ptr(mask), ptr(y), B, H, W, ci, cout, stride, stream_ptr()), name)
    return y


def conv3x3_wgrad(x, dy, mask, stride=1):
    """Weight gradient (Cout, Cin, 3, 3) fp32 of the masked 3x3 convolution (pad 1, stride 1 or 2): sum over the sites of `mask` (B,Ho,Wo uint8,
    the OUTPUT's active set) of dy[p] (x) x[stride * p + tap] (csrc/conv_wgrad.hip).  Deterministic.  x, dy: one channels_last bf16 tensor each
    (pnx_conv3x3_wgrad_bf16), or equal-length tuples of the 2 or 3 bf16 pieces of fp32 tensors (split_f32): three or six products in one pass
    (pnx_conv3x3_wgrad_x3 / _x6)."""
    xs, gs = _pieces(x), _pieces(dy)
    if len(xs) not in _PIECES_TAG or len(gs) != len(xs):
        raise PnxError("conv3x3_wgrad: x and dy must be one bf16 tensor each or tuples of 2 or 3 pieces of equal length")
    _bf16_maps(xs, "conv3x3_wgrad: x")
    _bf16_maps(gs, "conv3x3_wgrad: dy")
    B, ci, H, W = xs[0].shape
    co = gs[0].shape[1]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if stride not in (1, 2) or tuple(gs[0].shape) != (B, co, Ho, Wo) or tuple(mask.shape) != (B, Ho, Wo) or mask.dtype != torch.uint8:
        raise PnxError("conv3x3_wgrad: stride 1 or 2, dy (B,Cout,Ho,Wo) and a uint8 (B,Ho,Wo) mask of the output sites")
    nbytes = int(lib().pnx_conv3x3_wgrad_workspace_bytes(ci, co))
    if nbytes == 0:
        raise PnxError(f"conv3x3_wgrad: no kernel for {ci} -> {co} channels")
    ws = _PARTIALS_WS.get(nbytes, xs[0].device)
    dw = torch.empty((co, ci, 3, 3), dtype=torch.float32, device=xs[0].device)
    name = "pnx_conv3x3_wgrad_" + _PIECES_TAG[len(xs)]
    check(getattr(lib(), name)(*map(ptr, xs), *map(ptr, gs), ptr(mask), ptr(dw), B, H, W, ci, co, stride, ptr(ws), ws.numel(), stream_ptr()), name)
    return dw


def conv3x3_dgrad_s2(g, wfrag_t, cin, in_hw, mask_in):
    """Data gradient (B,cin,H,W) channels_last of a stride-2 masked 3x3 convolution from the upstream gradient g (B,cout,Ho,Wo) channels_last bf16 and the
    TRANSPOSED weight pack (conv3x3_pack_weights(w, transposed=True)); mask_in uint8 (B,H,W): the layer's input active set, zeros outside it.  One tensor
    each: bf16 out (pnx_conv3x3_dgrad_s2_bf16).  Equal-length tuples of the 2 or 3 bf16 pieces of an fp32 g (split_f32) and of the fp32 weights: the
    three- or six-product form, fp32 out (pnx_conv3x3_dgrad_s2_x3 / _x6)."""
    gs, ws = _pieces(g), _pieces(wfrag_t)
    if len(gs) not in _PIECES_TAG:
        raise PnxError("conv3x3_dgrad_s2: g must be one bf16 tensor or a tuple of 2 or 3 pieces")
    _bf16_maps(gs, "conv3x3_dgrad_s2")
    _bf16_packs(ws, len(gs), "conv3x3_dgrad_s2")
    H, W = in_hw
    B, co, Ho, Wo = gs[0].shape
    if (Ho, Wo) != ((H - 1) // 2 + 1, (W - 1) // 2 + 1) or tuple(mask_in.shape) != (B, H, W) or mask_in.dtype != torch.uint8 or not mask_in.is_contiguous():
        raise PnxError("conv3x3_dgrad_s2: g (B,cout,Ho,Wo) with Ho = (H - 1) // 2 + 1 and a contiguous uint8 (B,H,W) mask of the input sites")
    dx = torch.empty((B, cin, H, W), dtype=torch.bfloat16 if len(gs) == 1 else torch.float32, device=gs[0].device, memory_format=torch.channels_last)
    name = "pnx_conv3x3_dgrad_s2_" + _PIECES_TAG[len(gs)]
    check(getattr(lib(), name)(*map(ptr, gs), *map(ptr, ws), ptr(mask_in), ptr(dx), B, H, W, cin, co, stream_ptr()), name)
    return dx


def _smallk_check(x, what):
    if not (x.is_cuda and x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16) and x.is_contiguous(memory_format=torch.channels_last)):
        raise PnxError(f"{what} must be a channels_last fp32 / bf16 CUDA tensor")


def conv3x3_smallk(x, weight, bias=None):
    """nn.Conv2d(64, k, 3, padding=1) with k <= 4 on a channels_last fp32 / bf16 map (pnx_conv3x3_smallk): (B,k,H,W) channels_last of x's dtype;
    weight (k,64,3,3) and bias (k) fp32."""
    _smallk_check(x, "conv3x3_smallk: x")
    k = weight.shape[0]
    if not (weight.is_cuda and weight.dtype == torch.float32 and tuple(weight.shape[1:]) == (64, 3, 3) and weight.is_contiguous() and 1 <= k <= 4
            and x.shape[1] == 64 and (bias is None or (bias.is_cuda and bias.dtype == torch.float32 and bias.numel() == k and bias.is_contiguous()))):
        raise PnxError("conv3x3_smallk: weight must be a contiguous fp32 (k,64,3,3) with k <= 4, bias fp32 (k)")
    B, _, H, W = x.shape
    y = torch.empty((B, k, H, W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    if k == 1:   # (B,1,H,W): channels_last and contiguous coincide, torch may report either stride set
        y = torch.empty((B, H, W, 1), dtype=x.dtype, device=x.device).permute(0, 3, 1, 2)
    check(lib().pnx_conv3x3_smallk(ptr(x), ptr(weight), ptr(bias), ptr(y), B, H, W, 64, k, 0 if x.dtype == torch.float32 else 1, stream_ptr()), "pnx_conv3x3_smallk")
    return y


def conv3x3_smallk_wgrad(x, dy, want_bias=True):
    """(dw (k,64,3,3), dbias (k) or None), fp32, of conv3x3_smallk from x and the upstream gradient dy (B,k,H,W) (pnx_conv3x3_smallk_wgrad)."""
    _smallk_check(x, "conv3x3_smallk_wgrad: x")
    B, c, H, W = x.shape
    k = dy.shape[1]
    if not (c == 64 and 1 <= k <= 4 and dy.is_cuda and dy.dtype == x.dtype and tuple(dy.shape) == (B, k, H, W)):
        raise PnxError("conv3x3_smallk_wgrad: x (B,64,H,W), dy (B,k,H,W) of the same dtype, k <= 4")
    dyc = dy.permute(0, 2, 3, 1).contiguous()    # NHWC with k channels (a no-op for a channels_last gradient)
    nbytes = int(lib().pnx_conv3x3_smallk_wgrad_workspace_bytes(k))
    ws = _PARTIALS_WS.get(nbytes, x.device)
    dw = torch.empty((k, 64, 3, 3), dtype=torch.float32, device=x.device)
    db = torch.empty((k,), dtype=torch.float32, device=x.device) if want_bias else None
    check(lib().pnx_conv3x3_smallk_wgrad(ptr(x), ptr(dyc), ptr(dw), ptr(db), B, H, W, 64, k, 0 if x.dtype == torch.float32 else 1, ptr(ws), ws.numel(), stream_ptr()),
          "pnx_conv3x3_smallk_wgrad")
    return dw, db


def conv3x3_workspace(batch, cout, ho, wo, device, dtype=torch.bfloat16):
    """A persistent (output buffer, row_dirty flags) pair for conv3x3_masked(out=...): both start zeroed (pnx.h: row_dirty).  The flags are the
    (B, ho, segs) uint8 view at offset 0 of the row_dirty array; the written masks the kernels keep behind them are row_dirty_written(flags)."""
    y = torch.zeros((batch, cout, ho, wo), dtype=dtype, device=device).contiguous(memory_format=torch.channels_last)
    segs = (wo + 31) // 32
    arr = torch.zeros((row_dirty_bytes(batch, ho, wo),), dtype=torch.uint8, device=device)
    return y, arr[: batch * ho * segs].view(batch, ho, segs)


def row_dirty_bytes(batch, ho, wo):
    """Bytes of the row_dirty array of a (batch, *, ho, wo) output buffer: flag bytes, then one uint32 written mask per row segment (pnx.h)."""
    return int(lib().pnx_conv3x3_row_dirty_bytes(batch, ho, wo))


def _row_dirty_check(flags, batch, ho, wo):
    """The flags must be the head of an array of row_dirty_bytes: the kernels read and write the written masks behind them."""
    need = row_dirty_bytes(batch, ho, wo)
    if (flags.dtype != torch.uint8 or tuple(flags.shape) != (batch, ho, (wo + 31) // 32) or not flags.is_contiguous()
            or flags.untyped_storage().nbytes() - flags.storage_offset() < need):
        raise PnxError(f"conv3x3: row_dirty must be the flags of conv3x3_workspace ({need} bytes: flags + written masks)")


def row_dirty_written(flags, wo):
    """The written masks behind the flags of a conv3x3_workspace pair: int32 (B, ho, segs), bit p = pixel p of the segment may hold data."""
    B, ho, segs = flags.shape
    _row_dirty_check(flags, B, ho, wo)
    off = (B * ho * segs + 255) // 256 * 256     # pnx.h: the flag bytes, padded to a multiple of 256
    whole = torch.empty(0, dtype=torch.uint8, device=flags.device).set_(flags.untyped_storage(), flags.storage_offset(), (row_dirty_bytes(B, ho, wo),))
    return whole[off: off + 4 * B * ho * segs].view(torch.int32).view(B, ho, segs)


def conv_tile_rows(cin, cout, stride=1):
    """Rows of a tile of the kernel that serves (cin, cout, stride); 0 = that kernel walks all tiles (takes no tile list)."""
    return int(lib().pnx_conv3x3_tile_rows(cin, cout, stride))


def conv_tile_buffers(mask, tile_rows, out=None):
    """The (list int32[>= n_tiles], count int32[1]) pair conv_tile_list(mask, ..., tile_rows) fills: `out` if it is one, a new one without."""
    B, H, W = _like(mask).shape
    n_tiles = B * ((H + tile_rows - 1) // tile_rows) * ((W + 31) // 32)
    if out is None:
        return torch.empty((n_tiles,), dtype=torch.int32, device=mask.device), torch.zeros((1,), dtype=torch.int32, device=mask.device)
    if out[0].numel() < n_tiles or out[0].dtype != torch.int32 or out[1].dtype != torch.int32:
        raise PnxError("conv_tile_list: needs an int32 list of >= n_tiles entries + an int32 count")
    return out


def conv_tile_list(mask, dirties, tile_rows, out=None):
    """(list int32[n_tiles], count int32[1]) of the tile_rows x 32 tiles of `mask` (B,H,W uint8) that hold an active site or a stale row
    of one of the `dirties` (row_dirty arrays of conv3x3_workspace buffers); pass it as tiles= to every stride-1 conv over this mask."""
    B, H, W = mask.shape
    out = conv_tile_buffers(mask, tile_rows, out)
    arr = (ctypes.c_void_p * max(len(dirties), 1))(*[d.data_ptr() for d in dirties])
    check(lib().pnx_conv_tile_list(ptr(mask), arr, len(dirties), B, H, W, tile_rows, ptr(out[0]), ptr(out[1]), stream_ptr()), "pnx_conv_tile_list")
    return out


def _conv3x3_dims(x, wfrag, cout, stride, mask, residual, out, cuda=False):
    """-> (B, H, W, Cin, PNX_BF16 / PNX_F16, Ho, Wo); out: None, or the (y, row_dirty) pair the call writes -- (y, None) for a plain output buffer."""
    xs = _half_nhwc(x, "conv3x3", cuda=cuda)
    if wfrag.dtype != xs.dtype or (residual is not None and _like(residual).dtype != xs.dtype):
        raise PnxError("conv3x3: weights / residual of another dtype than the input")
    B, ci, H, W = xs.shape
    Ho, Wo = _out_hw(H, W, stride)
    if out is not None:
        y, dirty = out
        if (tuple(_half_nhwc(y, "conv3x3 output", xs.dtype).shape) != (B, cout, Ho, Wo)
                or (dirty is not None and (mask is None or tuple(dirty.shape) != (B, Ho, (Wo + 31) // 32)))):
            raise PnxError("conv3x3: output / workspace of the wrong shape (a workspace needs a mask)")
    return B, H, W, ci, _DT[xs.dtype], Ho, Wo


def conv3x3_masked(x, wfrag, bias, cout, stride=1, mask=None, residual=None, relu=True, out=None, tiles=None):
    """x (B,Cin,H,W) channels_last bf16 / fp16 -> (B,Cout,Ho,Wo) channels_last, same dtype (wfrag packed in it); mask uint8 (B,Ho,Wo) of the OUTPUT sites.
    out = (y, row_dirty) from conv3x3_workspace: write into the persistent buffer, touching only row segments that are or were active.
    tiles = conv_tile_list(mask, ...) of the same mask (stride 1 only): walk the listed tiles instead of all of them."""
    B, H, W, ci, _, Ho, Wo = _conv3x3_dims(x, wfrag, cout, stride, mask, residual, out, cuda=True)
    y, dirty = out if out is not None else (torch.empty((B, cout, Ho, Wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last), None)
    if dirty is not None:   # the launch reads and writes the written masks behind the flags: an array of the flags alone is no longer valid
        _row_dirty_check(dirty, B, Ho, Wo)
    tl, tc = tiles if tiles is not None else (None, None)
    check(_conv_fn("conv3x3", x.dtype)(ptr(x), ptr(wfrag), ptr(bias), ptr(residual), ptr(mask), ptr(y), B, H, W, ci, cout, stride, 1 if relu else 0,
                                       ptr(dirty), ptr(tl), ptr(tc), stream_ptr()), "pnx_conv3x3")
    return y


# --------------------------------------------------------------------------------------------- train-mode masked BatchNorm (csrc/masked_bn.hip)
# One call per launch of include/pnx.h's masked_bn family, in the order the autograd node (train_nodes._MaskedBNActFn) issues them:
#   forward   stats -> reduce -> [all-reduce of the sums] -> finalize -> apply
#   backward  bwd_stats -> reduce -> [all-reduce of a copy] -> bwd_finalize -> bwd_apply
# Maps: (B,C,H,W) channels_last bf16 / fp32 with C in MASKED_BN_CHANNELS; mask: flat fp32 [B*H*W] (0 = inactive) or None = every site active.
MASKED_BN_CHANNELS = (8, 16, 32, 64, 128, 256)


def _bn_maps(what, x, mask, *like_x):
    """Validator -> (n_sites, C, PNX_BF16 / PNX_F32): x as above, the mask flat fp32 or None, every other map None or of x's dtype, shape and layout."""
    if not (x.is_cuda and x.dim() == 4 and x.dtype in (torch.bfloat16, torch.float32) and x.shape[1] in MASKED_BN_CHANNELS
            and x.is_contiguous(memory_format=torch.channels_last)):
        raise PnxError(f"{what}: x must be a channels_last bf16 / fp32 CUDA map (B,C,H,W) with C in {MASKED_BN_CHANNELS}")
    n = x.shape[0] * x.shape[2] * x.shape[3]
    if mask is not None and not (mask.is_cuda and mask.dtype == torch.float32 and mask.dim() == 1 and mask.numel() == n and mask.is_contiguous()):
        raise PnxError(f"{what}: the mask must be a flat fp32 CUDA vector of B*H*W = {n} values, or None")
    for t in like_x:
        if t is not None and not (t.is_cuda and t.dtype == x.dtype and t.shape == x.shape and t.is_contiguous(memory_format=torch.channels_last)):
            raise PnxError(f"{what}: the residual and the gradient must have x's dtype, shape and channels_last layout")
    return n, x.shape[1], _DT[x.dtype]


def _bn_vecs(what, n, *vecs, dtype=torch.float32):
    """Validator: every vector that is given is a contiguous CUDA vector of n values (fp32 unless said otherwise)."""
    for v in vecs:
        if v is not None and not (v.is_cuda and v.dtype == dtype and v.dim() == 1 and v.numel() == n and v.is_contiguous()):
            raise PnxError(f"{what}: needs contiguous {str(dtype).split('.')[-1]} CUDA vectors of {n} values")


def masked_bn_blocks():
    """Rows of the partial sums masked_bn_stats / masked_bn_bwd_stats write (their grid size)."""
    return int(lib().pnx_masked_bn_blocks())


def masked_bn_stats(x, mask, center):
    """partials fp32 (blocks, 2C + 1): per workgroup [sum d | sum d^2 | active sites] with d = x - center (fp32 (C), or None = 0)."""
    n, C, dt = _bn_maps("masked_bn_stats", x, mask)
    _bn_vecs("masked_bn_stats", C, center)
    part = torch.empty((masked_bn_blocks(), 2 * C + 1), dtype=torch.float32, device=x.device)
    check(lib().pnx_masked_bn_stats(ptr(x), dt, ptr(mask), n, C, ptr(center), ptr(part), stream_ptr()), "pnx_masked_bn_stats")
    return part


def _masked_channels(c):
    return c in MASKED_BN_CHANNELS


def _bn_reduce(what, part, channels_ok, channels):
    """Shared body of masked_bn_reduce / sp3_bn_reduce; no rows (an empty set of rows): zeros."""
    if not (part.is_cuda and part.dtype == torch.float32 and part.dim() == 2 and part.is_contiguous() and channels_ok(part.shape[1] // 2)):
        raise PnxError(f"{what}: the partials must be a contiguous fp32 CUDA matrix of 2C or 2C + 1 columns with {channels}")
    rows, cols = part.shape
    if rows == 0:
        return torch.zeros((cols,), dtype=torch.float64, device=part.device)
    s = torch.empty((cols,), dtype=torch.float64, device=part.device)
    check(lib().pnx_masked_bn_reduce(ptr(part), rows, cols, ptr(s), stream_ptr()), "pnx_masked_bn_reduce")
    return s


def _bn_finalize(what, channels_ok, channels, sums, center, weight, bias, eps, momentum, running_mean, running_var, num_batches_tracked):
    """Shared body of masked_bn_finalize / sp3_bn_finalize."""
    C = (sums.numel() - 1) // 2
    _bn_vecs(what, 2 * C + 1, sums, dtype=torch.float64)
    _bn_vecs(what, C, center, weight, bias, running_mean, running_var)
    nbt = num_batches_tracked
    if not channels_ok(C) or (nbt is not None and not (nbt.is_cuda and nbt.dtype == torch.int64 and nbt.numel() == 1)):
        raise PnxError(f"{what}: 2C + 1 sums with {channels}, num_batches_tracked an int64 CUDA scalar")
    vec = torch.empty((4 * C + 1,), dtype=torch.float32, device=sums.device)
    mean, invstd, scale, shift, cnt = vec[:C], vec[C:2 * C], vec[2 * C:3 * C], vec[3 * C:4 * C], vec[4 * C:]
    check(lib().pnx_masked_bn_finalize(ptr(sums), C, ptr(center), ptr(weight), ptr(bias), float(eps), float(momentum), ptr(running_mean), ptr(running_var),
                                       ptr(nbt), ptr(mean), ptr(invstd), ptr(scale), ptr(shift), ptr(cnt), stream_ptr()), "pnx_masked_bn_finalize")
    return mean, invstd, scale, shift, cnt


def _bn_bwd_finalize(what, channels_ok, channels, sums_local, sums_global, count):
    """Shared body of masked_bn_bwd_finalize / sp3_bn_bwd_finalize."""
    C = sums_local.numel() // 2
    _bn_vecs(what, 2 * C, sums_local, sums_global, dtype=torch.float64)
    _bn_vecs(what, 1, count)
    if not channels_ok(C):
        raise PnxError(f"{what}: 2C sums with {channels}")
    vec = torch.empty((4 * C,), dtype=torch.float32, device=sums_local.device)
    dgamma, dbeta, mg, mgx = vec[:C], vec[C:2 * C], vec[2 * C:3 * C], vec[3 * C:]
    check(lib().pnx_masked_bn_bwd_finalize(ptr(sums_local), ptr(sums_global), C, ptr(count), ptr(dgamma), ptr(dbeta), ptr(mg), ptr(mgx), stream_ptr()),
          "pnx_masked_bn_bwd_finalize")
    return dgamma, dbeta, mg, mgx


def masked_bn_reduce(part):
    """fp64 (cols): the rows of a partials array added in a fixed order -- what is all-reduced under SyncBatchNorm."""
    return _bn_reduce("masked_bn_reduce", part, _masked_channels, f"C in {MASKED_BN_CHANNELS}")


def masked_bn_finalize(sums, center, weight, bias, eps, momentum, running_mean, running_var, num_batches_tracked):
    """(mean, invstd, scale, shift (C each), count (1)) fp32 from sums = [sum d | sum d^2 | count] around `center` (None = 0), and torch's update of the
    running statistics in place (num_batches_tracked += 1 when given)."""
    return _bn_finalize("masked_bn_finalize", _masked_channels, f"C in {MASKED_BN_CHANNELS}", sums, center, weight, bias, eps, momentum, running_mean,
                        running_var, num_batches_tracked)


def masked_bn_apply(x, residual, mask, scale, shift, relu):
    """y = [relu](x * scale + shift [+ residual]) at the active sites, zeros elsewhere; y like x."""
    n, C, dt = _bn_maps("masked_bn_apply", x, mask, residual)
    _bn_vecs("masked_bn_apply", C, scale, shift)
    y = torch.empty_like(x)
    check(lib().pnx_masked_bn_apply(ptr(x), ptr(residual), dt, ptr(mask), n, C, ptr(scale), ptr(shift), 1 if relu else 0, ptr(y), stream_ptr()),
          "pnx_masked_bn_apply")
    return y


def masked_bn_bwd_stats(gy, x, residual, mask, scale, shift, mean, invstd, relu):
    """partials fp32 (blocks, 2C): [sum g | sum g * xhat] with g = gy * [pre-activation > 0], xhat = (x - mean) * invstd."""
    n, C, dt = _bn_maps("masked_bn_bwd_stats", x, mask, residual, gy)
    _bn_vecs("masked_bn_bwd_stats", C, scale, shift, mean, invstd)
    part = torch.empty((masked_bn_blocks(), 2 * C), dtype=torch.float32, device=x.device)
    check(lib().pnx_masked_bn_bwd_stats(ptr(gy), ptr(x), ptr(residual), dt, ptr(mask), n, C, ptr(scale), ptr(shift), ptr(mean), ptr(invstd), 1 if relu else 0,
                                        ptr(part), stream_ptr()), "pnx_masked_bn_bwd_stats")
    return part


def masked_bn_bwd_finalize(sums_local, sums_global, count):
    """(dgamma, dbeta, mean_g, mean_gx) fp32 (C each): the parameter gradients from the LOCAL sums [sum g | sum g xhat] (fp64 (2C)), the means over
    `count` active sites from the global ones (None: the local ones)."""
    return _bn_bwd_finalize("masked_bn_bwd_finalize", _masked_channels, f"C in {MASKED_BN_CHANNELS}", sums_local, sums_global, count)


def masked_bn_bwd_apply(gy, x, residual, mask, scale, shift, mean, invstd, relu, mean_g, mean_gx, want_residual_grad=False):
    """(dx like x, the residual's gradient like it or None) of masked_bn_apply from the upstream gradient gy and the means of masked_bn_bwd_finalize."""
    n, C, dt = _bn_maps("masked_bn_bwd_apply", x, mask, residual, gy)
    _bn_vecs("masked_bn_bwd_apply", C, scale, shift, mean, invstd, mean_g, mean_gx)
    dx = torch.empty_like(x)
    gres = torch.empty_like(residual) if residual is not None and want_residual_grad else None
    check(lib().pnx_masked_bn_bwd_apply(ptr(gy), ptr(x), ptr(residual), dt, ptr(mask), n, C, ptr(scale), ptr(shift), ptr(mean), ptr(invstd), 1 if relu else 0,
                                        ptr(mean_g), ptr(mean_gx), ptr(dx), ptr(gres), stream_ptr()), "pnx_masked_bn_bwd_apply")
    return dx, gres


# --------------------------------------------------------------------------------------------- sparse 3-D convolution (csrc/sparse3d.hip)
def _i3(v):
    return (ctypes.c_int32 * 3)(*[int(a) for a in v])


class Sp3Index:
    """An active set's index on the device (pnx_sp3_index_bytes): key-order occupancy bitmap + popcount word prefix over (batch, D, H, W)."""

    def __init__(self, batch, grid, device):
        self.batch, self.grid = int(batch), tuple(int(g) for g in grid)
        self.nbytes = lib().pnx_sp3_index_bytes(self.batch, _i3(self.grid))
        if self.nbytes == 0:
            raise PnxError(f"sparse3d: bad grid {self.batch} x {self.grid}")
        self.buf = torch.empty((self.nbytes,), dtype=torch.uint8, device=device)


def _need_coords(coords):
    _need_cuda(coords, "coords")
    if coords.dtype != torch.int32 or coords.dim() != 2 or coords.shape[1] != 4:
        raise PnxError("coords must be (N, 4) int32 [b, z, y, x]")


def sp3_out_grid(batch, grid, kernel, stride, pad):
    """(n + 2 pad - k) // s + 1 per axis of (D, H, W)."""
    out = _i3((0, 0, 0))
    check(lib().pnx_sp3_out_grid(int(batch), _i3(grid), _i3(kernel), _i3(stride), _i3(pad), out), "pnx_sp3_out_grid")
    return tuple(out)


def sp3_index_build(coords, batch, grid, want_rows=False):
    """pnx_sp3_index_build -> (Sp3Index, row_of_rank (N,) int32 or None, count (1,) int32 device tensor)."""
    _need_coords(coords)
    ix = Sp3Index(batch, grid, coords.device)
    n = coords.shape[0]
    rows = torch.full((max(n, 1),), -1, dtype=torch.int32, device=coords.device) if want_rows else None
    count = torch.zeros((1,), dtype=torch.int32, device=coords.device)
    check(lib().pnx_sp3_index_build(ptr(coords), n, ix.batch, _i3(ix.grid), ptr(ix.buf), ix.nbytes, ptr(rows), ptr(count), stream_ptr()),
          "pnx_sp3_index_build")
    return ix, (rows[:n] if want_rows else None), count


def sp3_out_index(coords_in, batch, grid_in, kernel, stride, pad):
    """pnx_sp3_out_index: SparseConv3d's output set -> (Sp3Index over the output grid, count (1,) int32 device tensor)."""
    _need_coords(coords_in)
    ix = Sp3Index(batch, sp3_out_grid(batch, grid_in, kernel, stride, pad), coords_in.device)
    count = torch.zeros((1,), dtype=torch.int32, device=coords_in.device)
    check(lib().pnx_sp3_out_index(ptr(coords_in), coords_in.shape[0], ix.batch, _i3(grid_in), _i3(kernel), _i3(stride), _i3(pad), ptr(ix.buf), ix.nbytes,
                                  ptr(count), stream_ptr()), "pnx_sp3_out_index")
    return ix, count


def sp3_index_coords(ix, n):
    """pnx_sp3_index_coords: the set's first n rows [b, z, y, x] in rank order."""
    coords = torch.empty((max(int(n), 1), 4), dtype=torch.int32, device=ix.buf.device)
    check(lib().pnx_sp3_index_coords(ptr(ix.buf), ix.nbytes, ix.batch, _i3(ix.grid), ptr(coords), int(n), stream_ptr()), "pnx_sp3_index_coords")
    return coords[: int(n)]


def sp3_neighbor_map(coords_out, ix_in, row_of_rank, kernel, stride, pad):
    """pnx_sp3_neighbor_map -> (N_out, kd*kh*kw) int32, -1 for an inactive neighbour."""
    _need_coords(coords_out)
    T = int(kernel[0]) * int(kernel[1]) * int(kernel[2])
    m = torch.empty((coords_out.shape[0], T), dtype=torch.int32, device=coords_out.device)
    check(lib().pnx_sp3_neighbor_map(ptr(coords_out), coords_out.shape[0], ptr(ix_in.buf), ix_in.nbytes, ix_in.batch, _i3(ix_in.grid), ptr(row_of_rank),
                                     _i3(kernel), _i3(stride), _i3(pad), ptr(m), stream_ptr()), "pnx_sp3_neighbor_map")
    return m


def sp3_pack_weight(w):
    """(Cout, kd, kh, kw, Cin) fp32 (BN scale folded in) -> (T, round_up(Cin, 4), round_up(Cout, 16)) zero-padded, the layout of pnx_sp3_conv."""
    co, ci = w.shape[0], w.shape[-1]
    T = w.shape[1] * w.shape[2] * w.shape[3]
    n = lib().pnx_sp3_packed_weight_floats(T, ci, co)
    ci4, co16 = (ci + 3) // 4 * 4, (co + 15) // 16 * 16
    if n != T * ci4 * co16:
        raise PnxError(f"sp3_pack_weight: no packing for {tuple(w.shape)}")
    wp = torch.zeros((T, ci4, co16), dtype=torch.float32, device=w.device)
    wp[:, :ci, :co] = w.float().reshape(co, T, ci).permute(1, 2, 0)
    return wp


def sp3_conv(x, nbmap, w_packed, shift, cout, residual=None, relu=True, per_tap=False):
    """pnx_sp3_conv: x (N_in, Cin) fp32, nbmap (N_out, T) int32 -> (N_out, cout) fp32.  per_tap: pnx_sp3_conv_train, the training graph's summation
    order (every tap summed on its own, the taps added in order)."""
    for t, name in ((x, "x"), (nbmap, "nbmap"), (w_packed, "w_packed"), (shift, "shift")):
        _need_cuda(t, name)
    if x.dtype != torch.float32 or w_packed.dtype != torch.float32 or shift.dtype != torch.float32 or nbmap.dtype != torch.int32:
        raise PnxError("sp3_conv: fp32 features, weights and shift, int32 map")
    n_out, T = nbmap.shape
    ci = x.shape[1]
    if tuple(w_packed.shape) != (T, (ci + 3) // 4 * 4, (cout + 15) // 16 * 16) or shift.numel() < cout:
        raise PnxError(f"sp3_conv: packed weight {tuple(w_packed.shape)} does not fit {T} taps x {ci} -> {cout}")
    if residual is not None:
        _need_cuda(residual, "residual")
        if residual.dtype != torch.float32 or tuple(residual.shape) != (n_out, cout):
            raise PnxError("sp3_conv: residual must be (N_out, cout) fp32")
    y = torch.empty((n_out, cout), dtype=torch.float32, device=x.device)
    fn = lib().pnx_sp3_conv_train if per_tap else lib().pnx_sp3_conv
    check(fn(ptr(x), x.shape[0], ci, ptr(nbmap), n_out, T, ptr(w_packed), ptr(shift), ptr(residual), 1 if relu else 0, ptr(y), cout, stream_ptr()),
          "pnx_sp3_conv_train" if per_tap else "pnx_sp3_conv")
    return y


def sp3_dense(feat, coords, batch, grid):
    """pnx_sp3_dense: rows -> (batch, C*D, H, W) fp32, channel c*D + d, zero elsewhere."""
    _need_coords(coords)
    _need_cuda(feat, "feat")
    if feat.dtype != torch.float32 or feat.dim() != 2 or feat.shape[0] != coords.shape[0]:
        raise PnxError("sp3_dense: feat must be (N, C) fp32 with one row per coordinate")
    D, H, W = (int(g) for g in grid)
    C = feat.shape[1]
    out = torch.empty((int(batch), C * D, H, W), dtype=torch.float32, device=feat.device)
    check(lib().pnx_sp3_dense(ptr(feat), ptr(coords), coords.shape[0], C, int(batch), _i3(grid), ptr(out), stream_ptr()), "pnx_sp3_dense")
    return out


def sp3_pack_weight_t(w, mirror=False):
    """(Cout, kd, kh, kw, Cin) fp32 -> (T, round_up(Cout, 4), round_up(Cin, 16)): the weights of the data gradient, pnx_sp3_conv's layout with
    the channel roles swapped.  mirror=True reverses the taps, for a submanifold layer run on its own map (tmap[i][t] = map[i][T - 1 - t])."""
    co, ci = w.shape[0], w.shape[-1]
    T = w.shape[1] * w.shape[2] * w.shape[3]
    co4, ci16 = (co + 3) // 4 * 4, (ci + 15) // 16 * 16
    if lib().pnx_sp3_packed_weight_floats(T, co, ci) != T * co4 * ci16:
        raise PnxError(f"sp3_pack_weight_t: no packing for {tuple(w.shape)}")
    wt = w.float().reshape(co, T, ci).permute(1, 0, 2)
    wp = torch.zeros((T, co4, ci16), dtype=torch.float32, device=w.device)
    wp[:, :co, :ci] = wt.flip(0) if mirror else wt
    return wp


def sp3_transpose_map(nbmap, n_in):
    """pnx_sp3_transpose_map: nbmap (N_out, T) int32 -> tmap (n_in, T) int32 with tmap[nbmap[o][t]][t] = o, -1 elsewhere."""
    _need_cuda(nbmap, "nbmap")
    if nbmap.dtype != torch.int32 or nbmap.dim() != 2 or not nbmap.is_contiguous():
        raise PnxError("sp3_transpose_map: nbmap must be a contiguous (N_out, T) int32 tensor")
    n_out, T = nbmap.shape
    tmap = torch.empty((int(n_in), T), dtype=torch.int32, device=nbmap.device)
    check(lib().pnx_sp3_transpose_map(ptr(nbmap), n_out, T, int(n_in), ptr(tmap), stream_ptr()), "pnx_sp3_transpose_map")
    return tmap


def sp3_wgrad_workspace_bytes(n_out, taps, cin, cout):
    n = lib().pnx_sp3_wgrad_workspace_bytes(int(n_out), int(taps), int(cin), int(cout))
    if n == 0:
        raise PnxError(f"sp3_wgrad: no kernel for {cin} -> {cout} channels over {taps} taps and {n_out} rows")
    return n


SP3_WGRAD_MAX_CHANNELS = 144  # the widest operand of one pnx_sp3_wgrad call


def sp3_wgrad_blocks(channels):
    """The column blocks [(start, size)] in which sp3_wgrad serves `channels`: one block up to 144; above, k = ceil(channels / 144) blocks of
    round_up(ceil(channels / k), 16) columns, the last one taking what is left (192 -> 96 + 96, 176 -> 96 + 80, 150 -> 80 + 70)."""
    c = int(channels)
    if c < 1:
        raise PnxError(f"sp3_wgrad: {channels} channels")
    if c <= SP3_WGRAD_MAX_CHANNELS:
        return [(0, c)]
    k = -(-c // SP3_WGRAD_MAX_CHANNELS)
    size = (-(-c // k) + 15) // 16 * 16
    return [(s, min(size, c - s)) for s in range(0, c, size)]


def sp3_wgrad(x, nbmap, dy):
    """pnx_sp3_wgrad: x (N_in, Cin), nbmap (N_out, T), dy (N_out, Cout) -> dw (Cout, T, Cin) fp32.  Cin or Cout above 144 (the entry point's range):
    one call per pair of column blocks (sp3_wgrad_blocks) on contiguous column copies, written to dw[co block, :, ci block] -- every element of dw
    is still one call's fixed-order sum over the rows."""
    for t, name in ((x, "x"), (nbmap, "nbmap"), (dy, "dy")):
        _need_cuda(t, name)
    if x.dtype != torch.float32 or dy.dtype != torch.float32 or nbmap.dtype != torch.int32 or x.dim() != 2 or dy.dim() != 2 or nbmap.dim() != 2:
        raise PnxError("sp3_wgrad: fp32 (N, C) features and gradients, int32 map")
    if dy.shape[0] != nbmap.shape[0] or not (x.is_contiguous() and dy.is_contiguous() and nbmap.is_contiguous()):
        raise PnxError("sp3_wgrad: dy and nbmap must have one row per output site, and every operand must be contiguous")
    n_out, T = nbmap.shape
    ci, co = x.shape[1], dy.shape[1]

    def one(xb, dyb):
        cib, cob = xb.shape[1], dyb.shape[1]
        nbytes = sp3_wgrad_workspace_bytes(n_out, T, cib, cob)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
        dwb = torch.empty((cob, T, cib), dtype=torch.float32, device=x.device)
        check(lib().pnx_sp3_wgrad(ptr(xb), xb.shape[0], cib, ptr(dyb), cob, ptr(nbmap), n_out, T, ptr(dwb), ptr(ws), nbytes, stream_ptr()), "pnx_sp3_wgrad")
        return dwb

    ci_blocks, co_blocks = sp3_wgrad_blocks(ci), sp3_wgrad_blocks(co)
    if len(ci_blocks) == 1 and len(co_blocks) == 1:
        return one(x, dy)
    dw = torch.empty((co, T, ci), dtype=torch.float32, device=x.device)
    xs = [x if len(ci_blocks) == 1 else x[:, s:s + k].contiguous() for s, k in ci_blocks]
    for so, ko in co_blocks:
        dyb = dy if len(co_blocks) == 1 else dy[:, so:so + ko].contiguous()
        for (si, ki), xb in zip(ci_blocks, xs):
            dw[so:so + ko, :, si:si + ki] = one(xb, dyb)
    return dw


def sp3_dense_backward(dout, coords, channels):
    """pnx_sp3_dense_backward: dout (batch, C*D, H, W) fp32 -> (N, C) rows, the gradient of sp3_dense."""
    _need_coords(coords)
    dout = dout.contiguous()  # a broadcast gradient (the backward of a sum) arrives with zero strides
    _need_cuda(dout, "dout")
    C = int(channels)
    if dout.dtype != torch.float32 or dout.dim() != 4 or dout.shape[1] % C:
        raise PnxError("sp3_dense_backward: dout must be (batch, C*D, H, W) fp32")
    B, D, H, W = dout.shape[0], dout.shape[1] // C, dout.shape[2], dout.shape[3]
    dfeat = torch.empty((coords.shape[0], C), dtype=torch.float32, device=dout.device)
    check(lib().pnx_sp3_dense_backward(ptr(dout), ptr(coords), coords.shape[0], C, B, _i3((D, H, W)), ptr(dfeat), stream_ptr()), "pnx_sp3_dense_backward")
    return dfeat


# 16-bit inference form (csrc/sparse3d_half.h): rows in bf16 / fp16 with the channel count padded to a multiple of 8, pad columns zero
def _cpad(c):
    return (int(c) + 7) // 8 * 8


def _sp3_half(dtype, what):
    if dtype not in _HALF:
        raise PnxError(f"{what}: torch.bfloat16 or torch.float16, got {dtype}")
    return _DT[dtype]


def sp3_rows_h(x, dtype):
    """(N, C) fp32 rows -> (N, round_up(C, 8)) rows of `dtype`: rounded once to nearest even, pad columns zero."""
    _sp3_half(dtype, "sp3_rows_h")
    if x.dim() != 2 or x.dtype != torch.float32:
        raise PnxError("sp3_rows_h: x must be (N, C) fp32")
    out = torch.zeros((x.shape[0], _cpad(x.shape[1])), dtype=dtype, device=x.device)
    out[:, : x.shape[1]] = x.to(dtype)
    return out


def sp3_pack_weight_h(w, dtype):
    """(Cout, kd, kh, kw, Cin) fp32 (BN scale folded in) -> (S, ceil(Cout / 16), 64, 8) of `dtype`, the fragment order of pnx_sp3_conv_h: K runs
    over (tap, channel padded to cpad = round_up(Cin, 8)) in S = ceil(T * cpad / 32) steps of 32, and element e of lane l of tile j of step s is
    w[16 j + (l & 15)][tap][c] with 32 s + 8 (l >> 4) + e = tap * cpad + c, zero past the last tap / channel.  Rounded once (nearest even) from
    fp32.  Runs on CPU tensors too."""
    _sp3_half(dtype, "sp3_pack_weight_h")
    co, ci = w.shape[0], w.shape[-1]
    T = w.shape[1] * w.shape[2] * w.shape[3]
    cp, nt = _cpad(ci), (co + 15) // 16
    S = (T * cp // 8 + 3) // 4
    if lib().pnx_sp3_packed_weight_halfs(T, ci, co) != S * nt * 512:
        raise PnxError(f"sp3_pack_weight_h: no packing for {tuple(w.shape)}")
    wk = torch.zeros((S * 32, nt * 16), dtype=torch.float32, device=w.device)
    wk[: T * cp].view(T, cp, nt * 16)[:, :ci, :co] = w.float().reshape(co, T, ci).permute(1, 2, 0)
    # (s, kk, e, j, r) -> (s, j, lane = kk * 16 + r, e)
    return wk.view(S, 4, 8, nt, 16).permute(0, 3, 1, 4, 2).reshape(S, nt, 64, 8).to(dtype).contiguous()


def sp3_conv_h(x, nbmap, w_packed, shift, cin, cout, residual=None, relu=True):
    """pnx_sp3_conv_h: x (N_in, round_up(cin, 8)) bf16 / fp16 padded rows (sp3_rows_h, or a previous layer's output), nbmap (N_out, T) int32,
    w_packed from sp3_pack_weight_h in x's dtype, shift (cout,) fp32 -> (N_out, round_up(cout, 8)) in x's dtype, pad columns zero."""
    for t, name in ((x, "x"), (nbmap, "nbmap"), (w_packed, "w_packed"), (shift, "shift")):
        _need_cuda(t, name)
    dt = _sp3_half(x.dtype, "sp3_conv_h")
    if w_packed.dtype != x.dtype or shift.dtype != torch.float32 or nbmap.dtype != torch.int32 or x.dim() != 2 or nbmap.dim() != 2:
        raise PnxError("sp3_conv_h: features and weights of one 16-bit dtype, fp32 shift, int32 map")
    n_out, T = nbmap.shape
    ci, co = int(cin), int(cout)
    if x.shape[1] != _cpad(ci):
        raise PnxError(f"sp3_conv_h: rows of {x.shape[1]} columns for {ci} channels (padded rows have {_cpad(ci)})")
    n = lib().pnx_sp3_packed_weight_halfs(T, ci, co)
    if n == 0 or w_packed.numel() != n or shift.numel() < co:
        raise PnxError(f"sp3_conv_h: packed weight {tuple(w_packed.shape)} does not fit {T} taps x {ci} -> {co}")
    if residual is not None:
        _need_cuda(residual, "residual")
        if residual.dtype != x.dtype or tuple(residual.shape) != (n_out, _cpad(co)):
            raise PnxError("sp3_conv_h: residual must be (N_out, round_up(cout, 8)) of the input's dtype")
    y = torch.empty((n_out, _cpad(co)), dtype=x.dtype, device=x.device)
    check(lib().pnx_sp3_conv_h(ptr(x), x.shape[0], ci, x.shape[1], ptr(nbmap), n_out, T, ptr(w_packed), ptr(shift), ptr(residual), 1 if relu else 0,
                               ptr(y), co, y.shape[1], dt, stream_ptr()), "pnx_sp3_conv_h")
    return y


def sp3_dense_h(feat, coords, batch, grid, channels):
    """pnx_sp3_dense_h: padded bf16 / fp16 rows (N, round_up(channels, 8)) -> (batch, channels*D, H, W) fp32, channel c*D + d, zero elsewhere."""
    _need_coords(coords)
    _need_cuda(feat, "feat")
    dt = _sp3_half(feat.dtype, "sp3_dense_h")
    C = int(channels)
    if feat.dim() != 2 or feat.shape[0] != coords.shape[0] or feat.shape[1] != _cpad(C):
        raise PnxError("sp3_dense_h: feat must be (N, round_up(channels, 8)) with one row per coordinate")
    D, H, W = (int(g) for g in grid)
    out = torch.empty((int(batch), C * D, H, W), dtype=torch.float32, device=feat.device)
    check(lib().pnx_sp3_dense_h(ptr(feat), dt, ptr(coords), coords.shape[0], C, feat.shape[1], int(batch), _i3(grid), ptr(out), stream_ptr()),
          "pnx_sp3_dense_h")
    return out


# 16-bit training form (csrc/sparse3d_half_train.h): the same padded 16-bit operands, fp32 results
def sp3_conv_h_f32(x, nbmap, w_packed, cin, cout):
    """pnx_sp3_conv_h_f32: x (N_in, round_up(cin, 8)) bf16 / fp16 padded rows, nbmap (N_out, T) int32, w_packed from sp3_pack_weight_h in x's dtype
    -> (N_out, cout) fp32, the accumulators of the 16-bit gather-GEMM as they are (no shift, residual, ReLU or rounding)."""
    for t, name in ((x, "x"), (nbmap, "nbmap"), (w_packed, "w_packed")):
        _need_cuda(t, name)
    dt = _sp3_half(x.dtype, "sp3_conv_h_f32")
    if w_packed.dtype != x.dtype or nbmap.dtype != torch.int32 or x.dim() != 2 or nbmap.dim() != 2:
        raise PnxError("sp3_conv_h_f32: features and weights of one 16-bit dtype, int32 map")
    if not (x.is_contiguous() and nbmap.is_contiguous() and w_packed.is_contiguous()):
        raise PnxError("sp3_conv_h_f32: every operand must be contiguous")
    n_out, T = nbmap.shape
    ci, co = int(cin), int(cout)
    if x.shape[1] != _cpad(ci):
        raise PnxError(f"sp3_conv_h_f32: rows of {x.shape[1]} columns for {ci} channels (padded rows have {_cpad(ci)})")
    n = lib().pnx_sp3_packed_weight_halfs(T, ci, co)
    if n == 0 or w_packed.numel() != n:
        raise PnxError(f"sp3_conv_h_f32: packed weight {tuple(w_packed.shape)} does not fit {T} taps x {ci} -> {co}")
    y = torch.empty((n_out, co), dtype=torch.float32, device=x.device)
    check(lib().pnx_sp3_conv_h_f32(ptr(x), x.shape[0], ci, x.shape[1], ptr(nbmap), n_out, T, ptr(w_packed), ptr(y), co, dt, stream_ptr()),
          "pnx_sp3_conv_h_f32")
    return y


def sp3_wgrad_h_partials_bytes(n_out, taps, cin, cout):
    n = lib().pnx_sp3_wgrad_h_partials_bytes(int(n_out), int(taps), int(cin), int(cout))
    if n == 0:
        raise PnxError(f"sp3_wgrad_h: no kernel for {cin} -> {cout} channels over {taps} taps and {n_out} rows")
    return n


def sp3_wgrad_h(x, nbmap, dy, cin, cout):
    """pnx_sp3_wgrad_h: x (N_in, round_up(cin, 8)) and dy (N_out, round_up(cout, 8)) padded rows of one 16-bit dtype, nbmap (N_out, T) int32
    -> dw (cout, T, cin) fp32."""
    for t, name in ((x, "x"), (nbmap, "nbmap"), (dy, "dy")):
        _need_cuda(t, name)
    dt = _sp3_half(x.dtype, "sp3_wgrad_h")
    if dy.dtype != x.dtype or nbmap.dtype != torch.int32 or x.dim() != 2 or dy.dim() != 2 or nbmap.dim() != 2:
        raise PnxError("sp3_wgrad_h: (N, C) features and gradients of one 16-bit dtype, int32 map")
    if dy.shape[0] != nbmap.shape[0] or not (x.is_contiguous() and dy.is_contiguous() and nbmap.is_contiguous()):
        raise PnxError("sp3_wgrad_h: dy and nbmap must have one row per output site, and every operand must be contiguous")
    n_out, T = nbmap.shape
    ci, co = int(cin), int(cout)
    if x.shape[1] != _cpad(ci) or dy.shape[1] != _cpad(co):
        raise PnxError(f"sp3_wgrad_h: rows of {x.shape[1]} / {dy.shape[1]} columns for {ci} -> {co} channels (padded rows have {_cpad(ci)} / {_cpad(co)})")
    nbytes = sp3_wgrad_h_partials_bytes(n_out, T, ci, co)
    part = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)  # call-lifetime scratch
    dw = torch.empty((co, T, ci), dtype=torch.float32, device=x.device)
    check(lib().pnx_sp3_wgrad_h(ptr(x), x.shape[0], ci, x.shape[1], ptr(dy), co, dy.shape[1], ptr(nbmap), n_out, T, ptr(dw), dt, ptr(part), nbytes,
                                stream_ptr()), "pnx_sp3_wgrad_h")
    return dw


# Train-mode BatchNorm1d + residual + ReLU over the rows (csrc/sparse3d_bn.h).  y, out, gout, dy: (n, C) fp32 rows, C in 1..SP3_BN_MAX_CHANNELS;
# residual: None, fp32 (n, C), or padded 16-bit rows (n, round_up(C, 8)).  The per-channel passes are masked_bn's kernels, which take any C <= 256.
SP3_BN_MAX_CHANNELS = 256


def _sp3_bn_rows(what, y, *like_y):
    """Validator -> (n, C): y and every other fp32 operand that is given are contiguous CUDA (n, C) fp32 rows."""
    if not (y.is_cuda and y.dim() == 2 and y.dtype == torch.float32 and y.is_contiguous() and 1 <= y.shape[1] <= SP3_BN_MAX_CHANNELS):
        raise PnxError(f"{what}: y must be contiguous CUDA (n, C) fp32 rows with C in 1..{SP3_BN_MAX_CHANNELS}")
    for t in like_y:
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.shape == y.shape and t.is_contiguous()):
            raise PnxError(f"{what}: the gradient and an fp32 residual must be contiguous CUDA fp32 rows of y's shape")
    return y.shape[0], y.shape[1]


def _sp3_bn_residual(what, y, residual):
    """Validator -> the residual's PNX dtype: None, fp32 rows like y, or padded 16-bit rows (n, round_up(C, 8))."""
    if residual is None or residual.dtype == torch.float32:
        _sp3_bn_rows(what, y, residual)
        return PNX_F32
    if not (residual.is_cuda and residual.dtype in _HALF and tuple(residual.shape) == (y.shape[0], _cpad(y.shape[1])) and residual.is_contiguous()):
        raise PnxError(f"{what}: a 16-bit residual must be contiguous CUDA bf16 / fp16 rows (n, round_up(C, 8))")
    return _DT[residual.dtype]


def sp3_bn_split(n, channels):
    """(blocks, rows_per_pass, passes) of the four passes over n rows of `channels`: the rows of the partials, the rows a workgroup covers per pass
    and the passes of the busiest workgroup (include/pnx.h: pnx_sp3_bn_split; the longest fp32 chain of a partial is passes + rows_per_pass terms)."""
    s = (ctypes.c_int32 * 3)()
    check(lib().pnx_sp3_bn_split(int(n), int(channels), s), "pnx_sp3_bn_split")
    return int(s[0]), int(s[1]), int(s[2])


def sp3_bn_partials_bytes(n, channels, backward=False):
    nbytes = lib().pnx_sp3_bn_partials_bytes(int(n), int(channels), 1 if backward else 0)
    if nbytes == 0:
        raise PnxError(f"sp3_bn: no kernel for {n} rows of {channels} channels")
    return nbytes


def _sp3_bn_partials(n, C, backward, device):
    """(buffer, its bytes, the (blocks, cols) fp32 view the kernel fills): call-lifetime scratch of exactly the size the library asks for."""
    nbytes = sp3_bn_partials_bytes(n, C, backward)
    buf = torch.empty((nbytes,), dtype=torch.uint8, device=device)
    cols = 2 * C + (0 if backward else 1)
    blocks = sp3_bn_split(n, C)[0]
    return buf, nbytes, buf[: blocks * cols * 4].view(torch.float32).view(blocks, cols)


def sp3_bn_stats(y, center):
    """partials fp32 (blocks, 2C + 1): per workgroup [sum d | sum d^2 | rows] with d = y - center (fp32 (C), or None = 0)."""
    n, C = _sp3_bn_rows("sp3_bn_stats", y)
    _bn_vecs("sp3_bn_stats", C, center)
    buf, nbytes, part = _sp3_bn_partials(n, C, False, y.device)
    check(lib().pnx_sp3_bn_stats(ptr(y), n, C, ptr(center), ptr(buf), nbytes, stream_ptr()), "pnx_sp3_bn_stats")
    return part


def _sp3_bn_channels(c):
    return 1 <= c <= SP3_BN_MAX_CHANNELS


def sp3_bn_reduce(part):
    """fp64 (cols): the rows of a partials array added in a fixed order (pnx_masked_bn_reduce) -- what is all-reduced under SyncBatchNorm.
    No rows (an empty set): zeros."""
    return _bn_reduce("sp3_bn_reduce", part, _sp3_bn_channels, f"C in 1..{SP3_BN_MAX_CHANNELS}")


def sp3_bn_finalize(sums, center, weight, bias, eps, momentum, running_mean, running_var, num_batches_tracked):
    """masked_bn_finalize at any C in 1..SP3_BN_MAX_CHANNELS (pnx_masked_bn_finalize never depended on the channel count)."""
    return _bn_finalize("sp3_bn_finalize", _sp3_bn_channels, f"C in 1..{SP3_BN_MAX_CHANNELS}", sums, center, weight, bias, eps, momentum, running_mean,
                        running_var, num_batches_tracked)


def sp3_bn_apply(y, residual, scale, shift, relu, out_dtype=None):
    """(out (n, C) fp32, out_h): out = [relu](y * scale + shift [+ residual]); out_dtype bf16 / fp16: out_h (n, round_up(C, 8)) = out rounded once to
    nearest even, pad columns zero -- bit for bit sp3_rows_h(out, out_dtype) -- written in the same pass; None: out_h is None."""
    n, C = _sp3_bn_rows("sp3_bn_apply", y)
    rdt = _sp3_bn_residual("sp3_bn_apply", y, residual)
    _bn_vecs("sp3_bn_apply", C, scale, shift)
    odt = PNX_F32 if out_dtype is None else _sp3_half(out_dtype, "sp3_bn_apply")
    if rdt != PNX_F32 and odt != PNX_F32 and rdt != odt:
        raise PnxError("sp3_bn_apply: a 16-bit residual and out_h must have one dtype")
    out = torch.empty_like(y)
    out_h = None if out_dtype is None else torch.empty((n, _cpad(C)), dtype=out_dtype, device=y.device)
    check(lib().pnx_sp3_bn_apply(ptr(y), n, C, ptr(scale), ptr(shift), ptr(residual), rdt, 1 if relu else 0, ptr(out), ptr(out_h), odt, stream_ptr()),
          "pnx_sp3_bn_apply")
    return out, out_h


def sp3_bn_bwd_stats(gout, y, residual, scale, shift, mean, invstd, relu):
    """partials fp32 (blocks, 2C): [sum g | sum g * xhat] with g = gout * [pre-activation > 0] (relu) or gout, xhat = (y - mean) * invstd."""
    n, C = _sp3_bn_rows("sp3_bn_bwd_stats", y, gout)
    rdt = _sp3_bn_residual("sp3_bn_bwd_stats", y, residual)
    _bn_vecs("sp3_bn_bwd_stats", C, scale, shift, mean, invstd)
    buf, nbytes, part = _sp3_bn_partials(n, C, True, y.device)
    check(lib().pnx_sp3_bn_bwd_stats(ptr(gout), ptr(y), ptr(residual), rdt, n, C, ptr(scale), ptr(shift), ptr(mean), ptr(invstd), 1 if relu else 0,
                                     ptr(buf), nbytes, stream_ptr()), "pnx_sp3_bn_bwd_stats")
    return part


def sp3_bn_bwd_finalize(sums_local, sums_global, count):
    """masked_bn_bwd_finalize at any C in 1..SP3_BN_MAX_CHANNELS (`count`: the rows behind the global sums)."""
    return _bn_bwd_finalize("sp3_bn_bwd_finalize", _sp3_bn_channels, f"C in 1..{SP3_BN_MAX_CHANNELS}", sums_local, sums_global, count)


def sp3_bn_bwd_apply(gout, y, residual, scale, shift, mean, invstd, relu, mean_g, mean_gx, want_residual_grad=False):
    """(dy (n, C) fp32, the residual's gradient g (n, C) fp32 or None) of sp3_bn_apply from the upstream gradient and the means of sp3_bn_bwd_finalize."""
    n, C = _sp3_bn_rows("sp3_bn_bwd_apply", y, gout)
    rdt = _sp3_bn_residual("sp3_bn_bwd_apply", y, residual)
    _bn_vecs("sp3_bn_bwd_apply", C, scale, shift, mean, invstd, mean_g, mean_gx)
    dy = torch.empty_like(y)
    gres = torch.empty_like(y) if want_residual_grad else None
    check(lib().pnx_sp3_bn_bwd_apply(ptr(gout), ptr(y), ptr(residual), rdt, n, C, ptr(scale), ptr(shift), ptr(mean), ptr(invstd), 1 if relu else 0,
                                     ptr(mean_g), ptr(mean_gx), ptr(dy), ptr(gres), stream_ptr()), "pnx_sp3_bn_bwd_apply")
    return dy, gres


# --------------------------------------------------------------------------------------------- label assignment
_ASSIGN_OUT = (("hm", torch.float32), ("anno_box", torch.float32), ("ind", torch.int64), ("mask", torch.uint8), ("cat", torch.int64),
               ("gt_boxes", torch.float32))


def assign_workspace_bytes(batch, n_tasks, max_objs):
    return int(lib().pnx_assign_workspace_bytes(batch, n_tasks, max_objs))


def assign_labels(gt_boxes, gt_classes, num_gt, desc, out, counts, ws):
    """pnx_assign_labels: gt_boxes (B, K, 9) fp32, gt_classes (B, K) int32 indices into desc's class table, num_gt (B) int32 or None;
    desc a _lib.PnxAssignDesc; out: {hm, anno_box, ind, mask, cat, gt_boxes} -> one tensor per task, every element written by the call;
    counts (B, n_tasks) int32; ws: uint8 buffer of assign_workspace_bytes(B, n_tasks, max_objs).  Returns out."""
    _need_cuda(gt_boxes, "gt_boxes")
    _need_cuda(gt_classes, "gt_classes")
    if gt_boxes.dtype != torch.float32 or gt_boxes.dim() != 3 or gt_boxes.shape[2] != 9:
        raise PnxError(f"gt_boxes must be (B, K, 9) fp32, got {tuple(gt_boxes.shape)} {gt_boxes.dtype}")
    B, K = int(gt_boxes.shape[0]), int(gt_boxes.shape[1])
    if gt_classes.dtype != torch.int32 or tuple(gt_classes.shape) != (B, K):
        raise PnxError(f"gt_classes must be ({B}, {K}) int32, got {tuple(gt_classes.shape)} {gt_classes.dtype}")
    if num_gt is not None:
        _need_cuda(num_gt, "num_gt")
        if num_gt.dtype != torch.int32 or tuple(num_gt.shape) != (B,):
            raise PnxError(f"num_gt must be ({B},) int32, got {tuple(num_gt.shape)} {num_gt.dtype}")
    T, M = int(desc.n_tasks), int(desc.max_objs)
    want = {"hm": lambda t: (B, desc.ncls[t], desc.h[t], desc.w[t]), "anno_box": lambda t: (B, M, 10), "ind": lambda t: (B, M),
            "mask": lambda t: (B, M), "cat": lambda t: (B, M), "gt_boxes": lambda t: (B, M, 7)}
    arrs = []
    for key, dt in _ASSIGN_OUT:
        if len(out[key]) != T:
            raise PnxError(f"assign_labels: {len(out[key])} `{key}` outputs for {T} tasks")
        for t, o in enumerate(out[key]):
            _need_cuda(o, f"{key}[{t}]")
            if o.dtype != dt or tuple(o.shape) != tuple(want[key](t)):
                raise PnxError(f"assign_labels: {key}[{t}] must be {tuple(want[key](t))} {dt}, got {tuple(o.shape)} {o.dtype}")
        arrs.append((ctypes.c_void_p * T)(*[o.data_ptr() for o in out[key]]))
    _need_cuda(counts, "counts")
    if counts.dtype != torch.int32 or tuple(counts.shape) != (B, T):
        raise PnxError(f"counts must be ({B}, {T}) int32, got {tuple(counts.shape)} {counts.dtype}")
    _need_cuda(ws, "workspace")
    check(lib().pnx_assign_labels(ptr(gt_boxes), ptr(gt_classes), ptr(num_gt), B, K, ctypes.byref(desc), *arrs, ptr(counts), ptr(ws),
                                  ws.numel() * ws.element_size(), stream_ptr()), "pnx_assign_labels")
    return out


# --------------------------------------------------------------------------------------------- GT paste and global augmentation
def paste_chunk_rows():
    """Scene rows per workgroup of the point pass (tests aim at the seams with it)."""
    return int(lib().pnx_paste_chunk_rows())


def _typed(t, name, dtype, shape):
    _need_cuda(t, name)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise PnxError(f"{name} must be {tuple(shape)} {dtype}, got {tuple(t.shape)} {t.dtype}")


def paste_select(gt_boxes, gt_classes, num_gt, cand, bank_offsets, n_groups, out):
    """pnx_paste_select.  gt_boxes (B, K, D) fp32 with D 7 or 9, gt_classes (B, K) int32, num_gt (B) int32 or None.  cand: None (no candidates)
    or a dict {bank (B, S) int32, boxes (B, S, D) fp32, cls (B, S) int32, group (B, S) int32}; bank_offsets (n_obj + 1) int64.
    out: {accept (B, S) uint8, paste_offset (B, S) int32 (both may be None without candidates), boxes (B, K + S, D) fp32, classes (B, K + S)
    int32, num (B) int32, pasted_rows (B) int32}.  Returns out."""
    _need_cuda(gt_boxes, "gt_boxes")
    if gt_boxes.dtype != torch.float32 or gt_boxes.dim() != 3 or gt_boxes.shape[2] not in (7, 9):
        raise PnxError(f"gt_boxes must be (B, K, 7 or 9) fp32, got {tuple(gt_boxes.shape)} {gt_boxes.dtype}")
    B, K, D = (int(v) for v in gt_boxes.shape)
    _typed(gt_classes, "gt_classes", torch.int32, (B, K))
    if num_gt is not None:
        _typed(num_gt, "num_gt", torch.int32, (B,))
    S, n_obj = 0, 0
    if cand is not None:
        S = int(cand["bank"].shape[1])
        _typed(cand["bank"], "cand.bank", torch.int32, (B, S))
        _typed(cand["boxes"], "cand.boxes", torch.float32, (B, S, D))
        _typed(cand["cls"], "cand.cls", torch.int32, (B, S))
        _typed(cand["group"], "cand.group", torch.int32, (B, S))
        _need_cuda(bank_offsets, "bank_offsets")
        if bank_offsets.dtype != torch.int64 or bank_offsets.dim() != 1 or bank_offsets.numel() < 2:
            raise PnxError("bank_offsets must be (n_obj + 1) int64 with n_obj >= 1")
        n_obj = int(bank_offsets.numel()) - 1
        _typed(out["accept"], "out.accept", torch.uint8, (B, S))
        _typed(out["paste_offset"], "out.paste_offset", torch.int32, (B, S))
    _typed(out["boxes"], "out.boxes", torch.float32, (B, K + S, D))
    _typed(out["classes"], "out.classes", torch.int32, (B, K + S))
    _typed(out["num"], "out.num", torch.int32, (B,))
    _typed(out["pasted_rows"], "out.pasted_rows", torch.int32, (B,))
    c = cand or {}
    check(lib().pnx_paste_select(ptr(gt_boxes), ptr(gt_classes), ptr(num_gt), B, K, D, ptr(c.get("bank")), ptr(c.get("boxes")), ptr(c.get("cls")),
                                 ptr(c.get("group")), S, int(n_groups), ptr(bank_offsets) if cand is not None else None, n_obj, ptr(out.get("accept")) if S else None,
                                 ptr(out.get("paste_offset")) if S else None, ptr(out["boxes"]), ptr(out["classes"]), ptr(out["num"]), ptr(out["pasted_rows"]),
                                 stream_ptr()), "pnx_paste_select")
    return out


def paste_augment_workspace_bytes(n_points, batch):
    return int(lib().pnx_paste_augment_workspace_bytes(int(n_points), int(batch)))


def paste_augment_points(points, batch, cand, paste_offset, pasted_rows, bank_points, bank_offsets, xform, out, n_out, frame_rows, ws):
    """pnx_paste_augment_points.  points (N, 1 + F) fp32 [batch index, x, y, z, ..]; cand / paste_offset / pasted_rows as paste_select takes and
    leaves them (cand None: augment only); bank_points (P, F) fp32, bank_offsets (n_obj + 1) int64; xform (B, 6) fp64 or None; out
    (capacity, 1 + F) fp32, n_out (1) int32, frame_rows (B) int32; ws: uint8 buffer of paste_augment_workspace_bytes(N, B).  Returns out."""
    _need_cuda(points, "points")
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] < 4:
        raise PnxError(f"points must be (N, 1 + F) fp32 with F >= 3, got {tuple(points.shape)} {points.dtype}")
    N, F, B = int(points.shape[0]), int(points.shape[1]) - 1, int(batch)
    S, D, n_obj, P = 0, 0, 0, 0
    if cand is not None:
        S, D = int(cand["boxes"].shape[1]), int(cand["boxes"].shape[2])
        _typed(cand["bank"], "cand.bank", torch.int32, (B, S))
        _typed(cand["boxes"], "cand.boxes", torch.float32, (B, S, D))
        _typed(paste_offset, "paste_offset", torch.int32, (B, S))
        _typed(pasted_rows, "pasted_rows", torch.int32, (B,))
        _need_cuda(bank_points, "bank_points")
        _need_cuda(bank_offsets, "bank_offsets")
        if bank_points.dtype != torch.float32 or bank_points.dim() != 2 or int(bank_points.shape[1]) != F:
            raise PnxError(f"bank_points must be (P, {F}) fp32 (the scene rows have {F} columns after the batch index), got {tuple(bank_points.shape)} {bank_points.dtype}")
        if bank_offsets.dtype != torch.int64 or bank_offsets.dim() != 1 or bank_offsets.numel() < 2:
            raise PnxError("bank_offsets must be (n_obj + 1) int64 with n_obj >= 1")
        n_obj, P = int(bank_offsets.numel()) - 1, int(bank_points.shape[0])
    if xform is not None:
        _typed(xform, "xform", torch.float64, (B, 6))
    _need_cuda(out, "out")
    if out.dtype != torch.float32 or out.dim() != 2 or int(out.shape[1]) != F + 1:
        raise PnxError(f"out must be (capacity, {F + 1}) fp32, got {tuple(out.shape)} {out.dtype}")
    _typed(n_out, "n_out", torch.int32, (1,))
    _typed(frame_rows, "frame_rows", torch.int32, (B,))
    _need_cuda(ws, "workspace")
    c = cand or {}
    check(lib().pnx_paste_augment_points(ptr(points), N, F, B, ptr(c.get("bank")), ptr(c.get("boxes")), ptr(paste_offset) if S else None,
                                         ptr(pasted_rows) if S else None, S, D, ptr(bank_points) if S else None, ptr(bank_offsets) if S else None, n_obj, P,
                                         ptr(xform), ptr(out), int(out.shape[0]), ptr(n_out), ptr(frame_rows), ptr(ws), ws.numel() * ws.element_size(),
                                         stream_ptr()), "pnx_paste_augment_points")
    return out


def augment_boxes_(boxes, num, xform):
    """pnx_augment_boxes, in place: boxes (B, M, 7 or 9) fp32, num (B) int32 or None (= M), xform (B, 6) fp64."""
    _need_cuda(boxes, "boxes")
    if boxes.dtype != torch.float32 or boxes.dim() != 3 or boxes.shape[2] not in (7, 9):
        raise PnxError(f"boxes must be (B, M, 7 or 9) fp32, got {tuple(boxes.shape)} {boxes.dtype}")
    B, M, D = (int(v) for v in boxes.shape)
    if num is not None:
        _typed(num, "num", torch.int32, (B,))
    _typed(xform, "xform", torch.float64, (B, 6))
    check(lib().pnx_augment_boxes(ptr(boxes), ptr(num), B, M, D, ptr(xform), stream_ptr()), "pnx_augment_boxes")
    return boxes
