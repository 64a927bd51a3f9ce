"""Test helper (not a test): the fp64 statement of SparseConvHalfFunction, the 16-bit training node of the sparse 3-D convolution.

Every operand is rounded ONCE to the 16-bit type (sparse3d_half_ref.round_to), everything else is fp64:
    forward(nbmap, x, w, dtype)          y  = rulebook convolution (sparse_conv3d_ref.gather_conv) on round(x), round(w)
    grad_input(nbmap, w, dy, n_in, dtype)  dx = sparse_conv3d_grad_ref.grad_input on round(w), round(dy)
    grad_weight(nbmap, x, dy, dtype)     dw = sparse_conv3d_grad_ref.grad_weight on round(x), round(dy)
each with the sum of |terms| of every element, and
    RoundedConv                          the same node as a torch fp64 autograd.Function over per-tap (output rows, input rows) pairs
    wgrad_h_split / wgrad_h_partials_bytes / wgrad_h_tree_height   pnx_sp3_wgrad_h's static split as include/pnx.h documents it."""
import numpy as np
import torch

import sparse_conv3d_grad_ref as G
import sparse_conv3d_ref as R
from sparse3d_half_ref import round_to


def _round(v, dtype):
    return v if dtype is None else round_to(v, dtype)


def forward(nbmap, x, w, dtype):
    return R.gather_conv(_round(np.asarray(x, np.float64), dtype), nbmap, _round(np.asarray(w, np.float64), dtype))


def grad_input(nbmap, w, dy, n_in, dtype):
    return G.grad_input(nbmap, _round(np.asarray(w, np.float64), dtype), _round(np.asarray(dy, np.float64), dtype), n_in)


def grad_weight(nbmap, x, dy, dtype):
    return G.grad_weight(nbmap, _round(np.asarray(x, np.float64), dtype), _round(np.asarray(dy, np.float64), dtype))


def pairs_of(nbmap, device=None):
    """Per tap (output rows that have the tap, the input rows they read), as int64 tensors."""
    m = torch.as_tensor(np.asarray(nbmap), dtype=torch.int64, device=device)
    out = []
    for t in range(m.shape[1]):
        sel = (m[:, t] >= 0).nonzero()[:, 0]
        out.append((sel, m[sel, t]))
    return out


def plain_conv(x, w, pairs, n_out):
    """y[o] = sum_t w[:, t, :] . x[src_t] under ordinary autograd (w: (Cout, kd, kh, kw, Cin))."""
    wt = w.reshape(w.shape[0], -1, w.shape[-1])
    out = torch.zeros((n_out, w.shape[0]), dtype=x.dtype, device=x.device)
    for t, (sel, src) in enumerate(pairs):
        out = out.index_add(0, sel, x[src] @ wt[:, t].T)
    return out


class RoundedConv(torch.autograd.Function):
    """The node in fp64: forward on round(x), round(w); backward rounds dy once, dx from round(dy) and round(w), dw from round(x) and round(dy).
    dtype None: no rounding (plain_conv's own gradients)."""

    @staticmethod
    def forward(ctx, x, w, pairs, n_out, dtype):
        xr, wr = _round(x.detach(), dtype), _round(w.detach(), dtype)
        ctx.save_for_backward(xr, wr)
        ctx.pairs, ctx.dtype = pairs, dtype
        return plain_conv(xr, wr, pairs, n_out)

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        dyr = _round(dy, ctx.dtype)
        wt = wr.reshape(wr.shape[0], -1, wr.shape[-1])
        dx = torch.zeros_like(xr)
        dw = torch.zeros_like(wt)
        for t, (sel, src) in enumerate(ctx.pairs):
            dx = dx.index_add(0, src, dyr[sel] @ wt[:, t])
            dw[:, t] = dyr[sel].T @ xr[src]
        return dx, dw.view(wr.shape), None, None, None


def wgrad_h_split(n_out, cout):
    """pnx_sp3_wgrad_h's static split (include/pnx.h): (rows per workgroup R, partials P, output-channel tiles per wave, channel groups)."""
    tiles = (cout + 15) // 16
    mt = tiles if tiles <= 3 else (3 if tiles % 3 == 0 else (2 if tiles % 2 == 0 else 3))
    groups = (tiles + mt - 1) // mt
    p0 = max(1, 256 // groups)
    rows = min(max(((n_out + p0 - 1) // p0 + 31) // 32 * 32, 256), 4096)
    return rows, (n_out + rows - 1) // rows, mt, groups


def wgrad_h_partials_bytes(n_out, taps, cin, cout):
    """P * T * cin * cout floats rounded up to a multiple of 256 bytes, at least 256; 0 for shapes without a kernel."""
    if not (0 <= n_out < 2 ** 31 and 1 <= taps <= 27 and 1 <= cin <= 144 and 1 <= cout <= 144):
        return 0
    parts = wgrad_h_split(n_out, cout)[1]
    return max(256, (parts * taps * cin * cout * 4 + 255) // 256 * 256)


def wgrad_h_tree_height(n_out, cout):
    """Terms of the longest accumulation chain of one dw element (a workgroup's rows, 32 per MFMA, in step order) plus the partials added."""
    rows, parts, _, _ = wgrad_h_split(n_out, cout)
    return min(rows, n_out) + parts
