"""The fp64 statement of every layer of the inference graph, read off the ORIGINAL detector's modules (det.backbone.blocks[si][j], det.backbone.mapping,
det.neck, det.head), one function per layer kind.  Plain torch: no kernel of the project and no folding helper of pillarnext_amd is used -- the only thing
the functions take from the package are the module objects whose parameters they read.

Every function states its layer the way the module applies it: convolution (its bias, if it has one), eval BatchNorm with the module's own eps,
residual, ReLU, mask, in that order, all in fp64.  It returns a Layer:

  ref    the statement's output;
  terms  sum|terms|: the same expression on |x|, |W a| (a = gamma / sqrt(running_var + eps), the BatchNorm scale inside the weight), |shift|
         (shift = (conv bias - running_mean) a + beta) and |residual| -- what a kernel that multiplies rounded operands is bounded against;
  mask   the output mask of a backbone layer (None for the dense layers); parts: sum_d |part_d| of the neck's four partial maps (None elsewhere).

rounded=dtype gives the ONCE-ROUNDED statement: the same layer with a rounding to `dtype` exactly where the fused graph stores a value in its element
type -- the folded weight W a (rounded once, from fp64), the four partial maps of the neck, the layer's output -- and nowhere else; everything between
stays fp64.  conv_out=True additionally rounds the convolution's result before shift / residual / ReLU, for the layers whose convolution is a library
call that writes its result in the element type before the epilogue pass reads it.

The convolutions are written as a loop over the taps with one matrix product per tap (conv2d / deconv2x2 below), so that the statement neither depends
on which fp64 convolutions a GPU library implements nor is the code the CPU test compares it with (the modules run F.conv2d)."""
from collections import namedtuple

import torch
import torch.nn.functional as F

Layer = namedtuple("Layer", "ref terms mask parts", defaults=(None, None))
ASPP_DILATIONS = (1, 6, 12, 18)


def f64(t):
    return t.detach().double()


def rnd(t, dtype):
    """t rounded once to dtype (None: unchanged), held in fp64 again"""
    return t if dtype is None else t.to(dtype).double()


# ------------------------------------------------------------------------------------------------ convolutions, tap by tap
def conv2d(x, w, stride=1, padding=0, dilation=1):
    """F.conv2d(x, w, None, stride, padding, dilation) for (B,C,H,W) x and (O,C,kh,kw) w, zero padding"""
    O, C, kh, kw = w.shape
    B, _, H, W = x.shape
    Ho = (H + 2 * padding - dilation * (kh - 1) - 1) // stride + 1
    Wo = (W + 2 * padding - dilation * (kw - 1) - 1) // stride + 1
    xp = F.pad(x, (padding, padding, padding, padding)).permute(0, 2, 3, 1)
    out = None
    for ky in range(kh):
        for kx in range(kw):
            y0, x0 = ky * dilation, kx * dilation
            v = xp[:, y0:y0 + (Ho - 1) * stride + 1:stride, x0:x0 + (Wo - 1) * stride + 1:stride]
            t = v @ w[:, :, ky, kx].t()
            out = t if out is None else out + t
    return out.permute(0, 3, 1, 2)


def deconv2x2(x, w):
    """F.conv_transpose2d(x, w, None, 2) for a (Cin,Cout,2,2) weight: every output pixel has exactly one tap"""
    B, C, H, W = x.shape
    out = x.new_zeros((B, 2 * H, 2 * W, w.shape[1]))
    xl = x.permute(0, 2, 3, 1)
    for ky in range(2):
        for kx in range(2):
            out[:, ky::2, kx::2] = xl @ w[:, :, ky, kx]
    return out.permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ conv + eval BatchNorm
def bn_scale_shift(bn, conv_bias=None):
    """(a, shift) of an eval BatchNorm behind a convolution: bn(conv(x) + b0) = conv(x) a + shift"""
    a = f64(bn.weight) / torch.sqrt(f64(bn.running_var) + bn.eps)
    b0 = f64(conv_bias) if conv_bias is not None else torch.zeros_like(a)
    return a, (b0 - f64(bn.running_mean)) * a + f64(bn.bias)


def _cv(x, w, geom, transposed):
    return deconv2x2(x, w) if transposed else conv2d(x, w, *geom)


def conv_bn(conv, bn, x, rounded=None, conv_out=False):
    """-> (bn(conv(x)) before any residual / activation, its sum|terms|).  conv: an nn.Conv2d or the SepHead's ConvTranspose2d(2, 2);  bn None: the bare
    convolution with its bias.  Unrounded, the convolution and the BatchNorm are applied one after the other as the modules do; the rounded variant
    needs the folded weight to round it, so it convolves with rnd(W a) and adds the shift."""
    transposed = isinstance(conv, torch.nn.ConvTranspose2d)
    if transposed:
        assert tuple(conv.kernel_size) == (2, 2) and tuple(conv.stride) == (2, 2) and tuple(conv.padding) == (0, 0)
    assert conv.stride[0] == conv.stride[1] and conv.padding[0] == conv.padding[1] and conv.dilation[0] == conv.dilation[1] and conv.groups == 1
    geom = (conv.stride[0], conv.padding[0], conv.dilation[0])
    w = f64(conv.weight)
    cshape = (1, -1, 1, 1)
    if bn is None:
        a, shift = torch.ones(w.shape[1 if transposed else 0], dtype=torch.float64, device=w.device), f64(conv.bias)
    else:
        a, shift = bn_scale_shift(bn, conv.bias)
    wa = w * a.view((1, -1, 1, 1) if transposed else (-1, 1, 1, 1))
    terms = _cv(x.abs(), wa.abs(), geom, transposed) + shift.abs().view(cshape)
    if rounded is not None:
        y = _cv(x, rnd(wa, rounded), geom, transposed)
        return (rnd(y, rounded) if conv_out else y) + shift.view(cshape), terms
    y = _cv(x, w, geom, transposed)
    if conv.bias is not None:
        y = y + f64(conv.bias).view(cshape)
    if bn is not None:
        y = (y - f64(bn.running_mean).view(cshape)) / torch.sqrt(f64(bn.running_var).view(cshape) + bn.eps) * f64(bn.weight).view(cshape) + f64(bn.bias).view(cshape)
    return y, terms


# ------------------------------------------------------------------------------------------------ backbone
def pooled_mask(mask, stride):
    """the occupancy behind a 3x3 / stride / pad-1 sparse convolution: (B,1,H,W) 0/1 in fp64"""
    return F.max_pool2d(mask, 3, stride, 1)


def sparse_conv_block(m, x, mask, rounded=None):
    """SparseConvBlock: relu(bn(conv(x))) * mask_out; the entry convolution of a stage (use_subm=False) pools its mask, a submanifold one keeps it"""
    mask_out = mask if m.subm else pooled_mask(mask, m.stride)
    y, terms = conv_bn(m.conv, m.norm, x, rounded)
    return Layer(rnd(torch.relu(y) * mask_out, rounded), terms * mask_out, mask_out)


def sparse_block_tail(rb, y, x_in, mask, rounded=None):
    """second half of a SparseBasicBlock: relu(bn2(conv2(y)) + x_in) * mask, y = block1's output, x_in = the block's input"""
    z, terms = conv_bn(rb.conv2, rb.norm2, y, rounded)
    return Layer(rnd(torch.relu(z + x_in) * mask, rounded), (terms + x_in.abs()) * mask, mask)


def sparse_basic_block(rb, x, mask, rounded=None):
    y = sparse_conv_block(rb.block1, x, mask, rounded)
    return sparse_block_tail(rb, y.ref, x, mask, rounded)


def mapping(bb, x, mask, rounded=None, conv_out=False):
    """SparseResNet.mapping: 1x1 convolution + BN + ReLU on the last stage's mask"""
    y, terms = conv_bn(bb.mapping[0], bb.mapping[1], x, rounded, conv_out)
    return Layer(rnd(torch.relu(y) * mask, rounded), terms * mask, mask)


# ------------------------------------------------------------------------------------------------ neck
def conv_block(cb, x, rounded=None, conv_out=False):
    """ConvBlock (dense): relu(bn(conv(x)))"""
    y, terms = conv_bn(cb.conv.conv, cb.norm, x, rounded, conv_out)
    return Layer(rnd(torch.relu(y), rounded), terms)


def pre_conv_tail(pre, y, x_in, rounded=None, conv_out=False):
    """second half of the neck's BasicBlock: act(block2(y) + x_in) -- block2 ends in its own ReLU, the residual comes BEHIND it"""
    z, terms = conv_bn(pre.block2.conv.conv, pre.block2.norm, y, rounded, conv_out)
    return Layer(rnd(torch.relu(torch.relu(z) + x_in), rounded), terms + x_in.abs())


def pre_conv(pre, x, rounded=None, conv_out=False):
    y = conv_block(pre.block1, x, rounded, conv_out)
    return pre_conv_tail(pre, y.ref, x, rounded, conv_out)


def aspp_distributed(nk):
    """The neck behind pre_conv has no BN or activation between its six branches and post_conv's 1x1, so
        post(cat(x, conv1x1(x), conv_d(x, Ws) for d in 1, 6, 12, 18)) = sum_d conv_d(x, w_d) + shift,
        w_d = P_(2+d) Ws, with (P_0 + P_1 W1) added to the centre tap of w_1   (P_k: the k-th column block of the post weight times a).
    -> ([w_d], shift) in fp64.  The bars and the once-rounded statement need this form: the graph rounds w_d and stores conv_d(x, w_d)."""
    a, shift = bn_scale_shift(nk.post_conv.norm, nk.post_conv.conv.conv.bias)
    C = nk.weight.shape[0]
    P = (f64(nk.post_conv.conv.conv.weight).reshape(-1, 6 * C) * a.view(-1, 1)).reshape(-1, 6, C)
    ws = f64(nk.weight)
    wds = [torch.einsum("om,mikl->oikl", P[:, 2 + k], ws) for k in range(4)]
    wds[0][:, :, 1, 1] += P[:, 0] + P[:, 1] @ f64(nk.conv1x1.weight).reshape(C, C)
    return wds, shift


def aspp(nk, x, rounded=None):
    """ASPPNeck._forward behind pre_conv, as the module writes it: post_conv(cat(x, conv1x1(x), conv_d(x, W) for d in 1, 6, 12, 18)).
    terms and parts (sum_d |part_d|) are taken on the distributed form; the rounded variant IS the distributed form: rnd(w_d), every partial map rounded,
    their sum + shift in fp64, ReLU, the output rounded."""
    wds, shift = aspp_distributed(nk)
    parts = [conv2d(x, w, 1, d, d) for w, d in zip(wds, ASPP_DILATIONS)]
    terms = sum(conv2d(x.abs(), w.abs(), 1, d, d) for w, d in zip(wds, ASPP_DILATIONS)) + shift.abs().view(1, -1, 1, 1)
    pabs = sum(p.abs() for p in parts)
    if rounded is not None:
        s = sum(rnd(conv2d(x, rnd(w, rounded), 1, d, d), rounded) for w, d in zip(wds, ASPP_DILATIONS))
        return Layer(rnd(torch.relu(s + shift.view(1, -1, 1, 1)), rounded), terms, None, pabs)
    w = f64(nk.weight)
    outs = [x, conv2d(x, f64(nk.conv1x1.weight))] + [conv2d(x, w, 1, d, d) for d in ASPP_DILATIONS]
    y, _ = conv_bn(nk.post_conv.conv.conv, nk.post_conv.norm, torch.cat(outs, dim=1))
    return Layer(torch.relu(y), terms, None, pabs)


def neck(nk, x, rounded=None):
    return aspp(nk, pre_conv(nk.pre_conv, x, rounded).ref, rounded)


# ------------------------------------------------------------------------------------------------ head
def shared_conv(hd, x, rounded=None):
    """CenterHead.shared_conv: 3x3 convolution with bias + BN + ReLU"""
    y, terms = conv_bn(hd.shared_conv[0], hd.shared_conv[1], x, rounded)
    return Layer(rnd(torch.relu(y), rounded), terms)


def deblock(task, x, rounded=None):
    """SepHead.deblock: ConvTranspose2d 2x2 / stride 2 + BN + ReLU"""
    y, terms = conv_bn(task.deblock.conv.conv, task.deblock.norm, x, rounded)
    return Layer(rnd(torch.relu(y), rounded), terms)


def branch_first(task, name, x, rounded=None):
    """conv-BN-ReLU of one SepHead branch"""
    fc = getattr(task, name)
    assert len(fc) == 4
    y, terms = conv_bn(fc[0], fc[1], x, rounded)
    return Layer(rnd(torch.relu(y), rounded), terms)


def branch_last(task, name, h, rounded=None):
    """the output convolution of one SepHead branch (bias, no BN, no activation)"""
    y, terms = conv_bn(getattr(task, name)[3], None, h, rounded)
    return Layer(rnd(y, rounded), terms)


def head(hd, x, rounded=None):
    """-> per task {branch name: Layer}"""
    sh = shared_conv(hd, x, rounded).ref
    out = []
    for task in hd.tasks:
        up = deblock(task, sh, rounded).ref
        out.append({name: branch_last(task, name, branch_first(task, name, up, rounded).ref, rounded) for name in task.heads})
    return out
