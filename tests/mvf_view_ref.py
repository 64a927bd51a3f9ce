"""Test helper (not a test): a functional statement of ONE view net of the multi-view reader (mvf_encoder.SingleView.blocks + its sampling) on a
dense canvas, in any floating-point type -- fp64 is the yardstick of the GPU tests.  models.MaskedBatchNorm.forward casts to fp32, so the modules
themselves cannot run in fp64; this restates them with torch ops under autograd:

    SparseConv2d (SparseConvBlock, use_subm=False)  mask_out = the k x k / stride max-pooled mask; y = conv2d(x * mask_in, w) * mask_out
    SubMConv2d                                      mask_out = mask_in
    BatchNorm over ACTIVE sites                     training: mean and biased variance over mask == 1, running statistics moved with the unbiased
                                                    variance (momentum of the module); eval: the running statistics
    SparseBasicBlock                                relu(bn2(subm(relu(bn1(subm(x))))) + x), every result masked
    sampling                                        mvf_encoder.bilinear_interpolate (the reference's statement, mvf:208-246) of the last map at the
                                                    points' cell positions

The module supplies structure only (kernel sizes, strides, eps, momentum, training flags); parameters and buffers are passed as tensors of the
working type, so the same function serves fp64 (the twin) and fp32 (held to the modules on the CPU by tests/test_mvf_view_ref_cpu.py)."""
import torch
import torch.nn.functional as F

from pillarnext_amd.models import SparseBasicBlock, SparseConvBlock
from pillarnext_amd.mvf_encoder import bilinear_interpolate


def layers(view):
    """[(prefix of the conv, prefix of its norm, conv module, norm module, role)] in execution order; role: "entry", "block1" or "conv2"."""
    out = []
    for i, seq in enumerate(view.blocks):
        for j, m in enumerate(seq):
            if isinstance(m, SparseConvBlock):
                out.append((f"{i}.{j}.conv", f"{i}.{j}.norm", m.conv, m.norm, "entry" if not m.subm else "subm"))
            elif isinstance(m, SparseBasicBlock):
                out.append((f"{i}.{j}.block1.conv", f"{i}.{j}.block1.norm", m.block1.conv, m.block1.norm, "block1"))
                out.append((f"{i}.{j}.conv2", f"{i}.{j}.norm2", m.conv2, m.norm2, "conv2"))
            else:
                raise TypeError(type(m).__name__)
    return out


def tensors_of(view, dtype, device=None, requires_grad=True):
    """({name: parameter of view.blocks as a fresh leaf in dtype}, {name: buffer clone in dtype (num_batches_tracked stays int64)})."""
    params = {k: v.detach().to(device=device or v.device, dtype=dtype).clone().requires_grad_(requires_grad) for k, v in view.blocks.named_parameters()}
    buffers = {k: v.detach().to(device=device or v.device).clone() if v.dtype == torch.int64 else v.detach().to(device=device or v.device, dtype=dtype).clone()
               for k, v in view.blocks.named_buffers()}
    return params, buffers


def _bn(x, mask, pre, norm, params, buffers, new_buffers):
    g, b = params[pre + ".weight"].view(1, -1, 1, 1), params[pre + ".bias"].view(1, -1, 1, 1)
    if not norm.training:
        mean, var = buffers[pre + ".running_mean"], buffers[pre + ".running_var"]
        return (x - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + norm.eps) * g + b
    cnt = mask.sum()
    if float(cnt) <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {(int(cnt), x.shape[1])}")
    mean = (x * mask).sum(dim=(0, 2, 3)) / cnt
    var = (((x - mean.view(1, -1, 1, 1)) ** 2) * mask).sum(dim=(0, 2, 3)) / cnt
    mom = norm.momentum
    new_buffers[pre + ".running_mean"] = (1 - mom) * buffers[pre + ".running_mean"] + mom * mean.detach()
    new_buffers[pre + ".running_var"] = (1 - mom) * buffers[pre + ".running_var"] + mom * var.detach() * cnt / (cnt - 1)
    new_buffers[pre + ".num_batches_tracked"] = buffers[pre + ".num_batches_tracked"] + 1
    return (x - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + norm.eps) * g + b


def view_blocks(view, x, mask, params, buffers):
    """view.blocks on the dense map x (B, C, H, W) with the active mask (B, 1, H, W) (same dtype) -> (map, mask, [(map, mask)] per stage, new buffers)."""
    new_buffers = dict(buffers)
    stages = []
    resid = None
    plan = layers(view)
    ends, done = set(), 0            # the number of layers after which a stage is complete
    for seq in view.blocks:
        done += sum(1 if isinstance(m, SparseConvBlock) else 2 for m in seq)
        ends.add(done)
    for n, (cpre, npre, conv, norm, role) in enumerate(plan, 1):
        mask_in = mask
        if role == "entry":
            k = conv.kernel_size[0]
            mask = F.max_pool2d(mask, k, conv.stride[0], k // 2)
        if role == "block1":
            resid = x
        y = F.conv2d(x * mask_in, params[cpre + ".weight"], None, conv.stride, conv.padding) * mask
        y = _bn(y, mask, npre, norm, params, buffers, new_buffers)
        if role == "conv2":
            y = y + resid
        x = torch.relu(y) * mask
        if n in ends:
            stages.append((x, mask))
    return x, mask, stages, new_buffers


def active_set(mask):
    """(N, 3) int64 [b, y, x] of mask == 1, in [b, y, x] order."""
    return mask[:, 0].nonzero()


def cell_positions(pos, pos_min, pos_voxel, ds_rate):
    """The sample positions in cells of the last map, computed in fp32 with the kernels' operation order (bil_sample of csrc/group.hip:
    ((pos - min) / voxel) * (1 / ds), ds a power of two) -- an INPUT of the twin, which then works on them in its own type."""
    p = pos.detach().float()
    mn = torch.tensor([float(pos_min[0]), float(pos_min[1])], dtype=torch.float32, device=p.device)
    vs = torch.tensor([float(pos_voxel[0]), float(pos_voxel[1])], dtype=torch.float32, device=p.device)
    return ((p[:, :2] - mn) / vs) * torch.tensor(1.0 / float(ds_rate), dtype=torch.float32, device=p.device)


def view_twin(view, fv, unq, cells_xy, unq_inv, batch_size, H, W, params, buffers):
    """SingleView.forward after cell_features: fv (P, C) at unq (P, 3) [b, y, x] -> scatter, view.blocks, bilinear sampling at cells_xy (N, 2)
    (cell_positions) of image unq[unq_inv][:, 0].  Works in fv's dtype.
    -> dict(out (N, C_last), sets [(N_s, 3) int64 [b, y, x] per stage], maps [stage maps], buffers {name: value after the forward})."""
    dtype, dev = fv.dtype, fv.device
    u = unq.long()
    canvas = torch.zeros((batch_size, H, W, fv.shape[1]), dtype=dtype, device=dev)
    mask = torch.zeros((batch_size, 1, H, W), dtype=dtype, device=dev)
    canvas = canvas.index_put((u[:, 0], u[:, 1], u[:, 2]), fv)
    mask[u[:, 0], 0, u[:, 1], u[:, 2]] = 1
    x, mask, stages, new_buffers = view_blocks(view, canvas.permute(0, 3, 1, 2), mask, params, buffers)
    b = u[unq_inv.long(), 0:1].to(dtype) if len(u) else torch.zeros((cells_xy.shape[0], 1), dtype=dtype, device=dev)
    out = bilinear_interpolate(x, torch.cat([b, cells_xy.to(dtype)], dim=1))
    return dict(out=out, sets=[active_set(m) for _, m in stages], maps=[s for s, _ in stages], buffers=new_buffers)
