"""Test helper (not a test): the fp64 statement of sparse3d.SparseBNActFunction, the fused training node BatchNorm1d + residual + ReLU over the
(n, C) rows of an active set, on torch fp64 tensors (CPU or GPU).

    forward(y, gamma, beta, res, relu, eps, dtype)    out = relu?(z), z = (y - mean) * invstd * gamma + beta (+ r) with the batch's own mean and
                                                      biased variance; r = res, or under a 16-bit dtype round_to(res, dtype): the node reads the
                                                      ROUNDED rows of the block input there, as the 16-bit eval path does
    backward(gout, cache)                             the hand-written backward: g = gout * [z > 0] (or gout), dbeta = sum g, dgamma = sum g xhat,
                                                      dy = gamma invstd (g - mean g - xhat mean(g xhat)), dres = g (straight through the rounding)
    running(rm, rv, mean, var, n, momentum)           torch's training-mode update: momentum, unbiased variance
    round_ste(x, dtype)                               round_to under autograd with a straight-through gradient (the residual operand)
    bn_act(y, gamma, beta, res, relu, eps, dtype)     the same node as ordinary torch autograd ops (what the whole-graph statements use)
and, for the kernels (pnx_sp3_bn_* of csrc/sparse3d_bn.h) on the operands they saw:
    apply_ref / apply_bar, bwd_terms, bwd_apply_ref / bwd_apply_bar, chain(n, C, split)
    inputs(n, C, seed)                                the test inputs: |mean| ~ 30 std in every third channel, so that the centring matters."""
import torch

from sparse3d_half_ref import round_to

EPS32 = 2.0 ** -24


def _r(res, dtype):
    if res is None:
        return None
    return res if dtype is None else round_to(res, dtype)


def forward(y, gamma, beta, res, relu, eps, dtype=None):
    n = y.shape[0]
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = (y - mean) * invstd
    z = xhat * gamma + beta
    r = _r(res, dtype)
    if r is not None:
        z = z + r
    out = torch.relu(z) if relu else z
    return out, dict(y=y, z=z, xhat=xhat, mean=mean, var=var, invstd=invstd, gamma=gamma, relu=relu, n=n, has_res=res is not None)


def backward(gout, cache):
    g = gout * (cache["z"] > 0) if cache["relu"] else gout
    xhat = cache["xhat"]
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    dy = cache["gamma"] * cache["invstd"] * (g - g.mean(0) - xhat * (g * xhat).mean(0))
    return dy, dgamma, dbeta, (g if cache["has_res"] else None)


def running(rm, rv, mean, var, n, momentum):
    return (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * var * n / max(n - 1, 1)


def round_ste(x, dtype):
    return x if dtype is None else x + (round_to(x.detach(), dtype) - x.detach())


def bn_act(y, gamma, beta, res, relu, eps, dtype=None):
    mean, var = y.mean(0), y.var(0, unbiased=False)
    z = (y - mean) / torch.sqrt(var + eps) * gamma + beta
    if res is not None:
        z = z + round_ste(res, dtype)
    return torch.relu(z) if relu else z


# ------------------------------------------------------------------------------------------------ the kernels, on the operands they saw
def chain(split):
    """Longest fp32 chain of a partial, as include/pnx.h documents the split (blocks, rows_per_pass, passes): passes + rows_per_pass terms added,
    each term formed with at most 3 roundings."""
    blocks, rpp, passes = split
    return passes + rpp + 3


def apply_ref(y, scale, shift, r, relu):
    z = y * scale + shift + (0 if r is None else r)
    return (torch.relu(z) if relu else z), z


def apply_bar(y, scale, shift, r):
    return 3 * EPS32 * ((y * scale).abs() + shift.abs() + (0 if r is None else r.abs()))


def bwd_apply_ref(g, y, scale, mean, invstd, mean_g, mean_gx):
    return scale * (g - mean_g - (y - mean) * invstd * mean_gx)


def bwd_apply_bar(g, y, scale, mean, invstd, mean_g, mean_gx):
    return 8 * EPS32 * scale.abs() * (g.abs() + mean_g.abs() + (y.abs() + mean.abs()) * invstd * mean_gx.abs())


def inputs(n, C, seed, device="cpu"):
    """(y, res, gout, gamma, beta, running_mean, running_var) fp32: every third channel has |mean| ~ 30 std, the running mean sits near the batch
    mean (as after a few steps of training), the residual is of the activations' size."""
    g = torch.Generator().manual_seed(seed * 1000 + n * 7 + C)
    std = 0.5 + torch.rand(C, generator=g)
    mean = torch.randn(C, generator=g)
    mean[::3] = 30.0 * std[::3] * torch.where(torch.rand(C, generator=g)[::3] < 0.5, -1.0, 1.0)
    y = (mean + std * torch.randn((n, C), generator=g)).float()
    res = torch.randn((n, C), generator=g).float()
    gout = torch.randn((n, C), generator=g).float()
    gamma = (0.5 + torch.rand(C, generator=g)).float()
    beta = (0.4 * torch.rand(C, generator=g) - 0.2).float()
    rm = (mean + 0.1 * std * torch.randn(C, generator=g)).float()
    rv = (std * std * (0.8 + 0.4 * torch.rand(C, generator=g))).float()
    return tuple(t.to(device) for t in (y, res, gout, gamma, beta, rm, rv))
