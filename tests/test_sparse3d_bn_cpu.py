"""CPU: the fp64 statement of the fused BatchNorm1d + residual + ReLU node (tests/sparse3d_bn_ref.py) is what torch computes, and the switch of
SparseResNet3D.use_fused_norm.
  - forward and hand-written backward against fp64 torch autograd of relu(batch_norm(y) + res), allclose at 1e-12; in the 16-bit variant the
    residual goes through round_to with a straight-through gradient
  - the running statistics against nn.BatchNorm1d in fp64
  - the test inputs leave at most 1 % of the elements with a ReLU gate the fp32 kernels may decide either way (the cap of the GPU tests)
  - use_fused_norm returns self, toggles, changes no state-dict key; training on CPU tensors still raises the existing PnxError."""
import pytest

torch = pytest.importorskip("torch")

import sparse3d_bn_ref as BR  # noqa: E402
from sparse3d_half_ref import round_to  # noqa: E402

DTYPES = [None, torch.bfloat16, torch.float16]
SHAPES = [(2, 16), (33, 18), (500, 36), (257, 144)]
EPS = 1e-3


def _close(a, b):
    return torch.allclose(a, b, rtol=1e-12, atol=1e-12)


def _operands(n, C, seed=1):
    return tuple(t.double() for t in BR.inputs(n, C, seed))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("n,C", SHAPES)
def test_statement_is_torch_autograd(n, C, with_res, relu, dtype):
    y, res, gout, gamma, beta, rm, rv = _operands(n, C)
    res = res if with_res else None
    out, cache = BR.forward(y, gamma, beta, res, relu, EPS, dtype)
    dy, dgamma, dbeta, dres = BR.backward(gout, cache)
    # torch: F.batch_norm in training mode, the residual rounded with a straight-through gradient under a 16-bit dtype
    leaves = [t.clone().requires_grad_(True) for t in (y, gamma, beta)] + ([res.clone().requires_grad_(True)] if with_res else [])
    r = None
    if with_res:
        r = leaves[3] if dtype is None else leaves[3] + (round_to(leaves[3].detach(), dtype) - leaves[3].detach())
    z = torch.nn.functional.batch_norm(leaves[0], None, None, leaves[1], leaves[2], True, 0.0, EPS)
    z = z if r is None else z + r
    want = torch.relu(z) if relu else z
    want.backward(gout)
    assert _close(out, want.detach())
    assert _close(dy, leaves[0].grad) and _close(dgamma, leaves[1].grad) and _close(dbeta, leaves[2].grad)
    if with_res:
        assert _close(dres, leaves[3].grad)
        if dtype is not None:  # the rounded rows are what is added
            assert _close(cache["z"], cache["xhat"] * gamma + beta + round_to(res, dtype)) and not torch.equal(round_to(res, dtype), res)
    else:
        assert dres is None
    # the same node as ordinary autograd ops (what the whole-graph statements use)
    leaves2 = [t.clone().requires_grad_(True) for t in (y, gamma, beta)] + ([res.clone().requires_grad_(True)] if with_res else [])
    out2 = BR.bn_act(leaves2[0], leaves2[1], leaves2[2], leaves2[3] if with_res else None, relu, EPS, dtype)
    out2.backward(gout)
    assert _close(out2.detach(), out) and _close(leaves2[0].grad, dy) and _close(leaves2[1].grad, dgamma) and _close(leaves2[2].grad, dbeta)
    if with_res:
        assert _close(leaves2[3].grad, dres)


@pytest.mark.parametrize("n,C", SHAPES)
def test_running_statistics_are_batchnorm1d(n, C):
    y, res, gout, gamma, beta, rm, rv = _operands(n, C)
    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=0.01).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    want = bn(y)
    out, cache = BR.forward(y, gamma, beta, None, False, EPS)
    m, v = BR.running(rm, rv, cache["mean"], cache["var"], n, 0.01)
    assert _close(out, want.detach()) and _close(m, bn.running_mean) and _close(v, bn.running_var) and int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("n,C", [(n, C) for C in (16, 18, 36, 72, 128, 144) for n in (2, 33, 500)] + [(5000, 18), (5000, 144)])
def test_inputs_keep_undecided_gates_under_the_cap(n, C):
    """The GPU tests leave out elements whose pre-activation is within the apply bar of zero (the fp32 kernel may gate them either way) and cap
    their share at 1 %: the fp64 statement alone says the chosen inputs stay far below that, with every kind of residual."""
    y, res, gout, gamma, beta, rm, rv = _operands(n, C)
    assert float((y.mean(0).abs() / y.std(0).clamp(min=1e-6)).max()) > 10 or n < 3, "some channels must sit far from zero"
    for r in (None, res, round_to(res, torch.bfloat16), round_to(res, torch.float16)):
        out, cache = BR.forward(y, gamma, beta, r, True, EPS)
        scale = gamma * cache["invstd"]
        bar = BR.apply_bar(y, scale, beta - cache["mean"] * scale, r)
        assert float((cache["z"].abs() <= bar).double().mean()) <= 0.01


def _backbone():
    from pillarnext_amd.sparse3d import SparseResNet3D

    return SparseResNet3D(layer_nums=[1, 1], ds_layer_strides=[1, 2], ds_num_filters=[16, 32], num_input_features=5)


def test_use_fused_norm_switch():
    from pillarnext_amd._lib import PnxError

    bb = _backbone()
    keys = list(bb.state_dict())
    assert bb.fused_norm is False
    assert bb.use_fused_norm() is bb and bb.fused_norm is True
    assert bb.use_fused_norm(False) is bb and bb.fused_norm is False
    assert bb.use_fused_norm(True).fused_norm is True and list(bb.state_dict()) == keys
    assert bb.use_half_precision(torch.bfloat16, training=True).fused_norm is True and bb.half_train_dtype == torch.bfloat16  # independent switches
    for mode in (torch.bfloat16, None):
        bb.use_half_precision(mode, training=mode is not None)
        with pytest.raises(PnxError, match="training needs CUDA"):
            bb.train()(torch.zeros((4, 5)), torch.zeros((4, 4), dtype=torch.int32), [4, 4, 4], 1)
    other = _backbone()
    assert other.fused_norm is False  # per module


def test_node_is_public_and_documented():
    from pillarnext_amd import ops, sparse3d

    doc = sparse3d.SparseBNActFunction.__doc__
    assert "straight through" in doc and "rounded" in doc.lower()
    for name in ("sp3_bn_split", "sp3_bn_stats", "sp3_bn_reduce", "sp3_bn_finalize", "sp3_bn_apply", "sp3_bn_bwd_stats", "sp3_bn_bwd_finalize",
                 "sp3_bn_bwd_apply"):
        assert callable(getattr(ops, name))
    assert ops.sp3_bn_split(500, 144) == (36, 14, 1) and ops.sp3_bn_split(0, 18)[0] == 0
    blocks, rpp, passes = ops.sp3_bn_split(1 << 30, 18)
    assert (blocks, rpp) == (1024, 85) and passes == -(-(-(-(1 << 30) // 85)) // 1024)
    assert ops.sp3_bn_partials_bytes(500, 144) == -(-36 * (2 * 144 + 1) * 4 // 256) * 256 and ops.sp3_bn_partials_bytes(0, 16) == 256
