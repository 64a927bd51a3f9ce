"""CPU: the host side of SparseResNet3D's 16-bit training path.
  - the fp64 statement the GPU tests hold the node to (tests/sparse3d_half_train_ref.py): its autograd.Function equals plain fp64 autograd at
    1e-12 when the rounding is the identity, and rounds x, w and dy exactly where it says
  - pnx_sp3_wgrad_h's split restated from include/pnx.h against pnx_sp3_wgrad_h_partials_bytes
  - SparseResNet3D.use_half_precision(dtype, training=...)
  - the argument checks of pnx_sp3_conv_h_f32 / pnx_sp3_wgrad_h, which come before any HIP call."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sparse3d_half_train_ref as TR  # noqa: E402
import sparse_conv3d_ref as R  # noqa: E402
from sparse3d_half_ref import round_to  # noqa: E402

DTYPES = [torch.bfloat16, torch.float16]


def _small_layer(stride):
    rng = np.random.default_rng(17 + stride)
    B, grid, n, cin, cout = 2, (5, 6, 7), 120, 5, 6
    keys = rng.choice(B * grid[0] * grid[1] * grid[2], size=n, replace=False)
    c, _ = R.sort_rows(np.stack(np.unravel_index(keys, (B, *grid)), 1))
    oc = c if stride == 1 else R.output_set(c, grid, 3, stride, 1)[0]
    m = R.neighbor_map(oc, c, 3, stride, 1)
    x = torch.from_numpy(rng.standard_normal((n, cin)))
    w = torch.from_numpy(rng.standard_normal((cout, 3, 3, 3, cin)) / 10)
    dy = torch.from_numpy(rng.standard_normal((len(oc), cout)))
    return m, x, w, dy


def _autograd(fn, x, w, dy):
    x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = fn(x, w)
    y.backward(dy)
    return y.detach(), x.grad, w.grad


@pytest.mark.parametrize("stride", [1, 2])
def test_statement_is_plain_autograd_without_rounding(stride):
    m, x, w, dy = _small_layer(stride)
    pairs = TR.pairs_of(m)
    want = _autograd(lambda a, b: TR.plain_conv(a, b, pairs, m.shape[0]), x, w, dy)
    got = _autograd(lambda a, b: TR.RoundedConv.apply(a, b, pairs, m.shape[0], None), x, w, dy)
    for g, r, name in zip(got, want, ("y", "dx", "dw")):
        assert float((g - r).abs().max()) <= 1e-12 * max(1.0, float(r.abs().max())), name
    # and both are the numpy rulebook
    y, _ = TR.forward(m, x.numpy(), w.numpy(), None)
    dx, _ = TR.grad_input(m, w.numpy(), dy.numpy(), len(x), None)
    dw, _ = TR.grad_weight(m, x.numpy(), dy.numpy(), None)
    for g, r, name in zip(got, (y, dx, dw.reshape(w.shape)), ("y", "dx", "dw")):
        assert np.abs(g.numpy() - r).max() <= 1e-12 * max(1.0, np.abs(r).max()), name


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("stride", [1, 2])
def test_statement_rounds_x_w_and_dy_once(stride, dtype):
    m, x, w, dy = _small_layer(stride)
    pairs = TR.pairs_of(m)
    xr, wr, dyr = round_to(x, dtype), round_to(w, dtype), round_to(dy, dtype)
    assert not torch.equal(xr, x) and not torch.equal(wr, w) and not torch.equal(dyr, dy)
    got = _autograd(lambda a, b: TR.RoundedConv.apply(a, b, pairs, m.shape[0], dtype), x, w, dy)
    want = _autograd(lambda a, b: TR.plain_conv(a, b, pairs, m.shape[0]), xr, wr, dyr)  # plain autograd on the rounded operands
    for g, r, name in zip(got, want, ("y", "dx", "dw")):
        assert float((g - r).abs().max()) <= 1e-12 * max(1.0, float(r.abs().max())), name
    unrounded = _autograd(lambda a, b: TR.plain_conv(a, b, pairs, m.shape[0]), x, w, dy)
    for g, r in zip(got, unrounded):
        assert float((g - r).abs().max()) > 1e-6  # the rounding is really there
    y, _ = TR.forward(m, x.numpy(), w.numpy(), dtype)
    dx, _ = TR.grad_input(m, w.numpy(), dy.numpy(), len(x), dtype)
    dw, _ = TR.grad_weight(m, x.numpy(), dy.numpy(), dtype)
    for g, r, name in zip(got, (y, dx, dw.reshape(w.shape)), ("y", "dx", "dw")):
        assert np.abs(g.numpy() - r).max() <= 1e-12 * max(1.0, np.abs(r).max()), name


SPLIT_TABLE = [(n, T, ci, co) for n in (0, 20, 100, 807, 1203, 1500, 70_000, 3_000_000) for T, ci, co in ((27, 5, 18), (27, 18, 18), (1, 36, 72), (3, 144, 144))]


def test_wgrad_h_split_matches_the_size_query():
    from pillarnext_amd import _lib

    L = _lib.lib()
    for n, T, ci, co in SPLIT_TABLE:
        rows, parts, mt, groups = TR.wgrad_h_split(n, co)
        assert rows % 32 == 0 and 256 <= rows <= 4096 and parts == -(-n // rows) and mt * groups >= -(-co // 16)
        assert TR.wgrad_h_tree_height(n, co) == min(rows, n) + parts
        want = max(256, -(-parts * T * ci * co * 4 // 256) * 256)
        assert TR.wgrad_h_partials_bytes(n, T, ci, co) == want
        assert L.pnx_sp3_wgrad_h_partials_bytes(n, T, ci, co) == want, (n, T, ci, co)
    assert TR.wgrad_h_split(1500, 18)[:2] == (256, 6) and TR.wgrad_h_split(3_000_000, 144)[:2] == (4096, 733)
    assert TR.wgrad_h_split(70_000, 18)[:2] == (288, 244)  # ceil(70000 / 256) = 274 rounded up to the K step of 32
    # refused shapes: 0 from the query and from its restatement
    for n, T, ci, co in ((100, 27, 145, 16), (100, 27, 16, 145), (100, 28, 16, 16), (100, 0, 16, 16), (-1, 27, 16, 16), (2 ** 31, 27, 16, 16), (100, 27, 0, 16)):
        assert L.pnx_sp3_wgrad_h_partials_bytes(n, T, ci, co) == 0 == TR.wgrad_h_partials_bytes(n, T, ci, co), (n, T, ci, co)


def _backbone():
    from pillarnext_amd.sparse3d import SparseResNet3D

    return SparseResNet3D(layer_nums=[1, 1], ds_layer_strides=[1, 2], ds_num_filters=[16, 32], num_input_features=5)


def test_use_half_precision_training_switch():
    from pillarnext_amd._lib import PnxError

    bb = _backbone()
    assert bb.half_dtype is None and bb.half_train_dtype is None
    assert bb.use_half_precision(training=True) is bb and bb.half_train_dtype == torch.bfloat16 and bb.half_dtype == torch.bfloat16
    assert bb.use_half_precision(torch.float16, training=True).half_train_dtype == torch.float16
    with pytest.raises(PnxError, match="training=True needs"):
        bb.use_half_precision(None, training=True)
    with pytest.raises(PnxError, match="use_half_precision"):
        bb.use_half_precision(torch.float32, training=True)
    assert bb.half_train_dtype == torch.float16 and bb.half_dtype == torch.float16  # a rejected call changes nothing
    bb.use_half_precision(torch.bfloat16)  # training=False: as before, the autograd path is fp32
    assert bb.half_dtype == torch.bfloat16 and bb.half_train_dtype is None
    bb.use_half_precision(torch.bfloat16, training=True).use_half_precision(None)
    assert bb.half_dtype is None and bb.half_train_dtype is None  # dtype=None switches both paths back
    # the node's boundary is fp32: a differentiable forward never runs on 16-bit rows
    bb.use_half_precision(torch.float16, training=True)
    x = torch.zeros((4, 5))
    assert bb.train()._differentiable(x) and bb._half(True) is None
    with torch.no_grad():
        assert bb.eval()._half(bb._differentiable(x)) == torch.float16


def test_training_weights_are_packed_once_per_weight_version():
    from pillarnext_amd import ops

    bb = _backbone().train()
    p = bb._train_packed(torch.bfloat16)
    convs = [m for m in bb.modules() if type(m).__name__ == "SparseConv3d"]
    assert set(p) == set(convs) and all(v.dtype == torch.bfloat16 for v in p.values())
    with torch.no_grad():
        bb.blocks[0][0].norm.running_mean.add_(1.0)  # what every training forward does: no new packing
    assert bb._train_packed(torch.bfloat16) is p
    h = bb._train_packed(torch.float16)
    assert h is not p and bb._train_packed(torch.bfloat16) is p
    with torch.no_grad():
        convs[0].weight.mul_(2.0)
    q = bb._train_packed(torch.bfloat16)
    assert q is not p and torch.equal(q[convs[0]], ops.sp3_pack_weight_h(convs[0].weight.detach(), torch.bfloat16))


def test_half_train_ops_check_their_arguments():
    from pillarnext_amd import ops
    from pillarnext_amd._lib import PnxError

    x, m = torch.zeros((4, 8), dtype=torch.bfloat16), torch.zeros((4, 27), dtype=torch.int32)
    with pytest.raises(PnxError):
        ops.sp3_conv_h_f32(x, m, torch.zeros(1, dtype=torch.bfloat16), 5, 18)  # CPU tensors
    with pytest.raises(PnxError):
        ops.sp3_wgrad_h(x, m, x, 5, 5)
    with pytest.raises(PnxError, match="no kernel"):
        ops.sp3_wgrad_h_partials_bytes(100, 27, 145, 16)


def test_half_train_entry_points_validate_before_launching():
    from pillarnext_amd import _lib

    L = _lib.lib()
    buf = (ctypes.c_char * 65536)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)
    odd = ctypes.c_void_p(p.value + 8)
    BF, HF = _lib.PNX_BF16, _lib.PNX_F16

    def check(rc, code, msg):
        err = L.pnx_last_error()
        assert rc == code and msg in err, (rc, err)

    # (x, n_in, cin, cin_pad, map, n_out, taps, w_packed, y, cout, dtype, stream)
    check(L.pnx_sp3_conv_h_f32(p, 8, 16, 16, p, 8, 27, p, p, 16, _lib.PNX_F32, None), -2, b"dtype 0")
    check(L.pnx_sp3_conv_h_f32(p, 8, 160, 160, p, 8, 27, p, p, 16, BF, None), -2, b"160 -> 16 channels")
    check(L.pnx_sp3_conv_h_f32(p, 8, 16, 16, p, 8, 27, p, p, 145, HF, None), -2, b"16 -> 145 channels")
    check(L.pnx_sp3_conv_h_f32(p, 8, 16, 16, p, 8, 28, p, p, 16, BF, None), -2, b"28 taps")
    check(L.pnx_sp3_conv_h_f32(p, 8, 5, 5, p, 8, 27, p, p, 18, BF, None), -1, b"padded channel counts 5 / 24")
    check(L.pnx_sp3_conv_h_f32(p, -1, 16, 16, p, 8, 27, p, p, 16, BF, None), -1, b"rows")
    check(L.pnx_sp3_conv_h_f32(p, 8, 16, 16, None, 8, 27, p, p, 16, BF, None), -1, b"null pointer")
    check(L.pnx_sp3_conv_h_f32(None, 8, 16, 16, p, 8, 27, p, p, 16, HF, None), -1, b"null pointer")
    check(L.pnx_sp3_conv_h_f32(p, 8, 16, 16, p, 8, 27, p, None, 16, BF, None), -1, b"null pointer")
    check(L.pnx_sp3_conv_h_f32(odd, 8, 16, 16, p, 8, 27, p, p, 16, BF, None), -1, b"16-byte aligned")
    check(L.pnx_sp3_conv_h_f32(p, 8, 16, 16, p, 8, 27, odd, p, 16, BF, None), -1, b"16-byte aligned")
    assert L.pnx_sp3_conv_h_f32(None, 0, 16, 16, None, 0, 27, None, None, 16, BF, None) == 0  # no rows: nothing is touched
    # (x, n_in, cin, cin_pad, dy, cout, cout_pad, map, n_out, taps, dw, dtype, partials, partials_bytes, stream)
    need = L.pnx_sp3_wgrad_h_partials_bytes(8, 27, 16, 16)
    assert need == 27 * 16 * 16 * 4 and need <= 65536 - 512
    check(L.pnx_sp3_wgrad_h(p, 8, 16, 16, p, 16, 16, p, 8, 27, p, _lib.PNX_F32, p, need, None), -2, b"dtype 0")
    check(L.pnx_sp3_wgrad_h(p, 8, 145, 152, p, 16, 16, p, 8, 27, p, BF, p, need, None), -2, b"145 -> 16 channels")
    check(L.pnx_sp3_wgrad_h(p, 8, 16, 16, p, 16, 16, p, 8, 28, p, HF, p, need, None), -2, b"28 taps")
    check(L.pnx_sp3_wgrad_h(p, 8, 5, 8, p, 18, 18, p, 8, 27, p, BF, p, need, None), -1, b"padded channel counts 8 / 18")
    check(L.pnx_sp3_wgrad_h(p, 8, 5, 5, p, 18, 24, p, 8, 27, p, BF, p, need, None), -1, b"padded channel counts 5 / 24")
    check(L.pnx_sp3_wgrad_h(p, 8, 16, 16, p, 16, 16, p, -1, 27, p, BF, p, need, None), -1, b"rows")
    check(L.pnx_sp3_wgrad_h(p, 8, 16, 16, p, 16, 16, p, 8, 27, None, BF, p, need, None), -1, b"dw is NULL")
    check(L.pnx_sp3_wgrad_h(p, 0, 16, 16, p, 16, 16, p, 0, 27, None, BF, p, need, None), -1, b"dw is NULL")
    check(L.pnx_sp3_wgrad_h(None, 8, 16, 16, p, 16, 16, p, 8, 27, p, BF, p, need, None), -1, b"null pointer")
    check(L.pnx_sp3_wgrad_h(p, 8, 16, 16, None, 16, 16, p, 8, 27, p, HF, p, need, None), -1, b"null pointer")
    check(L.pnx_sp3_wgrad_h(p, 8, 16, 16, p, 16, 16, None, 8, 27, p, BF, p, need, None), -1, b"null pointer")
    check(L.pnx_sp3_wgrad_h(p, 8, 16, 16, odd, 16, 16, p, 8, 27, p, BF, p, need, None), -1, b"16-byte aligned")
    check(L.pnx_sp3_wgrad_h(p, 8, 16, 16, p, 16, 16, p, 8, 27, p, BF, None, need, None), -1, b"workspace is NULL")
    check(L.pnx_sp3_wgrad_h(p, 8, 16, 16, p, 16, 16, p, 8, 27, p, BF, p, need - 1, None), -3, b"workspace too small")
    check(L.pnx_sp3_wgrad_h(p, 8, 16, 16, p, 16, 16, p, 8, 27, p, BF, odd, need, None), -1, b"256-byte aligned")
