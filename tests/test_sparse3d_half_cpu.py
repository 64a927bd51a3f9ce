"""CPU: the host side of SparseResNet3D's 16-bit inference path.
  - ops.sp3_pack_weight_h against a numpy statement of the fragment layout (tests/sparse3d_half_ref.py), CPU tensors
  - SparseResNet3D.use_half_precision: argument checks; a module in train() still takes the autograd path
  - the rounding emulation the GPU tests are held to: idempotent, equal to torch.Tensor.to(dtype) on fp32 values, one rounding from fp64
  - the argument checks of pnx_sp3_conv_h / pnx_sp3_dense_h, which come before any HIP call."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sparse3d_half_ref as HR  # noqa: E402

DTYPES = [torch.bfloat16, torch.float16]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("cin,cout,k", [(5, 18, (3, 3, 3)), (16, 16, (3, 3, 3)), (144, 128, (1, 1, 1)), (16, 16, (3, 1, 1))])
def test_pack_weight_h_is_the_fragment_layout(cin, cout, k, dtype):
    from pillarnext_amd import _lib, ops

    rng = np.random.default_rng(cin * 100 + cout)
    w = rng.standard_normal((cout, *k, cin)).astype(np.float32)
    T = k[0] * k[1] * k[2]
    p = ops.sp3_pack_weight_h(torch.from_numpy(w), dtype)
    ref = HR.pack_weight_h_ref(w, dtype)
    assert p.dtype == dtype and not p.is_cuda and p.is_contiguous()
    assert tuple(p.shape) == ref.shape == ((T * ((cin + 7) // 8 * 8) + 31) // 32, (cout + 15) // 16, 64, 8)
    assert p.numel() == _lib.lib().pnx_sp3_packed_weight_halfs(T, cin, cout)
    assert np.array_equal(p.double().numpy(), ref)
    assert np.count_nonzero(ref) == np.count_nonzero(HR.round_to(w, dtype))  # every weight lands once, everything else is zero


def test_pack_weight_h_rejects_what_has_no_kernel():
    from pillarnext_amd import _lib, ops

    L = _lib.lib()
    assert L.pnx_sp3_packed_weight_halfs(27, 145, 16) == 0 and L.pnx_sp3_packed_weight_halfs(28, 16, 16) == 0
    assert L.pnx_sp3_packed_weight_halfs(27, 16, 0) == 0 and L.pnx_sp3_packed_weight_halfs(27, 16, 16) == 14 * 512
    with pytest.raises(_lib.PnxError, match="no packing"):
        ops.sp3_pack_weight_h(torch.zeros((16, 3, 3, 3, 160)), torch.bfloat16)
    with pytest.raises(_lib.PnxError, match="bfloat16"):
        ops.sp3_pack_weight_h(torch.zeros((16, 3, 3, 3, 16)), torch.float32)
    with pytest.raises(_lib.PnxError, match="bfloat16"):
        ops.sp3_rows_h(torch.zeros((3, 5)), torch.float64)
    r = ops.sp3_rows_h(torch.full((3, 5), 1.00390625), torch.bfloat16)  # 1 + 2^-8: a tie, to even
    assert tuple(r.shape) == (3, 8) and r.dtype == torch.bfloat16 and bool((r[:, :5] == 1).all()) and not bool(r[:, 5:].any())


def _backbone():
    from pillarnext_amd.sparse3d import SparseResNet3D

    return SparseResNet3D(layer_nums=[1, 1], ds_layer_strides=[1, 2], ds_num_filters=[16, 32], num_input_features=5)


def test_use_half_precision_argument_checks():
    from pillarnext_amd._lib import PnxError

    bb = _backbone()
    assert bb.half_dtype is None
    assert bb.use_half_precision() is bb and bb.half_dtype == torch.bfloat16
    assert bb.use_half_precision(torch.float16).half_dtype == torch.float16
    assert bb.use_half_precision(None).half_dtype is None
    for bad in (torch.float32, torch.float64, torch.int8, "bf16"):
        with pytest.raises(PnxError, match="use_half_precision"):
            bb.use_half_precision(bad)
    assert bb.half_dtype is None  # a rejected call changes nothing
    bb.use_half_precision()
    feats, coords = torch.zeros((4, 5), dtype=torch.bfloat16), torch.zeros((4, 4), dtype=torch.int32)
    with torch.no_grad(), pytest.raises(PnxError, match=r"features must be fp32, got torch.bfloat16 \(there is no bf16 / fp16 form\)"):
        bb.eval()(feats, coords, (8, 8, 8))  # inputs stay fp32 whatever the layers run in


def test_training_and_gradients_keep_the_autograd_path():
    bb = _backbone().use_half_precision()
    x = torch.zeros((4, 5))
    assert bb.train()._differentiable(x) and bb._half(bb._differentiable(x)) is None
    bb.eval()
    assert bb._differentiable(x) and bb._half(True) is None  # eval, gradients enabled, parameters require one
    with torch.no_grad():
        assert not bb._differentiable(x) and bb._half(bb._differentiable(x)) == torch.bfloat16
    for p in bb.parameters():
        p.requires_grad_(False)
    assert not bb._differentiable(x) and bb._differentiable(x.clone().requires_grad_(True))


def test_folded_plan_is_cached_per_version_and_dtype():
    bb = _backbone().eval()
    f32 = bb._folded()
    assert bb._folded() is f32 and f32["mapping"][0].dtype == torch.float32
    b16 = bb._folded(torch.bfloat16)
    assert bb._folded(torch.bfloat16) is b16 and bb._folded() is f32  # the two plans live side by side
    assert all(w.dtype == torch.bfloat16 and s.dtype == torch.float32 for w, s in b16.values()) and set(b16) == set(f32)
    h16 = bb._folded(torch.float16)
    assert h16 is not b16 and h16["blocks.0.0"][0].dtype == torch.float16
    with torch.no_grad():
        bb.blocks[0][0].conv.weight.mul_(2.0)  # a new parameter version
    again = bb._folded(torch.float16)
    assert again is not h16 and not torch.equal(again["blocks.0.0"][0], h16["blocks.0.0"][0])
    conv, bn = bb.blocks[0][0].conv, bb.blocks[0][0].norm
    a = bn.weight.detach() * torch.rsqrt(bn.running_var + bn.eps)
    want = HR.pack_weight_h_ref((conv.weight.detach() * a.view(-1, 1, 1, 1, 1)).numpy(), torch.float16)  # folded in fp32, rounded once
    assert np.array_equal(again["blocks.0.0"][0].double().numpy(), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_rounding_emulation(dtype):
    rng = np.random.default_rng(3)
    tiny = float(torch.finfo(dtype).tiny)
    x32 = np.concatenate([rng.standard_normal(4000) * 10.0 ** rng.integers(-9, 5, 4000), [0.0, -0.0, 1.0, 1.00390625, 1.01171875, tiny, tiny / 4, -tiny * 0.75,
                                                                                          65504.0, 65519.9, 65520.0, -7e4, 3e38]]).astype(np.float32)
    want = torch.from_numpy(x32).to(dtype).double().numpy()  # fp32 -> dtype is one rounding to nearest even
    got = HR.round_to(x32.astype(np.float64), dtype)
    assert np.array_equal(got, want)
    assert np.array_equal(HR.round_to(got, dtype), got)  # idempotent
    t = HR.round_to(torch.from_numpy(x32).double(), dtype)
    assert t.dtype == torch.float64 and np.array_equal(t.numpy(), want)
    # straight from fp64: 1 + h + 2^-40 lies above the tie 1 + h (h = half a spacing) and rounds up; through fp32 it would first fall onto the tie, then to even
    h = HR.U[dtype]
    assert HR.round_to(np.array([1.0 + h + 2.0 ** -40]), dtype)[0] == 1.0 + 2 * h and HR.round_to(np.array([1.0 + h]), dtype)[0] == 1.0
    assert abs(HR.round_to(np.array([np.pi]), dtype)[0] - np.pi) <= h * np.pi


def test_half_entry_points_validate_before_launching():
    from pillarnext_amd import _lib

    L = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p((base + 255) & ~255)
    odd = ctypes.c_void_p(p.value + 8)
    g = (ctypes.c_int32 * 3)(4, 4, 4)

    def check(rc, code, msg):
        err = L.pnx_last_error()
        assert rc == code and msg in err, (rc, err)

    # (x, n_in, cin, cin_pad, map, n_out, taps, w_packed, shift, residual, relu, y, cout, cout_pad, dtype, stream)
    check(L.pnx_sp3_conv_h(p, 8, 16, 16, p, 8, 27, p, p, None, 1, p, 16, 16, _lib.PNX_F32, None), -2, b"dtype 0")
    check(L.pnx_sp3_conv_h(p, 8, 160, 160, p, 8, 27, p, p, None, 1, p, 16, 16, _lib.PNX_BF16, None), -2, b"160 -> 16 channels")
    check(L.pnx_sp3_conv_h(p, 8, 16, 16, p, 8, 28, p, p, None, 1, p, 16, 16, _lib.PNX_BF16, None), -2, b"28 taps")
    check(L.pnx_sp3_conv_h(p, 8, 16, 16, p, 8, 0, p, p, None, 1, p, 16, 16, _lib.PNX_F16, None), -2, b"0 taps")
    check(L.pnx_sp3_conv_h(p, 8, 5, 5, p, 8, 27, p, p, None, 1, p, 18, 24, _lib.PNX_BF16, None), -1, b"padded channel counts 5 / 24")
    check(L.pnx_sp3_conv_h(p, 8, 5, 8, p, 8, 27, p, p, None, 1, p, 18, 18, _lib.PNX_BF16, None), -1, b"padded channel counts 8 / 18")
    check(L.pnx_sp3_conv_h(p, 8, 16, 16, None, 8, 27, p, p, None, 1, p, 16, 16, _lib.PNX_BF16, None), -1, b"null pointer")
    check(L.pnx_sp3_conv_h(None, 8, 16, 16, p, 8, 27, p, p, None, 1, p, 16, 16, _lib.PNX_BF16, None), -1, b"null pointer")
    check(L.pnx_sp3_conv_h(p, 8, 16, 16, p, 8, 27, p, None, None, 1, p, 16, 16, _lib.PNX_F16, None), -1, b"null pointer")
    check(L.pnx_sp3_conv_h(p, 8, 16, 16, p, 8, 27, p, p, odd, 1, p, 16, 16, _lib.PNX_BF16, None), -1, b"16-byte aligned")
    check(L.pnx_sp3_conv_h(p, 8, 16, 16, p, -1, 27, p, p, None, 1, p, 16, 16, _lib.PNX_BF16, None), -1, b"rows")
    assert L.pnx_sp3_conv_h(None, 0, 16, 16, None, 0, 27, None, None, None, 1, None, 16, 16, _lib.PNX_BF16, None) == 0  # no rows: nothing is touched
    # (feat, dtype, coords, n, channels, channels_pad, batch, grid, out, stream)
    check(L.pnx_sp3_dense_h(p, _lib.PNX_F32, p, 8, 128, 128, 1, g, p, None), -2, b"dtype 0")
    check(L.pnx_sp3_dense_h(p, _lib.PNX_BF16, p, 8, 18, 18, 1, g, p, None), -1, b"padded to 18")
    check(L.pnx_sp3_dense_h(p, _lib.PNX_BF16, None, 8, 128, 128, 1, g, p, None), -1, b"null pointer")
    check(L.pnx_sp3_dense_h(p, _lib.PNX_F16, p, 8, 128, 128, 1, None, p, None), -1, b"grid is NULL")
    assert L.pnx_sp3_dense_h(None, _lib.PNX_F16, None, 0, 128, 128, 0, g, None, None) == 0  # a batch of 0 samples
