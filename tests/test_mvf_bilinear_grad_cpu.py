"""CPU: the fp64 twin of the bilinear sampling's gradient (tests/mvf_bilinear_ref.py) against the reference's own autograd result
(tests/golden/mvf_bilinear_grad.npz, tools/gen_mvf_grad_golden.py), and the argument checks of ops.bilinear_gather_backward / the C entry point,
which come before any HIP call."""
import ctypes

import mvf_bilinear_ref as R
import numpy as np
import pytest
import torch
from conftest import load_golden


def fixture():
    parts, grad = load_golden("mvf_parts"), load_golden("mvf_bilinear_grad")
    return parts["bil_image"], parts["bil_coords"], grad["grad_out"], grad["grad_image"]


def test_the_twin_bounds_the_references_own_gradient():
    img, co, go, gi = fixture()
    assert img.shape == (2, 6, 9, 11) and co.shape == (200, 3) and go.shape == (200, 6) and gi.shape == img.shape
    S, A, k = R.grad_image(go, img.shape, co[:, 1:3], [0.0, 0.0], [1.0, 1.0], co[:, 0], 1)
    R.check(gi, S, A, k, "reference fixture")
    assert not np.any(gi[np.broadcast_to(k[:, None] == 0, gi.shape)] != 0) and not np.any(S[np.broadcast_to(k[:, None] == 0, S.shape)] != 0)
    assert int(k.sum()) == 4 * 200 and int((k > 0).sum()) == 185 and int(k.max()) == 24
    # the fixture exercises the reference's clamping rule: negative weights, and corners that clamping made one cell
    x0, x1, y0, y1, wa, wb, wc, wd = R.corners_and_weights(co[:, 1:3], [0.0, 0.0], [1.0, 1.0], 1, 9, 11)
    assert int(sum((w < 0).sum() for w in (wa, wb, wc, wd))) == 188 and int(((x0 == x1) | (y0 == y1)).sum()) == 94


def test_the_twin_reproduces_the_forward_fixture():
    """The same corners and weights give the committed forward output: the twin's weights are the reference's."""
    img, co, _, _ = fixture()
    parts = load_golden("mvf_parts")
    x0, x1, y0, y1, wa, wb, wc, wd = R.corners_and_weights(co[:, 1:3], [0.0, 0.0], [1.0, 1.0], 1, 9, 11)
    b = co[:, 0].astype(np.int64)
    out = (img[b, :, y0, x0] * wa[:, None] + img[b, :, y1, x0] * wb[:, None]) + img[b, :, y0, x1] * wc[:, None] + img[b, :, y1, x1] * wd[:, None]
    np.testing.assert_allclose(out, parts["bil_out"], rtol=0, atol=4 * R.U * np.abs(img).max() * 4)


def test_backward_op_refuses_cpu_tensors_and_bad_arguments():
    from pillarnext_amd import ops
    from pillarnext_amd._lib import PnxError

    n, C = 5, 6
    go, pos = torch.zeros((n, C)), torch.zeros((n, 2))
    cells, inv = torch.zeros((2, 3), dtype=torch.int32), torch.zeros((n,), dtype=torch.int64)
    shape, mn, vs = (2, C, 9, 11), [0.0, 0.0], [1.0, 1.0]
    with pytest.raises(PnxError, match="CUDA"):
        ops.bilinear_gather_backward(go, shape, pos, mn, vs, cells, inv, 1)
    with pytest.raises(PnxError, match="power of two"):
        ops.bilinear_gather_backward(go, shape, pos, mn, vs, cells, inv, 3)
    with pytest.raises(PnxError, match="grad_out"):
        ops.bilinear_gather_backward(go.double(), shape, pos, mn, vs, cells, inv, 1)
    with pytest.raises(PnxError, match="grad_out"):
        ops.bilinear_gather_backward(go[:, :5], shape, pos, mn, vs, cells, inv, 1)                    # fewer columns than channels
    with pytest.raises(PnxError, match="grad_out"):
        ops.bilinear_gather_backward(torch.zeros((C, n)).t(), shape, pos, mn, vs, cells, inv, 1)      # column stride != 1
    with pytest.raises(PnxError, match="grad_out"):
        ops.bilinear_gather_backward(torch.zeros((1, C)).expand(n, C), shape, pos, mn, vs, cells, inv, 1)   # row stride 0 < C
    with pytest.raises(PnxError, match="pos fp32"):
        ops.bilinear_gather_backward(go, shape, pos.double(), mn, vs, cells, inv, 1)
    with pytest.raises(PnxError, match="int32 coords"):
        ops.bilinear_gather_backward(go, shape, pos, mn, vs, cells.long(), inv, 1)
    with pytest.raises(PnxError, match="int64 unq_inv"):
        ops.bilinear_gather_backward(go, shape, pos, mn, vs, cells, inv.int(), 1)


def test_backward_entry_point_validates_before_launching():
    from pillarnext_amd import _lib

    L = _lib.lib()
    buf = (ctypes.c_char * 512)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)
    two = (ctypes.c_float * 2)(1.0, 1.0)
    call = lambda **kw: L.pnx_bilinear_gather_backward(*[{**dict(g=p, ld=6, b=2, h=9, w=11, c=6, pos=p, pld=2, mn=two, vs=two, cc=p, inv=p, ds=1, n=10, gi=p,  # noqa: E731
                                                                  ws=p, wsb=8, st=None), **kw}[k] for k in
                                                         ("g", "ld", "b", "h", "w", "c", "pos", "pld", "mn", "vs", "cc", "inv", "ds", "n", "gi", "ws", "wsb", "st")])
    assert call(ds=3) == -2 and b"power of two" in L.pnx_last_error()
    assert call(ds=0) == -2 and b"power of two" in L.pnx_last_error()
    assert call(ld=5) == -1 and b"grad_ld" in L.pnx_last_error()
    assert call(gi=None) == -1 and b"bad arguments" in L.pnx_last_error()
    assert call(g=None) == -1 and b"bad arguments" in L.pnx_last_error()
    assert call(pld=1) == -1 and b"bad arguments" in L.pnx_last_error()
    assert call(c=0, ld=0) == -1 and b"bad arguments" in L.pnx_last_error()
    assert call(b=1 << 15, h=1 << 8, w=1 << 8) == -2 and b"32-bit" in L.pnx_last_error()
    assert call(ws=ctypes.c_void_p(p.value + 4), wsb=1 << 20) == -1 and b"aligned" in L.pnx_last_error()   # the size is checked first: give it enough
    assert call() == -3 and b"workspace" in L.pnx_last_error()                                          # 8 bytes of workspace
    need = L.pnx_bilinear_gather_backward_workspace_bytes(10, 2, 9, 11)
    assert need >= 3 * 10 * 4 + (2 * 9 * 11 + 1) * 4 and need % 256 == 0
    assert L.pnx_bilinear_gather_backward_workspace_bytes(0, 2, 9, 11) >= 256
    assert L.pnx_bilinear_gather_backward_workspace_bytes(-1, 2, 9, 11) == 0
    assert L.pnx_bilinear_gather_backward_workspace_bytes(10, 1 << 15, 1 << 8, 1 << 8) == 0
    assert L.pnx_bilinear_gather_backward_workspace_bytes(360_000, 2, 256, 256) < 64 << 20
