"""CPU: the interface of the sparse-rows path of the MVF view nets (SingleView.use_sparse_rows): switches, unchanged state dict, the weight view,
the column blocks of ops.sp3_wgrad, the entry points that keep their ranges, and the refusal of CPU tensors."""
import ctypes

import pytest

torch = pytest.importorskip("torch")


def _net():
    from pillarnext_amd.mvf_encoder import MVFFeatureNet

    return MVFFeatureNet(5, [0.5, 0.5, 6.0], [0.0, 0.0, -2.0, 16.0, 16.0, 4.0], [1.8, 0.5, 16.0], [-180.0, -2.0, 0.0, 180.0, 4.0, 16.0], [16], [1, 1],
                         [1, 2], [8, 12], [3, 3], 16)


def test_switches_exist_and_return_self():
    net = _net()
    assert not net.pillarview.sparse_rows and not net.cylinderview.sparse_rows          # off by default
    assert net.use_sparse_rows() is net and net.pillarview.sparse_rows and net.cylinderview.sparse_rows
    assert net.use_sparse_rows(views=("pillar",)) is net and net.pillarview.sparse_rows and not net.cylinderview.sparse_rows
    assert net.use_sparse_rows(False) is net and not net.pillarview.sparse_rows and not net.cylinderview.sparse_rows
    v = net.cylinderview
    assert v.use_sparse_rows() is v and v.sparse_rows and v.use_sparse_rows(False) is v and not v.sparse_rows
    from pillarnext_amd._lib import PnxError

    with pytest.raises(PnxError, match="unknown views"):
        net.use_sparse_rows(views=("bev",))
    # use_hip_convs is another switch: neither touches the other
    net.use_sparse_rows().use_hip_convs(torch.bfloat16)
    assert net.pillarview.sparse_rows and net.pillarview.conv_dtype is torch.bfloat16
    net.use_hip_convs(None)
    assert net.pillarview.sparse_rows and net.pillarview.conv_dtype is None


def test_state_dict_is_the_same_either_way():
    a, b = _net(), _net().use_sparse_rows()
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(sa[k].shape == sb[k].shape and sa[k].dtype == sb[k].dtype for k in sa)
    assert [n for n, _ in a.named_modules()] == [n for n, _ in b.named_modules()]
    b.load_state_dict(sa)            # checkpoints written either way load either way
    a.load_state_dict(b.state_dict())
    assert sa["pillarview.blocks.1.0.conv.weight"].shape == (12, 8, 3, 3)


def test_weight_view_shares_the_parameter():
    from pillarnext_amd.mvf_encoder import sparse_weight_view

    conv = _net().pillarview.blocks[1][0].conv
    w = sparse_weight_view(conv)
    assert tuple(w.shape) == (12, 1, 3, 3, 8)
    assert w.untyped_storage().data_ptr() == conv.weight.untyped_storage().data_ptr() and w._base is not None
    assert torch.equal(w[:, 0], conv.weight.permute(0, 2, 3, 1))
    g = torch.randn(w.shape)
    (w * g).sum().backward()         # autograd delivers dW in the parameter's own layout
    assert conv.weight.grad.shape == conv.weight.shape and torch.equal(conv.weight.grad, g[:, 0].permute(0, 3, 1, 2))


def test_entry_points_keep_their_ranges():
    from pillarnext_amd import _lib

    L = _lib.lib()
    assert L.pnx_sp3_wgrad_workspace_bytes(100, 9, 145, 16) == 0 and L.pnx_sp3_wgrad_workspace_bytes(100, 9, 16, 160) == 0
    assert L.pnx_sp3_wgrad_workspace_bytes(100, 9, 144, 144) > 0
    assert L.pnx_sp3_wgrad_h_partials_bytes(100, 9, 145, 16) == 0 and L.pnx_sp3_packed_weight_halfs(9, 16, 145) == 0
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)
    assert L.pnx_sp3_wgrad(p, 10, 145, p, 16, p, 10, 9, p, p, 1 << 20, None) == -2 and b"channels 1..144" in L.pnx_last_error()
    # the forward's ceiling moved to 192 output channels, and no further
    assert L.pnx_sp3_conv(p, 10, 16, p, 10, 9, p, p, None, 1, p, 193, None) == -2 and b"cout 1..192" in L.pnx_last_error()
    assert L.pnx_sp3_conv_train(p, 10, 16, p, 10, 9, p, p, None, 1, p, 193, None) == -2 and b"cout 1..192" in L.pnx_last_error()
    assert L.pnx_sp3_conv(p, 10, 16, p, 0, 9, p, p, None, 1, p, 192, None) == 0         # accepted: no output rows, nothing launched


def test_wgrad_column_blocks():
    from pillarnext_amd import ops

    blocks = ops.sp3_wgrad_blocks
    assert blocks(1) == [(0, 1)] and blocks(144) == [(0, 144)]
    assert blocks(145) == [(0, 80), (80, 65)]
    assert blocks(150) == [(0, 80), (80, 70)]
    assert blocks(176) == [(0, 96), (96, 80)]
    assert blocks(192) == [(0, 96), (96, 96)]
    assert blocks(288) == [(0, 144), (144, 144)] and blocks(289) == [(0, 112), (112, 112), (224, 65)]
    for c in range(1, 700):
        b = blocks(c)
        assert b[0][0] == 0 and all(s + k == t for (s, k), (t, _) in zip(b, b[1:])) and b[-1][0] + b[-1][1] == c       # a partition of the columns
        assert all(1 <= k <= 144 for _, k in b) and (len(b) == 1 or all(k % 16 == 0 for _, k in b[:-1]))
        assert len({k for _, k in b[:-1]}) <= 1 and b[-1][1] <= b[0][1]                                                      # equal blocks, the last the rest
    with pytest.raises(ops.PnxError):
        blocks(0)


def test_cpu_tensors_are_refused():
    from pillarnext_amd import ops
    from pillarnext_amd._lib import PnxError

    view = _net().pillarview.use_sparse_rows().eval()
    unq = torch.tensor([[0, 1, 2], [0, 3, 3]], dtype=torch.int32)
    with pytest.raises(PnxError, match="CUDA"):
        view.sparse_sets(torch.zeros((2, 16)), unq, 1, 32, 32)
    with pytest.raises(PnxError):
        ops.sp3_wgrad(torch.zeros((4, 192)), torch.zeros((4, 9), dtype=torch.int32), torch.zeros((4, 192)))
    with pytest.raises(PnxError):
        ops.sp3_bilinear_gather(torch.zeros((2, 8)), None, torch.zeros((1, 2)), [0, 0], [1, 1], unq, torch.zeros((1,), dtype=torch.int64), 2)
    with pytest.raises(PnxError):
        ops.SparseBilinearGather.apply(torch.zeros((2, 8)), None, None, torch.zeros((1, 2)), [0, 0], [1, 1], unq, torch.zeros((1,), dtype=torch.int64), 2)
