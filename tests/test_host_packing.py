"""CPU: host-side packing helpers (plain torch, no GPU): the second-convolution weight layout of the lazy SepHead evaluator, the lazy
flavour of the decoder's task descriptor and the decoder's host layout (descriptors, key offsets, lists per task)."""
import struct

import numpy as np
import pytest
import torch

from pillarnext_amd import ops
from pillarnext_amd.decode import pack_task


def test_lazy_second_conv_weight_layout():
    off, k = [0, 2, 3, 6, 8], [2, 1, 3, 2, 2]
    g = torch.Generator().manual_seed(1)
    w2m = torch.zeros((9 * 320, 10))
    for pos in range(9):
        for j in range(5):
            w2m[pos * 320 + 64 * j: pos * 320 + 64 * (j + 1), off[j]:off[j] + k[j]] = torch.randn((64, k[j]), generator=g)
    p = ops.sephead_lazy_pack_w2(w2m)
    assert p.shape == (10, 9, 32, 3)
    for mt in range(10):
        j = mt // 2
        for pos in (0, 4, 8):
            for cl in (0, 17, 31):
                row = w2m[pos * 320 + mt * 32 + cl]
                assert torch.equal(p[mt, pos, cl, :k[j]], row[off[j]:off[j] + k[j]])
                assert bool((p[mt, pos, cl, k[j]:] == 0).all())
                assert float(row.abs().sum()) == float(p[mt, pos, cl].abs().sum())     # nothing outside the branch's own outputs


def test_lazy_task_descriptor_points_at_the_class_map_only():
    args = (16, True, 2, 3, 360, 360, 4, (0.075, 0.075), (-54.0, -54.0), 0.1, [-61.2, -61.2, -10, 61.2, 61.2, 10], [0.5, 0.5])
    dense, lazy = pack_task(*args), pack_task(*args, lazy=True)
    assert len(dense) == len(lazy) == 104
    d, z = struct.unpack("6i6f6fi4f3i", dense), struct.unpack("6i6f6fi4f3i", lazy)
    assert d[:23] == z[:23]                                  # geometry, thresholds, range, rectifier: the same
    assert d[-3:] == (11, 10, 0) and z[-3:] == (1, 0, 1)     # o_hm, o_iou, lazy: [reg .. vel | iou | hm] vs [iou | hm]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("num_classes", [[1, 2], [1, 2, 2, 1, 2, 2]])
def test_decoder_host_layout(num_classes, B):
    """PackedDecoder.host_layout (what launch, launch_lazy and launch_lazy_fused all start from) against the layout stated here: lists
    s = sample * nc_total + class; the keys of task t are the B*H_t*W_t cells of its map, tasks concatenated in order."""
    from pillarnext_amd.decode import PackedDecoder

    T, nc_total = len(num_classes), sum(num_classes)
    shapes = [(8, 8), (4, 6), (5, 3), (8, 8), (2, 7), (6, 4)][:T]                        # unequal maps per task
    lazy_ch, dense_ch = [16, 8, 16, 4, 16, 16][:T], [16, 17, 13, 16, 14, 15][:T]
    rect = [[0.5 + 0.01 * t] * n for t, n in enumerate(num_classes)]
    cfg = dict(nms=dict(nms_pre_max_size=7, nms_post_max_size=3, nms_iou_threshold=[[0.2] * n for n in num_classes]), score_threshold=0.1,
               pc_range=[-25.6, -25.6], voxel_size=[0.1, 0.1], out_size_factor=[8, 4, 8, 2, 8, 8][:T], post_center_limit_range=[-30, -30, -10, 30, 30, 10])
    dec = PackedDecoder(num_classes, rect, cfg, True, dense_ch)
    owner = []                                                                           # the task that owns class c
    for t, n in enumerate(num_classes):
        owner += [t] * n
    want_offs = [int(v) for v in np.concatenate([[0], np.cumsum([B * h * w for h, w in shapes])])]
    for lazy, channels in ((True, lazy_ch), (False, dense_ch)):
        lay = dec.host_layout(lazy, B, shapes, channels)
        assert lay.S == B * nc_total
        assert list(lay.offs) == want_offs                                               # running sum of B*H*W
        assert list(lay.kofs) == [want_offs[owner[s % nc_total]] for s in range(lay.S)]  # offset of the task that owns class s % nc_total
        assert len(lay.segs) == T and sorted(s for rows in lay.segs for s in rows) == list(range(lay.S))       # disjoint, cover range(S)
        for t, rows in enumerate(lay.segs):
            assert list(rows) == sorted(rows) and all(owner[s % nc_total] == t for s in rows)
        for t, (H, W) in enumerate(shapes):
            assert lay.descs[t] == pack_task(channels[t], True, num_classes[t], sum(num_classes[:t]), H, W, cfg["out_size_factor"][t], cfg["voxel_size"],
                                             cfg["pc_range"], 0.1, cfg["post_center_limit_range"], rect[t], lazy=lazy)


def test_launch_table_structures_mirror_the_c_ones():
    """plan.PnxOp / decode._PnxLazyDecode are ctypes mirrors of include/pnx.h's pnx_op / pnx_lazy_decode: same size as the compiled ones,
    pointers 8-byte aligned behind the integer block."""
    import ctypes

    from pillarnext_amd import _lib, decode, plan

    L = _lib.lib()
    assert ctypes.sizeof(plan.PnxOp) == L.pnx_op_bytes() == 128
    assert plan.PnxOp.p.offset == 40 and plan.PnxOp.i.offset == 4
    assert ctypes.sizeof(decode._PnxLazyDecode) == L.pnx_lazy_decode_bytes()
    assert decode._PnxLazyDecode.dense_host.offset == 24 and decode._PnxLazyDecode.flag_host.offset == L.pnx_lazy_decode_bytes() - 8
