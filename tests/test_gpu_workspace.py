"""GPU: the two statements about scratch memory (include/pnx.h: the workspace contract; ops.Workspace).

1. ops.Workspace keeps one grow-only buffer per (device, current stream), every pointer 256-byte aligned, and `.buf` follows the current stream.
2. An entry point needs no more than pnx_*_workspace_bytes: called with exactly that much at the front of a buffer painted 0xA5, it leaves the
   4096 bytes behind it untouched and computes, bit for bit, what it computes in four times the room.  Each entry runs at the smallest shape at
   which every field of its layout is non-empty; the inputs come from the helpers of the entries' own GPU tests."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 4096


# ------------------------------------------------------------------------------------------------------ 1: Workspace
def test_workspace_is_per_device_and_stream():
    from pillarnext_amd import ops

    dev = torch.device("cuda", torch.cuda.current_device())
    w = ops.Workspace()
    assert w.buf is None
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a = w.get(1000, dev)
        assert w.buf is a
    with torch.cuda.stream(s2):
        b = w.get(1000, dev)
        assert w.buf is b
    assert a.data_ptr() != b.data_ptr(), "two streams share one buffer"
    assert w.buf is None                                     # nothing was asked for on the default stream
    with torch.cuda.stream(s1):
        assert w.get(1000, dev) is a and w.get(1, dev) is a and w.get(a.numel(), dev) is a
        big = w.get(a.numel() + 1, dev)
        assert big is not a and big.numel() > a.numel() and w.buf is big and w.get(1000, dev) is big
    with torch.cuda.stream(s2):
        assert w.get(1000, dev) is b and w.buf is b          # the other stream's buffer did not change
    for t in (a, b, big):
        assert t.dtype == torch.uint8 and t.device == dev and t.data_ptr() % 256 == 0 and t.numel() >= 1000


def test_workspace_second_device_gets_its_own_buffer():
    from pillarnext_amd import ops

    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    dev = torch.device("cuda", torch.cuda.current_device())
    other = torch.device("cuda", (dev.index + 1) % torch.cuda.device_count())
    w = ops.Workspace()
    a = w.get(1000, dev)
    c = w.get(1000, other)
    assert c.device == other and c.data_ptr() % 256 == 0 and w.get(1000, other) is c
    assert w.get(1000, dev) is a and w.buf is a, "the first device's buffer is no longer the object it was"


# ------------------------------------------------------------------------------------------------------ 2: exactly workspace_bytes is enough
class Exact:
    """Stands where an ops.Workspace stands: hands out exactly the bytes asked for, at the front of a buffer painted 0xA5 with GUARD bytes behind
    them -- or, roomy, four times the request, all of it."""

    def __init__(self, roomy=False):
        self.roomy, self.need, self.whole = roomy, None, None

    def get(self, nbytes, device):
        self.need = int(nbytes)
        self.whole = torch.full((4 * self.need if self.roomy else self.need + GUARD,), 0xA5, dtype=torch.uint8, device=device)
        assert self.whole.data_ptr() % 256 == 0
        return self.whole if self.roomy else self.whole[:self.need]

    def guard_intact(self):
        return not self.roomy and bool((self.whole[self.need:] == 0xA5).all()) and self.whole.numel() - self.need == GUARD


def exact_then_roomy(run, need):
    """run(workspace stand-in) -> the call's outputs.  Once in exactly `need` bytes, once in 4 x need."""
    tight, roomy = Exact(), Exact(roomy=True)
    first = [t.clone() for t in run(tight)]
    torch.cuda.synchronize()
    assert tight.need == int(need) > 0, (tight.need, need)
    assert tight.guard_intact(), "the call wrote behind workspace_bytes"
    assert bool((tight.whole[:tight.need] != 0xA5).any()), "the call never touched its workspace"
    second = run(roomy)
    torch.cuda.synchronize()
    assert roomy.need == tight.need and len(first) == len(second) > 0
    for i, (x, y) in enumerate(zip(first, second)):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), i


def test_merge_in_exactly_its_workspace():
    from pillarnext_amd import _lib
    from pillarnext_amd.io import SweepMerger
    from test_gpu_merge import _sample

    sweeps = _sample(np.random.default_rng(3), 0, 2, 1016)                       # 1016 + 1033 = 2049 rows: a second scan block of one row
    raw = torch.from_numpy(np.concatenate([s["points"] for s in sweeps])).cuda()
    assert raw.shape[0] == 2049
    segs, o = [], 0
    for s in sweeps:
        segs.append(dict(begin=o, end=o + len(s["points"]), batch=s["batch"], time=s["time"], radius=s["radius"], transform=s["transform"]))
        o += len(s["points"])

    def run(ws):
        m = SweepMerger()
        m._ws = ws
        out, n_out = m(raw, segs, n_copy=4, out=torch.zeros((2049, 6), device="cuda"))
        assert 0 < int(n_out.item()) < 2049
        return [out, n_out]

    exact_then_roomy(run, _lib.lib().pnx_merge_sweeps_workspace_bytes(2049))


def test_topk_in_exactly_its_workspace():
    from pillarnext_amd._lib import check, lib, ptr, stream_ptr

    L = lib()
    n, S, pre_max = 16384 + 1, 2, 8                                              # kRsChunk + 1 keys: a second chunk of one key
    g = torch.Generator(device="cuda").manual_seed(4)
    seg = torch.arange(n, device="cuda") % S
    sc = (torch.rand((n,), device="cuda", generator=g) * 0.9 + 0.1).to(torch.bfloat16).float()       # ties, as in test_gpu_decode.py
    keys = (seg.to(torch.int64) << 32) | (0xFFFFFFFF - sc.view(torch.int32).to(torch.int64))
    need = int(L.pnx_decode_topk_workspace_bytes(n, S))

    def run(ws):
        w = ws.get(need, keys.device)
        out = [torch.zeros((S * pre_max,), dtype=torch.int64, device="cuda"), torch.zeros((S * pre_max,), dtype=torch.int64, device="cuda"),
               torch.zeros((S,), dtype=torch.int64, device="cuda"), torch.zeros((S,), dtype=torch.int32, device="cuda"),
               torch.zeros((S,), dtype=torch.int32, device="cuda")]
        check(L.pnx_decode_topk(ptr(keys), n, S, pre_max, *[ptr(t) for t in out], ptr(w), w.numel(), stream_ptr()), "pnx_decode_topk")
        assert out[3].tolist() == [pre_max] * S
        return out

    exact_then_roomy(run, need)


def test_center_loss_forward_then_backward_in_exactly_its_workspace():
    from pillarnext_amd._lib import check, lib, ptr, stream_ptr
    from test_gpu_loss import _case

    L = lib()
    B, H, W, M, C = 2, 8, 8, 8, 2
    pd, ex = _case(5, B=B, H=H, W=W, M=M, ncls=C, n_pos=5)
    maps = [pd[k].float().contiguous() for k in ("hm", "reg", "height", "dim", "rot", "vel", "iou")]
    hm_t, ind, mask, cat, anno, gtb = (ex[k][0].contiguous() for k in ("hm", "ind", "mask", "cat", "anno_box", "gt_boxes"))
    a_m = (ctypes.c_void_p * 7)(*[t.data_ptr() for t in maps])
    g4 = (ctypes.c_float * 4)(0.8, 0.8, -20.0, -16.0)
    up = torch.ones(13, dtype=torch.float32, device="cuda")
    need = int(L.pnx_center_loss_workspace_bytes(B, M))

    def run(ws):
        w = ws.get(need, hm_t.device)
        losses = torch.zeros(16, dtype=torch.float32, device="cuda")
        check(L.pnx_center_loss_forward(a_m, ptr(hm_t), ptr(ind), ptr(mask), ptr(cat), ptr(anno), ptr(gtb), B, C, H, W, M, g4, 1, ptr(losses), ptr(w),
                                        w.numel(), stream_ptr()), "pnx_center_loss_forward")
        grads = [torch.empty_like(maps[0])] + [torch.zeros_like(t) for t in maps[1:]]
        a_g = (ctypes.c_void_p * 7)(*[t.data_ptr() for t in grads])
        coef = torch.zeros(4, dtype=torch.float32, device="cuda")
        check(L.pnx_center_loss_backward(a_m, a_g, ptr(hm_t), ptr(ind), ptr(mask), ptr(cat), ptr(anno), ptr(gtb), B, C, H, W, M, g4, 1, ptr(losses), ptr(up),
                                         ptr(coef), ptr(w), w.numel(), stream_ptr()), "pnx_center_loss_backward")
        assert float(losses[0]) > 0 and float(grads[1].abs().sum()) > 0
        return [losses, *grads]

    exact_then_roomy(run, need)


def test_assign_in_exactly_its_workspace():
    from pillarnext_amd import ops
    from test_gpu_assign import KEYS, make

    a, _ = make([1, 1], [0.0, 0.0, -1.0, 8.0, 8.0, 1.0], [0.5, 0.5, 2.0], [2, 2], max_objs=8)      # 2 tasks, 8 objects, 8 x 8 maps
    assert a.map_size == [(8, 8), (8, 8)]
    b = np.zeros((2, 8, 9), np.float32)
    b[:, :, 0], b[:, :, 1] = 0.7 + 0.9 * np.arange(8), [[3.3], [5.1]]
    b[:, :, 3:6], b[:, :, 8] = 0.9, np.linspace(-3, 3, 8)
    boxes, cls = torch.from_numpy(b).cuda(), torch.from_numpy((np.arange(16).reshape(2, 8) % 2).astype(np.int32)).cuda()
    out, counts, _, desc = a._buffers(2, boxes.device)
    need = ops.assign_workspace_bytes(2, 2, 8)

    def run(ws):
        ops.assign_labels(boxes, cls, None, desc, out, counts, ws.get(need, boxes.device))
        assert counts.tolist() == [[4, 4], [4, 4]]
        return [counts] + [t for k in KEYS for t in out[k]]

    exact_then_roomy(run, need)


def test_paste_in_exactly_its_workspace():
    import paste_augment_cases as C
    from pillarnext_amd import ops
    from test_gpu_paste_augment import dev, dev_cand, run_select

    total, B, S = ops.paste_chunk_rows() + 1, 2, 2                                # a second chunk of one row; frames 0 and 1 of the case, 2 candidates
    c = C.points_batch(total)
    cand = {k: v[:B, :S] for k, v in c["cand"].items()}
    sel = run_select(c["gt"][:B], c["cls"][:B], c["num_gt"][:B], cand, c["bank_offsets"], c["n_groups"])
    points, dcand, bank_points, bank_offsets = dev(c["points"]), dev_cand(cand), dev(c["bank_points"]), dev(c["bank_offsets"])
    capacity = total + int(np.diff(c["bank_offsets"])[cand["bank"][cand["bank"] >= 0]].sum())
    need = ops.paste_augment_workspace_bytes(total, B)

    def run(ws):
        out = torch.full((capacity, points.shape[1]), 12345.0, dtype=torch.float32, device="cuda")
        n_out, frame_rows = torch.full((1,), -7, dtype=torch.int32, device="cuda"), torch.full((B,), -7, dtype=torch.int32, device="cuda")
        ops.paste_augment_points(points, B, dcand, sel["paste_offset"], sel["pasted_rows"], bank_points, bank_offsets, None, out, n_out, frame_rows,
                                 ws.get(need, points.device))
        assert int(n_out.item()) > 0 and not bool((out == 12345.0).any())
        return [out, n_out, frame_rows]

    exact_then_roomy(run, need)


def test_rotated_nms_in_exactly_its_workspace(monkeypatch):
    from pillarnext_amd import _lib, ops, synth
    from test_gpu_iou_nms import cu

    boxes = cu(np.concatenate([synth.clustered_boxes(65, 400 + i)[0] for i in range(2)]))            # 2 segments of 65 boxes: two mask words per row
    off, thr = cu(np.array([0, 65, 130]), torch.int32), cu(np.array([0.2, 0.25], np.float32))

    def run(ws):
        monkeypatch.setattr(ops, "_NMS_WS", ws)
        keep, cnt = ops.nms_batched(boxes, off, thr, 65, post_max=0)
        cnt = cnt[:2].clone()
        assert 0 < int(cnt.min()) and int(cnt.max()) < 65
        valid = torch.arange(65, device="cuda")[None, :] < cnt[:, None]                              # keep is defined up to each segment's count
        return [cnt, torch.where(valid, keep.view(2, 65), torch.full_like(keep.view(2, 65), -1))]

    exact_then_roomy(run, _lib.lib().pnx_nms_workspace_bytes(130, 2, 65))


def test_bf16_wgrad_in_exactly_its_workspace(monkeypatch):
    from pillarnext_amd import _lib, ops
    from test_gpu_masked_conv_train import _lidar_mask

    gen = torch.Generator(device="cuda").manual_seed(64 * 3 + 64 + 8)
    m = _lidar_mask(1, 8, 8, gen, 0.5)
    x = (torch.randn((1, 64, 8, 8), device="cuda", generator=gen) * m).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    g = torch.randn((1, 64, 8, 8), device="cuda", generator=gen).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    mu8 = (m[:, 0] != 0).to(torch.uint8).contiguous()
    assert 0 < int(mu8.sum())

    def run(ws):
        monkeypatch.setattr(ops, "_PARTIALS_WS", ws)
        dw = ops.conv3x3_wgrad(x, g, mu8, stride=1)
        assert float(dw.abs().max()) > 0
        return [dw]

    exact_then_roomy(run, _lib.lib().pnx_conv3x3_wgrad_workspace_bytes(64, 64))
