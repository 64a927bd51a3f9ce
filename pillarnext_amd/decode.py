"""Fused CenterHead.predict for packed head outputs (host side of csrc/decode.hip).

Semantics = det3d/models/heads/centerhead.py:231-384 (decode, score/range mask, IoU-rectified score, per-class
sort + top pre_max, rotated NMS, top post_max, task merge with label offsets), restructured so that the whole frame
batch needs one key kernel per task, ONE device sort, one box kernel, ONE batched NMS and ONE device->host copy."""
import collections
import ctypes
import struct
import weakref

import torch

from . import ops
from ._lib import PnxError, check, lib, ptr, stream_ptr
from .switches import on

_SIGN = -0x8000000000000000   # keys are unsigned: as int64 they sort (and search) as unsigned with the sign bit flipped


def _get(cfg, name):
    return cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)


def pack_task(C, has_iou, ncls, cls_off, H, W, osf, vs, pc_range, score_thr, lim, rect, lazy=False):
    """Host descriptor matching `struct DecodeTask` in csrc/decode.hip.  lazy: the packed tensor is [iou] hm only."""
    lim6 = [float(v) for v in lim] if len(lim) > 0 else [0.0] * 6
    r4 = [float(v) for v in rect] + [0.0] * (4 - len(rect))
    o_iou = 0 if lazy else 10
    o_hm = (1 if has_iou else 0) if lazy else 10 + int(bool(has_iou))
    blob = struct.pack("6i6f6fi4f3i", int(C), int(bool(has_iou)), int(ncls), int(cls_off), int(H), int(W),
                       float(osf), float(vs[0]), float(vs[1]), float(pc_range[0]), float(pc_range[1]), float(score_thr),
                       *lim6, int(len(lim) > 0), *r4, int(o_hm), int(o_iou), int(bool(lazy)))
    assert len(blob) == lib().pnx_decode_task_desc_bytes(), "DecodeTask layout drifted"
    return blob


class _PnxLazyDecode(ctypes.Structure):
    """include/pnx.h: pnx_lazy_decode."""
    _fields_ = ([(n, ctypes.c_int32) for n in ("n_tasks", "n_classes_total", "batch", "pre_max", "post_max", "dtype")]
                + [(n, ctypes.c_void_p) for n in ("dense_host", "task_descs_host", "task_descs_dev", "task_key_off_host", "task_key_off_dev",
                                                 "list_key_off_dev", "lazy_tasks_host", "class_task_host", "seg_off_dev", "nms_thresh_dev", "keys",
                                                 "sorted_keys", "order", "seg_start", "local", "seg_len", "seg_total", "cand", "boxes9", "boxes7",
                                                 "scores", "flag", "keep", "keep_count", "topk_ws")]
                + [("topk_ws_bytes", ctypes.c_size_t), ("nms_ws", ctypes.c_void_p), ("nms_ws_bytes", ctypes.c_size_t)]
                + [(n, ctypes.c_void_p) for n in ("out", "out_host", "keep_count_host", "flag_host")])


# What a launch needs to know about one (lazy or dense, batch, map shapes, channel counts): lists s = sample * nc_total + class, S of them.
# HostLayout (PackedDecoder.host_layout, no GPU): descs = the tasks' DecodeTask blobs, offs = cumulative key offsets of the tasks (T + 1),
# kofs[s] = key offset of the task that owns list s, segs[t] = the lists of task t.  Layout adds the device constants: kofs and segs as
# tensors, tdesc / koff = descs / offs, seg_off = s * pre_max, thr = NMS threshold per list, bounds = first possible key of every list
# (sign-flipped, for searchsorted), jj = arange(pre_max).
HostLayout = collections.namedtuple("HostLayout", "descs offs S kofs segs")
Layout = collections.namedtuple("Layout", "host tdesc koff kofs segs seg_off thr bounds jj")


class PackedDecoder:
    def __init__(self, num_classes, rectifier, test_cfg, has_iou, channels_per_task):
        self.num_classes = list(num_classes)
        self.nc_total = sum(num_classes)
        self.class_task = [t for t, n in enumerate(self.num_classes) for _ in range(n)]   # the task that owns every class
        self.rectifier = rectifier
        self.has_iou = has_iou
        self.channels = list(channels_per_task)
        nms = _get(test_cfg, "nms")
        self.pre_max = int(_get(nms, "nms_pre_max_size"))
        self.post_max = int(_get(nms, "nms_post_max_size"))
        self.thr = [float(v) for t in _get(nms, "nms_iou_threshold") for v in t]
        self.cfg = test_cfg
        # PNX_DECODE_TOPK=1 (default): exact radix-select top-k in HIP (pnx_decode_topk: most significant digit first over the composite
        # (score key, key index), lists that hold fewer than pre_max valid keys finish after the first pass) -- exactly the selection of
        # a stable sort + cut (tests/test_gpu_decode.py::test_segmented_topk_equals_the_full_stable_sort).  PNX_DECODE_TOPK=0 selects the
        # bit-ranged stable key sort of all keys (pnx_sort_keys), PNX_DECODE_TORCH_SORT=1 the generic 64-bit torch.sort (cross-checks).
        if on("PNX_DECODE_TOPK") and self.pre_max <= 4096:
            self.selection = "topk"
        else:
            self.selection = "torchsort" if on("PNX_DECODE_TORCH_SORT") else "keysort"
        self._dev = {}   # Layout per (kind, batch, element dtype, (C, H, W) per task, device); launch_lazy_fused's scratch under ("lazy_fused", ...)
        self._topk_ws, self._keysort_ws = ops.Workspace(), ops.Workspace()    # selection scratch
        self._tptr = {}
        self._pin = {}

    use_topk = property(lambda self: self.selection == "topk")
    use_torch_sort = property(lambda self: self.selection == "torchsort")

    def host_layout(self, lazy, B, shapes, channels):
        """HostLayout of T tasks with (H, W) = shapes[t] and channels[t] channels per map, B samples.  Plain Python: needs no GPU."""
        cfg, descs, offs = self.cfg, [], [0]
        for t, (H, W) in enumerate(shapes):
            descs.append(pack_task(channels[t], self.has_iou, self.num_classes[t], sum(self.num_classes[:t]), H, W, _get(cfg, "out_size_factor")[t],
                                   _get(cfg, "voxel_size"), _get(cfg, "pc_range"), _get(cfg, "score_threshold"),
                                   _get(cfg, "post_center_limit_range"), self.rectifier[t], lazy=lazy))
            offs.append(offs[-1] + B * H * W)
        S = B * self.nc_total
        owner = [self.class_task[s % self.nc_total] for s in range(S)]
        return HostLayout(descs, offs, S, [offs[t] for t in owner], [[s for s in range(S) if owner[s] == t] for t in range(len(shapes))])

    def _layout(self, lazy, maps):
        """The cached Layout of a launch's maps (list, one per task, of (B, C_t, H, W) tensors of one dtype)."""
        B, dev = maps[0].shape[0], maps[0].device
        chw = tuple(tuple(p.shape[1:]) for p in maps)
        ck = ("lazy" if lazy else "dense", B, maps[0].dtype, chw, dev)
        lay = self._dev.get(ck)
        if lay is None:
            h = self.host_layout(lazy, B, [s[1:] for s in chw], [s[0] for s in chw] if lazy else self.channels)
            i64 = dict(dtype=torch.int64, device=dev)
            lay = self._dev[ck] = Layout(
                host=h, tdesc=torch.frombuffer(bytearray(b"".join(h.descs)), dtype=torch.uint8).to(dev), koff=torch.tensor(h.offs, **i64),
                kofs=torch.tensor(h.kofs, **i64), segs=[torch.tensor(rows, **i64) for rows in h.segs],
                seg_off=(torch.arange(h.S + 1, dtype=torch.int32, device=dev) * self.pre_max).contiguous(),
                thr=torch.tensor(self.thr, dtype=torch.float32, device=dev).repeat(B),
                bounds=(torch.arange(h.S + 1, **i64) << 32) ^ _SIGN, jj=torch.arange(self.pre_max, **i64))
        return lay

    def _keys(self, maps, lay):
        """One 64-bit key per cell of every task's map (pnx_decode_keys), concatenated in task order."""
        h, B, dt = lay.host, maps[0].shape[0], ops._DT[maps[0].dtype]
        keys = torch.empty((h.offs[-1],), dtype=torch.int64, device=maps[0].device)
        for t, p in enumerate(maps):
            assert p.is_contiguous(memory_format=torch.channels_last), "head outputs must be channels_last"
            kp = ctypes.c_void_p(keys.data_ptr() + 8 * h.offs[t])
            check(lib().pnx_decode_keys(ptr(p), dt, B, self.nc_total, h.descs[t], kp, stream_ptr()), "pnx_decode_keys")
        return keys

    def _select(self, keys, lay):
        """The first pre_max keys of every list in stable ascending order, by self.selection.  -> skeys, order (source index of every sorted
        key; candidate j of list s at seg_start[s] + j), seg_start, seg_len (S,) int32 <= pre_max, seg_total (S,) int32 = valid keys of the list."""
        L, S, n, dev = lib(), lay.host.S, keys.numel(), keys.device
        if self.selection == "topk":
            # segmented top-k in HIP (csrc/decode.hip): exact radix select on (score key, key index) -> collect -> LDS sort of the <= pre_max
            # survivors of every list; no device sort of all keys, no searchsorted
            skeys = torch.empty((S * self.pre_max,), dtype=torch.int64, device=dev)
            order = torch.zeros((S * self.pre_max,), dtype=torch.int64, device=dev)    # slots behind seg_len are read (and ignored) by launch_lazy's glue
            seg_start = torch.empty((S,), dtype=torch.int64, device=dev)
            seg_len = torch.empty((S,), dtype=torch.int32, device=dev)
            seg_total = torch.empty((S,), dtype=torch.int32, device=dev)
            ws = self._topk_ws.get(int(L.pnx_decode_topk_workspace_bytes(n, S)), dev)
            check(L.pnx_decode_topk(ptr(keys), n, S, self.pre_max, ptr(skeys), ptr(order), ptr(seg_start), ptr(seg_len), ptr(seg_total), ptr(ws),
                                    ws.numel(), stream_ptr()), "pnx_decode_topk")
            return skeys, order, seg_start, seg_len, seg_total
        if self.selection == "torchsort":
            skeys, order = torch.sort(keys ^ _SIGN, stable=True)
            skeys = skeys ^ _SIGN
        else:
            # the same stable sort over the 32 + bit_length(S) bits that can differ (pnx_sort_keys: 5 radix passes instead of 8)
            skeys, order = torch.empty_like(keys), torch.empty_like(keys)
            ws = self._keysort_ws.get(int(L.pnx_sort_keys_workspace_bytes(n)), dev)
            check(L.pnx_sort_keys(ptr(keys), n, S, ptr(skeys), ptr(order), ptr(ws), ws.numel(), stream_ptr()), "pnx_sort_keys")
        seg_start = torch.searchsorted(skeys ^ _SIGN, lay.bounds)
        seg_total = (seg_start[1:] - seg_start[:-1]).to(torch.int32)
        return skeys, order, seg_start[:S], torch.clamp(seg_total, max=self.pre_max), seg_total

    def _box_buffers(self, S, dev):
        n_rows = S * self.pre_max
        return (torch.empty((n_rows, 9), dtype=torch.float32, device=dev), torch.zeros((n_rows, 7), dtype=torch.float32, device=dev),
                torch.empty((n_rows,), dtype=torch.float32, device=dev))

    @torch.no_grad()
    def launch(self, packed, tokens=None):
        """packed: list (one per task) of (B, C_t, H, W) channels_last tensors, fp32 or bf16 (all the same dtype).
        Enqueues decode + NMS + the D2H copy and returns a PendingDetections."""
        B, T, dev = packed[0].shape[0], len(packed), packed[0].device
        lay = self._layout(False, packed)
        S = lay.host.S
        skeys, order, seg_start, seg_len, _ = self._select(self._keys(packed, lay), lay)
        # pointer table of the task tensors: a torch.tensor(list, device=...) is a blocking copy from pageable memory (it would make
        # the host wait for the whole network before it could enqueue the sort/NMS); cached per pointer tuple, else a pinned async copy
        pk = tuple(p.data_ptr() for p in packed)
        tptr = self._tptr.get(pk)
        if tptr is None:
            hp = torch.tensor(pk, dtype=torch.int64).pin_memory()
            tptr = torch.empty((T,), dtype=torch.int64, device=dev)
            tptr.copy_(hp, non_blocking=True)
            if len(self._tptr) > 64:
                self._tptr.clear()
            self._tptr[pk] = tptr
            self._tptr_host = hp  # keep the pinned source alive until the copy ran
        boxes9, boxes7, scores = self._box_buffers(S, dev)
        check(lib().pnx_decode_boxes(ptr(tptr), ptr(lay.tdesc), ptr(lay.koff), T, ops._DT[packed[0].dtype], B, ptr(skeys), ptr(order), ptr(seg_start),
                                     ptr(seg_len), S, self.pre_max, ptr(boxes9), ptr(boxes7), ptr(scores), stream_ptr()), "pnx_decode_boxes")
        return self._finish(lay, boxes9, boxes7, scores, seg_len, B, tokens)

    def _finish(self, lay, boxes9, boxes7, scores, seg_len, B, tokens, flag=None, fallback=None):
        S, dev = lay.host.S, boxes9.device
        keep, cnt = ops.nms_batched(boxes7, lay.seg_off, lay.thr, self.pre_max, post_max=self.post_max, seg_len=seg_len)
        out = torch.empty((S, self.post_max, 10), dtype=torch.float32, device=dev)
        check(lib().pnx_gather_kept(ptr(boxes9), ptr(scores), ptr(keep), ptr(cnt), S, self.pre_max, self.post_max, ptr(out), stream_ptr()),
              "pnx_gather_kept")
        # the one device->host hand-off of the frame batch: asynchronous into pinned memory; PendingDetections.result() waits
        slot = self._pinned_slot(out.shape, S, out.dtype, cnt.dtype, flag=flag is not None)
        slot["out"].copy_(out, non_blocking=True)
        slot["cnt"].copy_(cnt[:S], non_blocking=True)
        if flag is not None:  # lazy head: the range-test flag rides on the same stream; result() falls back to the dense path if it is set
            slot["flag"].copy_(flag, non_blocking=True)
        return self._hand_off(slot, B, tokens, flag is not None, fallback)

    def _hand_off(self, slot, B, tokens, with_flag, fallback):
        """The PendingDetections of a pinned slot whose copies are enqueued on the current stream; it owns the slot until it is resolved."""
        ev = torch.cuda.Event()
        ev.record()
        pend = PendingDetections(ev, slot["out"], slot["cnt"], B, self.nc_total, tokens if tokens else [None] * B)
        if with_flag:
            pend.flag_h, pend.fallback = slot["flag"], fallback
        slot["owner"] = weakref.ref(pend)
        return pend

    @torch.no_grad()
    def launch_lazy(self, dense, evaluator, tokens=None, fallback=None):
        """Lazy head: dense = list (one per task) of (B, 16, H, W) channels_last maps holding [iou] hm only;
        evaluator(local (S, pre_max) int64, seg_len (S,) int32, valid (S, pre_max) bool, segs = per task the rows of its lists) returns the
        (S, pre_max, 10) fp32 regression values [reg 2, height 1, dim 3, rot 2, vel 2] at the cells local = b*H*W + cell of each list's task
        (slots behind seg_len are ignored).  Same selection as launch(): scores come from the dense maps, the candidates are the
        first pre_max of every (sample, class) list; the centre range test runs on the evaluated candidates (pnx_decode_boxes_lazy) and
        `fallback()` (the dense path) is taken by result() in the one case where that could change the selection."""
        B, T, dev = dense[0].shape[0], len(dense), dense[0].device
        lay = self._layout(True, dense)
        S = lay.host.S
        skeys, order, seg_start, seg_len, seg_total = self._select(self._keys(dense, lay), lay)
        # candidate cells per slot (s, j): local index b*H*W + cell inside the slot's task; 0 behind seg_len
        valid = lay.jj[None, :] < seg_len[:, None]
        pos = torch.clamp(seg_start[:, None] + lay.jj[None, :], max=order.numel() - 1)
        local = torch.where(valid, order[pos] - lay.kofs[:, None], torch.zeros_like(lay.kofs[:, None]))
        cand = evaluator(local, seg_len, valid, lay.segs)                      # (S, pre_max, 10) fp32
        boxes9, boxes7, scores = self._box_buffers(S, dev)
        flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        check(lib().pnx_decode_boxes_lazy(ptr(lay.tdesc), ptr(lay.koff), T, self.nc_total, ptr(skeys), ptr(order), ptr(seg_start), ptr(seg_len),
                                          ptr(seg_total), S, self.pre_max, ptr(cand), ptr(boxes9), ptr(boxes7), ptr(scores), ptr(flag), stream_ptr()),
              "pnx_decode_boxes_lazy")
        return self._finish(lay, boxes9, boxes7, scores, seg_len, B, tokens, flag=flag, fallback=fallback)

    @torch.no_grad()
    def launch_lazy_fused(self, dense, lazy_tasks, class_task, tokens=None, fallback=None):
        """launch_lazy with the HIP evaluator as ONE C call (include/pnx.h: pnx_decode_lazy_enqueue): keys per task, top-k, candidate cells,
        regression branches at the candidates, boxes, batched NMS, gather and the copies into pinned memory are enqueued from C++ out of a
        descriptor that is built once per (batch, map shapes); per step only the pointers of the dense maps, of the deblocked maps and of
        the pinned result slot change.  lazy_tasks: per task (up, wfrag1, bias1, w2c, bias2) as ops.sephead_lazy takes them.
        Every scratch buffer is persistent: the calls of consecutive steps are ordered by the stream."""
        B, dev, T, dtype = dense[0].shape[0], dense[0].device, len(dense), dense[0].dtype
        S, L = B * self.nc_total, lib()
        chw = tuple(tuple(p.shape[1:]) for p in dense)
        ck = ("lazy_fused", B, dtype, chw, dev, torch.cuda.current_stream().cuda_stream)   # persistent scratch: one set per stream
        st = self._dev.get(ck)
        if st is None:
            if [int(v) for v in class_task] != self.class_task:
                raise PnxError(f"lazy decode: class_task {list(class_task)} is not the decoder's {self.class_task}")
            lay = self._layout(True, dense)
            n_keys, n_rows = lay.host.offs[-1], S * self.pre_max
            i64, i32, f32, u8 = torch.int64, torch.int32, torch.float32, torch.uint8
            # keyed by the descriptor's field names: the host tables, then the device scratch as (elements, dtype)
            bufs = {"dense_host": (ctypes.c_void_p * T)(), "task_descs_host": ctypes.create_string_buffer(b"".join(lay.host.descs)),
                    "task_key_off_host": (ctypes.c_int64 * (T + 1))(*lay.host.offs), "lazy_tasks_host": (ops._PnxLazyTask * T)(),
                    "class_task_host": (ctypes.c_int32 * self.nc_total)(*self.class_task)}
            scratch = {"keys": (n_keys, i64), "sorted_keys": (n_rows, i64), "order": (n_rows, i64), "seg_start": (S, i64), "local": (n_rows, i64),
                       "seg_len": (S, i32), "seg_total": (S, i32), "cand": (n_rows * 10, f32), "boxes9": (n_rows * 9, f32), "boxes7": (n_rows * 7, f32),
                       "scores": (n_rows, f32), "flag": (1, i32), "keep": (n_rows, i32), "keep_count": (S, i32), "out": (S * self.post_max * 10, f32),
                       "topk_ws": (int(L.pnx_decode_topk_workspace_bytes(n_keys, S)), u8),
                       "nms_ws": (max(int(L.pnx_nms_workspace_bytes(n_rows, S, self.pre_max)), 1), u8)}
            d = _PnxLazyDecode()
            d.n_tasks, d.n_classes_total, d.batch, d.pre_max, d.post_max, d.dtype = T, self.nc_total, B, self.pre_max, self.post_max, ops._DT[dtype]
            for f in list(bufs):
                setattr(d, f, ctypes.cast(bufs[f], ctypes.c_void_p))
            for f, (n, dt) in scratch.items():
                bufs[f] = torch.empty((n,), dtype=dt, device=dev)
                setattr(d, f, bufs[f].data_ptr())
            for f, t in (("task_descs_dev", lay.tdesc), ("task_key_off_dev", lay.koff), ("list_key_off_dev", lay.kofs), ("seg_off_dev", lay.seg_off),
                         ("nms_thresh_dev", lay.thr)):
                setattr(d, f, t.data_ptr())
            d.topk_ws_bytes, d.nms_ws_bytes = bufs["topk_ws"].numel(), bufs["nms_ws"].numel()
            st = self._dev[ck] = (d, bufs, [s[1:] for s in chw])
        d, bufs, hw = st
        for t, p in enumerate(dense):
            if not (p.dtype == dtype and p.is_contiguous(memory_format=torch.channels_last)):
                raise PnxError("lazy decode: the dense [iou] hm maps must be channels_last bf16 / fp16, one dtype")
            bufs["dense_host"][t] = p.data_ptr()
        ops.lazy_task_table(lazy_tasks, B, dtype, hw, bufs["lazy_tasks_host"])
        slot = self._pinned_slot((S, self.post_max, 10), S, torch.float32, torch.int32, flag=True)
        d.out_host, d.keep_count_host, d.flag_host = slot["out"].data_ptr(), slot["cnt"].data_ptr(), slot["flag"].data_ptr()
        check(L.pnx_decode_lazy_enqueue(ctypes.byref(d), stream_ptr()), "pnx_decode_lazy_enqueue")
        return self._hand_off(slot, B, tokens, True, fallback)

    def _pinned_slot(self, out_shape, S, out_dtype, cnt_dtype, flag=False):
        """One of the rotating pinned result buffers of a shape (a serving loop has at most two batches in flight: bench.py / forward_async);
        a slot is only reused once the PendingDetections that owns it was resolved (result()); otherwise the ring grows."""
        ring = self._pin.setdefault((tuple(out_shape), S), [])
        slot = next((sl for sl in ring if sl["owner"] is None or sl["owner"]() is None or sl["owner"]().done), None)
        if slot is None:
            slot = {"out": torch.empty(out_shape, dtype=out_dtype, pin_memory=True), "cnt": torch.empty((S,), dtype=cnt_dtype, pin_memory=True),
                    "owner": None}
            ring.append(slot)
        if flag and "flag" not in slot:
            slot["flag"] = torch.zeros((1,), dtype=torch.int32, pin_memory=True)
        return slot

    def __call__(self, packed, tokens=None):
        return self.launch(packed, tokens).result()


class PendingDetections:
    """Detections of one frame batch on their way to the host.  Splitting launch() from result() lets a serving loop enqueue
    the next batch's GPU work before it blocks on this one (the GPU never idles on the host's post-processing)."""

    def __init__(self, event, out_h, cnt_h, batch, nc_total, tokens):
        self.event, self.out_h, self.cnt_h, self.batch, self.nc_total, self.tokens = event, out_h, cnt_h, batch, nc_total, tokens
        self.done = False  # the pinned buffers may be handed to a later launch once this is True (or this object is gone)
        self._res = None
        self.flag_h, self.fallback = None, None

    def result(self):
        if self._res is not None:
            return self._res
        self.event.synchronize()
        if self.flag_h is not None and int(self.flag_h[0]) != 0:
            if self.fallback is None:
                raise PnxError("lazy head: a candidate list cut at pre_max lost a candidate to the centre range test and no dense fallback "
                               "was supplied -- the selection may differ from CenterHead.post_processing (centerhead.py:341-363)")
            # a segment cut at pre_max lost a candidate to the centre range test: the dense path decides (exact, and rare)
            fb, self.fallback = self.fallback, None
            self._res, self.done = fb().result(), True
            return self._res
        self.fallback = None   # the closure holds every task's deblocked map (~1.2 GB at C2 x 12 frames): let the allocator have them back
        out_c, cnt_c = self.out_h, self.cnt_h.tolist()
        res = []
        for b in range(self.batch):
            bb, ss, ll = [], [], []
            for c in range(self.nc_total):
                k = cnt_c[b * self.nc_total + c]
                blk = out_c[b * self.nc_total + c, :k]
                bb.append(blk[:, :9])
                ss.append(blk[:, 9])
                ll.append(torch.full((k,), c, dtype=torch.int64))
            res.append({"box3d_lidar": torch.cat(bb), "scores": torch.cat(ss), "label_preds": torch.cat(ll), "token": self.tokens[b]})
        self._res, self.done = res, True  # torch.cat made copies: the pinned slot is free again
        return res
