"""CPU: every workspace layout of csrc/ is stated once (a *_carve function on PnxCarver), and one check stands in front of it.

1. Sizes: every pnx_*_workspace_bytes answers, argument tuple by argument tuple, what it answered before the hand-written sums of aligned terms
   were folded into the carves.  tests/golden/workspace_bytes.json was written at the commit named in its "commit" field, before any edit, by this
   module's own helper, from the repository root:

       import json, sys
       sys.path.insert(0, "tests")
       import test_workspace_layout_cpu as t
       json.dump({"commit": "<git rev-parse HEAD>", "bytes": t.workspace_bytes_table()}, open(t.GOLDEN, "w"), indent=0)

   No row is known-different: formula and carve agreed for every tuple below.
2. One check, one wording (pnx_check_workspace of csrc/pnx_common.h): null -> PNX_ERR_INVALID; short -> PNX_ERR_WORKSPACE with the entry's name, both
   byte counts and "workspace too small"; a base that is not 256-byte aligned -> PNX_ERR_INVALID with "256-byte aligned".  Every entry here is
   called with host memory only: its checks come before any HIP call."""
import ctypes
import json
import os


HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "workspace_bytes.json")

COUNTS = [0, 1, 2047, 2048, 2049, 300000]                 # around PNX_SCAN_ITEMS = 2048 (= kChunk of augment.hip)
RS_CHUNK = 16384                                          # kRsChunk of decode.hip
KEYS = COUNTS + [RS_CHUNK - 1, RS_CHUNK, RS_CHUNK + 1]
BATCHES, SEGMENTS = [1, 4, 12], [1, 6, 72]
GEOMS = {"nusc": ([-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], [0.075, 0.075, 8.0]), "small": ([0.0, 0.0, -1.0, 8.0, 8.0, 1.0], [0.5, 0.5, 2.0])}
GROUP_GEOMS = {"voxel": ([-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], [0.3, 0.3, 0.2], 0), "pillar": ([-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], [0.3, 0.3, 8.0], 1)}
PNX_ERR_INVALID, PNX_ERR_WORKSPACE = -1, -3


def _lib():
    from pillarnext_amd import _lib

    return _lib, _lib.lib()


def workspace_bytes_table():
    """{function: [[args, bytes], ..]} at the seams of the formulas.  A geometry is named by its key in GEOMS / GROUP_GEOMS; the last argument of an
    NMS row is the pair capacity set with pnx_debug_nms_pair_cap while the row is read (0 = the default)."""
    from pillarnext_amd import ops

    _l, L = _lib()
    geoms = {k: _l.make_geom(*v) for k, v in GEOMS.items()}
    ggeoms = {k: ops.group_geom(v[0], v[1], v[2]) for k, v in GROUP_GEOMS.items()}
    t = {}

    def rows(name, tuples, call=None):
        fn = getattr(L, name)
        t[name] = [[list(a), int(call(fn, *a) if call else fn(*a))] for a in tuples]

    rows("pnx_reader_workspace_bytes", [(n, b, g) for n in COUNTS for b in BATCHES for g in GEOMS],
         lambda fn, n, b, g: fn(n, b, ctypes.byref(geoms[g])))
    rows("pnx_group_workspace_bytes", [(n, s, b, g) for n in COUNTS for s in (4, 6) for b in BATCHES for g in GROUP_GEOMS],
         lambda fn, n, s, b, g: fn(n, s, b, ctypes.byref(ggeoms[g])))
    rows("pnx_bilinear_gather_backward_workspace_bytes", [(n, b, h, w) for n in COUNTS for b in BATCHES for h, w in ((8, 8), (180, 180))])
    rows("pnx_scatter_max_workspace_bytes", [(n, p) for n in COUNTS for p in COUNTS] + [(-1, 1)])
    rows("pnx_point_layer_workspace_bytes", [(n, ci, co, bw) for n in COUNTS for ci, co in ((10, 64), (64, 64), (576, 256), (577, 64)) for bw in (0, 1)])
    rows("pnx_merge_sweeps_workspace_bytes", [(n,) for n in COUNTS + [-1]])
    rows("pnx_conv3x3_wgrad_workspace_bytes", [(64, 64), (256, 256), (512, 512), (64, 128), (384, 128), (48, 64)])
    rows("pnx_conv3x3_smallk_wgrad_workspace_bytes", [(k,) for k in range(0, 6)])
    rows("pnx_decode_topk_workspace_bytes", [(n, s) for n in KEYS for s in SEGMENTS] + [(-1, 1), (1, 0)])
    rows("pnx_sort_keys_workspace_bytes", [(n,) for n in KEYS])
    rows("pnx_center_loss_workspace_bytes", [(b, m) for b in BATCHES + [0] for m in (0, 1, 500)])
    rows("pnx_assign_workspace_bytes", [(b, nt, m) for b in BATCHES + [0] for nt in (1, 6) for m in (1, 500)])
    rows("pnx_paste_augment_workspace_bytes", [(n, b) for n in COUNTS + [-1] for b in BATCHES + [0]])
    rows("pnx_sp3_wgrad_workspace_bytes", [(n, tp, ci, co) for n in COUNTS for tp in (1, 27) for ci, co in ((16, 16), (64, 128), (144, 144), (145, 16))])
    nms = []
    for cap in (0, 64):
        prev = L.pnx_debug_nms_pair_cap(cap)
        try:
            for total in (0, 1, 65, 4096):
                for s in SEGMENTS + [0]:
                    for msl in (0, 1, 64, 65, 4096):
                        nms.append([[total, s, msl, cap], int(L.pnx_nms_workspace_bytes(total, s, msl))])
        finally:
            L.pnx_debug_nms_pair_cap(prev)
    t["pnx_nms_workspace_bytes"] = nms
    return t


def test_every_workspace_size_is_the_parents():
    from pillarnext_amd import _lib

    with open(GOLDEN) as f:
        golden = json.load(f)
    assert len(golden["commit"]) == 40
    want, got = golden["bytes"], workspace_bytes_table()
    declared = sorted(n for n in _lib.PROTOTYPES if n.endswith("_workspace_bytes"))
    assert sorted(want) == sorted(got) == declared
    for name in declared:
        assert len(got[name]) == len(want[name]) > 0
        for g, w in zip(got[name], want[name]):
            assert g == w, (name, g, w)
    assert any(b > 0 for _, b in want["pnx_nms_workspace_bytes"]) and want["pnx_nms_workspace_bytes"][-1][0][3] == 64


# ------------------------------------------------------------------------------------------------------ 2: one check, one wording
def _entries():
    """(entry name, need, call(workspace, workspace_bytes) -> rc): every other argument is satisfied from host memory."""
    from pillarnext_amd.assign import AssignLabel

    _l, L = _lib()
    buf = (ctypes.c_char * (1 << 16))()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)
    arr = (ctypes.c_void_p * 8)(*([p.value] * 8))
    desc = AssignLabel([["a"], ["b", "c"]], 0.1, 8, 2, [0, 0, -1, 8, 8, 1], [0.5, 0.5, 2], [1, 2]).descriptor()
    wg = int(L.pnx_conv3x3_wgrad_workspace_bytes(64, 64))
    loss = int(L.pnx_center_loss_workspace_bytes(2, 8))
    nms = (p, p, p, 2, 65, p, 10, p, p)
    out = [
        ("pnx_merge_sweeps", L.pnx_merge_sweeps_workspace_bytes(2049), lambda w, n: L.pnx_merge_sweeps(p, 2049, 5, 4, p, 2, p, p, w, n, None)),
        ("pnx_decode_topk", L.pnx_decode_topk_workspace_bytes(RS_CHUNK + 1, 2),
         lambda w, n: L.pnx_decode_topk(p, RS_CHUNK + 1, 2, 8, p, p, p, p, p, w, n, None)),
        ("pnx_sort_keys", L.pnx_sort_keys_workspace_bytes(1000), lambda w, n: L.pnx_sort_keys(p, 1000, 4, p, p, w, n, None)),
        ("pnx_center_loss_forward", loss, lambda w, n: L.pnx_center_loss_forward(arr, p, p, p, p, p, p, 2, 2, 8, 8, 8, p, 1, p, w, n, None)),
        ("pnx_center_loss_backward", loss,
         lambda w, n: L.pnx_center_loss_backward(arr, arr, p, p, p, p, p, p, 2, 2, 8, 8, 8, p, 1, p, p, p, w, n, None)),
        ("pnx_assign_labels", L.pnx_assign_workspace_bytes(1, 2, 8),
         lambda w, n: L.pnx_assign_labels(p, p, None, 1, 4, ctypes.byref(desc), arr, arr, arr, arr, arr, arr, p, w, n, None)),
        ("pnx_paste_augment_points", L.pnx_paste_augment_workspace_bytes(2049, 2),
         lambda w, n: L.pnx_paste_augment_points(p, 2049, 5, 2, None, None, None, None, 0, 7, None, None, 0, 0, None, p, 4096, p, p, w, n, None)),
        ("pnx_conv3x3_wgrad_bf16", wg, lambda w, n: L.pnx_conv3x3_wgrad_bf16(p, p, p, p, 1, 8, 8, 64, 64, 1, w, n, None)),
        ("pnx_conv3x3_wgrad_x3", wg, lambda w, n: L.pnx_conv3x3_wgrad_x3(p, p, p, p, p, p, 1, 8, 8, 64, 64, 1, w, n, None)),
        ("pnx_conv3x3_wgrad_x6", wg, lambda w, n: L.pnx_conv3x3_wgrad_x6(p, p, p, p, p, p, p, p, 1, 8, 8, 64, 64, 1, w, n, None)),
        ("pnx_conv3x3_smallk_wgrad", L.pnx_conv3x3_smallk_wgrad_workspace_bytes(3),
         lambda w, n: L.pnx_conv3x3_smallk_wgrad(p, p, p, p, 1, 8, 8, 64, 3, 0, w, n, None)),
        ("pnx_nms_rotated_batched", L.pnx_nms_workspace_bytes(1, 2, 65), lambda w, n: L.pnx_nms_rotated_batched(*nms, w, n, None)),
        ("pnx_nms_normal_batched", 8, lambda w, n: L.pnx_nms_normal_batched(*nms, w, n, None)),   # one mask word: all the host can check
        ("pnx_scatter_max", L.pnx_scatter_max_workspace_bytes(100, 10), lambda w, n: L.pnx_scatter_max(p, p, 100, 64, 10, p, p, w, n, None)),
        ("pnx_sp3_wgrad", L.pnx_sp3_wgrad_workspace_bytes(100, 27, 16, 16), lambda w, n: L.pnx_sp3_wgrad(p, 100, 16, p, 16, p, 100, 27, p, w, n, None)),
        ("pnx_point_layer_stats", L.pnx_point_layer_workspace_bytes(10, 20, 24, 0), lambda w, n: L.pnx_point_layer_stats(p, 20, 10, 20, p, 24, p, w, n, None)),
    ]
    return L, p, buf, [(name, int(need), call) for name, need, call in out]


def test_one_workspace_check_one_wording():
    L, p, _keep, entries = _entries()
    assert len(entries) == 16
    for name, need, call in entries:
        assert need >= 8, name
        rc = call(p, need - 1)
        err = L.pnx_last_error().decode()
        assert rc == PNX_ERR_WORKSPACE and name in err and "workspace too small" in err and str(need - 1) in err and str(need) in err, (name, rc, err)
        rc = call(ctypes.c_void_p(p.value + 8), need)
        err = L.pnx_last_error().decode()
        assert rc == PNX_ERR_INVALID and "256-byte aligned" in err, (name, rc, err)
        assert call(None, need) == PNX_ERR_INVALID, name
