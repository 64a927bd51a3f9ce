"""CPU: the label assignment's yardstick and its host side.

tests/assign_fp64_ref.py (the fp64 numpy statement that tests/test_gpu_assign.py holds the kernels to) against the output of the reference's
own AssignLabel on the same input (tests/golden/assign_small.npz, written by tools/gen_assign_golden.py); AssignLabel's construction, the
det3d alias, the refusal of CPU tensors and the argument checks of the two entry points, none of which needs a GPU."""
import ctypes
import math
import os

import numpy as np
import pytest

import assign_fp64_ref as R
from conftest import ROOT, load_golden

KEYS = ("hm", "anno_box", "ind", "mask", "cat", "gt_boxes")


def fixture_cfg(g):
    return R.make_cfg(g["cfg_tasks_ncls"], g["cfg_pc_range"], g["cfg_voxel_size"], g["cfg_out_size_factor"], float(g["cfg_gaussian_overlap"]),
                      int(g["cfg_min_radius"]), int(g["cfg_max_objs"]))


def test_twin_equals_the_reference_output():
    g = load_golden("assign_small")
    cfg = fixture_cfg(g)
    assert cfg["hw"] == [(80, 96), (40, 48), (40, 48)]
    o = R.assign(g["in_boxes"][None], g["in_classes"][None], cfg)
    margin = math.ceil(float(g["ref_ulp"]))  # the reference takes log / sin / cos in fp32: its own distance from the fp64 truth, not the twin's
    assert 1 <= margin <= 4, float(g["ref_ulp"])
    kept = 0
    for t in range(3):
        for k in ("hm", "ind", "mask", "cat", "gt_boxes"):
            want = g[f"t{t}_{k}"]
            assert o[k][t][0].dtype == want.dtype and np.array_equal(o[k][t][0], want), (t, k)
        a, want = o["anno_box"][t][0], g[f"t{t}_anno_box"]
        assert np.array_equal(a[:, [0, 1, 2, 6, 7]], want[:, [0, 1, 2, 6, 7]]), t
        d = R.ulp_distance(want[:, [3, 4, 5, 8, 9]], o["anno64"][t][0][:, [3, 4, 5, 8, 9]])
        print(f"task {t}: reference log/sin/cos within {d.max():.2f} fp32 ulp of the twin's fp64 values (margin {margin})")
        assert d.max() <= margin, (t, d.max())
        assert int(o["counts"][0, t]) == int(want.any(axis=1).sum()) == int(g[f"t{t}_mask"].sum())
        kept += int(o["counts"][0, t])
    # the planted cases are in the fixture: a centre in (-1, 0) cells kept with a negative offset on both strides, the last cell, a shared centre
    assert kept == 71 and sum(int((g[f"t{t}_hm"] == 1.0).sum()) for t in range(3)) == 69
    assert g["t0_anno_box"][:, 0].min() == -0.75 and (g["t1_anno_box"][:, 1] < 0).any()
    assert (g["t2_ind"] == 39 * 48 + 47).any() and not (g["t2_ind"] >= 40 * 48).any()


def test_twin_overflow_rule():
    """More survivors than max_objs: the first max_objs in input order stay, the rest leave the lists AND the heat map; counts keeps the number."""
    cfg = R.make_cfg([1], [0, 0, -1, 8, 8, 1], [0.5, 0.5, 2], [1], 0.1, 2, 3)
    b = np.zeros((1, 5, 9), np.float32)
    b[0, :, 0] = [0.7, 2.2, 3.7, 5.2, 6.7]
    b[0, :, 1] = 4.2
    b[0, :, 3:6] = 1.0
    o = R.assign(b, np.zeros((1, 5), np.int32), cfg)
    assert int(o["counts"][0, 0]) == 5 and o["mask"][0][0].tolist() == [1, 1, 1]
    assert o["ind"][0][0].tolist() == [8 * 16 + 1, 8 * 16 + 4, 8 * 16 + 7]
    assert o["hm"][0][0, 0, 8, 7] == 1.0 and (o["hm"][0][0, 0, :, 10:] == 0).all()


def test_assign_label_construction_and_alias():
    from pillarnext_amd import config as C
    from pillarnext_amd.assign import AssignLabel

    y = C.load(os.path.join(ROOT, "configs", "pillarnext_b_nusc.yaml"))
    head = y["model"]["head"]
    node = {"_target_": "det3d.datasets.pipelines.assign.AssignLabel", "gaussian_overlap": 0.1, "max_objs": 500, "min_radius": 2,
            "tasks": head["tasks"], "pc_range": head["pc_range"], "voxel_size": head["voxel_size"], "out_size_factor": head["out_size_factor"]}
    a = C.instantiate(node)
    assert type(a) is AssignLabel
    assert a.grid.tolist()[:2] == [1344, 1344] and a.map_size == [(336, 336)] * 6
    assert a.class_table == [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (4, 0), (4, 1), (5, 0), (5, 1)]
    idx = a.class_index(["car", "traffic_cone", "animal", "trailer"])
    assert idx.dtype == np.int32 and idx.tolist() == [0, 9, -1, 4]
    d = a.descriptor()
    assert (d.n_tasks, d.n_classes, d.max_objs, d.min_radius) == (6, 10, 500, 2)
    assert d.voxel[0] == 0.075 and d.lo[0] == -50.4 and d.overlap == 0.1          # the config's doubles, not fp32 casts
    assert list(d.h)[:6] == [336] * 6 and list(d.ncls)[:6] == [1, 2, 2, 1, 2, 2] and list(d.class_task)[:10] == [0, 1, 1, 2, 2, 3, 4, 4, 5, 5]
    # per-task strides and a non-square range
    b = AssignLabel([["a"], ["b", "c"], ["d", "e"]], 0.1, 64, 2, [-9.6, -8, -5, 9.6, 8, 3], [0.1, 0.1, 8], [2, 4, 4])
    assert b.map_size == [(80, 96), (40, 48), (40, 48)]
    import det3d.datasets.pipelines.assign as alias

    assert alias.AssignLabel is AssignLabel


def test_cpu_tensors_are_refused():
    torch = pytest.importorskip("torch")
    from pillarnext_amd import ops
    from pillarnext_amd._lib import PnxError
    from pillarnext_amd.assign import AssignLabel

    a = AssignLabel([["a"]], 0.1, 8, 2, [0, 0, -1, 8, 8, 1], [0.5, 0.5, 2], [1])
    boxes, cls = torch.zeros((1, 4, 9)), torch.zeros((1, 4), dtype=torch.int32)
    with pytest.raises(PnxError, match="CUDA"):
        a.assign(boxes, cls)
    out = {"hm": [torch.zeros((1, 1, 16, 16))], "anno_box": [torch.zeros((1, 8, 10))], "ind": [torch.zeros((1, 8), dtype=torch.int64)],
           "mask": [torch.zeros((1, 8), dtype=torch.uint8)], "cat": [torch.zeros((1, 8), dtype=torch.int64)], "gt_boxes": [torch.zeros((1, 8, 7))]}
    with pytest.raises(PnxError, match="CUDA"):
        ops.assign_labels(boxes, cls, None, a.descriptor(), out, torch.zeros((1, 1), dtype=torch.int32), torch.zeros(4096, dtype=torch.uint8))


def test_entry_points_validate_before_any_hip_call():
    from pillarnext_amd import _lib
    from pillarnext_amd.assign import AssignLabel

    L = _lib.lib()
    assert L.pnx_assign_workspace_bytes(4, 6, 500) >= 4 * 6 * 500 * 16 + 4 * 6 * 4
    assert L.pnx_assign_workspace_bytes(0, 6, 500) == 0 and L.pnx_assign_workspace_bytes(4, 0, 500) == 0 and L.pnx_assign_workspace_bytes(4, 6, 0) == 0
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    arr = (ctypes.c_void_p * 8)(*([p.value] * 8))
    good = AssignLabel([["a"], ["b", "c"]], 0.1, 8, 2, [0, 0, -1, 8, 8, 1], [0.5, 0.5, 2], [1, 2])

    def call(desc=None, boxes=p, outs=None, ws_bytes=1 << 20, hm=arr, counts=p, k=4):
        d = desc if desc is not None else good.descriptor()
        o = outs if outs is not None else [hm, arr, arr, arr, arr, arr]
        rc = L.pnx_assign_labels(boxes, p, None, 1, k, ctypes.byref(d), *o, counts, p, ws_bytes, None)
        return rc, L.pnx_last_error()

    rc, msg = call(boxes=None)
    assert rc == -1 and b"null pointer" in msg
    rc, msg = call(counts=None)
    assert rc == -1 and b"null pointer" in msg
    rc, msg = call(outs=[arr, arr, None, arr, arr, arr])
    assert rc == -1 and b"null pointer" in msg
    holes = (ctypes.c_void_p * 8)(p.value, None, *([p.value] * 6))
    rc, msg = call(hm=holes)
    assert rc == -1 and b"null pointer" in msg and b"task 1" in msg
    rc = L.pnx_assign_labels(p, p, None, 1, 4, None, arr, arr, arr, arr, arr, arr, p, p, 1 << 20, None)
    assert rc == -1 and b"null pointer" in L.pnx_last_error()
    d = good.descriptor()
    d.max_objs = 0
    rc, msg = call(desc=d)
    assert rc < 0 and b"max_objs" in msg
    d = good.descriptor()
    d.n_tasks = 0
    rc, msg = call(desc=d)
    assert rc < 0 and b"n_tasks" in msg
    d = good.descriptor()
    d.h[1], d.w[1] = 65536, 32768                                    # 2^31 cells
    rc, msg = call(desc=d)
    assert rc < 0 and b"overflows int32" in msg
    rc, msg = call(ws_bytes=L.pnx_assign_workspace_bytes(1, 2, 8) - 1)
    assert rc == -3 and b"workspace too small" in msg
    d = good.descriptor()
    d.class_task[2] = 5
    rc, msg = call(desc=d)
    assert rc < 0 and b"class 2" in msg
