"""GPU: AssignLabel.assign (csrc/assign.hip behind pnx_assign_labels) against tests/assign_fp64_ref.py -- the fp64 numpy statement that
tests/test_assign_cpu.py pins to the reference's own output -- and against that output itself (tests/golden/assign_small.npz).

Bounds: integer outputs and copied values are bit-equal.  log / sin / cos and the heat map are fp64 results rounded once to fp32: at most
0.5 ulp from rounding plus the fp64 routine's error (far below 2^-29 relative), so within 1 fp32 ulp of the twin's fp64 values.  The
centre cell is exactly 1, a cell outside every window exactly 0."""
import numpy as np
import pytest

import assign_fp64_ref as R
from conftest import load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KEYS = ("hm", "anno_box", "ind", "mask", "cat", "gt_boxes")


def make(tasks_ncls, pc_range, voxel, osf, overlap=0.1, min_radius=2, max_objs=64):
    from pillarnext_amd.assign import AssignLabel

    names, tasks = iter("abcdefghijklmnopqrstuvwxyz"), []
    for n in tasks_ncls:
        tasks.append([next(names) for _ in range(n)])
    return (AssignLabel(tasks, overlap, max_objs, min_radius, pc_range, voxel, osf),
            R.make_cfg(tasks_ncls, pc_range, voxel, osf, overlap, min_radius, max_objs))


def run(a, boxes, cls, num_gt=None):
    res = a.assign(torch.from_numpy(boxes).cuda(), torch.from_numpy(cls.astype(np.int32)).cuda(),
                   None if num_gt is None else torch.from_numpy(np.asarray(num_gt, np.int32)).cuda())
    torch.cuda.synchronize()
    out = {k: [t.cpu().numpy().copy() for t in res[k]] for k in KEYS}
    out["counts"] = res["counts"].cpu().numpy().copy()
    return out


def check(got, want, what=""):
    """got: the kernels' output, want: the twin's."""
    assert np.array_equal(got["counts"], want["counts"]), (what, got["counts"], want["counts"])
    for t in range(len(want["hm"])):
        for k in ("ind", "mask", "cat", "gt_boxes"):
            assert got[k][t].dtype == want[k][t].dtype and np.array_equal(got[k][t], want[k][t]), (what, t, k)
        da = R.ulp_distance(got["anno_box"][t], want["anno64"][t])
        dh = R.ulp_distance(got["hm"][t], want["hm64"][t])
        print(f"{what} task {t}: anno_box within {da.max():.3f}, hm within {dh.max():.3f} fp32 ulp of the fp64 twin; {int(want['mask'][t].sum())} objects")
        assert got["anno_box"][t].dtype == np.float32 and da.max() <= 1.0, (what, t, da.max())
        assert np.array_equal(got["anno_box"][t][..., [0, 1, 2, 6, 7]], want["anno_box"][t][..., [0, 1, 2, 6, 7]]), (what, t)
        assert got["hm"][t].dtype == np.float32 and got["hm"][t].shape == want["hm"][t].shape and dh.max() <= 1.0, (what, t, dh.max())
        assert (got["hm"][t][~want["windows"][t]] == 0.0).all(), (what, t)
        B, M = want["mask"][t].shape
        H, W = want["hm"][t].shape[2:]
        for b in range(B):
            m = want["mask"][t][b].astype(bool)
            ind, cat = got["ind"][t][b][m], got["cat"][t][b][m]
            assert (got["hm"][t][b, cat, ind // W, ind % W] == 1.0).all(), (what, t, b)


def fixture_case():
    g = load_golden("assign_small")
    a, cfg = make(g["cfg_tasks_ncls"].tolist(), g["cfg_pc_range"].tolist(), g["cfg_voxel_size"].tolist(), g["cfg_out_size_factor"].tolist(),
                  float(g["cfg_gaussian_overlap"]), int(g["cfg_min_radius"]), int(g["cfg_max_objs"]))
    return g, a, cfg


def test_fixture_case():
    g, a, cfg = fixture_case()
    got = run(a, g["in_boxes"][None], g["in_classes"][None])
    for t in range(3):  # the reference's own output
        for k in ("ind", "mask", "cat", "gt_boxes"):
            assert np.array_equal(got[k][t][0], g[f"t{t}_{k}"]), (t, k)
        assert np.array_equal(got["anno_box"][t][0][:, [0, 1, 2, 6, 7]], g[f"t{t}_anno_box"][:, [0, 1, 2, 6, 7]]), t
    check(got, R.assign(g["in_boxes"][None], g["in_classes"][None], cfg), "fixture")
    assert got["anno_box"][0][0][:, 0].min() == -0.75  # the centre in (-1, 0) cells is kept with its negative offset


def border_case():
    """Map 50 x 37 (grid 150 x 111, stride 3): odd in both dimensions, rows of 200 bytes (no 16-byte row pitch), a last tile of 5 rows;
    wide objects on the four borders and in the four corners, so that every window is clipped, plus a few inside."""
    a, cfg = make([2], [0.0, 0.0, -1.0, 30.0, 22.2, 1.0], [0.2, 0.2, 2.0], [3], max_objs=32)
    cells = [(0, 0), (49, 0), (0, 36), (49, 36), (25, 0), (25, 36), (0, 18), (49, 18), (12, 7), (40, 30), (31, 8), (8, 33)]
    rng = np.random.default_rng(7)
    b = np.zeros((1, len(cells), 9), np.float32)
    b[0, :, 0] = [(x + 0.4) * 0.6 for x, _ in cells]
    b[0, :, 1] = [(y + 0.6) * 0.6 for _, y in cells]
    b[0, :, 3:6] = rng.uniform(2.0, 9.0, (len(cells), 3))
    b[0, :, 6:9] = rng.normal(0, 1.5, (len(cells), 3))
    return a, cfg, b, (np.arange(len(cells)) % 2).astype(np.int32)[None]


def test_tile_remainders_and_clipped_windows():
    a, cfg, b, c = border_case()
    assert a.map_size == [(37, 50)]
    want = R.assign(b, c, cfg)
    assert int(want["counts"][0, 0]) == 12 and sorted(want["ind"][0][0][:8].tolist()) == sorted(y * 50 + x for x, y in [(0, 0), (49, 0), (0, 36), (49, 36), (25, 0), (25, 36), (0, 18), (49, 18)])
    check(run(a, b, c), want, "borders")


def chunk_case():
    """K = 1500 objects (six chunks of the object pass), 80 % of them in one task (more than one LDS round of the heat-map pass), maps 132 wide
    (two tiles per row) and 66 wide at the second stride."""
    a, cfg = make([2, 1], [0.0, 0.0, -1.0, 26.4, 4.0, 1.0], [0.1, 0.1, 2.0], [2, 4], max_objs=1536)
    rng = np.random.default_rng(11)
    B, K = 3, 1500
    b = np.zeros((B, K, 9), np.float32)
    b[:, :, 0] = rng.uniform(-0.5, 26.9, (B, K))
    b[:, :, 1] = rng.uniform(-0.2, 4.2, (B, K))
    b[:, :, 2] = rng.uniform(-1, 1, (B, K))
    b[:, :, 3:6] = np.exp(rng.uniform(-1.5, 0.5, (B, K, 3)))
    b[:, :, 6:9] = rng.normal(0, 2, (B, K, 3))
    c = np.where(rng.random((B, K)) < 0.8, rng.integers(0, 2, (B, K)), 2).astype(np.int32)
    c[rng.random((B, K)) < 0.03] = -1
    c[0, 5], c[0, 6] = 3, 1 << 20  # beyond the class table
    num_gt = np.array([1500, 0, 17], np.int32)
    for i in range(B):
        b[i, num_gt[i]:] = np.nan  # rows beyond num_gt must never be used
    return a, cfg, b, c, num_gt


def test_scan_across_chunks_and_num_gt():
    a, cfg, b, c, num_gt = chunk_case()
    assert a.map_size == [(20, 132), (10, 66)]
    want = R.assign(b, c, cfg, num_gt)
    assert int(want["counts"][0, 0]) > 1024 and int(want["counts"][0, 1]) > 128 and want["counts"][1].tolist() == [0, 0]
    got = run(a, b, c, num_gt)
    check(got, want, "chunks")
    # slot order is input order: the kept boxes of task 0, frame 0, are the valid rows of the input in sequence
    n0 = int(got["counts"][0, 0])
    xs = got["gt_boxes"][0][0, :n0, 0]
    pos = [int(np.nonzero(b[0, :, 0] == v)[0][0]) for v in xs]
    assert pos == sorted(pos) and len(set(pos)) == n0
    for t in range(2):  # the empty frame
        assert not got["hm"][t][1].any() and not got["mask"][t][1].any() and not got["ind"][t][1].any() and not got["anno_box"][t][1].any()
    # K = 0 is a call that works
    e = run(a, np.zeros((3, 0, 9), np.float32), np.zeros((3, 0), np.int32))
    assert not e["counts"].any() and all(not e[k][t].any() for k in KEYS for t in range(2))


def test_overflow_drops_the_later_objects():
    a, cfg = make([1, 1], [0.0, 0.0, -1.0, 16.0, 8.0, 1.0], [0.25, 0.25, 2.0], [1, 2], max_objs=8)
    b = np.zeros((1, 24, 9), np.float32)
    b[0, :, 0] = 0.6 + 0.62 * np.arange(24)
    b[0, :, 1] = 3.3
    b[0, :, 3:6] = 0.9
    b[0, :, 8] = np.linspace(-3, 3, 24)
    c = np.zeros((1, 24), np.int32)
    c[0, [2, 9, 13, 21]] = 1  # 20 objects for task 0, 4 for task 1
    want = R.assign(b, c, cfg)
    assert want["counts"].tolist() == [[20, 4]]
    got = run(a, b, c)
    check(got, want, "overflow")
    assert got["counts"].tolist() == [[20, 4]] and got["mask"][0][0].tolist() == [1] * 8 and got["mask"][1][0].tolist() == [1] * 4 + [0] * 4
    first8 = [i for i in range(24) if c[0, i] == 0][:8]
    assert np.array_equal(got["gt_boxes"][0][0][:, 0], b[0, first8, 0])
    # objects 9..20 of task 0 are absent from the heat map: with room for all of them their centre cells would read 1
    _, roomy = make([1, 1], [0.0, 0.0, -1.0, 16.0, 8.0, 1.0], [0.25, 0.25, 2.0], [1, 2], max_objs=32)
    allind = R.assign(b, c, roomy)["ind"][0][0][:20]
    assert np.array_equal(allind[:8], got["ind"][0][0])
    late = got["hm"][0][0, 0].reshape(-1)[allind[8:]]
    assert (late < 1.0).all() and (late[2:] == 0.0).all()  # the two nearest ones lie inside the window of the last kept object


def test_every_element_is_written_and_runs_are_identical():
    g, a, cfg = fixture_case()
    boxes = np.stack([g["in_boxes"], g["in_boxes"][::-1]])
    cls = np.stack([g["in_classes"], g["in_classes"][::-1]])
    want = R.assign(boxes, cls, cfg)
    out, counts, ws, _ = a._buffers(2, torch.device("cuda", torch.cuda.current_device()))
    for t in [counts, ws] + [t for k in KEYS for t in out[k]]:
        t.view(torch.uint8).fill_(0xFF)
    first = run(a, boxes, cls)
    check(first, want, "prefilled")
    for t in [counts, ws] + [t for k in KEYS for t in out[k]]:
        t.view(torch.uint8).fill_(0x5A)
    second = run(a, boxes, cls)
    for k in KEYS:
        for t in range(3):
            assert first[k][t].tobytes() == second[k][t].tobytes(), (k, t)
    assert np.array_equal(first["counts"], second["counts"])


def test_labels_feed_the_fused_loss(monkeypatch):
    """The fixture's 40 x 48 two-class task through CenterHead.loss: fused kernels against the module losses, tolerances of tests/test_gpu_loss.py."""
    from pillarnext_amd.models import CenterHead

    g, a, _ = fixture_case()
    res = a.assign(torch.from_numpy(g["in_boxes"][None]).cuda(), torch.from_numpy(g["in_classes"][None]).cuda())
    ex = {k: [res[k][1].clone()] for k in KEYS}
    assert int(ex["mask"][0].sum()) == int(g["t1_mask"].sum()) > 20
    common = {"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2), "iou": (1, 2)}
    head = CenterHead(16, [["b", "c"]], 0.25, [1.0] * 6 + [0.2, 0.2, 1.0, 1.0], common, [2], share_conv_channel=16, with_reg_iou=True,
                      voxel_size=g["cfg_voxel_size"].tolist(), pc_range=g["cfg_pc_range"].tolist(), out_size_factor=[4]).cuda()
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("PNX_FUSED_LOSS", mode)
        gen = torch.Generator(device="cuda").manual_seed(3)
        r = lambda *s: torch.randn(*s, device="cuda", generator=gen)  # noqa: E731
        pd = {"hm": r(1, 2, 40, 48) - 2.0, "reg": torch.rand((1, 2, 40, 48), device="cuda", generator=gen), "height": r(1, 1, 40, 48) * 0.5,
              "dim": r(1, 3, 40, 48) * 0.4 + 0.5, "rot": r(1, 2, 40, 48), "vel": r(1, 2, 40, 48), "iou": r(1, 1, 40, 48) * 0.5}
        pd = {k: v.requires_grad_(True) for k, v in pd.items()}
        total, rets = head.loss(ex, [pd])
        total.backward()
        out[mode] = (float(total), {k: float(rets[0][k]) for k in rets[0] if k.endswith("loss")}, rets[0]["loc_loss_elem"].detach().cpu().float(),
                     {k: v.grad.clone() for k, v in pd.items()})
    t0, l0, e0, g0 = out["0"]
    t1, l1, e1, g1 = out["1"]
    assert np.isfinite(t1) and all(np.isfinite(v) for v in l1.values()) and bool(torch.isfinite(e1).all())
    assert abs(t0 - t1) <= 2e-5 * abs(t0) + 1e-6, (t0, t1)
    for k in l0:
        assert abs(l0[k] - l1[k]) <= 2e-5 * abs(l0[k]) + 1e-6, (k, l0[k], l1[k])
    torch.testing.assert_close(e1, e0, rtol=2e-5, atol=1e-7)
    for k in g0:
        torch.testing.assert_close(g1[k], g0[k], rtol=2e-4, atol=2e-7, msg=lambda s, k=k: f"grad {k}: {s}")
