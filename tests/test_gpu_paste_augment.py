"""GPU: the GT paste and augmentation kernels (csrc/augment.hip) against tests/paste_augment_ref.py, the fp64 numpy statement that
tests/test_paste_augment_cpu.py pins to the recorded run of the reference.

Bounds.  Selection: accept, the merged boxes, classes and counts are exactly equal; the seeded inputs are shown on the CPU to keep every decision
when all centres move by 1e-6 m and all yaws by 1e-7, far more than the distance between two fp64 sin / cos routines, and the planted degenerate
pairs use yaw 0 and dyadic numbers, for which both sides compute the same corners exactly.  Points: every row is bit-equal, except that a scene
row within 1e-5 m of a face plane of an accepted box (fp64 local frame) may be kept or removed (at most 0.1 % of the rows; the seeded layout has
none but the planted on-face rows, which are exact and must be removed).  Transforms: bit-equal -- every stage is a single correctly rounded
operation or a pair of fp64 products and one fp64 sum on values both sides share (cos a and sin a come from the host)."""
import numpy as np
import pytest

import paste_augment_cases as C
import paste_augment_ref as R
from conftest import load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_cand(cand):
    return None if cand is None else {k: dev(v) for k, v in cand.items()}


def run_select(gt, cls, num_gt, cand, bank_offsets, n_groups):
    from pillarnext_amd import ops

    B, K, D = gt.shape
    S = 0 if cand is None else cand["bank"].shape[1]
    e = lambda shape, dt: torch.full(shape, 77, dtype=dt, device="cuda")  # noqa: E731
    out = {"accept": e((B, S), torch.uint8), "paste_offset": e((B, S), torch.int32), "boxes": e((B, K + S, D), torch.float32),
           "classes": e((B, K + S), torch.int32), "num": e((B,), torch.int32), "pasted_rows": e((B,), torch.int32)}
    ops.paste_select(dev(gt), dev(cls), dev(num_gt), dev_cand(cand), dev(bank_offsets), n_groups, out)
    return out


def run_points(points, B, cand, sel, bank_points, bank_offsets, xform, capacity):
    from pillarnext_amd import ops

    out = torch.full((capacity, points.shape[1]), 12345.0, dtype=torch.float32, device="cuda")       # the sentinel: every row must be written
    n_out = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    frame_rows = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.paste_augment_workspace_bytes(len(points), B) + 256, dtype=torch.uint8, device="cuda")
    ops.paste_augment_points(dev(points), B, dev_cand(cand), None if sel is None else sel["paste_offset"], None if sel is None else sel["pasted_rows"],
                             dev(bank_points), dev(bank_offsets), dev(xform), out, n_out, frame_rows, ws)
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(n_out.item()), frame_rows.cpu().numpy()


def test_selection():
    c = C.selection_batch()
    _, off = C.object_bank()
    out = run_select(c["gt"], c["cls"], c["num_gt"], c["cand"], off, c["n_groups"])
    again = run_select(c["gt"], c["cls"], c["num_gt"], c["cand"], off, c["n_groups"])
    B, K, _ = c["gt"].shape
    S = c["cand"]["bank"].shape[1]
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for k, v in again.items():
        assert np.array_equal(got[k].view(np.uint8), v.cpu().numpy().view(np.uint8)), k
    rows = np.diff(off)
    for b in range(B):
        ng = int(c["num_gt"][b])
        valid = c["cand"]["bank"][b] >= 0
        accept, order = R.select(c["gt"][b, :ng], c["cand"]["boxes"][b], c["cand"]["group"][b], c["n_groups"], valid)
        boxes, classes, n = R.merge_boxes(c["gt"][b, :ng], c["cls"][b, :ng], c["cand"]["boxes"][b], c["cand"]["cls"][b], order, K + S)
        assert np.array_equal(got["accept"][b].astype(bool), accept), (b, got["accept"][b], accept)
        assert got["num"][b] == n and np.array_equal(got["classes"][b], classes) and same_bits(got["boxes"][b], boxes), b
        want_off = np.full(S, -1, np.int64)
        at = 0
        for i in order:
            want_off[i] = at
            at += rows[c["cand"]["bank"][b, i]]
        assert np.array_equal(got["paste_offset"][b], want_off) and got["pasted_rows"][b] == at, b
    assert np.array_equal(got["accept"][0][c["planted_index"]].astype(bool), C.planted()[3])
    assert got["accept"][1].sum() >= 5 and not got["accept"][1][21:].any() and not got["accept"][2].any() and got["num"][2] == 20


def test_selection_limit_and_full_size():
    from pillarnext_amd import _lib, ops

    # one box more than the limit: an error from the host check, nothing launched, nothing written
    gt = np.zeros((1, 500, 9), np.float32)
    cand = dict(bank=np.zeros((1, 13), np.int32), boxes=np.zeros((1, 13, 9), np.float32), cls=np.zeros((1, 13), np.int32), group=np.zeros((1, 13), np.int32))
    with pytest.raises(_lib.PnxError, match="PNX_PASTE_MAX_BOXES"):
        run_select(gt, np.zeros((1, 500), np.int32), None, cand, np.array([0, 5], np.int64), 1)
    assert torch.cuda.is_available() and ops.paste_chunk_rows() == 2048
    # exactly the limit, with enough candidates for the layout that needs more than 64 KiB of LDS: 200 gt boxes on a 10 m grid, 312
    # candidates of 4 groups between them, candidate 7 moved onto a gt box, candidate 300 onto candidate 5 (an accepted one of an earlier group)
    K, S = 200, 312
    gt = np.zeros((1, K, 9), np.float32)
    gt[0, :, 0], gt[0, :, 1] = 10.0 * (np.arange(K) % 25), 10.0 * (np.arange(K) // 25)
    gt[0, :, 3:6], gt[0, :, 8] = 2.0, 0.3
    cand = dict(bank=np.zeros((1, S), np.int32), boxes=np.zeros((1, S, 9), np.float32), cls=np.ones((1, S), np.int32), group=(np.arange(S, dtype=np.int32) // 78)[None])
    cand["boxes"][0, :, 0], cand["boxes"][0, :, 1] = 5.0 + 10.0 * (np.arange(S) % 26), 5.0 + 10.0 * (np.arange(S) // 26)
    cand["boxes"][0, :, 3:6], cand["boxes"][0, :, 8] = 2.0, -0.2
    cand["boxes"][0, 7, :2] = [240.5, 70.5]        # on the last gt box (240, 70)
    cand["boxes"][0, 300, :2] = cand["boxes"][0, 5, :2] + 0.5
    out = run_select(gt, np.arange(K, dtype=np.int32)[None], None, cand, np.array([0, 5], np.int64), 4)
    want = np.ones(S, bool)
    want[[7, 300]] = False
    assert np.array_equal(out["accept"].cpu().numpy()[0].astype(bool), want)
    assert int(out["num"].item()) == K + S - 2 and int(out["pasted_rows"].item()) == 5 * (S - 2)


@pytest.fixture(scope="module")
def chunk():
    from pillarnext_amd import ops

    return ops.paste_chunk_rows()


def compare_points(got, n_out, frame_rows, want, capacity, planted_tags=()):
    """Rows are identified by their tag (column 4).  Scene rows within 1e-5 m of a face plane may be kept or removed: they are taken out of both
    sides, everything else must be bit-equal, frame by frame and in order.  Returns how many rows were left out (the planted on-face rows, which
    the caller checks on their own, not counted)."""
    assert n_out <= capacity and (got[n_out:, 0] == -1.0).all() and not got[n_out:, 1:].any(), "rows [n_out, capacity) must be -1 rows, all written"
    assert not (got == 12345.0).any()
    amb = want["ambiguous"][:, 3]
    at_g = at_w = 0
    for b in range(len(want["frame_rows"])):
        gr = got[at_g:at_g + int(frame_rows[b])]
        wr = want["points"][at_w:at_w + int(want["frame_rows"][b])]
        assert (gr[:, 0] == b).all(), b
        gsel, wsel = gr[~np.isin(gr[:, 4], amb)], wr[~np.isin(wr[:, 4], amb)]
        assert gsel.shape == wsel.shape and np.array_equal(bits(gsel), bits(wsel)), (b, gsel.shape, wsel.shape)
        at_g += int(frame_rows[b])
        at_w += int(want["frame_rows"][b])
    assert at_g == n_out
    return int((~np.isin(amb, np.asarray(planted_tags, np.float32))).sum())


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_points_at_the_seams(chunk, delta):
    total = 3 * chunk + delta
    c = C.points_batch(total)
    xf = np.stack([R.xform_row(angle=0.3, scale=1.05, translate=-0.2, flip_x=True), R.xform_row(), R.xform_row(angle=-0.6, translate=0.4, flip_y=True)])
    sel = run_select(c["gt"], c["cls"], c["num_gt"], c["cand"], c["bank_offsets"], c["n_groups"])
    capacity = total + int(np.diff(c["bank_offsets"])[c["cand"]["bank"][c["cand"]["bank"] >= 0]].sum())
    got, n_out, frame_rows = run_points(c["points"], 3, c["cand"], sel, c["bank_points"], c["bank_offsets"], xf, capacity)
    got2, n_out2, _ = run_points(c["points"], 3, c["cand"], sel, c["bank_points"], c["bank_offsets"], xf, capacity)
    assert n_out2 == n_out and np.array_equal(bits(got), bits(got2)), "two runs must be bit-identical"
    want = R.paste_and_augment(c["points"], c["gt"], c["cls"], c["num_gt"], c["cand"], c["bank_points"], c["bank_offsets"], c["n_groups"], xf)
    assert np.array_equal(sel["accept"].cpu().numpy().astype(bool), want["accept"])
    # frame 0 loses its only scene row, frame 1 never had one: both hold pasted rows only
    rows = np.diff(c["bank_offsets"])
    assert frame_rows[0] == rows[0] and frame_rows[1] == rows[3] + rows[4]
    assert not np.isin(c["planted_tags"].astype(np.float32), got[:n_out, 4]).any(), "a row exactly on a face must be removed"
    left_out = compare_points(got, n_out, frame_rows, want, capacity, c["planted_tags"])
    print(f"total {total}: n_out {n_out}, frame rows {frame_rows.tolist()}, {left_out} near-face rows left out")
    assert left_out <= 0.001 * total
    assert n_out == len(want["points"]) or left_out > 0
    # the frame boundary and the start of the -1 tail lie inside chunks
    assert 0 < frame_rows[0] % chunk and 0 < n_out % chunk and n_out < capacity


def test_interleaved_frames_keep_their_order(chunk):
    """Rows of the frames shuffled into each other: every frame's survivors keep their input order."""
    c = C.points_batch(2 * chunk + 300)
    rng = np.random.default_rng(9)
    pts = c["points"].copy()
    live = pts[:, 0] == 2.0
    pts[live, 0] = rng.integers(0, 3, int(live.sum())).astype(np.float32)
    sel = run_select(c["gt"], c["cls"], c["num_gt"], c["cand"], c["bank_offsets"], c["n_groups"])
    capacity = len(pts) + 2100
    got, n_out, frame_rows = run_points(pts, 3, c["cand"], sel, c["bank_points"], c["bank_offsets"], None, capacity)
    want = R.paste_and_augment(pts, c["gt"], c["cls"], c["num_gt"], c["cand"], c["bank_points"], c["bank_offsets"], c["n_groups"])
    assert compare_points(got, n_out, frame_rows, want, capacity, c["planted_tags"]) <= 0.001 * len(pts)
    assert np.array_equal(frame_rows, want["frame_rows"]) and min(frame_rows) > 500


@pytest.mark.parametrize("cols", [7, 9])
def test_transforms_every_combination(cols):
    from pillarnext_amd import ops

    rng = np.random.default_rng(21)
    xf = C.xform_combos(rng)
    xf[3, 2], xf[3, 0], xf[3, 1] = 0.78, np.cos(0.78), np.sin(0.78)          # rotation + scaling, a yaw pushed across +pi
    B = len(xf)
    b1 = C.transform_boxes(cols)
    boxes = np.tile(b1[None], (B, 1, 1))
    num = np.full(B, len(b1), np.int32)
    num[5] = 10
    t = dev(boxes)
    ops.augment_boxes_(t, dev(num), dev(xf))
    got = t.cpu().numpy()
    for b in range(B):
        want = boxes[b].copy()
        want[:num[b]] = R.augment_boxes(boxes[b, :num[b]], xf[b])
        assert same_bits(got[b], want), (cols, b, int(xf[b, 5]))
    if cols == 9:
        assert np.isnan(got[:, 5, 6]).all() and np.isfinite(got[:, 5, 7]).all() and np.isnan(got[:, 11, 6:8]).all()
    assert (np.abs(got[8:, :, -1]) <= np.float32(np.pi) + 1e-6).all()          # after a flip the yaw is wrapped
    # the points of the same 32 frames, augment only (no candidates), 120 rows each, in one call
    g = load_golden("paste_augment_small")
    pts = np.zeros((B * 120, 6), np.float32)
    pts[:, 0] = np.repeat(np.arange(B), 120)
    pts[:, 1:4] = g["in_points"][:B * 120]
    pts[:, 4:] = rng.random((B * 120, 2))
    gp, n_out, frame_rows = run_points(pts, B, None, None, None, None, xf, len(pts) + 3)
    assert n_out == len(pts) and (frame_rows == 120).all() and (gp[n_out:, 0] == -1).all()
    for b in range(B):
        want = pts[b * 120:(b + 1) * 120].copy()
        want[:, 1:4] = R.augment_points(want[:, 1:4], xf[b])
        assert np.array_equal(bits(gp[b * 120:(b + 1) * 120]), bits(want)), (b, int(xf[b, 5]))


def fixture_assigner():
    import assign_fp64_ref as RA
    from pillarnext_amd.assign import AssignLabel

    g = load_golden("assign_small")
    names, tasks = iter("abcdefghijklmnopqrstuvwxyz"), []
    for n in g["cfg_tasks_ncls"].tolist():
        tasks.append([next(names) for _ in range(n)])
    args = (g["cfg_pc_range"].tolist(), g["cfg_voxel_size"].tolist(), g["cfg_out_size_factor"].tolist())
    a = AssignLabel(tasks, float(g["cfg_gaussian_overlap"]), int(g["cfg_max_objs"]), int(g["cfg_min_radius"]), *args)
    cfg = RA.make_cfg(g["cfg_tasks_ncls"].tolist(), *args, float(g["cfg_gaussian_overlap"]), int(g["cfg_min_radius"]), int(g["cfg_max_objs"]))
    return a, cfg, RA


def test_augment_only_through_the_entry_point():
    """paste_and_augment without a sampler: the draws are numpy's for the seed, frame-major; the result is the statement's."""
    from pillarnext_amd import augment as A

    g = load_golden("paste_augment_small")
    aug = {"rotation": A.Rotation(g["cfg_rotation"].tolist()), "scaling": A.Scaling(g["cfg_scale"].tolist()), "translation": A.Translation(float(g["cfg_noise"])),
           "flip": A.Flip(g["cfg_flip_prob"].tolist())}
    B = 2
    boxes = np.stack([g["in_boxes"], g["in_boxes"][::-1]])
    cls = np.stack([g["in_classes"], g["in_classes"][::-1]]).astype(np.int32)
    num_gt = np.array([48, 31], np.int32)
    pts = np.zeros((4000, 6), np.float32)
    pts[:, 0] = np.arange(4000) % 2
    pts[:, 1:4] = g["in_points"]
    np.random.seed(5)
    po, n_out, bo, co, no = A.paste_and_augment(dev(pts), dev(boxes), dev(cls), dev(num_gt), None, aug)
    np.random.seed(5)
    xf = np.stack([A.draw_xform(aug) for _ in range(B)])
    assert len(set(xf[:, 2])) == 2
    want = R.paste_and_augment(pts, boxes, cls, num_gt, xforms=xf)
    assert int(n_out.item()) == 4000 and np.array_equal(bits(po.cpu().numpy()), bits(want["points"]))
    assert np.array_equal(no.cpu().numpy(), num_gt) and np.array_equal(co.cpu().numpy(), want["classes"]) and same_bits(bo.cpu().numpy(), want["boxes"])


def test_merged_sweeps_feed_the_paste():
    """SweepMerger's whole output, -1 tail included, goes in; the result is that of its first n_out rows."""
    from pillarnext_amd.io import SweepMerger

    rng = np.random.default_rng(12)
    raw = np.zeros((9000, 5), np.float32)
    raw[:, :2] = rng.uniform(0, 40, (9000, 2))
    raw[: 900, :2] = rng.uniform(-0.9, 0.9, (900, 2))      # removed by the close-point filter of the past sweeps
    raw[:, 2] = rng.uniform(-1.5, 2.5, 9000)
    raw[:, 3] = np.arange(9000)                            # the tag
    segs = [dict(begin=0, end=2000, batch=0, time=0.05, radius=1.0, transform=None), dict(begin=2000, end=5000, batch=0, time=0.0, radius=0.0, transform=None),
            dict(begin=5000, end=9000, batch=2, time=0.0, radius=0.0, transform=None)]
    merged, m_out = SweepMerger()(dev(raw), segs, n_copy=4)
    c = C.points_batch(3 * 2048)
    sel = run_select(c["gt"], c["cls"], c["num_gt"], c["cand"], c["bank_offsets"], c["n_groups"])
    host = merged.cpu().numpy()
    m = int(m_out.item())
    assert m < 9000 - 500 and (host[m:, 0] == -1).all()
    # the bank rows have 5 columns, the merged rows 1 + 5
    capacity = 9000 + 2100
    got, n_out, frame_rows = run_points(host, 3, c["cand"], sel, c["bank_points"], c["bank_offsets"], None, capacity)
    want = R.paste_and_augment(host[:m], c["gt"], c["cls"], c["num_gt"], c["cand"], c["bank_points"], c["bank_offsets"], c["n_groups"])
    assert compare_points(got, n_out, frame_rows, want, capacity) <= 9     # 0.1 % of the rows
    assert np.array_equal(frame_rows, want["frame_rows"])


def test_end_to_end_into_assign():
    """paste_and_augment -> AssignLabel.assign on the fixture's three tasks (40 x 48 and 80 x 96 maps) equals assign on the statement's boxes."""
    from pillarnext_amd import augment as A
    from pillarnext_amd import synth

    g = load_golden("paste_augment_small")
    assigner, cfg, RA = fixture_assigner()
    names = assigner.class_names
    bank = synth.make_object_bank(names, 8, seed=2, point_dim=5, max_points=200)
    for ci, name in enumerate(names):              # into the fixture's 19.2 m x 16 m range, small enough to leave room
        for k, info in enumerate(bank[name]):
            info["box3d_lidar"][:2] = [-8.5 + 17.0 * ((ci * 8 + k) % 7) / 6.0 + 0.3 * ci, -7.0 + 14.0 * ((ci * 8 + k) // 7) / 5.0]
            info["box3d_lidar"][3:6] *= 0.3
    np.random.seed(8)
    sampler = A.DataBaseSamplerV2(groups=[{names[0]: 12}, {names[2]: 14, names[4]: 13}], rate=1.0, db_infos=bank, class_names=names)
    aug = [A.Rotation([-0.3, 0.3]), A.Scaling([0.95, 1.05]), A.Translation(0.2), A.Flip([0.5, 0.5])]
    B = 2
    boxes = np.nan_to_num(np.stack([g["in_boxes"][:40], g["in_boxes"][8:48]]))     # the NaN velocities have their own test; assign's twin compares values
    boxes[:, :, 3:6] *= 0.5
    cls = np.stack([g["in_classes"][:40], g["in_classes"][8:48]]).astype(np.int32)
    num_gt = np.array([40, 33], np.int32)
    pts = np.zeros((4000, 6), np.float32)
    pts[:, 0] = (np.arange(4000) >= 1500).astype(np.float32)
    pts[:, 1:4], pts[:, 4] = g["in_points"], np.arange(4000)
    host_classes = [cls[b, :num_gt[b]] for b in range(B)]
    stage = A.PasteAugment(sampler, aug)
    state = np.random.get_state()
    po, n_out, bo, co, no = stage(dev(pts), dev(boxes), dev(cls), dev(num_gt), host_classes=host_classes)
    labels = assigner.assign(bo, co, no)
    torch.cuda.synchronize()
    # the same draws on the host: a second sampler built from the same seed, then the statement
    np.random.seed(8)
    twin = A.DataBaseSamplerV2(groups=[{names[0]: 12}, {names[2]: 14, names[4]: 13}], rate=1.0, db_infos=bank, class_names=names)
    assert np.array_equal(np.random.get_state()[1], state[1])
    frames, xf = [], []
    for b in range(B):
        frames.append(twin.sample_frame(host_classes[b]))
        xf.append(A.draw_xform(aug))
    S = bo.shape[1] - 40
    assert S % 8 == 0 and max(len(f) for f in frames) <= S and min(len(f) for f in frames) >= 5
    cand = dict(bank=np.full((B, S), -1, np.int32), boxes=np.zeros((B, S, 9), np.float32), cls=np.full((B, S), -1, np.int32), group=np.full((B, S), -1, np.int32))
    for b, f in enumerate(frames):
        for i, (bank_id, box, c, grp) in enumerate(f):
            cand["bank"][b, i], cand["boxes"][b, i], cand["cls"][b, i], cand["group"][b, i] = bank_id, box, c, grp
    bank_points, bank_offsets = twin.bank_host()
    want = R.paste_and_augment(pts, boxes, cls, num_gt, cand, bank_points, bank_offsets, sampler.n_groups, np.stack(xf))
    assert want["accept"].sum() >= 6 and (~want["accept"] & (cand["bank"] >= 0)).sum() >= 3, "the case must accept some candidates and reject some"
    assert np.array_equal(no.cpu().numpy(), want["num"]) and np.array_equal(co.cpu().numpy(), want["classes"]) and same_bits(bo.cpu().numpy(), want["boxes"])
    n = int(n_out.item())
    assert n == len(want["points"]) and np.array_equal(bits(po.cpu().numpy()[:n]), bits(want["points"])) and (po.cpu().numpy()[n:, 0] == -1).all()
    ref = RA.assign(want["boxes"], want["classes"], cfg, want["num"])
    for t in range(3):
        for k in ("ind", "mask", "cat", "gt_boxes"):
            assert np.array_equal(labels[k][t].cpu().numpy(), ref[k][t]), (t, k)
        assert RA.ulp_distance(labels["hm"][t].cpu().numpy(), ref["hm64"][t]).max() <= 1.0 and RA.ulp_distance(labels["anno_box"][t].cpu().numpy(), ref["anno64"][t]).max() <= 1.0
    assert np.array_equal(labels["counts"].cpu().numpy(), ref["counts"])
