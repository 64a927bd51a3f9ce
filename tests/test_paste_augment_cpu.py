"""CPU: the yardstick of the GT paste / augmentation kernels and their host side.

tests/paste_augment_ref.py (the fp64 numpy statement tests/test_gpu_paste_augment.py holds the kernels to) against the recorded run of the
reference's augmentation.py (tests/golden/paste_augment_small.npz, written by tools/gen_paste_golden.py): flip, scaling and translation bit
for bit; rotation within 1 fp32 ulp of the recorded run (numpy hands the fp32 x fp64 matrix product to a BLAS, which may fuse the sum) and bit
for bit against the stepwise formula.  The draws and the BatchSampler index sequences against the same fixture, sampled_num's rounding, the
planted collision cases, the robustness of the seeded inputs the GPU tests use, and the argument checks of the new entry points."""
import ctypes

import numpy as np
import pytest

import paste_augment_cases as C
import paste_augment_ref as R
from conftest import load_golden


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    """bit-equal, any NaN counting as equal to any NaN at the same place"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    d = np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
    return np.where(np.isnan(a) & np.isnan(b), 0.0, d)


def fixture_xform(draws):
    a, s, t, fx, fy = draws
    return R.xform_row(angle=a, scale=s, translate=t, flip_x=bool(fx), flip_y=bool(fy))


@pytest.fixture(scope="module")
def g():
    return load_golden("paste_augment_small")


def test_statement_equals_the_recorded_run(g):
    worst = 0.0
    for ci in range(len(g["seeds"])):
        n = len(g[f"c{ci}_points_rot"])
        boxes = g["in_boxes"] if g[f"c{ci}_boxes_rot"].shape[1] == 9 else g["in_boxes"][:, [0, 1, 2, 3, 4, 5, 8]]
        xf = fixture_xform(g[f"c{ci}_draws"])
        for what, mine, pre in (("points", R.points_stages(g["in_points"][:n], xf), "points"), ("boxes", R.boxes_stages(boxes, xf), "boxes")):
            rec = [g[f"c{ci}_{pre}_{k}"] for k in ("rot", "scale", "trans", "flip")]
            d = ulps(mine[0], rec[0])
            worst = max(worst, float(d.max()))
            assert d.max() <= 1.0, (ci, what, d.max())
            # the later stages start from the RECORDED rotation, so that a fused sum there cannot hide a difference here
            cont = (R.points_stages if what == "points" else R.boxes_stages)(rec[0], _without_rotation(xf))
            assert same_bits(cont[1], rec[1]), (ci, what, "scaling")
            assert same_bits(cont[2], rec[2]), (ci, what, "translation")
            assert same_bits(cont[4], rec[3]), (ci, what, "flip")
    print(f"rotation: the recorded run lies within {worst:.2f} fp32 ulp of the stepwise formula")


def _without_rotation(xf):
    xf = xf.copy()
    xf[5] = float(int(xf[5]) & ~R.ROTATE)
    return xf


def test_rotation_is_the_stepwise_formula(g):
    xf = fixture_xform(g["c0_draws"])
    p = g["in_points"]
    c, s = np.cos(xf[2]), np.sin(xf[2])
    x, y = p[:, 0].astype(np.float64), p[:, 1].astype(np.float64)
    got = R.points_stages(p, xf)[0]
    assert np.array_equal(bits(got[:, 0]), bits(((x * c) - (y * s)).astype(np.float32)))
    assert np.array_equal(bits(got[:, 1]), bits(((x * s) + (y * c)).astype(np.float32)))
    assert np.array_equal(bits(got[:, 2]), bits(p[:, 2]))
    b = R.boxes_stages(g["in_boxes"], xf)[0]
    assert np.isnan(b[5, 6]) and not np.isnan(b[5, 7]) and np.isnan(b[11, 6:8]).all()
    vy = g["in_boxes"][5, 7].astype(np.float64)
    assert b[5, 7] == np.float32((0.0 * s) + (vy * c))     # a finite vy next to a NaN vx: rotated with vx = 0
    assert np.array_equal(bits(b[:, 8]), bits(g["in_boxes"][:, 8] + np.float32(xf[2])))


def test_draws_and_sampler_sequences(g):
    from pillarnext_amd import augment as A

    aug = {"rotation": A.Rotation(g["cfg_rotation"].tolist()), "scaling": A.Scaling(g["cfg_scale"].tolist()), "translation": A.Translation(float(g["cfg_noise"])),
           "flip": A.Flip(g["cfg_flip_prob"].tolist())}
    for ci, seed in enumerate(g["seeds"]):
        np.random.seed(int(seed))
        xf = A.draw_xform(aug)
        assert np.array_equal(xf, fixture_xform(g[f"c{ci}_draws"])), (ci, xf, g[f"c{ci}_draws"])
    si = 0
    wrapped = 0
    while f"s{si}_cfg" in g:
        seed, n = (int(v) for v in g[f"s{si}_cfg"])
        np.random.seed(seed)
        s = A.BatchSampler(list(range(100, 100 + n)), "x")
        at = 0
        for k, want_len in zip(g[f"s{si}_calls"], g[f"s{si}_lens"]):
            got = s.sample(int(k))
            assert got == g[f"s{si}_items"][at:at + want_len].tolist(), (si, int(k))
            wrapped += int(want_len != k)
            at += int(want_len)
        si += 1
    assert si >= 3 and wrapped >= 3
    with pytest.raises(ValueError):
        A.draw_xform([A.Scaling([0.9, 1.1]), A.Rotation([-1, 1])])     # not the kernels' order
    with pytest.raises(ValueError):
        A.Flip([1.0, 0.0])
    np.random.seed(1)
    state = np.random.get_state()[1].copy()
    assert A.Flip([0.0, 0.0]).draw() == (False, False) and np.array_equal(np.random.get_state()[1], state)   # probability 0: no draw


def test_sampled_num_rounding():
    from pillarnext_amd.augment import sampled_num

    assert [sampled_num(0.5, 5, 0), sampled_num(0.5, 3, 0), sampled_num(0.5, 7, 0), sampled_num(1.0, 2, 5), sampled_num(0.3, 6, 1)] == [2, 2, 4, -3, 2]


def test_planted_collision_cases():
    gt, cand, group, expect = C.planted()
    cg, cc = R.corners(gt), R.corners(cand)
    assert R.collide(cc[0], cg[0]) and R.collide(cg[0], cc[0])                   # containment, either way round
    assert not R.collide(cc[1], cg[1]) and not R.collide(cg[1], cc[1])           # collinear edges: overlap in area, no collision by the inequalities
    assert not R.collide(cc[2], cg[2])                                           # touching
    assert R.collide(cc[3], cc[4]) and R.collide(cc[5], cc[6]) and R.collide(cc[7], cc[3]) and not R.collide(cc[7], cc[4]) and R.collide(cc[8], cc[4])
    accept, order = R.select(gt, cand, group, 3)
    assert np.array_equal(accept, expect), accept
    assert order == [1, 2, 4, 6, 7]
    boxes, classes, n = R.merge_boxes(gt, np.arange(3), cand, 10 + np.arange(9), order, 12)
    assert n == 8 and classes.tolist() == [0, 1, 2, 11, 12, 14, 16, 17, -1, -1, -1, -1] and np.array_equal(boxes[3], cand[1]) and not boxes[8:].any()


def _decisions(case, shift=None):
    """accept (B, S) of a seeded case; shift = (centre shift (.., 2), yaw shift (..)) generators applied in fp64"""
    out = []
    for b in range(len(case["gt"])):
        ng = int(case["num_gt"][b])
        gt, cand = case["gt"][b, :ng].astype(np.float64), case["cand"]["boxes"][b].astype(np.float64)
        if shift is not None:
            for arr in (gt, cand):
                arr[:, :2] += shift[0](arr[:, :2].shape)
                arr[:, -1] += shift[1](arr[:, -1].shape)
        out.append(R.select(gt, cand, case["cand"]["group"][b], case["n_groups"], case["cand"]["bank"][b] >= 0)[0])
    return np.stack(out)


@pytest.mark.parametrize("case", ["selection", "points"])
def test_seeded_inputs_are_robust(case):
    """Every decision of the seeded inputs survives moving every centre by +-1e-6 m and every yaw by +-1e-7: the kernels' own sin / cos cannot flip
    one.  (The planted degenerate pairs are exact by construction -- yaw 0, dyadic numbers -- and are left where they are.)"""
    c = C.selection_batch() if case == "selection" else C.points_batch(3 * 2048)
    base = _decisions(c)
    if case == "selection":
        assert base[0].sum() >= 8 and base[1].sum() >= 5 and not base[2].any() and (~base[0]).sum() >= 6
        assert np.array_equal(base[0][c["planted_index"]], C.planted()[3])
        degenerate = np.zeros(base.shape, bool)
        degenerate[0, c["planted_index"][[1, 2]]] = True
    else:
        assert base.tolist() == [[1] + [0] * 7, [1, 1] + [0] * 6, [1, 0, 0, 1, 1, 1, 1, 1]]
        degenerate = np.zeros(base.shape, bool)
    rng = np.random.default_rng(0)
    signs = [(lambda s: np.full(s, 1e-6), lambda s: np.full(s, 1e-7)), (lambda s: np.full(s, -1e-6), lambda s: np.full(s, -1e-7)),
             (lambda s: np.full(s, 1e-6), lambda s: np.full(s, -1e-7))] + [(lambda s: rng.choice([-1e-6, 1e-6], s), lambda s: rng.choice([-1e-7, 1e-7], s))] * 3
    for sh in signs:
        moved = _decisions(c, sh)
        assert np.array_equal(moved[~degenerate], base[~degenerate])


def test_point_layout_has_no_near_face_rows():
    c = C.points_batch(3 * 2048 + 1)
    want = R.paste_and_augment(c["points"], c["gt"], c["cls"], c["num_gt"], c["cand"], c["bank_points"], c["bank_offsets"], c["n_groups"])
    near = int((want["near"] < 1e-5).sum()) + int((want["removed_near"] < 1e-5).sum())
    assert near == len(C.FACE_POINTS) - 1, near      # only the planted on-face rows (margin exactly 0; the box centre is not near a face)
    assert want["frame_rows"][0] == int(np.diff(c["bank_offsets"])[0]) and want["frame_rows"][1] == int(np.diff(c["bank_offsets"])[[3, 4]].sum())
    tags = want["points"][:, 4]
    assert not np.isin(c["planted_tags"], tags).any() and 0.0 not in tags        # the on-face rows and frame 0's only row are gone


def test_refusals_and_argument_checks():
    from pillarnext_amd import _lib, synth
    from pillarnext_amd import augment as A

    bank = synth.make_object_bank(["car", "pedestrian"], 6, seed=1)
    assert all(len(i["points"]) >= 5 and i["points"].dtype == np.float32 and np.abs(i["points"][:, :3]).max() < 8 for v in bank.values() for i in v)
    with pytest.raises(ValueError, match="gt_drop_percentage"):
        A.DataBaseSamplerV2(groups=[{"car": 2}], rate=1.0, gt_drop_percentage=0.2, db_infos=bank)
    bad = synth.make_object_bank(["car"], 2, seed=1)
    bad["car"][1]["rot_transform"] = 0.1
    with pytest.raises(ValueError, match="rot_transform"):
        A.DataBaseSamplerV2(groups=[{"car": 2}], rate=1.0, db_infos=bad)

    class OnDevice:
        pass

    dev = synth.make_object_bank(["car"], 2, seed=1)
    dev["car"][0]["points"] = OnDevice()
    with pytest.raises(ValueError, match="host"):
        A.DataBaseSamplerV2(groups=[{"car": 2}], rate=1.0, db_infos=dev)
    np.random.seed(0)
    s = A.DataBaseSamplerV2(groups=[{"car": 4}, {"pedestrian": 3}], rate=1.0, db_infos=bank, class_names=["car", "truck", "pedestrian"])
    f = s.sample_frame([0, 0, 2, 1])
    assert [c[3] for c in f] == [0, 0, 1, 1] and [c[2] for c in f] == [0, 0, 2, 2] and all(0 <= c[0] < 6 for c in f[:2]) and all(6 <= c[0] < 12 for c in f[2:])
    pts, off = s.bank_host()
    assert off[-1] == len(pts) == sum(len(i["points"]) for v in bank.values() for i in v) and s.n_obj == 12

    import det3d.datasets.pipelines.augmentation as al
    import det3d.datasets.pipelines.sample_ops as sl
    assert al.Rotation is A.Rotation and al.Flip is A.Flip and sl.DataBaseSamplerV2 is A.DataBaseSamplerV2

    L = _lib.lib()
    buf = (ctypes.c_char * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.pnx_paste_chunk_rows() == 2048
    sel = lambda **kw: L.pnx_paste_select(*[kw.get(k, d) for k, d in (("gt", p), ("cls", p), ("num", None), ("batch", 2), ("k", 4), ("d", 9), ("bank", p), ("cb", p),  # noqa: E731
                                                                     ("cc", p), ("cg", p), ("s", 8), ("groups", 2), ("off", p), ("n_obj", 3), ("acc", p), ("po", p),
                                                                     ("bo", p), ("co", p), ("no", p), ("pr", p), ("stream", None))])
    assert sel(k=500, s=13) == -2 and b"PNX_PASTE_MAX_BOXES" in L.pnx_last_error()        # the limit: refused before any launch
    assert sel(d=8) == -1 and b"box_dim" in L.pnx_last_error()
    assert sel(batch=65) == -1 and sel(cb=None) == -1 and b"candidate" in L.pnx_last_error()
    assert sel(groups=0) == -1 and sel(bo=None) == -1 and sel(gt=None) == -1
    assert L.pnx_paste_augment_workspace_bytes(300000, 4) > 0 and L.pnx_paste_augment_workspace_bytes(-1, 4) == 0
    pts_call = lambda **kw: L.pnx_paste_augment_points(*[kw.get(k, d) for k, d in (("pts", p), ("n", 10), ("f", 5), ("batch", 2), ("bank", None), ("cb", None),  # noqa: E731
                                                                                    ("po", None), ("pr", None), ("s", 0), ("d", 9), ("bp", None), ("off", None),
                                                                                    ("n_obj", 0), ("rows", 0), ("xf", None), ("out", p), ("cap", 10), ("no", p),
                                                                                    ("fr", p), ("ws", p), ("wsb", 16), ("stream", None))])
    assert pts_call() == -3 and b"workspace" in L.pnx_last_error()
    assert pts_call(f=2) == -1 and pts_call(pts=None) == -1 and pts_call(no=None) == -1 and pts_call(batch=0) == -1
    assert pts_call(bank=p, s=4, cb=p, po=p, pr=p, bp=None, off=p, n_obj=2) == -1 and b"bank" in L.pnx_last_error()
    assert L.pnx_augment_boxes(None, None, 2, 4, 9, p, None) == -1 and L.pnx_augment_boxes(p, None, 2, 4, 8, p, None) == -1
    assert L.pnx_augment_boxes(p, None, 2, 4, 9, None, None) == 0           # no transform: nothing to do, nothing launched
