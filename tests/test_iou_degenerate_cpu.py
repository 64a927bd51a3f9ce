"""CPU: the rotated-IoU host twins (csrc/iou3d_geom.h compiled for the host) on the degenerate pair families of tests/iou_cases.py, against
  * the oracle's deterministic-math variant: bit for bit, NaN / inf fields included;
  * the compiled reference's results in tests/golden/iou_degenerate.npz (oracle/gen_golden.py degenerate; re-derived bit for bit where oracle/_ref
    exists) THROUGH true geometry (tests/iou_exact_ref.py): per pair |host - exact| <= |ref - exact| + tol, tol = 1e-5 (the project's allowance between
    libm and the deterministic transcendentals) unless the family's recorded max |host - ref| exceeds 5e-6, then twice that recorded value;
  * the far_apart early-out, which only the kernels and the twins have: every pair it rejects has reference IoU exactly 0."""
import numpy as np
import pytest

import iou_cases as C
import iou_exact_ref as X
from conftest import load_golden
from iou_cases import same_bits

NAMES = list(C.FAMILIES)


@pytest.fixture(scope="module")
def g():
    return load_golden("iou_degenerate")


def test_fixture_holds_the_families(g, oracle):
    assert list(g["dev_names"]) == NAMES
    for name in NAMES:
        a, b = C.family(name)
        assert np.all(same_bits(g[name + "_a"], a)) and np.all(same_bits(g[name + "_b"], b)), name
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (256 if name in C.FILL_A_BLOCK else 64, 7)
        if name != "nan_inf_fields":
            assert not (a[:, 3:6] < 0).any() and not (b[:, 3:6] < 0).any()                              # negative sizes are left out
        if oracle.have_ref():
            assert np.all(same_bits(oracle.ref_boxes_aligned_iou_bev(a, b), g[name + "_ref_iou"])), name
            assert np.all(same_bits(oracle.ref_boxes_iou_bev(a[:17], b[:19]), g[name + "_ref_nm"])), name


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_equals_oracle_det(g, oracle, name):
    a, b = g[name + "_a"], g[name + "_b"]
    assert np.all(same_bits(C.host_aligned_iou(a, b), oracle.boxes_aligned_iou_bev(a, b, "det")))
    for n, m in ((17, 19), (17, 1), (1, 19)):
        assert np.all(same_bits(C.host_iou(a[:n], b[:m]), oracle.boxes_iou_bev(a[:n], b[:m], "det")))


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_no_further_from_true_geometry_than_the_reference(g, name):
    a, b, ref = g[name + "_a"], g[name + "_b"], g[name + "_ref_iou"].astype(np.float64)
    host = C.host_aligned_iou(a, b).astype(np.float64)
    exact = X.aligned(a, b)[1]
    i = NAMES.index(name)
    row = X.deviations(ref, host, exact)
    np.testing.assert_allclose(row[:2], [g["dev_ref_exact_max"][i], g["dev_share_gt1"][i]], rtol=1e-6, atol=1e-12)     # the table of DESIGN section 3
    recorded = float(g["dev_host_ref_max"][i])
    tol = 1e-5 if recorded <= 5e-6 else 2 * recorded
    assert row[2] <= tol
    ok = np.isfinite(exact)
    assert np.array_equal(np.isnan(host[~ok]), np.isnan(ref[~ok]))                  # a non-finite field: NaN where the reference has NaN
    fin = ~ok & np.isfinite(ref)
    assert np.all(np.abs(host[fin] - ref[fin]) <= tol)
    assert np.all(np.abs(host[ok] - exact[ok]) <= np.abs(ref[ok] - exact[ok]) + tol), name


def test_tiny_heading_family_fills_the_polygon_scratch(g, oracle):
    cnt = oracle.overlap_vertex_count(g["tiny_heading_a"], g["tiny_heading_b"])
    assert cnt.max() == 16, "more than 16 vertices: the kernel's scratch would drop one"
    assert (cnt == 16).mean() >= 0.9
    for name in NAMES:                                                              # no family goes past the capacity
        assert oracle.overlap_vertex_count(g[name + "_a"], g[name + "_b"]).max() <= 16, name


def test_far_apart_rejects_only_pairs_the_reference_scores_zero(g, oracle):
    rejected = 0
    for name in NAMES:
        a, b = g[name + "_a"], g[name + "_b"]
        al = np.diag(C.far_apart(a, b))
        nm = C.far_apart(a[:17], b[:19])
        assert np.all(g[name + "_ref_iou"][al] == 0) and np.all(g[name + "_ref_nm"][nm] == 0), name
        assert np.all(C.host_aligned_iou(a, b)[al] == 0)
        rejected += int(al.sum() + nm.sum())
    assert rejected > 3000
    # pairs right at the early-out's edge: a box against a copy moved out along a random direction to where the predicate flips
    rng = np.random.default_rng(9)
    a, _ = C.random(256, 9)
    b, _ = C.random(256, 10)
    phi = rng.uniform(-np.pi, np.pi, 256)
    r2 = (np.sqrt((a[:, 3] / 2) ** 2 + (a[:, 4] / 2) ** 2) + np.sqrt((b[:, 3] / 2) ** 2 + (b[:, 4] / 2) ** 2)) * 1.001 + 0.1
    for scale in (0.999, 1.0, 1.0001, 1.001):
        b[:, 0] = a[:, 0] + (scale * r2 * np.cos(phi)).astype(np.float32)
        b[:, 1] = a[:, 1] + (scale * r2 * np.sin(phi)).astype(np.float32)
        far = np.diag(C.far_apart(a, b))
        assert np.all(oracle.boxes_aligned_iou_bev(a, b, "libm")[far] == 0)          # the libm variant is pinned to the compiled reference bit for bit
        assert np.all(same_bits(C.host_aligned_iou(a, b), oracle.boxes_aligned_iou_bev(a, b, "det")))
    assert far.any()


def test_far_apart_needs_its_slack(g, oracle):
    """zone_of_slack: centres beyond the touching of the bare bounding circles (1.001 x half diagonal), inside the + 0.05 ones.  The reference's 1e-2
    in-box margin collects corners there: most pairs have a non-zero reference IoU, the early-out must let every one of them through, and the twin
    equals the oracle (which has no early-out) on bits."""
    a, b, ref = g["zone_of_slack_a"], g["zone_of_slack_b"], g["zone_of_slack_ref_iou"]
    dist = np.hypot(a[:, 0].astype(np.float64) - b[:, 0], a[:, 1].astype(np.float64) - b[:, 1])
    assert np.all(dist > C.bare_radius(a) + C.bare_radius(b) + 4e-4)            # the bare circles do not touch ...
    assert np.all(dist < C.bare_radius(a) + C.bare_radius(b) + 7e-3)            # ... and the inflated ones overlap by far
    assert not np.diag(C.far_apart(a, b)).any()
    assert (ref != 0).mean() > 0.5 and ref.max() > 10
    host = C.host_aligned_iou(a, b)
    assert np.all(same_bits(host, oracle.boxes_aligned_iou_bev(a, b, "det")))
    assert (host != 0).mean() > 0.5
    nm = C.far_apart(a[:17], b[:19])
    assert np.all(g["zone_of_slack_ref_nm"][nm] == 0)


def test_huge_headings_give_zero(oracle):
    a, b = C.huge_heading()
    assert np.array_equal(C.host_aligned_iou(a, b), [0.0, 0.0]) and np.array_equal(oracle.boxes_aligned_iou_bev(a, b, "det"), [0.0, 0.0])


def test_exact_cases(g, oracle):
    """heading +-0.0 with dyadic sizes: every operation is exact, overlap dx/2 * dy, IoU fp32(1/3) on every implementation, the reference included."""
    a, b = g["zero_heading_dyadic_a"], g["zero_heading_dyadic_b"]
    third = (np.float32(1) / np.float32(3))
    assert np.all(C.host_aligned_iou(a, b) == third) and np.all(g["zero_heading_dyadic_ref_iou"] == third)
    assert np.all(oracle.boxes_aligned_overlap_bev(a, b, "det") == a[:, 3] / 2 * a[:, 4])
    ch = C.chain(200)
    assert np.all(C.host_aligned_iou(ch[:-1], ch[1:]).view(np.uint32) == 0x3EAAAAAB)
    # along y at the fp32 nearest pi/2 the cosine is -4.4e-8, not 0: corners are rounded at the spacing of their coordinate (1.5e-5 at 200 m), two of
    # them move the overlap of 1.0 by <= 6e-5 and the IoU (slope 4/9 there) by <= 3e-5 -- the neighbours' IoU falls on either side of fp32(1/3)
    ch = C.chain(200, along_y=True)
    iou_y = oracle.boxes_aligned_iou_bev(ch[:-1], ch[1:], "det")
    assert np.abs(iou_y - third).max() < 3e-5 and (iou_y > third).any() and (iou_y == third).any()
    a, b = C.block16()
    assert (oracle.overlap_vertex_count(np.repeat(a, 16, 0), np.tile(b, (16, 1))) == 16).all()


NMS_KEYS = [f"chain_{c}_{t}" for c in ("x", "x130", "y") for t in ("lo", "at", "hi")] + ["spread_neg", "dense_t020", "dense_t070", "dense_t090", "bad_rows",
                                                                                        "identical_list", "tiny_heading_list"]


@pytest.mark.parametrize("key", NMS_KEYS)
def test_nms_lists_oracle_equals_recorded_reference(g, oracle, key):
    boxes, thr, keep = g[f"nms_{key}_boxes"], float(g[f"nms_{key}_thr"]), g[f"nms_{key}_keep"]
    assert np.array_equal(oracle.nms_rotated(boxes, thr, "det"), keep)
    if oracle.have_ref():
        assert np.array_equal(oracle.ref_nms_rotated(boxes, thr), keep)
    if key.startswith("chain_x"):
        assert len(keep) == ((len(boxes) + 1) // 2 if key.endswith("lo") else len(boxes))      # 100 / 200 / 200 of 200: strict >
    if key.startswith("dense"):
        assert np.array_equal(boxes, C.dense_cluster(int(g[f"nms_{key}_seed"])))
        assert 0 < float(g[f"nms_{key}_margin"]) < 1e-4                                         # recorded: how close the closest pair is to the threshold
        if oracle.have_ref():
            iu = np.triu_indices(len(boxes), 1)
            assert np.abs(oracle.ref_boxes_iou_bev(boxes, boxes)[iu] - np.float32(thr)).min() == g[f"nms_{key}_margin"]
    if key == "spread_neg":
        assert keep.tolist() == [0] and np.array_equal(boxes, C.spread_130())
    if key == "bad_rows":
        assert set(g["nms_bad_rows_which"].tolist()) <= set(keep.tolist())                     # a NaN / inf box is never suppressed
