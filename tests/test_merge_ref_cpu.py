"""CPU: the exact twin of the device merge (tests/merge_ref.py) against the numpy restatement of the reference (oracle.merge_sweeps) and, through the
golden file, against the reference's own output; the planted seam cases of tests/test_gpu_merge_seams.py stated as literal values; and the host-side
checks of io.pack_segments / io.SweepMerger.

Bars.  Batch, copied and time columns: bit-equal.  Kept rows: the same, in the same order.  Coordinates: <= 1 ulp of fp32, because the reference's
`T.dot(...)` is a BLAS dgemm that may fuse or reorder the four terms, each variant being the correctly rounded fp32 of an fp64 value that differs from
the twin's by a few fp64 ulp -- the two fp32 results are equal or neighbours.  At most 0.1 % of the coordinates may differ at all (the bar of the tests this
twin replaces; a condition, not a measurement: the inputs here meet it with 0 differing).  The kept sets can be compared only where no |x'|, |y'| lies within
2 ulp of the radius: that count is asserted to be 0, never masked."""
import merge_ref as M
import numpy as np
import pytest
from test_merge_golden import _nusc_sweeps, _waymo_sweeps

from conftest import load_golden


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _against(ref, sweeps, what, ref_cols=slice(0, None)):
    """twin of `sweeps` against ref (rows of [batch, x, y, z, copied.., time], or a column subset of it for the recorded reference output)."""
    raw, segs = M.segments_of(sweeps)
    assert M.near_radius(raw, segs) == 0, f"{what}: a coordinate within 2 ulp of the radius -- choose another seed"
    out, n_out = M.merge(raw, segs, 4)
    got = out[:n_out, ref_cols]
    assert n_out == len(ref) and got.shape == ref.shape, (what, n_out, ref.shape)
    xyz = slice(1, 4) if ref.shape[1] == 6 else slice(0, 3)
    rest = [c for c in range(ref.shape[1]) if not xyz.start <= c < xyz.stop]
    assert np.array_equal(_bits(got[:, rest]), _bits(ref[:, rest])), what          # the same rows in the same order: column 3 of the inputs differs per row
    d = M.ulp_distance(got[:, xyz], ref[:, xyz])
    differ = int((d != 0).sum())
    print(f"[{what}] {n_out} of {len(raw)} rows kept, {differ} of {d.size} coordinates differ, max {int(d.max()) if d.size else 0} ulp")
    assert int(d.max()) <= 1, what
    assert differ <= 0.001 * d.size, what
    assert np.array_equal(_bits(out[n_out:, 1:]), np.zeros((len(raw) - n_out, 5), np.uint32)) and bool((out[n_out:, 0] == -1).all())


@pytest.mark.parametrize("ds", ["nusc", "waymo"])
def test_twin_equals_oracle_and_recorded_reference(oracle, ds):
    g = load_golden("merge_sweeps")
    sweeps = _nusc_sweeps(g, batch=1) if ds == "nusc" else _waymo_sweeps(g, batch=1)
    _against(oracle.merge_sweeps(sweeps, n_copy=4), sweeps, f"{ds}: twin vs oracle")
    _against(g[f"{ds}_points"], sweeps, f"{ds}: twin vs recorded reference", ref_cols=slice(1, None))


def test_twin_equals_oracle_on_a_nuscenes_sized_batch(oracle):
    sweeps = M.nuscenes_batch()
    n = sum(len(s["points"]) for s in sweeps)
    assert n == 531_060 and M.blocks_and_passes(n) == (260, 2)
    _against(oracle.merge_sweeps(sweeps, n_copy=4), sweeps, "4 x 10 sweeps: twin vs oracle")


def test_twin_equals_oracle_on_the_reader_contract_batch(oracle):
    sweeps = M.contract_batch()
    _against(oracle.merge_sweeps(sweeps, n_copy=4), sweeps, "2 x 5 sweeps: twin vs oracle")


# ------------------------------------------------------------------------------------------------ planted cases, from first principles
def test_transform_is_the_stated_expression():
    """One row by hand: exact binary fractions, so every product and sum is exact and the result is known without running any implementation."""
    T = np.array([[0.5, -2.0, 0.25, 3.0], [1.0, 0.0, 0.0, -1.0], [0.0, 0.0, 0.0, 0.0]])
    got = M.transform_rows(T, np.array([[2.0, 0.75, -4.0]], np.float32))
    assert got.dtype == np.float32 and got.tolist() == [[0.5 * 2 - 2 * 0.75 + 0.25 * -4 + 3, 1.0, 0.0]] == [[1.5, 1.0, 0.0]]
    # order of summation: ((a + b) + c) + d with a = 2^60, b = -2^60, c = 1, d = 2^-30 gives 1 + 2^-30 -> fp32 1.0; any order that adds c or d to a first loses it
    T = np.array([[2.0 ** 60, -2.0 ** 60, 1.0, 2.0 ** -30], [0, 0, 0, 0], [0, 0, 0, 0]])
    assert M.transform_rows(T, np.array([[1.0, 1.0, 1.0]], np.float32))[0, 0] == 1.0
    # fp64 products, not fp32: (1 + 2^-23)^2 = 1 + 2^-22 + 2^-46 rounds UP past the tie to 1 + 2^-22 + 2^-23 from fp64; an fp32 product rounds the tie to even
    T = np.array([[1.0 + 2.0 ** -23, 0, 0, 2.0 ** -24], [0, 0, 0, 0], [0, 0, 0, 0]])
    x = np.float32(1.0 + 2.0 ** -23)
    assert float(M.transform_rows(T, np.array([[x, 0, 0]], np.float32))[0, 0]) == 1.0 + 2.0 ** -22 + 2.0 ** -23


@pytest.mark.parametrize("r", [1.0, 0.5])
def test_radius_cases_as_literal_values(r):
    raw, segs, kept = M.radius_case(r)
    xy, k1 = M.radius_rows(r)
    p = float(M.prev32(r))
    assert p < r and np.float32(p) == M.prev32(r) and len(xy) == 15
    # only rows with BOTH coordinates strictly inside are dropped; NaN fails the comparison; -0.0 is inside
    assert k1.tolist() == [True] * 4 + [False] * 4 + [True, False, True, True, True, False, True]
    out, n_out = M.merge(raw, segs, 3)
    assert n_out == int(kept.sum()) == 18 and out.shape == (30, 5)
    ident = raw[:15, :3].copy()                                  # through the identity, 0 * NaN and 0 * inf turn the other coordinates of a row into NaN
    ident[10], ident[11], ident[12] = np.nan, np.nan, [np.inf, np.nan, np.nan]
    want = np.concatenate([np.column_stack([np.full(9, b, np.float32), xyz[k1], np.full(9, t, np.float32)]) for b, xyz, t in ((0, ident, 0.0), (1, raw[15:, :3], 1.0))])
    M.assert_same_bits(out[:18], want, f"radius {r}")
    assert np.isnan(out[5, 1]) and np.isnan(out[6, 2]) and np.isinf(out[7, 1]) and np.isinf(out[16, 1]) and out[16, 2] == 0
    assert out[18:].tolist() == [[-1.0, 0.0, 0.0, 0.0, 0.0]] * 12 and not np.signbit(out[18:, 1:]).any()


def test_value_that_rounds_up_to_the_radius_is_kept():
    raw, segs, kept = M.rounds_up_to_radius_case()
    t = segs[0]["transform"][0, 3]
    assert 0.5 + t == 1.0 - 2.0 ** -26 < 1.0 and np.float32(0.5 + t) == np.float32(1.0)                  # under r in fp64, exactly r in fp32
    assert float(raw[1, 0]) + t == 1.0 - 2.0 ** -24 - 2.0 ** -26 and np.float32(float(raw[1, 0]) + t) == np.float32(1.0 - 2.0 ** -24)
    out, n_out = M.merge(raw, segs, 4)
    assert n_out == 1 and kept.tolist() == [True, False]
    assert out.tolist() == [[3.0, 1.0, 0.0, 0.0, 7.0, 0.5], [-1.0, 0.0, 0.0, 0.0, 0.0, 0.0]]


def test_all_dropped_none_dropped_and_empty():
    raw = np.zeros((5, 3), np.float32)
    raw[:, 2] = 9.0
    out, n_out = M.merge(raw, [dict(begin=0, end=5, batch=2, time=1.5, radius=0.5)], 3)
    assert n_out == 0 and out.tolist() == [[-1.0, 0.0, 0.0, 0.0, 0.0]] * 5
    out, n_out = M.merge(raw, [dict(begin=0, end=5, batch=2, time=1.5, radius=0.0)], 3)                  # n_copy == raw_stride == 3
    assert n_out == 5 and out.tolist() == [[2.0, 0.0, 0.0, 9.0, 1.5]] * 5
    out, n_out = M.merge(np.zeros((0, 4), np.float32), [dict(begin=0, end=0, batch=0, time=0.0)], 4)
    assert n_out == 0 and out.shape == (0, 6)


def test_columns_beyond_n_copy_are_ignored_and_empty_segments_stamp_nothing():
    raw = np.arange(24, dtype=np.float32).reshape(4, 6)
    segs = [dict(begin=0, end=0, batch=9, time=9.0), dict(begin=0, end=1, batch=1, time=0.25), dict(begin=1, end=1, batch=8, time=8.0),
            dict(begin=1, end=1, batch=7, time=7.0), dict(begin=1, end=4, batch=0, time=0.5), dict(begin=4, end=4, batch=6, time=6.0)]
    out, n_out = M.merge(raw, segs, 4)
    assert n_out == 4 and out.tolist() == [[1, 0, 1, 2, 3, 0.25], [0, 6, 7, 8, 9, 0.5], [0, 12, 13, 14, 15, 0.5], [0, 18, 19, 20, 21, 0.5]]


@pytest.mark.parametrize("n", M.ROW_COUNTS)
def test_pattern_cases_drop_what_they_plant(n):
    """The keep pattern of the row-count tests is what the twin computes from the planted coordinates, and it holds the block kinds the test promises."""
    raw, segs, keep = M.pattern_case(n, seed=n % 1000)
    out, n_out = M.merge(raw, segs, 4)
    assert n_out == int(keep.sum()) and np.array_equal(out[:n_out, 4], raw[keep, 3]) and M.near_radius(raw, segs) == 0
    assert not (out[:n_out] == 12345.0).any()
    nblk, passes = M.blocks_and_passes(n)
    assert passes == (1 if n <= 524_288 else 2 if n <= 2 * 524_288 else 3)
    if nblk >= 8:
        per = [keep[b * 2048:(b + 1) * 2048] for b in range(7)]
        assert not per[1].any() and per[2].all() and per[3].tolist() == [False, True] * 1024
        assert np.flatnonzero(per[4]).tolist() == [0, 2047] and np.flatnonzero(per[5]).tolist() == [1000] and 800 < per[0].sum() < 1250


def test_segment_layouts_of_the_gpu_test_are_well_formed():
    from pillarnext_amd.io import check_segments

    for lengths in M.segment_layouts().values():
        segs, n = M.segments_from_lengths(lengths)
        check_segments(segs, n)
    lengths = M.segment_layouts()["1000 seeded"]
    segs, n = M.segments_from_lengths(lengths)
    assert len(lengths) == 1000 and min(lengths) == 0 and max(lengths) == 300 and len({(s["batch"], s["time"]) for s in segs}) == 1000
    assert [s["batch"] for s in segs[:9]] == [0, 1, 2, 3, 4, 5, 6, 0, 1]                                   # not monotone
    ends = np.cumsum(M.segment_layouts()["every residue"])
    assert set(ends % 256) == set(range(256)) and set(ends % 2048) == set(range(2048))
    # a row stamped by a neighbouring segment shows: the twin's (batch, time) per kept row is that of the segment holding the row's tag
    raw = M.close_rows(M.tagged_raw(n, 5))
    out, n_out = M.merge(raw, segs, 4)
    seg_of_row = np.repeat(np.arange(1000), lengths)[out[:n_out, 4].astype(np.int64)]
    assert 0 < n_out < n and np.array_equal(out[:n_out, 0], (seg_of_row % 7).astype(np.float32)) and np.array_equal(out[:n_out, 5], (0.25 * seg_of_row).astype(np.float32))


def test_waymo_like_transforms_cancel_to_tens_of_metres():
    for T in M.waymo_like_transforms():
        assert 5.0 < np.linalg.norm(T[:3, 3]) < 100.0 and np.abs(T[:3, :3]).min() > 1e-4 and np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-9)


# ------------------------------------------------------------------------------------------------ host checks
def _segs(*pairs):
    return [dict(begin=b, end=e, batch=0, time=0.0) for b, e in pairs]


def test_pack_segments_refuses_tables_that_do_not_tile_the_rows():
    from pillarnext_amd.io import SweepMerger, check_segments, pack_segments

    good = _segs((0, 0), (0, 5), (5, 5), (5, 9))
    assert len(pack_segments(good)) == 4 * 128 and check_segments(good, 9) is None
    for bad, word in ((_segs((1, 5)), "row 0"), (_segs((0, 5), (6, 9)), "gap"), (_segs((0, 5), (4, 9)), "overlap"), (_segs((0, 5), (5, 3)), "begin")):
        with pytest.raises(ValueError, match=word):
            pack_segments(bad)
        with pytest.raises(ValueError, match=word):
            SweepMerger().descriptors(bad, "cpu")
    with pytest.raises(ValueError, match="9 rows"):
        check_segments(_segs((0, 5)), 9)                                                                 # the last sweep forgotten
    assert pack_segments([]) == b""


def test_sweep_merger_checks_before_it_calls_the_library(monkeypatch):
    torch = pytest.importorskip("torch")
    from pillarnext_amd import _lib
    from pillarnext_amd.io import SweepMerger

    def boom():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", boom)
    raw = torch.zeros((9, 5))
    m = SweepMerger()
    for n_copy in (2, 6, 0, -1):
        with pytest.raises(ValueError, match="n_copy"):
            m(raw, _segs((0, 9)), n_copy=n_copy)
    with pytest.raises(ValueError, match="9 rows"):
        m(raw, _segs((0, 5)), n_copy=4)
    with pytest.raises(ValueError, match="9 rows"):
        m(raw, _segs((0, 5), (5, 10)), n_copy=4)
    with pytest.raises(ValueError, match="gap"):
        m(raw, _segs((0, 5), (6, 9)), n_copy=4)
    with pytest.raises(AssertionError, match="library was reached"):                                     # a good call gets as far as the library
        m(raw, _segs((0, 5), (5, 9)), n_copy=5)


def test_existing_loaders_satisfy_the_checks():
    from pillarnext_amd import synth
    from pillarnext_amd.io import check_segments

    raw, segs = synth.raw_sweeps(synth.make_batch("C1", 2, "sweep", n=5_000))
    check_segments(segs, len(raw))
    assert len(segs) > 2
