"""GPU: the multi-sweep merge (csrc/merge.hip behind io.SweepMerger) against its exact twin (tests/merge_ref.py) at the seams of its kernels and at
scale, the contract of its output with the readers, and the ordering promise of io.PointUploader.

The comparison is always of the WHOLE (n_raw, n_copy + 2) buffer, pre-filled with a sentinel so that an unwritten row shows: bit-equal to the twin viewed
as uint32 (where the twin holds a NaN in a transformed column the kernel need only hold a NaN), n_out equal, a second run bit-identical.  The library is
built without contraction, so the kernel's coordinate is one fixed IEEE expression and nothing weaker than bit equality is asked.
tests/test_merge_ref_cpu.py holds the twin to the reference and states the planted cases as literal values."""
import merge_ref as M
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
POISON = 6.0221e23


def _bits(t):
    return t.contiguous().view(torch.int32)


def _merge(raw, segs, n_copy, merger=None, extra=3):
    """One device merge into a sentinel-filled buffer of `extra` more rows than needed.  Returns (the whole buffer, n_out) on the host."""
    from pillarnext_amd.io import SweepMerger

    out = torch.full((len(raw) + extra, n_copy + 2), SENTINEL, device="cuda")
    cnt = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    view, cnt2 = (merger or SweepMerger())(torch.from_numpy(raw).cuda(), segs, n_copy=n_copy, out=out, n_out=cnt)
    assert (len(raw) == 0 or view.data_ptr() == out.data_ptr()) and view.shape == (len(raw), n_copy + 2) and cnt2 is cnt
    return out.cpu().numpy(), int(cnt.item())


def _check(raw, segs, n_copy, what, merger=None, pair=None):
    """segs: the list form; pair: its descriptors() already on the device, handed to the merger in place of the list."""
    want, n_want = M.merge(raw, segs, n_copy)
    segs = segs if pair is None else pair
    got, n_got = _merge(raw, segs, n_copy, merger)
    assert n_got == n_want, (what, n_got, n_want)
    M.assert_same_bits(got[:len(raw)], want, what)
    assert (got[len(raw):] == SENTINEL).all(), f"{what}: rows beyond n_raw were written"
    again, n_again = _merge(raw, segs, n_copy, merger)
    assert n_again == n_got and np.array_equal(again.view(np.uint32), got.view(np.uint32)), f"{what}: the second run differs"
    return got, n_got


# ------------------------------------------------------------------------------------------------ row counts
@pytest.mark.parametrize("n", M.ROW_COUNTS)
def test_row_counts_through_the_scan_seams(n):
    """The vector and scalar tails of k_scan_local, one level-1 block, and one, two and three passes of the level-2 carry loop; whole blocks dropped, whole
    blocks kept, an alternating stretch and a block with only its first and last row kept (merge_ref.pattern_keep)."""
    raw, segs, keep = M.pattern_case(n, seed=n % 1000)
    nblk, passes = M.blocks_and_passes(n)
    print(f"[merge n={n}] {nblk} scan blocks, {passes} level-2 passes, {int(keep.sum())} rows kept")
    assert passes == {524_289: 2, 2 * 524_288 + 2049 + 5: 3}.get(n, 1) and nblk == -(-n // 2048)
    _, n_out = _check(raw, segs, 4, f"n={n}")
    assert n_out == int(keep.sum())
    if n >= 524_287:                                                                # a second pattern, shifted off the block grid
        raw, segs, keep = M.pattern_case(n, seed=7, shift=1031)
        assert _check(raw, segs, 4, f"n={n}, shifted")[1] == int(keep.sum())


# ------------------------------------------------------------------------------------------------ segments
@pytest.mark.parametrize("layout", list(M.segment_layouts()))
def test_segment_layouts(layout):
    """Distinct (batch, time) per segment make a row stamped by the wrong segment show; the batch index is not monotone."""
    segs, n = M.segments_from_lengths(M.segment_layouts()[layout])
    raw = M.close_rows(M.tagged_raw(n, seed=len(segs)))
    _, n_out = _check(raw, segs, 4, layout)
    assert 0 < n_out < n


def test_no_rows_and_one_empty_segment():
    got, n_out = _check(np.zeros((0, 4), np.float32), [dict(begin=0, end=0, batch=0, time=0.0, radius=1.0)], 4, "n_raw = 0")
    assert n_out == 0 and got.shape == (3, 6)                                       # _check: all three rows still hold the sentinel


# ------------------------------------------------------------------------------------------------ the radius
@pytest.mark.parametrize("r", [1.0, 0.5])
def test_radius_boundary_rows(r):
    raw, segs, kept = M.radius_case(r)
    got, n_out = _check(raw, segs, 4, f"radius {r}")
    assert n_out == int(kept.sum()) == 18
    assert np.array_equal(got[:n_out, 4], np.flatnonzero(kept).astype(np.float32))   # only rows with both coordinates strictly inside are gone; NaN rows stay


def test_value_that_rounds_up_to_the_radius_is_kept():
    raw, segs, kept = M.rounds_up_to_radius_case()
    got, n_out = _check(raw, segs, 4, "fp64 under r, fp32 equal to r")
    assert n_out == 1 and got[0].tolist() == [3.0, 1.0, 0.0, 0.0, 7.0, 0.5]


def test_all_rows_dropped_and_no_row_dropped():
    rng = np.random.default_rng(5)
    raw = np.zeros((4100, 4), np.float32)
    raw[:, :3] = rng.uniform(-0.4, 0.4, (4100, 3))
    raw[:, 3] = np.arange(4100)
    segs = [dict(begin=0, end=2048, batch=0, time=0.0, radius=0.5, transform=None), dict(begin=2048, end=4100, batch=1, time=0.25, radius=0.5, transform=np.eye(4))]
    got, n_out = _check(raw, segs, 4, "all dropped")
    assert n_out == 0 and (got[:4100, 0] == -1).all() and not got[:4100, 1:].view(np.uint32).any()     # the whole buffer is tail
    for s in segs:
        s["radius"] = 0.25
    raw[:, 0] += np.float32(0.75)
    assert _check(raw, segs, 4, "none dropped")[1] == 4100


# ------------------------------------------------------------------------------------------------ layouts
def test_strides_and_copied_columns():
    """raw_stride 3 .. 8 with n_copy 3 .. raw_stride; the columns beyond n_copy hold a poison value that must not appear in the output."""
    rng = np.random.default_rng(8)
    n = 2049 + 7
    T = np.eye(4)
    T[:2, :2] = [[np.cos(0.2), -np.sin(0.2)], [np.sin(0.2), np.cos(0.2)]]
    T[:3, 3] = [0.1, -0.2, 0.3]
    segs = [dict(begin=0, end=1000, batch=1, time=0.5, radius=0.0, transform=None), dict(begin=1000, end=1000, batch=5, time=5.0),
            dict(begin=1000, end=n, batch=0, time=0.25, radius=1.0, transform=T)]
    for stride in range(3, 9):
        raw = rng.uniform(-30, 30, (n, stride)).astype(np.float32)
        raw[1000::3, :3] *= np.float32(0.01)
        for n_copy in range(3, stride + 1):
            r = raw.copy()
            r[:, n_copy:] = POISON
            got, n_out = _check(r, segs, n_copy, f"stride {stride}, n_copy {n_copy}")
            assert 1000 < n_out < n and not (got == np.float32(POISON)).any()


# ------------------------------------------------------------------------------------------------ transforms
def test_transforms_that_cancel_a_zero_row_signed_zeros_and_subnormals():
    rng = np.random.default_rng(9)
    Ts = M.waymo_like_transforms()
    zero_row = Ts[1].copy()
    zero_row[1, :] = 0.0                                                            # y' = +0 for every row: inside any radius
    n_per = 3000
    raw = np.empty((6 * n_per, 4), np.float32)
    raw[:, :2] = rng.uniform(-75, 75, (len(raw), 2))
    raw[:, 2] = rng.uniform(-3, 5, len(raw))
    raw[:, 3] = np.arange(len(raw))
    special = np.array([-0.0, 0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.1754942e-38, 1.17549435e-38, 3e38, -3e38], np.float32)
    for k in range(6):                                                               # the same special rows in every segment, with and without a transform
        o = k * n_per
        raw[o:o + 10, 0], raw[o + 10:o + 20, 1], raw[o + 20:o + 30, 2] = special, special, special
        raw[o + 30:o + 40, :3] = special[:, None]
    trs = [None, Ts[0], Ts[1], Ts[2], Ts[3], zero_row]
    for k in (2, 4):                                                                 # rows whose IMAGES lie around the radius box: 1e4 m cancel to less than 1 m
        target = np.column_stack([rng.uniform(-1.5, 1.5, (200, 2)), rng.uniform(-3, 5, 200), np.ones(200)])
        raw[k * n_per + 100:k * n_per + 300, :3] = (np.linalg.inv(trs[k]) @ target.T).T[:, :3]
    segs = [dict(begin=k * n_per, end=(k + 1) * n_per, batch=k % 2, time=0.1 * k, radius=(0.0, 0.0, 1.0, 0.0, 1.0, 1.0)[k], transform=trs[k]) for k in range(6)]
    got, n_out = _check(raw, segs, 4, "cancelling transforms")
    assert 4 * n_per < n_out < 6 * n_per
    first = got[:n_per]                                                              # no transform, no radius: the three columns pass through bit for bit
    assert np.array_equal(first[:, 1:4].view(np.uint32), raw[:n_per, :3].view(np.uint32))
    ident = [dict(begin=0, end=len(raw), batch=0, time=0.0, radius=0.0, transform=np.eye(4))]
    _check(raw, ident, 4, "identity over signed zeros and subnormals")
    _check(raw, [dict(ident[0], transform=np.diag([2.0 ** -20, -(2.0 ** -126), 2.0 ** 100, 1.0]))], 4, "results that land in the subnormal range and overflow")


# ------------------------------------------------------------------------------------------------ workspace, out= and n_out= reused
def test_one_merger_reused_across_sizes():
    """600 000 rows, then 3000, then 600 000 rows of another keep pattern through one SweepMerger, one out= buffer and one n_out= tensor, as bench.py does:
    every call equals the twin and leaves the rows of `out` beyond its n alone."""
    from pillarnext_amd.io import SweepMerger

    m = SweepMerger()
    out = torch.full((600_000 + 5, 6), SENTINEL, device="cuda")
    cnt = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    expect = np.full((600_005, 6), SENTINEL, np.float32)
    for n, seed, shift in ((600_000, 1, 0), (3000, 2, 0), (600_000, 3, 517)):
        raw, segs, keep = M.pattern_case(n, seed=seed, shift=shift)
        want, n_want = M.merge(raw, segs, 4)
        view, _ = m(torch.from_numpy(raw).cuda(), segs, n_copy=4, out=out, n_out=cnt)
        assert view.shape == (n, 6) and int(cnt.item()) == n_want == int(keep.sum())
        expect[:n] = want
        M.assert_same_bits(out.cpu().numpy(), expect, f"reuse n={n}")


def test_descriptor_pair_equals_the_list_form():
    from pillarnext_amd.io import SweepMerger

    segs, n = M.segments_from_lengths(M.segment_layouts()["1000 seeded"])
    raw = M.close_rows(M.tagged_raw(n, seed=3))
    m = SweepMerger()
    pair = m.descriptors(segs, torch.device("cuda"))
    assert isinstance(pair, tuple) and pair[1] == 1000
    a, na = _check(raw, segs, 4, "list form", merger=m)
    for k in range(2):
        b, nb = _check(raw, segs, 4, f"pair form, use {k}", merger=m, pair=pair)
        assert nb == na and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------ the contract with the readers
@pytest.fixture(scope="module")
def merged_batch():
    """Two samples of 5 sweeps with the close-point radius on, merged on the device: (whole buffer, its first n_out rows as a tensor of their own, n_out)."""
    from pillarnext_amd.io import SweepMerger

    raw, segs = M.segments_of(M.contract_batch())
    out, cnt = SweepMerger()(torch.from_numpy(raw).cuda(), segs, n_copy=4)
    n_out = int(cnt.item())
    want, n_want = M.merge(raw, segs, 4)
    assert n_out == n_want and 0 < len(raw) - n_out                                  # a non-empty tail
    M.assert_same_bits(out.cpu().numpy(), want, "contract batch")
    return out, out[:n_out].clone(), n_out


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), what


def test_whole_buffer_feeds_the_fused_reader(merged_batch):
    """PillarFeatureNet.forward_dense on all n rows and on the first n_out: canvas, occupancy and counts bit-identical (the tail carries batch index -1)."""
    from pillarnext_amd import synth
    from test_gpu_reader import make_net

    whole, head, n_out = merged_batch
    cfg = synth.CONFIGS["C1"]
    net = make_net(cfg["pc_range"], cfg["voxel_size"], synth.pfn_params())
    ny, nx = (int(v) for v in net.grid_size)
    res = []
    for pts in (whole, head):
        occ = torch.full((2, ny, nx), 7, dtype=torch.uint8, device="cuda")
        counts = torch.full((2,), -3, dtype=torch.int32, device="cuda")
        res.append((net.forward_dense(pts, 2, occupancy=occ, counts=counts), occ, counts))
    for a, b, what in zip(res[0], res[1], ("canvas", "occupancy", "counts")):
        _same(a, b, what)
    P, kept = res[0][2].tolist()
    assert 0 < P <= kept <= n_out and int(res[0][1].sum()) == P and int((res[0][0] != 0).any(1).sum()) <= P


def test_whole_buffer_feeds_voxelize(merged_batch):
    from pillarnext_amd import ops, synth
    from pillarnext_amd._lib import make_geom

    whole, head, n_out = merged_batch
    cfg = synth.CONFIGS["C1"]
    geom = make_geom(cfg["pc_range"], cfg["voxel_size"])
    res = []
    for pts in (whole, head):
        n = pts.shape[0]
        feats = torch.full((n, pts.shape[1] + 4), SENTINEL, device="cuda")
        coords = torch.full((n, 3), -9, dtype=torch.int32, device="cuda")
        inv = torch.full((n,), -9, dtype=torch.int64, device="cuda")
        pop = torch.full((n,), -9, dtype=torch.int32, device="cuda")
        counts = torch.full((2,), -3, dtype=torch.int32, device="cuda")
        ops.voxelize(pts, 2, geom, ops.Workspace(), features=feats, coords=coords, unq_inv=inv, pillar_of_point=pop, counts=counts)
        P, m = counts.tolist()
        res.append((counts, feats[:m], coords[:P], inv[:m], pop[:n_out], pop[n_out:]))
    for a, b, what in zip(res[0][:5], res[1][:5], ("counts", "features", "coords", "unq_inv", "pillar_of_point")):
        _same(a, b, what)
    P, m = res[0][0].tolist()
    assert bool((res[0][5] == -1).all()) and res[0][5].numel() == whole.shape[0] - n_out and 0 < P <= m <= n_out


@pytest.mark.parametrize("mode", ["voxel", "pillar_clamp", "cylinder_clamp"])
def test_whole_buffer_feeds_group_points(merged_batch, mode):
    from pillarnext_amd import ops
    from pillarnext_amd._lib import PNX_GROUP_CYLINDER_CLAMP, PNX_GROUP_PILLAR_CLAMP, PNX_GROUP_VOXEL

    whole, head, n_out = merged_batch
    pr = [-38.4, -38.4, -3.0, 38.4, 38.4, 1.0]
    geom = {"voxel": lambda: ops.group_geom(pr, [0.2, 0.2, 0.5], PNX_GROUP_VOXEL),
            "pillar_clamp": lambda: ops.group_geom(pr, [0.4, 0.4, 4.0], PNX_GROUP_PILLAR_CLAMP),
            "cylinder_clamp": lambda: ops.group_geom([-180, -3.0, 0, 180, 1.0, 57.0], [0.5625, 0.5, 57.0], PNX_GROUP_CYLINDER_CLAMP)}[mode]()
    a = ops.group_points(whole, 2, geom, want_mean=True)
    b = ops.group_points(head, 2, geom, want_mean=True)
    assert (a["G"], a["Nk"]) == (b["G"], b["Nk"]) and 0 < a["G"] <= a["Nk"] <= n_out and (mode == "voxel" or a["Nk"] == n_out)
    for k in ("features", "coords", "unq_inv", "mean"):
        _same(a[k], b[k], f"{mode}: {k}")


# ------------------------------------------------------------------------------------------------ PointUploader
def _elapsed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def test_uploader_does_not_overwrite_a_slot_that_is_still_read():
    """depth 2: batch A is uploaded; the compute stream is given a delay followed by a clone of A's device view; B and C follow, C into A's slot.  The
    clone must hold A: the copy of C has to wait for the readers of A.  The delay is device work measured once with events and made at least ten times
    the H2D copy of one batch (and at least 20 ms), so that a copy that did not wait would have landed long before the clone ran."""
    from pillarnext_amd.io import PointUploader

    n, rng = 100_000, np.random.default_rng(21)
    A, B, C = (np.ascontiguousarray(rng.standard_normal((n, 6)), np.float32) + np.float32(10 * k) for k in range(3))
    pinned, devbuf = torch.from_numpy(A).pin_memory(), torch.empty((n, 6), device="cuda")
    devbuf.copy_(pinned, non_blocking=True)                                          # warm-up
    copy_ms = _elapsed_ms(lambda: devbuf.copy_(pinned, non_blocking=True))
    work = torch.zeros(16 << 20, device="cuda")                                      # 64 MiB: one pass reads and writes 128 MiB
    work.add_(1.0)
    unit_ms = _elapsed_ms(lambda: [work.add_(1.0) for _ in range(8)]) / 8
    reps = int(np.ceil(max(10 * copy_ms, 20.0) / unit_ms)) + 1
    delay_ms = reps * unit_ms
    print(f"[uploader] H2D copy of one batch {copy_ms:.3f} ms, delay {reps} x {unit_ms:.3f} ms = {delay_ms:.1f} ms")
    assert delay_ms >= 10 * copy_ms and delay_ms < 100.0, (copy_ms, unit_ms, reps)

    up = PointUploader(n, 5, "cuda", depth=2)
    a_dev = up.upload_rows(A)
    for _ in range(reps):
        work.add_(1.0)
    snap = a_dev.clone()
    b_dev = up.upload_rows(B)
    c_dev = up.upload_rows(C)
    assert c_dev.data_ptr() == a_dev.data_ptr() != b_dev.data_ptr()                  # C reuses A's slot
    torch.cuda.synchronize()
    assert np.array_equal(snap.cpu().numpy().view(np.uint32), A.view(np.uint32)), "the slot of batch A was overwritten while it was still being read"
    assert np.array_equal(b_dev.cpu().numpy().view(np.uint32), B.view(np.uint32)) and np.array_equal(c_dev.cpu().numpy().view(np.uint32), C.view(np.uint32))


def test_upload_rows_and_upload_round_trip():
    from pillarnext_amd.io import PointUploader

    rng = np.random.default_rng(22)
    up = PointUploader(5000, 5, "cuda", depth=2)
    for n in (5000, 1, 0, 4097, 5000):                                               # more calls than slots, sizes below the capacity
        rows = rng.standard_normal((n, 6)).astype(np.float32)
        rows[: n // 2, 0] = -0.0
        dev = up.upload_rows(rows)
        assert dev.shape == (n, 6) and np.array_equal(dev.cpu().numpy().view(np.uint32), rows.view(np.uint32))
    clouds = [rng.standard_normal((k, 5)).astype(np.float32) for k in (1200, 0, 7)]
    dev, B = up.upload(clouds)
    want = np.concatenate([np.column_stack([np.full(len(c), b, np.float32), c]) for b, c in enumerate(clouds)])
    assert B == 3 and np.array_equal(dev.cpu().numpy().view(np.uint32), want.view(np.uint32))
