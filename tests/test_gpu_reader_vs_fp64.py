"""GPU: the inference reader (chunk_sort.hip -> k_span_carve -> pfn_spans.hip -> k_pfn3_tail, and the binned pipeline reader_bins.h +
pfn_v3.hip behind it) against the fp64 reference of tests/reader_fp64_ref.py, path by path, at small shapes.

test_gpu_reader.py holds the reader to |d| <= 1e-4 + 1e-4 |ref| against an fp32 oracle: about a thousand times the error the kernels
claim.  Here every case (a) ASSERTS on the host, from the input and the constants of spans.h, that it takes the path it is there for,
and (b) holds feat_max to bars derived from the kernels' stated arithmetic.  The reference reproduces the fp32 steps of the reference
module bit for bit (cell index, range mask, mean, x - mean, x - centre), so the decorated features are the kernels' own inputs and what
is measured is the PFN: fold, layer 0, max, concat, layer 1, max.

The per-element bar (u = 2^-24, the fp32 unit roundoff; t1, t01, w1_l1, x_l1 as reader_fp64_ref.py returns them; F point features):

    |got - ref| <= u * (A1 * t1 + (F + 11) * t01) + 2^-30 * w1_l1[c] + 2^-33 * x_l1[p]

  fold (k_fold_bn)    a = fl(fl(1 / fl(sqrt(fl(var + eps)))) * gamma), W' = fl(W a): five roundings (the square root halves the one under
                      it), relative error <= 5 u of every W'; shift = fl(beta - fl(mean a)): <= 5 u (|beta| + |mean a|).  Both layers:
                      5 u of the layer's sum of |terms|.
  layer 0             v_mfma_f32_32x32x2_f32 over K = F + 5 features + the constant-1 column of the shift: a sum of F + 6 fp32 terms,
                      in any order <= (F + 6) u sum|terms|.  With the fold (F + 11) u * T0 per channel; the power-of-two pre-scale 2^SU,
                      ReLU and the pillar max are exact and 1-Lipschitz, so the same bound holds for the max half of the concat with the
                      pillar's largest T0.
  through |W1'|       layer 1 is linear: sum_k |W1'[c,k]| * (F + 11) u T0x[k] = (F + 11) u * t01.
  fp16 split          x * 2^SU -> hi (RTZ, 11 bits) + lo (RTZ of the exact remainder, 11 more bits): |x - hi - lo| < 2^-21 |x| = 8 u;
                      W1' * 2^SW -> hi (RNE) + lo (RNE of the exact remainder): <= 2^-22 = 4 u.  12 u * t1.  Where lo falls below the
                      smallest fp16 subnormal the error is absolute: 2^-24 / 2^SU = 2^-30 per x (times |W1'|: 2^-30 w1_l1), half of it
                      / 2^SW = 2^-33 per W1' (times x: 2^-33 x_l1).
  dropped lo*lo       |lo_w| <= 2^-11 |w|, |lo_x| < 2^-10 |x|: 2^-21 = 8 u * t1.
  accumulation        3 x 64 exact fp16 x fp16 products and the pre-scaled shift, summed in fp32 by 24 v_mfma_f32_32x32x16_f16 (whose
                      inner order is not documented: any order of 193 terms, every partial sum rounded no worse than fp32 RNE) <= 192 u * t1.
  un-scale and ReLU   * 2^-(SU+SW) exact; the shift rides in the accumulator: its addition is one of the 192.  1 u for the fold's shift
                      rounding counted separately above.
  A1 = 5 + 12 + 8 + 192 + 1 = 218 for the fp16x3 form.  The fp32 forms (k_pfn3_tail, the big-pillar walk, PNX_PFN_F16X3=0) run layer 1 as
  64 + 1 fp32 terms on the unscaled weights: A1_32 = 5 + 64 + 1 = 70, and no absolute floors; pillars that take them (more than 32
  points, or a layer-0 maximum beyond the fp16 range) are ALSO held to that tighter bar.
  These are worst-case bounds: every rounding at its maximum with the same sign.  Random roundings come out near the square root of
  the counts; a dropped cross product (2^-12 of a term, ~300 u of t1 after 64 terms of random sign) does not.

(b) Frobenius: ||got - ref||_F / ||ref||_F over all pillars of a case is at most 2 x that of the fp32 statement of the same PFN on the
same decorated features (oracle.pfn_eval: the C oracle's layers, fp32 throughout, sequential sums) -- the margin test_gpu_sparse3d_grad.py
gives a kernel over its torch statement.  The statement gets the reference's decorated features, not its own fp32 running-sum means, so
that its error is the PFN's alone and a fat pillar does not loosen the bar.  Measured per case AND over the pillars of the fp32 forms alone.
(c) Signed mean: |mean(got - ref)| <= mean(bar), what (a) implies; reported.

16-bit canvases: bit-exact feat_max rounded once (RNE) at the cells of `coords`, bit-zero elsewhere, and a Frobenius error against fp64
of at most 1.25 x that of the fp64 reference rounded once (the project's figure for 16-bit stores).

Paths.  F = 6 is served by the binned pipeline whatever PNX_READER_IMPL says, as are PNX_PFN_F16X3=0 and grids of more than 32 768 slabs
per frame (reader.hip).  The LDS record slots of k_span_pfn (`cap` of launch_spans) cannot be reached from Python; _lds_slots restates
span_pfn_lds_bytes for the default 80 000-byte budget, and the `segments` case asserts against that; should the restatement drift, the
spans_seg form (PNX_BINS_CAP=96) still forces several segments per span on the cases marked with it.  The reader's own counters (head of
its workspace: kCntBig, kCntOvf16, kCntSpill, kCntRows of spans.h) are read after a rank-output call as confirmation.

Measured on one MI355X: see the CHANGELOG entry of this module."""
import functools

import numpy as np
import pytest

import reader_fp64_ref as R
from test_gpu_reader import make_net

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U = 2.0 ** -24
A1_F16X3, A1_FP32 = 218, 70
FRO_RATIO = 2.0
FRO16 = 1.25
H16_LIMIT = 937.5            # 60000 / 2^SU: the range test of pfn_spans.hip / pfn_v3.hip on the pre-scaled pillar maximum
# spans.h
K_SLAB_SHIFT, K_SPAN_MAX_SLABS, K_SPAN_PILLARS, K_CHUNK, K_SPAN_QUOTA = 9, 16, 512, 2048, 640
K_CNT_BIG, K_CNT_OVF16, K_CNT_SPILL, K_CNT_ROWS = 3, 4, 6, 7

C1 = dict(pc_range=(-51.2, -51.2, -5.0, 51.2, 51.2, 3.0), voxel_size=(0.2, 0.2, 8.0))
GEOMS = {
    "g100x155": dict(pc_range=(-20.0, -31.0, -5.0, 20.0, 31.0, 3.0), voxel_size=(0.4, 0.4, 8.0)),   # unaligned pitch, cut last slab
    "g336": dict(pc_range=(-50.4, -50.4, -5.0, 50.4, 50.4, 3.0), voxel_size=(0.3, 0.3, 8.0)),
    "goffset": dict(pc_range=(0.0, -40.0, -3.0, 70.4, 40.0, 1.0), voxel_size=(0.2, 0.2, 4.0)),      # x - mean, x - centre cancel at x ~ 70
}
WIDE = dict(pc_range=(-51.25, -51.25, -5.0, 51.25, 51.25, 3.0), voxel_size=(0.025, 0.025, 8.0))     # 4100 x 4100: 32 833 slabs per frame


# ------------------------------------------------------------------------------------------------ the paths, restated on the host
def _lds_slots(pack, B):
    """Usable padded points of one segment of k_span_pfn: span_pfn_lds_bytes (pfn_spans.hip) at the default budget, minus the class slack."""
    S, bit_words, rec_w, slack = K_SPAN_PILLARS, K_SPAN_MAX_SLABS * (1 << K_SLAB_SHIFT) // 32, 8, 6 * 32
    head = (2 * (S + 4) + 3 * S) * 4 + 3 * S * 8 + 2 * bit_words * 4 + (48 + 4 * 24 + 64) * 4 + 3 * ((B + 1 + 3) & ~3) * 4
    wave_out = (32 * 36 if pack else 32 * 68) + 64
    return (80000 - head - 4 * wave_out * 4) // (rec_w * 4) - slack


def span_plan(r, n_rows, B):
    """chunk_sort.hip's chunks and k_span_carve's spans from the reference's pillar set."""
    gy, gx = (int(v) for v in r["grid"])
    nf = (gx * gy + (1 << K_SLAB_SHIFT) - 1) >> K_SLAB_SHIFT
    co = r["coords"].astype(np.int64)
    pslab = co[:, 0] * nf + ((co[:, 1] * gx + co[:, 2]) >> K_SLAB_SHIFT)         # frame-major slab of every pillar
    cnt = r["counts"]
    tot = np.bincount(pslab, weights=cnt, minlength=B * nf).astype(np.int64).reshape(B, nf)
    span_of_slab = np.empty((B, nf), np.int64)
    base = 0
    for b in range(B):
        T = tot[b]
        p = np.cumsum(T) - T                                                   # points of the frame in front of slab s
        tp = np.concatenate([[0], T[:-1]])
        s = np.arange(nf)
        cut = (s == 0) | (s % K_SPAN_MAX_SLABS == 0) | (p // K_SPAN_QUOTA != (p - tp) // K_SPAN_QUOTA)
        span_of_slab[b] = base + np.cumsum(cut) - 1
        base = span_of_slab[b, -1] + 1
    pspan = span_of_slab.reshape(-1)[pslab]
    padded = np.where(cnt <= 32, 1 << np.ceil(np.log2(np.maximum(cnt, 1))).astype(np.int64), 0)
    chunk = r["kept"] // K_CHUNK
    frame = co[r["unq_inv"], 0]
    pairs = len(np.unique(chunk * B + frame))
    return dict(nf=nf, pillars=np.bincount(pspan, minlength=base), points=np.bincount(pspan, weights=cnt, minlength=base).astype(np.int64),
                padded=np.bincount(pspan, weights=padded, minlength=base).astype(np.int64),
                nchunks=(n_rows + K_CHUNK - 1) // K_CHUNK, ovf_rows=pairs - len(np.unique(chunk)),
                frames_per_chunk=np.bincount(np.unique(chunk * B + frame) // B))


# ------------------------------------------------------------------------------------------------ the cases
def _in_cells(rng, xi, yi, geom, b, F=5, z=(-2.0, 1.0)):
    """One point in each of the cells (xi, yi), well inside the cell."""
    n = len(xi)
    p = np.empty((n, 1 + F), np.float32)
    p[:, 0] = b
    p[:, 1] = geom["pc_range"][0] + (xi + rng.uniform(0.1, 0.9, n)) * geom["voxel_size"][0]
    p[:, 2] = geom["pc_range"][1] + (yi + rng.uniform(0.1, 0.9, n)) * geom["voxel_size"][1]
    p[:, 3] = rng.uniform(z[0], z[1], n)
    p[:, 4:] = rng.uniform(0, 1, (n, F - 3))
    return p


def _sweep(geom, B, n, seed):
    from pillarnext_amd import synth

    return np.concatenate([synth.push_outside(synth.sweep_cloud(n, geom["pc_range"], seed + b, batch_idx=b), geom["pc_range"], 0.015, 7 + b)
                           for b in range(B)])


def _case_classes():
    """Pillars of every count 1..40 at least 20 times (all six size classes, both sides of every boundary, 33..40 spill to the tail), a
    few of 200 and of 3 000 points, on a thin uniform background; B = 2."""
    from pillarnext_amd import synth

    rng = np.random.default_rng(11)
    B, frames = 2, []
    for b in range(B):
        sizes = np.concatenate([np.repeat(np.arange(1, 41), 13), [200, 200, 200, 3000]])
        cells = rng.choice(512 * 512, len(sizes), replace=False)
        xi, yi = np.repeat(cells % 512, sizes), np.repeat(cells // 512, sizes)
        f = np.concatenate([_in_cells(rng, xi, yi, C1, b), synth.uniform_cloud(2500, C1["pc_range"], 300 + b, batch_idx=b)])
        frames.append(f[rng.permutation(len(f))])
    pts = np.concatenate(frames)

    def path(r, plan):
        occ = np.bincount(r["counts"], minlength=41)
        assert (occ[1:41] >= 20).all(), occ[1:41]
        assert (r["counts"] == 200).sum() >= 4 and (r["counts"] >= 3000).sum() >= 2
    return pts, B, C1, 5, path


def _case_slices():
    """About one point per occupied cell at a density at which the carve gives spans of more than kSpanPillars pillars."""
    rng = np.random.default_rng(12)
    n = 30_000
    pts = _in_cells(rng, rng.integers(0, 512, n), rng.integers(0, 512, n), C1, 0)

    def path(r, plan):
        assert plan["pillars"].max() > K_SPAN_PILLARS and (plan["pillars"] > K_SPAN_PILLARS).sum() >= 10, plan["pillars"].max()
        assert r["counts"].mean() < 1.2
    return pts, 1, C1, 5, path


def _case_segments():
    """A sweep cloud plus a block of 16 x 32 cells with ~20 points per cell: spans whose padded points exceed the LDS record slots."""
    rng = np.random.default_rng(13)
    xi, yi = np.meshgrid(np.arange(300, 332), np.arange(200, 216))           # 32 cells along a slab (a canvas row), 16 slabs
    per = rng.integers(17, 24, xi.size)
    blk = _in_cells(rng, np.repeat(xi.ravel(), per), np.repeat(yi.ravel(), per), C1, 0)
    f0 = np.concatenate([_sweep(C1, 1, 12_000, 50), blk])
    f1 = _sweep(C1, 1, 8_000, 60)
    f1[:, 0] = 1
    pts = np.concatenate([f0[rng.permutation(len(f0))], f1])

    def path(r, plan):
        assert plan["padded"].max() > _lds_slots(True, 2) > _lds_slots(False, 2), (plan["padded"].max(), _lds_slots(True, 2))
        assert (plan["padded"] > _lds_slots(True, 2)).sum() >= 4
    return pts, 2, C1, 5, path


def _case_frames(B, empty=None):
    """Rows of all frames interleaved: every chunk of 2048 rows holds every (non-empty) frame and needs an overflow row for each but one:
    B = 3 uses the whole pool (ovf_cap = nchunks * (B - 1))."""
    live = [b for b in range(B) if b != empty]
    fr = [_sweep(C1, 1, 6_000, 70 + b) for b in live]
    pts = np.stack(fr, axis=1).reshape(-1, 6).copy()                          # rows 0, 1, 2, 0, 1, 2, ... of the live frames
    pts[:, 0] = np.tile(np.array(live, np.float32), len(fr[0]))

    def path(r, plan):
        assert (plan["frames_per_chunk"] == len(live)).all() and plan["ovf_rows"] == plan["nchunks"] * (len(live) - 1)
        if empty is None:
            assert plan["ovf_rows"] == plan["nchunks"] * (B - 1)              # the pool's worst case
        else:
            assert not (r["coords"][:, 0] == empty).any()
    return pts, B, C1, 5, path


def _case_range():
    """The intensity of whole pillars scaled so that the layer-0 pillar maximum lies in [600, 937), in [937, 2000), or far beyond."""
    from pillarnext_amd import synth

    rng = np.random.default_rng(15)
    pts = _sweep(C1, 2, 10_000, 80)
    layers = synth.pfn_params(5, (64, 64), seed=0)
    v = R.voxelize(pts, C1["pc_range"], C1["voxel_size"])
    feat, cnt = R.decorate(pts, v)
    W0, s0, _ = R.fold64(layers[0])
    small = np.flatnonzero((cnt >= 1) & (cnt <= 12))
    pick = rng.choice(small, 240, replace=False)
    target = np.concatenate([rng.uniform(640, 900, 90), rng.uniform(1000, 1900, 90), np.full(60, np.inf)])
    pos = W0[:, 3] > 0
    for p, T in zip(pick, target):
        rows = np.flatnonzero(v["unq_inv"] == p)
        if np.isinf(T):
            pts[v["kept"][rows], 4] = 1.0e4
            continue
        f = feat[rows].astype(np.float64)
        f[:, 3] = 0
        base = f @ W0.T + s0                                                  # layer 0 without the intensity: h0 = base + W0'[:, 3] I
        pts[v["kept"][rows], 4] = np.float32(((T - base[:, pos]) / W0[pos, 3]).min())

    def path(r, plan):
        m = r["h0max"].max(1)
        assert ((m >= 600) & (m < 937)).sum() >= 50 and ((m >= 937) & (m < 2000)).sum() >= 50 and (m > 3000).sum() >= 30
        assert not (np.abs(m - H16_LIMIT) < 2e-3 * H16_LIMIT).any() and not (np.abs(m - 937) < 1e-3 * 937).any()
    return pts, 2, C1, 5, path


def _case_features(F):
    rng = np.random.default_rng(F)
    base = _sweep(C1, 2, 7_500, 90 + F)
    pts = np.concatenate([base[:, :4], rng.uniform(0, 1, (len(base), 3)).astype(np.float32)], axis=1)[:, : 1 + F].copy()
    return pts, 2, C1, F, lambda r, plan: None


def _case_grid(name):
    g = GEOMS[name]

    def path(r, plan):
        gy, gx = (int(v) for v in r["grid"])
        if name == "g100x155":
            assert (gx, gy) == (100, 155) and (gx * gy) % 512 != 0 and gx % 16 != 0
            last = (r["coords"][:, 1].astype(np.int64) * gx + r["coords"][:, 2]) >> K_SLAB_SHIFT == plan["nf"] - 1
            assert last.any()                                                 # pillars in the cut last slab of a frame
        if name == "goffset":
            assert np.abs(r["features"][:, 0]).max() > 65 and np.abs(r["features"][:, [5, 6, 8, 9]]).max() < 0.21
    pts = _sweep(g, 2, 8_000, 100)
    if name == "g100x155":  # the sweep does not reach the far rows: a few pillars in the cut last slab (cells 15 360 .. 15 499) of frame 1
        rng = np.random.default_rng(16)
        cell = rng.integers(15_360, 15_500, 300)
        pts = np.concatenate([pts, _in_cells(rng, cell % 100, cell // 100, g, 1)])
    return pts, 2, g, 5, path


BUILDERS = {
    "classes": _case_classes, "slices": _case_slices, "segments": _case_segments,
    "frames_b3": lambda: _case_frames(3), "frames_b4_gap": lambda: _case_frames(4, empty=2), "range": _case_range,
    "features_f3": lambda: _case_features(3), "features_f4": lambda: _case_features(4), "features_f5": lambda: _case_features(5),
    "features_f6": lambda: _case_features(6),
    "grid_100x155": lambda: _case_grid("g100x155"), "grid_336": lambda: _case_grid("g336"), "grid_offset": lambda: _case_grid("goffset"),
}
SEG_CASES = ("classes", "segments", "frames_b3", "frames_b4_gap")               # the cases that also run as spans_seg
CASE_PARAMS = [(c, i) for c in BUILDERS for i in (("spans", "spans_seg", "binned") if c in SEG_CASES else ("spans", "binned"))]


@functools.lru_cache(maxsize=None)
def build_case(name):
    """Input, fp64 reference and fp32 statement of a case, computed once and shared; the path assertions run here, before any compare."""
    from oracle import oracle as O
    from pillarnext_amd import synth

    pts, B, geom, F, path = BUILDERS[name]()
    pts = np.ascontiguousarray(pts, np.float32)
    assert 15_000 <= len(pts) <= 60_000 and pts.shape[1] == 1 + F, pts.shape
    layers = synth.pfn_params(F, (64, 64), seed=0 if F == 5 else F)
    r = R.reader_forward(pts, geom["pc_range"], geom["voxel_size"], layers)
    plan = span_plan(r, len(pts), B)
    path(r, plan)
    O.build()
    stmt = O.pfn_eval(r["features"], r["unq_inv"], r["P"], [64, 64], layers)    # fp32 throughout, on the reference's decorated features
    fp32_form = (r["counts"] > 32) | (r["h0max"].max(1) >= H16_LIMIT)            # pillars the spans / binned kernels hand to fp32 MFMA
    for a in (pts, stmt, *[x for x in r.values() if isinstance(x, np.ndarray)]):
        a.setflags(write=False)
    return dict(name=name, pts=pts, B=B, geom=geom, F=F, layers=layers, ref=r, plan=plan, stmt=stmt, fp32_form=fp32_form)


def _set_impl(monkeypatch, impl):
    monkeypatch.setenv("PNX_READER_IMPL", "4" if impl.startswith("spans") else "2")
    if impl == "spans_seg":
        monkeypatch.setenv("PNX_BINS_CAP", "96")


def _fro(d, ref):
    return float(np.linalg.norm(d) / np.linalg.norm(ref))


def bars(c, a1):
    r = c["ref"]
    b = U * (a1 * r["t1"] + (c["F"] + 11) * r["t01"])
    if a1 == A1_F16X3:
        b = b + 2.0 ** -30 * r["w1_l1"][None, :] + 2.0 ** -33 * r["x_l1"][:, None]
    return b


def check_feat_max(tag, c, fm, all_fp32=False):
    """(a), (b), (c) of the module docstring on a (P, 64) fp32 feat_max; prints every figure before it asserts."""
    r = c["ref"]
    got = fm.astype(np.float64)
    assert got.shape == r["feat_max"].shape and np.isfinite(got).all()
    d = got - r["feat_max"]
    bar = bars(c, A1_FP32 if all_fp32 else A1_F16X3)
    f32 = np.ones(r["P"], bool) if all_fp32 else c["fp32_form"]
    worst = float((np.abs(d) / bar).max())
    worst32 = float((np.abs(d[f32]) / bars(c, A1_FP32)[f32]).max()) if f32.any() else 0.0
    fro, fro_s = _fro(d, r["feat_max"]), _fro(c["stmt"] - r["feat_max"], r["feat_max"])
    fro32 = _fro(d[f32], r["feat_max"][f32]) if f32.any() else 0.0
    fro32_s = _fro((c["stmt"] - r["feat_max"])[f32], r["feat_max"][f32]) if f32.any() else 1.0
    mean = float(d.mean())
    print(f"[reader vs fp64] {tag}: P={r['P']} worst|err|/bar {worst:.3f} (fp32-form pillars {int(f32.sum())}: {worst32:.3f} of the fp32 bar)  "
          f"Frobenius {fro:.3e} = {fro / fro_s:.2f} x fp32 statement ({fro_s:.3e}); fp32-form pillars {fro32 / fro32_s:.2f} x  "
          f"signed mean {mean:+.2e} (bar {float(bar.mean()):.2e}, {mean / float(bar.mean()):+.3f})")
    assert worst <= 1.0, (tag, "per element", worst)
    assert worst32 <= 1.0, (tag, "per element, fp32-form pillars", worst32)
    assert fro <= FRO_RATIO * fro_s, (tag, "Frobenius ratio to the fp32 statement", fro / fro_s)
    assert fro32 <= FRO_RATIO * fro32_s, (tag, "Frobenius ratio, fp32-form pillars", fro32 / fro32_s)
    assert abs(mean) <= float(bar.mean()), (tag, "signed mean", mean, float(bar.mean()))


def check_canvas(tag, c, canvas, fm_t, coords_t, dtype):
    """A (B, 64, ny, nx) canvas: feat_max rounded once at the cells of coords, bit-zero elsewhere, Frobenius against fp64."""
    r = c["ref"]
    ny, nx = (int(v) for v in r["grid"])
    assert canvas.shape == (c["B"], 64, ny, nx) and canvas.dtype == dtype
    nhwc = canvas.permute(0, 2, 3, 1)
    exp = torch.zeros((c["B"], ny, nx, 64), dtype=dtype, device="cuda")
    k = coords_t.long()
    exp[k[:, 0], k[:, 1], k[:, 2]] = fm_t.to(dtype)
    ibits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(nhwc.contiguous().view(ibits), exp.view(ibits)), (tag, "canvas bits")   # -0.0 would not pass as a zero either
    if dtype != torch.float32:
        got = nhwc[k[:, 0], k[:, 1], k[:, 2]].double().cpu().numpy()
        once = torch.from_numpy(r["feat_max"]).to(dtype).double().numpy()
        fro, fro1 = _fro(got - r["feat_max"], r["feat_max"]), _fro(once - r["feat_max"], r["feat_max"])
        print(f"[reader vs fp64] {tag}: {dtype} canvas Frobenius {fro:.3e} = {fro / fro1:.4f} x the reference rounded once")
        assert fro <= FRO16 * fro1, (tag, "16-bit Frobenius", fro / fro1)


def read_counters(net):
    torch.cuda.synchronize()
    return net._ws.buf[:256].view(torch.int32).cpu().numpy()


def check_counters(c, impl, cnt):
    """The reader's own counters confirm the host's restatement of the paths (span pipeline; the binned one lists whole tiles)."""
    r, plan = c["ref"], c["plan"]
    big = r["counts"] > 32
    ovf = ~big & (r["h0max"].max(1) >= H16_LIMIT)
    print(f"[reader vs fp64] {c['name']}/{impl}: counters big {cnt[K_CNT_BIG]} (host {int(big.sum())}) ovf16 {cnt[K_CNT_OVF16]} (host {int(ovf.sum())}) "
          f"spill {cnt[K_CNT_SPILL]} rows {cnt[K_CNT_ROWS]} (host {plan['ovf_rows']}); spans {len(plan['pillars'])}, most pillars "
          f"{int(plan['pillars'].max())}, most padded points {int(plan['padded'].max())}")
    if impl.startswith("spans") and c["F"] <= 5:
        assert cnt[K_CNT_BIG] == big.sum() and cnt[K_CNT_OVF16] == ovf.sum()
        assert cnt[K_CNT_SPILL] == r["counts"][big | ovf].sum() and cnt[K_CNT_ROWS] == plan["ovf_rows"]
    else:
        assert cnt[K_CNT_BIG] == big.sum() and cnt[K_CNT_OVF16] >= ovf.sum()


def run_rank(c):
    net = make_net(c["geom"]["pc_range"], c["geom"]["voxel_size"], c["layers"], F=c["F"])
    tp = torch.from_numpy(c["pts"]).cuda()
    fm, coords, grid = net(tp, c["B"])
    return net, tp, fm, coords


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("case,impl", CASE_PARAMS)
def test_case_vs_fp64(case, impl, monkeypatch):
    c = build_case(case)
    _set_impl(monkeypatch, impl)
    net, tp, fm, coords = run_rank(c)
    cnt = read_counters(net)
    assert np.array_equal(coords.cpu().numpy(), c["ref"]["coords"])
    assert np.array_equal(np.asarray(net.grid_size), c["ref"]["grid"])
    check_counters(c, impl, cnt)
    check_feat_max(f"{case}/{impl}", c, fm.cpu().numpy())
    for dtype in (torch.bfloat16, torch.float16):
        canvas = net.forward_dense(tp, c["B"], dtype=dtype, channels_last=True)
        assert canvas.is_contiguous(memory_format=torch.channels_last)
        check_canvas(f"{case}/{impl}", c, canvas, fm, coords, dtype)


def test_range_fp32_layer1(monkeypatch):
    """PNX_PFN_F16X3=0 under the binned pipeline: every pillar on fp32 MFMA, held to the fp32 bar and to the Frobenius ratio 2."""
    c = build_case("range")
    _set_impl(monkeypatch, "binned")
    monkeypatch.setenv("PNX_PFN_F16X3", "0")
    net, tp, fm, coords = run_rank(c)
    assert np.array_equal(coords.cpu().numpy(), c["ref"]["coords"])
    check_feat_max("range/binned/fp32 layer 1", c, fm.cpu().numpy(), all_fp32=True)
    canvas = net.forward_dense(tp, c["B"], dtype=torch.bfloat16)
    check_canvas("range/binned/fp32 layer 1", c, canvas, fm, coords, torch.bfloat16)


@pytest.mark.parametrize("impl", ["spans", "binned"])
def test_fp32_nchw_canvas(impl, monkeypatch):
    c = build_case("classes")
    _set_impl(monkeypatch, impl)
    net, tp, fm, coords = run_rank(c)
    canvas = net.forward_dense(tp, c["B"], dtype=torch.float32, channels_last=False)
    assert canvas.is_contiguous()
    check_canvas(f"classes/{impl}/fp32 nchw", c, canvas, fm, coords, torch.float32)
    k = coords.long()
    check_feat_max(f"classes/{impl}/fp32 nchw canvas", c, canvas.permute(0, 2, 3, 1)[k[:, 0], k[:, 1], k[:, 2]].cpu().numpy())


@pytest.mark.parametrize("case,impl", [("classes", "spans"), ("slices", "spans"), ("segments", "spans_seg"), ("frames_b3", "spans"),
                                       ("range", "spans"), ("range", "binned"), ("features_f4", "spans"), ("features_f6", "binned"),
                                       ("grid_100x155", "spans")])
def test_deterministic_and_order_free(case, impl, monkeypatch):
    """A second call and a call on a row permutation of the input: bit-identical feat_max and canvas."""
    c = build_case(case)
    _set_impl(monkeypatch, impl)
    net, tp, fm, coords = run_rank(c)
    fm, coords = fm.clone(), coords.clone()
    canvas = net.forward_dense(tp, c["B"]).clone()
    perm = torch.randperm(tp.shape[0], device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    for t in (tp, tp[perm].contiguous()):
        fm2, coords2, _ = net(t, c["B"])
        assert torch.equal(coords, coords2) and torch.equal(fm.view(torch.int32), fm2.view(torch.int32))
        assert torch.equal(canvas.view(torch.int16), net.forward_dense(t, c["B"]).view(torch.int16))


@functools.lru_cache(maxsize=None)
def _wide_case():
    from oracle import oracle as O
    from pillarnext_amd import synth

    rng = np.random.default_rng(17)
    n = 20_000
    pts = _in_cells(rng, rng.integers(0, 4100, n), rng.integers(0, 4100, n), WIDE, 0)
    pts[:2000, 1:3] = pts[:200, 1:3].repeat(10, 0) + rng.uniform(-0.004, 0.004, (2000, 2)).astype(np.float32)   # some shared cells
    layers = synth.pfn_params(5, (64, 64), seed=0)
    r = R.reader_forward(pts, WIDE["pc_range"], WIDE["voxel_size"], layers)
    plan = span_plan(r, n, 1)
    assert tuple(r["grid"]) == (4100, 4100) and 32768 < plan["nf"] <= 32768 + 128       # a little beyond the span tables
    co = r["coords"].astype(np.int64)
    assert ((co[:, 1] * 4100 + co[:, 2]) >> K_SLAB_SHIFT).max() >= 32768 and r["counts"].max() >= 4
    O.build()
    stmt = O.pfn_eval(r["features"], r["unq_inv"], r["P"], [64, 64], layers)
    return dict(name="wide", pts=pts, B=1, geom=WIDE, F=5, layers=layers, ref=r, plan=plan, stmt=stmt,
                fp32_form=(r["counts"] > 32) | (r["h0max"].max(1) >= H16_LIMIT))


@pytest.mark.parametrize("impl", ["spans", "binned"])
def test_wide_grid_hands_over(impl, monkeypatch):
    """A little more than 32 768 slabs per frame: beyond the span tables, the reader hands the call to the binned pipeline.  Rank outputs
    only (the canvas of this grid is 2 GB)."""
    c = _wide_case()
    _set_impl(monkeypatch, impl)
    net, tp, fm, coords = run_rank(c)
    assert np.array_equal(coords.cpu().numpy(), c["ref"]["coords"])
    check_feat_max(f"wide/{impl}", c, fm.cpu().numpy())
