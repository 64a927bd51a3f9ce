"""GPU: the fused training reader (csrc/pfn_train.hip behind pnx_pfn_forward_train / pnx_pfn_backward, driven by pillarnext_amd/pfn_train.py)
against the fp64 twin of tests/pfn_train_ref.py: batch statistics, feat_max and the six parameter gradients of ONE training step.

test_gpu_reader.py holds this path to rtol = atol = 2e-3 on three fixtures of ~3 000 points with F = 5 (a wave of the 2 048 then walks 0-2
records and never carries a sum from one pillar to the next) and to 1e-3 against the torch path at full size.  Here every case first ASSERTS on
the host that it takes the path it is there for (pfn_train_ref.wave_split restates k_pfn_train's work split; the assertions run when the case is
built) and then holds every quantity to the bars the twin derives from the kernel's operation order, 2^-16 of the sum of |terms| at the most:

  many            ~40 000 points, 2 frames, 128 x 128 cells: ~20 records and >= 5 pillars per wave, one pillar of 600 points -- acc[], s1, s2
                  carried across pillars, the taken / taken0 resets and dg0 per pillar
  fat             one pillar with 62 % of 20 000 records, mid-rank: >= 1 000 waves with r0 == r1, exactly one wave owns the pillar
  few_*           700 points (one per pillar: 1 348 waves walk nothing); 1 point; one pillar of 3 000 points and nothing else: fewer records than
                  waves, the w == 0 and w + 1 == nw branches
  frames          B = 3, the middle frame empty, points outside the range, batch indices -1 and B: N' < n in every statistic
  features_f3..6  C0 = 8, 9, 10, 11: launch_train<C0>, the parameter block offset TP::W0, rec_f up to k = 10, the [32][C0 + 2] partial layout
  offset_*        a layer-0 pre-activation at mean / std = 30 exactly (the masked-BN precedent); a 1 m crop at x ~ 50 m (mean / std > 100);
                  gamma0 small against beta0, so that u = [h0 | g0] sits at mean / std >= 30: the batch VARIANCES under 2^-16 * 2 var
  planted         exact duplicates inside pillars (ties at the maximum of both layers), a channel whose every maximum is exactly 0
  unique          10 000 points, one per pillar

The setup: PillarFeatureNet(...).train() through its public forward with PNX_TRAIN_FUSED=1, momentum 1 and zero running statistics, so that
running_mean / running_var ARE the batch statistics (the variance times N'/(N' - 1)); random parameters with negative gammas, a zero gamma and a
closed channel per layer (pfn_train_ref.make_params); the upstream gradient zero on the fragile layer-1 decisions, the fragile layer-0 decisions
allowed for as the twin's docstring derives.  Every ordinary case also prints the relative Frobenius error of each gradient against fp64 for the
fused path and for PNX_TRAIN_FUSED=0 (torch fp32 on the same inputs) and their ratio: a measurement, not asserted.

Empty batch (n = 0, and every point outside the range): no error, feat_max (0, 64), coords (0, 3), the backward of the empty gradient gives
exactly-zero parameter gradients, nothing turns NaN.  BatchNorm1d itself raises on fewer than two rows, so the reference gives no answer for the
running statistics; the fused path treats the batch as one of mean 0 and variance 0 with N' clamped to 1 (as the masked BatchNorm node does with no
active site): running_mean and running_var move towards 0 by the momentum, num_batches_tracked counts the step.

Measured on one MI355X: see the CHANGELOG entry of this module."""
import functools

import numpy as np
import pytest

import pfn_train_ref as T

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GRADS = ("dW0", "dgamma0", "dbeta0", "dW1", "dgamma1", "dbeta1")
TINY = 1e-300


def make_net(c):
    from pillarnext_amd.reader import PillarFeatureNet

    net = PillarFeatureNet(c["F"], [64, 64], list(c["geom"]["voxel_size"]), list(c["geom"]["pc_range"])).cuda()
    with torch.no_grad():
        for i, pfn in enumerate(net.pfn_layers):
            pfn.linear.weight.copy_(torch.from_numpy(np.array(c["prm"][f"W{i}"])))
            pfn.norm.weight.copy_(torch.from_numpy(np.array(c["prm"][f"gamma{i}"])))
            pfn.norm.bias.copy_(torch.from_numpy(np.array(c["prm"][f"beta{i}"])))
            pfn.norm.running_mean.zero_()
            pfn.norm.running_var.zero_()
            pfn.norm.momentum = 1.0
    return net.train()


def run_step(c, fused=True):
    """One training step; everything as float64 numpy.  The environment switch is read at every forward."""
    import os

    old = os.environ.get("PNX_TRAIN_FUSED")
    os.environ["PNX_TRAIN_FUSED"] = "1" if fused else "0"
    try:
        net = make_net(c)
        fm, coords, grid = net(torch.from_numpy(np.array(c["pts"])).cuda(), c["B"])
        assert (type(fm.grad_fn).__name__ == "FusedPFNTrainBackward") == fused, type(fm.grad_fn).__name__
        fm.backward(torch.from_numpy(np.array(c["ref"]["G"])).cuda())
        torch.cuda.synchronize()
    finally:
        if old is None:
            del os.environ["PNX_TRAIN_FUSED"]
        else:
            os.environ["PNX_TRAIN_FUSED"] = old
    out = dict(feat_max=fm.detach(), coords=coords, grid=np.asarray(grid))
    for i, pfn in enumerate(net.pfn_layers):
        out[f"dW{i}"], out[f"dgamma{i}"], out[f"dbeta{i}"] = pfn.linear.weight.grad, pfn.norm.weight.grad, pfn.norm.bias.grad
        out[f"rm{i}"], out[f"rv{i}"] = pfn.norm.running_mean, pfn.norm.running_var
        assert int(pfn.norm.num_batches_tracked) == 1
    return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def _fro(got, ref):
    return float(np.linalg.norm(got.astype(np.float64) - ref) / max(np.linalg.norm(ref), TINY))


def ratios(c, got):
    """worst |err| / bar of every held quantity (the fp32 rounding of a stored value on top of the statistics' bars)"""
    s = c["ref"]
    w = {"feat_max": float((np.abs(got["feat_max"] - s["feat_max"]) / (s["feat_max_bar"] + TINY)).max())}
    for i in (0, 1):
        rm, rv, brm, brv = T.running(s[f"mu{i}"], s[f"var{i}"], s["N"], inp=s["stat1_in"] if i else (0.0, 0.0))
        w[f"mean{i}"] = float((np.abs(got[f"rm{i}"] - rm) / (brm + T.U * np.abs(rm) + TINY)).max())
        w[f"var{i}"] = float((np.abs(got[f"rv{i}"] - rv) / (brv + T.U * np.abs(rv) + TINY)).max())
    for k in GRADS:
        w[k] = float((np.abs(got[k] - s[k]) / (s[k + "_bar"] + TINY)).max())
    return w


@functools.lru_cache(maxsize=None)
def fused_step(name):
    return run_step(T.case(name), True)


@pytest.mark.parametrize("name", T.CASES)
def test_case_vs_fp64(name):
    c = T.case(name)                # the path assertions of the case run in here, on the host
    s = c["ref"]
    got = fused_step(name)
    assert np.array_equal(got["coords"], s["coords"]) and np.array_equal(got["grid"], s["grid"])
    assert got["feat_max"].shape == (s["P"], 64) and all(np.isfinite(got[k]).all() for k in got if k != "coords")
    w = ratios(c, got)
    frag, masked, positive = T.conditions(s)
    print(f"[pfn train vs fp64] {name}: N'={s['N']} P={s['P']} F={c['F']} fragile0 {100 * frag:.4f} % masked {100 * masked:.2f} % positive {100 * positive:.0f} %  "
          "worst |err| / bar " + " ".join(f"{k} {v:.3f}" for k, v in w.items()))
    if name not in T.OFFSET and s["N"] > 1:      # Frobenius against fp64, fused and torch fp32 on the same inputs: measured, not asserted
        ref = run_step(c, False)
        assert np.array_equal(ref["coords"], s["coords"])
        print(f"[pfn train vs fp64] {name}: relative Frobenius error, fused / torch fp32 (ratio) "
              + " ".join(f"{k} {_fro(got[k], s[k]):.1e} / {_fro(ref[k], s[k]):.1e} ({_fro(got[k], s[k]) / max(_fro(ref[k], s[k]), TINY):.2f})"
                         for k in ("feat_max",) + GRADS if np.linalg.norm(s[k]) > 0))
    bad = {k: v for k, v in w.items() if v > 1.0}
    assert not bad, (name, bad)
    # what is exactly zero stays exactly zero: the closed channels, and the zero-gamma channel whose every maximum is 0
    assert (got["feat_max"][:, [5, 9]] == 0).all() and (got["dgamma1"][[5, 9]] == 0).all() and (got["dbeta1"][[5, 9]] == 0).all()
    assert (got["dW0"][7] == 0).all() and got["dgamma0"][7] == 0 and got["dbeta0"][7] == 0 and (got["dW1"][[5, 9]] == 0).all()


@pytest.mark.parametrize("name", ["many", "fat", "planted", "features_f6", "unique", "few_1"])
def test_two_steps_are_bit_identical(name):
    """Outputs, statistics and gradients of two full steps on the same cloud, bit for bit.  The work split is "the same for the same cloud, whatever
    the timing", but the grouping kernels (reader_bins.h) place the records of a pillar through LDS atomic cursors: their order in the sorted
    records changes from call to call, and the sums over rows changed with it (dW0 by 1-10 ulp in most entries of `many`, feat_max by 1-4 ulp while
    the Gram sums were fp32) until pass 0 ranked every pillar's records by content (k_pfn_canon) and every pass walked them in that order."""
    a, b = fused_step(name), run_step(T.case(name), True)
    for k in a:
        assert np.array_equal(a[k].view(np.int32) if a[k].dtype == np.float32 else a[k], b[k].view(np.int32) if b[k].dtype == np.float32 else b[k]), k


class _Torch0xFF:
    """torch, with an `empty` that hands out fp32 buffers full of 0xFF bytes (and a byte buffer -- the workspace, with the record order `canon` all passes index through -- likewise)."""

    def __init__(self, real):
        self._real, self.made = real, []

    def __getattr__(self, k):
        return getattr(self._real, k)

    def empty(self, *a, **kw):
        t = self._real.empty(*a, **kw)
        if t.dtype == self._real.float32:
            t.view(self._real.int32).fill_(-1)
        elif t.dtype == self._real.uint8:
            t.fill_(0xFF)
        self.made.append(t)
        return t


@pytest.mark.parametrize("name", ["many", "fat", "few_700", "few_1", "few_pillar3000", "features_f3", "features_f6"])
def test_every_slot_is_written(name, monkeypatch):
    """Passes 0, 1, 2 and backward 0, 1 with the partial buffers, `out` and the whole workspace full of 0xFF bytes beforehand (the host code of
    pfn_train.py itself, its torch.empty replaced): every partial finite, every row of feat_max below P finite, and the host reduction equal to
    the plain step bit for bit: every wave busy (many), more than a thousand waves with nothing to walk (fat, few_*), every feature count's layout."""
    from pillarnext_amd import pfn_train

    a = fused_step(name)            # the plain step, before torch.empty is replaced
    proxy = _Torch0xFF(torch)
    monkeypatch.setattr(pfn_train, "torch", proxy)
    b = run_step(T.case(name), True)
    F = T.case(name)["F"]
    L = pfn_train.lib()
    sizes = {int(L.pnx_pfn_train_partial_floats(F, w)): w for w in (0, 1, 3, 4)}
    parts = [t for t in proxy.made if t.dtype == torch.float32 and t.dim() == 1 and t.numel() in sizes]
    assert len(parts) == 4 and {t.numel() for t in parts} == set(sizes), [tuple(t.shape) for t in proxy.made]
    for t in parts:             # the Gram sums of the forward passes are doubles
        assert bool(torch.isfinite(t.view(torch.float64) if sizes[t.numel()] < 2 else t).all()), ("partial", sizes[t.numel()])
    outs = [t for t in proxy.made if t.dtype == torch.float32 and t.dim() == 2]
    assert len(outs) == 1 and bool(torch.isfinite(outs[0][: a["feat_max"].shape[0]]).all())
    assert any(t.dtype == torch.uint8 for t in proxy.made)
    for k in a:
        assert np.array_equal(a[k].view(np.int32) if a[k].dtype == np.float32 else a[k], b[k].view(np.int32) if b[k].dtype == np.float32 else b[k]), k


@pytest.mark.parametrize("kind", ["n0", "all_dropped"])
def test_empty_batch(kind, monkeypatch):
    monkeypatch.setenv("PNX_TRAIN_FUSED", "1")
    c = dict(T.case("features_f5"))
    net = make_net(c)
    with torch.no_grad():
        for pfn in net.pfn_layers:
            pfn.norm.momentum = 0.25
            pfn.norm.running_mean.fill_(0.5)
            pfn.norm.running_var.fill_(2.0)
    pts = torch.zeros((0, 6), device="cuda") if kind == "n0" else torch.full((100, 6), 1e6, device="cuda") * torch.tensor([0, 1, 1, 1, 1, 1], device="cuda")
    fm, coords, _ = net(pts, 2)
    assert fm.shape == (0, 64) and coords.shape == (0, 3) and type(fm.grad_fn).__name__ == "FusedPFNTrainBackward"
    fm.backward(torch.zeros((0, 64), device="cuda"))
    torch.cuda.synchronize()
    for p in net.parameters():
        assert p.grad is not None and bool((p.grad == 0).all()), "parameter gradients of an empty batch are exactly zero"
    for pfn in net.pfn_layers:      # the behaviour found (module docstring): a batch of mean 0 and variance 0
        assert bool((pfn.norm.running_mean == 0.375).all()) and bool((pfn.norm.running_var == 1.5).all()) and int(pfn.norm.num_batches_tracked) == 1
    # and the next, ordinary step is untouched by it
    got = run_step(c, True)
    assert np.array_equal(got["feat_max"], fused_step("features_f5")["feat_max"])
