"""CPU: tests/pfn_train_ref.py, the fp64 twin of one training step of the fused reader, pinned before tests/test_gpu_pfn_train_vs_fp64.py
leans on it -- no GPU, no kernel code.

(a) an independent float64 torch AUTOGRAD statement on every case input (nn.Linear / nn.BatchNorm1d in double, scatter_reduce('amax'), gather, cat):
    forward, batch statistics and the six gradients agree to 1e-10 of each quantity's sum of |terms|.  amax's backward shares the gradient among
    equal maxima: between the planted duplicates that changes no sum, and at a maximum of exactly 0 the ReLU closes it, as the twin's docstring says.
    One row (`few_1`) is beyond BatchNorm1d, which raises on fewer than two rows: there the statement normalises by hand.
(b) the reference's own fp32 run stored in reader_nusc_b2, reader_c1_train_fat, reader_c1_b3_gap_train (train_feat_max, train_l*_dW / dgamma /
    dbeta, running statistics at momentum 0.01) sits inside the twin's bars.  Its upstream gradient is NOT zero on the fragile layer-1 decisions;
    the gradients are linear in every such decision, so each one is flipped on its own through grads_of_dz1 (the maximum moved to the second
    distinct row, a gate within its bound toggled) and the sum of |change| is the allowance added for them.  Worst |err| / bar is printed.
(c) the conditions the GPU module relies on, on every case with at least 100 pillars (with one pillar a share moves in steps of 1/64):
    fragile layer-0 entries <= 0.02 % of N' x 32, masked G <= 2 % of the positive maxima, at least 25 % of the maxima positive;
    and what each case plants (a closed channel per layer, the zero-gamma channel, the widened entries and their median widening, printed)."""
import numpy as np
import pytest

import pfn_train_ref as T
from conftest import golden_layers, load_golden

torch = pytest.importorskip("torch")

GRADS = ("dW0", "dgamma0", "dbeta0", "dW1", "dgamma1", "dbeta1")
TINY = 1e-300


def torch_statement(s, G):
    import torch.nn as nn

    N, P = s["N"], s["P"]
    f, inv = torch.from_numpy(np.array(s["f"])), torch.from_numpy(np.array(s["inv_s"]))
    mods = []
    for i, (cin, cout) in enumerate(((f.shape[1], 32), (64, 64))):
        lin, bn = nn.Linear(cin, cout, bias=False).double(), nn.BatchNorm1d(cout, eps=T.EPS, momentum=1.0).double().train()
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(np.array(s["prm"][f"W{i}"])))
            bn.weight.copy_(torch.from_numpy(np.array(s["prm"][f"gamma{i}"])))
            bn.bias.copy_(torch.from_numpy(np.array(s["prm"][f"beta{i}"])))
        mods.append((lin, bn))

    def layer(lin, bn, x):
        y = lin(x)
        if N > 1:
            y = bn(y)
        else:
            y = (y - y.mean(0)) / torch.sqrt(y.var(0, unbiased=False) + T.EPS) * bn.weight + bn.bias
        h = torch.relu(y)
        mx = torch.zeros((P, h.shape[1]), dtype=torch.float64).scatter_reduce(0, inv[:, None].expand(-1, h.shape[1]), h, "amax", include_self=False)
        return h, mx

    h0, g0 = layer(*mods[0], f)
    h1, fm = layer(*mods[1], torch.cat([h0, g0[inv]], dim=1))
    fm.backward(torch.from_numpy(np.asarray(G, np.float64)))
    out = dict(feat_max=fm.detach().numpy())
    for i, (lin, bn) in enumerate(mods):
        out[f"dW{i}"], out[f"dgamma{i}"], out[f"dbeta{i}"] = lin.weight.grad.numpy(), bn.weight.grad.numpy(), bn.bias.grad.numpy()
        if N > 1:
            out[f"mu{i}"], out[f"rvar{i}"] = bn.running_mean.numpy(), bn.running_var.numpy()
    return out


@pytest.mark.parametrize("name", T.CASES)
def test_twin_equals_the_float64_autograd_statement(name):
    s = T.case(name)["ref"]
    t = torch_statement(s, s["G"])
    worst = {}
    for k in ("feat_max",) + GRADS:
        worst[k] = float((np.abs(t[k] - s[k]) / (s[k + "_terms"] + TINY)).max())
    if s["N"] > 1:
        for i in (0, 1):
            rm, rv, _, _ = T.running(s[f"mu{i}"], s[f"var{i}"], s["N"])
            worst[f"mu{i}"] = float((np.abs(t[f"mu{i}"] - rm) / (np.abs(rm) + np.sqrt(s[f"var{i}"]) + TINY)).max())
            worst[f"var{i}"] = float((np.abs(t[f"rvar{i}"] - rv) / (2 * rv + TINY)).max())
    print(f"[pfn train twin] {name}: worst |twin - autograd| / sum|terms| " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) <= 1e-10, worst
    lin = T.grads_of_dz1(s, _dz1(s, s["G"]))
    for k in GRADS:
        assert float((np.abs(lin[k] - s[k]) / (s[k + "_terms"] + TINY)).max()) <= 1e-12, k


def _dz1(s, G):
    dz1 = np.zeros((s["N"], 64))
    dz1[s["arg1"], np.arange(64)[None, :]] = np.asarray(G, np.float64) * s["positive1"]
    return dz1


def _layer1_allowance(s, G):
    """Sum over the fragile layer-1 decisions with a non-zero upstream gradient of |change of every gradient| when that one decision flips."""
    allow = {k: np.zeros_like(s[k]) for k in GRADS}
    starts, cnt, y1, first = s["starts"], s["cnt"], s["y1"], s["first"][:, 0]
    flips = 0
    for p, c in zip(*np.nonzero(s["mask1"] & (np.asarray(G) != 0))):
        lo, a = starts[p], s["arg1"][p, c]
        rows = np.arange(lo, lo + cnt[p])
        g = float(G[p, c])
        alts = []
        if abs(y1[a, c]) <= s["e_y1"][a, c]:                                     # the gate of the maximum toggles
            alts.append((a, -g if y1[a, c] > 0 else g))
        others = rows[first[rows] & (rows != a)]
        near = others[y1[a, c] - y1[others, c] <= s["e_y1"][a, c] + s["e_y1"][others, c]]
        for b in near:                                                          # the maximum moves to another distinct row
            alts.append((None, (a, b, g)))
        for alt in alts:
            dz = np.zeros((s["N"], 64))
            if alt[0] is not None:
                dz[alt[0], c] = alt[1]
            else:
                a_, b_, g_ = alt[1]
                if y1[a_, c] > 0:
                    dz[a_, c] -= g_
                dz[b_, c] += g_
            d = T.grads_of_dz1(s, dz)
            for k in GRADS:
                allow[k] += np.abs(d[k])
            flips += 1
    return allow, flips


@pytest.mark.parametrize("fixture", ["reader_nusc_b2", "reader_c1_train_fat", "reader_c1_b3_gap_train"])
def test_reference_run_sits_inside_the_twins_bars(fixture):
    g = load_golden(fixture)
    L = golden_layers(g)
    prm = dict(W0=L[0]["W"], gamma0=L[0]["gamma"], beta0=L[0]["beta"], W1=L[1]["W"], gamma1=L[1]["gamma"], beta1=L[1]["beta"])
    B = int(g["coords"][:, 0].max()) + 1
    s = T.forward(g["points"], B, g["pc_range"], g["voxel_size"], prm, eps=float(g["eps"]))
    assert np.array_equal(s["coords"], g["coords"])
    G = g["train_upstream_grad"]
    s.update(T.backward(s, G))
    allow, flips = _layer1_allowance(s, G)
    worst = {"feat_max": float((np.abs(g["train_feat_max"] - s["feat_max"]) / (s["feat_max_bar"] + T.U * np.abs(s["feat_max"]) + TINY)).max())}
    for i in (0, 1):
        for k, gk in ((f"dW{i}", f"train_l{i}_dW"), (f"dgamma{i}", f"train_l{i}_dgamma"), (f"dbeta{i}", f"train_l{i}_dbeta")):
            worst[k] = float((np.abs(g[gk] - s[k]) / (s[k + "_bar"] + allow[k] + T.U * np.abs(s[k]) + TINY)).max())     # + the fp32 rounding of the stored value
        rm, rv, brm, brv = T.running(s[f"mu{i}"], s[f"var{i}"], s["N"], 0.01, L[i]["mean"].astype(np.float64), L[i]["var"].astype(np.float64),
                                       s["stat1_in"] if i else (0.0, 0.0))
        worst[f"running_mean{i}"] = float((np.abs(g[f"train_l{i}_running_mean"] - rm) / (brm + 2 * T.U * np.abs(rm) + TINY)).max())
        worst[f"running_var{i}"] = float((np.abs(g[f"train_l{i}_running_var"] - rv) / (brv + 2 * T.U * np.abs(rv) + TINY)).max())
    print(f"[pfn train twin] {fixture}: N'={s['N']} P={s['P']} fragile layer-1 flips allowed for {flips}; reference worst |err| / bar "
          + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("name", T.CASES)
def test_conditions_and_plants(name):
    c = T.case(name)
    s = c["ref"]
    frag, masked, positive = T.conditions(s)
    wide = [(s[k + "_allow"] / (s[k + "_bar0"] + TINY))[s[k + "_allow"] > 0] for k in ("dW0", "dgamma0", "dbeta0")]
    wide = np.concatenate([w.ravel() for w in wide])
    print(f"[pfn train twin] {name}: N'={s['N']} P={s['P']} F={c['F']} fragile layer-0 entries {s['fragile0']} = {100 * frag:.4f} % of N' x 32, masked "
          f"{100 * masked:.2f} % of the positive maxima, positive {100 * positive:.1f} %; widened gradient entries {len(wide)}"
          + (f", median widening {np.median(wide):.2f} x the bar" if len(wide) else "")
          + "; ceiling binds on " + " ".join(f"{k} {100 * s[k + '_capped']:.0f}%" for k in GRADS))
    if s["P"] >= 100:
        assert frag <= T.MAX_FRAGILE0 and masked <= T.MAX_MASKED1 and positive >= T.MIN_POSITIVE1, (frag, masked, positive)
    # the plants of make_params
    assert (s["h0"][:, 7] == 0).all() and (s["feat_max"][:, 9] == 0).all() and (s["feat_max"][:, 5] == 0).all() and (s["y1"][:, 5] == 0).all()
    assert (c["prm"]["gamma0"] < 0).any() and (c["prm"]["gamma1"] < 0).any() and c["prm"]["gamma1"][5] == 0
    assert not (s["G"][s["mask1"]] != 0).any() and s["mask1"][:, 5].all()
    for k in ("feat_max",) + GRADS:
        assert (s[k + "_bar"] <= T.BN_REL * s[k + "_terms"] + (s[k + "_allow"] if k != "feat_max" else 0) + TINY).all(), k      # the ceiling


def test_wave_split_is_the_kernels_binary_search():
    """wave_split against a literal restatement of first_at on a few count vectors (one fat pillar, one pillar, none)."""
    rng = np.random.default_rng(0)
    for cnt in (rng.integers(1, 9, 5000), np.r_[rng.integers(1, 4, 700), 9000, rng.integers(1, 4, 900)], np.array([3000]), np.zeros(0, np.int64), np.array([1])):
        P, n_rec, nw = len(cnt), int(np.sum(cnt)), T.N_WAVES
        pfirst = np.concatenate([[0], np.cumsum(cnt)[:-1]]) if P else []

        def first_at(target):
            lo, hi = 0, P
            while lo < hi:
                mid = (lo + hi) >> 1
                if pfirst[mid] >= target:
                    hi = mid
                else:
                    lo = mid + 1
            return lo
        r0, r1 = T.wave_split(cnt)
        for w in (0, 1, 2, 500, 1023, 1024, nw - 2, nw - 1):
            assert r0[w] == (0 if w == 0 else first_at(n_rec * w // nw)) and r1[w] == (P if w + 1 == nw else first_at(n_rec * (w + 1) // nw))
        assert (r1 - r0).sum() == P and (r0[1:] == r1[:-1]).all()
