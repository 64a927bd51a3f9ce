"""GPU: the per-point training layer of the multi-view reader (ops.PointLayer on csrc/point_layer_train.hip: Linear + BatchNorm1d with batch
statistics + ReLU [+ per-cell maximum], forward and backward) against the fp64 twin of tests/point_layer_ref.py.

Every held quantity -- y, gmax, the batch mean and variance (read through the running statistics with momentum 1 and zero initial values, as
test_gpu_pfn_train_vs_fp64.py does), dx, dW, dgamma, dbeta -- stays within the twin's bar, 2^-16 of the sum of |terms| (the statistics:
2^-16 (|mean| + std) and 2^-16 * 2 var); argmax equals the twin's exactly wherever the decision is not fragile.  The upstream gradient is zero on
the fragile decisions (ambiguous ReLU gates for dy, ambiguous cell maxima for dgmax); their share per case is asserted under GATE_CAP = 2^-8, the
constant of tests/train_graph_ref.py.  Each case prints the worst |error| / bar of the node and of the torch fp32 statement on the same inputs
(F.linear, BatchNorm1d, relu, ops.scatter_max); the second is a measurement and is not asserted.

Cases (n, cin, cout): n = 2, 63, 64, 65 and 1000 at 20 -> 24; more than one workgroup's rows and a row tail, n = 4097, at the reader's 20 -> 24,
48 -> 48 and 20 -> 192; more row tiles than workgroups (1 024 x 128 rows), so that a workgroup walks a second tile with its sums carried over, n = 131 201;
the K loop and the widest tile at (1500, 576, 256); odd widths (65, 33, 17) and (3000, 5, 3); x read in place from columns
5.. of a buffer cin + 7 wide, y written with ldy > cout (the C entry point directly); one cell holding every row, one row per cell, 300 cells over
4097 rows, cells without a row, planted bit-equal duplicate rows in one cell; want_y / want_max in the three combinations; dx not requested; dy
and dgmax both present; inputs offset by 4 through forward and backward and by 50 for the statistics and the forward only (the ambiguous band
grows with |mean|: the reference alone would pass the cap there); n = 1 raises; two calls, the second over workspaces full of 0xFF, give equal bits."""
import functools

import numpy as np
import pytest

import point_layer_ref as P

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
TINY = 1e-300

# name: (n, cin, cout, make_case keywords, want_y, want_max, dx requested, gradients asserted)
CASES = {
    "n2": (2, 20, 24, dict(G=2), True, True, True, True),
    "n63": (63, 20, 24, dict(G=9), True, True, True, True),
    "n64": (64, 20, 24, dict(G=9), True, False, True, True),
    "n65": (65, 20, 24, dict(G=9), False, True, True, True),
    "n1000": (1000, 20, 24, dict(G=140), True, True, True, True),
    "rows4097_20_24": (4097, 20, 24, dict(G=300), True, True, True, True),
    "rows4097_48_48": (4097, 48, 48, dict(G=300), False, True, True, True),
    "rows4097_20_192": (4097, 20, 192, dict(), True, False, True, True),
    "rows_loop": (131_201, 20, 24, dict(G=9000), True, True, True, True),
    "k576_256": (1500, 576, 256, dict(G=200), False, True, True, True),
    "odd_65_33_17": (65, 33, 17, dict(G=11), True, True, True, True),
    "odd_3000_5_3": (3000, 5, 3, dict(G=400), True, True, True, True),
    "slice_ldx": (1000, 20, 24, dict(G=140, ldx=True), True, True, True, True),
    "one_cell": (4097, 20, 24, dict(cells="one"), False, True, True, True),
    "each_cell": (1000, 48, 48, dict(cells="each"), True, True, True, True),
    "empty_cells": (300, 20, 24, dict(G=2000), True, True, True, True),
    "duplicates": (1000, 20, 24, dict(G=60, dup=200), True, True, True, True),
    "no_dx": (1000, 48, 48, dict(G=140), True, True, False, True),
    "offset4": (4097, 20, 24, dict(G=300, offset=4.0), True, True, True, True),
    "offset50": (4097, 20, 24, dict(G=300, offset=50.0), True, True, True, False),
}
SEEDS = {name: 100 + i for i, name in enumerate(c for c in CASES if c != "rows_loop")}
SEEDS["rows_loop"] = 150
SEEDS.update(odd_65_33_17=209)      # chosen so that the twin alone meets the cap: 187 maxima, one near-tie among them is already 2^-7.5


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs, twin and upstream gradients of a case, computed once, shared and read-only."""
    n, cin, cout, kw, want_y, want_max, need_dx, grads = CASES[name]
    kw = dict(kw)
    ldx = kw.pop("ldx", False)
    c = P.make_case(n, cin, cout, SEEDS[name], **kw)
    s = P.forward(c["x"], c["W"], c["gamma"], c["beta"], c["inv"] if want_max else None, c["G"] if want_max else 0)
    rng = np.random.default_rng(SEEDS[name] + 500)
    dy = dg = None
    if want_y:
        dy = rng.standard_normal((n, cout)).astype(np.float32)
        dy[s["gate_amb"]] = 0
    if want_max:
        dg = rng.standard_normal((c["G"], cout)).astype(np.float32)
        dg[s["max_amb"]] = 0
    b = P.backward(s, dy, dg)
    c.update(name=name, ref=s, bwd=b, dy=dy, dg=dg, want_y=want_y, want_max=want_max, need_dx=need_dx, grads=grads, ldx=ldx)
    for a in (c["x"], c["W"], c["gamma"], c["beta"], c["inv"], dy, dg, *[v for v in s.values() if isinstance(v, np.ndarray)]):
        if a is not None:
            a.setflags(write=False)
    return c


def _modules(c):
    from torch import nn

    cout, cin = c["W"].shape
    lin = nn.Linear(cin, cout, bias=False).cuda()
    norm = nn.BatchNorm1d(cout, eps=P.EPS, momentum=1.0).cuda().train()
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(np.array(c["W"])))
        norm.weight.copy_(torch.from_numpy(np.array(c["gamma"])))
        norm.bias.copy_(torch.from_numpy(np.array(c["beta"])))
        norm.running_mean.zero_()
        norm.running_var.zero_()
    return lin, norm


def _input(c):
    x = torch.from_numpy(np.array(c["x"])).cuda()
    if c["ldx"]:                                                    # columns 5.. of a buffer cin + 7 wide, read in place
        wide = torch.full((x.shape[0], x.shape[1] + 7), float("nan"), device="cuda")
        wide[:, 5:5 + x.shape[1]] = x
        x = wide[:, 5:5 + x.shape[1]]
        assert x.stride(0) == c["x"].shape[1] + 7
    return x.requires_grad_(True) if c["need_dx"] else x


def run(c, node=True):
    """One forward + backward on the node (or the torch fp32 statement); everything as numpy."""
    from pillarnext_amd import ops

    lin, norm = _modules(c)
    x = _input(c)
    inv = torch.from_numpy(np.array(c["inv"])).cuda() if c["want_max"] else None
    G = c["G"]
    arg = None
    if node:
        y, gmax, arg = ops.PointLayer.apply(x, lin.weight, norm.weight, norm.bias, inv, G, c["want_y"], c["want_max"], float(norm.eps), norm)
        assert type((y if y is not None else gmax).grad_fn).__name__ == "PointLayerBackward"
    else:
        y = torch.relu(norm(lin(x)))
        gmax = None
        if c["want_max"]:
            gmax, arg = ops.scatter_max(y, inv, G)
        if not c["want_y"]:
            y = None
    outs, gos = [], []
    if y is not None:
        outs.append(y), gos.append(torch.from_numpy(np.array(c["dy"])).cuda())
    if gmax is not None:
        outs.append(gmax), gos.append(torch.from_numpy(np.array(c["dg"])).cuda())
    torch.autograd.backward(outs, gos)
    torch.cuda.synchronize()
    assert int(norm.num_batches_tracked) == 1
    out = dict(y=y, gmax=gmax, argmax=arg, running_mean=norm.running_mean, running_var=norm.running_var, dW=lin.weight.grad, dgamma=norm.weight.grad,
               dbeta=norm.bias.grad, dx=x.grad if c["need_dx"] else None)
    return {k: (None if v is None else v.detach().cpu().numpy()) for k, v in out.items()}


def ratios(c, got):
    s, b = c["ref"], c["bwd"]
    w = {}
    if c["want_y"]:
        w["y"] = float((np.abs(got["y"] - s["y"]) / (s["y_bar"] + TINY)).max())
    if c["want_max"]:
        w["gmax"] = float((np.abs(got["gmax"] - s["gmax"]) / (s["gmax_bar"] + TINY)).max())
    w["mean"] = float((np.abs(got["running_mean"] - s["running_mean"]) / (s["running_mean_bar"] + P.U * np.abs(s["running_mean"]) + TINY)).max())
    w["var"] = float((np.abs(got["running_var"] - s["running_var"]) / (s["running_var_bar"] + P.U * np.abs(s["running_var"]) + TINY)).max())
    if c["grads"]:
        for k in ("dx", "dW", "dgamma", "dbeta"):
            if got[k] is not None:
                w[k] = float((np.abs(got[k] - b[k]) / (b[k + "_bar"] + TINY)).max())
    return w


@functools.lru_cache(maxsize=None)
def node_step(name):
    return run(case(name), True)


@pytest.mark.parametrize("name", list(CASES))
def test_case_vs_fp64(name):
    from train_graph_ref import GATE_CAP

    c = case(name)
    s = c["ref"]
    n, cout = s["n"], s["cout"]
    # the share of the upstream gradient that is left out, per case: asserted under the cap
    gate_share = float(s["gate_amb"].mean()) if c["want_y"] else 0.0
    max_share = float(s["max_amb"].sum()) / max(int(s["has"].sum()) * cout, 1) if c["want_max"] else 0.0
    if c["grads"]:
        assert gate_share <= GATE_CAP and max_share <= GATE_CAP, (name, gate_share, max_share)
        if c["want_y"]:
            assert int((c["dy"] == 0).sum()) <= int(s["gate_amb"].sum()) + 8      # nothing else is left out (a normal deviate is not 0)
        if c["want_max"]:
            assert int((c["dg"] == 0).sum()) <= int(s["max_amb"].sum()) + 8
    got = node_step(name)
    assert all(np.isfinite(v).all() for v in got.values() if v is not None)
    w = ratios(c, got)
    ref = ratios(c, run(c, False))
    print(f"[point layer vs fp64] {name}: n={n} {s['cin']} -> {cout} G={c['G']} gate share {gate_share:.2e} max share {max_share:.2e}  worst |err| / bar: node "
          + " ".join(f"{k} {v:.3f}" for k, v in w.items()) + " | torch fp32 " + " ".join(f"{k} {v:.3f}" for k, v in ref.items()))
    bad = {k: v for k, v in w.items() if v > 1.0}
    assert not bad, (name, bad)
    if c["want_max"]:
        empty = ~s["has"]
        assert (got["gmax"][empty] == 0).all() and (got["argmax"][empty] == n).all()
        firm = ~s["max_amb"]
        assert np.array_equal(got["argmax"][firm], s["argmax"][firm]), int((got["argmax"][firm] != s["argmax"][firm]).sum())
        assert ((got["argmax"] >= 0) & (got["argmax"] <= n)).all()
    if not c["need_dx"]:
        assert got["dx"] is None


def test_the_cases_take_their_paths():
    """On the host: what each case is there for holds in the twin."""
    s = case("empty_cells")["ref"]
    assert (~s["has"]).sum() > 1500
    c = case("duplicates")
    s = c["ref"]
    rows0 = np.flatnonzero(c["inv"] == 0)
    x0 = np.array(c["x"])[rows0]
    assert len(rows0) >= 400 and len(np.unique(x0, axis=0)) <= len(rows0) - 200
    held = [ch for ch in range(s["cout"]) if s["max_open"][0, ch] and not s["max_amb"][0, ch]
            and (np.array(c["x"])[rows0] == np.array(c["x"])[s["argmax"][0, ch]]).all(1).sum() > 1]
    assert len(held) >= 1, "no maximum of cell 0 is held by a planted pair"
    assert case("one_cell")["ref"]["has"].all() and case("one_cell")["G"] == 1
    assert (np.bincount(case("each_cell")["inv"]) == 1).all()
    s = case("offset50")["ref"]
    assert (np.abs(s["mean"]) / np.sqrt(s["var"])).max() > 30
    s = case("offset4")["ref"]
    assert (np.abs(s["mean"]) / np.sqrt(s["var"])).max() > 3


def test_one_row_raises():
    from pillarnext_amd import ops

    c = dict(case("n2"))
    lin, norm = _modules(c)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        ops.point_layer(torch.zeros((1, 20), device="cuda"), lin, norm)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):     # what BatchNorm1d raises
        norm(lin(torch.zeros((1, 20), device="cuda")))


def test_ldy_wider_than_cout():
    """The C entry point writes y into the first cout columns of rows ldy apart and touches nothing else."""
    from pillarnext_amd._lib import check, lib, ptr, stream_ptr

    c = case("slice_ldx")
    s = c["ref"]
    n, cin, cout = s["n"], s["cin"], s["cout"]
    x = _input(dict(c, need_dx=False))
    w = torch.from_numpy(np.array(c["W"])).cuda()
    prm = torch.zeros((6, cout), device="cuda")
    prm[0], prm[1] = torch.from_numpy(s["mean"]).float().cuda(), torch.from_numpy(s["invstd"]).float().cuda()
    prm[2], prm[3] = torch.from_numpy(np.array(c["gamma"])).cuda(), torch.from_numpy(np.array(c["beta"])).cuda()
    y = torch.full((n, cout + 5), -7.0, device="cuda")
    check(lib().pnx_point_layer_forward(ptr(x), x.stride(0), n, cin, ptr(w), cout, ptr(prm), None, 0, ptr(y), cout + 5, None, None, stream_ptr()), "forward")
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    assert (y[:, cout:] == -7.0).all()
    assert float((np.abs(y[:, :cout] - s["y"]) / (s["y_bar"] + TINY)).max()) <= 1.0


class _Torch0xFF:
    """torch, with an `empty` that hands out buffers full of 0xFF bytes."""

    def __init__(self, real):
        self._real = real
        self.made = 0

    def __getattr__(self, k):
        return getattr(self._real, k)

    def empty(self, *a, **kw):
        t = self._real.empty(*a, **kw)
        t.view(self._real.uint8).fill_(0xFF)
        self.made += 1
        return t


@pytest.mark.parametrize("name", ["rows4097_20_24", "k576_256", "duplicates", "n2"])
def test_two_calls_give_equal_bits(name, monkeypatch):
    """The second call runs over 0xFF: the persistent forward workspace, and every buffer ops.py allocates (outputs, the statistics' sums, the
    backward's workspace) through a torch.empty that fills it first."""
    from pillarnext_amd import ops

    a = node_step(name)
    assert ops._PL_WS.buf is not None
    ops._PL_WS.buf.fill_(0xFF)
    proxy = _Torch0xFF(torch)
    monkeypatch.setattr(ops, "torch", proxy)
    b = run(case(name), True)
    assert proxy.made >= 5
    for k in a:
        if a[k] is None:
            assert b[k] is None
            continue
        va = a[k].view(np.int32) if a[k].dtype == np.float32 else a[k]
        vb = b[k].view(np.int32) if b[k].dtype == np.float32 else b[k]
        assert np.array_equal(va, vb), k
