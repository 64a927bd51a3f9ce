"""No GPU: the fp64 twin of the per-point training layer (tests/point_layer_ref.py) against torch autograd in float64 on the CPU -- F.linear,
F.batch_norm(training=True), relu and a maximum by index -- to 1e-12 relative, and the argument checks of the five entry points of
csrc/point_layer_train.hip, which reject what they do not serve before any HIP call (by return code and message)."""
import ctypes

import numpy as np
import pytest

import point_layer_ref as P

torch = pytest.importorskip("torch")
F = torch.nn.functional
RTOL = 1e-12


def _close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(float(np.abs(ref).max()), 1e-300)
    assert float(np.abs(got - ref).max()) <= RTOL * scale, (what, float(np.abs(got - ref).max()) / scale)


@pytest.mark.parametrize("n,cin,cout", [(65, 33, 17), (300, 20, 24)])
def test_twin_against_torch_autograd_fp64(n, cin, cout):
    G = max(n // 7, 1) + 3                                         # a few cells stay empty
    c = P.make_case(n, cin, cout, seed=7 + n, G=G)
    c["inv"][c["inv"] >= G - 3] = 0
    s = P.forward(c["x"], c["W"], c["gamma"], c["beta"], c["inv"], G)
    rng = np.random.default_rng(1)
    dy, dg = rng.standard_normal((n, cout)), rng.standard_normal((G, cout))
    b = P.backward(s, dy, dg)

    x = torch.tensor(c["x"], dtype=torch.float64, requires_grad=True)
    W = torch.tensor(c["W"], dtype=torch.float64, requires_grad=True)
    ga = torch.tensor(c["gamma"], dtype=torch.float64, requires_grad=True)
    be = torch.tensor(c["beta"], dtype=torch.float64, requires_grad=True)
    rm, rv = torch.zeros(cout, dtype=torch.float64), torch.zeros(cout, dtype=torch.float64)
    y = torch.relu(F.batch_norm(F.linear(x, W), rm, rv, ga, be, training=True, momentum=1.0, eps=P.EPS))
    arg = torch.from_numpy(s["argmax"])
    live = torch.from_numpy(s["has"])
    gmax = torch.zeros((G, cout), dtype=torch.float64)
    gmax[live] = torch.gather(y, 0, arg[live])                     # the maximum by index
    (y * torch.from_numpy(dy)).sum().add((gmax * torch.from_numpy(dg)).sum()).backward()

    _close(s["y"], y.detach(), "y")
    ref_max = torch.full((G, cout), -1.0, dtype=torch.float64).scatter_reduce(0, torch.from_numpy(c["inv"])[:, None].expand(n, cout), y.detach(), "amax")
    _close(s["gmax"], torch.where(live[:, None], ref_max, torch.zeros(())), "gmax")
    assert (s["gmax"][~s["has"]] == 0).all() and (s["argmax"][~s["has"]] == n).all() and (~s["has"]).sum() >= 3
    # the lowest row that attains the maximum
    yn, inv = s["y"], c["inv"]
    for g in np.flatnonzero(s["has"])[:40]:
        rows = np.flatnonzero(inv == g)
        for ch in range(cout):
            assert s["argmax"][g, ch] == rows[np.argmax(yn[rows, ch])]
    _close(s["running_mean"], rm, "running_mean")
    _close(s["running_var"], rv, "running_var")
    _close(b["dx"], x.grad, "dx")
    _close(b["dW"], W.grad, "dW")
    _close(b["dgamma"], ga.grad, "dgamma")
    _close(b["dbeta"], be.grad, "dbeta")
    for k in ("dx", "dW", "dgamma", "dbeta"):                      # the sums of |terms| dominate the values
        assert (b[k + "_terms"] >= np.abs(b[k]) * (1 - 1e-9)).all(), k
    assert (s["y_terms"] >= np.abs(s["pre"]) * (1 - 1e-9)).all()


def test_duplicates_count_as_one_row():
    c = P.make_case(200, 20, 24, seed=3, G=10, dup=30)
    s = P.forward(c["x"], c["W"], c["gamma"], c["beta"], c["inv"], 10)
    # cell 0 holds 30 bit-equal pairs: a maximum held by a pair is not ambiguous for that reason, and the first copy is named
    rows0 = np.flatnonzero(c["inv"] == 0)
    held = 0
    for ch in range(24):
        r = s["argmax"][0, ch]
        twins = [q for q in rows0 if q != r and np.array_equal(c["x"][q], c["x"][r])]
        if twins and s["max_open"][0, ch]:
            held += 1
            assert r < min(twins)
    assert held >= 1


def _lib():
    from pillarnext_amd import _lib

    return _lib.lib()


def test_entry_points_reject_before_any_hip_call():
    L = _lib()
    buf = np.zeros(1 << 16, np.uint8)
    base = (buf.ctypes.data + 255) // 256 * 256                   # host memory: a call that got past its checks would fail, none does
    p = ctypes.c_void_p(base)
    big = 1 << 40
    ok = dict(x=p, ldx=20, n=10, cin=20, w=p, cout=24)
    bad = [("cin = 0", dict(cin=0, ldx=20), -1, b"bad sizes"), ("cin = 577", dict(cin=577, ldx=577), -2, b"at most 576"),
           ("cout = 257", dict(cout=257), -2, b"at most 576 -> 256"), ("ldx < cin", dict(ldx=19), -1, b"ldx 19 < cin 20"), ("n < 0", dict(n=-1), -1, b"bad sizes"),
           ("NULL W", dict(w=None), -1, b"null pointer")]

    def stats(a):
        return L.pnx_point_layer_stats(a["x"], a["ldx"], a["n"], a["cin"], a["w"], a["cout"], p, p, big, None)

    def fwd(a, y=p, gmax=p):
        return L.pnx_point_layer_forward(a["x"], a["ldx"], a["n"], a["cin"], a["w"], a["cout"], p, p, 5, y, a["cout"], gmax, p, None)

    def bstats(a, dy=p, dg=p):
        return L.pnx_point_layer_backward_stats(a["x"], a["ldx"], a["n"], a["cin"], a["w"], a["cout"], p, dy, a["cout"], p, 5, dg, p, p, p, big, None)

    def bwd(a, dy=p, dg=p):
        return L.pnx_point_layer_backward(a["x"], a["ldx"], a["n"], a["cin"], a["w"], a["cout"], p, dy, a["cout"], p, 5, dg, p, p, a["cin"], p, p, big, None)

    for name, fn in (("pnx_point_layer_stats", stats), ("pnx_point_layer_forward", fwd), ("pnx_point_layer_backward_stats", bstats),
                     ("pnx_point_layer_backward", bwd)):
        for what, change, code, msg in bad:
            rc = fn({**ok, **change})
            err = L.pnx_last_error()
            assert rc == code and msg in err and name.encode() in err, (name, what, rc, err)
    # neither output / neither upstream gradient requested
    assert fwd(ok, y=None, gmax=None) == -1 and b"pnx_point_layer_forward: neither y nor gmax requested" in L.pnx_last_error()
    assert bstats(ok, dy=None, dg=None) == -1 and b"pnx_point_layer_backward_stats: neither dy nor dgmax given" in L.pnx_last_error()
    assert bwd(ok, dy=None, dg=None) == -1 and b"pnx_point_layer_backward: neither dy nor dgmax given" in L.pnx_last_error()
    # the workspace query answers 0 for the same shapes, and a workspace that is too small or misaligned is refused
    W = L.pnx_point_layer_workspace_bytes
    assert W(10, 0, 24, 0) == 0 and W(10, 577, 24, 0) == 0 and W(10, 20, 257, 1) == 0 and W(-1, 20, 24, 0) == 0
    assert 0 < W(10, 20, 24, 0) <= W(10, 20, 24, 1) and W(360_000, 576, 256, 0) < 8 << 20
    assert L.pnx_point_layer_stats(p, 20, 10, 20, p, 24, p, p, 16, None) == -3 and b"pnx_point_layer_stats: workspace" in L.pnx_last_error()
    assert L.pnx_point_layer_stats(p, 20, 10, 20, p, 24, p, ctypes.c_void_p(base + 8), big, None) == -1 and b"256-byte aligned" in L.pnx_last_error()


def test_switch_is_declared():
    from pillarnext_amd import switches

    assert "PNX_TRAIN_POINT_HIP" in switches.SWITCHES and "csrc/point_layer_train.hip" in switches.SWITCHES["PNX_TRAIN_POINT_HIP"][1]
