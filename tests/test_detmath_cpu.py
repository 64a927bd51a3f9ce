"""CPU: csrc/pnx_detmath.h's sin / cos / atan2 -- the transcendentals the rotated-IoU kernels, the host twins, the cylinder view and the oracle share --
against the correctly rounded fp32 value (tests/golden/detmath_cases.npz, written by tools/gen_detmath_golden.py from mpmath at 256 bits).

The header's contract: the fp64 value (abs err < 1e-15) rounded once to fp32, for every |a| < 1e9 and every atan2 pair; NaN at and beyond the limit;
sin(+-0) = +-0.  The list is fixed and both sides are deterministic, so the number of results that may differ from the correctly rounded value is a
condition, not a measurement: only a result the fixture names as a hard rounding case (within 1e-7 ulp of a rounding boundary) may sit on the other
neighbour, and the fixture may name at most 4."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, load_golden
from iou_cases import host_detmath, same_bits

MAX_HARD = 4


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def generator():
    spec = importlib.util.spec_from_file_location("gen_detmath_golden", os.path.join(ROOT, "tools", "gen_detmath_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def g():
    return load_golden("detmath_cases")


@pytest.fixture(scope="module")
def host(g):
    s, c, _ = host_detmath(g["sc_a"], np.ones_like(g["sc_a"]))
    _, _, t = host_detmath(g["at_y"], g["at_x"])
    return s, c, t


def test_fixture_is_the_generators_list(g):
    gen = generator()
    assert float(g["limit"]) == gen.LIMIT == 1.0e9                      # the number in pnx_detmath.h's header
    assert np.all(same_bits(g["sc_a"], gen.sincos_args()))
    y, x = gen.atan2_args()
    assert np.all(same_bits(g["at_y"], y)) and np.all(same_bits(g["at_x"], x))
    a = g["sc_a"]
    assert len(a) > 20000 and len(y) > 8000
    fin = np.isfinite(a)
    assert (np.abs(a[fin]) >= 1e8).sum() > 1000 and (np.abs(a[fin]) < 1e-38).sum() > 500 and (~fin).sum() >= 3
    assert np.isnan(g["sc_sin"][~fin]).all() and np.isnan(g["sc_sin"][fin & (np.abs(a) >= 1e9)]).all()
    assert np.isfinite(g["sc_sin"][fin & (np.abs(a) < 1e9)]).all()
    assert len(g["hard_kind"]) <= MAX_HARD and np.all(g["hard_err_ulp"] < 0.5000001)


def test_host_equals_oracle_export(g, host, oracle):
    s, c, _ = oracle.detmath(g["sc_a"], np.ones_like(g["sc_a"]))
    _, _, t = oracle.detmath(g["at_y"], g["at_x"])
    for got, want in zip(host, (s, c, t)):
        assert np.all(same_bits(got, want))


def test_host_is_correctly_rounded(g, host):
    wrong = 0
    for kind, (got, want, what) in enumerate(zip(host, (g["sc_sin"], g["sc_cos"], g["at_r"]), ("sin", "cos", "atan2"))):
        bad = np.nonzero(~same_bits(got, want))[0]
        named = set(g["hard_index"][g["hard_kind"] == kind].tolist())
        args = g["sc_a"] if kind < 2 else np.stack([g["at_y"], g["at_x"]], 1)
        assert set(bad.tolist()) <= named, f"{what}: {len(bad)} results not correctly rounded, first at {args[bad[:5]]!r}: {got[bad[:5]]!r} != {want[bad[:5]]!r}"
        for i in bad:                                                     # a named hard case: the other fp32 neighbour, nothing further
            assert abs(int(bits(got[i:i + 1])[0]) - int(bits(want[i:i + 1])[0])) == 1
        wrong += len(bad)
    assert wrong <= MAX_HARD


def test_signed_zeros_and_limit(g):
    z = np.asarray([0.0, -0.0], np.float32)
    s, c, _ = host_detmath(z, z)
    assert np.array_equal(bits(s), bits(z)) and np.array_equal(c, [1.0, 1.0])      # sin keeps the sign of the zero, as libm (and so the reference) does
    lim = np.float32(g["limit"])
    a = np.asarray([np.nextafter(lim, np.float32(0)), lim, -lim, np.nextafter(-lim, np.float32(0))], np.float32)
    s, c, _ = host_detmath(a, a)
    assert np.isfinite(s[[0, 3]]).all() and np.isnan(s[[1, 2]]).all() and np.isnan(c[[1, 2]]).all()
    # IEEE atan2 on signed zeros against a negative x: +-pi, the sign that orders a polygon's vertices
    _, _, t = host_detmath(np.asarray([0.0, -0.0, 0.0, -0.0], np.float32), np.asarray([-1.0, -1.0, 1.0, 1.0], np.float32))
    assert np.array_equal(bits(t), bits(np.asarray([np.pi, -np.pi, 0.0, -0.0], np.float32)))


def test_sample_rederived_where_mpmath_is(g):
    if importlib.util.find_spec("mpmath") is None:
        return                                                            # the fixture stands alone; only its generator needs mpmath
    gen = generator()
    pick = np.random.default_rng(0).choice(len(g["sc_a"]), 400, replace=False)
    s, c, _, _ = gen.expect_sincos(g["sc_a"][pick])
    assert np.all(same_bits(s, g["sc_sin"][pick])) and np.all(same_bits(c, g["sc_cos"][pick]))
    pick = np.random.default_rng(1).choice(len(g["at_y"]), 400, replace=False)
    r, _ = gen.expect_atan2(g["at_y"][pick], g["at_x"][pick])
    assert np.all(same_bits(r, g["at_r"][pick]))
