"""CPU: the PNX_TRAIN_F32_PIECES switch of the fp32 training graph (models.train_f32_pieces) and the numpy statement of the three-piece bf16 split
(pnx_split3_f32: hi = RNE(x), mid = RNE(x - hi), lo = RNE(x - hi - mid)) -- exact for every fp32 value with |x| >= 2^-100."""
import numpy as np
import pytest


def bf16(x):
    """round-to-nearest-even fp32 -> bf16 -> fp32 (finite values)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split3(x):
    x = np.asarray(x, np.float32)
    hi = bf16(x)
    r = (x - hi).astype(np.float32)
    mid = bf16(r)
    lo = bf16((r - mid).astype(np.float32))
    return hi, mid, lo


def test_switch_parsing(monkeypatch):
    from pillarnext_amd import ops
    from pillarnext_amd.models import train_f32_pieces

    monkeypatch.delenv("PNX_TRAIN_F32_PIECES", raising=False)
    assert train_f32_pieces() == 2
    for v, want in (("2", 2), ("3", 3), (" 3", 3)):
        monkeypatch.setenv("PNX_TRAIN_F32_PIECES", v)
        assert train_f32_pieces() == want
    for v in ("1", "4", "", "x", "2.0", "three"):
        monkeypatch.setenv("PNX_TRAIN_F32_PIECES", v)
        with pytest.raises(ops.PnxError):
            train_f32_pieces()


def test_numpy_split3_is_exact():
    rng = np.random.default_rng(0)
    n = 200_000
    e = rng.integers(-100, 120, n)
    x = (rng.choice([-1.0, 1.0], n) * (1.0 + rng.random(n)) * np.exp2(e.astype(np.float64))).astype(np.float32)
    x[:3] = [0.0, -0.0, 2.0 ** -100]
    hi, mid, lo = split3(x)
    for p in (hi, mid, lo):   # each piece is a bf16 value: the low 16 bits are zero
        assert not np.any(p.view(np.uint32) & 0xFFFF)
    assert np.array_equal(hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64), x.astype(np.float64))
    assert np.array_equal(hi, bf16(x))
    # two pieces are not exact: 16 of fp32's 24 bits
    h2 = bf16(x)
    l2 = bf16((x - h2).astype(np.float32))
    assert not np.array_equal(h2.astype(np.float64) + l2, x.astype(np.float64))
