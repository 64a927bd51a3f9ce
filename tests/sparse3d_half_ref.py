"""Test helper (not a test): what the 16-bit sparse 3-D path is held to.

    round_to(x, dtype)            fp64 -> the nearest bf16 / fp16 value (ties to even), as fp64: ONE rounding, straight from fp64
    pack_weight_h_ref(w, dtype)   numpy statement of the fragment order of pnx_sp3_conv_h's weights
    U, FLOOR                      unit roundoff and absolute floor per element type
"""
import numpy as np
import torch

# significand bits (hidden one included), smallest exponent of a normal number, largest finite value
_FMT = {torch.bfloat16: (8, -126, float(torch.finfo(torch.bfloat16).max)), torch.float16: (11, -14, 65504.0)}
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}      # one rounding to nearest: |y - v| <= U |v|
FLOOR = {torch.bfloat16: 1e-30, torch.float16: 6e-8}            # fp16: the spacing of its subnormals, 2^-24


def round_to(x, dtype):
    """x (fp64 numpy array or torch tensor) rounded once to the nearest value of `dtype`, ties to even, returned in fp64 (same kind as x).
    A value is m * 2^e with 0.5 <= |m| < 1 (frexp); its neighbours in the format are spaced q = 2^(max(e, emin + 1) - bits) apart, so the
    rounding is rint(x / q) * q -- x / q and the product are exact in fp64, rint rounds half to even.  Past the largest finite value: inf."""
    bits, emin, big = _FMT[dtype]
    if torch.is_tensor(x):
        x = x.double()
        _, e = torch.frexp(x)
        q = torch.exp2((torch.clamp(e, min=emin + 1) - bits).double())
        y = torch.round(x / q) * q
        return torch.where(y.abs() > big, torch.copysign(torch.full_like(y, float("inf")), y), y)
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)
    q = np.exp2((np.maximum(e, emin + 1) - bits).astype(np.float64))
    y = np.rint(x / q) * q
    return np.where(np.abs(y) > big, np.copysign(np.inf, y), y)


def pack_weight_h_ref(w, dtype):
    """(Cout, kd, kh, kw, Cin) -> (S, ceil(Cout / 16), 64, 8) fp64 holding values of `dtype`: K = (tap, channel padded to a multiple of 8) in steps
    of 32; element e of lane l of tile j of step s is w[16 j + (l & 15)][tap][c] with 32 s + 8 (l >> 4) + e = tap * cpad + c, else zero."""
    w = np.asarray(w, np.float64)
    co, ci = w.shape[0], w.shape[-1]
    wt = w.reshape(co, -1, ci)
    T = wt.shape[1]
    cpad = (ci + 7) // 8 * 8
    S, nt = (T * cpad + 31) // 32, (co + 15) // 16
    out = np.zeros((S, nt, 64, 8))
    for s in range(S):
        for j in range(nt):
            for l in range(64):
                for e in range(8):
                    k = 32 * s + 8 * (l >> 4) + e
                    tap, c, o = k // cpad, k % cpad, 16 * j + (l & 15)
                    if tap < T and c < ci and o < co:
                        out[s, j, l, e] = wt[o, tap, c]
    return round_to(out, dtype)
