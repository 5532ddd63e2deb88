"""Exactly summable conv operands and a numpy mirror of conv3x3_flow's rounding steps (tests/test_gpu_exact.py).

On the operand grid below every partial sum of a 3x3 convolution -- bias, products, the identity tap of the residual forms -- is
an integer multiple of 2^-16 below 2^8 in magnitude, i.e. exact in fp32 (24 bits) whatever the summation order, MFMA-internal
included.  What is left of the kernel's arithmetic are the rounding steps of its epilogues (conv_flow.hip row_emit / row_pack /
row_emit4), which the functions here restate one by one; a kernel is then right when its output equals the mirror BIT FOR BIT.

Operands:  x = k/64, |k| <= 128 (fp16-normal, |x| <= 2);  w = j/1024, |j| <= 32;  b = odd multiples of 2^-16 in [2^-5, 4) (never
fp16-representable: a bias rounded to fp16 shows).  Worst case 1728 * 2/32 + 4 + 5 * 2 = 122 < 2^8.
"""
import numpy as np
import torch
import torch.nn.functional as F

X_EXP, W_EXP = 6, 10          # x on the 2^-6 grid, w on the 2^-10 grid
ACC_EXP = X_EXP + W_EXP       # products, biases and every partial sum on the 2^-16 grid
ACC_LIMIT = 2.0 ** (24 - ACC_EXP)  # |partial sum| < 2^8: an integer multiple of 2^-16 with < 24 significant bits
SLOPE = np.float32(0.2)       # LeakyReLU slope as the kernel holds it (fp32 0.2f)
F16_MIN_NORMAL = 2.0 ** -14


# ---- operands ---------------------------------------------------------------------------------------------
def grid_x(rng, shape, kmax=128):
    return (rng.integers(-kmax, kmax + 1, shape) / 2.0 ** X_EXP).astype(np.float16)


def grid_w(rng, shape, jmax=32):
    return (rng.integers(-jmax, jmax + 1, shape) / 2.0 ** W_EXP).astype(np.float32)


def grid_b(rng, n, bmax=4.0):
    """Odd multiples of 2^-16 with 2^-5 <= |b| < bmax: 11 bits are not enough for any of them."""
    m = rng.integers(2 ** (ACC_EXP - 6), int(bmax * 2 ** (ACC_EXP - 1)), n) * 2 + 1
    b = (np.where(rng.integers(0, 2, n) == 1, -m, m) / 2.0 ** ACC_EXP).astype(np.float32)
    assert (b.astype(np.float16).astype(np.float32) != b).all()
    return b


def _on_grid(a, e):
    s = np.asarray(a, dtype=np.float64) * 2.0 ** e
    return bool((s == np.round(s)).all())


def assert_exact(x, w, b, idt_coef=0.0, ups=False):
    """Every partial sum of conv3x3(x, w) + b (+ idt_coef * x[:cout], the residual forms' identity tap) is exact in fp32, in any
    order: the operands are on the grid, fp16-normal (or zero) and fp16-representable, and the sum of the magnitudes of every term of
    an output value stays below 2^8.  Raises AssertionError otherwise."""
    x64 = np.asarray(x, dtype=np.float64)
    w64 = np.asarray(w, dtype=np.float64)
    b64 = np.asarray(b, dtype=np.float64)
    assert _on_grid(x64, X_EXP), "x is not on the 2^-%d grid" % X_EXP
    assert _on_grid(w64, W_EXP), "w is not on the 2^-%d grid" % W_EXP
    assert _on_grid(b64, ACC_EXP), "b is not on the 2^-%d grid" % ACC_EXP
    for name, t in (("x", x64), ("w", w64)):
        nz = np.abs(t[t != 0])
        assert (nz >= F16_MIN_NORMAL).all(), "%s has fp16 denormals" % name
        assert (t.astype(np.float16).astype(np.float64) == t).all(), "%s is not fp16-representable" % name
    assert (b64.astype(np.float32).astype(np.float64) == b64).all(), "b is not fp32-representable"
    xmax = np.abs(x64).reshape(x64.shape[0], -1).max(axis=1)          # per input channel
    bound = np.abs(w64).sum(axis=(2, 3)) @ xmax + np.abs(b64)           # per output channel
    if idt_coef:
        bound = bound + abs(float(idt_coef)) * xmax[: w64.shape[0]]
    assert bound.max() < ACC_LIMIT, "worst-case sum %g needs more than 24 bits on the 2^-%d grid" % (bound.max(), ACC_EXP)
    return float(bound.max())


# ---- exact sums ------------------------------------------------------------------------------------------------
def conv_sum(x, w, b, ups=False):
    """conv3x3(x, w) + b in float64, zero padding (exact on the grid: every term and partial sum is a multiple of 2^-16 far below
    2^53).  Also checks that the sum is exact in fp32."""
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))[None]
    if ups:
        xt = xt.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    y = F.conv2d(xt, torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)),
                 torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64)), padding=1)[0].numpy()
    assert (y.astype(np.float32).astype(np.float64) == y).all()
    return y


def idt_coef(s1):
    """The identity tap's coefficient as the kernel multiplies it: fp16(fp32(1 / s1)) (engine res1_coef, conv_flow.hip RSR_IDTAP)."""
    return float(np.float16(np.float32(1.0) / np.float32(s1)))


# ---- rounding steps ----------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fp32 fma of fp32 operands: the exact a*b + c rounded ONCE to fp32, to nearest even.  a*b is exact in float64 (24 + 24 bits); the
    sum is carried exactly as s + e (TwoSum), and e decides the rounding where s itself falls on an fp32 midpoint -- the one case in
    which rounding s instead of the exact sum could go the other way."""
    a, b, c = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (a, b, c))
    p = a * b
    assert (p / b == a)[b != 0].all()
    s = p + c
    bp = s - c
    e = (p - bp) + (c - (s - bp))
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    other = np.nextafter(r, np.where(s > r64, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    tie = (s != r64) & (np.abs(s - r64) == np.abs(other.astype(np.float64) - s))
    away = tie & (e != 0) & (np.sign(other.astype(np.float64) - s) == np.sign(e))
    return np.where(away, other, r).astype(np.float32)


def f16(v):
    """fp32 -> fp16, round to nearest even (numpy's casts are correctly rounded)."""
    return np.asarray(v, dtype=np.float32).astype(np.float16)


def lrelu32(f):
    """med3(f, fl32(f * 0.2f), +inf) = max(f, fl32(f * 0.2f)) in fp32 (conv_flow.hip row_emit / row_pack)."""
    f = np.asarray(f, dtype=np.float32)
    return np.maximum(f, f * SLOPE)


def epi1(acc, lrelu):
    """EPI 1: fp16(act(acc)), acc = the exact fp32 sum (bias included)."""
    f = np.asarray(acc, dtype=np.float32)
    return f16(lrelu32(f) if lrelu else f)


def epi2(acc, s1, r=None, s2=1.0):
    """EPI 2: v = fp16(fl32(s1 * acc)) -- acc includes the identity tap x * idt_coef(s1) for the conv5 forms -- then, with a second
    residual, v = fp16(fma32(v, s2, r)) (the trunk form runs as s1 = 1, r = its residual, s2 = 1: engine launch_conv_flow)."""
    v = f16(np.asarray(acc, dtype=np.float32) * np.float32(s1))
    if r is not None:
        v = f16(fma32(v.astype(np.float32), np.float32(s2), np.asarray(r, dtype=np.float16).astype(np.float32)))
    return v


_E5M2 = None


def e5m2_values():
    """The 256 e5m2 (bf8) codes as float64 (NaN / inf codes included as NaN / inf)."""
    global _E5M2
    if _E5M2 is None:
        _E5M2 = (np.arange(256, dtype=np.uint16) << 8).view(np.float16).astype(np.float64)
    return _E5M2


def bf8_decode(b):
    return e5m2_values()[np.asarray(b, dtype=np.uint8)].astype(np.float32)


def bf8_rne(t):
    """fp32 -> e5m2 byte: the nearest finite value, ties to the even code; the sign kept for zeros (|t| far below the e5m2 range
    here: never saturates)."""
    t = np.asarray(t, dtype=np.float32).astype(np.float64)
    vals = e5m2_values()[:124]                      # +0 .. 57344 (codes 0x00 .. 0x7b; 0x7c.. are inf / NaN)
    mag = np.abs(t).ravel()
    assert (mag < 57344).all()
    hi_idx = np.searchsorted(vals, mag, side="left")  # first value >= mag
    hi_idx = np.minimum(hi_idx, len(vals) - 1)
    lo_idx = np.maximum(hi_idx - 1, 0)
    dlo, dhi = mag - vals[lo_idx], vals[hi_idx] - mag
    pick = np.where(dhi < dlo, hi_idx, np.where(dlo < dhi, lo_idx, np.where(hi_idx % 2 == 0, hi_idx, lo_idx)))
    pick = np.where(vals[hi_idx] == mag, hi_idx, pick)
    code = pick.astype(np.uint8) | (np.signbit(t.ravel()).astype(np.uint8) << 7)
    return code.reshape(t.shape)


def split_hi_lo(f):
    """EPI 4 / 5 output: hi = fp16(f), lo = bf8((f - hi) * 2048) (the difference and the scaling are exact in fp32)."""
    f = np.asarray(f, dtype=np.float32)
    hi = f16(f)
    t = (f - hi.astype(np.float32)) * np.float32(2048.0)
    assert (t.astype(np.float64) == (f.astype(np.float64) - hi.astype(np.float64)) * 2048.0).all()
    return hi, bf8_rne(t)


def epi_precise(acc, s1, x_lo=None, r_hi=None, r_lo=None, s2=1.0):
    """EPI 4 / 5 (conv_flow.hip row_emit4), all in fp32:  f = fl32(fl32(s1 * acc) + bf8(x_lo) / 2048)
    [;  f = fl32(fl32(f * s2 + r_hi) + bf8(r_lo) / 2048)]  ->  split_hi_lo(f).  Absent lo planes read as zeros; the trunk / conv_first
    forms run as s1 = 1 with their residual as the second one (s2 = 1)."""
    zeros = np.zeros(np.shape(acc), dtype=np.uint8)
    inv = np.float32(1.0 / 2048.0)
    f = fma32(bf8_decode(zeros if x_lo is None else x_lo), inv, np.asarray(acc, dtype=np.float32) * np.float32(s1))
    if r_hi is not None:
        f = fma32(f, np.float32(s2), np.asarray(r_hi, dtype=np.float16).astype(np.float32))
        f = fma32(bf8_decode(zeros if r_lo is None else r_lo), inv, f)
    return split_hi_lo(f)


# ---- impulses -------------------------------------------------------------------------------------------------
def impulse_input(cin, h, w, hits):
    """hits: [(c, y0, x0)] -> fp16 [cin][h][w], 1.0 at each hit.  The 3x3 footprints must not overlap."""
    x = np.zeros((cin, h, w), dtype=np.float16)
    seen = np.zeros((h, w), dtype=bool)
    for c, y0, x0 in hits:
        fy, fx = slice(max(y0 - 1, 0), y0 + 2), slice(max(x0 - 1, 0), x0 + 2)
        assert not seen[fy, fx].any(), "overlapping impulse footprints at %s" % ((c, y0, x0),)
        seen[fy, fx] = True
        x[c, y0, x0] = 1.0
    return x


def impulse_sum(w, b, h, wd, hits):
    """The exact pre-activation output for impulse_input(...): b everywhere, b + w[:, c, 1 - oy, 1 - ox] at (y0 + oy, x0 + ox) for
    oy, ox in {-1, 0, 1} inside the plane -- tap orientation, halo and zero padding without any conv arithmetic."""
    cout = w.shape[0]
    out = np.broadcast_to(np.asarray(b, dtype=np.float64)[:, None, None], (cout, h, wd)).copy()
    for c, y0, x0 in hits:
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                y, xx = y0 + oy, x0 + ox
                if 0 <= y < h and 0 <= xx < wd:
                    out[:, y, xx] += w[:, c, 1 - oy, 1 - ox]
    return out


def grid_lo(rng, hi):
    """Random bf8 residue bytes for an fp16 tensor (the precise stream's lo planes): a random sign and 2-bit mantissa, an exponent field
    1..5 below hi's (clamped to the normal range) -- what a residue of at most half an ulp of hi looks like."""
    hi = np.asarray(hi, dtype=np.float16)
    e_hi = ((hi.view(np.uint16) >> 10) & 31).astype(np.int64)
    e_lo = np.clip(e_hi - rng.integers(1, 6, hi.shape), 1, 30)
    return ((rng.integers(0, 2, hi.shape) << 7) | (e_lo << 2) | rng.integers(0, 4, hi.shape)).astype(np.uint8)


def impulse_sets(h, w, positions):
    """Split impulse positions into groups whose 3x3 footprints do not overlap (one launch per group)."""
    sets = []
    for y, x in positions:
        assert 0 <= y < h and 0 <= x < w, (y, x)
        for s in sets:
            if all(abs(y - yy) >= 3 or abs(x - xx) >= 3 for yy, xx in s):
                s.append((y, x))
                break
        else:
            sets.append([(y, x)])
    return sets
