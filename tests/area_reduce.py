"""The numpy reference of rsr_set_out_ratio (include/realsr_hip.h, "The definition, exact"), shared by tests/test_out_ratio.py and
tests/test_gpu_out_ratio.py: steps 1 to 4 in float32 and in the stated order.  The sibling of tests/box_reduce.py, whose u8_expected
serves step 5 here as well."""
import math

import numpy as np

from box_reduce import u8_expected  # noqa: F401  (step 5: the uint8 rule is the one of "out_scale")

F32 = np.float32

# every ratio rsr_set_out_ratio takes, in lowest terms: d in 1..4, 1 <= n / d <= 4
RATIOS = [(n, d) for d in (1, 2, 3, 4) for n in range(d, 4 * d + 1) if math.gcd(n, d) == 1]
BOX = [(4, 1), (2, 1), (1, 1)]                   # option "out_scale" 4 / 2 / 1: the box kernels
GENERIC = [r for r in RATIOS if r not in BOX]    # the 16 ratios postproc_tiles_area serves


def taps(X, n, d):
    """[(i, g_i)] of output pixel X along one axis: on the grid where x4 pixel i covers [i n, (i + 1) n), X covers [X L, (X + 1) L),
    L = 4 d; g_i is the overlap."""
    L = 4 * d
    i0, i1 = X * L // n, ((X + 1) * L - 1) // n
    return [(i, min((X + 1) * L, (i + 1) * n) - max(X * L, i * n)) for i in range(i0, i1 + 1)]


def _along_x(c, n, d):
    """Steps 2 / 3 along the last axis: H = g_i0 * c_i0, then H = H + g_i * c_i in ascending i; float32 operands and intermediates."""
    N = c.shape[-1]
    assert N * n % (4 * d) == 0
    out = np.empty(c.shape[:-1] + (N * n // (4 * d),), dtype=np.float32)
    for X in range(out.shape[-1]):
        t = taps(X, n, d)
        H = F32(t[0][1]) * c[..., t[0][0]]
        for i, g in t[1:]:
            H = H + F32(g) * c[..., i]
        assert H.dtype == np.float32
        out[..., X] = H
    return out


def area_reduce(v, n, d, top=1.0):
    """v: float32 (..., 4h, 4w), the x4 image; n / d in lowest terms with 4h * n and 4w * n multiples of 4 d.  Returns the float32
    (..., h n / d, w n / d) array of min(V * fp32(1 / (16 d^2)), top): c = min(max(v, 0), top), horizontally first, then vertically.
    top = 1 for colour; 255 for alpha (whose values are in 0 .. 255)."""
    v = np.asarray(v)
    assert v.dtype == np.float32 and math.gcd(n, d) == 1
    c = np.minimum(np.maximum(v, F32(0)), F32(top))
    H = _along_x(c, n, d)
    V = np.swapaxes(_along_x(np.ascontiguousarray(np.swapaxes(H, -1, -2)), n, d), -1, -2)
    m = np.minimum(V * F32(1.0 / (16.0 * d * d)), F32(top))
    assert m.dtype == np.float32
    return np.ascontiguousarray(m)


def exact_area_mean(v, n, d, top=1.0):
    """The same average in float64 with exact rational weights: the area mean of the clamped x4 image over every output pixel."""
    c = np.clip(np.asarray(v, dtype=np.float64), 0.0, top)

    def along(a):
        out = np.zeros(a.shape[:-1] + (a.shape[-1] * n // (4 * d),))
        for X in range(out.shape[-1]):
            for i, g in taps(X, n, d):
                out[..., X] += g * a[..., i]
        return out
    return np.swapaxes(along(np.swapaxes(along(c), -1, -2)), -1, -2) / (16.0 * d * d)


def check_u8(gots, ds, what=""):
    """gots: uint8 HWC outputs; ds: their float32 references m, planar.  The rule of tests/test_gpu_out_scale.py over the pooled elements."""
    g = np.concatenate([got.transpose(2, 0, 1).reshape(-1) for got in gots])
    want, near = u8_expected(np.concatenate([d.reshape(-1) for d in ds]))
    print("%suint8: %d elements, %d left out (within 2^-14 of a rounding boundary), %d differ" % (what, g.size, near.sum(), ((g != want) & ~near).sum()))
    assert g.size >= 20000, g.size
    assert near.mean() <= 1e-3, near.mean()
    assert np.array_equal(g[~near], want[~near])
    assert (np.abs(g.astype(int) - want.astype(int))[near] <= 1).all()
