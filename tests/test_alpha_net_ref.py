"""tests/alpha_net_ref.py against hand-checked values, and the binding's side of option "alpha_net" (no GPU)."""
from fractions import Fraction

import numpy as np
import pytest

import alpha_net_ref as A
import realsr_ncnn_vulkan_amd as R

F32 = np.float32


def bits(x):
    return F32(np.uint32(x).view(np.float32))


def test_three_ones_give_exactly_one():
    """(1 + 1 + 1) * fp32(1/3): fp32(1/3) = 0x3eaaaaab lies ABOVE 1/3, 3 * it = 1 + 2^-25 exactly, a tie that rounds to the even 1.0 -- and
    the min of step 1 would catch anything above.  255 / 65535 leave."""
    assert A.THIRD.view(np.uint32) == 0x3EAAAAAB
    m = A.mean3(F32(1), F32(1), F32(1))
    assert m.dtype == F32 and m == F32(1) and (F32(3) * A.THIRD).astype(F32) == F32(1)
    one = np.ones((3, 2, 2), F32)
    assert np.array_equal(A.alpha(one, 8), np.full((2, 2), 255, np.uint8))
    assert np.array_equal(A.alpha(one, 16), np.full((2, 2), 65535, np.uint16))


def test_all_zero_gives_zero():
    z = np.zeros((3, 3, 5), F32)
    assert np.array_equal(A.alpha(z, 8), np.zeros((3, 5), np.uint8)) and np.array_equal(A.alpha(z, 16), np.zeros((3, 5), np.uint16))
    assert A.alpha(z, 8).dtype == np.uint8 and A.alpha(z, 16).dtype == np.uint16


def test_mean_is_rounded_step_by_step():
    """The sum is rounded twice, in the order (A0 + A1) + A2, then the product: with A0 = 1, A1 = A2 = 2^-24 the first sum is a tie that
    stays at 1, and so does the second -- any other order or a wider accumulator gives 1 + 2^-23 before the product."""
    t = F32(2.0 ** -24)
    assert A.mean3(F32(1), t, t) == (F32(1) * A.THIRD).astype(F32)
    assert A.mean3(t, t, F32(1)) == (F32(1 + 2.0 ** -23) * A.THIRD).astype(F32)
    assert A.mean3(F32(1), t, t) != A.mean3(t, t, F32(1))


# (bit pattern of m, depth, the stored sample): code boundaries at which the product m * max, rounded by itself, lands ON n - 0.5 although
# the exact product lies below it (or, first entry, the sum lands on n) -- the stored sample is n where exact arithmetic gives n - 1.
BORDERLINE = [(0x3B008080, 8, 1), (0x3F010101, 8, 129), (0x3F020202, 8, 130), (0x3F7F7F7F, 8, 255),
              (0x37000080, 16, 1), (0x37C000C0, 16, 2), (0x3F008000, 16, 32896), (0x3F7F7F7F, 16, 65407)]


@pytest.mark.parametrize("pattern,depth,want", BORDERLINE)
def test_borderline_store_values(pattern, depth, want):
    """Hand-checked borderline values of the store.  For each, in exact rational arithmetic, m * max + 0.5 lies just BELOW `want`: the fp32
    rule, which rounds the product and the sum each by itself, stores `want`; floor of the exact value stores want - 1.

    On the contracted form: an exhaustive search over the fp32 values within 8 ulp of every code boundary (n - 0.5) / max, n = 1 .. max,
    for max = 255 and 65535, found NO m in [0, 1] for which floor(fma(m, max, 0.5)) differs from the separately rounded store -- the two
    could part only where the product and the sum fall into different binades (n = 1) or on an exact tie, and no fp32 m hits either.  The
    rule is pinned (mul_rn / add_rn) all the same; what this test holds it to is that it is the fp32 rule and not exact arithmetic, and that
    the single-rounded form agrees on these very values."""
    m = bits(pattern)
    top = 255 if depth == 8 else 65535
    assert 0 <= m <= 1
    assert int(A.store(m, depth)) == want
    exact = Fraction(float(m)) * top + Fraction(1, 2)
    assert exact < want and int(exact) == want - 1            # exact arithmetic would store want - 1
    p32 = (m * F32(top)).astype(F32)
    prod = Fraction(float(p32))
    # the product was rounded UP onto n - 0.5 -- or (n = 1 at 8 bits: the product lies a binade below the sum) the sum onto n
    assert (prod == Fraction(2 * want - 1, 2) and prod > Fraction(float(m)) * top) or (prod + Fraction(1, 2) < want and (p32 + F32(0.5)).astype(F32) == want)
    fused = F32(float(exact))                                  # m * max + 0.5 is exact in double: ONE rounding to fp32 = the fma
    assert int(np.floor(fused)) == want


def test_store_clamps():
    assert int(A.store(F32(1), 8)) == 255 and int(A.store(F32(1), 16)) == 65535
    assert int(A.store(F32(-0.25), 8)) == 0 and int(A.store(F32(2), 8)) == 255 and int(A.store(F32(2), 16)) == 65535


def test_gray():
    img = np.arange(2 * 3 * 4, dtype=np.uint16).reshape(2, 3, 4)
    g = A.gray(img)
    assert g.shape == (2, 3, 3) and g.dtype == np.uint16 and all(np.array_equal(g[:, :, q], img[:, :, 3]) for q in range(3))


def test_binding_exposes_alpha_net():
    """A property of RealSR like yuv_siting, and the header names the option and its stat."""
    assert isinstance(R.RealSR.__dict__["alpha_net"], property) and R.RealSR.alpha_net.fset is not None
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "realsr_hip.h")) as fh:
        text = fh.read()
    assert '"alpha_net"' in text and '"alpha_tiles"' in text
