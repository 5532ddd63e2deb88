"""CPU self-tests of tests/exact_conv.py, the exact-operand mirror that tests/test_gpu_exact.py holds conv3x3_flow to."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_conv as X
import oracle


def test_grid_operands_pass_the_exactness_check_at_the_worst_case():
    rng = np.random.default_rng(1)
    x = np.full((192, 4, 5), 2.0, np.float16)                      # |k| = 128 everywhere
    w = np.full((64, 192, 3, 3), 32 / 1024.0, np.float32)          # |j| = 32 everywhere
    b = np.full(64, 4.0 - 2.0 ** -16, np.float32)
    assert X.assert_exact(x, w, b, idt_coef=X.idt_coef(0.2)) == pytest.approx(1728 * 2 / 32 + 4 + 10, abs=1e-3)
    X.assert_exact(X.grid_x(rng, (64, 5, 6)), X.grid_w(rng, (32, 64, 3, 3)), X.grid_b(rng, 32))


def test_grid_assertion_rejects_operands_that_would_not_sum_exactly():
    rng = np.random.default_rng(2)
    x, w, b = X.grid_x(rng, (192, 4, 5)), X.grid_w(rng, (64, 192, 3, 3)), X.grid_b(rng, 64)
    with pytest.raises(AssertionError, match="24 bits"):
        X.assert_exact(x, w * 8, b)                                # up to 1/4: 1728 * 2/4 > 2^8
    with pytest.raises(AssertionError, match="grid"):
        X.assert_exact(x, w + 2.0 ** -12, b)                       # products on the 2^-18 grid
    with pytest.raises(AssertionError, match="grid"):
        X.assert_exact((x.astype(np.float32) + 2.0 ** -8).astype(np.float16), w, b)
    with pytest.raises(AssertionError, match="grid"):
        X.assert_exact(x, w, b + np.float32(2.0 ** -18))
    # what the check guards against: off the grid, two summation orders of the same fp32 terms disagree; on it they cannot
    p = (rng.standard_normal(1728).astype(np.float16).astype(np.float32) * rng.standard_normal(1728).astype(np.float16).astype(np.float32))
    assert np.cumsum(p, dtype=np.float32)[-1] != np.cumsum(p[::-1], dtype=np.float32)[-1]
    q = x[:, 0, 0].astype(np.float32).repeat(9) * w[0].ravel()
    assert np.cumsum(q, dtype=np.float32)[-1] == np.cumsum(q[::-1], dtype=np.float32)[-1] == q.astype(np.float64).sum()


def test_biases_are_not_fp16_representable_and_round_trip_fp32():
    b = X.grid_b(np.random.default_rng(3), 4096)
    assert (np.abs(b) >= 2.0 ** -5).all() and (np.abs(b) < 4).all()
    assert (b.astype(np.float16).astype(np.float32) != b).all()


@pytest.mark.parametrize("lrelu", [False, True])
def test_mirror_reproduces_the_oracle_conv_bit_for_bit(lrelu):
    rng = np.random.default_rng(4 + lrelu)
    x, w, b = X.grid_x(rng, (96, 13, 21)), X.grid_w(rng, (32, 96, 3, 3)), X.grid_b(rng, 32)
    X.assert_exact(x, w, b)
    acc = X.conv_sum(x, w, b)
    ref = oracle.conv3x3(x.astype(np.float32), w, b, 2 if lrelu else 0, 0.2)
    mine = X.lrelu32(acc) if lrelu else acc.astype(np.float32)
    assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(X.epi1(acc, lrelu).view(np.uint16), ref.astype(np.float16).view(np.uint16))


def test_float16_casts_round_correctly():
    # float64 -> float16 directly: 1 + 2^-11 + 2^-40 is above the midpoint; through fp32 it would become the midpoint (ties: 1.0)
    v = 1.0 + 2.0 ** -11 + 2.0 ** -40
    assert float(np.float64(v).astype(np.float16)) == 1.0 + 2.0 ** -10
    assert float(np.float32(v).astype(np.float16)) == 1.0
    assert float(X.f16(np.float32(1.0 + 2.0 ** -11))) == 1.0 and float(X.f16(np.float32(1.0 + 3 * 2.0 ** -11))) == 1.0 + 2.0 ** -9


def test_fma32_rounds_once():
    a, b, c = np.float32(1.0 + 2.0 ** -12), np.float32(1.0 + 2.0 ** -12), np.float32(-1.0)
    assert float(X.fma32(a, b, c)) == 2.0 ** -11 + 2.0 ** -24          # the product's low bits survive
    assert float(a * b + c) == 2.0 ** -11                             # two roundings lose them
    # beyond float64: (1 + 2^-23) * (1 - 2^-23) * 2^-24 + (1 + 2^-23) = 1 + 3 * 2^-24 - 2^-70 lies just below an fp32 midpoint, which
    # float64 rounds it onto (and the midpoint's even neighbour is the upper one)
    one = np.float32(1.0)
    a, b, c = np.float32(1.0 + 2.0 ** -23), np.float32((1.0 - 2.0 ** -23) * 2.0 ** -24), np.float32(1.0 + 2.0 ** -23)
    assert float(X.fma32(a, b, c)) == 1.0 + 2.0 ** -23
    assert float(np.float64(a) * np.float64(b) + np.float64(c)) == 1.0 + 3 * 2.0 ** -24 and float(np.float32(1.0 + 3 * 2.0 ** -24)) == 1.0 + 2.0 ** -22
    assert float(X.fma32(np.float32(1.0 + 2.0 ** -23), np.float32(2.0 ** -24), one)) == 1.0 + 2.0 ** -23   # above the tie: up
    assert float(X.fma32(np.float32(1.0 - 2.0 ** -24), np.float32(2.0 ** -24), one)) == 1.0                # below the tie: down
    assert float(X.fma32(np.float32(1.0), np.float32(2.0 ** -24), one)) == 1.0                            # on it: to even
    assert float(X.fma32(np.float32(1.0), np.float32(3 * 2.0 ** -24), one)) == 1.0 + 2.0 ** -22


def test_bf8_rounding_is_nearest_even():
    vals = X.e5m2_values()
    assert vals[0x3C] == 1.0 and vals[0x7B] == 57344.0 and vals[0x01] == 2.0 ** -16
    for code in range(1, 0x7B):
        lo, hi = vals[code], vals[code + 1]
        mid = np.float32((lo + hi) / 2)
        want = code if code % 2 == 0 else code + 1
        assert X.bf8_rne(mid) == want, hex(code)
        assert X.bf8_rne(np.float32(lo + (hi - lo) * 0.25)) == code and X.bf8_rne(np.float32(lo + (hi - lo) * 0.75)) == code + 1
        assert X.bf8_rne(-mid) == want | 0x80
    assert X.bf8_rne(np.float32(0.0)) == 0 and X.bf8_rne(np.float32(2.0 ** -18)) == 0 and X.bf8_rne(np.float32(-2.0 ** -18)) == 0x80
    # torch's own e5m2 cast (round to nearest even) agrees on a dense sample
    t = np.random.default_rng(5).standard_normal(20000).astype(np.float32) * np.float32(2.0) ** np.random.default_rng(6).integers(-18, 10, 20000).astype(np.float32)
    ref = torch.from_numpy(t).to(torch.float8_e5m2).view(torch.uint8).numpy()
    assert np.array_equal(X.bf8_rne(t), ref)


def test_split_hi_lo_reconstructs_within_the_bf8_residue():
    f = (np.random.default_rng(7).standard_normal(10000) * 8).astype(np.float32)
    hi, lo = X.split_hi_lo(f)
    back = hi.astype(np.float64) + X.bf8_decode(lo).astype(np.float64) / 2048
    assert (np.abs(back - f) <= np.abs(f) * 2.0 ** -13 + 2.0 ** -27).all()


def test_impulse_expectation_matches_conv2d():
    rng = np.random.default_rng(8)
    h, wd = 37, 44
    w, b = X.grid_w(rng, (32, 64, 3, 3)), X.grid_b(rng, 32)
    hits = [(0, 0, 0), (5, 0, wd - 1), (17, h - 1, 0), (63, h - 1, wd - 1), (33, 15, 31), (40, 16, 35), (2, 20, 4), (9, 7, 12)]
    x = X.impulse_input(64, h, wd, hits)
    ref = F.conv2d(torch.from_numpy(x.astype(np.float64))[None], torch.from_numpy(w.astype(np.float64)),
                   torch.from_numpy(b.astype(np.float64)), padding=1)[0].numpy()
    assert np.array_equal(X.impulse_sum(w, b, h, wd, hits), ref)
    with pytest.raises(AssertionError, match="overlapping"):
        X.impulse_input(64, h, wd, [(0, 5, 5), (1, 7, 7)])


def test_residual_mirror_forms():
    """EPI 2 at a power-of-two scale only rounds at the fp16 stores; at 0.2 the fp32 product is rounded first (and that differs from
    rounding the exact product to fp16 in one step on some values, which the GPU test relies on to see a fused conversion)."""
    rng = np.random.default_rng(9)
    x, w, b = X.grid_x(rng, (192, 40, 60)), X.grid_w(rng, (64, 192, 3, 3)), X.grid_b(rng, 64)
    acc = X.conv_sum(x, w, b)
    for s1 in (0.25, 0.5):
        a = acc + X.idt_coef(s1) * x[:64].astype(np.float64)
        assert np.array_equal(X.epi2(a, s1).view(np.uint16), (a * s1).astype(np.float16).view(np.uint16))
    a = acc + X.idt_coef(0.2) * x[:64].astype(np.float64)
    two = X.epi2(a, 0.2)
    one = (a * np.float64(np.float32(0.2))).astype(np.float16)        # the exact product, one rounding
    assert 0 < (two != one).sum() < 0.01 * two.size
