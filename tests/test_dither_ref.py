"""tests/dither_ref.py against the text of include/realsr_hip.h ("dither") and against the properties the header draws from the rule.  No
GPU: the tie between the reference and the kernels is tests/test_gpu_dither.py."""
import os

import numpy as np

import realsr_ncnn_vulkan_amd as R

import dither_ref as D

F = np.float32


def test_header_holds_the_rule():
    text = open(os.path.join(R.INCLUDE_DIR, "realsr_hip.h")).read()
    for needle in ('"dither"', "0xC13FA9A9u", "0x91E10DA5u", "h >> 25", "(2k + 1)", "floor(add_rn(mul_rn(d, M), theta))",
                   "floor(add_rn(mul_rn(v, scale), add_rn(offset, theta)))"):
        assert needle in text, needle


def test_first_values():
    t = D.theta(8, 4)
    assert t.dtype == np.float32 and t.shape == (4, 8)
    assert t[0, :4].tolist() == [1 / 256, 193 / 256, 131 / 256, 67 / 256]
    assert t[1, 0] == 145 / 256
    # wrap-around: far from the origin the products leave 32 bits, and the value is still the rule's
    for x, y in ((70001, 3), (2, 50003)):
        k = ((x * D.CX + y * D.CY) % (1 << 32)) >> 25
        assert D.theta(x + 1, y + 1)[y, x] == (2 * k + 1) / 256


def test_every_value_equally_often():
    t = D.theta(256, 256)
    vals, counts = np.unique(t, return_counts=True)
    assert len(vals) == 128 and np.array_equal(vals * 256, np.arange(1, 256, 2))
    print("occurrences of the 128 thresholds on 256 x 256: %d .. %d" % (counts.min(), counts.max()))
    assert counts.min() >= 507 and counts.max() <= 517


def test_a_code_keeps_its_code():
    """n + theta is exact in fp32 for every code n of every depth, at both extreme thresholds: floor gives n back."""
    for M in (255, 1023, 65535):
        n = np.arange(M + 1, dtype=np.int64)
        for th in (F(1 / 256), F(255 / 256)):
            s = n.astype(F) + th
            assert s.dtype == np.float32 and np.array_equal(s.astype(np.float64), n + float(th))  # exact
            assert np.array_equal(np.floor(s).astype(np.int64), n)
    # ... through the quantiser: an image of exact codes passes unchanged (d = n / 255 rounded to fp32, times 255, is n again)
    img = np.random.default_rng(1).integers(0, 256, size=(3, 33, 47))
    d = (img.astype(F) / F(255)).astype(F)
    assert np.array_equal(d * F(255), img.astype(F))
    assert np.array_equal(D.quantise_rgb(d, 255), img.transpose(1, 2, 0))
    assert D.quantise_rgb(np.zeros((3, 5, 7), F), 65535).max() == 0 and D.quantise_rgb(np.ones((3, 5, 7), F), 65535).min() == 65535


def box_means(a, k=8):
    h, w = a.shape
    return a.reshape(h // k, k, w // k, k).astype(np.float64).mean(axis=(1, 3))


def test_gradient_does_not_band():
    """A horizontal ramp of 1/16 code per pixel (512 x 64, from 0.5): the 8 x 8 box means of the dithered codes stay within a quarter of
    the error plain rounding makes.  Measured with numpy: 0.031 against 0.281, a ratio of 9; the factor 4 leaves a margin of 2."""
    v = np.broadcast_to(F(0.5) + np.arange(512, dtype=F) / F(16), (64, 512))
    d = np.stack([(v / F(255)).astype(F)] * 3)
    true = box_means((d[0] * F(255)).astype(np.float64))
    plain = np.abs(box_means(np.floor(d[0] * F(255) + F(0.5))) - true).max()
    dith = np.abs(box_means(D.quantise_rgb(d, 255)[..., 0]) - true).max()
    print("largest error of the 8 x 8 box means: dithered %.4f, rounded %.4f codes" % (dith, plain))
    assert dith < plain / 4


def test_yuv_encodes_differ_from_rounding_only_by_one_code():
    """The dithered encodes quantise the very values of the plain references (floor(v + theta) and floor(v + 0.5) differ by at most one):
    every code is the plain one or its neighbour, and on a random image some are the neighbour."""
    import yuv444_ref
    import yuv_ref
    import yuv_siting_ref
    import yuv422_ref
    d = np.random.default_rng(3).random((3, 32, 48), dtype=np.float32)
    for bits in (8, 10):
        pairs = [(D.encode420(d, 0, 0, 709, 0, bits), yuv_ref.encode(d, 709, 0, bits)),
                 (D.encode420(d, 2, 16, 601, 1, bits), yuv_siting_ref.encode(d, 2, 16, 601, 1, bits)),
                 (D.encode422(d, 1, 16, 2020, 0, bits), yuv422_ref.encode(d, 2020, 0, bits, 1, 16)),
                 (D.encode444(d, 709, 1, bits), yuv444_ref.encode(d, 709, 1, bits))]
        for got, want in pairs:
            for g, w_ in zip(got, want):
                assert g.shape == w_.shape and np.abs(g - w_).max() == 1
