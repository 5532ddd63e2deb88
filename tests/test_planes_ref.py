"""tests/planes_ref.py, the numpy definition of rsr_pack_planes / rsr_unpack_planes, checked against itself, against the format table
(tests/pixfmt_ref.py) and against what the library and its header say without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import realsr_ncnn_vulkan_amd as R

import pixfmt_ref as F
import planes_ref as P

SIZES = [(2, 2), (4, 2), (18, 26), (34, 2), (66, 26), (130, 4), (36, 26)]
ODD = [(18, 3), (35, 25), (1, 1)]


def test_the_six_yuv_formats_and_nothing_else():
    assert sorted(P.FORMATS) == sorted(f for f in F.FORMATS if F.is_yuv(f)) and len(P.FORMATS) == 6
    assert [P.chroma_dims(f, 36, 26) for f in (F.NV12, F.P010, F.NV16, F.P210, F.YUV444P, F.YUV444P10)] == [(18, 13)] * 2 + [(18, 26)] * 2 + [(36, 26)] * 2


@pytest.mark.parametrize("fmt", P.FORMATS)
def test_shapes_agree_with_the_format_table_and_the_library(fmt):
    for w, h in SIZES + ODD:
        if not P.admits(fmt, w, h):
            assert R.lib().rsr_image_bytes(fmt, w, h, 3) == R.RSR_E_ARG  # the parity rule is the library's
            continue
        y, u, v = P.frame(1, fmt, w, h)
        s = P.pack(fmt, y, u, v)
        assert s.shape == F.shape_of(fmt, w, h) and s.dtype == F.NP[fmt] and s.nbytes == R.image_bytes(fmt, w, h)
        assert sum(p.nbytes for p in (y, u, v)) == s.nbytes  # the same samples, laid out differently
        assert [p.shape for p in P.unpack(fmt, s, w, h)] == list(P.plane_shapes(fmt, w, h))
    assert any(P.admits(fmt, w, h) for w, h in ODD) == (fmt in F.P444 + F.S422)


@pytest.mark.parametrize("fmt", P.FORMATS)
def test_round_trips(fmt):
    for i, (w, h) in enumerate((w, h) for w, h in SIZES + ODD if P.admits(fmt, w, h)):
        planes = P.frame(10 + i, fmt, w, h)
        s = P.pack(fmt, *planes)
        back = P.unpack(fmt, s, w, h)
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(planes, back))
        assert np.array_equal(P.pack(fmt, *back), s)
        # a surface as the engine writes it (pixfmt_ref.image: the code where the format holds it) survives unpack -> pack
        img = F.image(20 + i, fmt, w, h)
        assert np.array_equal(P.pack(fmt, *P.unpack(fmt, img, w, h)), img)


def test_the_interleave_by_hand():
    y = np.arange(8, dtype=np.uint8).reshape(2, 4)
    u, v = np.array([[100, 101]], dtype=np.uint8), np.array([[200, 201]], dtype=np.uint8)
    assert P.pack(F.NV12, y, u, v).tolist() == [[0, 1, 2, 3], [4, 5, 6, 7], [100, 200, 101, 201]]
    u2, v2 = np.array([[100, 101], [102, 103]], dtype=np.uint8), np.array([[200, 201], [202, 203]], dtype=np.uint8)
    assert P.pack(F.NV16, y, u2, v2).tolist() == [[0, 1, 2, 3], [4, 5, 6, 7], [100, 200, 101, 201], [102, 202, 103, 203]]
    w = lambda a: np.array(a, dtype=np.uint16)
    assert P.pack(F.P010, w([[1, 2], [3, 1023]]), w([[512]]), w([[4]])).tolist() == [[64, 128], [192, 1023 << 6], [512 << 6, 256]]


@pytest.mark.parametrize("fmt", (F.P010, F.P210))
def test_high_bits_of_planar_words_are_masked(fmt):
    clean, dirty = P.frame(3, fmt, 18, 26), P.frame(3, fmt, 18, 26, dirty=True)
    assert not any(np.array_equal(a, b) for a, b in zip(clean, dirty)) and all(np.array_equal(a, b & 1023) for a, b in zip(clean, dirty))
    s = P.pack(fmt, *dirty)
    assert np.array_equal(s, P.pack(fmt, *clean)) and not (s & 63).any() and (s >> 6).max() == 1023
    assert all(np.array_equal(a, b) for a, b in zip(P.unpack(fmt, s, 18, 26), clean))


def test_444p10_words_are_copied_verbatim():
    dirty = P.frame(4, F.YUV444P10, 7, 5, dirty=True)
    s = P.pack(F.YUV444P10, *dirty)
    assert (s >> 10).any() and all(np.array_equal(a, b) for a, b in zip(P.unpack(F.YUV444P10, s, 7, 5), dirty))


@pytest.mark.parametrize("fmt", (F.P010, F.P210))
def test_low_bits_of_a_surface_word_are_dropped(fmt):
    img = F.image(5, fmt, 18, 26)
    noisy = img | np.random.default_rng(6).integers(0, 64, size=img.shape).astype(np.uint16)
    assert not np.array_equal(noisy, img)
    assert all(np.array_equal(a, b) and a.max() <= 1023 for a, b in zip(P.unpack(fmt, noisy, 18, 26), P.unpack(fmt, img, 18, 26)))
    assert np.array_equal(P.pack(fmt, *P.unpack(fmt, noisy, 18, 26)), img)


def test_the_header_states_the_definition_and_the_binding_has_the_struct():
    text = open(os.path.join(R.INCLUDE_DIR, "realsr_hip.h")).read()
    for needle in ("typedef struct rsr_planes", "(plane word & 1023) << 6", "surface word >> 6", "UV[r][2X] = U[r][X]", "copied verbatim",
                   "ONE launch per call", "yuv420p", "yuv422p", "three-plane", "4:1:1"):
        assert needle in text, needle
    for name in ("rsr_pack_planes", "rsr_unpack_planes"):
        assert name in R.EXPORTS and hasattr(R.lib(), name) and re.search(r"^int %s\(rsr_ctx\* ctx, int n, " % name, text, re.M)
    assert [f[0] for f in R.Planes._fields_] == ["y", "u", "v", "y_pitch", "c_pitch"] and C.sizeof(R.Planes) == 40
    assert not [n for n in dir(R) if n.startswith("RSR_FMT_") and getattr(R, n) not in F.FORMATS]
