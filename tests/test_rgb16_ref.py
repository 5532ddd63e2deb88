"""RSR_FMT_U16_HWC without a GPU: the numpy definition of tests/rgb16_ref.py against the statements of include/realsr_hip.h ("16-bit RGB(A)"),
and the host-only rules of id 16 against the library."""
import ctypes as C
import importlib.util
import itertools
import os

import numpy as np
import pytest

import realsr_ncnn_vulkan_amd as R
import rgb16_ref as Z

HERE = os.path.dirname(os.path.abspath(__file__))
U16 = R.RSR_FMT_U16_HWC


def _rules():
    spec = importlib.util.spec_from_file_location("make_format_rules", os.path.join(HERE, "golden", "make_format_rules.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- the definition -----------------------------------------------------------------------------------------------------------------------
def test_id():
    assert U16 == Z.U16 == 16


def test_decode_of_257b_is_the_uint8_decode():
    b = np.arange(256, dtype=np.uint8)
    assert np.array_equal(Z.decode(Z.widen(b)).view(np.uint16), Z.decode8(b).view(np.uint16))


def test_decode_is_unsigned_and_monotone():
    k = np.arange(65536, dtype=np.uint16)
    d = Z.decode(k).astype(np.float32)
    assert d[0] == 0 and d[65535] == 1 and (np.diff(d) >= 0).all()  # (an int16 reading would put 32768 .. 65535 below 0)
    assert np.array_equal(Z.decode(k.view(np.int16).view(np.uint16)), Z.decode(k))


def test_precision_statement():
    """The header's figures: 7,169 distinct inputs; code -> input -> code is off by at most 16 codes, an 8-bit hop by 128."""
    k = np.arange(65536, dtype=np.uint16)
    d = Z.decode(k)
    assert np.unique(d.view(np.uint16)).size == 7169
    back = Z.encode(d.astype(np.float32)).astype(np.int64)
    assert np.abs(back - k).max() == 16
    hop = np.floor(k / 257.0 + 0.5) * 257
    assert np.abs(hop - k).max() == 128


def test_encode_ends_and_monotone_over_all_halfs():
    halfs = np.arange(0, 0x3C01, dtype=np.uint16).view(np.float16).astype(np.float32)  # every fp16 value in [0, 1], ascending
    assert halfs[0] == 0 and halfs[-1] == 1
    e = Z.encode(halfs).astype(np.int64)
    assert e[0] == 0 and e[-1] == 65535 and (np.diff(e) >= 0).all()
    assert np.diff(e).max() == 32  # "spacing up to 2^-11, about 32 codes near white"


def test_encode_rounds_each_operation():
    """d * 65535 + 0.5 in ONE rounding (an fma) differs from the two roundings of the definition somewhere: the definition is what counts."""
    d = np.random.default_rng(1).random(1 << 16, dtype=np.float32)
    two = Z.encode(d)
    one = np.floor((d.astype(np.float64) * 65535.0 + 0.5).astype(np.float32)).astype(np.uint16)
    assert np.abs(two.astype(int) - one.astype(int)).max() <= 1


def test_alpha_units():
    v = np.array([0, 1, 127.5, 255], dtype=np.float32)
    assert np.array_equal(Z.alpha_units(v, Z.U8, Z.U16), v * np.float32(257))
    assert Z.alpha_units(np.float32(255), Z.U8, Z.U16) == 65535
    assert Z.alpha_store(Z.alpha_units(np.float32(65535), Z.U16, Z.U8), Z.U8) == 255
    assert Z.alpha_units(v, Z.U16, Z.U16) is not None and np.array_equal(Z.alpha_units(v, Z.U8, Z.U8), v)


def test_bicubic_mirror_agrees_with_its_exact_form():
    """The float32 evaluation of the x4 alpha (any chain) stays within the rounding bound of the exact one: 12 roundings of values below
    65535 * 1.4^2."""
    a = np.random.default_rng(2).integers(0, 65536, size=(9, 7)).astype(np.uint16)
    exact = Z.bicubic_x4(a)
    for chain in ("fma", "seq", "none"):
        assert np.abs(Z.bicubic_x4_f32(a, chain) - exact).max() <= 12 * 2.0 ** -24 * 65535 * 1.96, chain
    flat = np.full((5, 6), 65535, dtype=np.uint16)
    assert (Z.bicubic_x4(flat) == 65535).all()


# ---- the host rules of id 16 ----------------------------------------------------------------------------------------------------------
def test_image_bytes_and_span():
    m = _rules()
    for c, w, h in itertools.product((3, 4), m.WS, m.HS):
        assert R.image_bytes(U16, w, h, c) == 2 * w * h * c
        packed = 2 * w * c
        assert R.image_span(U16, w, h, c) == h * packed
        assert R.image_span(U16, w, h, c, packed + 2, 12345) == (h - 1) * (packed + 2) + packed  # plane_pitch is ignored
        for bad in (packed - 2, packed + 1, packed + 3):
            with pytest.raises(R.RealSRError):
                R.image_span(U16, w, h, c, bad, 0)
    for c in (1, 2, 5):
        with pytest.raises(R.RealSRError):
            R.image_bytes(U16, 4, 4, c)


def test_out_size_fmt_is_out_size_xy_on_the_grid():
    m = _rules()
    L = R.lib()
    n = 0
    for ((nx, dx), (ny, dy)), T, w, h in itertools.product(m.XY, m.TILES, m.WS, m.HS):
        a = m.ask(L, "rsr_out_size_fmt", (U16, nx, dx, ny, dy, T, w, h))
        b = m.ask(L, "rsr_out_size_xy", (nx, dx, ny, dy, T, w, h))
        assert a == b, ((nx, dx, ny, dy, T, w, h), a, b)
        n += 1
    assert n == len(m.XY) * len(m.TILES) * len(m.WS) * len(m.HS)


@pytest.mark.parametrize("fmt", [-1, 3, 6, 7, 10, 11, 14, 15, 17])
def test_unknown_ids_stay_unknown(fmt):
    L = R.lib()
    assert L.rsr_image_bytes(fmt, 4, 4, 3) < 0
    assert L.rsr_image_span(fmt, 4, 4, 3, 0, 0) < 0
    ow, oh = C.c_int(0), C.c_int(0)
    assert L.rsr_out_size_fmt(fmt, 4, 1, 4, 1, 32, 8, 8, C.byref(ow), C.byref(oh)) == R.RSR_E_ARG
    assert L.rsr_last_error(None).decode() == "unknown pixel format"


def test_format_array_spec():
    assert R.format_array_spec(U16, 5, 4, 4) == ((4, 5, 4), np.dtype(np.uint16))
    assert R.format_array_dims(U16, np.zeros((4, 5, 3), np.uint16)) == (5, 4, 3)
    assert R.format_array_dims(R.RSR_FMT_NV12, np.zeros((6, 8), np.uint8)) == (8, 4, 3)
    assert R.format_array_dims(R.RSR_FMT_P210, np.zeros((8, 8), np.uint16)) == (8, 4, 3)
    with pytest.raises(ValueError):
        R.format_array_dims(U16, np.zeros((4, 5, 3), np.int16))
    with pytest.raises(ValueError):
        R.format_array_spec(14, 4, 4)
