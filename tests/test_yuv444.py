"""YUV444P / YUV444P10 (planar YUV 4:4:4) without a GPU: the host-only functions (rsr_image_bytes, rsr_image_span, rsr_out_size_fmt), the
ties of tests/yuv444_ref.py to the 4:2:0 and 4:2:2 references, and what torch_io hands the engine with chroma=444 (a fake context and
stream, as in tests/test_yuv422.py)."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

import yuv422_ref
import yuv444_ref
import yuv_ref
from pixfmt_ref import NV12, NV16, YUV444P, YUV444P10

Y444, Y444_10 = YUV444P, YUV444P10
F = np.float32
# the 67 ratios of one axis (rsr_set_out_ratio_xy): n / d in lowest terms, d in 1..8, 1 <= n / d <= 4
RATIOS = sorted({Fraction(n, d) for d in range(1, 9) for n in range(d, 4 * d + 1) if Fraction(n, d).denominator == d})


def test_constants_are_in_the_header_and_the_binding_agrees():
    text = open(os.path.join(R.INCLUDE_DIR, "realsr_hip.h")).read()
    for name, val in (("RSR_FMT_YUV444P", 12), ("RSR_FMT_YUV444P10", 13)):
        assert re.search(r"^#define %s +%d +/\*" % (name, val), text, re.M), name
        assert getattr(R, name) == val
    for needle in ("YUV 4:4:4", "word & 1023", "code << 6", "LOW 10 bits", "NO PARITY RULE", "yuv420p", "yuv422p", "three-plane", "4:1:1",
                   "the same kernels and the same bytes"):
        assert needle in text, needle
    assert len(RATIOS) == 67


def test_image_bytes_and_span():
    L = R.lib()
    for w, h in ((1, 1), (35, 25), (36, 26), (1280, 1080), (7680, 4320)):  # any parity
        assert L.rsr_image_bytes(Y444, w, h, 3) == 3 * w * h == R.image_bytes(Y444, w, h)
        assert L.rsr_image_bytes(Y444_10, w, h, 3) == 6 * w * h == R.image_bytes(Y444_10, w, h)
        assert R.image_span(Y444, w, h) == 3 * w * h and R.image_span(Y444_10, w, h) == 6 * w * h
    assert L.rsr_image_bytes(Y444_10, 8 * 7680, 8 * 4320, 3) == 6 * 64 * 7680 * 4320 > 2 ** 32  # a long long
    assert L.rsr_image_bytes(Y444, 65535, 32769, 3) == 3 * 65535 * 32769 > 2 ** 32                 # ... at odd sizes
    # pitched: plane q at q * plane_pitch, the last row of the last plane w samples long
    assert R.image_span(Y444, 35, 25, 3, 64, 0) == 2 * 25 * 64 + 24 * 64 + 35
    assert R.image_span(Y444, 35, 25, 3, 64, 2000) == 2 * 2000 + 24 * 64 + 35
    assert R.image_span(Y444, 35, 25, 3, 37, 1001) == 2 * 1001 + 24 * 37 + 35           # YUV444P: any byte pitches
    assert R.image_span(Y444_10, 35, 25, 3, 80, 0) == 2 * 25 * 80 + 24 * 80 + 70
    assert R.image_span(Y444_10, 35, 25, 3, 80, 4000) == 2 * 4000 + 24 * 80 + 70
    assert R.image_span(Y444, 1, 1, 3, 0, 0) == 3
    far = (1 << 31) + (1 << 20) + 6                                                       # plane 1 beyond 2^31, plane 2 beyond 2^32
    assert R.image_span(Y444, 35, 25, 3, 64, far) == 2 * far + 24 * 64 + 35 > 2 ** 32
    assert R.image_span(Y444_10, 35, 25, 3, 80, far) == 2 * far + 24 * 80 + 70


@pytest.mark.parametrize("fmt", [Y444, Y444_10])
def test_argument_errors_that_need_no_context(fmt):
    L = R.lib()
    es = 1 if fmt == Y444 else 2
    for c in (1, 4):
        assert L.rsr_image_bytes(fmt, 8, 8, c) == R.RSR_E_ARG and L.rsr_image_span(fmt, 8, 8, c, 0, 0) == R.RSR_E_ARG
    for w, h in ((0, 8), (8, 0), (-2, 8), (8, -1)):
        assert L.rsr_image_bytes(fmt, w, h, 3) == R.RSR_E_ARG, (w, h)
        assert L.rsr_image_span(fmt, w, h, 3, 0, 0) == R.RSR_E_ARG, (w, h)
    assert L.rsr_image_bytes(fmt, 7, 5, 3) == 3 * es * 7 * 5 == L.rsr_image_span(fmt, 7, 5, 3, 0, 0)  # odd on both axes: an image
    assert L.rsr_image_span(fmt, 8, 8, 3, 8 * es - 1, 0) == R.RSR_E_ARG     # a row pitch below the bytes of a row
    assert L.rsr_image_span(fmt, 8, 8, 3, -16, 0) == R.RSR_E_ARG and L.rsr_image_span(fmt, 8, 8, 3, 0, -1) == R.RSR_E_ARG
    odd = L.rsr_image_span(fmt, 7, 8, 3, 8 * es + 1, 0), L.rsr_image_span(fmt, 7, 8, 3, 0, 8 * 8 * es + 1)
    if fmt == Y444_10:  # 16-bit samples: an odd pitch is refused
        assert odd == (R.RSR_E_ARG, R.RSR_E_ARG)
    else:
        assert odd == (2 * 8 * 9 + 7 * 9 + 7, 2 * 65 + 7 * 7 + 7)
    with pytest.raises(R.RealSRError) as e:
        R.image_bytes(fmt, 9, 8, 4)
    assert e.value.code == R.RSR_E_ARG
    assert L.rsr_process_device_fmt(None, None, fmt, 8, 8, 3, None, fmt, None) == R.RSR_E_ARG
    for bad in (3, 6, 7, 10, 11, 14, -1):  # the ids around the new ones stay unknown
        assert L.rsr_image_bytes(bad, 8, 8, 3) == R.RSR_E_ARG
        assert L.rsr_image_span(bad, 8, 8, 3, 0, 0) == R.RSR_E_ARG


# ---- rsr_out_size_fmt --------------------------------------------------------------------------------------------------------------
def _call(fn, *a):
    ow, oh = C.c_int(-7), C.c_int(-7)
    rc = fn(*a, C.byref(ow), C.byref(oh))
    return (rc, ow.value, oh.value) if rc == 0 else (rc, R.lib().rsr_last_error(None).decode())


@pytest.mark.parametrize("w,h,tile", [(36, 26, 16), (35, 25, 24), (35, 25, 33), (720, 576, 192)])
def test_out_size_fmt_is_exactly_the_rgb_rule(w, h, tile):
    """All 67 x 67 ratio pairs: a 4:4:4 output is sized and refused as an RGB one, error text included -- and is taken where NV16 is refused
    for its parity."""
    L = R.lib()
    taken = beyond_nv16 = 0
    for rx in RATIOS:
        for ry in RATIOS:
            a = (rx.numerator, rx.denominator, ry.numerator, ry.denominator, tile, w, h)
            rgb = _call(L.rsr_out_size_xy, *a)
            for fmt in (Y444, Y444_10):
                got = _call(L.rsr_out_size_fmt, fmt, *a)
                assert got == rgb, (fmt, a)
                assert got[0] == 0 or "YUV" not in got[1]
            if rgb[0] == 0:
                taken += 1
                nv16 = _call(L.rsr_out_size_fmt, NV16, *a)
                if nv16[0] != 0:
                    assert "YUV" in nv16[1]
                    beyond_nv16 += 1
    # 36 x 26 at tile 16 too: 5/4 along x gives 45 columns.  Only 720 and 192, multiples of 16, stay even at every ratio with d <= 8.
    assert taken > 0 and (beyond_nv16 > 0) == ((w, tile) != (720, 192))


def test_out_size_fmt_examples():
    L = R.lib()
    f = lambda *a: _call(L.rsr_out_size_fmt, *a)  # noqa: E731
    assert f(Y444, 4, 1, 4, 1, 16, 35, 25) == (0, 140, 100)
    assert f(Y444, 1, 1, 1, 1, 16, 35, 25) == (0, 35, 25)                      # out_scale 1 at an odd size: no 4:2:x surface takes it
    assert f(NV16, 1, 1, 1, 1, 16, 35, 25)[0] == R.RSR_E_ARG and f(NV12, 1, 1, 1, 1, 16, 36, 25)[0] == R.RSR_E_ARG
    assert f(Y444_10, 1, 1, 1, 1, 33, 35, 25) == (0, 35, 25)                   # ... nor an odd tile size
    assert f(Y444, 3, 2, 3, 2, 30, 36, 26) == (0, 54, 39)                      # 45 columns per tile
    assert f(Y444_10, 8, 3, 9, 4, 24, 45, 28) == (0, 120, 63)
    assert f(Y444, 3, 2, 3, 2, 16, 35, 25)[0] == R.RSR_E_ARG                   # the ratio rule holds as ever
    assert "YUV" not in f(Y444, 3, 2, 3, 2, 16, 35, 25)[1]
    for bad in (3, 6, 7, 10, 11, 14, -1):
        assert f(bad, 4, 1, 4, 1, 16, 36, 26)[0] == R.RSR_E_ARG
    assert L.rsr_out_size_fmt(Y444, 4, 1, 4, 1, 16, 35, 25, None, None) == 0   # either pointer may be NULL


def test_yuv_constants_keep_refusing_other_depths():
    out = (C.c_float * 18)()
    assert R.lib().rsr_yuv_constants(709, 0, 8, out, 18) == 0 and R.lib().rsr_yuv_constants(709, 0, 10, out, 18) == 0
    for bits in (12, 16):
        assert R.lib().rsr_yuv_constants(709, 0, bits, out, 18) == R.RSR_E_ARG


# ---- the new reference against the existing ones -----------------------------------------------------------------------------------
CFG2 = [(709, 0), (601, 1)]


@pytest.mark.parametrize("matrix,full", CFG2)
@pytest.mark.parametrize("bits", [8, 10])
def test_encode_tie_constant_quads(bits, matrix, full):
    """An image whose 2 x 2 quads are constant: the 4:4:4 luma is the 4:2:0 luma everywhere, and the 4:4:4 chroma at the quads' first pixels
    is NV12's at siting 0 -- ((d + d) + (d + d)) * 0.25f is d exactly."""
    rng = np.random.default_rng(9 + bits + matrix)
    w, h = 22, 12
    d = np.repeat(np.repeat(rng.uniform(0, 1, size=(3, h // 2, w // 2)).astype(F), 2, axis=1), 2, axis=2)
    y4, u4, v4 = yuv444_ref.encode(d, matrix, full, bits)
    y0, uv0 = yuv_ref.encode(d, matrix, full, bits)
    assert y4.shape == u4.shape == v4.shape == (h, w) and len(np.unique(u4)) > 16
    assert np.array_equal(y4, y0)
    assert np.array_equal(u4[0::2, 0::2], uv0[..., 0]) and np.array_equal(v4[0::2, 0::2], uv0[..., 1])
    assert np.array_equal(u4[1::2, 1::2], uv0[..., 0])  # (every pixel of a constant quad, in fact)


@pytest.mark.parametrize("matrix,full", CFG2)
@pytest.mark.parametrize("bits", [8, 10])
def test_decode_tie_even_columns(bits, matrix, full):
    """At even columns decode(Y, U, V) is the 4:2:2 decode of (Y, UV(U[:, ::2], V[:, ::2])) at siting 1: the co-sited rule takes c[n]
    itself there."""
    rng = np.random.default_rng(5 + bits + matrix)
    w, h = 22, 7
    y, u, v = (rng.integers(0, 1 << bits, size=(h, w)) for _ in range(3))
    got = yuv444_ref.decode(y, u, v, matrix, full, bits)
    want = yuv422_ref.decode(y, np.stack([u[:, ::2], v[:, ::2]], axis=-1), matrix, full, bits, siting=1)
    assert got.dtype == want.dtype == np.float32 and got.shape == (3, h, w)
    assert np.array_equal(got[:, :, ::2].view(np.uint32), want[:, :, ::2].view(np.uint32))
    assert not np.array_equal(got[:, :, 1::2], want[:, :, 1::2])  # (odd columns are filtered at 4:2:2)
    assert (got == 0).any() and (got == 1).any()                  # the clamp acts


def test_split_and_join_are_inverse_and_high_bits_are_no_code():
    rng = np.random.default_rng(3)
    for bits, dt in ((8, np.uint8), (10, np.uint16)):
        s = rng.integers(0, 1 << bits, size=(3, 7, 9)).astype(dt)
        y, u, v = yuv444_ref.split(s, bits)
        assert y.shape == (7, 9) and np.array_equal(yuv444_ref.join(y, u, v, bits), s)
        rgb = yuv444_ref.decode(y, u, v, 709, 0, bits)
        assert rgb.shape == (3, 7, 9)
        assert all(p.shape == (7, 9) for p in yuv444_ref.encode(rgb, 709, 0, bits))
    dirty = s | (rng.integers(0, 64, size=s.shape).astype(np.uint16) << 10)
    assert not np.array_equal(dirty, s) and all(np.array_equal(p, q) for p, q in zip(yuv444_ref.split(dirty, 10), yuv444_ref.split(s, 10)))
    assert all(np.array_equal(p, q) for p, q in zip(yuv444_ref.split(s.view(np.int16), 10), yuv444_ref.split(s, 10)))


# ---- torch_io with chroma=444: what it hands the engine ----------------------------------------------------------------------------
class _Stream:
    cuda_stream = 5  # (not the null stream: the call is enqueued on it directly)


class _Ctx:
    gpuid, scale, out_scale, tilesize = 0, 4, 2, 16

    def __init__(self, ratio=None):
        self.calls, self.sized, self.ratio = [], [], ratio
        if ratio is not None:
            self.out_scale = 0

    def out_size_fmt(self, fmt, w, h):
        self.sized.append((fmt, w, h))
        rx, ry = self.ratio if self.ratio is not None else (Fraction(self.out_scale),) * 2
        ow, oh = C.c_int(0), C.c_int(0)
        if R.lib().rsr_out_size_fmt(fmt, rx.numerator, rx.denominator, ry.numerator, ry.denominator, self.tilesize, w, h, C.byref(ow), C.byref(oh)):
            raise ValueError(R.lib().rsr_last_error(None).decode())
        return ow.value, oh.value

    def process_device_batch(self, *a, **k):
        self.calls.append((a, k))


class _Cuda0(torch.Tensor):
    """A CPU tensor that claims to live on cuda:0 (tests/test_tensor_batch.py)."""
    @property
    def device(self):
        return torch.device("cuda", 0)


def _on_cuda0(t):
    return t.as_subclass(_Cuda0)


@pytest.fixture
def fake_stream(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _Stream())


def test_upscale_yuv_444_describes_a_view_and_sizes_the_result(fake_stream):
    s = _Ctx()
    x = _on_cuda0(torch.zeros(3, 25, 35, dtype=torch.uint8))
    out = _on_cuda0(torch.zeros(3, 50, 70, dtype=torch.uint8))
    assert torch_io.upscale_yuv(s, x, out=out, chroma=444) is out
    (a, k), = s.calls
    assert a == ([(x.data_ptr(), 35, 25 * 35)], Y444, 35, 25, 3, [(out.data_ptr(), 70, 50 * 70)], Y444) and k == {"stream": 5}
    assert s.sized == [(Y444, 35, 25)]
    # yuv444p10le as int16, a crop of a larger frame in, a window of a canvas out: pointer and pitches in bytes, no copy
    s = _Ctx()
    big = torch.zeros(3, 40, 64, dtype=torch.int16)
    canvas = torch.zeros(3, 60, 100, dtype=torch.int16)
    x, win = _on_cuda0(big[:, 3:28, 5:40]), _on_cuda0(canvas[:, 7:57, 11:81])
    assert torch_io.upscale_yuv(s, x, out=win, chroma=444) is win
    (a, k), = s.calls
    assert a[0] == [(big.data_ptr() + 2 * (3 * 64 + 5), 128, 40 * 128)] and a[1:5] == (Y444_10, 35, 25, 3) and a[6] == Y444_10
    assert a[5] == [(canvas.data_ptr() + 2 * (7 * 100 + 11), 200, 60 * 200)]
    # a new result: (3, oh, ow) of the same dtype; at a ratio, odd sizes where the arithmetic gives them
    s = _Ctx((Fraction(3, 2), Fraction(3, 2)))
    y = torch_io.upscale_yuv(s, _on_cuda0(torch.zeros(3, 26, 36, dtype=torch.int16)), chroma=444)
    assert tuple(y.shape) == (3, 39, 54) and y.dtype == torch.int16 and s.calls[0][0][5] == [(y.data_ptr(), 108, 39 * 108)]
    # a (y, u, v) triple of equally spaced views
    s = _Ctx()
    pool = torch.zeros(8192, dtype=torch.uint8)
    planes = tuple(_on_cuda0(pool[q * 1500:q * 1500 + 25 * 40].view(25, 40)[:, :35]) for q in range(3))
    got = torch_io.upscale_yuv(s, planes, chroma=444)
    (a, k), = s.calls
    assert a[0] == [(pool.data_ptr(), 40, 1500)] and isinstance(got, tuple) and len(got) == 3 and all(tuple(p.shape) == (50, 70) for p in got)


def _planes_with_row_strides(*strides):
    pool = torch.zeros(16384, dtype=torch.uint8)
    return tuple(_on_cuda0(pool[q * 4000:q * 4000 + 25 * st].view(25, st)[:, :35]) for q, st in enumerate(strides))


@pytest.mark.parametrize("x", [
    torch.zeros(3, 25, 35, dtype=torch.uint8),                        # wrong device (CPU)
    _on_cuda0(torch.zeros(3, 25, 35, dtype=torch.float16)),           # dtype
    _on_cuda0(torch.zeros(3, 25, 35, dtype=torch.int32)),
    _on_cuda0(torch.zeros(75, 35, dtype=torch.uint8)),                # a 2-D tensor is no (3, H, W) image
    _on_cuda0(torch.zeros(4, 25, 35, dtype=torch.uint8)),             # four planes
    _on_cuda0(torch.zeros(3, 25, 70, dtype=torch.uint8)[:, :, ::2]),  # a step along W
    _on_cuda0(torch.zeros(25, 35, 3, dtype=torch.uint8).permute(2, 0, 1)),  # HWC memory
    _on_cuda0(torch.zeros(1, 25, 35, dtype=torch.uint8).expand(3, 25, 35)),  # no plane pitch
    _planes_with_row_strides(40, 40, 48),                             # planes with different row strides
    (_planes_with_row_strides(40, 40, 40)[0], _planes_with_row_strides(40, 40, 40)[2], _planes_with_row_strides(40, 40, 40)[1]),  # not one allocation, not equally spaced
    _planes_with_row_strides(40, 40),                                 # a pair is no 4:4:4 image
], ids=lambda x: "planes%d" % len(x) if isinstance(x, tuple) else "%s-%s-%s" % (str(x.dtype).split(".")[-1], "x".join(map(str, x.shape)), "x".join(map(str, x.stride()))))
def test_upscale_yuv_444_rejects_bad_images_before_launching(fake_stream, x):
    s = _Ctx()
    with pytest.raises(ValueError):
        torch_io.upscale_yuv(s, x, chroma=444)
    assert s.calls == []


def test_upscale_yuv_444_rejects_a_bad_out_and_what_the_engine_would_refuse(fake_stream):
    s = _Ctx()
    x = _on_cuda0(torch.zeros(3, 25, 35, dtype=torch.uint8))
    for out in (_on_cuda0(torch.zeros(3, 50, 72, dtype=torch.uint8)),            # the wrong size
                _on_cuda0(torch.zeros(3, 50, 70, dtype=torch.int16)),            # the wrong dtype
                _on_cuda0(torch.zeros(3, 50, 140, dtype=torch.uint8)[:, :, ::2]),  # a step along W
                torch.zeros(3, 50, 70, dtype=torch.uint8),                       # CPU
                _planes_with_row_strides(40, 40, 40)):                           # a triple for a tensor
        with pytest.raises(ValueError):
            torch_io.upscale_yuv(s, x, out=out, chroma=444)
    s.ratio, s.out_scale = (Fraction(3, 2), Fraction(3, 2)), 0
    with pytest.raises(ValueError) as e:  # 35 * 3 / 2 is no whole number: the ratio rule, with no word of YUV in it
        torch_io.upscale_yuv(s, x, chroma=444)
    assert "YUV" not in str(e.value)
    with pytest.raises(ValueError):
        torch_io.upscale_yuv(s, x, chroma=411)
    assert s.calls == []


def test_delta_and_sequence_444_validate_before_launching(fake_stream):
    s = _Ctx()
    s.tile_count = lambda w, h: (3, 2)
    x = _on_cuda0(torch.zeros(3, 25, 35, dtype=torch.uint8))
    y = _on_cuda0(torch.zeros(3, 50, 70, dtype=torch.uint8))
    with pytest.raises(ValueError):  # prev_y of the wrong size
        torch_io.upscale_delta(s, x, x, _on_cuda0(torch.zeros(3, 50, 72, dtype=torch.uint8)), chroma=444)
    with pytest.raises(ValueError):  # x is no 4:4:4 image
        torch_io.upscale_delta(s, _on_cuda0(torch.zeros(75, 35, dtype=torch.uint8)), None, y, chroma=444)
    with pytest.raises(ValueError):  # mixed layouts
        torch_io.upscale_sequence(s, [x, _on_cuda0(torch.zeros(3, 25, 36, dtype=torch.uint8))], chroma=444)
    with pytest.raises(ValueError):  # an out[k] of the wrong size
        torch_io.upscale_sequence(s, [x, x], out=[y, _on_cuda0(torch.zeros(3, 50, 72, dtype=torch.uint8))], chroma=444)
    assert s.calls == []


def test_chroma_420_and_422_calls_are_unchanged(fake_stream):
    """chroma=420 -- given or not -- and chroma=422 size, describe and refuse as before; a (3, H, W) uint8 tensor stays no surface there."""
    class Old:
        gpuid, scale, out_scale = 0, 4, 2

        def __init__(self):
            self.calls = []

        def process_device_batch(self, *a, **k):
            self.calls.append((a, k))

    x = _on_cuda0(torch.zeros(39, 36, dtype=torch.uint8))  # 36 x 26 NV12
    for kw in ({}, {"chroma": 420}):
        s = Old()
        y = torch_io.upscale_yuv(s, x, **kw)
        (a, k), = s.calls
        assert a == ([(x.data_ptr(), 36, 26 * 36)], NV12, 36, 26, 3, [(y.data_ptr(), 72, 52 * 72)], NV12) and k == {"stream": 5}
        with pytest.raises(ValueError):
            torch_io.upscale_yuv(s, _on_cuda0(torch.zeros(3, 26, 36, dtype=torch.uint8)), **kw)
        assert len(s.calls) == 1
    s = _Ctx()
    x = _on_cuda0(torch.zeros(50, 36, dtype=torch.uint8))  # 36 x 25 NV16
    y = torch_io.upscale_yuv(s, x, chroma=422)
    (a, k), = s.calls
    assert a == ([(x.data_ptr(), 36, 25 * 36)], NV16, 36, 25, 3, [(y.data_ptr(), 72, 50 * 72)], NV16) and s.sized == [(NV16, 36, 25)]
    with pytest.raises(ValueError):
        torch_io.upscale_yuv(s, _on_cuda0(torch.zeros(3, 25, 36, dtype=torch.uint8)), chroma=422)
    with pytest.raises(ValueError):  # a 4:4:4 call needs a context that knows the formats
        torch_io.upscale_yuv(Old(), _on_cuda0(torch.zeros(3, 25, 35, dtype=torch.uint8)), chroma=444)
