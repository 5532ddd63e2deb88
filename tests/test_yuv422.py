"""NV16 / P210 (YUV 4:2:2) without a GPU: the host-only functions (rsr_image_bytes, rsr_image_span, rsr_out_size_fmt), the ties of
tests/yuv422_ref.py to the 4:2:0 references, and what torch_io hands the engine with chroma=422 (a fake context and stream, as in
tests/test_yuv.py)."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

import yuv422_ref
import yuv_ref
import yuv_siting_ref
from pixfmt_ref import F16, F32, NV12, NV16, P010, P210, U8

F = np.float32
# the 67 ratios of one axis (rsr_set_out_ratio_xy): n / d in lowest terms, d in 1..8, 1 <= n / d <= 4
RATIOS = sorted({Fraction(n, d) for d in range(1, 9) for n in range(d, 4 * d + 1) if Fraction(n, d).denominator == d})


def test_constants_and_symbols_are_in_the_header_and_exported():
    text = open(os.path.join(R.INCLUDE_DIR, "realsr_hip.h")).read()
    for name, val in (("RSR_FMT_NV16", 8), ("RSR_FMT_P210", 9)):
        assert "#define %s %d " % (name, val) in text and getattr(R, name) == val
    assert "rsr_out_size_fmt" in R.EXPORTS and hasattr(R.lib(), "rsr_out_size_fmt")
    for needle in ("YUV 4:2:2", "Hs(y) * 0.25f", "(d(2X, y) + d(2X+1, y)) * 0.5f", "IS siting 1", "three-plane", "4:4:4", "4:1:1"):
        assert needle in text, needle
    assert len(RATIOS) == 67


def test_image_bytes_and_span():
    L = R.lib()
    for w, h in ((2, 1), (2, 2), (36, 25), (36, 26), (1280, 1080), (7680, 4320)):  # odd heights are taken
        assert L.rsr_image_bytes(NV16, w, h, 3) == 2 * w * h == R.image_bytes(NV16, w, h)
        assert L.rsr_image_bytes(P210, w, h, 3) == 4 * w * h == R.image_bytes(P210, w, h)
        assert R.image_span(NV16, w, h) == 2 * w * h and R.image_span(P210, w, h) == 4 * w * h
    assert L.rsr_image_bytes(P210, 8 * 7680, 8 * 4320, 3) == 4 * 64 * 7680 * 4320 > 2 ** 32  # a long long
    # pitched: the UV plane plane_pitch bytes behind Y(0,0), h rows of the Y rows' pitch, the last one w samples long
    assert R.image_span(NV16, 36, 25, 3, 64, 0) == 25 * 64 + 24 * 64 + 36
    assert R.image_span(NV16, 36, 25, 3, 64, 2000) == 2000 + 24 * 64 + 36
    assert R.image_span(NV16, 36, 25, 3, 37, 1001) == 1001 + 24 * 37 + 36          # NV16: any byte pitch
    assert R.image_span(P210, 36, 25, 3, 80, 0) == 25 * 80 + 24 * 80 + 72
    assert R.image_span(P210, 36, 25, 3, 80, 4000) == 4000 + 24 * 80 + 72
    assert R.image_span(NV16, 2, 1, 3, 0, 0) == 4
    assert R.image_span(NV16, 36, 25, 3, 64, (1 << 32) + 6) == (1 << 32) + 6 + 24 * 64 + 36


@pytest.mark.parametrize("fmt", [NV16, P210])
def test_argument_errors_that_need_no_context(fmt):
    L = R.lib()
    es = 1 if fmt == NV16 else 2
    for c in (1, 4):
        assert L.rsr_image_bytes(fmt, 8, 8, c) == R.RSR_E_ARG and L.rsr_image_span(fmt, 8, 8, c, 0, 0) == R.RSR_E_ARG
    for w, h in ((7, 8), (7, 7), (0, 8), (8, 0), (-2, 8)):  # an odd (or no) width; no height
        assert L.rsr_image_bytes(fmt, w, h, 3) == R.RSR_E_ARG, (w, h)
        assert L.rsr_image_span(fmt, w, h, 3, 0, 0) == R.RSR_E_ARG, (w, h)
    assert L.rsr_image_bytes(fmt, 8, 7, 3) == 2 * es * 8 * 7 == L.rsr_image_span(fmt, 8, 7, 3, 0, 0)  # an odd height is a surface
    assert L.rsr_image_span(fmt, 8, 8, 3, 8 * es - 1, 0) == R.RSR_E_ARG     # a row pitch below the bytes of a row
    assert L.rsr_image_span(fmt, 8, 8, 3, -16, 0) == R.RSR_E_ARG and L.rsr_image_span(fmt, 8, 8, 3, 0, -1) == R.RSR_E_ARG
    odd = L.rsr_image_span(fmt, 8, 8, 3, 8 * es + 1, 0), L.rsr_image_span(fmt, 8, 8, 3, 0, 8 * 8 * es + 1)
    if fmt == P210:  # 16-bit samples: an odd pitch is refused
        assert odd == (R.RSR_E_ARG, R.RSR_E_ARG)
    else:
        assert min(odd) > 0
    with pytest.raises(R.RealSRError) as e:
        R.image_bytes(fmt, 9, 8)
    assert e.value.code == R.RSR_E_ARG
    assert L.rsr_process_device_fmt(None, None, fmt, 8, 8, 3, None, fmt, None) == R.RSR_E_ARG
    for bad in (3, 6, 7, 10, -1):  # the ids around the new ones stay unknown
        assert L.rsr_image_bytes(bad, 8, 8, 3) == R.RSR_E_ARG


# ---- rsr_out_size_fmt --------------------------------------------------------------------------------------------------------------
def _call(fn, *a):
    ow, oh = C.c_int(-7), C.c_int(-7)
    rc = fn(*a, C.byref(ow), C.byref(oh))
    return (rc, ow.value, oh.value) if rc == 0 else (rc, R.lib().rsr_last_error(None).decode())


@pytest.mark.parametrize("w,h,tile", [(36, 26, 16), (35, 25, 24), (1280, 1080, 200), (720, 576, 192), (48, 28, 33)])
def test_out_size_fmt_is_the_old_rule_for_the_old_formats(w, h, tile):
    L = R.lib()
    for rx in RATIOS:
        for ry in RATIOS:
            a = (rx.numerator, rx.denominator, ry.numerator, ry.denominator, tile, w, h)
            rgb, yuv = _call(L.rsr_out_size_xy, *a), _call(L.rsr_out_size_yuv_xy, *a)
            for fmt in (U8, F16, F32):
                assert _call(L.rsr_out_size_fmt, fmt, *a) == rgb, (fmt, a)
            for fmt in (NV12, P010):
                assert _call(L.rsr_out_size_fmt, fmt, *a) == yuv, (fmt, a)


def rule422(rx, ry, tile, w, h):
    """The 4:2:2 admission rule restated: None = refused by the ratio rule, "YUV" = refused by the parity of the columns alone."""
    if (w * rx).denominator != 1 or (tile * rx).denominator != 1 or (h * ry).denominator != 1 or (tile * ry).denominator != 1:
        return None
    if int(w * rx) % 2 or int(tile * rx) % 2:
        return "YUV"
    return int(w * rx), int(h * ry)


@pytest.mark.parametrize("w,h,tile", [(36, 26, 16), (36, 25, 16), (35, 25, 24), (1280, 1080, 200), (36, 26, 30), (48, 28, 24), (48, 28, 33)])
def test_out_size_fmt_states_the_422_rule(w, h, tile):
    L = R.lib()
    taken = parity = 0
    for rx in RATIOS:
        for ry in RATIOS:
            want = rule422(rx, ry, tile, w, h)
            for fmt in (NV16, P210):
                got = _call(L.rsr_out_size_fmt, fmt, rx.numerator, rx.denominator, ry.numerator, ry.denominator, tile, w, h)
                if want is None:
                    assert got[0] == R.RSR_E_ARG, (rx, ry, got)
                elif want == "YUV":
                    assert got[0] == R.RSR_E_ARG and "YUV" in got[1], (rx, ry, got)
                    parity += 1
                else:
                    assert got == (0,) + want, (rx, ry, got)
                    taken += 1
    assert taken > 0 and (parity > 0 or tile % 2 == 0 and w % 2 == 0)


def test_out_size_fmt_examples_and_refusals():
    L = R.lib()
    f = lambda *a: _call(L.rsr_out_size_fmt, *a)  # noqa: E731
    assert f(P210, 3, 2, 1, 1, 200, 1280, 1080) == (0, 1920, 1080)             # DVCPRO-HD to 1080p
    assert f(NV16, 3, 2, 3, 2, 16, 36, 26) == (0, 54, 39)                      # an odd output height: taken here ...
    assert f(NV12, 3, 2, 3, 2, 16, 36, 26)[0] == R.RSR_E_ARG                   # ... and refused for NV12
    assert f(NV16, 6, 4, 3, 2, 16, 36, 26) == (0, 54, 39)                      # ratios are reduced first
    got = f(NV16, 3, 2, 3, 2, 30, 36, 26)                                      # 45 columns per tile
    assert got[0] == R.RSR_E_ARG and "YUV" in got[1]
    got = f(NV16, 1, 1, 1, 1, 33, 36, 25)                                      # out_scale 1 at an odd tile size
    assert got[0] == R.RSR_E_ARG and "YUV" in got[1]
    assert f(NV16, 1, 1, 1, 1, 16, 36, 25) == (0, 36, 25) and f(NV16, 4, 1, 4, 1, 33, 35, 25) == (0, 140, 100)
    for bad in (3, 6, 7, 10, -1):
        assert f(bad, 4, 1, 4, 1, 16, 36, 26)[0] == R.RSR_E_ARG
    assert f(NV16, 9, 2, 1, 1, 16, 36, 26)[0] == R.RSR_E_ARG and f(NV16, 4, 1, 4, 1, 0, 36, 26)[0] == R.RSR_E_ARG
    assert L.rsr_out_size_fmt(NV16, 4, 1, 4, 1, 16, 36, 25, None, None) == 0   # either pointer may be NULL


# ---- the new reference against the existing ones -----------------------------------------------------------------------------------
@pytest.mark.parametrize("siting", [0, 1, 2])
@pytest.mark.parametrize("bits", [8, 10])
def test_decode_tie_equal_chroma_rows(siting, bits):
    """A surface whose chroma rows are all equal has nothing to filter vertically: the 4:2:2 decode is the 4:2:0 decode, bit for bit."""
    rng = np.random.default_rng(5 + bits + siting)
    w, h = 22, 12
    y = rng.integers(0, 1 << bits, size=(h, w))
    row = rng.integers(0, 1 << bits, size=(1, w // 2, 2))
    uv422, uv420 = np.repeat(row, h, axis=0), np.repeat(row, h // 2, axis=0)
    for matrix, full in ((709, 0), (601, 1), (2020, 0)):
        got = yuv422_ref.decode(y, uv422, matrix, full, bits, siting)
        want = yuv_siting_ref.decode(y, uv420, siting, matrix, full, bits)
        assert got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        if siting == 0:
            assert np.array_equal(want, yuv_ref.decode(y, uv420, matrix, full, bits))
    assert np.array_equal(yuv422_ref.decode(y, uv422, 709, 0, bits, 2), yuv422_ref.decode(y, uv422, 709, 0, bits, 1))


@pytest.mark.parametrize("siting", [0, 1, 2])
@pytest.mark.parametrize("bits", [8, 10])
def test_encode_tie_equal_rows(siting, bits):
    """An image whose rows are all equal: the quad mean of two equal rows is (a + b) * 0.5f exactly, and (Hs + Hs) * 0.125f = Hs * 0.25f (top-left:
    ((Hs + Hs) + (Hs + Hs)) * 0.0625f) -- the 4:2:2 chroma rows are the 4:2:0 encode's, the luma rows the same."""
    rng = np.random.default_rng(9 + bits + siting)
    w, h, tile_w = 40, 8, 16
    d = np.repeat(rng.uniform(0, 1, size=(3, 1, w)).astype(F), h, axis=1)
    for matrix, full in ((709, 0), (601, 1), (2020, 1)):
        y2, uv2 = yuv422_ref.encode(d, matrix, full, bits, siting, tile_w)
        y0, uv0 = yuv_siting_ref.encode(d, siting, tile_w, matrix, full, bits)
        assert uv2.shape == (h, w // 2, 2) and uv0.shape == (h // 2, w // 2, 2)
        assert np.array_equal(y2, y0) and np.array_equal(uv2[0::2], uv0) and np.array_equal(uv2[1::2], uv0)
    if siting:  # the tile-first clamp is in: columns 16 and 32 differ from the unclamped filter
        free = yuv422_ref.encode(d, 709, 0, bits, siting, 0)[1]
        cols = np.flatnonzero((free != yuv422_ref.encode(d, 709, 0, bits, siting, tile_w)[1]).any(axis=(0, 2)))
        assert len(cols) and set(cols) <= {8, 16}


def test_split_and_join_are_inverse_and_odd_heights_work():
    rng = np.random.default_rng(3)
    for bits, dt in ((8, np.uint8), (10, np.uint16)):
        s = (rng.integers(0, 1 << bits, size=(2 * 7, 10)) << (0 if bits == 8 else 6)).astype(dt)
        y, uv = yuv422_ref.split(s, bits)
        assert y.shape == (7, 10) and uv.shape == (7, 5, 2) and np.array_equal(yuv422_ref.join(y, uv, bits), s)
        rgb = yuv422_ref.decode(y, uv, 709, 0, bits, 1)
        assert rgb.shape == (3, 7, 10)
        y2, uv2 = yuv422_ref.encode(rgb, 709, 0, bits, 0)
        assert y2.shape == (7, 10) and uv2.shape == (7, 5, 2)


# ---- torch_io with chroma=422: what it hands the engine ----------------------------------------------------------------------------
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


def test_upscale_yuv_422_describes_a_surface_and_sizes_the_result(fake_stream):
    s = _Ctx()
    x = _on_cuda0(torch.zeros(50, 36, dtype=torch.uint8))  # 36 x 25 NV16
    out = _on_cuda0(torch.zeros(100, 72, dtype=torch.uint8))
    assert torch_io.upscale_yuv(s, x, out=out, chroma=422) is out
    (a, k), = s.calls
    assert a == ([(x.data_ptr(), 36, 25 * 36)], NV16, 36, 25, 3, [(out.data_ptr(), 72, 50 * 72)], NV16) and k == {"stream": 5}
    assert s.sized == [(NV16, 36, 25)]
    # P210 as int16, rows of a padded surface: the pitch in bytes, the UV plane where the view puts it
    s = _Ctx()
    big = torch.zeros(64, 64, dtype=torch.int16)
    x = _on_cuda0(big[:50, :36])
    y = torch_io.upscale_yuv(s, x, chroma=422)
    (a, k), = s.calls
    assert a[0] == [(big.data_ptr(), 128, 25 * 128)] and a[1] == P210 and a[6] == P210 and a[5][0][1:] == (144, 50 * 144)
    assert tuple(y.shape) == (100, 72) and y.dtype == torch.int16
    # at a ratio: 36 x 26 at 3/2 is 54 x 39 -- an odd height
    s = _Ctx((Fraction(3, 2), Fraction(3, 2)))
    y = torch_io.upscale_yuv(s, _on_cuda0(torch.zeros(52, 36, dtype=torch.uint8)), chroma=422)
    assert tuple(y.shape) == (78, 54) and s.calls[0][0][5] == [(y.data_ptr(), 54, 39 * 54)]


def test_upscale_yuv_422_takes_a_pair_of_planes(fake_stream):
    s = _Ctx()
    pool = torch.zeros(8192, dtype=torch.uint8)
    y = _on_cuda0(pool[:25 * 40].view(25, 40)[:, :36])
    uv = _on_cuda0(pool[2000:2000 + 25 * 40].view(25, 40)[:, :36])
    oy, ouv = torch_io.upscale_yuv(s, (y, uv), chroma=422)
    (a, k), = s.calls
    assert a[0] == [(pool.data_ptr(), 40, 2000)] and a[1:5] == (NV16, 36, 25, 3)
    assert tuple(oy.shape) == (50, 72) and tuple(ouv.shape) == (50, 72) and oy.dtype == torch.uint8
    # a uv plane BELOW y in memory has no plane pitch: the pair is packed into one allocation first
    s = _Ctx()
    torch_io.upscale_yuv(s, (_on_cuda0(pool[2000:2000 + 25 * 36].view(25, 36)), _on_cuda0(pool[:25 * 36].view(25, 36))), chroma=422)
    (a, k), = s.calls
    assert a[0][0][1:] == (36, 25 * 36) and a[0][0][0] not in (pool.data_ptr(), pool.data_ptr() + 2000)


@pytest.mark.parametrize("x", [
    torch.zeros(50, 36, dtype=torch.uint8),                       # wrong device (CPU)
    _on_cuda0(torch.zeros(50, 35, dtype=torch.uint8)),            # odd width
    _on_cuda0(torch.zeros(51, 36, dtype=torch.uint8)),            # rows that are not 2 h
    _on_cuda0(torch.zeros(50, 36, dtype=torch.float16)),          # dtype
    _on_cuda0(torch.zeros(3, 25, 36, dtype=torch.uint8)),         # not a surface
    (_on_cuda0(torch.zeros(26, 36, dtype=torch.uint8)), _on_cuda0(torch.zeros(13, 36, dtype=torch.uint8))),  # a 4:2:0 pair
    (_on_cuda0(torch.zeros(25, 36, dtype=torch.uint8)), _on_cuda0(torch.zeros(25, 18, dtype=torch.uint8))),  # uv rows are w samples long
    (_on_cuda0(torch.zeros(25, 36, dtype=torch.uint8)), _on_cuda0(torch.zeros(25, 36, dtype=torch.int16))),  # mixed depths
], ids=lambda x: "pair" if isinstance(x, tuple) else "%s-%s" % (str(x.dtype).split(".")[-1], "x".join(map(str, x.shape))))
def test_upscale_yuv_422_rejects_bad_surfaces_before_launching(fake_stream, x):
    s = _Ctx()
    with pytest.raises(ValueError):
        torch_io.upscale_yuv(s, x, chroma=422)
    assert s.calls == []


def test_upscale_yuv_422_refuses_what_the_engine_would(fake_stream):
    s = _Ctx((Fraction(3, 2), Fraction(3, 2)))
    s.tilesize = 30  # 45 columns per tile
    with pytest.raises(ValueError, match="YUV"):
        torch_io.upscale_yuv(s, _on_cuda0(torch.zeros(52, 36, dtype=torch.uint8)), chroma=422)
    s = _Ctx()
    with pytest.raises(ValueError):
        torch_io.upscale_yuv(s, _on_cuda0(torch.zeros(50, 36, dtype=torch.uint8)), chroma=444)
    with pytest.raises(ValueError):  # out of the wrong size
        torch_io.upscale_yuv(s, _on_cuda0(torch.zeros(50, 36, dtype=torch.uint8)), out=_on_cuda0(torch.zeros(78, 72, dtype=torch.uint8)), chroma=422)
    assert s.calls == []


def test_chroma_420_calls_are_todays(fake_stream):
    """chroma=420 -- given or not -- sizes, describes and refuses as before: a context without out_size_fmt serves it."""
    class Old:
        gpuid, scale, out_scale = 0, 4, 2

        def __init__(self):
            self.calls = []

        def process_device_batch(self, *a, **k):
            self.calls.append((a, k))

    x = _on_cuda0(torch.zeros(39, 36, dtype=torch.uint8))  # 36 x 26 NV12
    got = []
    for kw in ({}, {"chroma": 420}):
        s = Old()
        y = torch_io.upscale_yuv(s, x, **kw)
        (a, k), = s.calls
        assert a == ([(x.data_ptr(), 36, 26 * 36)], NV12, 36, 26, 3, [(y.data_ptr(), 72, 52 * 72)], NV12) and k == {"stream": 5}
        got.append(tuple(y.shape))
        with pytest.raises(ValueError):
            torch_io.upscale_yuv(s, _on_cuda0(torch.zeros(38, 36, dtype=torch.uint8)), **kw)  # rows that are not 3 h / 2 with an even h
        with pytest.raises(ValueError):
            torch_io.upscale_yuv(s, _on_cuda0(torch.zeros(50, 36, dtype=torch.uint8)), **kw)  # a 4:2:2 surface is no 4:2:0 surface
        assert len(s.calls) == 1
    assert got == [(78, 72), (78, 72)]
    with pytest.raises(ValueError):  # ... and a 4:2:2 call needs a context that knows the formats
        torch_io.upscale_yuv(Old(), _on_cuda0(torch.zeros(50, 36, dtype=torch.uint8)), chroma=422)
