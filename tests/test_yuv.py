"""NV12 / P010 device images (RSR_FMT_NV12, RSR_FMT_P010; options "yuv_matrix", "yuv_range"): what can be said without a GPU -- the C
ABI, buffer sizes and spans, the argument errors that need no context, the constants of the definition, and the numpy restatement
(tests/yuv_ref.py) the device tests compare against.  The device side is tests/test_gpu_yuv.py; the errors and the option validation that
need a context (an odd tile at out_scale 1, an odd P010 pointer, a bad matrix) are checked there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

import yuv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8, F16, F32, NV12, P010 = R.RSR_FMT_U8_HWC, R.RSR_FMT_F16_CHW, R.RSR_FMT_F32_CHW, R.RSR_FMT_NV12, R.RSR_FMT_P010
CONFIGS = [(m, full, bits) for m in (709, 601, 2020) for full in (0, 1) for bits in (8, 10)]


def test_constants_and_symbols_are_in_the_header_and_exported():
    text = open(os.path.join(R.INCLUDE_DIR, "realsr_hip.h")).read()
    for name, val in (("RSR_FMT_NV12", 4), ("RSR_FMT_P010", 5)):
        assert "#define %s %d " % (name, val) in text and getattr(R, name) == val
    assert "rsr_yuv_constants" in R.EXPORTS and hasattr(R.lib(), "rsr_yuv_constants")
    for needle in ('"yuv_matrix"', '"yuv_range"', "(3 * c_near + c_far) * 0.25f", "0.2126 / 0.0722", "0.299 / 0.114", "0.2627 / 0.0593",
                   "floor(Y' * yscale + (yoff + 0.5f))", "code << 6", "CENTRE"):
        assert needle in text, needle


def test_image_bytes_and_span():
    L = R.lib()
    for w, h in ((2, 2), (36, 26), (1920, 1080), (7680, 4320)):
        assert L.rsr_image_bytes(NV12, w, h, 3) == w * h * 3 // 2 == R.image_bytes(NV12, w, h)
        assert L.rsr_image_bytes(P010, w, h, 3) == 3 * w * h == R.image_bytes(P010, w, h)
        assert R.image_span(NV12, w, h) == w * h * 3 // 2 and R.image_span(P010, w, h) == 3 * w * h
    assert L.rsr_image_bytes(P010, 8 * 7680, 8 * 4320, 3) == 3 * 64 * 7680 * 4320 > 2 ** 32  # a long long
    # pitched: the UV plane plane_pitch bytes behind Y(0,0), h / 2 rows of the Y rows' pitch, the last one w samples long
    assert R.image_span(NV12, 36, 26, 3, 64, 0) == 26 * 64 + 12 * 64 + 36
    assert R.image_span(NV12, 36, 26, 3, 64, 2000) == 2000 + 12 * 64 + 36
    assert R.image_span(NV12, 36, 26, 3, 37, 1001) == 1001 + 12 * 37 + 36          # NV12: any byte pitch
    assert R.image_span(P010, 36, 26, 3, 80, 0) == 26 * 80 + 12 * 80 + 72
    assert R.image_span(P010, 36, 26, 3, 80, 4000) == 4000 + 12 * 80 + 72
    assert R.image_span(NV12, 2, 2, 3, 0, 0) == 6


@pytest.mark.parametrize("fmt", [NV12, P010])
def test_argument_errors_that_need_no_context(fmt):
    L = R.lib()
    es = 1 if fmt == NV12 else 2
    for c in (1, 4):
        assert L.rsr_image_bytes(fmt, 8, 8, c) == R.RSR_E_ARG and L.rsr_image_span(fmt, 8, 8, c, 0, 0) == R.RSR_E_ARG
    for w, h in ((7, 8), (8, 7), (7, 7), (0, 8), (8, 0), (-2, 8)):  # an odd (or no) width or height
        assert L.rsr_image_bytes(fmt, w, h, 3) == R.RSR_E_ARG, (w, h)
        assert L.rsr_image_span(fmt, w, h, 3, 0, 0) == R.RSR_E_ARG, (w, h)
    assert L.rsr_image_span(fmt, 8, 8, 3, 8 * es - 1, 0) == R.RSR_E_ARG     # a row pitch below the bytes of a row
    assert L.rsr_image_span(fmt, 8, 8, 3, -16, 0) == R.RSR_E_ARG and L.rsr_image_span(fmt, 8, 8, 3, 0, -1) == R.RSR_E_ARG
    odd = L.rsr_image_span(fmt, 8, 8, 3, 8 * es + 1, 0), L.rsr_image_span(fmt, 8, 8, 3, 0, 8 * 8 * es + 1)
    if fmt == P010:  # 16-bit samples: an odd pitch is refused
        assert odd == (R.RSR_E_ARG, R.RSR_E_ARG)
    else:
        assert min(odd) > 0
    with pytest.raises(R.RealSRError) as e:
        R.image_bytes(fmt, 9, 8)
    assert e.value.code == R.RSR_E_ARG
    # a null context is an argument error on every entry point, whatever the formats
    assert L.rsr_process_device_fmt(None, None, fmt, 8, 8, 3, None, fmt, None) == R.RSR_E_ARG
    assert L.rsr_process_device_batch(None, 1, None, fmt, 8, 8, 3, None, F16, None) == R.RSR_E_ARG
    assert L.rsr_set_option(None, b"yuv_matrix", 601) == R.RSR_E_ARG and L.rsr_set_option(None, b"yuv_range", 1) == R.RSR_E_ARG


def test_ids_3_and_7_stay_unknown():
    L = R.lib()
    for fmt in (3, 6, 7, -1):
        assert L.rsr_image_bytes(fmt, 8, 8, 3) == R.RSR_E_ARG and L.rsr_image_span(fmt, 8, 8, 3, 0, 0) == R.RSR_E_ARG


@pytest.mark.parametrize("matrix,full,bits", CONFIGS)
def test_library_constants_are_the_reference_constants(matrix, full, bits):
    """Both sides compute in double from Kr and Kb and round once: the 18 float32 values agree bit for bit."""
    want = np.array([yuv_ref.constants(matrix, full, bits)[n] for n in yuv_ref.NAMES], dtype=np.float32)
    got = R.yuv_constants(matrix, full, bits)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    k = 1 << (bits - 8)
    assert want[yuv_ref.NAMES.index("coff")] == 128 * k and want[yuv_ref.NAMES.index("maxcode")] == (1 << bits) - 1
    assert want[yuv_ref.NAMES.index("yscale")] == ((1 << bits) - 1 if full else 219 * k)
    assert want[yuv_ref.NAMES.index("cscale")] == ((1 << bits) - 1 if full else 224 * k)
    assert want[yuv_ref.NAMES.index("yadd")] == (0 if full else 16 * k) + 0.5


def test_constants_refuse_what_the_options_refuse():
    out = (C.c_float * 18)()
    L = R.lib()
    for matrix, full, bits in ((0, 0, 8), (708, 0, 8), (709, 2, 8), (709, -1, 8), (709, 0, 9), (709, 0, 12), (2021, 1, 10)):
        assert L.rsr_yuv_constants(matrix, full, bits, out, 18) == R.RSR_E_ARG
    assert L.rsr_yuv_constants(709, 0, 8, None, 18) == R.RSR_E_ARG
    with pytest.raises(R.RealSRError):
        R.yuv_constants(470)


def test_reference_decodes_the_anchor_codes():
    """Limited range: (16, 128, 128) is black and (235, 128, 128) white; full range: (0, 128, 128) and (255, 128, 128); x4 at 10 bits."""
    for matrix, full, bits in CONFIGS:
        k = 1 << (bits - 8)
        lo, hi = (0, (1 << bits) - 1) if full else (16 * k, 235 * k)
        y = np.array([[lo, hi], [hi, lo]])
        uv = np.full((1, 1, 2), 128 * k)
        rgb = yuv_ref.decode(y, uv, matrix, full, bits)
        assert np.array_equal(rgb[:, 0, 0], [0, 0, 0]) and np.array_equal(rgb[:, 0, 1], [1, 1, 1]), (matrix, full, bits, rgb)
        y2, uv2 = yuv_ref.encode(rgb, matrix, full, bits)
        assert np.array_equal(y2, y) and np.array_equal(uv2, uv)


def test_reference_chroma_weights_and_clamp():
    """Centre siting: luma column 2k takes 3/4 of chroma k and 1/4 of k - 1, column 2k + 1 1/4 of k + 1; the edge repeats its sample.
    With Y at the neutral code and full range, R - yn = rv * cr shows the interpolated V directly."""
    c = yuv_ref.constants(709, 1, 8)
    v = np.array([100, 140, 180, 60])
    uv = np.empty((1, 4, 2), dtype=np.int64)
    uv[0, :, 0], uv[0, :, 1] = 128, v
    y = np.full((2, 8), 128)
    rgb = yuv_ref.decode(y, uv, 709, 1, 8)
    want_v = np.array([100, 110, 130, 150, 170, 150, 90, 60], dtype=np.float32)  # (3 near + far) / 4
    yn = np.float32(128) * c["ys"]
    want_r = (yn + c["rv"] * ((want_v - c["coff"]) * c["cs"])).astype(np.float16).astype(np.float32)
    assert np.array_equal(rgb[0, 0], want_r) and np.array_equal(rgb[0, 1], want_r)
    # out of gamut: the clamp acts
    sat = yuv_ref.decode(np.full((2, 2), 255), np.array([[[255, 255]]]), 709, 0, 8)
    assert sat.max() == 1 and yuv_ref.decode(np.full((2, 2), 0), np.array([[[0, 0]]]), 709, 0, 8)[0].max() == 0


def test_split_and_join_are_inverse():
    rng = np.random.default_rng(3)
    s8 = rng.integers(0, 256, size=(39, 36), dtype=np.uint8)
    assert np.array_equal(yuv_ref.join(*yuv_ref.split(s8, 8), 8), s8)
    s10 = (rng.integers(0, 1024, size=(39, 36)) << 6).astype(np.uint16)
    y, uv = yuv_ref.split(s10, 10)
    assert y.shape == (26, 36) and uv.shape == (13, 18, 2) and y.max() < 1024
    assert np.array_equal(yuv_ref.join(y, uv, 10), s10)
    assert np.array_equal(yuv_ref.split(s10.view(np.int16), 10)[0], y)  # torch has no uint16 arithmetic: int16 tensors carry P010 too


@pytest.mark.parametrize("matrix,full,bits", CONFIGS)
def test_reference_round_trip(matrix, full, bits):
    """encode -> decode -> encode of an RGB image whose chroma is constant over every 2 x 2 quad reproduces the codes within +-1.  The
    image is the decode of a random surface: random luma per pixel, and -- the decoder interpolates chroma between neighbouring samples,
    so chroma that is constant over every quad of the IMAGE means chroma that does not vary over the surface -- one random (U, V) pair per
    surface, 40 surfaces per configuration, all inside the gamut (luma 0.2 .. 0.8, |Cb|, |Cr| <= 0.1: a clamped colour has no code of its
    own to come back to).  Measured bound: 0 in all twelve configurations, for the luma and the chroma codes, against the surface and
    between the two encodes.  (An fp16 in [0.5, 1) is at most 2^-12 from the fp32 value, 0.21 of a 10-bit code: never enough to cross
    the .5 the encoder floors at, from a decoded code that sits on an integer.)  Asserted as measured, which implies the +-1."""
    rng = np.random.default_rng(1000 * matrix + 10 * full + bits)
    k, top = 1 << (bits - 8), (1 << bits) - 1
    yoff, yscale, cscale = (0, top, top) if full else (16 * k, 219 * k, 224 * k)
    worst = 0
    for _ in range(40):
        y = rng.integers(yoff + int(0.2 * yscale), yoff + int(0.8 * yscale) + 1, size=(32, 48))
        uv = np.empty((16, 24, 2), dtype=np.int64)
        uv[...] = rng.integers(int(-0.1 * cscale), int(0.1 * cscale) + 1, size=2) + 128 * k
        img = yuv_ref.decode(y, uv, matrix, full, bits)
        assert 0 < img.min() and img.max() < 1
        y1, uv1 = yuv_ref.encode(img, matrix, full, bits)
        y2, uv2 = yuv_ref.encode(yuv_ref.decode(y1, uv1, matrix, full, bits), matrix, full, bits)
        worst = max(worst, np.abs(y1 - y).max(), np.abs(uv1 - uv).max(), np.abs(y2 - y1).max(), np.abs(uv2 - uv1).max())
    print("round trip %d range %d %d bits: worst code difference %d" % (matrix, full, bits, worst))
    assert worst <= 1
    assert worst == 0


def test_header_with_the_yuv_api_is_plain_c_and_a_c_host_reaches_it(tmp_path):
    src = tmp_path / "host.c"
    src.write_text(r'''
#include <stdio.h>
#include "realsr_hip.h"
int main(void)
{
    float k[18];
    long long a = rsr_image_bytes(RSR_FMT_NV12, 10, 6, 3), b = rsr_image_bytes(RSR_FMT_P010, 10, 6, 3);
    long long c = rsr_image_bytes(RSR_FMT_NV12, 9, 6, 3), d = rsr_image_span(RSR_FMT_P010, 10, 6, 3, 21, 0);
    int rc = rsr_yuv_constants(601, 1, 10, k, 18), bad = rsr_yuv_constants(601, 1, 9, k, 18);
    int nul = rsr_process_device_fmt(NULL, NULL, RSR_FMT_NV12, 10, 6, 3, NULL, RSR_FMT_P010, NULL);
    printf("bytes %lld %lld bad %lld %lld k %d %d %.1f %.1f null %d\n", a, b, c, d, rc, bad, k[2], k[17], nul);
    return 0;
}
''')
    lib = os.path.join(ROOT, "realsr-ncnn-vulkan_amd", "lib")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(inc, "realsr_hip.h")])
    exe = str(tmp_path / "host")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", inc, "-o", exe, str(src), "-L", lib, "-lrealsr_hip", "-Wl,-rpath," + lib])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bytes 90 180 bad -1 -1 k 0 -1 512.0 1023.0 null -1" in r.stdout, r.stdout


# ---- torch_io.upscale_yuv: what it hands the engine -------------------------------------------------------------------------------
class _Stream:
    cuda_stream = 5  # (not the null stream: the call is enqueued on it directly)


class _Ctx:
    gpuid, scale, out_scale = 0, 4, 2

    def __init__(self):
        self.calls = []

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


def test_upscale_yuv_describes_a_surface_and_sizes_the_result(fake_stream):
    s = _Ctx()
    x = _on_cuda0(torch.zeros(39, 36, dtype=torch.uint8))  # 36 x 26 NV12
    out = _on_cuda0(torch.zeros(78, 72, dtype=torch.uint8))
    assert torch_io.upscale_yuv(s, x, out=out) is out
    (a, k), = s.calls
    assert a == ([(x.data_ptr(), 36, 26 * 36)], NV12, 36, 26, 3, [(out.data_ptr(), 72, 52 * 72)], NV12) and k == {"stream": 5}
    # P010 as int16, rows of a padded decoder surface: the pitch in bytes, the UV plane where the view puts it
    s = _Ctx()
    big = torch.zeros(48, 64, dtype=torch.int16)
    x = _on_cuda0(big[:39, :36])
    torch_io.upscale_yuv(s, x, out=_on_cuda0(torch.zeros(78, 72, dtype=torch.int16)))
    (a, k), = s.calls
    assert a[0] == [(big.data_ptr(), 128, 26 * 128)] and a[1] == P010 and a[5][0][1:] == (144, 52 * 144)


def test_upscale_yuv_takes_a_pair_of_planes(fake_stream):
    s = _Ctx()
    pool = torch.zeros(4096, dtype=torch.uint8)
    y = _on_cuda0(pool[:26 * 40].view(26, 40)[:, :36])
    uv = _on_cuda0(pool[2000:2000 + 13 * 40].view(13, 40)[:, :36])
    oy, ouv = torch_io.upscale_yuv(s, (y, uv))
    (a, k), = s.calls
    assert a[0] == [(pool.data_ptr(), 40, 2000)] and a[2:5] == (36, 26, 3)
    assert tuple(oy.shape) == (52, 72) and tuple(ouv.shape) == (26, 72) and oy.dtype == torch.uint8
    # a uv plane BELOW y in memory has no plane pitch: the pair is packed into one allocation first
    s = _Ctx()
    torch_io.upscale_yuv(s, (_on_cuda0(pool[2000:2000 + 26 * 36].view(26, 36)), _on_cuda0(pool[:13 * 36].view(13, 36))))
    (a, k), = s.calls
    assert a[0][0][1:] == (36, 26 * 36) and a[0][0][0] not in (pool.data_ptr(), pool.data_ptr() + 2000)


@pytest.mark.parametrize("x", [
    torch.zeros(39, 36, dtype=torch.uint8),                       # wrong device (CPU)
    _on_cuda0(torch.zeros(39, 35, dtype=torch.uint8)),            # odd width
    _on_cuda0(torch.zeros(38, 36, dtype=torch.uint8)),            # rows that are not 3 h / 2 with an even h
    _on_cuda0(torch.zeros(39, 36, dtype=torch.float16)),          # dtype
    _on_cuda0(torch.zeros(3, 26, 36, dtype=torch.uint8)),         # not a surface
    (_on_cuda0(torch.zeros(26, 36, dtype=torch.uint8)), _on_cuda0(torch.zeros(13, 18, dtype=torch.uint8))),  # uv rows are w samples long
    (_on_cuda0(torch.zeros(26, 36, dtype=torch.uint8)), _on_cuda0(torch.zeros(13, 36, dtype=torch.int16))),  # mixed depths
], ids=lambda x: "pair" if isinstance(x, tuple) else "%s-%s" % (str(x.dtype).split(".")[-1], "x".join(map(str, x.shape))))
def test_upscale_yuv_rejects_bad_surfaces_before_launching(fake_stream, x):
    s = _Ctx()
    with pytest.raises(ValueError):
        torch_io.upscale_yuv(s, x)
    assert s.calls == []
