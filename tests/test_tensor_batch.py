"""Tensor batches and strided device images (rsr_process_device_batch, rsr_image_span, torch_io.describe, upscale(..., out=)): what can
be said without a GPU -- the C ABI, the size arithmetic, which views fit a descriptor, argument checking.  The device side is
tests/test_gpu_tensor_batch.py."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rsr_process_device_batch", "rsr_image_span")
U8, F16, F32 = R.RSR_FMT_U8_HWC, R.RSR_FMT_F16_CHW, R.RSR_FMT_F32_CHW


def test_symbols_and_struct_mirror():
    assert set(NEW_SYMBOLS) <= set(R.EXPORTS)
    for s in NEW_SYMBOLS:
        assert hasattr(R.lib(), s), s
    assert C.sizeof(R.Image) == 24 and [f[0] for f in R.Image._fields_] == ["data", "row_pitch", "plane_pitch"]


def test_header_is_plain_c_and_a_c_host_reaches_the_batch_api(tmp_path):
    """include/realsr_hip.h still compiles as C99 -pedantic; a host written in C links the two new symbols, sees a 24-byte rsr_image and
    gets the spans and the argument errors without a GPU."""
    src = tmp_path / "host.c"
    src.write_text(r'''
#include <stdio.h>
#include "realsr_hip.h"
int main(void)
{
    rsr_image im;
    long long a = rsr_image_span(RSR_FMT_U8_HWC, 10, 7, 3, 0, 0), b = rsr_image_span(RSR_FMT_U8_HWC, 10, 7, 3, 31, 0);
    long long c = rsr_image_span(RSR_FMT_F16_CHW, 10, 7, 3, 64, 1000), d = rsr_image_span(RSR_FMT_F32_CHW, 10, 7, 3, 39, 0);
    int rc;
    im.data = NULL; im.row_pitch = 0; im.plane_pitch = 0;
    rc = rsr_process_device_batch(NULL, 1, &im, RSR_FMT_F16_CHW, 10, 7, 3, &im, RSR_FMT_F32_CHW, NULL);
    printf("size %d span %lld %lld %lld bad %lld null %d\n", (int)sizeof(rsr_image), a, b, c, d, rc);
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
    # 6 * 31 + 30 = 216;  2 * 1000 + 6 * 64 + 20 = 2404
    assert "size 24 span 210 216 2404 bad -1 null -1" in r.stdout, r.stdout
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(lib, "librealsr_hip.so")], text=True)
    for s in NEW_SYMBOLS:
        assert " T %s\n" % s in out, s


def test_image_span():
    L = R.lib()
    for w, h in ((1, 1), (61, 47), (1920, 1080), (4 * 7680, 4 * 4320)):
        for fmt, c in ((U8, 3), (U8, 4), (F16, 3), (F32, 3)):
            assert L.rsr_image_span(fmt, w, h, c, 0, 0) == L.rsr_image_bytes(fmt, w, h, c) > 0
            es = {U8: c, F16: 2, F32: 4}[fmt]
            assert L.rsr_image_span(fmt, w, h, c, w * es, 0) == L.rsr_image_bytes(fmt, w, h, c)  # the packed pitch, spelled out
    # pitched: the last row is not padded
    assert R.image_span(U8, 61, 47, 3, 61 * 3 + 1) == 46 * 184 + 183
    assert R.image_span(U8, 61, 47, 4, 300) == 46 * 300 + 244
    assert R.image_span(U8, 61, 47, 3, 200, 12345) == 46 * 200 + 183                  # the plane pitch of a uint8 image is ignored
    assert R.image_span(F16, 61, 47, 3, 128) == 2 * 47 * 128 + 46 * 128 + 122           # plane pitch 0 = h * row pitch
    assert R.image_span(F32, 61, 47, 3, 256, 20000) == 2 * 20000 + 46 * 256 + 244
    assert R.image_span(F32, 61, 47, 3, 0, 20000) == 2 * 20000 + 46 * 244 + 244
    assert R.image_span(F16, 61, 47, 3, 3 * 122, 122) == 2 * 122 + 46 * 366 + 122       # planes interleaved by rows: [h][3][w]
    bad = [(7, 8, 8, 3, 0, 0), (-1, 8, 8, 3, 0, 0), (F16, 8, 8, 4, 0, 0), (F32, 8, 8, 1, 0, 0), (U8, 8, 8, 5, 0, 0),  # format / channels
           (U8, 0, 8, 3, 0, 0), (F16, 8, -1, 3, 0, 0),
           (U8, 8, 8, 3, 23, 0), (U8, 8, 8, 4, 31, 0), (F16, 8, 8, 3, 14, 0), (F32, 8, 8, 3, 28, 0),                 # row pitch below a row
           (F16, 8, 8, 3, 17, 0), (F32, 8, 8, 3, 34, 0), (F16, 8, 8, 3, 16, 129), (F32, 8, 8, 3, 32, 258),            # not element multiples
           (U8, 8, 8, 3, -24, 0), (F16, 8, 8, 3, -16, 0), (F16, 8, 8, 3, 16, -128), (U8, 8, 8, 3, 0, -1),             # negative
           (U8, 8, 8, 3, 2 ** 31, 0)]
    for a in bad:
        assert L.rsr_image_span(*a) == R.RSR_E_ARG, a
    with pytest.raises(R.RealSRError) as e:
        R.image_span(F16, 8, 8, 3, 17)
    assert e.value.code == R.RSR_E_ARG


def test_null_context_is_an_argument_error():
    im = (R.Image * 1)()
    assert R.lib().rsr_process_device_batch(None, 1, im, F16, 8, 8, 3, im, F32, None) == R.RSR_E_ARG


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_describe_float_views(dtype):
    es = torch.zeros(1, dtype=dtype).element_size()
    big = torch.zeros(5, 3, 40, 64, dtype=dtype)
    p0 = big.data_ptr()
    # contiguous image and every image of a batch
    assert torch_io.describe(big[0]) == (p0, 64 * es, 40 * 64 * es)
    assert torch_io.describe(big[3]) == (p0 + 3 * 3 * 40 * 64 * es, 64 * es, 40 * 64 * es)
    assert torch_io.describe(big[1:4][2]) == torch_io.describe(big[3])
    # a crop at odd offsets: the pitches stay, the pointer moves
    crop = big[2, :, 7:30, 5:46]
    assert not crop.is_contiguous()
    assert torch_io.describe(crop) == (p0 + ((2 * 3 * 40 + 7) * 64 + 5) * es, 64 * es, 40 * 64 * es)
    # every second image of a batch, cropped: the batch stride is free
    v = big[::2, :, 1:, 1:]
    assert torch_io.describe(v[1]) == (p0 + ((2 * 3 * 40 + 1) * 64 + 1) * es, 64 * es, 40 * 64 * es)
    # planes stored apart / interleaved by rows ([h][3][w]) still have contiguous rows
    rows = torch.zeros(40, 3, 64, dtype=dtype)
    assert torch_io.describe(rows.permute(1, 0, 2)) == (rows.data_ptr(), 3 * 64 * es, 64 * es)
    # a single row or column has no stride to speak of
    assert torch_io.describe(big[0, :, 3:4, :]) == (p0 + 3 * 64 * es, 64 * es, 40 * 64 * es)
    assert torch_io.describe(big[0, :, :, 9:10])[1:] == (64 * es, 40 * 64 * es)
    # no descriptor: HWC seen as CHW, expand, steps, a transposed image, not an image
    hwc = torch.zeros(40, 64, 3, dtype=dtype)
    assert torch_io.describe(hwc.permute(2, 0, 1)) is None
    assert torch_io.describe(torch.zeros(1, 40, 64, dtype=dtype).expand(3, 40, 64)) is None
    assert torch_io.describe(torch.zeros(3, 1, 64, dtype=dtype).expand(3, 40, 64)) is None
    assert torch_io.describe(big[0, :, :, ::2]) is None
    assert torch_io.describe(big[0].transpose(1, 2)) is None
    assert torch_io.describe(big) is None
    assert torch_io.describe(big[0, :, ::2, :]) == (p0, 2 * 64 * es, 40 * 64 * es)  # (every second ROW is a pitch)


def test_describe_uint8_views():
    big = torch.zeros(50, 70, 4, dtype=torch.uint8)
    p0 = big.data_ptr()
    assert torch_io.describe(big) == (p0, 280, 0)
    crop = big[3:40, 5:66]
    assert torch_io.describe(crop) == (p0 + 3 * 280 + 20, 280, 0)
    rgb = torch.zeros(50, 70, 3, dtype=torch.uint8)
    assert torch_io.describe(rgb[1:, 1:]) == (rgb.data_ptr() + 213, 210, 0)  # a base aligned to nothing
    assert torch_io.describe(big[:, :, :3]) is None      # RGB of RGBA: pixel stride 4, c 3
    assert torch_io.describe(big[:, ::2]) is None
    assert torch_io.describe(torch.zeros(3, 50, 70, dtype=torch.uint8).permute(1, 2, 0)) is None
    assert torch_io.describe(torch.zeros(1, 70, 3, dtype=torch.uint8).expand(50, 70, 3)) is None


class _Ctx:
    """What torch_io.upscale reads of a context before it launches anything; any call into the engine would be a test failure."""
    gpuid, scale = 0, 4

    def process_device_fmt(self, *a, **k):
        raise AssertionError("launched despite bad arguments")

    process_device_batch = process_device_fmt


class _Cuda0(torch.Tensor):
    """A CPU tensor that claims to live on cuda:0: passes upscale's device check, so that the checks of `out` behind it are reached."""
    @property
    def device(self):
        return torch.device("cuda", 0)


def _on_cuda0(t):
    return t.as_subclass(_Cuda0)


@pytest.mark.parametrize("make_out", [
    lambda: torch.zeros(3, 32, 31, dtype=torch.float16),                       # shape
    lambda: torch.zeros(1, 3, 32, 32, dtype=torch.float16),                    # a batch dimension too many
    lambda: torch.zeros(3, 32, 32, dtype=torch.float32),                       # dtype
    lambda: torch.zeros(32, 32, 3, dtype=torch.float16).permute(2, 0, 1),      # layout: HWC seen as CHW
    lambda: torch.zeros(3, 32, 64, dtype=torch.float16)[:, :, ::2],            # layout: a step
    lambda: torch.zeros(1, 32, 32, dtype=torch.float16).expand(3, 32, 32),     # layout: expand
    lambda: "not a tensor",
], ids=["shape", "dims", "dtype", "permuted", "step", "expand", "type"])
def test_upscale_rejects_a_bad_out_before_launching(make_out):
    x = _on_cuda0(torch.zeros(3, 8, 8, dtype=torch.float16))
    out = make_out()
    out = _on_cuda0(out) if isinstance(out, torch.Tensor) else out
    with pytest.raises(ValueError, match="out"):
        torch_io.upscale(_Ctx(), x, out=out)


def test_upscale_rejects_out_on_another_device_and_bad_batched_outs():
    x = _on_cuda0(torch.zeros(2, 3, 8, 8, dtype=torch.float32))
    with pytest.raises(ValueError, match="out"):
        torch_io.upscale(_Ctx(), x, out=torch.zeros(2, 3, 32, 32, dtype=torch.float32))  # a CPU tensor
    with pytest.raises(ValueError, match="out"):
        torch_io.upscale(_Ctx(), x, out=_on_cuda0(torch.zeros(3, 32, 32, dtype=torch.float32)))
    with pytest.raises(ValueError, match="out"):
        torch_io.upscale(_Ctx(), x, out=_on_cuda0(torch.zeros(1, 3, 32, 32, dtype=torch.float32).expand(2, 3, 32, 32)))  # both images in one place
    u = _on_cuda0(torch.zeros(8, 8, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="out"):
        torch_io.upscale(_Ctx(), u, out=_on_cuda0(torch.zeros(32, 32, 3, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="out"):
        torch_io.upscale(_Ctx(), u, out=_on_cuda0(torch.zeros(32, 64, 4, dtype=torch.uint8)[:, ::2]))
