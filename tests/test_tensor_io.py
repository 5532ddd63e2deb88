"""Planar fp16 / fp32 device images (rsr_process_device_fmt, rsr_image_bytes) and the torch entry point (torch_io.upscale): what can be
said without a GPU -- buffer sizes, the C ABI, argument checking.  The device side is tests/test_gpu_tensor_io.py."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import realsr_ncnn_vulkan_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rsr_process_device_fmt", "rsr_image_bytes")
U8, F16, F32 = R.RSR_FMT_U8_HWC, R.RSR_FMT_F16_CHW, R.RSR_FMT_F32_CHW


def test_format_constants_match_the_header():
    text = open(os.path.join(R.INCLUDE_DIR, "realsr_hip.h")).read()
    for name, val in (("RSR_FMT_U8_HWC", 0), ("RSR_FMT_F16_CHW", 1), ("RSR_FMT_F32_CHW", 2)):
        assert "#define %s %d" % (name, val) in text and getattr(R, name) == val
    assert set(NEW_SYMBOLS) <= set(R.EXPORTS)
    for s in NEW_SYMBOLS:
        assert hasattr(R.lib(), s), s


def test_image_bytes():
    L = R.lib()
    for w, h in ((1, 1), (61, 47), (1920, 1080), (7680, 4320)):
        assert L.rsr_image_bytes(U8, w, h, 3) == 3 * w * h
        assert L.rsr_image_bytes(U8, w, h, 4) == 4 * w * h
        assert L.rsr_image_bytes(F16, w, h, 3) == 6 * w * h
        assert L.rsr_image_bytes(F32, w, h, 3) == 12 * w * h
        assert R.image_bytes(F32, w, h) == 12 * w * h
    # beyond 2 GiB: the result is a long long (an 8K frame at 4x as fp32)
    assert L.rsr_image_bytes(F32, 4 * 7680, 4 * 4320, 3) == 12 * 16 * 7680 * 4320 > 2 ** 32
    bad = [(F16, 8, 8, 4), (F32, 8, 8, 4), (F16, 8, 8, 1), (U8, 8, 8, 1), (U8, 8, 8, 5), (7, 8, 8, 3), (-1, 8, 8, 3), (3, 8, 8, 3),
           (U8, 0, 8, 3), (U8, 8, 0, 3), (F16, -1, 8, 3), (F32, 8, -5, 3)]
    for fmt, w, h, c in bad:
        assert L.rsr_image_bytes(fmt, w, h, c) == R.RSR_E_ARG, (fmt, w, h, c)
    with pytest.raises(R.RealSRError) as e:
        R.image_bytes(F16, 8, 8, 4)
    assert e.value.code == R.RSR_E_ARG


def test_null_context_is_an_argument_error():
    assert R.lib().rsr_process_device_fmt(None, None, F16, 8, 8, 3, None, F32, None) == R.RSR_E_ARG


def test_header_with_the_format_api_is_plain_c_and_a_c_host_reaches_it(tmp_path):
    """include/realsr_hip.h still compiles as C99 -pedantic; a host written in C links against the two new symbols and gets the sizes and
    the argument errors without a GPU."""
    src = tmp_path / "host.c"
    src.write_text(r'''
#include <stdio.h>
#include "realsr_hip.h"
int main(void)
{
    long long a = rsr_image_bytes(RSR_FMT_U8_HWC, 10, 7, 3), b = rsr_image_bytes(RSR_FMT_U8_HWC, 10, 7, 4);
    long long c = rsr_image_bytes(RSR_FMT_F16_CHW, 10, 7, 3), d = rsr_image_bytes(RSR_FMT_F32_CHW, 10, 7, 3);
    long long e = rsr_image_bytes(RSR_FMT_F16_CHW, 10, 7, 4), f = rsr_image_bytes(7, 10, 7, 3), g = rsr_image_bytes(RSR_FMT_F32_CHW, 0, 7, 3);
    int rc = rsr_process_device_fmt(NULL, NULL, RSR_FMT_F16_CHW, 10, 7, 3, NULL, RSR_FMT_F32_CHW, NULL);
    printf("bytes %lld %lld %lld %lld bad %lld %lld %lld null %d\n", a, b, c, d, e, f, g, rc);
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
    assert "bytes 210 280 420 840 bad -1 -1 -1 null -1" in r.stdout, r.stdout
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(lib, "librealsr_hip.so")], text=True)
    for s in NEW_SYMBOLS:
        assert " T %s\n" % s in out, s


class _Ctx:
    """What torch_io.upscale reads of a context before it launches anything; any call into the engine would be a test failure."""
    gpuid, scale = 0, 4

    def process_device_fmt(self, *a, **k):
        raise AssertionError("launched despite bad arguments")


@pytest.mark.parametrize("x", [
    torch.zeros(3, 8, 8, dtype=torch.float16),           # right shape and dtype, wrong device (CPU)
    torch.zeros(2, 3, 8, 8, dtype=torch.float32),        # likewise, batched
    torch.zeros(8, 8, 3, dtype=torch.uint8),             # likewise, uint8 HWC
    torch.zeros(3, 8, 8, dtype=torch.float64),           # dtype
    torch.zeros(3, 8, 8, dtype=torch.bfloat16),
    torch.zeros(3, 8, 8, dtype=torch.int32),
    torch.zeros(4, 8, 8, dtype=torch.float16),           # planar RGBA is out of scope
    torch.zeros(8, 8, 3, dtype=torch.float16),           # HWC floats
    torch.zeros(8, 8, dtype=torch.float32),
    torch.zeros(1, 2, 3, 8, 8, dtype=torch.float32),
    torch.zeros(3, 8, 8, dtype=torch.uint8),             # CHW bytes
    torch.zeros(2, 8, 8, 3, dtype=torch.uint8),          # batched bytes
    torch.zeros(3, 0, 8, dtype=torch.float16),           # empty
], ids=lambda x: "%s-%s" % (str(x.dtype).split(".")[-1], "x".join(map(str, x.shape))))
def test_upscale_rejects_bad_tensors_before_launching(x):
    from realsr_ncnn_vulkan_amd import torch_io
    with pytest.raises(ValueError):
        torch_io.upscale(_Ctx(), x)


def test_upscale_rejects_what_is_not_a_tensor():
    import numpy as np
    from realsr_ncnn_vulkan_amd import torch_io
    with pytest.raises(ValueError):
        torch_io.upscale(_Ctx(), np.zeros((3, 8, 8), dtype=np.float16))


def test_upscale_names_the_device_it_expects():
    """A tensor that is not on the context's GPU (here: a meta tensor) is refused with both devices in the message."""
    from realsr_ncnn_vulkan_amd import torch_io
    x = torch.zeros(2, 3, 8, 8, dtype=torch.float16, device="meta")
    with pytest.raises(ValueError, match="cuda:0"):
        torch_io.upscale(_Ctx(), x)
