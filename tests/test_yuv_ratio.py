"""NV12 / P010 OUTPUT at a rational output ratio (include/realsr_hip.h, "YUV output at a ratio"): what can be said without a GPU --
rsr_out_size_yuv against a restatement of the admission rule, the binding's out_size_yuv, how torch_io sizes and checks a YUV `out`
while a ratio other than 4 / 2 / 1 is in force, and the header's text.  The device side is tests/test_gpu_yuv_ratio.py."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

from area_reduce import RATIOS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NV12, P010 = R.RSR_FMT_NV12, R.RSR_FMT_P010


def out_size_yuv(n, d, T, w, h):
    ow, oh = C.c_int(-1), C.c_int(-1)
    rc = R.lib().rsr_out_size_yuv(n, d, T, w, h, C.byref(ow), C.byref(oh))
    return rc, ow.value, oh.value


def admitted(n, d, T, w, h):
    """The rule, restated: n / d in lowest terms; w and h even; w n, h n and T n divisible by d; w n / d, h n / d and T n / d even."""
    if w % 2 or h % 2:
        return False
    if any(v * n % d for v in (w, h, T)):
        return False
    return not any((v * n // d) % 2 for v in (w, h, T))


# ---- rsr_out_size_yuv -----------------------------------------------------------------------------------------------------------------
def test_out_size_yuv_is_the_rule_over_every_ratio():
    assert len(RATIOS) == 19
    L = R.lib()
    ow, oh = C.c_int(), C.c_int()
    yes = no = 0
    for n, d in RATIOS:
        for T in range(24, 41):
            for w in range(2, 25):
                for h in range(2, 25):
                    ow.value = oh.value = -1
                    rc = L.rsr_out_size_yuv(n, d, T, w, h, C.byref(ow), C.byref(oh))
                    if admitted(n, d, T, w, h):
                        assert rc == R.RSR_OK and (ow.value, oh.value) == (w * n // d, h * n // d), (n, d, T, w, h)
                        yes += 1
                    else:
                        assert rc == R.RSR_E_ARG and (ow.value, oh.value) == (-1, -1), (n, d, T, w, h)
                        no += 1
    assert yes > 1000 and no > 1000, (yes, no)


def test_the_video_cases():
    assert out_size_yuv(3, 2, 200, 1280, 720) == (R.RSR_OK, 1920, 1080)
    assert out_size_yuv(6, 4, 200, 1280, 720) == (R.RSR_OK, 1920, 1080)  # 6/4 is 3/2
    assert out_size_yuv(4, 3, 198, 1920, 1080) == (R.RSR_OK, 2560, 1440)
    assert out_size_yuv(4, 3, 201, 1920, 1080) == (R.RSR_OK, 2560, 1440)
    assert out_size_yuv(9, 4, 200, 720, 480) == (R.RSR_OK, 1620, 1080)
    assert out_size_yuv(3, 1, 200, 1280, 720) == (R.RSR_OK, 3840, 2160)
    assert out_size_yuv(3, 1, 200, 50, 38) == (R.RSR_OK, 150, 114)
    for n, d, T, w, h in [(4, 3, 200, 1920, 1080),   # tile 200 at 4/3: not a whole rectangle, as for every format
                          (3, 2, 30, 1280, 720),     # tile 30 at 3/2: a rectangle of 45, odd
                          (3, 2, 33, 1280, 720),     # tile 33 at 3/2
                          (3, 2, 32, 62, 46),        # 93 x 69
                          (3, 2, 32, 70, 50),        # 105 x 75
                          (3, 2, 32, 64, 46),        # an odd height only
                          (3, 2, 32, 61, 44), (3, 2, 32, 60, 43),   # an odd w / h of the surface itself
                          (3, 1, 200, 51, 38), (4, 1, 200, 64, 63),
                          (1, 1, 33, 64, 64),        # out_scale 1 at an odd tile: what the engine refuses today
                          (5, 1, 200, 64, 64), (3, 0, 200, 64, 64), (3, 4, 200, 64, 64),
                          (3, 2, 200, 0, 64), (3, 2, 0, 64, 64)]:
        rc, ow, oh = out_size_yuv(n, d, T, w, h)
        assert rc == R.RSR_E_ARG and (ow, oh) == (-1, -1), (n, d, T, w, h)
        assert R.lib().rsr_last_error(None)
    # what check_yuv_out enforces at 4 / 2 / 1: only out_scale 1 asks anything of the tile
    assert out_size_yuv(4, 1, 33, 64, 48) == (R.RSR_OK, 256, 192)
    assert out_size_yuv(2, 1, 33, 64, 48) == (R.RSR_OK, 128, 96)
    assert out_size_yuv(1, 1, 32, 64, 48) == (R.RSR_OK, 64, 48)
    # the refusal names the format
    assert out_size_yuv(3, 2, 30, 60, 44)[0] == R.RSR_E_ARG and b"YUV" in R.lib().rsr_last_error(None)
    assert out_size_yuv(3, 2, 33, 60, 44)[0] == R.RSR_E_ARG and b"YUV" in R.lib().rsr_last_error(None)


def test_null_output_pointers_are_accepted():
    L = R.lib()
    assert L.rsr_out_size_yuv(3, 2, 32, 60, 44, None, None) == R.RSR_OK
    ow = C.c_int(-1)
    assert L.rsr_out_size_yuv(3, 2, 32, 60, 44, C.byref(ow), None) == R.RSR_OK and ow.value == 90
    oh = C.c_int(-1)
    assert L.rsr_out_size_yuv(3, 2, 32, 60, 44, None, C.byref(oh)) == R.RSR_OK and oh.value == 66
    assert L.rsr_out_size_yuv(3, 2, 30, 60, 44, None, None) == R.RSR_E_ARG


def test_symbol_is_exported_and_a_c_host_links_it(tmp_path):
    assert "rsr_out_size_yuv" in R.EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", R.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T rsr_out_size_yuv\n" in out
    src = tmp_path / "host.c"
    src.write_text(r'''
#include <stdio.h>
#include "realsr_hip.h"
int main(void)
{
    int ow = -1, oh = -1, a, b, c;
    a = rsr_out_size_yuv(3, 2, 200, 1280, 720, &ow, &oh);
    b = rsr_out_size_yuv(3, 2, 30, 1280, 720, NULL, NULL);
    c = rsr_out_size_yuv(3, 2, 200, 1281, 720, NULL, NULL);
    printf("rc %d %d x %d odd tile %d odd w %d\n", a, ow, oh, b, c);
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
    assert "rc 0 1920 x 1080 odd tile -1 odd w -1" in r.stdout, r.stdout


def test_header_carries_the_new_sentences():
    text = open(os.path.join(R.INCLUDE_DIR, "realsr_hip.h")).read()
    for needle in ("int rsr_out_size_yuv(int num, int den, int tilesize, int w, int h, int* ow, int* oh);",
                   "Out of scope: a YUV OUTPUT (RSR_FMT_NV12 / RSR_FMT_P010) whose w * n / d, h * n / d or tilesize * n / d is odd: RSR_E_ARG",
                   "YUV output at a ratio.", "w * n / d, h * n / d and tilesize * n / d EVEN",
                   "no 2 x 2 chroma quad crosses a tile or the image's edge",
                   "starts at multiples of tilesize * n / d output pixels", "postproc_tiles_yuv_area",
                   '"YUV" in rsr_last_error',
                   # the YUV section and the ratio section keep theirs
                   "A tile's rectangle starts\n *            at multiples of tilesize * out_scale output pixels (even: see Errors).",
                   "The input side is independent: a YUV input works at\n *            any ratio."):
        assert needle in text, needle


# ---- the binding ---------------------------------------------------------------------------------------------------------------------
class _Engine:
    """Stands in for the C library behind a RealSR (tests/test_out_ratio.py): holds the ratio as the engine does; the host-only size
    functions are the real ones."""

    def __init__(self):
        self.n, self.d = 4, 1

    def rsr_set_option(self, h, key, value):
        if key == b"out_scale":
            if value not in (1, 2, 4):
                return R.RSR_E_ARG
            self.n, self.d = value, 1
        return 0

    def rsr_set_out_ratio(self, h, n, d):
        f = Fraction(n, d) if d > 0 else None
        if f is None or (f.numerator, f.denominator) not in RATIOS:
            return R.RSR_E_ARG
        self.n, self.d = f.numerator, f.denominator
        return 0

    def rsr_out_size(self, *a):
        return R.lib().rsr_out_size(*a)

    def rsr_out_size_yuv(self, *a):
        return R.lib().rsr_out_size_yuv(*a)

    def rsr_get_stat(self, h, key, ref):
        box = self.d == 1 and self.n in (1, 2, 4)
        ref._obj.value = {b"out_scale": self.n if box else 0, b"out_num": self.n, b"out_den": self.d}[key]
        return 0

    def rsr_last_error(self, h):
        return b"bad argument"

    def rsr_destroy(self, h):
        pass


def test_realsr_out_size_yuv_without_a_gpu():
    sr = R.RealSR(0, _adopt=1)  # (adopts a handle: no device is opened)
    sr._L = _Engine()
    sr.tilesize = 200
    assert sr.out_size_yuv(1280, 720) == (5120, 2880)
    sr.out_ratio = Fraction(3, 2)
    assert sr.out_size_yuv(1280, 720) == (1920, 1080)
    sr.out_ratio = Fraction(9, 4)
    assert sr.out_size_yuv(720, 480) == (1620, 1080)
    sr.out_ratio = (4, 3)
    with pytest.raises(ValueError, match="YUV"):
        sr.out_size_yuv(1920, 1080)  # tile 200 at 4/3
    sr.tilesize = 201
    assert sr.out_size_yuv(1920, 1080) == (2560, 1440)
    sr.out_ratio = Fraction(3, 2)
    sr.tilesize = 32
    assert sr.out_size(62, 46) == (93, 69)  # an RGB output takes it ...
    for w, h in ((62, 46), (70, 50), (61, 44)):
        with pytest.raises(ValueError, match="YUV"):
            sr.out_size_yuv(w, h)  # ... a surface does not
    assert sr.out_size_yuv(60, 44) == (90, 66)
    sr.tilesize = 30
    with pytest.raises(ValueError, match="YUV"):
        sr.out_size_yuv(60, 44)
    sr.out_ratio = 1
    sr.tilesize = 33
    with pytest.raises(ValueError, match="YUV"):
        sr.out_size_yuv(64, 48)  # out_scale 1 at an odd tile
    sr.out_ratio = 2
    assert sr.out_size_yuv(64, 48) == (128, 96)
    sr._h = None


# ---- torch_io against a recording context -------------------------------------------------------------------------------------------------
class _Stream:
    cuda_stream = 5


class _Ctx:
    """A context that records what torch_io hands the engine, at ratio 3/2 and tile 32, WITH out_size_yuv."""
    gpuid, scale, out_scale, tilesize = 0, 4, 0, 32
    out_ratio = Fraction(3, 2)

    def __init__(self):
        self.calls = []

    def out_size_yuv(self, w, h):
        rc, ow, oh = out_size_yuv(3, 2, self.tilesize, w, h)
        if rc:
            raise ValueError("a YUV output at 3/2 does not take %d x %d" % (w, h))
        return ow, oh

    def process_device_batch(self, *a, **k):
        self.calls.append(("batch", a, k))


class _Cuda0(torch.Tensor):
    @property
    def device(self):
        return torch.device("cuda", 0)


def _on_cuda0(t):
    return t.as_subclass(_Cuda0)


@pytest.mark.parametrize("dtype, fmt", [(torch.uint8, NV12), (torch.int16, P010)], ids=["nv12", "p010"])
def test_upscale_yuv_sizes_and_checks_out_with_the_ratio(monkeypatch, dtype, fmt):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _Stream())
    s = _Ctx()
    es = 1 if dtype == torch.uint8 else 2
    surf = _on_cuda0(torch.zeros(66, 60, dtype=dtype))  # 60 x 44
    y = torch_io.upscale_yuv(s, surf)
    assert tuple(y.shape) == (99, 90) and y.dtype == dtype  # (3 oh / 2, ow) at 90 x 66
    (kind, a, k), = s.calls
    assert kind == "batch" and k == {"stream": 5}
    assert a == ([(surf.data_ptr(), 60 * es, 44 * 60 * es)], fmt, 60, 44, 3, [(y.data_ptr(), 90 * es, 66 * 90 * es)], fmt)
    # out=: the surface of the reduced size, or a window of a canvas with that size
    out = _on_cuda0(torch.zeros(99, 90, dtype=dtype))
    assert torch_io.upscale_yuv(s, surf, out=out) is out
    assert s.calls[-1][1][5] == [(out.data_ptr(), 90 * es, 66 * 90 * es)]
    canvas = torch.zeros(120, 128, dtype=dtype)
    pair = (_on_cuda0(canvas[4:70, 8:98]), _on_cuda0(canvas[80:113, 8:98]))
    got = torch_io.upscale_yuv(s, (surf[:44], surf[44:]), out=pair)
    assert got is pair
    p0 = canvas.data_ptr() + (4 * 128 + 8) * es
    assert s.calls[-1][1][5] == [(p0, 128 * es, 76 * 128 * es)]
    n = len(s.calls)
    for shape in ((264, 240), (132, 120), (66, 60), (99, 88), (96, 90)):  # the x4, x2 and x1 sizes; a narrower and a shorter surface
        with pytest.raises(ValueError, match="YUV"):
            torch_io.upscale_yuv(s, surf, out=_on_cuda0(torch.zeros(shape, dtype=dtype)))
    # sizes the rule refuses: nothing is called
    with pytest.raises(ValueError, match="YUV"):
        torch_io.upscale_yuv(s, _on_cuda0(torch.zeros(69, 62, dtype=dtype)))  # 62 x 46 -> 93 x 69
    s.tilesize = 30
    with pytest.raises(ValueError, match="YUV"):
        torch_io.upscale_yuv(s, surf)
    assert len(s.calls) == n


def test_upscale_delta_and_sequence_size_their_surfaces_with_the_ratio(monkeypatch):
    """prev_y / out of the x4 size are refused with "YUV" in the text before anything is called (the checks come in front of the diff)."""
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _Stream())
    s = _Ctx()
    surf = _on_cuda0(torch.zeros(66, 60, dtype=torch.uint8))
    for shape in ((264, 240), (66, 60)):
        wrong = _on_cuda0(torch.zeros(shape, dtype=torch.uint8))
        with pytest.raises(ValueError, match="YUV"):
            torch_io.upscale_delta(s, surf, surf, wrong)
        with pytest.raises(ValueError, match="YUV"):
            torch_io.upscale_sequence(s, [surf], prev_x=surf, prev_y=wrong)
        with pytest.raises(ValueError, match="YUV"):
            torch_io.upscale_sequence(s, [surf], out=[wrong])
    with pytest.raises(ValueError, match="YUV"):
        torch_io.upscale_delta(s, _on_cuda0(torch.zeros(69, 62, dtype=torch.uint8)), None, surf)  # 93 x 69
    assert not s.calls


def test_a_context_without_out_size_yuv_keeps_the_refusal(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _Stream())

    class Old:
        gpuid, scale, out_scale, tilesize = 0, 4, 0, 32
        out_ratio = Fraction(3, 2)
        calls = []

        def process_device_batch(self, *a, **k):
            self.calls.append(a)

    s = Old()
    surf = _on_cuda0(torch.zeros(66, 60, dtype=torch.uint8))
    with pytest.raises(ValueError, match="YUV"):
        torch_io.upscale_yuv(s, surf)
    with pytest.raises(ValueError, match="YUV"):
        torch_io.upscale_delta(s, surf, None, surf)
    with pytest.raises(ValueError, match="YUV"):
        torch_io.upscale_sequence(s, [surf])
    assert not s.calls
    # ... and at out_scale 4 / 2 / 1 nothing asks for out_size_yuv
    s.out_scale = 2
    y = torch_io.upscale_yuv(s, surf)
    assert tuple(y.shape) == (132, 120) and len(s.calls) == 1
