"""Rational output scales (rsr_set_out_ratio: x3, x3/2, x4/3, x9/4 ... area-averaged on the device): what can be said without a GPU --
rsr_out_size and the set of ratios, the binding's out_ratio / out_size, how torch_io sizes and checks `out`, the CLI's RSR_OUT_SCALE,
and the numpy reference the device tests compare against (tests/area_reduce.py).  The device side is tests/test_gpu_out_ratio.py."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

from area_reduce import BOX, GENERIC, RATIOS, area_reduce, exact_area_mean, taps
from box_reduce import box_reduce

F16 = R.RSR_FMT_F16_CHW


def out_size(n, d, T, w, h):
    ow, oh = C.c_int(-1), C.c_int(-1)
    rc = R.lib().rsr_out_size(n, d, T, w, h, C.byref(ow), C.byref(oh))
    return rc, ow.value, oh.value


# ---- rsr_out_size ------------------------------------------------------------------------------------------------------------------
def test_exactly_the_19_ratios_are_taken():
    assert len(RATIOS) == 19 and len(GENERIC) == 16
    assert sorted(Fraction(n, d) for n, d in RATIOS) == sorted(set(
        [Fraction(k) for k in (1, 2, 3, 4)] + [Fraction(k, 2) for k in (3, 5, 7)] + [Fraction(k, 3) for k in (4, 5, 7, 8, 10, 11)] +
        [Fraction(k, 4) for k in (5, 7, 9, 11, 13, 15)]))
    taken = set()
    for d in range(0, 7):
        for n in range(0, 30):
            rc, ow, oh = out_size(n, d, 120, 240, 360)  # (sizes every d up to 6 divides)
            if rc == R.RSR_OK:
                taken.add(Fraction(n, d))
                assert (ow, oh) == (240 * n // d, 360 * n // d)
            else:
                assert rc == R.RSR_E_ARG and (ow, oh) == (-1, -1)
    assert taken == {Fraction(n, d) for n, d in RATIOS}


def test_out_size_reduces_and_refuses():
    assert out_size(6, 4, 200, 1280, 720) == (R.RSR_OK, 1920, 1080)  # 6/4 is 3/2
    assert out_size(3, 2, 200, 1280, 720) == (R.RSR_OK, 1920, 1080)
    assert out_size(4, 3, 201, 1920, 1080) == (R.RSR_OK, 2560, 1440)
    assert out_size(9, 4, 200, 852 + 4, 480) == (R.RSR_OK, 1926, 1080)
    assert out_size(3, 1, 200, 1280, 720) == (R.RSR_OK, 3840, 2160)
    assert out_size(12, 4, 33, 7, 5) == (R.RSR_OK, 21, 15)  # 3/1: nothing to divide
    for n, d, T, w, h in [(0, 1, 200, 64, 64), (5, 1, 200, 64, 64), (3, 4, 200, 64, 64), (9, 5, 200, 60, 60), (3, 0, 200, 64, 64), (-3, -2, 200, 64, 64),
                          (3, 2, 32, 61, 47),     # an odd w (and h) at 3/2
                          (3, 2, 32, 62, 47), (3, 2, 32, 61, 46),
                          (3, 2, 33, 62, 46),     # tile 33 at 3/2: a tile's rectangle would start on half an output pixel
                          (4, 3, 200, 63, 48),    # tile 200 at 4/3
                          (9, 4, 198, 64, 64)]:
        rc, ow, oh = out_size(n, d, T, w, h)
        assert rc == R.RSR_E_ARG and (ow, oh) == (-1, -1), (n, d, T, w, h)
        assert R.lib().rsr_last_error(None)
    # either pointer may be NULL
    assert R.lib().rsr_out_size(3, 2, 32, 62, 46, None, None) == R.RSR_OK


def test_header_carries_the_definition():
    text = open(os.path.join(R.INCLUDE_DIR, "realsr_hip.h")).read()
    for needle in ("rsr_set_out_ratio", "rsr_out_size", "floor(X L / n)", "min((X + 1) L, (i + 1) n) - max(X L, i n)", "fp32(1 / (16 d^2))", '"out_num"', '"out_den"',
                   "Out of scope: a YUV OUTPUT"):
        assert needle in text, needle


# ---- the binding ---------------------------------------------------------------------------------------------------------------------
class _Engine:
    """Stands in for the C library behind a RealSR (tests/test_out_scale.py): holds the ratio as the engine does."""

    def __init__(self):
        self.n, self.d, self.calls = 4, 1, []

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
        return R.lib().rsr_out_size(*a)  # (host-only: the real one)

    def rsr_get_stat(self, h, key, ref):
        box = self.d == 1 and self.n in (1, 2, 4)
        ref._obj.value = {b"out_scale": self.n if box else 0, b"out_num": self.n, b"out_den": self.d}[key]
        return 0

    def rsr_set_params(self, *a):
        return 0

    def rsr_process(self, h, src, w, h_, c, dst):
        self.calls.append((w, h_, c))
        return 0

    def rsr_last_error(self, h):
        return b"bad argument"

    def rsr_destroy(self, h):
        pass


def test_out_ratio_property_and_out_size():
    assert isinstance(R.RealSR.out_ratio, property) and R.RealSR.out_ratio.fset is not None
    e = _Engine()
    sr = R.RealSR(0, _adopt=1)  # (adopts a handle: no device is opened)
    sr._L = e
    sr.tilesize = 32
    img = np.zeros((46, 62, 3), dtype=np.uint8)
    assert sr.out_ratio == 4 and isinstance(sr.out_ratio, Fraction) and sr.out_size(62, 46) == (248, 184)
    sr.out_ratio = Fraction(3, 2)
    assert (e.n, e.d) == (3, 2) and sr.out_ratio == Fraction(3, 2) and sr.out_scale == 0
    assert sr.out_size(62, 46) == (93, 69) and sr.process(img).shape == (69, 93, 3)
    sr.out_ratio = (6, 4)
    assert sr.out_ratio == Fraction(3, 2)
    sr.out_ratio = 3
    assert sr.out_ratio == 3 and sr.out_scale == 0 and sr.process(img).shape == (138, 186, 3)
    sr.out_ratio = (4, 3)
    with pytest.raises(ValueError):
        sr.out_size(62, 46)        # 62 * 4 is no multiple of 3
    with pytest.raises(ValueError):
        sr.process(img)
    sr.tilesize = 33
    assert sr.out_size(63, 48) == (84, 64)
    sr.tilesize = 32
    with pytest.raises(ValueError):
        sr.out_size(63, 48)        # tile 32 at 4/3
    for bad in (Fraction(3, 4), 5, (9, 5), (3, 0)):
        with pytest.raises(R.RealSRError) as err:
            sr.out_ratio = bad
        assert err.value.code == R.RSR_E_ARG and sr.out_ratio == Fraction(4, 3)
    sr.out_ratio = 2  # 2/1 IS out_scale 2
    assert sr.out_scale == 2 and sr.out_ratio == 2
    sr.out_ratio = Fraction(9, 4)
    sr.out_scale = 4  # ... and out_scale leaves a fractional ratio again
    assert sr.out_ratio == 4 and sr.process(img).shape == (184, 248, 3)
    assert len(e.calls) == 3
    sr._h = None


class _Stream:
    cuda_stream = 5


class _Ctx:
    """A context that records what torch_io hands the engine (tests/test_out_scale.py), at ratio 3/2 and tile 32."""
    gpuid, scale, out_scale, tilesize = 0, 4, 0, 32
    out_ratio = Fraction(3, 2)

    def __init__(self):
        self.calls = []

    def out_size(self, w, h):
        rc, ow, oh = out_size(3, 2, self.tilesize, w, h)
        if rc:
            raise ValueError("no such size")
        return ow, oh

    def process_device_fmt(self, *a, **k):
        self.calls.append(("fmt", a, k))

    def process_device_batch(self, *a, **k):
        self.calls.append(("batch", a, k))


class _Cuda0(torch.Tensor):
    @property
    def device(self):
        return torch.device("cuda", 0)


def _on_cuda0(t):
    return t.as_subclass(_Cuda0)


def test_upscale_sizes_and_checks_out_with_the_ratio(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _Stream())
    s = _Ctx()
    x = _on_cuda0(torch.zeros(3, 8, 12, dtype=torch.float16))
    out = _on_cuda0(torch.zeros(3, 12, 18, dtype=torch.float16))
    assert torch_io.upscale(s, x, out=out) is out
    (kind, a, k), = s.calls
    assert kind == "fmt" and a == (x.data_ptr(), F16, 12, 8, 3, out.data_ptr(), F16) and k == {"stream": 5}
    for shape in ((3, 32, 48), (3, 16, 24), (3, 12, 17)):
        with pytest.raises(ValueError, match="out"):
            torch_io.upscale(s, x, out=_on_cuda0(torch.zeros(shape, dtype=torch.float16)))
    with pytest.raises(ValueError):
        torch_io.upscale(s, _on_cuda0(torch.zeros(3, 8, 11, dtype=torch.float16)))  # an odd width at 3/2
    # a batch into a x3/2 window of a canvas: the window's pointers and pitches
    xb = _on_cuda0(torch.zeros(2, 3, 8, 12, dtype=torch.float32))
    canvas = torch.zeros(2, 3, 40, 64, dtype=torch.float32)
    torch_io.upscale(s, xb, out=_on_cuda0(canvas[..., 6:18, 10:28]))
    kind, a, k = s.calls[-1]
    p0 = canvas.data_ptr() + (6 * 64 + 10) * 4
    assert kind == "batch" and a[5] == [(p0, 256, 40 * 256), (p0 + 3 * 40 * 256, 256, 40 * 256)]
    assert len(s.calls) == 2
    # a YUV output has no fractional ratio
    surf = _on_cuda0(torch.zeros(12, 12, dtype=torch.uint8))
    with pytest.raises(ValueError, match="YUV"):
        torch_io.upscale_yuv(s, surf)
    assert len(s.calls) == 2


def test_cli_takes_ratios_and_still_refuses_the_rest(tmp_path):
    """RSR_OUT_SCALE is checked with the flags, before an image is read or a GPU touched: n/d of the set passes that check (the run then
    ends at the missing input), everything else is refused there -- a lone 3 included, as ever: x3 is written 3/1."""
    cli = os.path.join(os.path.dirname(R.LIB_PATH), "..", "bin", "realsr-hip")

    def run(v):
        return subprocess.run([cli, "-i", str(tmp_path / "missing.png"), "-o", str(tmp_path / "o.png")], capture_output=True, text=True,
                              env=dict(os.environ, RSR_OUT_SCALE=v), timeout=60)
    for bad in ("3", "5/1", "3/4", "9/5", "3/0", "3/2x", "/2", "3/", "1.5", "3/2/1", "-3/-2"):
        r = run(bad)
        assert r.returncode != 0 and "invalid RSR_OUT_SCALE" in r.stderr, (bad, r.stderr)
    for good in ("3/2", "6/4", "4/3", "9/4", "3/1", "15/4", "2/1", "4"):
        r = run(good)
        assert r.returncode != 0 and "invalid RSR_OUT_SCALE" not in r.stderr, (good, r.stderr)


# ---- the numpy reference -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", RATIOS, ids=["%d/%d" % r for r in RATIOS])
def test_weights_sum_to_4d_and_taps_are_few(nd):
    n, d = nd
    for X in range(0, 3 * n + 5):
        t = taps(X, n, d)
        assert sum(g for _, g in t) == 4 * d and all(1 <= g <= n for _, g in t) and len(t) <= 4
        assert [i for i, _ in t] == list(range(t[0][0], t[-1][0] + 1))
    # n output pixels cover exactly 4 d x4 pixels: the pattern repeats from there, so a tile that starts on such a multiple starts afresh
    assert taps(n, n, d)[0] == (4 * d, taps(0, n, d)[0][1])


@pytest.mark.parametrize("nd", RATIOS, ids=["%d/%d" % r for r in RATIOS])
def test_a_constant_image_stays_that_constant_bit_for_bit(nd):
    """For a constant c with the 11 significant bits of an fp16 value every partial sum is k * c with an integer k <= 16 d^2 <= 256: at most
    19 bits, exact in float32.  The last product is exact for d = 1, 2, 4 (a power of two); for d = 3, fp32(1 / 144) = (1 / 144)(1 + 2^-27),
    and c (1 + 2^-27) rounds back to c.  Every fifth fp16 value of [0, 1] and both ends, one 48 x 48 plane each."""
    n, d = nd
    c = np.arange(0, 0x3C01, 5, dtype=np.uint16).view(np.float16).astype(np.float32)
    assert c[0] == 0 and c[-1] == 1
    v = np.ascontiguousarray(np.broadcast_to(c[:, None, None], (c.size, 48, 48)))
    got = area_reduce(v, n, d)
    assert got.shape == (c.size, 12 * n // d, 12 * n // d)
    assert (got.view(np.uint32) == c.view(np.uint32)[:, None, None]).all()


def test_2_over_1_is_box_reduce_bit_for_bit():
    v = np.random.default_rng(11).uniform(-0.2, 1.2, size=(3, 48, 64)).astype(np.float32)
    assert np.array_equal(area_reduce(v, 2, 1).view(np.uint32), box_reduce(v, 2).view(np.uint32))
    assert np.array_equal(area_reduce(v, 4, 1).view(np.uint32), box_reduce(v, 1).view(np.uint32))
    h = np.random.default_rng(12).random((3, 48, 64), dtype=np.float32).astype(np.float16).astype(np.float32)
    assert np.array_equal(area_reduce(h, 2, 1).view(np.uint32), box_reduce(h, 2).view(np.uint32))


@pytest.mark.parametrize("nd", RATIOS, ids=["%d/%d" % r for r in RATIOS])
def test_reference_is_the_exact_area_mean_to_float32_rounding(nd):
    """The bound, from the term count: an output pixel is a sum of at most 4 x 4 = 16 non-negative terms.  A term goes through at most
    1 product with its horizontal weight, 3 additions of the row sum, 1 product with the vertical weight, 3 additions of the column sum
    and the final product, whose constant fp32(1 / (16 d^2)) carries one more rounding: 10 roundings of relative size u = 2^-24 each.
    All terms have one sign, so the relative error of the result is at most gamma_10 = 10 u / (1 - 10 u), and the result is at most 1."""
    n, d = nd
    u = 2.0 ** -24
    bound = 10 * u / (1 - 10 * u)
    v = np.random.default_rng(13).uniform(-0.2, 1.2, size=(3, 48, 96)).astype(np.float32)
    got, want = area_reduce(v, n, d), exact_area_mean(v, n, d)
    assert got.shape == want.shape and got.min() >= 0 and got.max() <= 1
    err = np.abs(got.astype(np.float64) - np.minimum(want, 1.0))
    print("%d/%d: max |reference - exact area mean| = %.3e (bound %.3e)" % (n, d, err.max(), bound))
    assert err.max() <= bound
    # and `want` IS the area mean: every x4 pixel repeated n times per axis, then plain L x L block means (no taps, no weights)
    L = 4 * d
    rep = np.repeat(np.repeat(np.clip(v.astype(np.float64), 0, 1), n, axis=-1), n, axis=-2)
    blocks = rep.reshape(3, rep.shape[1] // L, L, rep.shape[2] // L, L).mean(axis=(2, 4))
    assert np.abs(blocks - want).max() <= 1e-14


def test_order_is_horizontal_first_and_ascending():
    """3/1 (weights 3, 1 | 2, 2 | 1, 3 over L = 4): a footprint whose float32 sum depends on the order."""
    e = np.float32(2.0 ** -24)
    v = np.zeros((4, 4), dtype=np.float32)
    v[0, 0], v[0, 1] = 1.0 / 3.0, e          # output (0, 0): taps x 0, 1 with weights 3, 1; rows 0, 1 with weights 3, 1
    H = np.float32(3) * np.float32(1.0 / 3.0) + np.float32(1) * e
    want = np.float32(np.float32(3) * H) * np.float32(1 / 16.0)
    assert area_reduce(v, 3, 1)[0, 0] == want
    assert area_reduce(v, 3, 1).shape == (3, 3)
