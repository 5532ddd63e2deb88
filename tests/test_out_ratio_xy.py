"""A ratio per axis (rsr_set_out_ratio_xy: DVD and HDV frames to square-pixel sizes, e.g. 720 x 480 -> 1920 x 1080 at 8/3 x 9/4): what can
be said without a GPU -- rsr_out_size_xy / rsr_out_size_yuv_xy and the set of pairs, the binding's out_ratio_xy / out_ratio / out_size,
how torch_io sizes `out`, the CLI's RSR_OUT_SCALE=x,y, and the numpy reference the device tests compare against
(tests/area_reduce_xy.py).  The device side is tests/test_gpu_out_ratio_xy.py."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

import yuv_siting_ref
from area_reduce import RATIOS, area_reduce
from area_reduce_xy import AXIS_RATIOS, admitted, area_reduce_xy, encode_xy, exact_area_mean_xy, out_size_xy, taps

F16 = R.RSR_FMT_F16_CHW
NEW = ("rsr_set_out_ratio_xy", "rsr_out_size_xy", "rsr_out_size_yuv_xy")


def c_out_size(fn, nx, dx, ny, dy, T, w, h):
    ow, oh = C.c_int(-1), C.c_int(-1)
    rc = getattr(R.lib(), fn)(nx, dx, ny, dy, T, w, h, C.byref(ow), C.byref(oh))
    return rc, ow.value, oh.value


# ---- the header and the exports ------------------------------------------------------------------------------------------------------
def test_header_carries_the_names_and_the_per_axis_definition():
    text = open(os.path.join(R.INCLUDE_DIR, "realsr_hip.h")).read()
    for needle in NEW + ("fp32(1 / (16 dx dy))", "(nx, Lx = 4 dx)", "(ny, Ly = 4 dy)", '"out_num_x"', '"out_den_x"', '"out_num_y"', '"out_den_y"',
                         "720 x 480", "512 x 432", "512 x 360", "264 x 198", "15/8"):
        assert needle in text, needle


def test_the_three_symbols_are_exported():
    L = R.lib()
    for name in NEW:
        assert name in R.EXPORTS and hasattr(L, name), name


# ---- rsr_out_size_xy -----------------------------------------------------------------------------------------------------------------
def test_exactly_the_67_ratios_per_axis_are_taken():
    assert len(AXIS_RATIOS) == 67 and set(RATIOS) <= set(AXIS_RATIOS)
    taken = set()
    for d in range(0, 11):
        for n in range(0, 45):
            want = admitted(n, d)
            rc, ow, oh = c_out_size("rsr_out_size_xy", n, d, 4, 1, 840, 840, 1680)  # (840: every d up to 8 divides it)
            rc2, ow2, oh2 = c_out_size("rsr_out_size_xy", 1, 1, n, d, 840, 840, 1680)
            if want:
                taken.add(want)
                assert (rc, ow, oh) == (R.RSR_OK, 840 * n // d, 6720) and (rc2, ow2, oh2) == (R.RSR_OK, 840, 1680 * n // d), (n, d)
            else:
                assert (rc, ow, oh) == (R.RSR_E_ARG, -1, -1) and (rc2, ow2, oh2) == (R.RSR_E_ARG, -1, -1), (n, d)
    assert taken == set(AXIS_RATIOS)


def test_all_pairs_follow_the_python_formula():
    """67 x 67 pairs at a tile and an image size that only some of them take."""
    T, w, h = 48, 60, 64
    taken = 0
    for rx in AXIS_RATIOS:
        for ry in AXIS_RATIOS:
            want = out_size_xy(rx, ry, T, w, h)
            got = c_out_size("rsr_out_size_xy", 2 * rx[0], 2 * rx[1], 3 * ry[0], 3 * ry[1], T, w, h)  # (unreduced: the library reduces)
            assert got == ((R.RSR_OK,) + want if want else (R.RSR_E_ARG, -1, -1)), (rx, ry)
            wanty = out_size_xy(rx, ry, T, w, h, yuv=True)
            goty = c_out_size("rsr_out_size_yuv_xy", rx[0], rx[1], ry[0], ry[1], T, w, h)
            assert goty == ((R.RSR_OK,) + wanty if wanty else (R.RSR_E_ARG, -1, -1)), (rx, ry)
            taken += want is not None
    assert 0 < taken < 67 * 67
    assert out_size_xy((8, 3), (15, 8), T, w, h) == (160, 120)


def test_out_size_xy_refusals():
    ok = (8, 3, 9, 4, 24, 60, 44)
    assert c_out_size("rsr_out_size_xy", *ok) == (R.RSR_OK, 160, 99)
    for args in [(8, 3, 9, 4, 24, 61, 44),    # w * 8 is no multiple of 3
                 (8, 3, 9, 4, 24, 60, 45),    # h * 9 is no multiple of 4
                 (8, 3, 9, 4, 25, 60, 44),    # the tile: neither axis takes 25
                 (8, 3, 9, 4, 28, 60, 44),    # the tile: 28 * 9 / 4 is whole, 28 * 8 / 3 is not
                 (8, 3, 9, 4, 30, 60, 44),    # ... and the other way round
                 (8, 0, 9, 4, 24, 60, 44), (8, 3, 9, 0, 24, 60, 44), (9, 9, 1, 0, 24, 60, 44),
                 (10, 9, 1, 1, 72, 72, 72), (1, 1, 10, 9, 72, 72, 72),   # den 9
                 (3, 4, 1, 1, 24, 60, 44), (1, 1, 7, 8, 24, 64, 64),     # a ratio below 1
                 (17, 4, 1, 1, 24, 60, 44), (1, 1, 33, 8, 24, 64, 64),   # ... above 4
                 (-8, -3, 9, 4, 24, 60, 44),
                 (8, 3, 9, 4, 0, 60, 44), (8, 3, 9, 4, 24, 0, 44), (8, 3, 9, 4, 24, 60, 0), (8, 3, 9, 4, 24, (1 << 24) + 3, 44)]:
        assert c_out_size("rsr_out_size_xy", *args) == (R.RSR_E_ARG, -1, -1), args
        assert R.lib().rsr_last_error(None)
    # either pointer may be NULL
    assert R.lib().rsr_out_size_xy(8, 3, 9, 4, 24, 60, 44, None, None) == R.RSR_OK
    assert R.lib().rsr_out_size_yuv_xy(8, 3, 9, 4, 24, 60, 40, None, None) == R.RSR_OK
    # the isotropic functions keep their set: 15/8 and 6/5 are pairs only
    ow, oh = C.c_int(-1), C.c_int(-1)
    for n, d in ((15, 8), (6, 5), (9, 5)):
        assert R.lib().rsr_out_size(n, d, 840, 840, 840, C.byref(ow), C.byref(oh)) == R.RSR_E_ARG
        assert R.lib().rsr_out_size_yuv(n, d, 840, 840, 840, C.byref(ow), C.byref(oh)) == R.RSR_E_ARG


def test_worked_examples_and_their_odd_counter_examples():
    y = "rsr_out_size_yuv_xy"
    assert c_out_size(y, 8, 3, 9, 4, 192, 720, 480) == (R.RSR_OK, 1920, 1080)   # NTSC DVD: tile rectangle 512 x 432
    assert (192 * 8 // 3, 192 * 9 // 4) == (512, 432)
    assert c_out_size(y, 8, 3, 15, 8, 192, 720, 576) == (R.RSR_OK, 1920, 1080)  # PAL DVD: 512 x 360
    assert (192 * 8 // 3, 192 * 15 // 8) == (512, 360)
    assert c_out_size(y, 4, 3, 1, 1, 198, 1440, 1080) == (R.RSR_OK, 1920, 1080)  # HDV: 264 x 198
    assert c_out_size(y, 8, 3, 2, 1, 198, 1440, 1080) == (R.RSR_OK, 3840, 2160)
    assert c_out_size(y, 3, 2, 1, 1, 200, 1280, 1080) == (R.RSR_OK, 1920, 1080)  # DVCPRO-HD
    for fn in (y, "rsr_out_size_xy"):
        assert c_out_size(fn, 8, 3, 9, 4, 200, 720, 480) == (R.RSR_E_ARG, -1, -1)  # tile 200: 1600 is no multiple of 3
    # sizes the RGB formats take and a YUV output does not, "YUV" in the message
    for args in [(4, 3, 1, 1, 33, 66, 44),      # the tile rectangle is 44 x 33: an odd number of rows
                 (4, 3, 1, 1, 30, 60, 45),      # an odd h (and 45 rows out)
                 (8, 3, 9, 4, 12, 60, 40),      # tile rectangle 32 x 27
                 (8, 3, 9, 4, 24, 60, 44),      # 160 x 99
                 (3, 2, 1, 1, 30, 62, 44)]:     # 93 columns; tile rectangle 45 x 30
        assert c_out_size("rsr_out_size_xy", *args)[0] == R.RSR_OK, args
        assert c_out_size(y, *args) == (R.RSR_E_ARG, -1, -1), args
        assert b"YUV" in R.lib().rsr_last_error(None)


# ---- the numpy reference -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", AXIS_RATIOS, ids=["%d-%d" % r for r in AXIS_RATIOS])
def test_weights_sum_to_4d_and_taps_are_few(nd):
    n, d = nd
    most = 0
    for X in range(0, 3 * n + 5):
        t = taps(X, n, d)
        assert sum(g for _, g in t) == 4 * d and all(1 <= g <= n for _, g in t)
        assert [i for i, _ in t] == list(range(t[0][0], t[-1][0] + 1))
        most = max(most, len(t))
    assert most <= (4 if nd in RATIOS else 5)
    assert taps(n, n, d)[0] == (4 * d, taps(0, n, d)[0][1])  # n output pixels cover exactly 4 d x4 pixels: a tile starts afresh


def test_some_ratio_needs_five_taps():
    assert max(len(taps(X, 9, 8)) for X in range(9)) == 5


@pytest.mark.parametrize("nd", RATIOS, ids=["%d-%d" % r for r in RATIOS])
def test_equal_axes_reproduce_area_reduce_bit_for_bit(nd):
    v = np.random.default_rng(21).uniform(-0.2, 1.2, size=(3, 48, 96)).astype(np.float32)
    assert np.array_equal(area_reduce_xy(v, nd, nd).view(np.uint32), area_reduce(v, *nd).view(np.uint32))
    a = np.random.default_rng(22).uniform(-5, 260, size=(48, 48)).astype(np.float32)
    assert np.array_equal(area_reduce_xy(a, nd, nd, top=255.0).view(np.uint32), area_reduce(a, *nd, top=255.0).view(np.uint32))


PAIRS = [((8, 3), (9, 4)), ((8, 3), (15, 8)), ((4, 3), (1, 1)), ((4, 1), (2, 1)), ((1, 1), (4, 1)), ((9, 8), (15, 4)), ((7, 5), (10, 7)), ((15, 8), (15, 8))]
PAIR_IDS = ["%d-%d_%d-%d" % (rx + ry) for rx, ry in PAIRS]


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_a_constant_image_stays_that_constant(pair):
    """For a constant c with the 11 significant bits of an fp16 value every partial sum is k * c with an integer k <= 16 dx dy <= 1024: at
    most 21 bits, exact in float32.  The last product is c * 16 dx dy * fp32(1 / (16 dx dy)): exact where dx dy is a power of two; else the
    constant is (1 / (16 dx dy))(1 + e) with |e| <= 2^-24, and c (1 + e), c of 11 bits, rounds back to c."""
    rx, ry = pair
    c = np.arange(0, 0x3C01, 5, dtype=np.uint16).view(np.float16).astype(np.float32)
    side = 4 * rx[1] * ry[1]
    v = np.ascontiguousarray(np.broadcast_to(c[:, None, None], (c.size, side, side)))
    got = area_reduce_xy(v, rx, ry)
    assert got.shape == (c.size, side * ry[0] // (4 * ry[1]), side * rx[0] // (4 * rx[1]))
    assert (got.view(np.uint32) == c.view(np.uint32)[:, None, None]).all()


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_reference_is_the_exact_area_mean_to_float32_rounding(pair):
    """The bound, from the term count, as in tests/test_out_ratio.py with up to 5 taps per axis: a term goes through 1 product with its
    horizontal weight, at most 4 additions of the row sum, 1 product with the vertical weight, at most 4 additions of the column sum and
    the final product, whose constant carries one more rounding: 12 roundings of relative size u = 2^-24.  All terms have one sign, so the
    relative error is at most gamma_12 = 12 u / (1 - 12 u), and the result is at most 1."""
    rx, ry = pair
    u = 2.0 ** -24
    bound = 12 * u / (1 - 12 * u)
    v = np.random.default_rng(23).uniform(-0.2, 1.2, size=(3, 4 * ry[1] * 3, 4 * rx[1] * 5)).astype(np.float32)
    got, want = area_reduce_xy(v, rx, ry), exact_area_mean_xy(v, rx, ry)
    assert got.shape == want.shape and got.min() >= 0 and got.max() <= 1
    err = np.abs(got.astype(np.float64) - np.minimum(want, 1.0))
    print("%s x %s: max |reference - exact area mean| = %.3e (bound %.3e)" % (rx, ry, err.max(), bound))
    assert err.max() <= bound
    # and `want` IS the area mean: every x4 pixel repeated nx / ny times, then plain Ly x Lx block means
    Lx, Ly = 4 * rx[1], 4 * ry[1]
    rep = np.repeat(np.repeat(np.clip(v.astype(np.float64), 0, 1), rx[0], axis=-1), ry[0], axis=-2)
    blocks = rep.reshape(3, rep.shape[1] // Ly, Ly, rep.shape[2] // Lx, Lx).mean(axis=(2, 4))
    assert np.abs(blocks - want).max() <= 1e-14


def test_the_axes_are_not_interchangeable():
    v = np.random.default_rng(24).random((24, 24), dtype=np.float32)
    a, b = area_reduce_xy(v, (4, 3), (1, 1)), area_reduce_xy(v, (1, 1), (4, 3))
    assert a.shape == (6, 8) and b.shape == (8, 6)
    # the transposed image at the swapped pair is the same mean, summed in another order: equal to rounding, no bit claim
    assert np.abs(b - area_reduce_xy(np.ascontiguousarray(v.T), (4, 3), (1, 1)).T).max() <= 12 * 2.0 ** -24


@pytest.mark.parametrize("siting", [0, 1, 2])
def test_sited_encode_with_equal_tile_sizes_is_the_isotropic_one(siting):
    d = np.random.default_rng(25).random((3, 36, 48), dtype=np.float32)
    for tile_out in (0, 12, 24):
        for cfg in ((709, 0, 8), (601, 1, 10)):
            y0, uv0 = yuv_siting_ref.encode(d, siting, tile_out, *cfg)
            y1, uv1 = encode_xy(d, siting, tile_out, tile_out, *cfg)
            assert np.array_equal(y0, y1) and np.array_equal(uv0, uv1)
    if siting == 2:  # the row clamp follows tile_out_y alone
        assert not np.array_equal(encode_xy(d, 2, 12, 12)[1], encode_xy(d, 2, 12, 18)[1])
        assert np.array_equal(encode_xy(d, 1, 12, 12)[1], encode_xy(d, 1, 12, 18)[1])


# ---- the binding -------------------------------------------------------------------------------------------------------------------------
class _Engine:
    """Stands in for the C library behind a RealSR (tests/test_out_ratio.py), holding a ratio per axis as the engine does."""

    def __init__(self):
        self.x, self.y, self.calls, self.stats = (4, 1), (4, 1), [], []

    def rsr_set_option(self, h, key, value):
        if key == b"out_scale":
            if value not in (1, 2, 4):
                return R.RSR_E_ARG
            self.x = self.y = (value, 1)
        return 0

    def rsr_set_out_ratio(self, h, n, d):
        r = admitted(n, d)
        if r is None or r not in RATIOS:
            return R.RSR_E_ARG
        self.x = self.y = r
        return 0

    def rsr_set_out_ratio_xy(self, h, nx, dx, ny, dy):
        rx, ry = admitted(nx, dx), admitted(ny, dy)
        if rx is None or ry is None:
            return R.RSR_E_ARG
        self.x, self.y = rx, ry
        return 0

    def rsr_out_size(self, *a):
        return R.lib().rsr_out_size(*a)  # (host-only: the real ones)

    def rsr_out_size_yuv(self, *a):
        return R.lib().rsr_out_size_yuv(*a)

    def rsr_out_size_xy(self, *a):
        return R.lib().rsr_out_size_xy(*a)

    def rsr_out_size_yuv_xy(self, *a):
        return R.lib().rsr_out_size_yuv_xy(*a)

    def rsr_get_stat(self, h, key, ref):
        same = self.x == self.y
        box = same and self.x in ((4, 1), (2, 1), (1, 1))
        self.stats.append(key)
        ref._obj.value = {b"out_scale": self.x[0] if box else 0, b"out_num": self.x[0] if same else 0, b"out_den": self.x[1] if same else 0,
                          b"out_num_x": self.x[0], b"out_den_x": self.x[1], b"out_num_y": self.y[0], b"out_den_y": self.y[1]}[key]
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


def test_out_ratio_xy_property_out_ratio_and_out_size():
    assert isinstance(R.RealSR.out_ratio_xy, property) and R.RealSR.out_ratio_xy.fset is not None
    e = _Engine()
    sr = R.RealSR(0, _adopt=1)  # (adopts a handle: no device is opened)
    sr._L = e
    sr.tilesize = 24
    img = np.zeros((44, 60, 3), dtype=np.uint8)
    assert sr.out_ratio_xy == (4, 4) and all(isinstance(r, Fraction) for r in sr.out_ratio_xy)
    sr.out_ratio_xy = (Fraction(8, 3), Fraction(9, 4))
    assert (e.x, e.y) == ((8, 3), (9, 4)) and sr.out_ratio_xy == (Fraction(8, 3), Fraction(9, 4)) and sr.out_scale == 0
    with pytest.raises(ValueError, match="out_ratio_xy"):
        sr.out_ratio
    assert sr.out_size(60, 44) == (160, 99) and sr.process(img).shape == (99, 160, 3)
    assert sr.out_size_yuv(60, 40) == (160, 90)
    with pytest.raises(ValueError, match="YUV"):
        sr.out_size_yuv(60, 44)           # 99 rows
    with pytest.raises(ValueError):
        sr.out_size(61, 44)
    with pytest.raises(ValueError):
        sr.process(np.zeros((45, 60, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="8/3 x 9/4"):
        sr.process_rows(img, np.zeros((176, 240, 3), dtype=np.uint8), 0, 1)  # a x4 buffer; the text names the pair
    sr.out_ratio_xy = ((16, 6), 2)        # (n, d) members and ints, unreduced
    assert sr.out_ratio_xy == (Fraction(8, 3), Fraction(2)) and sr.out_size(60, 44) == (160, 88)
    sr.out_ratio_xy = (Fraction(15, 8), Fraction(15, 8))  # equal axes outside the 19: one ratio, served by the _xy functions
    assert sr.out_ratio == Fraction(15, 8) and sr.out_ratio_xy == (Fraction(15, 8), Fraction(15, 8))
    sr.tilesize = 48
    assert sr.out_size(64, 64) == (120, 120) and sr.out_size_yuv(64, 64) == (120, 120)
    sr.tilesize = 24
    for bad in ((Fraction(3, 4), 1), (1, 5), ((10, 9), 1), ((3, 0), 1), (1, (9, 0))):
        with pytest.raises(R.RealSRError) as err:
            sr.out_ratio_xy = bad
        assert err.value.code == R.RSR_E_ARG and sr.out_ratio == Fraction(15, 8)
    for bad in (Fraction(3, 2), (1, 2, 3), 4):
        with pytest.raises(ValueError):
            sr.out_ratio_xy = bad
    # equal axes among the 19 ARE out_ratio; out_ratio and out_scale leave a pair again
    sr.out_ratio_xy = (Fraction(3, 2), Fraction(3, 2))
    assert sr.out_ratio == Fraction(3, 2) and sr.out_size(60, 44) == (90, 66)
    sr.out_ratio_xy = (2, 2)
    assert sr.out_scale == 2 and sr.out_ratio == 2
    sr.out_ratio_xy = (4, 2)
    assert sr.out_scale == 0 and sr.out_size(60, 44) == (240, 88)
    sr.out_ratio = Fraction(3, 2)
    assert sr.out_ratio_xy == (Fraction(3, 2), Fraction(3, 2))
    sr.out_ratio_xy = (1, 4)
    sr.out_scale = 4
    assert sr.out_ratio_xy == (4, 4) and sr.process(img).shape == (176, 240, 3)
    assert len(e.calls) == 2
    # while the axes agree on one of the 19 only today's stats are read
    e.stats.clear()
    sr.out_ratio = Fraction(3, 2)
    sr.out_size(60, 44), sr.out_size_yuv(60, 44), sr.out_ratio, sr.process(img)
    assert set(e.stats) <= {b"out_scale", b"out_num", b"out_den"}
    sr._h = None


class _Stream:
    cuda_stream = 5


class _Ctx:
    """A context that records what torch_io hands the engine (tests/test_out_ratio.py), at (8/3, 9/4) and tile 24; its out_ratio raises."""
    gpuid, scale, out_scale, tilesize = 0, 4, 0, 24
    out_ratio_xy = (Fraction(8, 3), Fraction(9, 4))

    def __init__(self):
        self.calls = []

    @property
    def out_ratio(self):
        raise ValueError("the output ratio differs per axis: read out_ratio_xy")

    def out_size(self, w, h):
        rc, ow, oh = c_out_size("rsr_out_size_xy", 8, 3, 9, 4, self.tilesize, w, h)
        if rc:
            raise ValueError("no such size")
        return ow, oh

    def out_size_yuv(self, w, h):
        rc, ow, oh = c_out_size("rsr_out_size_yuv_xy", 8, 3, 9, 4, self.tilesize, w, h)
        if rc:
            raise ValueError("a YUV output does not take this size")
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


def test_upscale_sizes_out_per_axis(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _Stream())
    s = _Ctx()
    x = _on_cuda0(torch.zeros(3, 8, 12, dtype=torch.float16))
    out = _on_cuda0(torch.zeros(3, 18, 32, dtype=torch.float16))
    assert torch_io.upscale(s, x, out=out) is out
    (kind, a, k), = s.calls
    assert kind == "fmt" and a == (x.data_ptr(), F16, 12, 8, 3, out.data_ptr(), F16) and k == {"stream": 5}
    for shape in ((3, 32, 18), (3, 32, 48), (3, 18, 27), (3, 32, 32)):  # transposed, x4, 9/4 on both axes, 8/3 on both
        with pytest.raises(ValueError, match="out"):
            torch_io.upscale(s, x, out=_on_cuda0(torch.zeros(shape, dtype=torch.float16)))
    with pytest.raises(ValueError):
        torch_io.upscale(s, _on_cuda0(torch.zeros(3, 7, 12, dtype=torch.float16)))  # 7 * 9 is no multiple of 4
    assert len(s.calls) == 1
    # the texts survive a context whose out_ratio raises
    assert torch_io._ratio_text(s) == "8/3 x 9/4" and "8/3 x 9/4" in torch_io._yuv_ratio_note(s)
    with pytest.raises(ValueError, match="YUV"):
        torch_io.upscale_yuv(s, _on_cuda0(torch.zeros(18, 12, dtype=torch.uint8)))  # 12 rows at 9/4 are 27
    assert len(s.calls) == 1


# ---- the CLI -----------------------------------------------------------------------------------------------------------------------------
def test_cli_takes_pairs_and_refuses_the_rest(tmp_path):
    """RSR_OUT_SCALE=x,y is checked with the flags, before an image is read or a GPU touched: a pair of the set passes that check (the run
    then ends at the missing input), everything else is refused there."""
    cli = os.path.join(os.path.dirname(R.LIB_PATH), "..", "bin", "realsr-hip")

    def run(v):
        return subprocess.run([cli, "-i", str(tmp_path / "missing.png"), "-o", str(tmp_path / "o.png")], capture_output=True, text=True,
                              env=dict(os.environ, RSR_OUT_SCALE=v), timeout=60)
    for bad in ("8/3,", ",9/4", "8/3,9/4,1", "8/3;9/4", "3/4,1", "9/9,1/0", "8/3,9/5x", "8/3, 9/4", "10/9,1", "9/5"):
        r = run(bad)
        assert r.returncode != 0 and "invalid RSR_OUT_SCALE" in r.stderr, (bad, r.stderr)
    for good in ("8/3,9/4", "4/3,1", "15/8,15/8", "16/6,2", "4,4"):
        r = run(good)
        assert r.returncode != 0 and "invalid RSR_OUT_SCALE" not in r.stderr, (good, r.stderr)
