"""A ratio per axis on the GPU (run with -m gpu): rsr_set_out_ratio_xy -- DVD and HDV frames to square-pixel sizes, area-averaged on the
device with the horizontal taps of nx / dx and the vertical taps of ny / dy (include/realsr_hip.h, "a ratio per axis").

The contract is exact.  F32 output equals area_reduce_xy (tests/area_reduce_xy.py) of the SAME context's F32 output at x4, bit for bit; F16
is that rounded once; uint8 follows check_u8 of tests/test_gpu_out_ratio.py (at least 20,000 pooled elements, at most 1e-3 of them left
out as within 2^-14 of a rounding boundary, those within 1).  A YUV surface equals the reference encode (encode_xy) of the F32 output at
the same pair, with the sited filters clamped at per-axis tile multiples.  Every entry point gives the bytes of the plain device call.
Outputs are pre-filled with NaN / 0xCD."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import oracle
import realsr_ncnn_vulkan_amd as R
import yuv_ref

import far_layout as fl
import gpu_support as G
from area_reduce_xy import area_reduce_xy, encode_xy, out_rect_xy
from area_reduce import check_u8
from gpu_support import context_fixtures, dev, paths, profile_of  # noqa: F401
from pixfmt_ref import BITS, F16, F32, NP, NV12, P010, U8, bits, image as surface, paste, pattern, same_bits, u8_image as image

pytestmark = pytest.mark.gpu
SENTINEL = 0xCD
# (x ratio, y ratio, w, h, tilesize)
CASES = [((8, 3), (9, 4), 60, 44, 24),     # 160 x 99: a 3 x 2 tile grid whose last tiles are 12 wide, 20 high
         ((8, 3), (15, 8), 60, 64, 48),    # 160 x 120
         ((4, 3), (1, 1), 42, 36, 18),     # one axis at a box ratio
         ((4, 1), (2, 1), 62, 46, 32),     # both box, different
         ((1, 1), (4, 1), 62, 46, 32),
         ((9, 8), (15, 4), 64, 60, 24),    # the 5-tap and the shortest footprint
         ((7, 5), (10, 7), 70, 49, 35)]
CASE_IDS = ["%d-%d_%d-%d" % (c[0] + c[1]) for c in CASES]
RX, RY, W, H, T = CASES[0]
HY = 40  # the height of the YUV cases at (8/3, 9/4): 160 x 90, tile rectangles of 64 x 54


ctxs, ctx = context_fixtures(T, 10, others=("other",))


def fr(r):
    return Fraction(*r)


def set_pair(s, rx, ry, tile=None):
    if tile is not None:
        s.tilesize = tile
    s.out_ratio_xy = (fr(rx), fr(ry))
    assert s.out_ratio_xy == (fr(rx), fr(ry))


def filled_bytes(n, fmt):
    """n bytes of 0xCD -- or, for a float format, of NaN."""
    if fmt in (F16, F32):
        es = 2 if fmt == F16 else 4
        return torch.full((n // es,), float("nan"), dtype=torch.float16 if fmt == F16 else torch.float32, device="cuda").view(torch.uint8)
    return torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")


def untouched_np(a, fmt):
    return bool(np.isnan(a).all()) if fmt in (F16, F32) else bool((a.view(np.uint8) == SENTINEL).all())


def run(s, x, in_fmt, out_fmt):
    """One synchronous rsr_process_device_fmt call at the context's ratio or pair on the packed numpy image x; the result as a numpy array."""
    return G.run(s, x, in_fmt, out_fmt, nan=True)


def x4_f32(s, x, in_fmt):
    """The context's own F32 output at x4 for the image x."""
    s.out_scale = 4
    ref = run(s, x, in_fmt, F32)
    assert ref.min() >= 0 and ref.max() <= 1
    return ref


def check_formats(s, rx, ry, w, h, tile, seed, pool=1):
    """F32, F16 and uint8 at the pair against area_reduce_xy of the context's own x4 F32 output; `pool` images share the uint8 comparison."""
    s.tilesize = tile
    gots, refs = [], []
    for k in range(pool):
        img = image(seed + k, w, h)
        m = area_reduce_xy(x4_f32(s, img, U8), rx, ry)
        set_pair(s, rx, ry)
        got = run(s, img, U8, F32)
        assert got.shape == (3, h * ry[0] // ry[1], w * rx[0] // rx[1]) and s.get_stat("out_scale") == 0
        nd = int((bits(got) != bits(m)).sum())
        print("%s x %s: F32 %d of %d elements differ in bits" % (fr(rx), fr(ry), nd, m.size))
        assert nd == 0
        assert np.array_equal(bits(run(s, img, U8, F16)), bits(m.astype(np.float16)))  # rounded once, to nearest even
        gots.append(run(s, img, U8, U8))
        refs.append(m)
    check_u8(gots, refs, "%s x %s: " % (fr(rx), fr(ry)))


# ---- 1. every pair ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_pair(ctx, case):
    rx, ry, w, h, tile = case
    ow, oh = w * rx[0] // rx[1], h * ry[0] // ry[1]
    check_formats(ctx[False], rx, ry, w, h, tile, 6100, pool=-(-20000 // (3 * ow * oh)))


# ---- 2. modes on (8/3, 9/4) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precise", [0, 1], ids=["fp16", "precise"])
@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_tta_and_precise(ctx, tta, precise):
    s = ctx[tta]
    s.set_option("precise", precise)
    check_formats(s, RX, RY, W, H, T, 6200)


def test_bgr_swaps_channels_of_the_reduced_image(ctx):
    s = ctx[False]
    set_pair(s, RX, RY)
    img = image(6300, W, H)
    rgb8, rgbf = run(s, img, U8, U8), run(s, img, U8, F32)
    rgba = run(s, image(6301, W, H, 4), U8, U8)
    s.set_option("bgr", 1)
    bgr8, bgrf = run(s, np.ascontiguousarray(img[:, :, ::-1]), U8, U8), run(s, np.ascontiguousarray(img[:, :, ::-1]), U8, F32)
    bgra = run(s, np.ascontiguousarray(image(6301, W, H, 4)[:, :, [2, 1, 0, 3]]), U8, U8)
    assert np.array_equal(bgr8[:, :, ::-1], rgb8) and not np.array_equal(bgr8, rgb8)
    assert np.array_equal(bits(np.ascontiguousarray(bgrf[::-1])), bits(rgbf))
    assert np.array_equal(bgra[:, :, [2, 1, 0, 3]], rgba)


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_alpha_is_the_area_mean_of_the_x4_alpha_under_the_per_axis_weights(ctx, tta):
    """The rule and the band of tests/test_gpu_out_ratio.py::test_alpha_is_the_area_mean_of_the_x4_alpha: the reference applied to the
    bicubic x4 of every tile's un-padded alpha rectangle, clamped to [0, 255], stored as floor(mean + 0.5): +-0 outside the elements whose
    mean + 0.5 lies within 2^-10 of an integer, +-1 there (the bicubic's 3.6e-4 and the weighted mean's 12 * 2^-24 * 255 = 1.8e-4 of fp32
    rounding: 5.4e-4 < 2^-10)."""
    s = ctx[tta]
    img = image(6400, W, H, 4)
    a4 = np.empty((4 * H, 4 * W), dtype=np.float32)
    for y0 in range(0, H, T):
        for x0 in range(0, W, T):
            th, tw = min(y0 + T, H) - y0, min(x0 + T, W) - x0
            a4[4 * y0:4 * (y0 + th), 4 * x0:4 * (x0 + tw)] = oracle.bicubic(img[y0:y0 + th, x0:x0 + tw, 3].astype(np.float32), 4 * th, 4 * tw)
    set_pair(s, RX, RY)
    got = run(s, img, U8, U8)
    assert got.shape == (99, 160, 4)
    E = area_reduce_xy(a4, RX, RY, top=255.0).astype(np.float64) + 0.5
    near = np.abs(E - np.rint(E)) < 2.0 ** -10
    want = np.clip(np.floor(E), 0, 255).astype(np.uint8)
    ga = got[:, :, 3]
    print("alpha at 8/3 x 9/4: %d elements, %d left out (within 2^-10 of a rounding boundary), %d differ" % (ga.size, near.sum(), ((ga != want) & ~near).sum()))
    assert near.mean() <= 1e-2
    assert np.array_equal(ga[~near], want[~near])
    assert (np.abs(ga.astype(int) - want.astype(int))[near] <= 1).all()
    assert np.array_equal(got[:, :, :3], run(s, np.ascontiguousarray(img[:, :, :3]), U8, U8))  # RGB as without alpha
    for a in (0, 255):
        flat = img.copy()
        flat[:, :, 3] = a
        assert (run(s, flat, U8, U8)[:, :, 3] == a).all(), a


def test_f16_input_the_uint8_path_cannot_make(ctx):
    s = ctx[False]
    hx = np.random.default_rng(6500).random((3, H, W), dtype=np.float32).astype(np.float16)
    m = area_reduce_xy(x4_f32(s, hx, F16), RX, RY)
    set_pair(s, RX, RY)
    assert np.array_equal(bits(run(s, hx, F16, F32)), bits(m))
    assert np.array_equal(bits(run(s, hx, F16, F16)), bits(m.astype(np.float16)))
    assert np.array_equal(bits(run(s, hx.astype(np.float32), F32, F32)), bits(m))


def test_nv12_input_to_f32_output(ctx):
    """The input side is independent of the output side: an NV12 surface in, F32 out at (8/3, 9/4)."""
    s = ctx[False]
    surf = surface(6600, NV12, W, H)
    ref = x4_f32(s, surf, NV12)
    assert np.array_equal(bits(ref), bits(run(s, yuv_ref.decode(*yuv_ref.split(surf, 8), 709, 0, 8), F32, F32)))
    set_pair(s, RX, RY)
    assert np.array_equal(bits(run(s, surf, NV12, F32)), bits(area_reduce_xy(ref, RX, RY)))


# ---- 3. YUV outputs ----------------------------------------------------------------------------------------------------------------------
YUV_CASES = [((8, 3), (9, 4), 60, HY, 24), ((8, 3), (15, 8), 60, 64, 48), ((4, 3), (1, 1), 42, 36, 18)]
YUV_RUNS = [(c, siting, False, (709, 0)) for c in YUV_CASES for siting in (0, 1, 2)] + [(YUV_CASES[0], 2, True, (709, 0)), (YUV_CASES[1], 1, False, (601, 1))]


@pytest.mark.parametrize("i", range(len(YUV_RUNS)), ids=["%d-%d_%d-%d_s%d_%s_%d-%d" % (c[0] + c[1] + (st, "tta" if t else "plain") + cfg) for c, st, t, cfg in YUV_RUNS])
def test_yuv_outputs(ctx, i):
    (rx, ry, w, h, tile), siting, tta, cfg = YUV_RUNS[i]
    s = ctx[tta]
    set_pair(s, rx, ry, tile)
    s.yuv_siting = siting
    s.set_option("yuv_matrix", cfg[0])
    s.set_option("yuv_range", cfg[1])
    tx, ty = tile * rx[0] // rx[1], tile * ry[0] // ry[1]
    assert s.out_size_yuv(w, h) == (w * rx[0] // rx[1], h * ry[0] // ry[1]) and tx % 2 == 0 and ty % 2 == 0
    x = image(6700 + i, w, h)
    dd = run(s, x, U8, F32)
    assert np.isfinite(dd).all() and len(np.unique(dd)) > 16
    for fmt in (NV12, P010):
        got = run(s, x, U8, fmt)
        want = yuv_ref.join(*encode_xy(dd, siting, tx, ty, cfg[0], cfg[1], BITS[fmt]), BITS[fmt])
        nd = int((got != want).sum()) if got.shape == want.shape else -1
        print("%s x %s siting %d tta %d fmt %d cfg %s: %d of %d samples differ" % (fr(rx), fr(ry), siting, tta, fmt, cfg, nd, want.size))
        assert same_bits(got, want), fmt
        if siting:  # the tile grid shows, and at top-left siting it shows per axis
            assert not same_bits(want, yuv_ref.join(*encode_xy(dd, siting, 0, 0, cfg[0], cfg[1], BITS[fmt]), BITS[fmt]))
        if siting == 2 and tx != ty:
            assert not same_bits(want, yuv_ref.join(*encode_xy(dd, siting, tx, tx, cfg[0], cfg[1], BITS[fmt]), BITS[fmt]))


# ---- 4. equal axes -----------------------------------------------------------------------------------------------------------------------
COUNTS = ("conv_launches", "post_bytes", "pre_bytes", "tiles", "calls", "conv_flops")
STATS = ("out_scale", "out_num", "out_den", "out_num_x", "out_den_x", "out_num_y", "out_den_y")


def test_equal_axes_are_the_single_ratio(ctx):
    s = ctx[False]
    s.tilesize = 32
    img, surf = image(6800, 60, 44), surface(6801, NV12, 60, 44)
    for ratio, stats in ((Fraction(3, 2), (0, 3, 2, 3, 2, 3, 2)), (Fraction(2), (2, 2, 1, 2, 1, 2, 1))):
        if ratio == 2:
            s.out_scale = 2
        else:
            s.out_ratio = ratio
        assert tuple(s.get_stat(k) for k in STATS) == stats
        want, p0 = profile_of(s, lambda: [run(s, img, U8, U8), run(s, img, U8, F32), run(s, surf, NV12, NV12)], merge=1)
        set_pair(s, RX, RY)  # (leave it, and come back through rsr_set_out_ratio_xy, unreduced)
        assert tuple(s.get_stat(k) for k in STATS) == (0, 0, 0, 8, 3, 9, 4)
        with pytest.raises(ValueError, match="out_ratio_xy"):
            s.out_ratio
        n, d = ratio.numerator, ratio.denominator
        assert s._L.rsr_set_out_ratio_xy(s._h, 2 * n, 2 * d, 3 * n, 3 * d) == R.RSR_OK
        assert tuple(s.get_stat(k) for k in STATS) == stats and s.out_ratio == ratio
        got, p1 = profile_of(s, lambda: [run(s, img, U8, U8), run(s, img, U8, F32), run(s, surf, NV12, NV12)], merge=1)
        for a, b in zip(got, want):
            assert same_bits(a, b)
        for key in COUNTS:
            assert p1[key] == p0[key], (ratio, key)
        assert p0["post_ms"] > 0 and p1["post_ms"] > 0
    # out_ratio = ... and out_scale = ... leave a pair again
    set_pair(s, RX, RY)
    s.out_ratio = Fraction(9, 4)
    assert tuple(s.get_stat(k) for k in STATS) == (0, 9, 4, 9, 4, 9, 4)
    set_pair(s, (4, 1), (2, 1))
    assert tuple(s.get_stat(k) for k in STATS) == (0, 0, 0, 4, 1, 2, 1)
    s.out_scale = 1
    assert tuple(s.get_stat(k) for k in STATS) == (1, 1, 1, 1, 1, 1, 1)
    # a refused pair leaves the one in force
    set_pair(s, RX, RY)
    for bad in ((3, 4, 1, 1), (1, 1, 17, 4), (10, 9, 1, 1), (8, 0, 9, 4), (8, 3, 9, 0), (0, 1, 1, 1)):
        assert s._L.rsr_set_out_ratio_xy(s._h, *bad) == R.RSR_E_ARG
        assert tuple(s.get_stat(k) for k in STATS) == (0, 0, 0, 8, 3, 9, 4)
    # 15/8 on both axes: one ratio in the stats, area-averaged
    set_pair(s, (15, 8), (15, 8), 48)
    assert tuple(s.get_stat(k) for k in STATS) == (0, 15, 8, 15, 8, 15, 8) and s.out_ratio == Fraction(15, 8)
    img2 = image(6802, 64, 64)
    got = run(s, img2, U8, F32)
    assert np.array_equal(bits(got), bits(area_reduce_xy(x4_f32(s, img2, U8), (15, 8), (15, 8))))


def test_default_path_guard(ctx, paths):
    """After calls at pairs, xy(4, 4) is the default path: a profiled uint8 call gives the bytes and makes the launches a fresh context does --
    conv_last writes the image itself (351 conv launches, no post-processing launch).  (tests/test_gpu_yuv_ratio.py::test_default_path_guard.)"""
    img = image(6900, W, H)

    def u8_call(s):
        s.tilesize, s.prepadding = T, 10
        return profile_of(s, lambda: run(s, img, U8, U8), merge=1)

    fresh = R.RealSR(0)
    try:
        fresh.load(*paths)
        want, p0 = u8_call(fresh)
    finally:
        fresh.close()
    s = ctx[False]
    for rx, ry in ((RX, RY), ((4, 1), (2, 1)), ((1, 1), (4, 1))):
        set_pair(s, rx, ry)
        run(s, img, U8, U8)
        run(s, image(6901, W, HY), U8, NV12)
    set_pair(s, (4, 1), (4, 1))
    assert s.out_scale == 4 and s.out_ratio == 4
    got, p1 = u8_call(s)
    assert same_bits(got, want) and got.shape == (4 * H, 4 * W, 3)
    assert p0["conv_launches"] == R.NUM_CONVS and p0["post_ms"] == 0 and p0["post_bytes"] == 0 and p0["calls"] == 1
    for key in COUNTS + ("post_ms",):
        assert p1[key] == p0[key], key
    # a pair is the same conv launches and ONE post-processing launch; the byte accounting follows both axes
    set_pair(s, RX, RY)
    _, p2 = profile_of(s, lambda: run(s, img, U8, F32), merge=1)
    set_pair(s, RX, (4, 1))
    _, p3 = profile_of(s, lambda: run(s, img, U8, F32), merge=1)
    assert p2["conv_launches"] == R.NUM_CONVS and p2["post_ms"] > 0 and p2["calls"] == 1
    assert 0 < p2["post_bytes"] < p3["post_bytes"]


# ---- 5. entry points at (8/3, 9/4) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_batch_of_five_into_pitched_windows_equals_lone_calls(ctx, tta):
    s = ctx[tta]
    set_pair(s, RX, RY)
    OW, OH = 160, 99
    for in_fmt, out_fmt, es in ((U8, U8, 3), (U8, F32, 4)):
        xs = [image(7000 + i, W, H) for i in range(5)]
        want = [run(s, x, in_fmt, out_fmt) for x in xs]
        d_in = [dev(x) for x in xs]
        # five windows side by side in ONE canvas of 0xCD / NaN: a margin of 3 rows and 5 elements around each
        cw, ch = 5 * (OW + 5) + 5, OH + 6
        nplanes = 1 if out_fmt == U8 else 3
        canvas = filled_bytes(nplanes * ch * cw * es, out_fmt)
        pitch, plane = cw * es, (0 if out_fmt == U8 else ch * cw * es)
        outs = [(canvas.data_ptr() + 3 * pitch + (5 + i * (OW + 5)) * es, pitch, plane) for i in range(5)]
        g0 = s.get_stat("batch_groups")
        s.process_device_batch([t.data_ptr() for t in d_in], in_fmt, W, H, 3, outs, out_fmt)
        torch.cuda.synchronize()
        assert s.get_stat("batch_groups") == g0 + 1  # ONE merged group
        got = canvas.cpu().numpy().view(NP[out_fmt])
        got = got.reshape(ch, cw, 3) if out_fmt == U8 else got.reshape(3, ch, cw)
        inside = np.zeros(got.shape, dtype=bool)
        for i in range(5):
            x0 = 5 + i * (OW + 5)
            win = got[3:3 + OH, x0:x0 + OW] if out_fmt == U8 else got[:, 3:3 + OH, x0:x0 + OW]
            assert same_bits(np.ascontiguousarray(win), want[i]), (out_fmt, i)
            if out_fmt == U8:
                inside[3:3 + OH, x0:x0 + OW] = True
            else:
                inside[:, 3:3 + OH, x0:x0 + OW] = True
        assert untouched_np(got[~inside], out_fmt)  # the outside of every window


@pytest.mark.parametrize("fmt", [U8, NV12], ids=["u8", "nv12"])
def test_masked_call_writes_exactly_the_marked_per_axis_rectangles(ctx, fmt):
    s = ctx[False]
    set_pair(s, RX, RY)
    s.yuv_siting = 2
    h = H if fmt == U8 else HY
    x = image(7100, W, h) if fmt == U8 else surface(7100, fmt, W, h)
    plain = run(s, x, fmt, fmt)
    nt = 6
    rects = [out_rect_xy(W, h, T, t, RX, RY) for t in range(nt)]
    assert rects[0] == (0, 0, 64, 54) and rects[5] == (128, 54, 160, h * 9 // 4) and rects[4][:2] == (64, 54)
    before = pattern(fmt, plain.shape)
    for mask in ([0, 1, 0, 0, 0, 0], [1, 0, 0, 0, 1, 1], [1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0]):
        d_in, d_out = dev(x), dev(before)
        run0 = s.get_stat("masked_tiles_run")
        s.process_device_masked(d_in.data_ptr(), fmt, W, h, 3, d_out.data_ptr(), fmt, np.asarray(mask, dtype=np.uint8))
        torch.cuda.synchronize()
        assert s.get_stat("masked_tiles_run") == run0 + sum(mask)
        want = before.copy()
        for t in range(nt):
            if mask[t]:
                paste(fmt, want, plain, rects[t])
        assert same_bits(d_out.cpu().numpy().view(NP[fmt]).reshape(plain.shape), want), mask


@pytest.mark.parametrize("fmt", [U8, NV12], ids=["u8", "nv12"])
def test_sequence_of_three_frames_with_a_previous_output(ctx, fmt):
    s = ctx[False]
    set_pair(s, RX, RY)
    s.yuv_siting = 1
    h, n, nt = (H if fmt == U8 else HY), 3, 6
    xs = [image(7200 + k, W, h) if fmt == U8 else surface(7200 + k, fmt, W, h) for k in range(n)]
    plains = [run(s, x, fmt, fmt) for x in xs]
    prev = pattern(fmt, plains[0].shape)
    rects = [out_rect_xy(W, h, T, t, RX, RY) for t in range(nt)]
    masks = np.asarray([[0, 1, 0, 0, 0, 1], [0, 0, 0, 1, 0, 0], [1, 0, 0, 0, 0, 1]], dtype=np.uint8)
    src = R.sequence_sources(masks, True)
    assert (src < 0).any() and (src[2] == [2, 0, -1, 1, -1, 2]).all()
    d_ins = [dev(x) for x in xs]
    d_outs = [torch.full((plains[0].nbytes,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in xs]
    d_prev = dev(prev)
    copied = s.get_stat("seq_tiles_copied")
    s.process_device_sequence([t.data_ptr() for t in d_ins], fmt, W, h, 3, [t.data_ptr() for t in d_outs], fmt, masks.reshape(-1), prev_out=d_prev.data_ptr())
    torch.cuda.synchronize()
    assert s.get_stat("seq_tiles_copied") == copied + int((src != np.arange(n)[:, None]).sum())
    for k in range(n):
        want = np.full(plains[0].shape, SENTINEL, dtype=NP[fmt])
        for t in range(nt):
            paste(fmt, want, prev if src[k, t] < 0 else plains[src[k, t]], rects[t])
        assert sum((r[2] - r[0]) * (r[3] - r[1]) for r in rects) == 160 * (h * 9 // 4)  # the rectangles cover the window: every byte is written
        assert same_bits(d_outs[k].cpu().numpy().view(NP[fmt]).reshape(plains[0].shape), want), k
    assert same_bits(d_prev.cpu().numpy().view(NP[fmt]).reshape(prev.shape), prev)


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_host_entry_points_agree_with_the_device_call(ctx, tta):
    s = ctx[tta]
    set_pair(s, RX, RY)
    tx, ty = 64, 54  # a tile's columns / rows in the output
    for c in (3, 4):
        img = image(7300 + c, W, H, c)
        want = run(s, img, U8, U8)
        assert want.shape == (99, 160, c)
        assert np.array_equal(s.process(img), want)
        assert np.array_equal(s.process_many([img, img])[1], want)
        rows = np.full_like(want, SENTINEL)
        s.process_rows(img, rows, 0, 1)
        assert (rows[ty:] == SENTINEL).all() and np.array_equal(rows[:ty], want[:ty])
        s.process_rows(img, rows, 1, 2)
        assert np.array_equal(rows, want)
        tiles = np.full_like(want, SENTINEL)
        s.process_tiles(img, tiles, 2, 4)  # the last tile of tile row 0 and the first of row 1: rectangles
        assert (tiles[:ty, :2 * tx] == SENTINEL).all() and (tiles[ty:, tx:] == SENTINEL).all()
        assert np.array_equal(tiles[:ty, 2 * tx:], want[:ty, 2 * tx:]) and np.array_equal(tiles[ty:, :tx], want[ty:, :tx])
        s.process_tiles(img, tiles, 0, 2)
        s.process_tiles(img, tiles, 4, 6)
        assert np.array_equal(tiles, want)
        assert np.array_equal(R.process_group([s], img), want)
        with pytest.raises(ValueError):
            s.process_rows(img, np.zeros((4 * H, 4 * W, c), np.uint8), 0, 1)  # a x4 buffer at a pair
    if not tta:  # two members that agree on both axes share the image
        o = ctx["other"]
        set_pair(o, RX, RY)
        img = image(7310, W, H)
        assert np.array_equal(R.process_group([s, o], img), run(s, img, U8, U8))


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(ctx):
    s = ctx[False]
    L = s._L
    set_pair(s, RX, RY)
    s._push_params()
    g0 = s.get_stat("batch_groups")

    def refused(w, h, out_fmt=F32, pitch=0, out_shape=None, yuv=False):
        d_in = torch.zeros((3, h, w), dtype=torch.float32, device="cuda")
        shape = out_shape or (3, h * 9 // 4 + 4, w * 8 // 3 + 4)
        d_out = filled_bytes(int(np.prod(shape)) * (4 if out_fmt == F32 else 1), F32 if out_fmt == F32 else U8)
        torch.cuda.synchronize()
        rc = L.rsr_process_device_batch(s._h, 1, R._images([d_in.data_ptr()]), F32, w, h, 3, R._images([(d_out.data_ptr(), pitch, 0)]), out_fmt, None)
        rc2 = L.rsr_process_device_fmt(s._h, C.c_void_p(d_in.data_ptr()), F32, w, h, 3, C.c_void_p(d_out.data_ptr()), out_fmt, None) if not pitch else rc
        nt = -(-w // s.tilesize) * -(-h // s.tilesize)
        ones = np.ones(nt, dtype=np.uint8)
        rc3 = L.rsr_process_device_masked(s._h, R._images([d_in.data_ptr()]), F32, w, h, 3, R._images([(d_out.data_ptr(), pitch, 0)]), out_fmt, R._p(ones), nt, None)
        torch.cuda.synchronize()
        assert rc == R.RSR_E_ARG and rc2 == R.RSR_E_ARG and rc3 == R.RSR_E_ARG, (rc, rc2, rc3)
        msg = L.rsr_last_error(s._h).decode()
        assert msg and (not yuv or "YUV" in msg), msg
        got = d_out.cpu().numpy()
        assert untouched_np(got.view(np.float32) if out_fmt == F32 else got, F32 if out_fmt == F32 else U8) and s.get_stat("batch_groups") == g0
    refused(61, 44)                                   # a w the x ratio does not take (61 * 8 / 3)
    refused(60, 45)                                   # an h the y ratio does not take (45 * 9 / 4)
    for tile in (28, 30, 25):                         # 28: the y ratio takes it, the x ratio does not; 30: the other way round; 25: neither
        s.tilesize = tile
        s._push_params()
        refused(60, 44)
    s.tilesize = T
    s._push_params()
    refused(60, 44, pitch=4 * (160 - 1), out_shape=(3, 99, 160))          # a pitch one element short of the per-axis row
    refused(60, 44, pitch=4 * 135, out_shape=(3, 99, 160))                # the row pitch of the 9/4 x 9/4 size: a window too narrow for 8/3 along x
    refused(60, 44, out_fmt=NV12, out_shape=(300, 300), yuv=True)         # 99 rows: an odd reduced size
    s.tilesize = 12
    s._push_params()
    refused(60, 40, out_fmt=NV12, out_shape=(300, 300), yuv=True)         # tile rectangle 32 x 27: odd
    s.tilesize = T
    s._push_params()
    with pytest.raises(ValueError, match="YUV"):
        s.out_size_yuv(60, 44)
    # the host entry points: an h the y ratio does not take
    img, out = image(7400, 60, 45), np.full((101, 160, 3), SENTINEL, dtype=np.uint8)
    assert L.rsr_process(s._h, R._p(img), 60, 45, 3, R._p(out)) == R.RSR_E_ARG and (out == SENTINEL).all()
    hs = (C.c_void_p * 1)(s._h)
    assert L.rsr_process_group(hs, 1, R._p(img), 60, 45, 3, R._p(out)) == R.RSR_E_ARG and (out == SENTINEL).all()
    with pytest.raises(ValueError):
        s.process(img)
    # a group whose members differ on one axis
    o = ctx["other"]
    set_pair(o, RX, (2, 1))
    img, out = image(7401, W, H), np.full((99, 160, 3), SENTINEL, dtype=np.uint8)
    with pytest.raises(R.RealSRError) as e:
        R.process_group([s, o], img, out=out)
    assert e.value.code == R.RSR_E_ARG and (out == SENTINEL).all()
    # and the context is as usable as before
    assert run(s, image(7402, W, H), U8, U8).shape == (99, 160, 3)


# ---- 7. 64-bit addressing ----------------------------------------------------------------------------------------------------------------
def test_an_output_window_whose_rows_lie_beyond_2_to_32(ctx):
    """Layout R of tests/far_layout.py for the 128 x 108 uint8 output of a 48 x 48 image at (8/3, 9/4): the row pitch puts the last six rows
    beyond 2^32 bytes from `data`.  The window holds the bytes of the packed call; with the window refilled the arena is untouched."""
    s = ctx[False]
    set_pair(s, RX, RY)
    w = h = 48
    ow, oh = s.out_size(w, h)
    assert (ow, oh) == (128, 108)
    win = fl.Window("R", U8, ow, oh)
    assert (oh - 1) * win.row_pitch > fl.B32
    nbytes = -(-(fl.BASE + win.tail() + 4096) // 4096) * 4096
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + fl.HEADROOM:
        pytest.skip("the far window needs %.2f GiB of free device memory + 4 GiB headroom, %.2f GiB are free" % (nbytes / fl.GIB, free / fl.GIB))
    img = image(7500, w, h)
    want = run(s, img, U8, U8)
    arena = fl.new_arena(nbytes)
    try:
        d_in = dev(img)
        torch.cuda.synchronize()
        s.process_device_batch([d_in.data_ptr()], U8, w, h, 3, [win.desc(arena)], U8)
        torch.cuda.synchronize()
        got = fl.get(arena, win)
        fl.refill(arena, win)
        bad = fl.scan(arena)
    finally:
        del arena
        torch.cuda.empty_cache()
    assert np.array_equal(got, fl.raw(want))
    assert bad is None, "the arena was written outside the window, first at byte %d from the image base" % (bad - fl.BASE)


# ---- 8. the CLI --------------------------------------------------------------------------------------------------------------------------
def test_cli_out_ratio_xy(ctx, tmp_path, model_dir):
    from cli_support import CLI, read_png, write_png
    s = ctx[False]
    img = image(7600, 72, 48)
    write_png(tmp_path / "a.png", img)
    r = subprocess.run([CLI, "-i", str(tmp_path / "a.png"), "-o", str(tmp_path / "o.png"), "-m", model_dir, "-t", "36", "-v"],
                       capture_output=True, text=True, env=dict(os.environ, RSR_OUT_SCALE="8/3,9/4"), timeout=300)
    assert r.returncode == 0, r.stderr
    assert "8/3 along x, 9/4 along y" in r.stderr
    got = read_png(tmp_path / "o.png")
    assert got.shape == (108, 192, 3)
    set_pair(s, RX, RY, 36)
    assert np.abs(got.astype(int) - s.process(img).astype(int)).max() <= 1
    write_png(tmp_path / "odd.png", image(7601, 72, 46))
    r = subprocess.run([CLI, "-i", str(tmp_path / "odd.png"), "-o", str(tmp_path / "odd_o.png"), "-m", model_dir, "-t", "36"],
                       capture_output=True, text=True, env=dict(os.environ, RSR_OUT_SCALE="8/3,9/4"), timeout=300)
    assert r.returncode != 0 and not (tmp_path / "odd_o.png").exists()
