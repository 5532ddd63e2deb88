"""NV12 / P010 OUTPUT at a rational output ratio on the GPU (run with -m gpu): include/realsr_hip.h, "YUV output at a ratio".

Everything here is EXACT, no tolerance anywhere.  The tie is the one of tests/test_gpu_yuv.py and tests/test_gpu_yuv_siting.py, at the
ratio in force: the surface a call writes equals

    yuv_ref.join(*yuv_siting_ref.encode(F32 output of the same context at that ratio, siting, tilesize * n / d, matrix, range, bits))

bit for bit -- the F32 output itself is pinned to area_reduce of the x4 image by tests/test_gpu_out_ratio.py.  Every image is a 2 x 2 tile
grid whose last tiles are partial, so tile-first columns and rows and short tiles are all hit.  Outputs are pre-filled with 0xCD."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

import sequence_ref
import tile_diff_ref
import yuv_ref
import yuv_siting_ref as ref
from gpu_support import context_fixtures, dev, paths, profile_of, run  # noqa: F401
from pixfmt_ref import BITS, F16, F32, NP, NV12, P010, U8, image_at, lift, paste, pattern, place, same_bits

pytestmark = pytest.mark.gpu
CFGS = [(709, 0), (601, 1), (2020, 0), (709, 1), (601, 0), (2020, 1)]  # (yuv_matrix, yuv_range)
SENTINEL = 0xCD
# (n, d, tilesize, w, h): w n / d, h n / d and tilesize n / d are even; 2 x 2 tiles, the last ones partial
RATIOS = [(3, 2, 32, 60, 44), (4, 3, 30, 54, 42), (9, 4, 32, 56, 40), (3, 1, 32, 50, 38), (5, 2, 32, 52, 36), (7, 4, 32, 56, 40)]
W, H, T = 60, 44, 32  # the 3/2 case: 90 x 66, tile rectangles of 48; tiles of 32 and 28 columns, 32 and 12 rows
OW, OH = 90, 66
NT = 4


ctxs, ctx = context_fixtures(T, 10)
surface = rgb_image = image_at(W, H)


def set_cfg(s, cfg):
    s.set_option("yuv_matrix", cfg[0])
    s.set_option("yuv_range", cfg[1])


def encoded(d, siting, tile_out, cfg, fmt):
    return yuv_ref.join(*ref.encode(d, siting, tile_out, cfg[0], cfg[1], BITS[fmt]), BITS[fmt])


def planes(surf):
    h = surf.shape[0] * 2 // 3
    return surf[:h], surf[h:]


# ---- 1. the definition ------------------------------------------------------------------------------------------------------------------
# the whole cross product ratio x siting x TTA x precise (a case is a few hundredths of a second); every case writes BOTH surface formats;
# the matrix / range rotate with the case and the format, the source alternates between uint8 and fp16
DEFN = [(r, siting, tta, precise) for r in RATIOS for siting in (0, 1, 2) for tta in (False, True) for precise in (0, 1)]


@pytest.mark.parametrize("i", range(len(DEFN)), ids=["%d-%d_s%d_%s_%s" % (r[0], r[1], st, "tta" if t else "plain", "precise" if p else "fp16") for r, st, t, p in DEFN])
def test_definition(ctx, i):
    (n, d, tile, w, h), siting, tta, precise = DEFN[i]
    s = ctx[tta]
    s.tilesize = tile
    s.set_option("precise", precise)
    s.out_ratio = Fraction(n, d)
    s.yuv_siting = siting
    assert tile * n % d == 0 and (tile * n // d) % 2 == 0
    src = (U8, F16)[(i // 4 + i) % 2]
    x = rgb_image(9000 + i, src, w, h)
    dd = run(s, x, src, F32, w, h)
    assert dd.shape == (3, h * n // d, w * n // d) and np.isfinite(dd).all() and len(np.unique(dd)) > 16
    for fmt in (NV12, P010):
        cfg = CFGS[(i + i // 6 + fmt) % 6]
        set_cfg(s, cfg)
        got = run(s, x, src, fmt, w, h)
        want = encoded(dd, siting, tile * n // d, cfg, fmt)
        nd = int((got != want).sum()) if got.shape == want.shape else -1
        print("%d/%d siting %d tta %d precise %d fmt %d cfg %s: %d of %d samples differ" % (n, d, siting, tta, precise, fmt, cfg, nd, want.size))
        assert same_bits(got, want), (fmt, cfg)
        if siting:  # the tile grid shows: without the clamp at tile-first columns / rows the surface would differ
            assert not same_bits(want, encoded(dd, siting, 0, cfg, fmt))
    assert same_bits(run(s, x, src, F32, w, h), dd)  # (the RGB formats are not concerned by any of the YUV options)


def test_sitings_share_luma_and_differ_in_chroma(ctx):
    s = ctx[False]
    s.out_ratio = Fraction(3, 2)
    x = rgb_image(9100, U8)
    seen = []
    for siting in (0, 1, 2):
        s.yuv_siting = siting
        seen.append(run(s, x, U8, NV12))
    for a in range(3):
        for b in range(a):
            assert np.array_equal(planes(seen[a])[0], planes(seen[b])[0]) and not np.array_equal(planes(seen[a])[1], planes(seen[b])[1])


# ---- 2. the input side is independent ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,siting", [(NV12, 0), (NV12, 1), (P010, 2)], ids=["nv12-s0", "nv12-s1", "p010-s2"])
def test_yuv_input_to_yuv_output_is_the_composition(ctx, fmt, siting):
    s = ctx[False]
    s.out_ratio = Fraction(3, 2)
    s.yuv_siting = siting
    surf = surface(9200 + fmt, fmt)
    x = ref.decode(*yuv_ref.split(surf, BITS[fmt]), siting, 709, 0, BITS[fmt])
    got = run(s, surf, fmt, fmt)
    assert got.shape == (OH * 3 // 2, OW)
    assert same_bits(got, run(s, x, F32, fmt))
    assert same_bits(got, encoded(run(s, x, F32, F32), siting, 48, (709, 0), fmt))


# ---- 3. batches ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_batch_of_five_equals_lone_calls(ctx, tta):
    s = ctx[tta]
    s.out_ratio = Fraction(3, 2)
    s.yuv_siting = 1
    for fmt in (NV12, P010):
        xs = [surface(9300 + k, fmt) for k in range(5)]
        want = [run(s, x, fmt, fmt) for x in xs]
        assert not same_bits(want[0], want[1])
        d_in = [dev(x) for x in xs]
        d_out = [torch.full((want[0].nbytes,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in xs]
        calls = s.get_stat("batch_calls")
        s.process_device_batch([t.data_ptr() for t in d_in], fmt, W, H, 3, [t.data_ptr() for t in d_out], fmt)
        torch.cuda.synchronize()
        assert s.get_stat("batch_calls") == calls + 1
        for k in range(5):
            assert same_bits(d_out[k].cpu().numpy().view(NP[fmt]).reshape(want[k].shape), want[k]), (fmt, k)


# ---- 4. pitched surfaces, a window inside a larger canvas ------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [NV12, P010], ids=["nv12", "p010"])
def test_pitched_surfaces_into_windows(ctx, fmt):
    """Two top-left-sited surfaces in ONE batch call, each inside a larger allocation (row pitch > w, the UV plane farther than h * pitch
    behind Y, NV12 at odd addresses), each into a window of a 0xCD canvas: the windows hold the lone call's bytes, nothing else is touched."""
    s = ctx[False]
    s.out_ratio = Fraction(3, 2)
    s.yuv_siting = 2
    es = NP[fmt]().itemsize
    surfs = [surface(9400 + k, fmt) for k in range(2)]
    lone = [run(s, x, fmt, fmt) for x in surfs]
    ipitch, iplane, ioff = (W + 5) * es, (H + 3) * (W + 5) * es, 3 * es
    opitch, oplane, ooff = (OW + 7) * es, (OH + 2) * (OW + 7) * es + 6 * es, 5 * es
    ispan, ospan = R.image_span(fmt, W, H, 3, ipitch, iplane), R.image_span(fmt, OW, OH, 3, opitch, oplane)
    ins, outs, keep = [], [], []
    for x in surfs:
        canvas = np.full(ioff + ispan + 64, 0x5A, dtype=np.uint8)
        place(canvas, ioff, ipitch, iplane, x, fmt)
        d_in = torch.from_numpy(canvas).cuda()
        d_out = torch.full((ooff + ospan + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        keep.append((d_in, d_out))
        ins.append((d_in.data_ptr() + ioff, ipitch, iplane))
        outs.append((d_out.data_ptr() + ooff, opitch, oplane))
    s.process_device_batch(ins, fmt, W, H, 3, outs, fmt)
    torch.cuda.synchronize()
    for (_, d_out), want in zip(keep, lone):
        got = d_out.cpu().numpy()
        assert same_bits(lift(got, ooff, opitch, oplane, fmt, OW, OH), want)
        inside = place(np.zeros_like(got), ooff, opitch, oplane, want, fmt)
        assert (got[~inside] == SENTINEL).all()  # no byte outside the Y and UV windows is touched
        assert inside.sum() == want.nbytes


def test_upscale_yuv_of_a_crop_into_a_window_of_a_canvas(ctx):
    """torch_io: a 60 x 44 crop of a decoder frame (a (y, uv) pair of views) into the 90 x 66 window of a larger NV12 canvas."""
    s = ctx[False]
    s.out_ratio = Fraction(3, 2)
    s.yuv_siting = 1
    frame = torch.from_numpy(surface(9500, NV12, 80, 60)).cuda()  # 60 rows of Y, 30 of UV
    fy, fuv = frame[:60], frame[60:]
    crop = (fy[8:8 + H, 12:12 + W], fuv[4:4 + H // 2, 12:12 + W])
    want = torch_io.upscale_yuv(s, torch.cat([crop[0], crop[1]]).contiguous())
    assert tuple(want.shape) == (OH * 3 // 2, OW) and want.dtype == torch.uint8
    canvas = torch.full((150, 128), SENTINEL, dtype=torch.uint8, device="cuda")  # 100 rows of Y, 50 of UV
    window = (canvas[12:12 + OH, 18:18 + OW], canvas[100 + 6:100 + 6 + OH // 2, 18:18 + OW])
    got = torch_io.upscale_yuv(s, crop, out=window)
    torch.cuda.synchronize()
    assert got is window
    assert torch.equal(torch.cat([window[0], window[1]]), want) and not bool((want == SENTINEL).all())
    outside = torch.ones_like(canvas, dtype=torch.bool)
    outside[12:12 + OH, 18:18 + OW] = False
    outside[106:106 + OH // 2, 18:18 + OW] = False
    assert bool((canvas[outside] == SENTINEL).all())


# ---- 5. masked and sequence calls -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,siting", [(NV12, 0), (NV12, 2), (P010, 1)], ids=["nv12-s0", "nv12-s2", "p010-s1"])
def test_masked_call_writes_the_plain_bytes_of_its_tiles_only(ctx, fmt, siting):
    s = ctx[False]
    s.out_ratio = Fraction(3, 2)
    s.yuv_siting = siting
    x = surface(9600 + fmt, fmt)
    plain = run(s, x, fmt, fmt)
    rects = [tile_diff_ref.out_rect(W, H, T, t, 3, 2) for t in range(NT)]
    assert rects == [(0, 0, 48, 48), (48, 0, 90, 48), (0, 48, 48, 66), (48, 48, 90, 66)]
    before = pattern(fmt, plain.shape)
    for mask in ([0, 1, 0, 0], [1, 0, 0, 1], [0, 0, 1, 1], [1, 1, 1, 1], [0, 0, 0, 0]):
        d_in, d_out = dev(x), dev(before)
        run0 = s.get_stat("masked_tiles_run")
        s.process_device_masked(d_in.data_ptr(), fmt, W, H, 3, d_out.data_ptr(), fmt, np.asarray(mask, dtype=np.uint8))
        torch.cuda.synchronize()
        assert s.get_stat("masked_tiles_run") == run0 + sum(mask)
        want = before.copy()
        for t in range(NT):
            if mask[t]:
                paste(fmt, want, plain, rects[t])
        assert same_bits(d_out.cpu().numpy().view(NP[fmt]).reshape(plain.shape), want), mask


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_sequence_call_computes_and_propagates_reduced_rectangles(ctx, tta):
    s = ctx[tta]
    s.out_ratio = Fraction(3, 2)
    s.yuv_siting = 1
    n = 3
    xs = [surface(9700 + k, NV12) for k in range(n)]
    plains = [run(s, x, NV12, NV12) for x in xs]
    prev = pattern(NV12, plains[0].shape)
    rects = [tile_diff_ref.out_rect(W, H, T, t, 3, 2) for t in range(NT)]
    for masks, pv in (([[0, 1, 0, 0], [0, 0, 0, 1], [1, 0, 0, 0]], prev), ([[1, 1, 1, 1], [0, 0, 0, 0], [0, 1, 1, 0]], None)):
        src = sequence_ref.sources(np.asarray(masks), pv is not None)
        d_ins = [dev(x) for x in xs]
        d_outs = [torch.full((plains[0].nbytes,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in xs]
        d_prev = dev(pv) if pv is not None else None
        copied = s.get_stat("seq_tiles_copied")
        s.process_device_sequence([t.data_ptr() for t in d_ins], NV12, W, H, 3, [t.data_ptr() for t in d_outs], NV12, np.asarray(masks, dtype=np.uint8).reshape(-1),
                                  prev_out=d_prev.data_ptr() if d_prev is not None else None)
        torch.cuda.synchronize()
        assert s.get_stat("seq_tiles_copied") == copied + int((src != np.arange(n)[:, None]).sum())
        for k in range(n):
            want = np.full(plains[0].shape, SENTINEL, dtype=np.uint8)
            for t in range(NT):
                paste(NV12, want, pv if src[k, t] < 0 else plains[src[k, t]], rects[t])  # a propagated rectangle is identical to its source
            assert same_bits(d_outs[k].cpu().numpy().reshape(plains[0].shape), want), (masks, k)
        if d_prev is not None:
            assert same_bits(d_prev.cpu().numpy().reshape(prev.shape), prev)


def test_upscale_delta_and_upscale_sequence_on_surfaces(ctx):
    s = ctx[False]
    s.out_ratio = Fraction(3, 2)
    s.yuv_siting = 1
    frames = [surface(9800, NV12)]
    for k, (px, py) in enumerate([(58, 42), (2, 3), (58, 42)]):  # one luma sample moves per frame: the last tile, the first, the last
        f = frames[-1].copy()
        f[py, px] ^= 0x80
        frames.append(f)
    frames.append(frames[-1].copy())  # a frame that repeats
    ts = [torch.from_numpy(f).cuda() for f in frames]
    wants = [torch_io.upscale_yuv(s, t) for t in ts]
    torch.cuda.synchronize()
    assert tuple(wants[0].shape) == (OH * 3 // 2, OW) and not torch.equal(wants[0], wants[1])
    y = wants[0].clone()
    total = 0
    for k in range(1, len(ts)):
        y, nrun = torch_io.upscale_delta(s, ts[k], ts[k - 1], y)
        torch.cuda.synchronize()
        assert torch.equal(y, wants[k]), k
        assert nrun == (0 if k == 4 else 1), (k, nrun)
        total += nrun
    out = torch.full_like(wants[0], SENTINEL)
    y2, nrun = torch_io.upscale_delta(s, ts[1], None, wants[0], out=out)  # every tile runs; wants[0] only lends its layout
    torch.cuda.synchronize()
    assert y2 is out and nrun == NT and torch.equal(out, wants[1])
    ys, nrun = torch_io.upscale_sequence(s, ts)
    torch.cuda.synchronize()
    assert nrun == NT + total and len(ys) == len(ts)
    for k, yk in enumerate(ys):
        assert torch.equal(yk, wants[k]), k
    pairs = [(t[:H], t[H:]) for t in ts]
    yp, nrun = torch_io.upscale_sequence(s, pairs[1:], prev_x=pairs[0], prev_y=(wants[0][:OH], wants[0][OH:]))
    torch.cuda.synchronize()
    assert nrun == total
    for k, (py_, puv) in enumerate(yp):
        assert torch.equal(torch.cat([py_, puv]), wants[1 + k]), k


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_output_untouched_and_launch_nothing(ctx):
    s = ctx[False]
    s.out_ratio = Fraction(3, 2)
    d_out = torch.full((4 * 300 * 300,), SENTINEL, dtype=torch.uint8, device="cuda")
    groups, calls = s.get_stat("batch_groups"), s.get_stat("batch_calls")
    seq = [s.get_stat(k) for k in ("seq_calls", "seq_tiles_run", "masked_calls")]

    def refused(fn):
        with pytest.raises(R.RealSRError) as e:
            fn()
        torch.cuda.synchronize()
        assert e.value.code == R.RSR_E_ARG and "YUV" in str(e.value), str(e.value)
        assert bool((d_out == SENTINEL).all())
        assert s.get_stat("batch_groups") == groups and s.get_stat("batch_calls") == calls
        assert [s.get_stat(k) for k in ("seq_calls", "seq_tiles_run", "masked_calls")] == seq

    def calls_for(w, h, in_fmt=NV12, out_fmt=NV12):
        d_in = dev(surface(9900, in_fmt, w, h) if in_fmt in BITS else rgb_image(9900, in_fmt, w, h))
        nt = int(np.prod(tile_diff_ref.tile_count(w, h, s.tilesize)))
        yield lambda: s.process_device_fmt(d_in.data_ptr(), in_fmt, w, h, 3, d_out.data_ptr(), out_fmt)
        yield lambda: s.process_device_batch([d_in.data_ptr()], in_fmt, w, h, 3, [d_out.data_ptr()], out_fmt)
        yield lambda: s.process_device_masked(d_in.data_ptr(), in_fmt, w, h, 3, d_out.data_ptr(), out_fmt, np.ones(nt, dtype=np.uint8))
        yield lambda: s.process_device_sequence([d_in.data_ptr()], in_fmt, w, h, 3, [d_out.data_ptr()], out_fmt, np.ones(nt, dtype=np.uint8))

    for w, h in ((62, 46), (70, 50), (60, 46), (62, 44)):  # 93 x 69, 105 x 75, an odd height, an odd width
        for fn in calls_for(w, h):
            refused(fn)
    for fn in calls_for(62, 46, U8, P010):  # the input side does not help
        refused(fn)
    for tile in (30, 33):  # a tile's rectangle would be 45 / would not be whole
        s.tilesize = tile
        for fn in calls_for(W, H):
            refused(fn)
        with pytest.raises(ValueError, match="YUV"):
            s.out_size_yuv(W, H)
        with pytest.raises(ValueError, match="YUV"):
            torch_io.upscale_yuv(s, torch.zeros((H * 3 // 2, W), dtype=torch.uint8, device="cuda"))
    s.tilesize = T
    surf = torch.from_numpy(surface(9901, NV12)).cuda()
    for shape in ((4 * H * 3 // 2, 4 * W), (2 * H * 3 // 2, 2 * W), (H * 3 // 2, W)):  # out= of the x4, x2 and x1 sizes
        out = torch.full(shape, SENTINEL, dtype=torch.uint8, device="cuda")
        with pytest.raises(ValueError, match="YUV"):
            torch_io.upscale_yuv(s, surf, out=out)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())
    with pytest.raises(ValueError, match="YUV"):
        torch_io.upscale_yuv(s, torch.zeros((69, 62), dtype=torch.uint8, device="cuda"))
    assert s.get_stat("batch_groups") == groups and s.get_stat("batch_calls") == calls
    # the context is usable afterwards
    x = surface(9902, NV12)
    got = run(s, x, NV12, NV12)
    assert same_bits(got, encoded(run(s, yuv_ref.decode(*yuv_ref.split(x, 8), 709, 0, 8), F32, F32), 0, 48, (709, 0), NV12))


# ---- 7. the integer ratios and the default path are untouched --------------------------------------------------------------------------
COUNTS = ("conv_launches", "post_bytes", "pre_bytes", "tiles", "calls", "conv_flops")


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_ratios_4_2_1_are_out_scale_4_2_1(ctx, tta):
    s = ctx[tta]
    s.yuv_siting = 1
    x = surface(9950, NV12)
    for k in (4, 2, 1):
        s.out_scale = k
        want, p0 = profile_of(s, lambda: run(s, x, NV12, NV12), merge=1)
        s.out_ratio = Fraction(3, 2)  # (leave it, and come back through rsr_set_out_ratio)
        assert s.out_scale == 0
        s.out_ratio = (2 * k, 2)
        assert s.out_scale == k and s.out_size_yuv(W, H) == (W * k, H * k)
        got, p1 = profile_of(s, lambda: run(s, x, NV12, NV12), merge=1)
        assert same_bits(got, want) and got.shape == (H * k * 3 // 2, W * k)
        for key in COUNTS:
            assert p1[key] == p0[key], (k, key)
        assert p0["conv_launches"] > 0 and p0["post_ms"] > 0 and p1["post_ms"] > 0


def test_default_path_guard(ctx, paths):
    """After YUV calls at ratios on a context, a uint8 call gives the bytes and makes the launches a fresh context does: conv_last writes
    the image itself (351 conv launches, no post-processing launch).  (The approach of tests/test_gpu_yuv.py::test_default_path_guard.)"""
    img = rgb_image(9960, U8)

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
    for ratio in (Fraction(3, 2), Fraction(3), Fraction(5, 2)):
        s.out_ratio = ratio
        for fmt in (NV12, P010):
            s.yuv_siting = fmt % 3
            run(s, surface(9961, fmt), fmt, fmt)
            run(s, img, U8, fmt)
    s.yuv_siting = 0
    s.out_scale = 4
    got, p1 = u8_call(s)
    assert same_bits(got, want) and got.shape == (4 * H, 4 * W, 3)
    assert p0["conv_launches"] == R.NUM_CONVS and p0["post_ms"] == 0 and p0["post_bytes"] == 0 and p0["calls"] == 1
    for key in COUNTS + ("post_ms",):
        assert p1[key] == p0[key], key
    # a YUV output at 3/2 is the same conv launches and ONE post-processing launch, which writes fewer bytes than the x4 surface's
    _, p4 = profile_of(s, lambda: run(s, img, U8, NV12), merge=1)
    s.out_ratio = Fraction(3, 2)
    _, p2 = profile_of(s, lambda: run(s, img, U8, NV12), merge=1)
    assert p2["conv_launches"] == R.NUM_CONVS and p2["post_ms"] > 0 and p2["calls"] == 1
    assert 0 < p2["post_bytes"] < p4["post_bytes"]
