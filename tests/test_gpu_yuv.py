"""NV12 / P010 device images on the GPU (run with -m gpu): RSR_FMT_NV12 / RSR_FMT_P010 on either side of rsr_process_device_fmt and
rsr_process_device_batch, options "yuv_matrix" / "yuv_range", torch_io.upscale_yuv.

Everything here is EXACT, no tolerance anywhere: the YUV formats are tied bit for bit to the planar fp32 format of the same context
through tests/yuv_ref.py, the numpy float32 restatement of the definition in include/realsr_hip.h (the float formats' own tie to the
uint8 path is tests/test_gpu_tensor_io.py, that path's parity against the oracle tests/test_gpu_parity.py).

    input side    yuv -> f32  ==  f32 -> f32 with x = yuv_ref.decode(surface)
    output side   x -> yuv    ==  yuv_ref.encode(x -> f32)
    end to end    yuv -> yuv  ==  yuv_ref.encode(f32 -> f32 with x = yuv_ref.decode(surface))

The baseline image is 36 x 26 at tile 16, prepadding 10: 3 x 2 tiles, partial tiles on both edges, reflect halos wider than a chroma sample.
"""
import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

import yuv_ref
from gpu_support import context_fixtures, paths, run as run_sized  # noqa: F401
from pixfmt_ref import BITS, F16, F32, NP, NV12, P010, U8, image_at, lift, place, same_bits

pytestmark = pytest.mark.gpu
W, H, T = 36, 26, 16
CFGS = [(709, 0), (601, 1), (2020, 0), (709, 1), (601, 0), (2020, 1)]  # (yuv_matrix, yuv_range)
SENTINEL = 0xCD
ctxs, ctx = context_fixtures(T, 10)
surface = rgb_image = image_at(W, H)


def run(s, x, in_fmt, out_fmt, w=W, h=H):
    """One synchronous rsr_process_device_fmt call on the numpy image x into w x h times out_scale -- sized here, not by the library: a call
    the library must refuse has to reach it."""
    return run_sized(s, x, in_fmt, out_fmt, w, h, out_size=(w * s.out_scale, h * s.out_scale))


def set_cfg(s, cfg):
    s.set_option("yuv_matrix", cfg[0])
    s.set_option("yuv_range", cfg[1])


# ---- 1. input tie ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [NV12, P010], ids=["nv12", "p010"])
@pytest.mark.parametrize("mode", ["default", "tta", "precise"])
def test_input_tie(ctx, mode, fmt):
    s = ctx[mode == "tta"]
    s.set_option("precise", int(mode == "precise"))
    surf = surface(11 + fmt, fmt)
    y, uv = yuv_ref.split(surf, BITS[fmt])
    seen = []
    for cfg in CFGS:
        set_cfg(s, cfg)
        ref = yuv_ref.decode(y, uv, cfg[0], cfg[1], BITS[fmt])
        assert (ref == 0).any() and (ref == 1).any() and len(np.unique(ref)) > 100  # the clamp acts, and not everywhere
        got = run(s, surf, fmt, F32)
        assert not (got.view(np.uint8) == SENTINEL).all()
        assert same_bits(got, run(s, ref, F32, F32)), cfg
        seen.append(got)
    assert s.get_stat("yuv_matrix") == CFGS[-1][0] and s.get_stat("yuv_range") == CFGS[-1][1]
    assert not any(np.array_equal(seen[i], seen[j]) for i in range(len(seen)) for j in range(i))  # every matrix and range is a different image


# ---- 2. output tie -----------------------------------------------------------------------------------------------------------------
CASES = [(tta, precise, os_) for tta in (False, True) for precise in (0, 1) for os_ in (4, 2, 1)]


@pytest.mark.parametrize("case", range(len(CASES)), ids=["%s-%s-x%d" % ("tta" if t else "plain", "precise" if p else "fp16", o) for t, p, o in CASES])
def test_output_tie(ctx, case):
    tta, precise, os_ = CASES[case]
    s = ctx[tta]
    s.set_option("precise", precise)
    s.out_scale = os_
    for src in (U8, F16):
        x = rgb_image(20 + case + src, src)
        d = run(s, x, src, F32)
        assert d.shape == (3, H * os_, W * os_) and np.isfinite(d).all() and len(np.unique(d)) > 16
        for fmt in (NV12, P010):
            for cfg in (CFGS[case % 6], CFGS[(case + 3) % 6], CFGS[(case + 1 + (src == F16)) % 6]):
                set_cfg(s, cfg)
                want = yuv_ref.join(*yuv_ref.encode(d, cfg[0], cfg[1], BITS[fmt]), BITS[fmt])
                assert len(np.unique(want)) > 16  # an image, not a constant
                assert same_bits(run(s, x, src, fmt), want), (src, fmt, cfg)


def test_output_tie_every_matrix_and_range(ctx):
    s = ctx[False]
    x = rgb_image(40, U8)
    d = run(s, x, U8, F32)
    for fmt in (NV12, P010):
        outs = []
        for cfg in CFGS:
            set_cfg(s, cfg)
            outs.append(run(s, x, U8, fmt))
            assert same_bits(outs[-1], yuv_ref.join(*yuv_ref.encode(d, cfg[0], cfg[1], BITS[fmt]), BITS[fmt])), (fmt, cfg)
        assert not any(np.array_equal(outs[i], outs[j]) for i in range(6) for j in range(i))


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_odd_tiles(ctx, tta):
    """An odd tile size: at out_scale 4 and 2 every tile still starts on an even output pixel -- same codes as any other tiling of the
    image --; at out_scale 1 a 2 x 2 chroma quad would cross a tile, and the call is refused before anything is launched."""
    s = ctx[tta]
    x = rgb_image(50, U8)
    for os_ in (4, 2):
        s.out_scale = os_
        s.tilesize = 15
        d = run(s, x, U8, F32)
        for fmt in (NV12, P010):
            assert same_bits(run(s, x, U8, fmt), yuv_ref.join(*yuv_ref.encode(d, 709, 0, BITS[fmt]), BITS[fmt])), (os_, fmt)
    s.out_scale = 1
    for fmt in (NV12, P010):
        with pytest.raises(R.RealSRError) as e:
            run(s, x, U8, fmt)
        assert e.value.code == R.RSR_E_ARG
    s.tilesize = 16
    assert run(s, x, U8, NV12).shape == (H * 3 // 2, W)  # (the context is as usable as before)
    odd = rgb_image(51, U8, 35, 26)                       # an odd width at out_scale 1: no 4:2:0 surface of that size
    buf = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    with pytest.raises(R.RealSRError) as e:
        s.process_device_fmt(buf.data_ptr(), U8, 35, 26, 3, buf.data_ptr() + 4096, NV12)
    assert e.value.code == R.RSR_E_ARG
    s.out_scale = 2                                       # ... at x2 there is
    d = run(s, odd, U8, F32, 35, 26)
    assert same_bits(run(s, odd, U8, NV12, 35, 26), yuv_ref.join(*yuv_ref.encode(d, 709, 0, 8), 8))


# ---- 3. end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [NV12, P010], ids=["nv12", "p010"])
@pytest.mark.parametrize("tta,precise,os_", [(False, 0, 4), (True, 0, 2), (False, 1, 1), (True, 1, 4)], ids=["plain-x4", "tta-x2", "precise-x1", "tta-precise-x4"])
def test_end_to_end_is_the_composition(ctx, tta, precise, os_, fmt):
    s = ctx[tta]
    s.set_option("precise", precise)
    s.out_scale = os_
    cfg = CFGS[(os_ + fmt) % 6]
    set_cfg(s, cfg)
    surf = surface(60 + fmt, fmt)
    d = run(s, yuv_ref.decode(*yuv_ref.split(surf, BITS[fmt]), cfg[0], cfg[1], BITS[fmt]), F32, F32)
    want = yuv_ref.join(*yuv_ref.encode(d, cfg[0], cfg[1], BITS[fmt]), BITS[fmt])
    assert same_bits(run(s, surf, fmt, fmt), want)
    # the two sides are independent: the other depth out of the same surface
    other = P010 if fmt == NV12 else NV12
    assert same_bits(run(s, surf, fmt, other), yuv_ref.join(*yuv_ref.encode(d, cfg[0], cfg[1], BITS[other]), BITS[other]))


# ---- 4. batches, pitches, windows, torch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [NV12, P010], ids=["nv12", "p010"])
@pytest.mark.parametrize("tta,os_", [(False, 4), (True, 2), (False, 1)], ids=["plain-x4", "tta-x2", "plain-x1"])
def test_batch_of_three_pitched_windows(ctx, tta, os_, fmt):
    """Three surfaces in ONE rsr_process_device_batch call, each inside a larger allocation (row pitch > w, UV plane farther than
    h * pitch behind Y, NV12 at odd addresses), each into a window of a sentinel-filled canvas: every window holds what the lone call
    gives, every other byte of the canvases its sentinel."""
    s = ctx[tta]
    s.out_scale = os_
    es = NP[fmt]().itemsize
    surfs = [surface(70 + i, fmt) for i in range(3)]
    lone = [run(s, x, fmt, fmt) for x in surfs]
    ipitch, iplane, ioff = (W + 5) * es, (H + 3) * (W + 5) * es, 3 * es
    opitch, oplane, ooff = (W * os_ + 7) * es, (H * os_ + 2) * (W * os_ + 7) * es + 6 * es, 5 * es
    ispan, ospan = R.image_span(fmt, W, H, 3, ipitch, iplane), R.image_span(fmt, W * os_, H * os_, 3, opitch, oplane)
    ins, outs, keep = [], [], []
    for x in surfs:
        canvas = np.full(ioff + ispan + 64, 0x5A, dtype=np.uint8)
        place(canvas, ioff, ipitch, iplane, x, fmt)
        d_in = torch.from_numpy(canvas).cuda()
        d_out = torch.full((ooff + ospan + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        keep.append((d_in, d_out))
        ins.append((d_in.data_ptr() + ioff, ipitch, iplane))
        outs.append((d_out.data_ptr() + ooff, opitch, oplane))
    calls = s.get_stat("batch_calls")
    s.process_device_batch(ins, fmt, W, H, 3, outs, fmt)
    torch.cuda.synchronize()
    assert s.get_stat("batch_calls") == calls + 1
    for (_, d_out), want in zip(keep, lone):
        got = d_out.cpu().numpy()
        assert same_bits(lift(got, ooff, opitch, oplane, fmt, W * os_, H * os_), want)
        inside = place(np.zeros_like(got), ooff, opitch, oplane, want, fmt)
        assert (got[~inside] == SENTINEL).all()  # no byte outside the Y and UV windows is touched
        assert inside.sum() == want.nbytes


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16], ids=["nv12", "p010"])
def test_torch_upscale_yuv(ctx, dtype):
    s = ctx[False]
    s.out_scale = 2
    fmt = NV12 if dtype == torch.uint8 else P010
    surf = surface(80, fmt)
    want = run(s, surf, fmt, fmt)
    as_t = lambda a: torch.from_numpy(a.view(np.int16) if fmt == P010 else a).cuda()  # noqa: E731
    back = lambda t: t.cpu().numpy().view(NP[fmt])  # noqa: E731
    x = as_t(surf)
    y = torch_io.upscale_yuv(s, x)
    torch.cuda.synchronize()
    assert y.dtype == dtype and tuple(y.shape) == (H * 3, W * 2) and same_bits(back(y), want)
    # a (y, uv) pair of views into a padded decoder surface, written into a pair of views of a canvas
    big = torch.zeros(H * 3 // 2 + 9, W + 12, dtype=dtype, device="cuda")
    big[4:4 + H, 2:2 + W], big[H + 7:H + 7 + H // 2, 2:2 + W] = x[:H], x[H:]
    canvas = torch.full((H * 3 + 8, W * 2 + 6), 0x4D4D if fmt == P010 else 0x4D, dtype=dtype, device="cuda")
    oy, ouv = canvas[1:1 + 2 * H, 4:4 + 2 * W], canvas[2 * H + 5:3 * H + 5, 4:4 + 2 * W]
    got = torch_io.upscale_yuv(s, (big[4:4 + H, 2:2 + W], big[H + 7:H + 7 + H // 2, 2:2 + W]), out=(oy, ouv))
    torch.cuda.synchronize()
    assert got[0] is oy and got[1] is ouv
    assert same_bits(back(torch.cat([oy, ouv]).contiguous()), want)
    untouched = torch.ones_like(canvas, dtype=torch.bool)
    untouched[1:1 + 2 * H, 4:4 + 2 * W] = False
    untouched[2 * H + 5:3 * H + 5, 4:4 + 2 * W] = False
    assert (canvas[untouched] == (0x4D4D if fmt == P010 else 0x4D)).all()
    # a uv plane that lies BELOW y in memory: packed into one allocation first, same result
    pool = torch.zeros(2 * H * W, dtype=dtype, device="cuda")
    uv_lo, y_hi = pool[:H // 2 * W].view(H // 2, W), pool[H * W:2 * H * W].view(H, W)
    uv_lo.copy_(x[H:])
    y_hi.copy_(x[:H])
    ry, ruv = torch_io.upscale_yuv(s, (y_hi, uv_lo))
    torch.cuda.synchronize()
    assert same_bits(back(torch.cat([ry, ruv]).contiguous()), want)


# ---- argument errors and options that need a context -------------------------------------------------------------------------------
def test_refusals_and_option_validation(ctx):
    s = ctx[False]
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()

    def refused(*a, batch=False):
        with pytest.raises(R.RealSRError) as e:
            (s.process_device_batch if batch else s.process_device_fmt)(*a)
        assert e.value.code == R.RSR_E_ARG, a

    for fmt in (NV12, P010):
        refused(p, fmt, 8, 8, 4, p + 4096, U8)          # c != 3
        refused(p, U8, 8, 8, 4, p + 4096, fmt)
        for w, h in ((7, 8), (8, 7)):                    # an odd w or h of a YUV input
            refused(p, fmt, w, h, 3, p + 4096, F16)
            refused([p], fmt, w, h, 3, [p + 4096], F16, batch=True)
    refused(p + 1, P010, 8, 8, 3, p + 4096, F16)         # P010: an odd data pointer, an odd pitch -- on either side
    refused(p, F16, 8, 8, 3, p + 4097, P010)
    refused([(p + 1, 0, 0)], P010, 8, 8, 3, [p + 4096], F16, batch=True)
    refused([(p, 17, 0)], P010, 8, 8, 3, [p + 4096], F16, batch=True)
    refused([(p, 0, 8 * 16 + 1)], P010, 8, 8, 3, [p + 4096], F16, batch=True)
    refused([p], F16, 8, 8, 3, [(p + 4096, 65, 0)], P010, batch=True)
    for fmt in (3, 7):                                   # ids 3 and 7 stay unknown
        refused(p, fmt, 8, 8, 3, p + 4096, U8)
        refused(p, U8, 8, 8, 3, p + 4096, fmt)
    torch.cuda.synchronize()
    assert (buf == 0).all()                              # nothing was launched
    for key, good, bad in (("yuv_matrix", 2020, (0, 1, 708, 470, -709)), ("yuv_range", 1, (2, -1, 16))):
        s.set_option(key, good)
        for v in bad:
            with pytest.raises(R.RealSRError) as e:
                s.set_option(key, v)
            assert e.value.code == R.RSR_E_ARG and s.get_stat(key) == good  # the value in force stays


def test_bgr_concerns_rgb_sides_only(ctx):
    s = ctx[False]
    surf = surface(90, NV12)
    plain = run(s, surf, NV12, NV12), run(s, surf, NV12, U8)
    s.set_option("bgr", 1)
    assert same_bits(run(s, surf, NV12, NV12), plain[0])
    assert same_bits(run(s, surf, NV12, U8), np.ascontiguousarray(plain[1][:, :, ::-1]))


# ---- 5. the default path stays what it was -----------------------------------------------------------------------------------------
def test_default_path_guard(ctx, paths):
    """After YUV calls of every kind on a context, a uint8 call gives the bytes and makes the launches a fresh context does: conv_last
    writes the image itself (351 conv launches, no post-processing launch), the pre-processing accounts the same bytes."""
    img = rgb_image(100, U8)

    def profiled_u8(s):
        s.tilesize, s.prepadding = T, 10
        s.set_option("merge", 1)
        s.set_profiling(True)
        try:
            s.get_profile(reset=True)
            out = run(s, img, U8, U8)
            return out, s.get_profile(reset=True)
        finally:
            s.set_profiling(False)
            s.set_option("merge", 16)

    fresh = R.RealSR(0)
    try:
        fresh.load(*paths)
        want, p0 = profiled_u8(fresh)
    finally:
        fresh.close()
    s = ctx[False]
    for os_ in (4, 1):
        s.out_scale = os_
        for fmt in (NV12, P010):
            set_cfg(s, CFGS[1 + os_ % 2])
            run(s, surface(101, fmt), fmt, fmt)
            run(s, img, U8, fmt)
    s.out_scale = 4
    got, p1 = profiled_u8(s)
    assert same_bits(got, want)
    assert p0["conv_launches"] == R.NUM_CONVS and p0["post_ms"] == 0 and p0["post_bytes"] == 0 and p0["calls"] == 1
    for key in ("conv_launches", "post_ms", "post_bytes", "pre_bytes", "tiles", "calls", "conv_flops"):
        assert p1[key] == p0[key], key
    assert p1["pre_ms"] > 0
    # a YUV output at out_scale 4 takes the route RGBA, TTA and out_scale < 4 take: the same conv launches and ONE post-processing launch,
    # whose bytes follow the format (per x4 pixel: 6 of the blob read; 3 of a uint8 pixel or 1.5 of NV12 written)
    s.set_option("merge", 1)
    s.set_profiling(True)
    try:
        s.get_profile(reset=True)
        run(s, img, U8, NV12)
        p2 = s.get_profile(reset=True)
        s.set_option("dbg", 8192)
        run(s, img, U8, U8)
        p3 = s.get_profile(reset=True)
    finally:
        s.set_option("dbg", 0)
        s.set_profiling(False)
        s.set_option("merge", 16)
    assert p2["conv_launches"] == p0["conv_launches"] and p2["post_ms"] > 0 and p3["post_ms"] > 0
    assert p2["post_bytes"] == pytest.approx(p3["post_bytes"] * (6 + 1.5) / (6 + 3))
