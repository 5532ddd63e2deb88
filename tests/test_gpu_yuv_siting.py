"""Chroma siting of the NV12 / P010 device images on the GPU (run with -m gpu): option "yuv_siting" 1 (left) and 2 (top-left) on either
side of rsr_process_device_fmt and rsr_process_device_batch.

Everything here is EXACT, no tolerance anywhere, with the ties of tests/test_gpu_yuv.py -- the YUV formats against the planar fp32 format
of the same context -- through tests/yuv_siting_ref.py, the numpy float32 restatement of "Chroma siting, exact" in include/realsr_hip.h:

    input side    yuv -> f32  ==  f32 -> f32 with x = ref.decode(surface, siting)
    output side   x -> yuv    ==  ref.encode(x -> f32, siting, tilesize * out_scale)
    end to end    yuv -> yuv  ==  ref.encode(f32 -> f32 with x = ref.decode(surface, siting), siting, tilesize * out_scale)

The baseline image is 36 x 26 at tile 16, prepadding 10: 3 x 2 tiles, partial tiles on both edges, interior tile edges on both axes -- the
sited chroma filters clamp there -- and, at out_scale 4, 32 quad rows per tile: the row above a quad crosses thread blocks.  Every test
leaves yuv_siting at 0 (the ctx fixture resets it on either side of a test).
"""
import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R

import yuv_ref
import yuv_siting_ref as ref
from gpu_support import context_fixtures, paths, run as run_sized  # noqa: F401
from pixfmt_ref import BITS, F16, F32, NP, NV12, P010, U8, image_at, lift, place, same_bits

pytestmark = pytest.mark.gpu
W, H, T = 36, 26, 16
CFGS = [(709, 0), (601, 1), (2020, 0), (709, 1), (601, 0), (2020, 1)]  # (yuv_matrix, yuv_range)
SENTINEL = 0xCD
ctxs, ctx = context_fixtures(T, 10)
surface = rgb_image = image_at(W, H)


def run(s, x, in_fmt, out_fmt, w=W, h=H):
    """One synchronous rsr_process_device_fmt call on the numpy image x into w x h times out_scale."""
    return run_sized(s, x, in_fmt, out_fmt, w, h, out_size=(w * s.out_scale, h * s.out_scale))


def set_cfg(s, cfg):
    s.set_option("yuv_matrix", cfg[0])
    s.set_option("yuv_range", cfg[1])


def encoded(d, siting, tile_out, cfg, fmt):
    return yuv_ref.join(*ref.encode(d, siting, tile_out, cfg[0], cfg[1], BITS[fmt]), BITS[fmt])


def planes(surf):
    h = surf.shape[0] * 2 // 3
    return surf[:h], surf[h:]


# ---- 1. input tie ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [NV12, P010], ids=["nv12", "p010"])
@pytest.mark.parametrize("mode", ["default", "tta", "precise"])
def test_input_tie(ctx, mode, fmt):
    s = ctx[mode == "tta"]
    s.set_option("precise", int(mode == "precise"))
    cfg = CFGS[(fmt + len(mode)) % 6]
    set_cfg(s, cfg)
    surf = surface(11 + fmt, fmt)
    y, uv = yuv_ref.split(surf, BITS[fmt])
    seen = []
    for siting in (0, 1, 2):
        s.yuv_siting = siting
        assert s.get_stat("yuv_siting") == siting
        got = run(s, surf, fmt, F32)
        assert not (got.view(np.uint8) == SENTINEL).all()
        if siting:
            want = ref.decode(y, uv, siting, cfg[0], cfg[1], BITS[fmt])
            assert (want == 0).any() and (want == 1).any() and len(np.unique(want)) > 100  # the clamp acts, and not everywhere
            assert same_bits(got, run(s, want, F32, F32)), siting
        seen.append(got)
    assert not any(np.array_equal(seen[i], seen[j]) for i in range(3) for j in range(i))  # three sitings, three images


# ---- 2. output tie -----------------------------------------------------------------------------------------------------------------
CASES = [(tta, precise, os_) for tta in (False, True) for precise in (0, 1) for os_ in (4, 2, 1)]


@pytest.mark.parametrize("case", range(len(CASES)), ids=["%s-%s-x%d" % ("tta" if t else "plain", "precise" if p else "fp16", o) for t, p, o in CASES])
def test_output_tie(ctx, case):
    tta, precise, os_ = CASES[case]
    s = ctx[tta]
    s.set_option("precise", precise)
    s.out_scale = os_
    src = (U8, F16)[case % 2]
    x = rgb_image(20 + case, src)
    d = run(s, x, src, F32)
    assert d.shape == (3, H * os_, W * os_) and np.isfinite(d).all() and len(np.unique(d)) > 16
    for fmt in (NV12, P010):
        cfg = CFGS[(case + fmt) % 6]
        set_cfg(s, cfg)
        s.yuv_siting = 0
        y0, uv0 = planes(run(s, x, src, fmt))
        for siting in (1, 2):
            s.yuv_siting = siting
            want = encoded(d, siting, T * os_, cfg, fmt)
            got = run(s, x, src, fmt)
            assert same_bits(got, want), (fmt, siting, cfg)
            assert same_bits(run(s, x, src, F32), d)                                  # the RGB formats are not concerned
            assert np.array_equal(planes(got)[0], y0) and not np.array_equal(planes(got)[1], uv0)  # luma is siting 0's, chroma is not


# ---- 3. tile edges are the definition's --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,os_", [(16, 4), (15, 4), (15, 2)], ids=["t16-x4", "t15-x4", "t15-x2"])
@pytest.mark.parametrize("siting", [1, 2])
def test_tile_edges(ctx, siting, tile, os_):
    """The chroma filter clamps at the first column (siting 2: and row) of every tile's rectangle: the reference with the tile grid
    differs from the one without it there, and only there, and the device gives the gridded one.  Tile 15: the rectangles start at
    multiples of 60 / 30 output pixels, even but no multiple of 4."""
    s = ctx[False]
    s.tilesize, s.out_scale = tile, os_
    x = rgb_image(30 + tile + os_, U8)
    d = run(s, x, U8, F32)
    s.yuv_siting = siting
    for fmt in (NV12, P010):
        grid, free = encoded(d, siting, tile * os_, (709, 0), fmt), encoded(d, siting, 0, (709, 0), fmt)
        assert np.array_equal(planes(grid)[0], planes(free)[0])
        diff = (planes(grid)[1] != planes(free)[1]).reshape(H * os_ // 2, W * os_ // 2, 2).any(axis=-1)
        assert diff.any()                                                    # (else the comparison below would show nothing)
        first = np.zeros_like(diff)
        step = tile * os_ // 2
        first[:, step::step] = True
        if siting == 2:
            first[step::step, :] = True
        assert not (diff & ~first).any()
        got = run(s, x, U8, fmt)
        assert same_bits(got, grid), fmt
        assert not same_bits(got, free)


# ---- 4. a tile wider than one 64-lane group of quads -------------------------------------------------------------------------------
@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
@pytest.mark.parametrize("siting", [1, 2])
def test_wide_tile(ctx, siting, tta):
    """40 x 20 at tilesize 36: at out_scale 4 the first tile has 72 quads per row -- more than the 64 lanes of a wave --, the second is 4
    pixels wide; at out_scale 1 it has 18 quads whose neighbours are 4 x 4 boxes."""
    s = ctx[tta]
    s.tilesize = 36
    x = rgb_image(40 + siting, U8, 40, 20)
    for os_ in (4, 1):
        s.out_scale = os_
        s.yuv_siting = 0
        d = run(s, x, U8, F32, 40, 20)
        s.yuv_siting = siting
        for fmt in (NV12, P010):
            want = encoded(d, siting, 36 * os_, (709, 0), fmt)
            assert not same_bits(want, encoded(d, siting, 0, (709, 0), fmt))  # the second tile's first column
            assert same_bits(run(s, x, U8, fmt, 40, 20), want), (os_, fmt)


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("siting,fmt,tta,os_", [(1, NV12, False, 4), (2, P010, False, 4), (1, NV12, True, 2), (2, P010, False, 1)],
                         ids=["left-nv12-x4", "topleft-p010-x4", "left-nv12-tta-x2", "topleft-p010-x1"])
def test_end_to_end_is_the_composition(ctx, siting, fmt, tta, os_):
    s = ctx[tta]
    s.out_scale = os_
    cfg = CFGS[(os_ + fmt) % 6]
    set_cfg(s, cfg)
    s.yuv_siting = siting
    surf = surface(60 + fmt, fmt)
    d = run(s, ref.decode(*yuv_ref.split(surf, BITS[fmt]), siting, cfg[0], cfg[1], BITS[fmt]), F32, F32)
    got = run(s, surf, fmt, fmt)
    assert same_bits(got, encoded(d, siting, T * os_, cfg, fmt))
    s.yuv_siting = 0
    assert not same_bits(run(s, surf, fmt, fmt), got)


# ---- 6. batches, pitches, windows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [NV12, P010], ids=["nv12", "p010"])
def test_batch_of_three_pitched_windows(ctx, fmt):
    """Three left-sited surfaces in ONE rsr_process_device_batch call, each inside a larger allocation (row pitch > w, UV plane farther
    than h * pitch behind Y, NV12 at odd addresses), each into a window of a sentinel-filled canvas: every window holds what the lone
    call gives, every other byte of the canvases its sentinel."""
    s = ctx[False]
    os_ = 4
    s.yuv_siting = 1
    es = NP[fmt]().itemsize
    surfs = [surface(70 + i, fmt) for i in range(3)]
    lone = [run(s, x, fmt, fmt) for x in surfs]
    s.yuv_siting = 0
    assert not same_bits(run(s, surfs[0], fmt, fmt), lone[0])
    s.yuv_siting = 1
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


# ---- 7. the option -----------------------------------------------------------------------------------------------------------------
def test_option(ctx, paths):
    fresh = R.RealSR(0)
    try:
        assert fresh.yuv_siting == 0 and fresh.get_stat("yuv_siting") == 0  # the default, before and after a model is loaded
        fresh.load(*paths)
        assert fresh.yuv_siting == 0
    finally:
        fresh.close()
    s = ctx[False]
    for good in (1, 2, 0, 2):
        s.set_option("yuv_siting", good)
        assert s.get_stat("yuv_siting") == good and s.yuv_siting == good
        for bad in (3, -1, 709):
            with pytest.raises(R.RealSRError) as e:
                s.set_option("yuv_siting", bad)
            assert e.value.code == R.RSR_E_ARG and s.get_stat("yuv_siting") == good  # the value in force stays
    with pytest.raises(R.RealSRError):
        s.yuv_siting = 5
    assert s.yuv_siting == 2
    # the RGB formats are not concerned: the same bytes with siting 2 in force as at siting 0
    x8, x16 = rgb_image(90, U8), rgb_image(91, F16)
    with2 = run(s, x8, U8, U8), run(s, x16, F16, F32)
    s.yuv_siting = 0
    assert same_bits(run(s, x8, U8, U8), with2[0]) and same_bits(run(s, x16, F16, F32), with2[1])
    # back at siting 0 the surfaces are the centre-sited definition's
    for fmt in (NV12, P010):
        assert same_bits(run(s, x8, U8, fmt), yuv_ref.join(*yuv_ref.encode(run(s, x8, U8, F32), 709, 0, BITS[fmt]), BITS[fmt]))
