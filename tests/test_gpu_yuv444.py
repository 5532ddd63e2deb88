"""YUV444P / YUV444P10 device images on the GPU (run with -m gpu): RSR_FMT_YUV444P / RSR_FMT_YUV444P10 -- planar YUV 4:4:4, three full
planes, the 10-bit code in the LOW bits of its word -- on either side of every device entry point that takes NV16 / P210, and torch_io's
chroma=444.

Everything here is EXACT, no tolerance anywhere: np.array_equal on bytes against tests/yuv444_ref.py, the numpy float32 restatement of
"YUV 4:4:4" in include/realsr_hip.h, tied to the planar fp32 format of the same context as tests/test_gpu_yuv422.py ties NV16 / P210:

    input side    yuv -> f32  ==  f32 -> f32 with x = yuv444_ref.decode(image)
    output side   x -> yuv    ==  yuv444_ref.encode(x -> f32)
    end to end    yuv -> yuv  ==  yuv444_ref.encode(f32 -> f32 with x = yuv444_ref.decode(image))

Destinations are pre-filled with 0xCD.  The baseline image is 35 x 25 at tile 16, prepadding 10: 3 x 2 tiles, partial tiles on both
edges, an odd width AND an odd height -- which no other YUV format admits."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

import tile_diff_ref as ref
import yuv422_ref
import yuv444_ref
import yuv_ref
from gpu_support import context_fixtures, dev, paths, run  # noqa: F401
from pixfmt_ref import BITS, F16, F32, NP, NV12, NV16, U8, YUV444P, YUV444P10, image, image_at, lift, paste, place, same_bits

pytestmark = pytest.mark.gpu
Y444, Y444_10 = YUV444P, YUV444P10
W, H, T, P = 35, 25, 16, 10
CFGS = [(709, 0), (601, 1), (2020, 0), (709, 1), (601, 0), (2020, 1)]  # (yuv_matrix, yuv_range)
SENTINEL = 0xCD
ONE_PIXEL, TWO_PIXELS = 32768, 65536  # option "dbg": the 4:4:4 post kernels make one pixel / two neighbouring pixels per thread everywhere
ctxs, ctx = context_fixtures(T, P)
image444 = rgb_image = image_at(W, H)
semi_surface = image


def set_cfg(s, cfg):
    s.set_option("yuv_matrix", cfg[0])
    s.set_option("yuv_range", cfg[1])


def want444(d, fmt, cfg=(709, 0)):
    return yuv444_ref.join(*yuv444_ref.encode(d, cfg[0], cfg[1], BITS[fmt]), BITS[fmt])


def decode444(img, fmt, cfg=(709, 0)):
    return yuv444_ref.decode(*yuv444_ref.split(img, BITS[fmt]), cfg[0], cfg[1], BITS[fmt])


# ---- 1. input tie ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [Y444, Y444_10], ids=["yuv444p", "yuv444p10"])
@pytest.mark.parametrize("mode", ["default", "tta", "precise"])
def test_input_tie(ctx, mode, fmt):
    s = ctx[mode == "tta"]
    s.set_option("precise", int(mode == "precise"))
    img = image444(11 + fmt, fmt)
    case = ["default", "tta", "precise"].index(mode) + (3 if fmt == Y444_10 else 0)
    seen = []
    for cfg in (CFGS[case], CFGS[(case + 1) % 6], CFGS[(case + 3) % 6]):  # all six configurations, spread over the six cases
        set_cfg(s, cfg)
        ref = decode444(img, fmt, cfg)
        assert (ref == 0).any() and (ref == 1).any() and len(np.unique(ref)) > 100  # the clamp acts, and not everywhere
        got = run(s, img, fmt, F32)
        assert got.shape == (3, 4 * H, 4 * W) and not (got.view(np.uint8) == SENTINEL).all()
        assert same_bits(got, run(s, ref, F32, F32)), cfg
        seen.append(got)
    assert not any(np.array_equal(seen[i], seen[j]) for i in range(len(seen)) for j in range(i))  # every matrix and range is a different image
    if fmt == Y444_10:  # whatever a producer left above bit 9 is no part of the sample
        rng = np.random.default_rng(5)
        dirty = img | (rng.integers(0, 64, size=img.shape) * (rng.uniform(size=img.shape) < 0.3) << 10).astype(np.uint16)
        assert (dirty != img).sum() > 100 and same_bits(run(s, dirty, fmt, F32), seen[-1])


# ---- 2. output tie -----------------------------------------------------------------------------------------------------------------
CASES = [(tta, precise, os_) for tta in (False, True) for precise in (0, 1) for os_ in (4, 2, 1)]


def check_outputs(s, x, src, w, h, d, salt):
    """x -> YUV444P and x -> YUV444P10 against the encode of d = x -> F32, at a configuration each; with the default thread shape (two pixels
    per thread at out_scale 4, one elsewhere) and with either shape forced."""
    for fmt in (Y444, Y444_10):
        cfg = CFGS[(salt + fmt + src) % 6]
        set_cfg(s, cfg)
        want = want444(d, fmt, cfg)
        assert want.shape == d.shape and len(np.unique(want)) > 16 and want.max() < (1 << BITS[fmt])  # an image; the high six bits are 0
        got = run(s, x, src, fmt, w, h)
        assert same_bits(got, want), (src, fmt, cfg)
        for dbg in (ONE_PIXEL, TWO_PIXELS):
            s.set_option("dbg", dbg)
            got2 = run(s, x, src, fmt, w, h)
            s.set_option("dbg", 0)
            assert same_bits(got2, want), (src, fmt, cfg, dbg)


@pytest.mark.parametrize("case", range(len(CASES)), ids=["%s-%s-x%d" % ("tta" if t else "plain", "precise" if p else "fp16", o) for t, p, o in CASES])
def test_output_tie(ctx, case):
    """out_scale 4 / 2 / 1 at tile 16: 35 x 25 gives 140 x 100, 70 x 50 and 35 x 25 -- odd on both axes, tile rectangles of 16 and a
    last column of tiles 3 pixels wide."""
    tta, precise, os_ = CASES[case]
    s = ctx[tta]
    s.set_option("precise", precise)
    s.out_scale = os_
    for src in (U8, F16):
        x = rgb_image(20 + case + src, src)
        d = run(s, x, src, F32)
        assert d.shape == (3, H * os_, W * os_) and np.isfinite(d).all() and len(np.unique(d)) > 16
        check_outputs(s, x, src, W, H, d, case)


@pytest.mark.parametrize("tta,precise", [(False, 0), (True, 0), (False, 1)], ids=["plain", "tta", "precise"])
def test_output_tie_at_3_2(ctx, tta, precise):
    """38 x 26 at 3/2 and tile 16: 57 x 39 -- odd on both axes; tile rectangles of 24 x 24, the last ones 9 columns / 15 rows.  Neither NV12
    nor NV16 takes it."""
    s = ctx[tta]
    s.set_option("precise", precise)
    s.out_ratio = Fraction(3, 2)
    assert s.out_size_fmt(Y444, 38, 26) == (57, 39) == s.out_size_fmt(F32, 38, 26)
    for fmt in (NV12, NV16):
        with pytest.raises(ValueError, match="YUV"):
            s.out_size_fmt(fmt, 38, 26)
    x = rgb_image(300 + tta, U8, 38, 26)
    d = run(s, x, U8, F32, 38, 26)
    assert d.shape == (3, 39, 57)
    check_outputs(s, x, U8, 38, 26, d, tta + precise)


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_output_tie_at_a_pair(ctx, tta):
    """(8/3, 9/4) at tile 24: 45 x 28 gives 120 x 63, tile rectangles 64 x 54; and the pair swapped, 28 x 45 to 63 x 120 -- an odd width
    with 5-tap footprints along the rows."""
    s = ctx[tta]
    s.tilesize = 24
    for pair, w, h, ow, oh in (((Fraction(8, 3), Fraction(9, 4)), 45, 28, 120, 63), ((Fraction(9, 4), Fraction(8, 3)), 28, 45, 63, 120)):
        s.out_ratio_xy = pair
        assert s.out_size_fmt(Y444_10, w, h) == (ow, oh)
        x = rgb_image(310 + w, F16, w, h)
        d = run(s, x, F16, F32, w, h)
        assert d.shape == (3, oh, ow)
        check_outputs(s, x, F16, w, h, d, w)


# ---- 3. end to end, cross-format, siting -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tta,precise,os_", [(False, 0, 4), (True, 0, 2), (False, 1, 1)], ids=["plain-x4", "tta-x2", "precise-x1"])
def test_end_to_end_and_cross_format(ctx, tta, precise, os_):
    s = ctx[tta]
    s.set_option("precise", precise)
    s.out_scale = os_
    cfg = CFGS[os_ % 6]
    set_cfg(s, cfg)
    for fmt in (Y444, Y444_10):
        img = image444(60 + fmt, fmt)
        d = run(s, decode444(img, fmt, cfg), F32, F32)
        assert same_bits(run(s, img, fmt, fmt), want444(d, fmt, cfg)), fmt
    # the two sides are independent: 8 -> 10 bits ...
    img = image444(64, Y444)
    d = run(s, decode444(img, Y444, cfg), F32, F32)
    assert same_bits(run(s, img, Y444, Y444_10), want444(d, Y444_10, cfg))
    # ... NV12 in (an even size: 36 x 26), 4:4:4 out ...
    surf = semi_surface(70, NV12, 36, 26)
    d = run(s, yuv_ref.decode(*yuv_ref.split(surf, 8), cfg[0], cfg[1], 8), F32, F32, 36, 26)
    assert same_bits(run(s, surf, NV12, Y444, 36, 26), want444(d, Y444, cfg))
    # ... 4:4:4 in, NV16 out (an even width, any height: 36 x 25) ...
    img = image444(71, Y444_10, 36, 25)
    d = run(s, decode444(img, Y444_10, cfg), F32, F32, 36, 25)
    assert same_bits(run(s, img, Y444_10, NV16, 36, 25), yuv422_ref.join(*yuv422_ref.encode(d, cfg[0], cfg[1], 8, 0, T * os_), 8))
    # ... and uint8 RGB in
    x = rgb_image(72, U8)
    assert same_bits(run(s, x, U8, Y444), want444(run(s, x, U8, F32), Y444, cfg))


def test_yuv_siting_means_nothing(ctx):
    s = ctx[False]
    for fmt in (Y444, Y444_10):
        img, x = image444(80 + fmt, fmt), rgb_image(81 + fmt, F16)
        ins, outs = [], []
        for siting in (0, 1, 2):
            s.yuv_siting = siting
            ins.append(run(s, img, fmt, F32))
            outs.append(run(s, x, F16, fmt))
        assert same_bits(ins[0], ins[1]) and same_bits(ins[0], ins[2]) and same_bits(outs[0], outs[1]) and same_bits(outs[0], outs[2])


# ---- 4. batches, masks, sequences -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [Y444, Y444_10], ids=["yuv444p", "yuv444p10"])
@pytest.mark.parametrize("tta,os_", [(False, 4), (True, 2), (False, 1)], ids=["plain-x4", "tta-x2", "plain-x1"])
def test_batch_of_three_pitched_windows(ctx, tta, os_, fmt):
    """Three images in ONE rsr_process_device_batch call, each inside a larger allocation (row pitch > w, planes farther apart than
    h * pitch; YUV444P at odd addresses and odd pitches), each into a window of a sentinel-filled canvas: every window holds what the lone
    call gives, every other byte of the canvases its sentinel."""
    s = ctx[tta]
    s.out_scale = os_
    es = NP[fmt]().itemsize
    imgs = [image444(70 + i, fmt) for i in range(3)]
    lone = [run(s, x, fmt, fmt) for x in imgs]
    ipitch, iplane, ioff = (W + 6) * es, (H + 3) * (W + 6) * es + es, 3 * es          # uint8: pitch 41, plane 1149, offset 3
    opitch, oplane, ooff = (W * os_ + 8) * es, (H * os_ + 2) * (W * os_ + 8) * es + 7 * es, 5 * es
    assert es == 2 or (ipitch % 2 and iplane % 2 and ioff % 2 and ooff % 2)
    ispan, ospan = R.image_span(fmt, W, H, 3, ipitch, iplane), R.image_span(fmt, W * os_, H * os_, 3, opitch, oplane)
    assert ospan == 2 * oplane + (H * os_ - 1) * opitch + W * os_ * es
    ins, outs, keep = [], [], []
    for x in imgs:
        canvas = np.full(ioff + ispan + 64, 0x5A, dtype=np.uint8)
        place(canvas, ioff, ipitch, iplane, x, fmt)
        d_in = torch.from_numpy(canvas).cuda()
        d_out = torch.full((ooff + ospan + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        keep.append((d_in, d_out))
        ins.append((d_in.data_ptr() + ioff, ipitch, iplane))
        outs.append((d_out.data_ptr() + ooff, opitch, oplane))
    for dbg in (0, ONE_PIXEL, TWO_PIXELS):  # (an odd window address: the pair store of the two-pixel shape falls back to sample stores)
        s.set_option("dbg", dbg)
        for _, d_out in keep:
            d_out.fill_(SENTINEL)
        calls = s.get_stat("batch_calls")
        s.process_device_batch(ins, fmt, W, H, 3, outs, fmt)
        torch.cuda.synchronize()
        assert s.get_stat("batch_calls") == calls + 1
        for (_, d_out), want in zip(keep, lone):
            got = d_out.cpu().numpy()
            assert same_bits(lift(got, ooff, opitch, oplane, fmt, W * os_, H * os_), want)
            inside = place(np.zeros_like(got), ooff, opitch, oplane, want, fmt)
            assert (got[~inside] == SENTINEL).all()  # no byte outside the three windows is touched
            assert inside.sum() == want.nbytes


@pytest.mark.parametrize("fmt,ratio", [(Y444, None), (Y444_10, Fraction(3, 2))], ids=["yuv444p-x4", "yuv444p10-x3_2"])
def test_masked_tiles(ctx, fmt, ratio):
    """A partial mask: the marked tiles' rectangles hold the full call's bytes, the unmarked ones the sentinel -- in all three planes."""
    s = ctx[False]
    w, h = (W, H) if ratio is None else (38, 26)
    r = Fraction(4) if ratio is None else ratio
    if ratio is not None:
        s.out_ratio = ratio
    img = image444(90 + fmt, fmt, w, h)
    full = run(s, img, fmt, fmt, w, h)
    nx, ny = s.tile_count(w, h)
    assert (nx, ny) == (3, 2)
    mask = np.array([1, 0, 1, 0, 1, 0], dtype=np.uint8)
    d_in, d_out = dev(img), torch.full((full.nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    s.process_device_masked(d_in.data_ptr(), fmt, w, h, 3, d_out.data_ptr(), fmt, mask)
    torch.cuda.synchronize()
    want = np.full(full.shape, SENTINEL | (SENTINEL << 8) if BITS[fmt] == 10 else SENTINEL, dtype=NP[fmt])
    for t in np.flatnonzero(mask):
        paste(fmt, want, full, ref.out_rect(w, h, T, t, r.numerator, r.denominator))
    got = d_out.cpu().numpy().view(NP[fmt]).reshape(full.shape)
    assert same_bits(got, want) and not same_bits(got, full)


@pytest.mark.parametrize("fmt", [Y444, Y444_10], ids=["yuv444p", "yuv444p10"])
def test_sequence_of_three_frames_with_prev_out(ctx, fmt):
    """Three frames and a previous output: a rectangle nobody computed is copied from the frame that computed it last or from prev_out,
    in each of the three planes (35 x 25: rectangles 64, 64 and 12 columns wide, 64 and 36 rows high)."""
    s = ctx[False]
    frames = [image444(100 + i + fmt, fmt) for i in range(3)]
    full = [run(s, x, fmt, fmt) for x in frames]
    prev = image444(110, fmt, 4 * W, 4 * H)
    masks = np.array([[1, 0, 0, 0, 1, 0],
                      [0, 1, 0, 0, 0, 0],
                      [0, 0, 0, 1, 1, 0]], dtype=np.uint8)
    d_ins = [dev(x) for x in frames]
    d_outs = [torch.full((full[0].nbytes,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in frames]
    d_prev = dev(prev)
    s.process_device_sequence([t.data_ptr() for t in d_ins], fmt, W, H, 3, [t.data_ptr() for t in d_outs], fmt, masks.reshape(-1), prev_out=d_prev.data_ptr())
    torch.cuda.synchronize()
    state = prev.copy()
    for k in range(3):
        for t in np.flatnonzero(masks[k]):
            paste(fmt, state, full[k], ref.out_rect(W, H, T, t))
        got = d_outs[k].cpu().numpy().view(NP[fmt]).reshape(full[k].shape)
        assert same_bits(got, state), k
    assert same_bits(d_prev.cpu().numpy().view(NP[fmt]).reshape(prev.shape), prev)


# ---- 5. the frame diff -------------------------------------------------------------------------------------------------------------
def pokes(w, h):
    """(plane, row, column) of single samples to change: in each plane, just inside and just outside the source rectangles of tiles 0 and 4."""
    out = []
    for q in range(3):
        x0, y0, x1, y1 = ref.source_rect(w, h, T, P, 0)   # (0, 0, 26, 25): the right edge is inside the image
        assert (x0, y0, x1, y1) == (0, 0, 26, 25)
        out += [(q, y1 - 1, x1 - 1), (q, y1 - 1, x1), (q, 0, 0)]
        x0, y0, x1, y1 = ref.source_rect(w, h, T, P, 4)   # (6, 6, 35, 25): the left and the upper edge are
        assert (x0, y0, x1, y1) == (6, 6, 35, 25)
        out += [(q, y0, x0), (q, y0 - 1, x0), (q, y0, x0 - 1), (q, y1 - 1, x1 - 1)]
    return out


@pytest.mark.parametrize("fmt", [Y444, Y444_10], ids=["yuv444p", "yuv444p10"])
def test_diff_tiles_and_sequence(ctx, fmt):
    s = ctx[False]
    a = image444(120 + fmt, fmt)
    d_a = dev(a)
    nt = 6
    seen = set()
    pos = pokes(W, H)
    for i, at in enumerate(pos):
        b = a.copy()
        b[at] ^= 1 if (BITS[fmt] == 8 or i % 2) else 0x800  # (YUV444P10: a bit above the code differs as well -- whole words are compared)
        want = ref.diff_mask(fmt, a, b, T, P)
        d_mask = torch.full((nt,), SENTINEL, dtype=torch.uint8, device="cuda")
        s.diff_tiles(d_a.data_ptr(), dev(b).data_ptr(), fmt, W, H, 3, d_mask.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_mask.cpu().numpy(), want), (at, want)
        seen.add(tuple(want))
    assert len(seen) >= 4 and any(sum(m) == 1 for m in seen) and any(sum(m) > 1 for m in seen)
    # pitched images with far-apart planes give the same masks
    b = a.copy()
    b[pos[4]] ^= 1
    es = NP[fmt]().itemsize
    pitch, plane = (W + 7) * es, (H + 2) * (W + 7) * es + 10
    ca, cb = (np.full(R.image_span(fmt, W, H, 3, pitch, plane) + 8, 0x11 * (k + 1), dtype=np.uint8) for k in range(2))
    place(ca, 2 * es, pitch, plane, a, fmt), place(cb, 4 * es, pitch, plane, b, fmt)
    da, db = torch.from_numpy(ca).cuda(), torch.from_numpy(cb).cuda()
    d_mask = torch.full((nt,), SENTINEL, dtype=torch.uint8, device="cuda")
    s.diff_tiles((da.data_ptr() + 2 * es, pitch, plane), (db.data_ptr() + 4 * es, pitch, plane), fmt, W, H, 3, d_mask.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_mask.cpu().numpy(), ref.diff_mask(fmt, a, b, T, P))
    # the sequence form: row k is the diff of the pair (frame k - 1, frame k), row 0 against prev; without a prev every tile of row 0 is set
    frames = [a.copy() for _ in range(3)]
    frames[1][pos[1]] ^= 1
    frames[2][pos[1]] ^= 1
    frames[2][pos[-1]] ^= 1
    d_f = [dev(x) for x in frames]
    for prev in (a, None):
        d_masks = torch.full((3 * nt,), SENTINEL, dtype=torch.uint8, device="cuda")
        s.diff_tiles_sequence([t.data_ptr() for t in d_f], d_a.data_ptr() if prev is not None else None, fmt, W, H, 3, d_masks.data_ptr())
        torch.cuda.synchronize()
        want = np.stack([ref.diff_mask(fmt, p, q, T, P) for p, q in zip([a] + frames[:2], frames)])
        if prev is None:
            want[0] = 1
        assert np.array_equal(d_masks.cpu().numpy().reshape(3, nt), want)
        assert want[1].any() and want[2].any()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_before_launch(ctx):
    s = ctx[False]
    buf = torch.full((1 << 18,), SENTINEL, dtype=torch.uint8, device="cuda")
    p, q = buf.data_ptr(), buf.data_ptr() + (1 << 17)

    def refused(*a, batch=False):
        with pytest.raises(R.RealSRError) as e:
            (s.process_device_batch if batch else s.process_device_fmt)(*a)
        assert e.value.code == R.RSR_E_ARG, a

    for fmt in (Y444, Y444_10):
        refused(p, fmt, 8, 8, 4, q, U8)                              # c = 4
        refused(p, U8, 8, 8, 4, q, fmt)
        refused([p], fmt, 8, 8, 4, [q], fmt, batch=True)
        es = BITS[fmt] // 8 + (BITS[fmt] % 8 > 0)
        refused([(p, 7 * es, 0)], fmt, 8, 8, 3, [q], F16, batch=True)     # a pitch below a row, on either side
        refused([p], F16, 8, 8, 3, [(q, 31 * es, 0)], fmt, batch=True)
        refused([(p, 0, -8)], fmt, 8, 8, 3, [q], F16, batch=True)
    refused(p + 1, Y444_10, 8, 8, 3, q, F16)                         # YUV444P10: an odd address, an odd pitch -- on either side
    refused(p, F16, 8, 8, 3, q + 1, Y444_10)
    refused([(p + 1, 0, 0)], Y444_10, 8, 8, 3, [q], F16, batch=True)
    refused([(p, 17, 0)], Y444_10, 8, 8, 3, [q], F16, batch=True)
    refused([(p, 0, 8 * 16 + 1)], Y444_10, 8, 8, 3, [q], F16, batch=True)
    refused([p], F16, 8, 8, 3, [(q, 65, 0)], Y444_10, batch=True)
    refused([p], F16, 8, 8, 3, [(q, 0, 32 * 64 + 1)], Y444_10, batch=True)
    s.out_ratio = Fraction(3, 2)                                     # the ratio rule holds as for RGB: 35 * 3 / 2 is no pixel count
    refused(p, U8, 35, 25, 3, q, Y444)
    for bad in (10, 11, 14):                                         # the ids around the new ones stay unknown
        refused(p, bad, 8, 8, 3, q, F16)
        refused(p, F16, 8, 8, 3, q, bad)
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()                                   # nothing was launched
    s.out_scale = 1
    s.tilesize = 33                                                  # out_scale 1 at an odd tile size and an odd image: taken
    assert run(s, image444(130, Y444, 7, 5), Y444, Y444, 7, 5).shape == (3, 5, 7)


# ---- 7. 64-bit addressing: plane 1 beyond 2^31 bytes, plane 2 beyond 2^32 --------------------------------------------------------------
FAR = (1 << 31) + (1 << 20) + 6  # plane pitch of the far images (even: YUV444P10)
ARENA = (1 << 32) + (3 << 27)    # ~ 4.4 GiB, a whole number of 8-byte words


@pytest.fixture(scope="module")
def arena():
    a = torch.full((ARENA,), SENTINEL, dtype=torch.uint8, device="cuda")
    yield a
    del a
    torch.cuda.empty_cache()


def arena_clean(arena):
    words = arena.view(torch.int64)
    fill = int(np.array([SENTINEL] * 8, dtype=np.uint8).view(np.int64)[0])
    return int(words.min()) == fill and int(words.max()) == fill


@pytest.mark.parametrize("fmt", [Y444, Y444_10], ids=["yuv444p", "yuv444p10"])
def test_far_planes_on_either_side(ctx, arena, fmt):
    """The planes FAR apart inside one arena of 0xCD -- U beyond 2^31 bytes, V beyond 2^32: as an input the call gives the packed call's
    bytes; as an output the three windows hold the packed call's bytes and the rest of the arena stays 0xCD (checked on the device)."""
    s = ctx[False]
    es = NP[fmt]().itemsize
    assert ARENA % 8 == 0 and FAR > 2 ** 31 and 2 * FAR > 2 ** 32 and arena_clean(arena)
    # input side
    img = image444(140 + fmt, fmt)
    want = run(s, img, fmt, F32)
    off, pitch = 4096 + 2 * es, (W + 9) * es
    assert R.image_span(fmt, W, H, 3, pitch, FAR) == 2 * FAR + (H - 1) * pitch + W * es < ARENA - off
    rows = torch.from_numpy(img.view(np.uint8).reshape(3, H, -1)).cuda()
    where = [(q, r, off + q * FAR + r * pitch) for q in range(3) for r in range(H)]
    for q, r, o in where:
        arena[o:o + W * es] = rows[q, r]
    d_out = torch.full((want.nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    s.process_device_batch([(arena.data_ptr() + off, pitch, FAR)], fmt, W, H, 3, [d_out.data_ptr()], F32)
    torch.cuda.synchronize()
    assert same_bits(d_out.cpu().numpy().view(np.float32).reshape(want.shape), want)
    for q, r, o in where:
        assert torch.equal(arena[o:o + W * es], rows[q, r])
        arena[o:o + W * es] = SENTINEL
    assert arena_clean(arena)
    # output side
    x = rgb_image(150 + fmt, U8)
    want = run(s, x, U8, fmt)
    ow, oh = 4 * W, 4 * H
    opitch = (ow + 11) * es
    assert R.image_span(fmt, ow, oh, 3, opitch, FAR) < ARENA - off
    s.process_device_batch([dev(x).data_ptr()], U8, W, H, 3, [(arena.data_ptr() + off, opitch, FAR)], fmt)
    torch.cuda.synchronize()
    wrows = torch.from_numpy(want.view(np.uint8).reshape(3, oh, -1)).cuda()
    for q in range(3):
        for r in range(oh):
            o = off + q * FAR + r * opitch
            assert torch.equal(arena[o:o + ow * es], wrows[q, r]), (q, r)
            arena[o:o + ow * es] = SENTINEL
    assert arena_clean(arena)


# ---- 8. torch_io, chroma=444 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16], ids=["yuv444p", "yuv444p10"])
def test_torch_upscale_yuv_444(ctx, dtype):
    s = ctx[False]
    s.out_scale = 2
    fmt = Y444 if dtype == torch.uint8 else Y444_10
    img = image444(160, fmt)
    want = run(s, img, fmt, fmt)
    as_t = lambda a: torch.from_numpy(a.view(np.int16) if fmt == Y444_10 else a).cuda()  # noqa: E731
    back = lambda t: t.cpu().numpy().view(NP[fmt])  # noqa: E731
    x = as_t(img)
    y = torch_io.upscale_yuv(s, x, chroma=444)
    torch.cuda.synchronize()
    assert y.dtype == dtype and tuple(y.shape) == (3, 2 * H, 2 * W) and same_bits(back(y), want)
    # a crop of a larger frame in, a window of a canvas out: no copies, no byte outside the window changes
    big = torch.zeros(3, H + 9, W + 12, dtype=dtype, device="cuda")
    big[:, 4:4 + H, 3:3 + W] = x
    fill = 0x4D4D if fmt == Y444_10 else 0x4D
    canvas = torch.full((3, 2 * H + 8, 2 * W + 7), fill, dtype=dtype, device="cuda")
    win = canvas[:, 1:1 + 2 * H, 5:5 + 2 * W]
    got = torch_io.upscale_yuv(s, big[:, 4:4 + H, 3:3 + W], out=win, chroma=444)
    torch.cuda.synchronize()
    assert got is win and same_bits(back(win.contiguous()), want)
    untouched = torch.ones_like(canvas, dtype=torch.bool)
    untouched[:, 1:1 + 2 * H, 5:5 + 2 * W] = False
    assert (canvas[untouched] == fill).all()


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16], ids=["yuv444p", "yuv444p10"])
def test_torch_delta_and_sequence_444(ctx, dtype):
    """upscale_delta and upscale_sequence with chroma=444 give, frame by frame, the bytes of the lone C-level call."""
    s = ctx[False]
    fmt = Y444 if dtype == torch.uint8 else Y444_10
    as_t = lambda a: torch.from_numpy(a.view(np.int16) if fmt == Y444_10 else a).cuda()  # noqa: E731
    back = lambda t: t.cpu().numpy().view(NP[fmt])  # noqa: E731
    frames = [image444(170, fmt)]
    for at in ((0, 3, 5), (2, 20, 30)):  # frame 1: one Y sample of tile 0; frame 2: one V sample of the last tile row
        f = frames[-1].copy()
        f[at] ^= 0x80
        frames.append(f)
    want = [run(s, f, fmt, fmt) for f in frames]
    xs = [as_t(f) for f in frames]
    y0 = torch_io.upscale_yuv(s, xs[0], chroma=444)
    out, n = torch_io.upscale_delta(s, xs[1], xs[0], y0.clone(), chroma=444)
    torch.cuda.synchronize()
    assert 0 < n < 6 and same_bits(back(out), want[1])
    ys, n = torch_io.upscale_sequence(s, xs, chroma=444)
    torch.cuda.synchronize()
    assert 6 < n < 18 and all(tuple(y.shape) == (3, 4 * H, 4 * W) for y in ys)
    for y, w_ in zip(ys, want):
        assert same_bits(back(y), w_)
    ys, n2 = torch_io.upscale_sequence(s, torch.stack(xs), chroma=444)  # a stacked (N, 3, H, W) tensor
    torch.cuda.synchronize()
    assert n2 == n and tuple(ys.shape) == (3, 3, 4 * H, 4 * W) and all(same_bits(back(ys[k]), want[k]) for k in range(3))
