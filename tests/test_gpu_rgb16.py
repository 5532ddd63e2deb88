"""RSR_FMT_U16_HWC device images on the GPU (run with -m gpu): 16-bit RGB(A) on either side of every device entry point.

Every comparison is np.array_equal on the samples, against tests/rgb16_ref.py -- the numpy float32 restatement of "16-bit RGB(A)" in
include/realsr_hip.h -- tied to the planar fp32 format of the SAME context, the way the YUV formats are tied:

    input side    u16 -> f32  ==  f32 -> f32 with x = k * fp32(1/65535)
    output side   x -> u16    ==  rgb16_ref.encode(x -> f32)

Alpha is compared with the float32 mirror of kernels.hip alpha_bicubic (rgb16_ref.alpha_x4) reduced as the image is reduced.
Destinations are pre-filled with 0xCD.  The baseline image is 36 x 25 at tile 16, prepadding 10: 3 x 2 tiles, partial tiles on both edges."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import exact_net as N
import realsr_ncnn_vulkan_amd as R
import rgb16_ref as Z
import tile_diff_ref as ref
import yuv_ref
from area_reduce import area_reduce
from gpu_support import context_fixtures, dev, paths, profile_of  # noqa: F401
from pixfmt_ref import F16, F32, NV12, P010, U8, image, same_bits
from realsr_ncnn_vulkan_amd import synth

pytestmark = pytest.mark.gpu
U16 = R.RSR_FMT_U16_HWC
W, H, T, P = 36, 25, 16, 10
SENTINEL = 0xCD
ctxs, ctx = context_fixtures(T, P)


def run(s, x, in_fmt, out_fmt, out_c=None):
    """One synchronous rsr_process_device_fmt call on the packed numpy image x; the result as a packed numpy image.  The destination is
    sized by s.out_size_fmt and pre-filled with 0xCD bytes."""
    w, h = Z.dims_of(in_fmt, x)
    c = Z.channels_of(in_fmt, x)
    assert x.dtype == Z.np_dtype(in_fmt) and x.shape == Z.shape_of(in_fmt, w, h, c) and x.nbytes == R.image_bytes(in_fmt, w, h, c)
    ow, oh = s.out_size_fmt(out_fmt, w, h)
    oshape = Z.shape_of(out_fmt, ow, oh, c)
    d_in, d_out = dev(x), dev(Z.sentinel_bytes(out_fmt, oshape))
    assert d_out.numel() == R.image_bytes(out_fmt, ow, oh, c)
    s.process_device_fmt(d_in.data_ptr(), in_fmt, w, h, c, d_out.data_ptr(), out_fmt)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(Z.np_dtype(out_fmt)).reshape(oshape)


def hwc(planar):
    return np.ascontiguousarray(planar.transpose(1, 2, 0))


# ---- 1. input tie -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "tta", "precise"])
def test_input_tie(ctx, mode):
    """u16 -> f32 is f32 -> f32 of k * fp32(1/65535); the image carries the sign and byte-order traps of a 16-bit word."""
    s = ctx[mode == "tta"]
    s.set_option("precise", int(mode == "precise"))
    img = Z.image16(11, W, H)
    for k in Z.TRAPS:
        assert (img == k).any()
    got = run(s, img, U16, F32)
    assert got.shape == (3, 4 * H, 4 * W) and not (got.view(np.uint8) == SENTINEL).all()
    assert same_bits(got, run(s, Z.as_f32_chw(img), F32, F32))
    # a byte-swapped or sign-extended reading of the words is another image
    assert not same_bits(got, run(s, img.byteswap(), U16, F32))


def test_widened_uint8_is_the_same_network_input(ctx):
    s = ctx[False]
    img8 = image(12, U8, W, H)
    assert same_bits(run(s, Z.widen(img8), U16, F32), run(s, img8, U8, F32))


# ---- 2. output tie ------------------------------------------------------------------------------------------------------------------
def check_output(s, x, in_fmt):
    d = run(s, x, in_fmt, F32)
    assert d.min() >= 0 and d.max() <= 1 and len(np.unique(d)) > 100
    got = run(s, x, in_fmt, U16)
    want = hwc(Z.encode(d))
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    return got


# (dbg 32768 / 65536: one / two pixels per thread of the x4 launch forced -- for uint8 images, the per-pixel / the LDS-staged kernels)
MODES = ["plain", "tta", "dbg8192", "dbg65536", "tta-dbg65536", "precise", "tta-precise", "bgr", "x2", "x1", "tta-x2", "precise-x1", "dbg32768",
         "tta-dbg32768", "bgr-dbg32768", "bgr-dbg65536"]


@pytest.mark.parametrize("mode", MODES)
def test_output_tie(ctx, mode):
    s = ctx[mode.startswith("tta")]
    if "dbg" in mode:
        s.set_option("dbg", int(mode.split("dbg")[1]))
    s.set_option("precise", int("precise" in mode))
    s.set_option("bgr", int("bgr" in mode))
    if "x2" in mode or "x1" in mode:
        s.out_scale = int(mode[-1])
    outs = [check_output(s, Z.image16(20 + MODES.index(mode), W, H, traps=False), U16), check_output(s, image(40, U8, W, H), U8)]
    if mode == "bgr":  # samples 0 and 2 swap on both sides: the image of the swapped input, swapped back
        x = Z.image16(20 + MODES.index(mode), W, H, traps=False)
        s.set_option("bgr", 0)
        assert np.array_equal(run(s, np.ascontiguousarray(x[:, :, ::-1]), U16, U16)[:, :, ::-1], outs[0])
    if "dbg" in mode:  # the forced kernels give the default kernels' bytes
        s.set_option("dbg", 0)
        assert np.array_equal(run(s, image(40, U8, W, H), U8, U16), outs[1])


@pytest.mark.parametrize("tta,precise", [(False, 0), (True, 0), (False, 1)], ids=["plain", "tta", "precise"])
def test_output_tie_at_3_2(ctx, tta, precise):
    """38 x 26 at 3/2 and tile 16: 57 x 39, odd on both axes."""
    s = ctx[tta]
    s.set_option("precise", precise)
    s.out_ratio = Fraction(3, 2)
    assert s.out_size_fmt(U16, 38, 26) == (57, 39)
    assert check_output(s, Z.image16(60, 38, 26), U16).shape == (39, 57, 3)


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_output_tie_at_a_pair(ctx, tta):
    """(8/3, 9/4) at 36 x 24, tile 24: 96 x 54."""
    s = ctx[tta]
    s.tilesize = 24
    s.out_ratio_xy = (Fraction(8, 3), Fraction(9, 4))
    assert s.out_size_fmt(U16, 36, 24) == (96, 54)
    assert check_output(s, Z.image16(61, 36, 24), U16).shape == (54, 96, 3)


# ---- 3. clamping ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exact_ctx(tmp_path_factory):
    """The two-term exact model of tests/exact_net.py: its conv_last reaches both clamps on exact_net.frame_u8 (tests/test_exact_net.py
    asserts that of the numpy mirror, without a GPU: "both clamps")."""
    import os
    d = str(tmp_path_factory.mktemp("rgb16_exact"))
    synth.write_param(os.path.join(d, "x4.param"))
    synth.write_bin(os.path.join(d, "x4.bin"), N.dense_weights(N.make_model()), "fp16")
    s = R.RealSR(0)
    s.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
    yield s
    s.close()


@pytest.mark.parametrize("precise", [0, 1], ids=["fp16", "precise"])
def test_clamped_samples(exact_ctx, precise):
    s = exact_ctx
    w, h, t = N.FRAME
    s.tilesize, s.prepadding = t, 10
    s.set_option("precise", precise)
    try:
        x = Z.widen(N.frame_u8(w, h))
        d = run(s, x, U16, F32)
        assert (d == 0).sum() >= 0.01 * d.size and (d == 1).sum() >= 0.01 * d.size and ((d > 0) & (d < 1)).mean() >= 0.3
        got = run(s, x, U16, U16)
        assert np.array_equal(got, hwc(Z.encode(d)))
        assert (got == 0).any() and (got == 65535).any()
    finally:
        s.set_option("precise", 0)


# ---- 4. RGBA ------------------------------------------------------------------------------------------------------------------------
def rgba(seed, fmt, w, h):
    """A seeded RGBA image of U8 or U16 whose alpha carries 0 and the maximum: a flat corner of each, the rest over the whole range."""
    top = 65535 if fmt == U16 else 255
    img = np.random.default_rng(seed).integers(0, top + 1, size=(h, w, 4)).astype(Z.np_dtype(fmt))
    img[:6, :7, 3] = 0
    img[-6:, -7:, 3] = top
    img[10, 3:9, 3] = top
    img[11, 3:9, 3] = 0
    return img


def alpha_want(img, in_fmt, out_fmt, scale):
    """The alpha plane of the output: the float32 x4 alpha in source units, in destination units, clamped, reduced, floor(mean + 0.5)."""
    a4 = Z.alpha_units(Z.alpha_x4(img[:, :, 3], T, f32=Z.alpha_chain(in_fmt)), in_fmt, out_fmt)
    top = Z.alpha_max(out_fmt)
    if scale == 4:
        m = a4
    elif scale in (2, 1):
        m = Z.box_mean(np.clip(a4, 0, top).astype(np.float32), 4 // scale)
    else:
        m = area_reduce(a4, scale.numerator, scale.denominator, top=top)
    return Z.alpha_store(m, out_fmt)


PAIRS = [(U8, U8), (U8, U16), (U16, U8), (U16, U16)]


@pytest.mark.parametrize("scale", [4, 2, Fraction(3, 2)], ids=["x4", "x2", "x3_2"])
@pytest.mark.parametrize("pair", PAIRS, ids=["u8-u8", "u8-u16", "u16-u8", "u16-u16"])
def test_rgba(ctx, pair, scale):
    """33 x 21 at tile 16 (tiles 16, 16 and 1 wide; 16 and 5 high) -- 34 x 22 at 3/2, which takes no odd size."""
    in_fmt, out_fmt = pair
    w, h = (33, 21) if scale in (4, 2) else (34, 22)
    for tta in (False, True):
        s = ctx[tta]
        if scale in (4, 2):
            s.out_scale = scale
        else:
            s.out_ratio = scale
        img = rgba(70 + in_fmt, in_fmt, w, h)
        got = run(s, img, in_fmt, out_fmt)
        ow, oh = s.out_size_fmt(out_fmt, w, h)
        assert got.shape == (oh, ow, 4) and got.dtype == Z.np_dtype(out_fmt)
        assert np.array_equal(got[:, :, :3], run(s, np.ascontiguousarray(img[:, :, :3]), in_fmt, out_fmt))  # RGB as without alpha
        want = alpha_want(img, in_fmt, out_fmt, scale)
        ga = got[:, :, 3]
        nd = int((ga != want).sum())
        print("%s -> %s at %s%s: %d of %d alpha samples differ, max |diff| %d" % (in_fmt, out_fmt, scale, " tta" if tta else "", nd, ga.size,
                                                                                  np.abs(ga.astype(int) - want.astype(int)).max()))
        assert np.array_equal(ga, want)
        assert (ga == 0).any() and (ga == Z.alpha_max(out_fmt)).any()
        for dbg in (32768, 65536):  # either thread shape of the x4 launch (uint8: either kernel) forced: the same bytes
            s.set_option("dbg", dbg)
            assert np.array_equal(run(s, img, in_fmt, out_fmt), got), dbg
            s.set_option("dbg", 0)
        if tta:
            assert np.array_equal(ga, alpha_plain)  # (alpha does not pass through the network)
        alpha_plain = ga


# ---- 5. one pair each ---------------------------------------------------------------------------------------------------------------
def test_nv12_to_u16(ctx):
    s = ctx[False]
    surf = image(80, NV12, W, 26)
    d = run(s, surf, NV12, F32)
    assert np.array_equal(run(s, surf, NV12, U16), hwc(Z.encode(d)))


def test_u16_to_p010(ctx):
    s = ctx[False]
    img = Z.image16(81, W, 26)
    d = run(s, Z.as_f32_chw(img), F32, F32)
    want = yuv_ref.join(*yuv_ref.encode(d, 709, 0, 10), 10)
    assert same_bits(run(s, img, U16, P010), want)
    assert same_bits(run(s, img, U16, P010), run(s, Z.as_f32_chw(img), F32, P010))


def test_u16_to_u8_is_the_uint8_path_fed_the_halfs(ctx):
    for tta in (False, True):
        s = ctx[tta]
        img = Z.image16(82, W, H)
        halfs = np.ascontiguousarray(Z.decode(img).transpose(2, 0, 1))
        assert np.array_equal(run(s, img, U16, U8), run(s, halfs, F16, U8))
        assert same_bits(run(s, img, U16, F16), run(s, halfs, F16, F16))


# ---- 6. layouts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,tta,os_", [(3, False, 4), (4, False, 4), (3, True, 2), (4, False, 1)], ids=["rgb-x4", "rgba-x4", "rgb-tta-x2", "rgba-x1"])
def test_batch_of_three_pitched_windows(ctx, c, tta, os_):
    """Three images in ONE rsr_process_device_batch call, each a window at an ODD PIXEL offset of a larger allocation, its row pitch two
    bytes beyond its rows: every window holds what the lone call gives, every other byte of the 0xCD canvases stays."""
    s = ctx[tta]
    s.out_scale = os_
    imgs = [(rgba(90 + i, U16, W, H) if c == 4 else Z.image16(90 + i, W, H)) for i in range(3)]
    lone = [run(s, x, U16, U16) for x in imgs]
    ow, oh = W * os_, H * os_
    ipitch, opitch = 2 * W * c + 2, 2 * ow * c + 2
    ioff, ooff = 2 * ipitch + 3 * 2 * c, opitch + 5 * 2 * c  # pixel 3 of row 2, pixel 5 of row 1 of the surrounding rows
    assert (ioff | ooff) % 8 != 0  # (odd pixel offsets: no window starts where a wider access would be aligned)
    ispan, ospan = R.image_span(U16, W, H, c, ipitch, 0), R.image_span(U16, ow, oh, c, opitch, 0)
    assert ospan == (oh - 1) * opitch + 2 * ow * c
    ins, outs, keep = [], [], []
    for x in imgs:
        canvas = np.full(ioff + ispan + 64, 0x5A, dtype=np.uint8)
        rows = x.view(np.uint8).reshape(H, -1)
        for r in range(H):
            canvas[ioff + r * ipitch:ioff + r * ipitch + rows.shape[1]] = rows[r]
        d_in = torch.from_numpy(canvas).cuda()
        d_out = torch.full((ooff + ospan + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        keep.append((d_in, d_out))
        ins.append((d_in.data_ptr() + ioff, ipitch, 0))
        outs.append((d_out.data_ptr() + ooff, opitch, 777))  # (plane_pitch is ignored)
    calls = s.get_stat("batch_calls")
    s.process_device_batch(ins, U16, W, H, c, outs, U16)
    torch.cuda.synchronize()
    assert s.get_stat("batch_calls") == calls + 1
    for (_, d_out), want in zip(keep, lone):
        got = d_out.cpu().numpy()
        inside = np.zeros(got.shape, dtype=bool)
        wrows = want.view(np.uint8).reshape(oh, -1)
        for r in range(oh):
            o = ooff + r * opitch
            assert np.array_equal(got[o:o + wrows.shape[1]], wrows[r]), r
            inside[o:o + wrows.shape[1]] = True
        assert (got[~inside] == SENTINEL).all() and inside.sum() == want.nbytes


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_before_launch(ctx):
    s = ctx[False]
    buf = torch.full((1 << 18,), SENTINEL, dtype=torch.uint8, device="cuda")
    p, q = buf.data_ptr(), buf.data_ptr() + (1 << 17)

    def refused(*a, batch=False):
        with pytest.raises(R.RealSRError) as e:
            (s.process_device_batch if batch else s.process_device_fmt)(*a)
        assert e.value.code == R.RSR_E_ARG, a

    def work():
        refused(p + 1, U16, 8, 8, 3, q, U8)                                  # odd data, on either side
        refused(p, U8, 8, 8, 3, q + 1, U16)
        refused([(p + 1, 0, 0)], U16, 8, 8, 3, [q], U16, batch=True)
        refused([p], U16, 8, 8, 3, [(q + 1, 0, 0)], U16, batch=True)
        refused([(p, 49, 0)], U16, 8, 8, 3, [q], U16, batch=True)            # odd row pitch
        refused([p], U16, 8, 8, 3, [(q, 32 * 6 + 1, 0)], U16, batch=True)
        refused([(p, 46, 0)], U16, 8, 8, 3, [q], U16, batch=True)            # a pitch below a row
        refused([p], U16, 8, 8, 4, [(q, 32 * 8 - 2, 0)], U16, batch=True)
        for c in (2, 5):
            refused(p, U16, 8, 8, c, q, U16)
            refused([p], U16, 8, 8, c, [q], U8, batch=True)
        for planar in (F16, F32, NV12):                                          # c == 4 with a planar other side
            refused(p, U16, 8, 8, 4, q, planar)
            refused(p, planar, 8, 8, 4, q, U16)
        for bad in (14, 15, 17):                                                 # the ids around the new one stay unknown
            refused(p, bad, 8, 8, 3, q, U16)
            refused(p, U16, 8, 8, 3, q, bad)
        s.out_ratio = Fraction(3, 2)
        refused(p, U16, 35, 25, 3, q, U16)                                   # the ratio rule holds as for uint8

    _, prof = profile_of(s, work)
    torch.cuda.synchronize()
    assert prof["calls"] == 0 and prof["conv_launches"] == 0 and prof["tiles"] == 0  # nothing was launched
    assert (buf == SENTINEL).all()


# ---- 8. masked and sequence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [3, 4], ids=["rgb", "rgba"])
def test_masked_tiles(ctx, c):
    s = ctx[False]
    img = rgba(100, U16, W, H) if c == 4 else Z.image16(100, W, H)
    full = run(s, img, U16, U16)
    assert s.tile_count(W, H) == (3, 2)
    mask = np.array([1, 0, 1, 0, 1, 0], dtype=np.uint8)
    d_in, d_out = dev(img), torch.full((full.nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    s.process_device_masked(d_in.data_ptr(), U16, W, H, c, d_out.data_ptr(), U16, mask)
    torch.cuda.synchronize()
    want = Z.sentinel_bytes(U16, full.shape)
    for t in np.flatnonzero(mask):
        x0, y0, x1, y1 = ref.out_rect(W, H, T, t)
        want[y0:y1, x0:x1] = full[y0:y1, x0:x1]
    got = d_out.cpu().numpy().view(np.uint16).reshape(full.shape)
    assert np.array_equal(got, want) and not np.array_equal(got, full)


def test_sequence_of_three_frames_with_prev_out(ctx):
    s = ctx[False]
    frames = [Z.image16(110 + i, W, H) for i in range(3)]
    full = [run(s, x, U16, U16) for x in frames]
    prev = Z.image16(115, 4 * W, 4 * H)
    masks = np.array([[1, 0, 0, 0, 1, 0],
                      [0, 1, 0, 0, 0, 0],
                      [0, 0, 0, 1, 1, 0]], dtype=np.uint8)
    d_ins = [dev(x) for x in frames]
    d_outs = [torch.full((full[0].nbytes,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in frames]
    d_prev = dev(prev)
    s.process_device_sequence([t.data_ptr() for t in d_ins], U16, W, H, 3, [t.data_ptr() for t in d_outs], U16, masks.reshape(-1), prev_out=d_prev.data_ptr())
    torch.cuda.synchronize()
    state = prev.copy()
    for k in range(3):
        for t in np.flatnonzero(masks[k]):
            x0, y0, x1, y1 = ref.out_rect(W, H, T, t)
            state[y0:y1, x0:x1] = full[k][y0:y1, x0:x1]
        got = d_outs[k].cpu().numpy().view(np.uint16).reshape(full[k].shape)
        assert np.array_equal(got, state), k
    assert np.array_equal(d_prev.cpu().numpy().view(np.uint16).reshape(prev.shape), prev)


# ---- 9. the frame diff --------------------------------------------------------------------------------------------------------------
def diff_want(w, h, x, y):
    """The tiles whose rsr_tile_source_rect holds pixel (x, y)."""
    nx, ny = ref.tile_count(w, h, T)
    m = np.zeros(nx * ny, dtype=np.uint8)
    for t in range(nx * ny):
        x0, y0, x1, y1 = ref.source_rect(w, h, T, P, t)
        m[t] = x0 <= x < x1 and y0 <= y < y1
    return m


@pytest.mark.parametrize("c", [3, 4], ids=["rgb", "rgba"])
def test_diff_tiles(ctx, c):
    """The LOW byte of one sample flipped -- of one colour sample, of one alpha sample -- flags exactly the tiles whose source rectangle
    holds the pixel; a pitched pair at different offsets gives the same masks."""
    s = ctx[False]
    a = rgba(120, U16, W, H) if c == 4 else Z.image16(120, W, H)
    d_a = dev(a)
    seen = set()
    for i, (x, y) in enumerate([(0, 0), (25, 24), (26, 24), (6, 6), (5, 6), (6, 5), (35, 24), (15, 15), (16, 5)]):
        b = a.copy()
        b[y, x, (c - 1) if i % 2 else i % 3] ^= 0x0001  # (odd cases: the last sample of the pixel -- alpha when c == 4)
        want = diff_want(W, H, x, y)
        assert s.tile_source_rect(W, H, 0) == ref.source_rect(W, H, T, P, 0)
        d_mask = torch.full((6,), SENTINEL, dtype=torch.uint8, device="cuda")
        s.diff_tiles(d_a.data_ptr(), dev(b).data_ptr(), U16, W, H, c, d_mask.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_mask.cpu().numpy(), want), ((x, y), want)
        seen.add(tuple(want))
        if i == 3:
            pitch = 2 * W * c + 2
            ca, cb = (np.full(R.image_span(U16, W, H, c, pitch, 0) + 16, 0x11 * (k + 1), dtype=np.uint8) for k in range(2))
            for canvas, off, im in ((ca, 2, a), (cb, 6, b)):
                rows = im.view(np.uint8).reshape(H, -1)
                for r in range(H):
                    canvas[off + r * pitch:off + r * pitch + rows.shape[1]] = rows[r]
            da, db = torch.from_numpy(ca).cuda(), torch.from_numpy(cb).cuda()
            d_mask.fill_(SENTINEL)
            s.diff_tiles((da.data_ptr() + 2, pitch, 0), (db.data_ptr() + 6, pitch, 0), U16, W, H, c, d_mask.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(d_mask.cpu().numpy(), want)
    assert len(seen) >= 4 and any(sum(m) == 1 for m in seen) and any(sum(m) > 1 for m in seen)
    # the sequence form
    frames = [a.copy() for _ in range(3)]
    frames[1][24, 26, 0] ^= 1
    frames[2][24, 26, 0] ^= 1
    frames[2][0, 0, c - 1] ^= 0x0100
    d_f = [dev(x) for x in frames]
    d_masks = torch.full((18,), SENTINEL, dtype=torch.uint8, device="cuda")
    s.diff_tiles_sequence([t.data_ptr() for t in d_f], d_a.data_ptr(), U16, W, H, c, d_masks.data_ptr())
    torch.cuda.synchronize()
    want = np.stack([np.zeros(6, np.uint8), diff_want(W, H, 26, 24), diff_want(W, H, 0, 0)])
    assert np.array_equal(d_masks.cpu().numpy().reshape(3, 6), want) and want[1].any() and want[2].any()


# ---- 10. the default path keeps its launches ------------------------------------------------------------------------------------------
def test_default_path_guard(ctx):
    """u8 -> u8 is still conv_last writing the image itself: no post-processing launch.  A U16 output costs exactly one launch more --
    the same convs, one postproc_tiles -- and a U16 INPUT none."""
    s = ctx[False]
    img8 = image(130, U8, W, H)
    got8, p0 = profile_of(s, lambda: run(s, img8, U8, U8))
    assert p0["conv_launches"] == R.NUM_CONVS and p0["post_ms"] == 0 and p0["post_bytes"] == 0 and p0["calls"] == 1
    _, p1 = profile_of(s, lambda: run(s, Z.widen(img8), U16, U8))
    assert p1["conv_launches"] == R.NUM_CONVS and p1["post_ms"] == 0 and p1["post_bytes"] == 0 and p1["calls"] == 1
    assert p1["pre_bytes"] > p0["pre_bytes"]
    _, p2 = profile_of(s, lambda: run(s, img8, U8, U16))
    assert p2["conv_launches"] == R.NUM_CONVS and p2["post_ms"] > 0 and p2["calls"] == 1 and p2["tiles"] == p0["tiles"]
    s.set_option("dbg", 8192)
    _, p3 = profile_of(s, lambda: run(s, img8, U8, U8))                # the unfused uint8 route: the same one launch more
    assert p3["conv_launches"] == R.NUM_CONVS and p3["post_ms"] > 0
    assert p2["post_bytes"] > p3["post_bytes"] > 0  # (the same blob read; 6 bytes per pixel written, not 3)
    assert np.array_equal(run(s, img8, U8, U8), got8)
