"""Option "dither" on the GPU (run with -m gpu): every comparison is np.array_equal against tests/dither_ref.py applied to what the SAME
context leaves as RSR_FMT_F32_CHW -- the definition of include/realsr_hip.h ("dither").  Tile 16, images of 35 x 25 and 83 x 44 (3 x 2 and
6 x 3 tiles: a pattern keyed to the tile instead of the image would show), 36 x 26 for the subsampled surfaces, 1 x 1 and 40 x 1.
tests/gpu_support.py's DEFAULTS does not know the option, so this module puts it (and "alpha_net") back itself around every test."""
import os
import threading
from fractions import Fraction

import numpy as np
import pytest
import torch

import exact_net as N
import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import synth

import dither_ref as D
import rgb16_ref as Z
import tile_diff_ref as ref
from gpu_support import context_fixtures, dev, paths, profile_of  # noqa: F401
from pixfmt_ref import F16, F32, NV12, NV16, P010, P210, U8, YUV444P, YUV444P10, S420, S422, image, lift, paste, place, same_bits

pytestmark = pytest.mark.gpu
U16 = R.RSR_FMT_U16_HWC
T, P = 16, 10
SENTINEL = 0xCD
INTEGER = [U8, U16, NV12, P010, NV16, P210, YUV444P, YUV444P10]
NAMES = {U8: "u8", U16: "u16", NV12: "nv12", P010: "p010", NV16: "nv16", P210: "p210", YUV444P: "yuv444p", YUV444P10: "yuv444p10"}
ctxs, ctx_ = context_fixtures(T, P)


@pytest.fixture(autouse=True)
def ctx(ctx_):
    for s in ctx_.values():
        s.dither, s.alpha_net = 0, 0
    yield ctx_
    for s in ctx_.values():
        s.dither, s.alpha_net = 0, 0


def run(s, x, in_fmt, out_fmt):
    """One synchronous rsr_process_device_fmt call on the packed numpy image x into a destination of 0xCD bytes."""
    w, h = Z.dims_of(in_fmt, x)
    c = Z.channels_of(in_fmt, x)
    ow, oh = s.out_size_fmt(out_fmt, w, h)
    oshape = Z.shape_of(out_fmt, ow, oh, c)
    d_in, d_out = dev(x), dev(Z.sentinel_bytes(out_fmt, oshape))
    assert d_out.numel() == R.image_bytes(out_fmt, ow, oh, c)
    s.process_device_fmt(d_in.data_ptr(), in_fmt, w, h, c, d_out.data_ptr(), out_fmt)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(Z.np_dtype(out_fmt)).reshape(oshape)


def check(s, x, in_fmt, fmt, cfg=(709, 0), siting=0, tile_out=4 * T):
    """The dithered output of format fmt is dither_ref of the context's F32 output; the float outputs do not see the option.  Returns it."""
    rgb = np.ascontiguousarray(x[:, :, :3]) if in_fmt in (U8, U16) else x
    s.dither = 0
    d, d16, plain = run(s, rgb, in_fmt, F32), run(s, rgb, in_fmt, F16), run(s, x, in_fmt, fmt)
    assert d.min() >= 0 and d.max() <= 1 and (d.size < 64 or len(np.unique(d)) > 16)
    s.dither = 1
    assert s.dither == 1 and s.get_stat("dither") == 1
    assert same_bits(run(s, rgb, in_fmt, F32), d) and same_bits(run(s, rgb, in_fmt, F16), d16)
    got = run(s, x, in_fmt, fmt)
    want = D.encode(fmt, d, cfg, siting, tile_out)
    assert got.dtype == want.dtype
    if fmt in (U8, U16) and got.shape[2] == 4:  # RGBA: the colour is dithered, the alpha is the plain call's
        assert np.array_equal(got[:, :, :3], want) and np.array_equal(got[:, :, 3], plain[:, :, 3])
    else:
        assert got.shape == want.shape and np.array_equal(got, want), (NAMES[fmt], np.argwhere(got != want)[:4])
    if d.size >= 64:
        assert not np.array_equal(got, plain)  # (the option acts)
    return got


def size_for(fmt, big=False):
    if fmt in S420 or fmt in S422:
        return (84, 44) if big else (36, 26)
    return (83, 44) if big else (35, 25)


# ---- 1. every integer format --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", INTEGER, ids=[NAMES[f] for f in INTEGER])
def test_every_integer_format(ctx, fmt):
    s = ctx[False]
    for big in (False, True):
        w, h = size_for(fmt, big)
        check(s, image(10 + fmt + big, U8, w, h), U8, fmt)
    check(s, image(30 + fmt, F16, *size_for(fmt)), F16, fmt)  # values the uint8 path cannot make


@pytest.mark.parametrize("c", [3, 4], ids=["rgb", "rgba"])
def test_rgba_keeps_its_alpha(ctx, c):
    """U8 and U16, either side; at x4 (one and two pixels per thread), out_scale 2 (the box kernel's alpha) and 3/2 (the area kernel's)."""
    for tta in (False, True):
        s = ctx[tta]
        for scale in (4, 2, Fraction(3, 2)):
            s.out_ratio = Fraction(scale)
            w, h = (33, 21) if scale != Fraction(3, 2) else (34, 22)
            for in_fmt, out_fmt in ((U8, U8), (U16, U16), (U8, U16), (U16, U8)):
                x = image(40 + in_fmt, U8, w, h, c)
                x = Z.widen(x) if in_fmt == U16 else x
                if c == 4:
                    x[:, :, 3] = np.random.default_rng(41).integers(0, int(x.max()) + 1, size=(h, w))
                check(s, x, in_fmt, out_fmt, tile_out=int(T * scale))


# ---- 2. every mode ------------------------------------------------------------------------------------------------------------------
MODES = ["tta", "precise", "tta-precise", "bgr", "x2", "x1", "tta-x2", "dbg32768", "dbg65536", "tta-dbg32768"]


@pytest.mark.parametrize("mode", MODES)
def test_modes(ctx, mode):
    """TTA (the staged and the per-pixel uint8 kernel, one and two uint16 pixels per thread through "dbg"), precise, bgr, out_scale 2 / 1."""
    s = ctx[mode.startswith("tta")]
    s.set_option("precise", int("precise" in mode))
    s.set_option("bgr", int("bgr" in mode))
    if "dbg" in mode:
        s.set_option("dbg", int(mode.split("dbg")[1]))
    os_ = int(mode[-1]) if mode[-2:] in ("x2", "x1") else 4
    s.out_scale = os_
    k = MODES.index(mode)
    fmts = [U8, U16] if "bgr" in mode or "dbg" in mode else INTEGER
    for fmt in fmts:
        cfg = [(709, 0), (601, 1), (2020, 0)][(k + fmt) % 3]
        s.set_option("yuv_matrix", cfg[0])
        s.set_option("yuv_range", cfg[1])
        w, h = size_for(fmt)
        check(s, image(50 + k + fmt, U8, w, h), U8, fmt, cfg, 0, T * os_)


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_ratio_3_2(ctx, tta):
    """36 x 26 at 3/2 and tile 16: 54 x 39, rectangles of 24 x 24 -- an odd height, which NV12 refuses; 36 x 28 for the 4:2:0 surfaces."""
    s = ctx[tta]
    s.out_ratio = Fraction(3, 2)
    for fmt in INTEGER:
        w, h = (36, 28) if fmt in S420 else (36, 26)
        check(s, image(70 + fmt, U8, w, h), U8, fmt, tile_out=24)


def test_a_ratio_per_axis(ctx):
    """48 x 28 at (8/3, 9/4) and tile 24: rectangles of 64 x 54, output 128 x 63 (odd rows: no 4:2:0 surface)."""
    s = ctx[False]
    s.tilesize = 24
    s.out_ratio_xy = (Fraction(8, 3), Fraction(9, 4))
    for fmt in (U8, U16, NV16, P210, YUV444P, YUV444P10):
        assert s.out_size_fmt(fmt, 48, 28) == (128, 63)
        check(s, image(80 + fmt, U8, 48, 28), U8, fmt, tile_out=64)


@pytest.mark.parametrize("siting", [1, 2])
def test_sitings(ctx, siting):
    """Left and top-left chroma: the sited filters and their tile-first clamp give the value, the threshold sits at the chroma sample's own
    indices.  x4 and out_scale 2; under TTA too."""
    for tta, os_ in ((False, 4), (False, 2), (True, 4)):
        s = ctx[tta]
        s.out_scale = os_
        s.yuv_siting = siting
        for fmt in (NV12, P010, NV16, P210):
            check(s, image(90 + fmt + os_, U8, 36, 26), U8, fmt, (709, 0), siting, T * os_)


@pytest.mark.parametrize("w,h", [(1, 1), (40, 1)])
def test_tiny_images(ctx, w, h):
    for tta in (False, True):
        for fmt in (U8, U16, YUV444P, YUV444P10):
            check(ctx[tta], image(100 + w, U8, w, h), U8, fmt)
    if w % 2 == 0:
        check(ctx[False], image(101, U8, w, h), U8, NV16)


# ---- 3. black stays black, white stays white ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exact_ctx(tmp_path_factory):
    """The two-term exact model of tests/exact_net.py: its conv_last reaches both clamps on exact_net.frame_u8."""
    d = str(tmp_path_factory.mktemp("dither_exact"))
    synth.write_param(os.path.join(d, "x4.param"))
    synth.write_bin(os.path.join(d, "x4.bin"), N.dense_weights(N.make_model()), "fp16")
    s = R.RealSR(0)
    s.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
    yield s
    s.close()


def test_exact_codes_keep_their_code(exact_ctx):
    """No hook forces the F32 output to arbitrary code values; the exact model forces it to the two codes that matter most -- at least a
    hundredth of its output each is exactly 0 and exactly 1 -- and every sample there keeps its code at every depth: 0 and M."""
    s = exact_ctx
    w, h, t = N.FRAME
    s.tilesize, s.prepadding = t, 10
    x = N.frame_u8(w, h)
    d = run(s, x, U8, F32)
    assert (d == 0).sum() >= 0.01 * d.size and (d == 1).sum() >= 0.01 * d.size and ((d > 0) & (d < 1)).mean() >= 0.3
    s.dither = 1
    try:
        for fmt, M in ((U8, 255), (U16, 65535)):
            got = run(s, x, U8, fmt)
            assert np.array_equal(got, D.quantise_rgb(d, M))
            planes = got.transpose(2, 0, 1)
            assert (planes[d == 0] == 0).all() and (planes[d == 1] == M).all()
            codes = d * np.float32(M) == np.floor(d * np.float32(M))  # every d that is exactly a code
            assert np.array_equal(planes[codes], (d * np.float32(M))[codes].astype(planes.dtype))
    finally:
        s.dither = 0


# ---- 4. the entry points ------------------------------------------------------------------------------------------------------------
def test_host_pointers(ctx):
    s = ctx[False]
    x = image(110, U8, 35, 25)
    d = s.process_fmt(x, U8, F32)
    s.dither = 1
    assert np.array_equal(s.process(x), D.quantise_rgb(d, 255))  # (the early download of the fused route is off: the bytes arrive whole)
    assert np.array_equal(s.process_fmt(x, U8, U16), D.quantise_rgb(d, 65535))
    x2 = image(111, U8, 36, 26)
    d2 = s.process_fmt(x2, U8, F32)
    assert same_bits(s.process_fmt(x2, U8, NV12), D.encode(NV12, d2))
    assert same_bits(s.process_fmt(x2, U8, F32), d2)


@pytest.mark.parametrize("fmt", [U8, NV12, YUV444P10], ids=["u8", "nv12", "yuv444p10"])
def test_batch_window_carries_the_pattern_from_its_own_origin(ctx, fmt):
    """Two images in one rsr_process_device_batch call, each into a window at a nonzero offset of a 0xCD canvas, rows pitched: the window
    holds the bytes of the lone dithered call -- theta(0, 0) at the window's first sample -- and no byte outside it is written."""
    s = ctx[False]
    s.dither = 1
    w, h = 36, 26
    ow, oh = 4 * w, 4 * h
    es = 3 if fmt == U8 else Z.np_dtype(fmt).itemsize
    pitch = ow * es + 6
    rows = {U8: oh, NV12: oh + oh // 2, YUV444P10: oh}[fmt]
    plane = pitch * rows + 64
    off = 3 * pitch + 10 * es
    imgs = [image(120 + i, U8, w, h) for i in range(2)]
    lone = [run(s, x, U8, fmt) for x in imgs]
    d_ins = [dev(x) for x in imgs]
    span = off + plane * 3 + 64
    d_outs = [torch.full((span,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in imgs]
    s.process_device_batch([t.data_ptr() for t in d_ins], U8, w, h, 3, [(t.data_ptr() + off, pitch, plane) for t in d_outs], fmt)
    torch.cuda.synchronize()
    for t, want in zip(d_outs, lone):
        got = t.cpu().numpy()
        assert same_bits(lift(got, off, pitch, plane, fmt, ow, oh), want)
        inside = place(np.zeros(span, np.uint8), off, pitch, plane, want, fmt)
        assert inside.sum() == want.nbytes and (got[~inside] == SENTINEL).all()


@pytest.mark.parametrize("fmt", [U8, NV12], ids=["u8", "nv12"])
def test_masked_call_and_sequence(ctx, fmt):
    """A partial mask gives the plain dithered call on the marked rectangles and leaves the rest alone; a sequence with a repeated frame
    copies rectangles that are the bytes a computation would give."""
    s = ctx[False]
    s.dither = 1
    w, h = 36, 26
    frames = [image(130, U8, w, h), image(130, U8, w, h), image(131, U8, w, h)]
    full = [run(s, x, U8, fmt) for x in frames]
    assert s.tile_count(w, h) == (3, 2)
    mask = np.array([1, 0, 1, 0, 1, 0], dtype=np.uint8)
    d_out = dev(Z.sentinel_bytes(fmt, full[0].shape))
    s.process_device_masked(dev(frames[0]).data_ptr(), U8, w, h, 3, d_out.data_ptr(), fmt, mask)
    torch.cuda.synchronize()
    want = Z.sentinel_bytes(fmt, full[0].shape)
    for t in np.flatnonzero(mask):
        paste(fmt, want, full[0], ref.out_rect(w, h, T, t))
    got = d_out.cpu().numpy().view(full[0].dtype).reshape(full[0].shape)
    assert np.array_equal(got, want) and not np.array_equal(got, full[0])
    masks = np.array([[1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0], [1, 0, 0, 1, 1, 0]], dtype=np.uint8)
    d_ins = [dev(x) for x in frames]
    d_outs = [dev(Z.sentinel_bytes(fmt, full[0].shape)) for _ in frames]
    s.process_device_sequence([t.data_ptr() for t in d_ins], U8, w, h, 3, [t.data_ptr() for t in d_outs], fmt, masks.reshape(-1))
    torch.cuda.synchronize()
    state = full[0].copy()
    for k in range(3):
        for t in np.flatnonzero(masks[k]):
            paste(fmt, state, full[k], ref.out_rect(w, h, T, t))
        assert np.array_equal(d_outs[k].cpu().numpy().view(full[0].dtype).reshape(full[0].shape), state), k
    assert np.array_equal(full[0], full[1])


def test_tile_ranges_carry_the_image_pattern(ctx):
    """rsr_process_rows / rsr_process_tiles: a range's device buffer holds only its rows, the pattern is still the image's."""
    s = ctx[False]
    x = image(140, U8, 35, 41)  # 3 x 3 tiles
    d = s.process_fmt(x, U8, F32)
    s.dither = 1
    want = D.quantise_rgb(d, 255)
    out = np.full(want.shape, SENTINEL, np.uint8)
    s.process_rows(x, out, 1, 3)
    assert np.array_equal(out[64:], want[64:]) and (out[:64] == SENTINEL).all()
    s.process_rows(x, out, 0, 1)
    assert np.array_equal(out, want)
    out = np.full(want.shape, SENTINEL, np.uint8)
    s.process_tiles(x, out, 4, 8)
    part = np.full(want.shape, SENTINEL, np.uint8)
    for t in range(4, 8):
        paste(U8, part, want, ref.out_rect(35, 41, T, t))
    assert np.array_equal(out, part)
    s.process_tiles(x, out, 0, 4)
    s.process_tiles(x, out, 8, 9)
    assert np.array_equal(out, want)


def test_concurrent_small_calls(ctx):
    """Two callers at once (their images may share a merged batch, of two geometries) and rsr_process_many: the bytes of the lone calls."""
    s = ctx[False]
    imgs = [image(150, U8, 35, 25), image(151, U8, 21, 30, 4)]
    d = [s.process_fmt(np.ascontiguousarray(x[:, :, :3]), U8, F32) for x in imgs]
    plain_alpha = s.process(imgs[1])[:, :, 3]
    s.dither = 1
    outs = [None, None]
    gate = threading.Barrier(2)

    def work(i):
        gate.wait()
        outs[i] = s.process(imgs[i], push_params=False)
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    many = s.process_many(imgs)
    print("merged batches: %d" % s.get_stat("merged_batches"))
    for got in (outs, many):
        assert np.array_equal(got[0], D.quantise_rgb(d[0], 255))
        assert np.array_equal(got[1][:, :, :3], D.quantise_rgb(d[1], 255)) and np.array_equal(got[1][:, :, 3], plain_alpha)


def test_alpha_net_alpha_is_not_dithered(ctx):
    s = ctx[False]
    x = image(160, U8, 33, 21, 4)
    s.alpha_net = 1
    for fmt in (U8, U16):
        plain = run(s, x, U8, fmt)
        got = check(s, x, U8, fmt)
        s.dither = 0
        assert np.array_equal(got[:, :, 3], plain[:, :, 3]) and np.array_equal(run(s, x, U8, fmt), plain)
        s.alpha_net = 0
        assert not np.array_equal(run(s, x, U8, fmt)[:, :, 3], plain[:, :, 3])  # (the network's alpha is not the bicubic: the pass did run)
        s.alpha_net = 1


# ---- 5. the option itself -----------------------------------------------------------------------------------------------------------
def test_off_after_on_is_a_fresh_context(ctx, paths):
    """dither 0 after 1: the bytes and the launches of a context that never saw the option -- u8 -> u8 is conv_last's fused store again, no
    post launch -- and a context that alternates between the two keeps giving each setting its own bytes off one cached plan."""
    x = image(170, U8, 35, 25)
    fresh = R.RealSR(0)
    try:
        fresh.load(*paths)
        fresh.tilesize, fresh.prepadding = T, P
        want0, p_fresh = profile_of(fresh, lambda: run(fresh, x, U8, U8))
        want0_nv = run(fresh, image(171, U8, 36, 26), U8, NV12)
    finally:
        fresh.close()
    s = ctx[False]
    want1 = D.quantise_rgb(run(s, x, U8, F32), 255)
    plans = None
    for k in range(3):
        s.dither = 1
        got1, p1 = profile_of(s, lambda: run(s, x, U8, U8))
        s.dither = 0
        got0, p0 = profile_of(s, lambda: run(s, x, U8, U8))
        assert np.array_equal(got1, want1) and np.array_equal(got0, want0), k
        assert p1["conv_launches"] == p0["conv_launches"] == p_fresh["conv_launches"] == R.NUM_CONVS
        assert p1["post_ms"] > 0 and p1["post_bytes"] > 0                       # one post launch under the option ...
        assert p0["post_ms"] == 0 and p0["post_bytes"] == 0 == p_fresh["post_bytes"]  # ... none without: the fused store
        assert p0["tiles"] == p1["tiles"] == p_fresh["tiles"] and p0["pre_bytes"] == p_fresh["pre_bytes"]
        plans = s.get_stat("plans") if plans is None else plans
        assert s.get_stat("plans") == plans  # (one cached plan serves both settings)
    assert same_bits(run(s, image(171, U8, 36, 26), U8, NV12), want0_nv)


def test_refusals_stat_and_property(ctx):
    s = ctx[False]
    for held in (0, 1):
        s.dither = held
        for bad in (2, -1):
            with pytest.raises(R.RealSRError) as e:
                s.set_option("dither", bad)
            assert e.value.code == R.RSR_E_ARG and "dither" in str(e.value)
            assert s.dither == held and s.get_stat("dither") == held
        for bad in (0.5, 2, -1):
            with pytest.raises(R.RealSRError) as e:
                s.dither = bad
            assert e.value.code == R.RSR_E_ARG
            assert s.dither == held
    s.dither = True
    assert s.dither == 1
    s.set_option("dither", 0)
    assert s.dither == 0


def test_group_members_must_agree(ctx, paths):
    a, b = R.RealSR(0), R.RealSR(0)
    try:
        x = image(180, U8, 35, 25)
        for m in (a, b):
            m.load(*paths)
            m.tilesize, m.prepadding = T, P
        d = a.process_fmt(x, U8, F32)
        a.dither = 1
        out = np.full((100, 140, 3), SENTINEL, np.uint8)
        with pytest.raises(R.RealSRError) as e:
            R.process_group([a, b], x, out)
        assert e.value.code == R.RSR_E_ARG and "dither" in str(e.value) and (out == SENTINEL).all()
        b.dither = 1
        assert np.array_equal(R.process_group([a, b], x, out), D.quantise_rgb(d, 255))  # the shares of two contexts: one pattern
    finally:
        a.close()
        b.close()
