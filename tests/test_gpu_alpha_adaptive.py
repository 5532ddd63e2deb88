"""Option "alpha_adaptive" on the GPU (run with -m gpu): under "alpha_net" 1, tiles whose source rectangle holds ONE alpha value skip the
alpha pass.

The rule of include/realsr_hip.h ("alpha_adaptive") is exact, so every comparison is np.array_equal: the output rectangles of the flat tiles
of tests/alpha_flat_ref.py hold the bytes of the library's own "alpha_net" 0 call, all others those of its "alpha_net" 1 call, and the
counters move by the reference's counts.  Tile 16, prepadding 10; the base image is 83 x 44: 6 x 3 tiles, partial at both far edges.
Destinations are pre-filled with 0xCD."""
import threading
from fractions import Fraction

import numpy as np
import pytest
import torch

import alpha_flat_ref as AF
import realsr_ncnn_vulkan_amd as R
import rgb16_ref as Z
import tile_diff_ref as ref
from gpu_support import context_fixtures, dev, filled, paths, profile_of, run, untouched  # noqa: F401
from pixfmt_ref import U8

pytestmark = pytest.mark.gpu
U16 = R.RSR_FMT_U16_HWC
W, H, T, P = 83, 44, 16, 10
TOP = {U8: 255, U16: 65535}
ctxs, ctx = context_fixtures(T, P, others=("other",))


@pytest.fixture(autouse=True)
def alpha_options_off(ctxs):
    """gpu_support.DEFAULTS knows neither option: both 0 before and after every test of this module."""
    for s in ctxs.values():
        s.alpha_net = 0
        s.alpha_adaptive = 0
    yield
    for s in ctxs.values():
        s.alpha_net = 0
        s.alpha_adaptive = 0


# ---- images ---------------------------------------------------------------------------------------------------------------------------------
def colour(fmt, w, h, seed):
    return np.random.default_rng(seed).integers(0, TOP[fmt] + 1, size=(h, w, 4)).astype(Z.np_dtype(fmt))


def constant(k, fmt=U8, w=W, h=H, seed=3):
    img = colour(fmt, w, h, seed)
    img[:, :, 3] = k
    return img


def two_constants(hi, lo, fmt=U8, w=W, h=H, seed=4):
    """Alpha hi for x < 26, lo for x >= 38, a ramp between: at tile 16 / prepadding 10 the tile columns 1 and 2 ([6, 42) and [22, 58)) see
    more than one value, every other column one."""
    img = colour(fmt, w, h, seed)
    a = np.empty(w, dtype=np.int64)
    a[:26], a[38:] = hi, lo
    a[26:38] = hi + (lo - hi) * np.arange(1, 13) // 13
    img[:, :, 3] = a[None, :]
    return img


def rgba(fmt=U8, w=W, h=H, seed=7):
    """The pattern of tests/test_gpu_alpha_net.py: a ramp over the whole range, a band with a hard edge, seeded noise -- nothing flat."""
    top = TOP[fmt]
    img = colour(fmt, w, h, seed)
    a = img[:, :, 3]
    a[:h // 3, :] = (np.arange(w) * top // max(w - 1, 1))[None, :]
    a[h // 3:2 * h // 3, :w // 2] = 0
    a[h // 3:2 * h // 3, w // 2:] = top
    return img


# ---- calls ----------------------------------------------------------------------------------------------------------------------------------
def call(s, x, in_fmt=U8, out_fmt=U8):
    """One synchronous rsr_process_device_fmt call on the packed numpy image x (U8 / U16 HWC), into a 0xCD destination."""
    if in_fmt == U8 and out_fmt == U8:
        return run(s, x, in_fmt, out_fmt)
    w, h, c = x.shape[1], x.shape[0], x.shape[2]
    ow, oh = s.out_size_fmt(out_fmt, w, h)
    oshape = Z.shape_of(out_fmt, ow, oh, c)
    d_in, d_out = dev(x), dev(Z.sentinel_bytes(out_fmt, oshape))
    s.process_device_fmt(d_in.data_ptr(), in_fmt, w, h, c, d_out.data_ptr(), out_fmt)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(Z.np_dtype(out_fmt)).reshape(oshape)


def modes(s, fn):
    """(fn() at alpha_net 0, at alpha_net 1, at alpha_net 1 + alpha_adaptive 1, tiles the last ran the alpha pass on, tiles it skipped)."""
    s.alpha_net, s.alpha_adaptive = 0, 0
    o0 = fn()
    s.alpha_net = 1
    o1 = fn()
    s.alpha_adaptive = 1
    assert s.alpha_adaptive == 1 and s.get_stat("alpha_adaptive") == 1
    ran0, flat0 = s.get_stat("alpha_tiles"), s.get_stat("alpha_tiles_flat")
    oa = fn()
    ran, flat = int(s.get_stat("alpha_tiles") - ran0), int(s.get_stat("alpha_tiles_flat") - flat0)
    s.alpha_net, s.alpha_adaptive = 0, 0
    return o0, o1, oa, ran, flat


def check(s, img, in_fmt=U8, out_fmt=U8, fn=None, mixed=True, ratio=(4, 1, 4, 1)):
    """The selection rule for one image through fn (default: the device call).  mixed: some tiles are flat and some run, and on a flat tile
    the two alphas differ -- the case is not vacuous.  Returns (flags, adaptive image)."""
    h, w = img.shape[:2]
    tile = s.tilesize
    flags = AF.varies(img, tile, P)
    o0, o1, oa, ran, flat = modes(s, fn or (lambda: call(s, img, in_fmt, out_fmt)))
    want = AF.select(flags, o0, o1, w, h, tile, *ratio)
    print("alpha_adaptive %dx%d tile %d: %d tiles run, %d flat; %d bytes differ from the rule" % (w, h, tile, ran, flat, int((oa != want).sum())))
    assert oa.shape == o0.shape == o1.shape and oa.dtype == o0.dtype
    assert np.array_equal(oa, want)
    assert np.array_equal(oa[:, :, :3], o0[:, :, :3]) and np.array_equal(o1[:, :, :3], o0[:, :, :3])
    assert (ran, flat) == (int(flags.sum()), int((flags == 0).sum()))
    if mixed:
        assert 0 < ran and 0 < flat
        differs = 0
        for t in np.flatnonzero(flags == 0):
            x0, y0, x1, y1 = ref.out_rect(w, h, tile, int(t), *ratio)
            differs += int(not np.array_equal(o0[y0:y1, x0:x1, 3], o1[y0:y1, x0:x1, 3]))
        assert differs, "on no flat tile does the network's alpha differ from the bicubic: choose another constant"
    return flags, oa


# ---- 1. selection -----------------------------------------------------------------------------------------------------------------------------
def test_selection_on_a_sprite(ctx):
    """A sprite-like alpha: an opaque body, a transparent outside, noise along a band and in one corner."""
    s = ctx[False]
    img = constant(255, seed=10)
    img[:, 60:, 3] = 0
    img[12:20, 30:66, 3] = np.random.default_rng(11).integers(0, 256, size=(8, 36))
    img[40:, :4, 3] = 9
    flags, _ = check(s, img)
    assert flags.size == 18


@pytest.mark.parametrize("x,y,count", [(5, 5, 1), (6, 5, 2), (25, 0, 3), (26, 0, 2), (82, 43, 2), (69, 43, 2)])
def test_edges_of_the_rectangle(ctx, x, y, count):
    """Constant alpha and ONE differing sample: an off-by-one at either end of a source rectangle changes one of these counts."""
    s = ctx[False]
    img = constant(200, seed=12)
    img[y, x, 3] = 7
    flags, _ = check(s, img)
    assert int(flags.sum()) == count


@pytest.mark.parametrize("hi,lo", [(255, 0), (128, 77)])
def test_two_constants(ctx, hi, lo):
    """Columns 0, 3, 4 and 5 are flat (12 tiles) and hold exactly their constant; columns 1 and 2 run (6 tiles)."""
    s = ctx[False]
    img = two_constants(hi, lo)
    flags, oa = check(s, img)
    assert np.array_equal(flags.reshape(3, 6), np.array([[0, 1, 1, 0, 0, 0]] * 3, dtype=np.uint8))
    assert (oa[:, :64, 3] == hi).all() and (oa[:, 192:, 3] == lo).all()


@pytest.mark.parametrize("k", [255, 77])
def test_all_flat(ctx, k):
    """alpha_tiles does not move and the image is the alpha_net 0 image."""
    s = ctx[False]
    img = constant(k)
    o0, o1, oa, ran, flat = modes(s, lambda: call(s, img))
    assert (ran, flat) == (0, 18) and np.array_equal(oa, o0) and (oa[:, :, 3] == k).all()


def test_nothing_flat(ctx):
    s = ctx[False]
    img = rgba()
    assert AF.varies(img, T, P).all()
    o0, o1, oa, ran, flat = modes(s, lambda: call(s, img))
    assert (ran, flat) == (18, 0) and np.array_equal(oa, o1) and not np.array_equal(oa, o0)


# ---- 2. modes ---------------------------------------------------------------------------------------------------------------------------------
def test_tta(ctx):
    """The scan runs once per tile, not per orientation: 18 tiles are counted."""
    check(ctx[True], two_constants(255, 0))


def test_precise(ctx):
    s = ctx[False]
    s.set_option("precise", 1)
    check(s, two_constants(255, 0))


@pytest.mark.parametrize("scale", [2, 1], ids=["x2", "x1"])
def test_out_scale(ctx, scale):
    s = ctx[False]
    s.out_scale = scale
    _, oa = check(s, two_constants(255, 0), ratio=(scale, 1, scale, 1))
    assert oa.shape == (scale * H, scale * W, 4)


def test_ratio_3_2(ctx):
    s = ctx[False]
    s.out_ratio = Fraction(3, 2)
    _, oa = check(s, two_constants(255, 0, w=84), ratio=(3, 2, 3, 2))
    assert oa.shape == (66, 126, 4)


def test_pair_8_3_and_9_4(ctx):
    s = ctx[False]
    s.tilesize = 24
    s.out_ratio_xy = (Fraction(8, 3), Fraction(9, 4))
    _, oa = check(s, two_constants(255, 0, w=84), ratio=(8, 3, 9, 4))
    assert oa.shape == (99, 224, 4)


@pytest.mark.parametrize("pair", [(U16, U16), (U8, U16), (U16, U8)], ids=["u16-u16", "u8-u16", "u16-u8"])
def test_depths(ctx, pair):
    s = ctx[False]
    in_fmt, out_fmt = pair
    _, oa = check(s, two_constants(TOP[in_fmt], 0, in_fmt), in_fmt, out_fmt)
    assert oa.dtype == Z.np_dtype(out_fmt)
    assert (oa[:, :64, 3] == TOP[out_fmt]).all() and (oa[:, 192:, 3] == 0).all()


@pytest.mark.parametrize("out_fmt", [U16, U8], ids=["u16-u16", "u16-u8"])
def test_u16_low_byte_alone_varies(ctx, out_fmt):
    """0x8000 on the left, 0x80ff on the right: every sample shares its high byte, and the tiles in between still run."""
    s = ctx[False]
    img = two_constants(0x8000, 0x80ff, U16)
    assert ((img[:, :, 3] >> 8) == 0x80).all()
    flags, _ = check(s, img, U16, out_fmt)
    assert int(flags.sum()) == 6


# ---- 3. entry points --------------------------------------------------------------------------------------------------------------------------
def test_process(ctx):
    s = ctx[False]
    img = two_constants(255, 0, seed=30)
    check(s, img, fn=lambda: s.process(img))


def test_process_fmt(ctx):
    s = ctx[False]
    img = two_constants(65535, 0, U16, seed=31)
    check(s, img, U16, U16, fn=lambda: s.process_fmt(img, U16, U16))


def test_torch_upscale(ctx):
    from realsr_ncnn_vulkan_amd import torch_io
    s = ctx[False]
    img = two_constants(255, 0, seed=32)
    x = torch.from_numpy(img).cuda()
    check(s, img, fn=lambda: torch_io.upscale(s, x).cpu().numpy())


def test_batch_of_two_with_a_pitched_window(ctx):
    """Two images of different flags in ONE rsr_process_device_batch call.  The second is a window of a canvas whose alpha OUTSIDE the window
    is noise: the canvas is not read into the decision (the window's left columns stay flat) and not written."""
    s = ctx[False]
    a, b = two_constants(255, 0, seed=40), constant(77, seed=41)
    b[30:, 70:, 3] = 5
    fa, fb = AF.varies(a, T, P), AF.varies(b, T, P)
    assert not np.array_equal(fa, fb) and 0 < fb.sum() < 18
    canvas = np.random.default_rng(42).integers(0, 256, size=(H + 6, W + 9, 4), dtype=np.uint8)
    x0, y0 = 5, 3
    canvas[y0:y0 + H, x0:x0 + W] = b
    assert len(np.unique(canvas[:y0, :, 3])) > 1 and len(np.unique(canvas[:, :x0, 3])) > 1
    held = np.concatenate([np.array([0xEE], np.uint8), canvas.reshape(-1)])   # one byte in front: the window's rows start on no pixel boundary
    ipitch, ioff = (W + 9) * 4, (y0 * (W + 9) + x0) * 4 + 1
    ow, oh = 4 * W, 4 * H
    opitch, ooff = ow * 4 + 3, 2 * (ow * 4 + 3) + 5 * 4 + 1   # an odd pitch, an odd byte offset
    ospan = R.image_span(U8, ow, oh, 4, opitch, 0)
    d_a, d_canvas = dev(a), dev(held)

    def both():
        d_outs = [filled((ooff + ospan + 64,), U8) for _ in range(2)]
        s.process_device_batch([d_a.data_ptr(), (d_canvas.data_ptr() + ioff, ipitch, 0)], U8, W, H, 4, [(t.data_ptr() + ooff, opitch, 0) for t in d_outs], U8)
        torch.cuda.synchronize()
        outs = []
        for d_out in d_outs:
            got = d_out.cpu().numpy()
            inside = np.zeros(got.shape, dtype=bool)
            rows = np.empty((oh, ow * 4), dtype=np.uint8)
            for r in range(oh):
                o = ooff + r * opitch
                rows[r] = got[o:o + ow * 4]
                inside[o:o + ow * 4] = True
            assert (got[~inside] == 0xCD).all()
            outs.append(rows.reshape(oh, ow, 4))
        return outs
    o0, o1, oa, ran, flat = modes(s, both)
    assert (ran, flat) == (int(fa.sum() + fb.sum()), int((fa == 0).sum() + (fb == 0).sum()))
    for k, (img, flags) in enumerate(((a, fa), (b, fb))):
        assert np.array_equal(oa[k], AF.select(flags, o0[k], o1[k], W, H, T)), k
        assert not np.array_equal(oa[k], o1[k]) and not np.array_equal(oa[k], o0[k])
    assert np.array_equal(d_canvas.cpu().numpy(), held)


def test_masked_tiles(ctx):
    """Marked tiles only, flat and varying ones among them: tiles 0 and 3 are flat, 1 and 8 vary; nothing else is written."""
    s = ctx[False]
    img = two_constants(255, 0, seed=50)
    flags = AF.varies(img, T, P)
    mask = np.zeros(18, dtype=np.uint8)
    mask[[0, 1, 3, 8]] = 1
    assert flags[[0, 1, 3, 8]].tolist() == [0, 1, 0, 1]
    d_in = dev(img)

    def masked():
        d_out = filled((4 * H * 4 * W * 4,), U8)
        s.process_device_masked(d_in.data_ptr(), U8, W, H, 4, d_out.data_ptr(), U8, mask)
        torch.cuda.synchronize()
        return d_out.cpu().numpy().reshape(4 * H, 4 * W, 4)
    o0, o1, oa, ran, flat = modes(s, masked)
    assert (ran, flat) == (2, 2)
    full = AF.select(flags, o0, o1, W, H, T)
    want = np.full(full.shape, 0xCD, dtype=np.uint8)
    for t in np.flatnonzero(mask):
        x0, y0, x1, y1 = ref.out_rect(W, H, T, int(t))
        want[y0:y1, x0:x1] = full[y0:y1, x0:x1]
    assert np.array_equal(oa, want) and not np.array_equal(oa, o1) and not np.array_equal(oa, o0)


def test_sequence_of_two_frames(ctx):
    """Frame 1 differs from frame 0 in one alpha sample of a flat region: its marked tiles now vary, and the copied ones keep frame 0's
    bytes, flat or not."""
    s = ctx[False]
    a = two_constants(255, 0, seed=60)
    b = a.copy()
    b[43, 80, 3] = 3   # inside the source rectangles of tiles (2, 4) and (2, 5) alone
    fa, fb = AF.varies(a, T, P), AF.varies(b, T, P)
    mark = ref.diff_mask(U8, a, b, T, P)
    assert mark.sum() == 2 and fb.sum() == fa.sum() + 2
    masks = np.concatenate([np.ones(18, np.uint8), mark])
    d_f = [dev(a), dev(b)]

    def sequence():
        d_outs = [filled((4 * H * 4 * W * 4,), U8) for _ in range(2)]
        s.process_device_sequence([t.data_ptr() for t in d_f], U8, W, H, 4, [t.data_ptr() for t in d_outs], U8, masks)
        torch.cuda.synchronize()
        return [t.cpu().numpy().reshape(4 * H, 4 * W, 4) for t in d_outs]
    o0, o1, oa, ran, flat = modes(s, sequence)
    assert (ran, flat) == (int(fa.sum()) + 2, int((fa == 0).sum()))
    assert np.array_equal(oa[0], AF.select(fa, o0[0], o1[0], W, H, T))
    assert np.array_equal(oa[1], AF.select(fb, o0[1], o1[1], W, H, T))
    assert not np.array_equal(oa[1], oa[0])


def test_four_threads_merged(ctx):
    """Four concurrent rsr_process calls on small images of different sizes with "merge" 16: whether or not their tiles shared a batch, each
    image follows the rule."""
    s = ctx[False]
    imgs = [two_constants(255, 0, w=45, h=18, seed=70), constant(77, w=20, h=18, seed=71), rgba(w=13, h=22, seed=72), two_constants(128, 77, w=50, h=9, seed=73)]
    flags = [AF.varies(x, T, P) for x in imgs]
    assert [int(f.sum()) for f in flags] == [4, 0, 2, 2] and [f.size for f in flags] == [6, 4, 2, 4]
    s.set_option("merge", 16)

    def all_four():
        got = [None] * len(imgs)
        errs = []

        def work(k):
            try:
                got[k] = s.process(imgs[k], push_params=False)
            except Exception as e:  # noqa: BLE001
                errs.append(e)
        ths = [threading.Thread(target=work, args=(k,)) for k in range(len(imgs))]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        assert not errs, errs
        return got
    o0, o1, oa, ran, flat = modes(s, all_four)
    assert (ran, flat) == (8, 8)
    for k, x in enumerate(imgs):
        assert np.array_equal(oa[k], AF.select(flags[k], o0[k], o1[k], x.shape[1], x.shape[0], T)), k


def test_second_batch_forced_by_the_workspace_budget(ctx):
    """max_workspace_mb 1 cuts the 18 tiles into several batches: one scan and one wait per batch, the same bytes."""
    s = ctx[False]
    img = two_constants(255, 0, seed=80)
    _, whole = check(s, img)
    s.set_option("max_workspace_mb", 1)
    s.alpha_net, s.alpha_adaptive = 1, 1
    got, prof = profile_of(s, lambda: call(s, img))
    assert np.array_equal(got, whole)
    # 18 colour tiles and 6 alpha tiles went through the network in more than one batch: more conv launches than two passes of one batch
    assert prof["conv_launches"] > 2 * R.NUM_CONVS and prof["conv_launches"] % R.NUM_CONVS == 0


# ---- 4. inertness -------------------------------------------------------------------------------------------------------------------------------
STAT_KEYS = ("alpha_net", "alpha_tiles", "alpha_tiles_flat", "alpha_wait_us")
PROFILE_KEYS = ("conv_launches", "calls", "tiles", "pre_bytes", "post_bytes", "conv_flops")


@pytest.mark.parametrize("c", [4, 3], ids=["rgba-alpha_net-0", "rgb"])
def test_inert_without_an_alpha_pass(ctx, c):
    """alpha_adaptive 1 with alpha_net 0, and with a c == 3 call under alpha_net 1: bytes, stats and the launch list of the parent path."""
    s = ctx["other"]
    img = np.ascontiguousarray(two_constants(255, 0, seed=90)[:, :, :c])
    s.alpha_net = int(c == 3)
    got0, p0 = profile_of(s, lambda: call(s, img))
    stats0 = [s.get_stat(k) for k in STAT_KEYS]
    s.alpha_adaptive = 1
    assert s.get_stat("alpha_adaptive") == 1
    got1, p1 = profile_of(s, lambda: call(s, img))
    assert np.array_equal(got0, got1)
    assert [p0[k] for k in PROFILE_KEYS] == [p1[k] for k in PROFILE_KEYS] and p0["conv_launches"] == R.NUM_CONVS
    assert [s.get_stat(k) for k in STAT_KEYS] == stats0


def test_the_scan_counts_as_preprocessing(ctx):
    """Profiled, the adaptive call on an all-varying image is the alpha_net 1 call plus the scan's bytes in the preprocessing class."""
    s = ctx[False]
    img = rgba(seed=91)
    s.alpha_net = 1
    _, p1 = profile_of(s, lambda: call(s, img))
    s.alpha_adaptive = 1
    _, pa = profile_of(s, lambda: call(s, img))
    assert pa["conv_launches"] == p1["conv_launches"] == 2 * R.NUM_CONVS and pa["post_bytes"] == p1["post_bytes"]
    assert pa["pre_bytes"] > p1["pre_bytes"] and s.get_stat("alpha_wait_us") > 0


def test_refusals(ctx):
    s = ctx[False]
    for keep in (0, 1):
        s.alpha_adaptive = keep
        for bad in (2, -1):
            with pytest.raises(R.RealSRError) as e:
                s.alpha_adaptive = bad
            assert e.value.code == R.RSR_E_ARG
            with pytest.raises(R.RealSRError) as e:
                s.set_option("alpha_adaptive", bad)
            assert e.value.code == R.RSR_E_ARG
            assert s.alpha_adaptive == keep and s.get_stat("alpha_adaptive") == keep


def test_group_members_must_agree(ctx):
    a, b = ctx[False], ctx["other"]
    img = two_constants(255, 0, seed=92)
    a.alpha_net = b.alpha_net = 1
    a.alpha_adaptive = 1
    with pytest.raises(R.RealSRError) as e:
        R.process_group([a, b], img)
    assert e.value.code == R.RSR_E_ARG and "alpha_adaptive" in str(e.value)
    b.alpha_adaptive = 1
    flags = AF.varies(img, T, P)
    got = R.process_group([a, b], img)
    a.alpha_adaptive = b.alpha_adaptive = 0
    net = a.process(img)
    a.alpha_net = 0
    assert np.array_equal(got, AF.select(flags, a.process(img), net, W, H, T))
