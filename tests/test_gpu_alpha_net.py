"""Option "alpha_net" on the GPU (run with -m gpu): the alpha of an RGBA image through the network.

The definition of include/realsr_hip.h ("alpha through the network") ties the alpha samples to the library's OWN planar fp32 output for the
gray image G of the alpha (tests/alpha_net_ref.py restates the three steps behind it in numpy), and item 9 ties them to the two-term exact
model of tests/exact_net.py, which owes the library nothing.  Every comparison is np.array_equal.  Tile 16, prepadding 10; the main image is
35 x 25: 3 x 2 tiles, partial at both far edges.  Destinations are pre-filled with 0xCD."""
import os
import threading
from fractions import Fraction

import numpy as np
import pytest
import torch

import alpha_net_ref as A
import exact_net as N
import realsr_ncnn_vulkan_amd as R
import rgb16_ref as Z
import tile_diff_ref as ref
from gpu_support import context_fixtures, dev, filled, paths, profile_of, run, untouched  # noqa: F401
from pixfmt_ref import F32, U8
from realsr_ncnn_vulkan_amd import synth

pytestmark = pytest.mark.gpu
U16 = R.RSR_FMT_U16_HWC
W, H, T, P = 35, 25, 16, 10
BITS = {U8: 8, U16: 16}
ctxs, ctx = context_fixtures(T, P, others=("rgb",))   # "rgb": a context no RGBA image ever sees (item 7)


@pytest.fixture(autouse=True)
def alpha_net_off(ctxs):
    """gpu_support.DEFAULTS does not know the option: 0 before and after every test of this module."""
    for s in ctxs.values():
        s.alpha_net = 0
    yield
    for s in ctxs.values():
        s.alpha_net = 0


def call(s, x, in_fmt, out_fmt):
    """One synchronous rsr_process_device_fmt call on the packed numpy image x (U8 / U16 HWC, or planar F32 out)."""
    if in_fmt == U8 and out_fmt in (U8, F32):
        return run(s, x, in_fmt, out_fmt)
    w, h, c = x.shape[1], x.shape[0], x.shape[2]
    ow, oh = s.out_size_fmt(out_fmt, w, h)
    oshape = Z.shape_of(out_fmt, ow, oh, c)
    d_in, d_out = dev(x), dev(Z.sentinel_bytes(out_fmt, oshape))
    assert d_out.numel() == R.image_bytes(out_fmt, ow, oh, c)
    s.process_device_fmt(d_in.data_ptr(), in_fmt, w, h, c, d_out.data_ptr(), out_fmt)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(Z.np_dtype(out_fmt)).reshape(oshape)


def rgba(fmt=U8, w=W, h=H, seed=7):
    """A seeded RGBA image whose alpha holds, from top to bottom: a ramp over the whole range, a band with a hard edge between a block of 0
    and a block of the maximum, and seeded noise."""
    top = 65535 if fmt == U16 else 255
    rng = np.random.default_rng(seed)
    img = rng.integers(0, top + 1, size=(h, w, 4)).astype(Z.np_dtype(fmt))
    a = img[:, :, 3]
    a[:h // 3, :] = (np.arange(w) * top // max(w - 1, 1))[None, :]
    a[h // 3:2 * h // 3, :w // 2] = 0
    a[h // 3:2 * h // 3, w // 2:] = top
    return img


def alpha_want(s, img, in_fmt, out_fmt):
    """alpha_net_ref of the F32_CHW output of the library's own call on G, "bgr" 0, in the context's current mode and scale."""
    before = s.get_stat("alpha_net"), s.get_stat("alpha_tiles")
    s.set_option("bgr", 0)
    planes = call(s, A.gray(img), in_fmt, F32)
    assert (s.get_stat("alpha_net"), s.get_stat("alpha_tiles")) == before   # (a c == 3 call runs no alpha pass)
    assert planes.dtype == np.float32 and planes.min() >= 0 and planes.max() <= 1
    return A.alpha(planes, BITS[out_fmt])


def check(s, img, in_fmt=U8, out_fmt=U8, varied=True):
    """The definition: colour as at alpha_net 0, alpha from the network.  Returns the alpha_net 1 image."""
    assert s.alpha_net == 0
    base = call(s, img, in_fmt, out_fmt)
    want = alpha_want(s, img, in_fmt, out_fmt)
    tiles0 = s.get_stat("alpha_tiles")
    s.alpha_net = 1
    assert s.alpha_net == 1 and s.get_stat("alpha_net") == 1
    got = call(s, img, in_fmt, out_fmt)
    s.alpha_net = 0
    nx, ny = s.tile_count(img.shape[1], img.shape[0])
    assert s.get_stat("alpha_tiles") == tiles0 + nx * ny
    assert got.shape == base.shape and got.dtype == base.dtype and got.shape[2] == 4
    assert np.array_equal(got[:, :, :3], base[:, :, :3])
    ga = got[:, :, 3]
    nd = int((ga != want).sum())
    print("alpha_net u%d -> u%d %dx%d: %d of %d alpha samples differ from the definition%s" % (
        BITS[in_fmt], BITS[out_fmt], img.shape[1], img.shape[0], nd, ga.size, "" if not nd else ", max |diff| %d" % np.abs(ga.astype(int) - want.astype(int)).max()))
    assert np.array_equal(ga, want)
    if varied:
        assert len(np.unique(ga)) > 8 and not np.array_equal(ga, base[:, :, 3])   # (the network's alpha, not the bicubic)
    return got


# ---- 1. the definition ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precise", [0, 1], ids=["fp16", "precise"])
@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_definition(ctx, tta, precise):
    s = ctx[tta]
    s.set_option("precise", precise)
    got = check(s, rgba())
    assert got.shape == (4 * H, 4 * W, 4)


# ---- 2. scales --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
@pytest.mark.parametrize("scale", [2, 1], ids=["x2", "x1"])
def test_out_scale(ctx, scale, tta):
    s = ctx[tta]
    s.out_scale = scale
    assert check(s, rgba()).shape == (scale * H, scale * W, 4)


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_ratio_3_2(ctx, tta):
    s = ctx[tta]
    s.out_ratio = Fraction(3, 2)
    assert check(s, rgba(w=36, h=26)).shape == (39, 54, 4)


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_pair_8_3_and_9_4(ctx, tta):
    s = ctx[tta]
    s.tilesize = 24
    s.out_ratio_xy = (Fraction(8, 3), Fraction(9, 4))
    assert check(s, rgba(w=36, h=28)).shape == (63, 96, 4)


# ---- 3. depths --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precise", [0, 1], ids=["fp16", "precise"])
@pytest.mark.parametrize("pair", [(U16, U16), (U8, U16), (U16, U8)], ids=["u16-u16", "u8-u16", "u16-u8"])
def test_depths(ctx, pair, precise):
    """G is read at the source's depth, m stored at the destination's: no x257 or 1/257 step."""
    s = ctx[False]
    s.set_option("precise", precise)
    in_fmt, out_fmt = pair
    got = check(s, rgba(in_fmt, seed=11), in_fmt, out_fmt)
    assert got.dtype == Z.np_dtype(out_fmt)


def test_depths_reduced_and_tta(ctx):
    s = ctx[True]
    s.out_scale = 2
    check(s, rgba(U16, seed=12), U16, U16)


# ---- 4. bgr -----------------------------------------------------------------------------------------------------------------------------
def test_bgr_does_not_change_the_alpha(ctx):
    s = ctx[False]
    img = rgba(seed=13)
    plain = check(s, img)
    s.set_option("bgr", 1)
    s.alpha_net = 1
    swapped = call(s, img, U8, U8)
    assert np.array_equal(swapped[:, :, 3], plain[:, :, 3])
    s.alpha_net = 0
    assert np.array_equal(swapped[:, :, :3], call(s, img, U8, U8)[:, :, :3])   # (check() set "bgr" 0 for G: back to 1 here)
    assert not np.array_equal(swapped[:, :, :3], plain[:, :, :3])


# ---- 5. geometry ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,pad", [(1, 1, P), (7, 9, P), (40, 1, P), (33, 17, 0)], ids=["1x1", "7x9", "40x1", "33x17-pad0"])
def test_geometry(ctx, w, h, pad):
    """One pixel; an image below the halo; one row over three tiles; no halo at all."""
    s = ctx[False]
    s.prepadding = pad
    img = rgba(w=w, h=h, seed=20 + w)
    if (w, h) == (1, 1):
        img[0, 0, 3] = 140
    check(s, img, varied=w * h > 64)


# ---- 6. entry points --------------------------------------------------------------------------------------------------------------------
def lone(s, img, in_fmt=U8, out_fmt=U8):
    s.alpha_net = 1
    return call(s, img, in_fmt, out_fmt)


def test_host_calls(ctx):
    """rsr_process and rsr_process_fmt give the device call's bytes."""
    s = ctx[False]
    img = rgba(seed=30)
    want = lone(s, img)
    assert np.array_equal(s.process(img), want)
    img16 = rgba(U16, seed=31)
    want16 = lone(s, img16, U16, U16)
    got16 = s.process_fmt(img16, U16, U16)
    assert got16.dtype == np.uint16 and np.array_equal(got16, want16)
    assert np.array_equal(s.process_fmt(img, U8, U8), want)


def test_torch_entry_points(ctx):
    """torch_io.upscale on (H, W, 4) uint8 / int16 tensors and upscale_delta honour the option with no code of their own."""
    from realsr_ncnn_vulkan_amd import torch_io
    s = ctx[False]
    img, img16 = rgba(seed=35), rgba(U16, seed=36)
    want, want16 = lone(s, img), lone(s, img16, U16, U16)
    assert np.array_equal(torch_io.upscale(s, torch.from_numpy(img).cuda()).cpu().numpy(), want)
    assert np.array_equal(torch_io.upscale(s, torch.from_numpy(img16.view(np.int16)).cuda()).cpu().numpy().view(np.uint16), want16)
    nxt = img.copy()
    nxt[3, 2, 3] ^= 0x40
    y, ran = torch_io.upscale_delta(s, torch.from_numpy(nxt).cuda(), torch.from_numpy(img).cuda(), torch.from_numpy(want).cuda())
    assert ran == 1 and np.array_equal(y.cpu().numpy(), lone(s, nxt))


def test_batch_of_two_pitched_windows(ctx):
    """Two images in ONE rsr_process_device_batch call, each into a window of a 0xCD canvas: the lone calls' bytes, nothing outside."""
    s = ctx[False]
    imgs = [rgba(seed=40 + i) for i in range(2)]
    wants = [lone(s, x) for x in imgs]
    ow, oh = 4 * W, 4 * H
    opitch, ooff = ow * 4 + 3, 2 * (ow * 4 + 3) + 5 * 4 + 1   # an odd pitch, an odd byte offset
    ospan = R.image_span(U8, ow, oh, 4, opitch, 0)
    d_ins = [dev(x) for x in imgs]
    d_outs = [filled((ooff + ospan + 64,), U8) for _ in imgs]
    tiles0 = s.get_stat("alpha_tiles")
    s.process_device_batch([t.data_ptr() for t in d_ins], U8, W, H, 4, [(t.data_ptr() + ooff, opitch, 0) for t in d_outs], U8)
    torch.cuda.synchronize()
    assert s.get_stat("alpha_tiles") == tiles0 + 12
    for d_out, want in zip(d_outs, wants):
        got = d_out.cpu().numpy()
        inside = np.zeros(got.shape, dtype=bool)
        rows = want.reshape(oh, -1)
        for r in range(oh):
            o = ooff + r * opitch
            assert np.array_equal(got[o:o + rows.shape[1]], rows[r]), r
            inside[o:o + rows.shape[1]] = True
        assert (got[~inside] == 0xCD).all() and inside.sum() == want.nbytes


def test_masked_tiles(ctx):
    """Two of six tiles set: only their rectangles change, alpha included, and exactly two tiles ran the alpha pass."""
    s = ctx[False]
    img = rgba(seed=50)
    full = lone(s, img)
    assert s.tile_count(W, H) == (3, 2)
    mask = np.array([0, 1, 0, 0, 0, 1], dtype=np.uint8)
    d_in, d_out = dev(img), filled((full.nbytes,), U8)
    tiles0 = s.get_stat("alpha_tiles")
    s.process_device_masked(d_in.data_ptr(), U8, W, H, 4, d_out.data_ptr(), U8, mask)
    torch.cuda.synchronize()
    assert s.get_stat("alpha_tiles") == tiles0 + 2
    want = np.full(full.shape, 0xCD, dtype=np.uint8)
    for t in np.flatnonzero(mask):
        x0, y0, x1, y1 = ref.out_rect(W, H, T, t)
        want[y0:y1, x0:x1] = full[y0:y1, x0:x1]
    got = d_out.cpu().numpy().reshape(full.shape)
    assert np.array_equal(got, want) and not np.array_equal(got, full)
    d_none = filled((full.nbytes,), U8)
    s.process_device_masked(d_in.data_ptr(), U8, W, H, 4, d_none.data_ptr(), U8, np.zeros(6, np.uint8))
    torch.cuda.synchronize()
    assert untouched(d_none) and s.get_stat("alpha_tiles") == tiles0 + 2


def test_sequence_of_two_frames(ctx):
    """The second frame differs from the first in ONE alpha sample: the diff marks the tiles whose source rectangle holds it, the sequence
    call runs them alone, and both outputs equal the lone calls."""
    s = ctx[False]
    a = rgba(seed=60)
    b = a.copy()
    b[3, 2, 3] ^= 0x40   # near the first corner: inside the source rectangle of the first tile only (the next ones begin at 16 - 10)
    wants = [lone(s, a), lone(s, b)]
    assert not np.array_equal(wants[0][:, :, 3], wants[1][:, :, 3]) and np.array_equal(wants[0][:, :, :3], wants[1][:, :, :3])
    d_f = [dev(a), dev(b)]
    d_masks = filled((12,), U8)
    s.diff_tiles_sequence([t.data_ptr() for t in d_f], None, U8, W, H, 4, d_masks.data_ptr())
    torch.cuda.synchronize()
    masks = d_masks.cpu().numpy().reshape(2, 6)
    mark = np.array([int(r[0] <= 2 < r[2] and r[1] <= 3 < r[3]) for r in (ref.source_rect(W, H, T, P, t) for t in range(6))], dtype=np.uint8)
    assert np.array_equal(masks[0], np.ones(6, np.uint8)) and np.array_equal(masks[1], mark) and mark.sum() == 1 and mark[0] == 1
    d_outs = [filled((wants[0].nbytes,), U8) for _ in range(2)]
    tiles0 = s.get_stat("alpha_tiles")
    s.process_device_sequence([t.data_ptr() for t in d_f], U8, W, H, 4, [t.data_ptr() for t in d_outs], U8, masks.reshape(-1))
    torch.cuda.synchronize()
    assert s.get_stat("alpha_tiles") == tiles0 + 6 + int(mark.sum())
    for k in range(2):
        assert np.array_equal(d_outs[k].cpu().numpy().reshape(wants[k].shape), wants[k]), k


def test_two_threads_merged(ctx):
    """Two threads calling rsr_process on small RGBA images with "merge" 16: whether or not their tiles shared a batch, the lone calls' bytes."""
    s = ctx[False]
    imgs = [rgba(w=20, h=18, seed=70), rgba(w=20, h=18, seed=71), rgba(w=13, h=22, seed=72), rgba(w=13, h=22, seed=73)]
    wants = [lone(s, x) for x in imgs]
    s.set_option("merge", 16)
    got = [None] * len(imgs)
    errs = []

    def work(k):
        try:
            for i in range(k, len(imgs), 2):
                got[i] = s.process(imgs[i], push_params=False)
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ths = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs, errs
    for g, w_ in zip(got, wants):
        assert np.array_equal(g, w_)


# ---- 7. c == 3 is not concerned -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dbg", [0, 8192], ids=["fused", "unfused"])
def test_rgb_calls_are_untouched(ctx, dbg):
    s = ctx["rgb"]
    s.set_option("dbg", dbg)
    img = np.ascontiguousarray(rgba(seed=80)[:, :, :3])
    keys = ("conv_launches", "calls", "tiles", "pre_bytes", "post_bytes", "conv_flops")
    got0, p0 = profile_of(s, lambda: call(s, img, U8, U8))
    s.alpha_net = 1
    got1, p1 = profile_of(s, lambda: call(s, img, U8, U8))
    assert np.array_equal(got0, got1)
    assert [p0[k] for k in keys] == [p1[k] for k in keys] and p0["conv_launches"] == R.NUM_CONVS and (p1["post_ms"] > 0) == (dbg != 0)
    assert s.get_stat("alpha_tiles") == 0


def test_rgba_runs_the_network_twice(ctx):
    """The cost, as the profile sees it: twice the conv launches and FLOPs, one progress call per tile."""
    s = ctx[False]
    img = rgba(seed=81)
    _, p0 = profile_of(s, lambda: call(s, img, U8, U8))
    s.alpha_net = 1
    _, p1 = profile_of(s, lambda: call(s, img, U8, U8))
    assert p0["conv_launches"] == R.NUM_CONVS and p1["conv_launches"] == 2 * R.NUM_CONVS and abs(p1["conv_flops"] - 2 * p0["conv_flops"]) <= 1e-9 * p1["conv_flops"]
    assert p1["calls"] == 1 and p1["tiles"] == p0["tiles"] and p1["post_bytes"] > p0["post_bytes"] and p1["pre_bytes"] > p0["pre_bytes"]


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    s = ctx[False]
    for keep in (0, 1):
        s.alpha_net = keep
        for bad in (2, -1):
            with pytest.raises(R.RealSRError) as e:
                s.alpha_net = bad
            assert e.value.code == R.RSR_E_ARG
            with pytest.raises(R.RealSRError) as e:
                s.set_option("alpha_net", bad)
            assert e.value.code == R.RSR_E_ARG
            assert s.alpha_net == keep and s.get_stat("alpha_net") == keep


# ---- 9. independent of the library's RGB route ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exact_model():
    return N.make_model()


@pytest.fixture(scope="module")
def exact_ctx(exact_model, tmp_path_factory):
    """The two-term exact model of tests/exact_net.py in a model directory of its own, as tests/test_gpu_exact_net.py builds it."""
    d = str(tmp_path_factory.mktemp("alpha_net_exact"))
    synth.write_param(os.path.join(d, "x4.param"))
    synth.write_bin(os.path.join(d, "x4.bin"), N.dense_weights(exact_model), "fp16")
    s = R.RealSR(0)
    s.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
    s.tilesize, s.prepadding = T, P
    yield s
    s.close()


@pytest.mark.parametrize("precise", [False, True], ids=["fp16", "precise"])
def test_against_the_exact_model(exact_ctx, exact_model, precise):
    """The alpha bytes against the numpy mirror of the whole network on G -- no call of the library on G is involved."""
    s = exact_ctx
    img = N.frame_u8(W, H, 4)
    want = A.alpha(N.to_unit(N.image_x4(exact_model, N.halfs_of_u8(A.gray(img)), T, precise=precise)), 8)
    assert len(np.unique(want)) > 50
    s.set_option("precise", int(precise))
    s.alpha_net = 1
    try:
        got = s.process(img)
        nd = int((got[:, :, 3] != want).sum())
        print("exact model, precise=%s: %d of %d alpha samples differ" % (precise, nd, want.size))
        assert got.shape == (4 * H, 4 * W, 4) and np.array_equal(got[:, :, 3], want)
        rgb = N.to_u8(N.image_x4(exact_model, N.halfs_of_u8(img), T, precise=precise)) if not precise else None
        if rgb is not None:   # (the colour route beside it, as tests/test_gpu_exact_net.py holds it)
            assert np.array_equal(got[:, :, :3], np.ascontiguousarray(rgb.transpose(1, 2, 0)))
    finally:
        s.alpha_net = 0
        s.set_option("precise", 0)
