"""Rational output scales on the GPU (run with -m gpu): rsr_set_out_ratio -- x3, x3/2, x4/3, x9/4 ... area-averaged on the device
(include/realsr_hip.h, "The definition, exact").

The contract is exact, and every comparison is against the SAME context's F32_CHW output at out_scale 4, reduced by area_reduce
(tests/area_reduce.py: float32, the stated order), bit for bit: F32 matches with no tolerance; F16 is that rounded once; uint8 is
floor(m * 255 + 0.5), compared against the exact evaluation except where it lies within 2^-14 of an integer (check_u8, the rule of
tests/test_gpu_out_scale.py: those elements must be within 1, and at most 1e-3 of the elements may be left out; every uint8 comparison
covers at least 20,000 elements -- where one image of a case is smaller, two images are pooled).  Every entry point gives the same bytes.
Outputs are pre-filled with NaN / 0xCD."""
import ctypes as C
import os
import subprocess
import threading
from fractions import Fraction

import numpy as np
import pytest
import torch

import oracle
import realsr_ncnn_vulkan_amd as R
import yuv_ref
from realsr_ncnn_vulkan_amd import torch_io

import gpu_support as G
from area_reduce import GENERIC, area_reduce, check_u8
from gpu_support import context_fixtures, filled, paths, untouched  # noqa: F401
from pixfmt_ref import F16, F32, NV12, U8, bits, halfs, u8_image as image

pytestmark = pytest.mark.gpu
ctxs, back_to_defaults = context_fixtures(autouse=True)


def run(s, x, in_fmt, out_fmt, ratio):
    """One synchronous rsr_process_device_fmt call at output ratio `ratio` on the packed numpy image x; the result as a numpy array."""
    s.out_ratio = ratio
    assert s.out_ratio == (Fraction(*ratio) if isinstance(ratio, tuple) else Fraction(ratio))
    return G.run(s, x, in_fmt, out_fmt, nan=True)


def check_formats(s, n, d, w, h, seed, pool=1):
    """F32, F16 and uint8 at n / d against area_reduce of the context's own x4 F32 output; `pool` images share the uint8 comparison."""
    gots, refs = [], []
    for k in range(pool):
        img = image(seed + k, w, h)
        ref = run(s, img, U8, F32, 4)
        assert ref.shape == (3, 4 * h, 4 * w) and ref.min() >= 0 and ref.max() <= 1
        m = area_reduce(ref, n, d)
        got = run(s, img, U8, F32, (n, d))
        assert got.shape == (3, h * n // d, w * n // d) and s.get_stat("out_scale") == 0
        nd = int((bits(got) != bits(m)).sum())
        print("%d/%d: F32 %d of %d elements differ in bits" % (n, d, nd, m.size))
        assert nd == 0
        assert np.array_equal(bits(run(s, img, U8, F16, (n, d))), bits(m.astype(np.float16)))  # rounded once, to nearest even
        gots.append(run(s, img, U8, U8, (n, d)))
        refs.append(m)
    check_u8(gots, refs, "%d/%d: " % (n, d))


# ---- 1. every generic ratio ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", GENERIC, ids=["%d-%d" % r for r in GENERIC])
def test_every_generic_ratio(ctxs, nd):
    """84 x 60 at tile 36: all three are multiples of 12, so every d divides them; a 3 x 2 tile grid whose last tiles are 12 wide, 24 high."""
    s = ctxs[False]
    s.tilesize = 36
    check_formats(s, nd[0], nd[1], 84, 60, 7100)


# ---- 2. modes ------------------------------------------------------------------------------------------------------------------------
MODES = [(3, 2, 62, 46, 32), (4, 3, 63, 48, 33)]


@pytest.mark.parametrize("precise", [0, 1], ids=["fp16", "precise"])
@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
@pytest.mark.parametrize("case", MODES, ids=["%d-%d_%dx%d-T%d" % c for c in MODES])
def test_modes(ctxs, case, tta, precise):
    n, d, w, h, T = case  # 62 x 46 at tile 32: partial tiles 30 and 14; 63 x 48 at tile 33: 30 and 15
    s = ctxs[tta]
    s.tilesize = T
    s.set_option("precise", precise)
    check_formats(s, n, d, w, h, 7200 + w, pool=2)


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
@pytest.mark.parametrize("nd", [(5, 4), (15, 4)], ids=["5-4", "15-4"])
def test_longest_and_shortest_footprint(ctxs, nd, tta):
    s = ctxs[tta]
    s.tilesize = 32
    check_formats(s, nd[0], nd[1], 60, 44, 7300, pool=2)


# ---- 3. alpha, bgr -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tta,precise", [(False, 0), (True, 0), (False, 1)], ids=["plain", "tta", "precise"])
def test_alpha_is_the_area_mean_of_the_x4_alpha(ctxs, tta, precise):
    """Alpha at 3/2: the reference applied to the x4 path's alpha -- the bicubic x4 of every tile's un-padded alpha rectangle
    (oracle.bicubic, the arithmetic behind the x4 path's alpha byte), clamped to [0, 255] -- and stored as floor(mean + 0.5): +-0 outside
    the elements whose mean + 0.5 lies within 2^-10 of an integer, +-1 there.  The band: a 4 x 4-tap bicubic value of bytes <= 255 with
    sum |coefficient| <= 1.4 per axis carries at most gamma_12 * 255 * 1.4^2 = 3.6e-4 of fp32 rounding in either evaluation (the engine's
    may be contracted, the oracle's is not), the weighted mean 10 * 2^-24 * 255 = 1.5e-4 more: 8.7e-4 < 2^-10."""
    w, h, T = 62, 46, 32
    s = ctxs[tta]
    s.tilesize = T
    s.set_option("precise", precise)  # (the blob is fp32 then: the kernels' <float, uint8_t, ., true> instances)
    img = image(7400, w, h, 4)
    full = run(s, img, U8, U8, 4)
    a4 = np.empty((4 * h, 4 * w), dtype=np.float32)
    for y0 in range(0, h, T):
        for x0 in range(0, w, T):
            th, tw = min(y0 + T, h) - y0, min(x0 + T, w) - x0
            a4[4 * y0:4 * (y0 + th), 4 * x0:4 * (x0 + tw)] = oracle.bicubic(img[y0:y0 + th, x0:x0 + tw, 3].astype(np.float32), 4 * th, 4 * tw)
    assert np.abs(np.clip(np.floor(a4 + 0.5), 0, 255) - full[:, :, 3]).max() <= 1  # (it IS the x4 path's alpha)
    got = run(s, img, U8, U8, (3, 2))
    assert got.shape == (69, 93, 4)
    E = area_reduce(a4, 3, 2, top=255.0).astype(np.float64) + 0.5
    near = np.abs(E - np.rint(E)) < 2.0 ** -10
    want = np.clip(np.floor(E), 0, 255).astype(np.uint8)
    ga = got[:, :, 3]
    print("alpha at 3/2: %d elements, %d left out (within 2^-10 of a rounding boundary), %d differ" % (ga.size, near.sum(), ((ga != want) & ~near).sum()))
    assert near.mean() <= 1e-2
    assert np.array_equal(ga[~near], want[~near])
    assert (np.abs(ga.astype(int) - want.astype(int))[near] <= 1).all()
    assert np.array_equal(got[:, :, :3], run(s, np.ascontiguousarray(img[:, :, :3]), U8, U8, (3, 2)))  # RGB as without alpha
    for a in (0, 255):
        flat = img.copy()
        flat[:, :, 3] = a
        assert (run(s, flat, U8, U8, (3, 2))[:, :, 3] == a).all(), a


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_bgr_swaps_channels_of_the_reduced_image(ctxs, tta):
    w, h, T = 62, 46, 32
    s = ctxs[tta]
    s.tilesize = T
    img = image(7500, w, h)
    planar = np.ascontiguousarray((img.astype(np.float32) * np.float32(1 / 255.0)).transpose(2, 0, 1)).astype(np.float16)
    rgb8, rgbf = run(s, img, U8, U8, (3, 2)), run(s, planar, F16, F32, (3, 2))
    rgba = run(s, image(7501, w, h, 4), U8, U8, (3, 2))
    s.set_option("bgr", 1)
    bgr8 = run(s, np.ascontiguousarray(img[:, :, ::-1]), U8, U8, (3, 2))
    bgrf = run(s, np.ascontiguousarray(planar[::-1]), F16, F32, (3, 2))
    bgra = run(s, np.ascontiguousarray(image(7501, w, h, 4)[:, :, [2, 1, 0, 3]]), U8, U8, (3, 2))
    assert np.array_equal(bgr8[:, :, ::-1], rgb8) and not np.array_equal(bgr8, rgb8)
    assert np.array_equal(bits(np.ascontiguousarray(bgrf[::-1])), bits(rgbf))
    assert np.array_equal(bgra[:, :, [2, 1, 0, 3]], rgba)


# ---- 4. other inputs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_f16_input_the_uint8_path_cannot_make(ctxs, tta):
    w, h = 62, 46
    s = ctxs[tta]
    s.tilesize = 32
    hx = halfs(7600, w, h)
    ref = run(s, hx, F16, F32, 4)
    assert not np.array_equal(ref, run(s, image(7600, w, h), U8, F32, 4))
    for n, d in ((3, 2), (5, 2), (3, 1)):
        m = area_reduce(ref, n, d)
        assert np.array_equal(bits(run(s, hx, F16, F32, (n, d))), bits(m))
        assert np.array_equal(bits(run(s, hx, F16, F16, (n, d))), bits(m.astype(np.float16)))
    x32 = hx.astype(np.float32)
    assert np.array_equal(bits(run(s, x32, F32, F32, (3, 2))), bits(area_reduce(ref, 3, 2)))


def test_nv12_input_to_f32_output(ctxs):
    """The input side is independent of the output side: an NV12 surface in, F32 out at 3/2."""
    w, h = 62, 46
    s = ctxs[False]
    s.tilesize = 32
    surf = np.random.default_rng(7700).integers(0, 256, size=(h * 3 // 2, w)).astype(np.uint8)
    d_in = torch.from_numpy(surf).cuda()

    def call(ratio):
        s.out_ratio = ratio
        ow, oh = s.out_size(w, h)
        d_out = filled((3, oh, ow), F32)
        s.process_device_fmt(d_in.data_ptr(), NV12, w, h, 3, d_out.data_ptr(), F32)
        torch.cuda.synchronize()
        return d_out.cpu().numpy()
    ref = call(4)
    assert not np.isnan(ref).any()
    assert np.array_equal(bits(ref), bits(run(s, yuv_ref.decode(*yuv_ref.split(surf, 8), 709, 0, 8), F32, F32, 4)))  # (the input tie of tests/test_gpu_yuv.py)
    assert np.array_equal(bits(call((3, 2))), bits(area_reduce(ref, 3, 2)))


# ---- 5. batches and windows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_batch_of_five_equals_lone_calls(ctxs, tta):
    w, h, T = 62, 46, 32
    s = ctxs[tta]
    s.tilesize = T
    for in_fmt, out_fmt in ((U8, U8), (F16, F32)):
        xs = [image(7800 + i, w, h) if in_fmt == U8 else halfs(7800 + i, w, h) for i in range(5)]
        want = [run(s, x, in_fmt, out_fmt, (3, 2)) for x in xs]
        d_in = [torch.from_numpy(x).cuda() for x in xs]
        d_out = [filled(want[0].shape, out_fmt) for _ in xs]
        torch.cuda.synchronize()
        g0 = s.get_stat("batch_groups")
        s.process_device_batch([t.data_ptr() for t in d_in], in_fmt, w, h, 3, [t.data_ptr() for t in d_out], out_fmt)
        torch.cuda.synchronize()
        assert s.get_stat("batch_groups") == g0 + 1  # ONE merged group
        for i in range(5):
            assert np.array_equal(d_out[i].cpu().numpy().view(np.uint8), want[i].view(np.uint8)), (in_fmt, i)


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_upscale_a_crop_into_a_3_over_2_window(ctxs, tta):
    s = ctxs[tta]
    s.tilesize = 32
    s.out_ratio = Fraction(3, 2)
    y0, y1, x0, x1 = 4, 50, 6, 68  # a 62 x 46 crop at even offsets: the window starts on whole output pixels
    Y0, Y1, X0, X1 = 6, 75, 9, 102
    for dtype in (torch.float16, torch.float32):
        frame = torch.rand((2, 3, 60, 70), device="cuda").to(dtype)
        want = torch_io.upscale(s, frame[..., y0:y1, x0:x1].contiguous())
        assert tuple(want.shape) == (2, 3, 69, 93)
        canvas = filled((2, 3, 90, 105), F16 if dtype == torch.float16 else F32)
        r = torch_io.upscale(s, frame[..., y0:y1, x0:x1], out=canvas[..., Y0:Y1, X0:X1])
        torch.cuda.synchronize()
        assert r.data_ptr() == canvas[..., Y0:Y1, X0:X1].data_ptr()
        assert torch.equal(r, want) and not torch.isnan(want).any()
        mask = torch.ones_like(canvas, dtype=torch.bool)
        mask[..., Y0:Y1, X0:X1] = False
        assert untouched(canvas[mask])
        for bad in (canvas[..., 0:4 * (y1 - y0), 0:4 * (x1 - x0)], canvas[..., 0:2 * (y1 - y0), 0:2 * (x1 - x0)]):  # a x4 and a x2 window
            with pytest.raises(ValueError):
                torch_io.upscale(s, frame[..., y0:y1, x0:x1], out=bad)
    frame8 = torch.randint(0, 256, (60, 70, 3), dtype=torch.uint8, device="cuda")
    want8 = torch_io.upscale(s, frame8[y0:y1, x0:x1].contiguous())
    canvas8 = filled((90, 105, 3), U8)
    torch_io.upscale(s, frame8[y0:y1, x0:x1], out=canvas8[Y0:Y1, X0:X1])
    torch.cuda.synchronize()
    assert torch.equal(canvas8[Y0:Y1, X0:X1], want8)
    mask = torch.ones_like(canvas8, dtype=torch.bool)
    mask[Y0:Y1, X0:X1] = False
    assert untouched(canvas8[mask])
    surf = torch.zeros((46 * 3 // 2, 62), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="YUV"):
        torch_io.upscale_yuv(s, surf)


# ---- 6. host entry points, merging ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_host_entry_points_agree_with_the_device_call(ctxs, tta):
    w, h, T = 62, 46, 32  # 2 x 2 tiles
    s = ctxs[tta]
    s.tilesize = T
    for c, ratio in ((3, (3, 2)), (4, (3, 2)), (3, (5, 2)), (3, (3, 1))):
        img = image(7900 + c, w, h, c)
        want = run(s, img, U8, U8, ratio)
        ty, tx = T * ratio[0] // ratio[1], T * ratio[0] // ratio[1]  # a tile's rows / columns in the output
        assert np.array_equal(s.process(img), want)                               # pageable in and out
        pin_in, pin_out = R.PinnedArray(img.shape), R.PinnedArray(want.shape)
        pin_in.array[:] = img
        pin_out.array[:] = 0xCD
        assert np.array_equal(s.process(pin_in.array, out=pin_out.array), want)   # pinned in and out
        pin_in.free()
        pin_out.free()
        assert np.array_equal(s.process_many([img, img])[1], want)
        halves = np.full_like(want, 0xCD)
        s.process_rows(img, halves, 0, 1)
        assert (halves[ty:] == 0xCD).all() and np.array_equal(halves[:ty], want[:ty])
        s.process_rows(img, halves, 1, 2)
        assert np.array_equal(halves, want)
        tiles = np.full_like(want, 0xCD)
        s.process_tiles(img, tiles, 1, 3)  # the tail of tile row 0 and the head of row 1: rectangles
        assert (tiles[:ty, :tx] == 0xCD).all() and (tiles[ty:, tx:] == 0xCD).all()
        s.process_tiles(img, tiles, 0, 1)
        s.process_tiles(img, tiles, 3, 4)
        assert np.array_equal(tiles, want)
        assert np.array_equal(R.process_group([s], img), want)
        with pytest.raises(ValueError):
            s.process_rows(img, np.zeros((4 * h, 4 * w, c), np.uint8), 0, 1)  # a x4 buffer at another ratio


def test_sixteen_threads_still_merge_at_a_ratio(ctxs):
    s = ctxs[False]
    s.tilesize = 32
    sizes = [(62, 46), (54, 46), (40, 30), (34, 22)]
    imgs = [image(8000 + i, *sizes[i % 4]) for i in range(16)]
    s.out_ratio = Fraction(3, 2)
    s.set_option("merge", 1)
    lone = [s.process(im) for im in imgs]
    s.set_option("merge", 16)
    assert lone[0].shape == (69, 93, 3)
    m0 = s.get_stat("merged_batches")
    got, errs = [None] * 16, []

    def work(i):
        try:
            got[i] = s.process(imgs[i], push_params=False)
        except Exception as e:  # noqa: BLE001
            errs.append((i, repr(e)))
    th = [threading.Thread(target=work, args=(i,)) for i in range(16)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    nb = s.get_stat("merged_batches") - m0
    print("16 images of 4 sizes at ratio 3/2 in %d merged batches" % nb)
    assert 0 < nb < 16
    for i in range(16):
        assert np.array_equal(got[i], lone[i]), i


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_output_untouched(ctxs):
    s = ctxs[False]
    L = s._L
    s.tilesize = 32
    s.out_ratio = Fraction(3, 2)
    s._push_params()
    g0 = s.get_stat("batch_groups")

    def refused(w, h, out_fmt=F32, pitch=0, in_fmt=F32, out_shape=None):
        d_in = torch.zeros((3, h, w), dtype=torch.float32, device="cuda")
        d_out = filled(out_shape or (3, h * 3 // 2 + 2, w * 3 // 2 + 2), F32 if out_fmt == F32 else U8)
        torch.cuda.synchronize()
        rc = L.rsr_process_device_batch(s._h, 1, R._images([d_in.data_ptr()]), in_fmt, w, h, 3, R._images([(d_out.data_ptr(), pitch, 0)]), out_fmt, None)
        rc2 = L.rsr_process_device_fmt(s._h, C.c_void_p(d_in.data_ptr()), in_fmt, w, h, 3, C.c_void_p(d_out.data_ptr()), out_fmt, None) if not pitch else rc
        torch.cuda.synchronize()
        assert rc == R.RSR_E_ARG and rc2 == R.RSR_E_ARG, (rc, rc2)
        assert L.rsr_last_error(s._h)
        assert untouched(d_out) and s.get_stat("batch_groups") == g0
    refused(61, 46)                                  # an odd w at 3/2
    refused(62, 47)                                  # an odd h
    s.tilesize = 33
    s._push_params()
    refused(62, 46)                                  # tile 33 at 3/2
    s.tilesize = 32
    s._push_params()
    refused(62, 46, pitch=4 * (93 - 1), out_shape=(3, 69, 93))   # a pitch one element short of the reduced row
    refused(62, 46, out_fmt=NV12, out_shape=(200, 200))          # an NV12 output at 3/2
    assert "YUV" in L.rsr_last_error(s._h).decode()
    # the host entry point: rsr_process with an odd w
    img, out = image(8100, 61, 46), np.full((69, 93, 3), 0xCD, dtype=np.uint8)
    assert L.rsr_process(s._h, R._p(img), 61, 46, 3, R._p(out)) == R.RSR_E_ARG and (out == 0xCD).all()
    hs = (C.c_void_p * 1)(s._h)
    assert L.rsr_process_group(hs, 1, R._p(img), 61, 46, 3, R._p(out)) == R.RSR_E_ARG and (out == 0xCD).all()
    with pytest.raises(ValueError):
        s.process(img)
    # and the context is as usable as before
    assert run(s, image(8101, 62, 46), U8, U8, (3, 2)).shape == (69, 93, 3)


# ---- 8. the integer ratios are option "out_scale" ------------------------------------------------------------------------------------
def test_integer_ratios_are_out_scale(ctxs, paths):
    s = ctxs[False]
    s.tilesize = 32
    img = image(8200, 61, 47)
    fresh = R.RealSR(0)
    fresh.load(*paths)
    fresh.tilesize = 32
    assert fresh.out_ratio == 4 and fresh.get_stat("out_num") == 4 and fresh.get_stat("out_den") == 1 and fresh.get_stat("out_scale") == 4
    want4 = fresh.process(img)
    fresh.close()
    for k in (2, 1):
        s.out_scale = k
        want = s.process(img)
        wantf = run(s, img, U8, F32, k)
        s.out_scale = 4
        assert s._L.rsr_set_out_ratio(s._h, 2 * k, 2) == R.RSR_OK  # (k / 1, unreduced)
        assert s.get_stat("out_scale") == k and s.get_stat("out_num") == k and s.get_stat("out_den") == 1 and s.out_ratio == k
        assert np.array_equal(s.process(img), want)
        assert np.array_equal(bits(run(s, img, U8, F32, (k, 1))), bits(wantf))
    s.out_ratio = Fraction(3, 2)
    assert s.get_stat("out_scale") == 0 and (s.get_stat("out_num"), s.get_stat("out_den")) == (3, 2)
    for n, d in ((0, 1), (5, 1), (3, 4), (9, 5), (3, 0), (17, 4)):
        assert s._L.rsr_set_out_ratio(s._h, n, d) == R.RSR_E_ARG
        assert (s.get_stat("out_num"), s.get_stat("out_den")) == (3, 2)  # the value in force stays
    assert s.process(image(8201, 62, 46)).shape == (69, 93, 3)
    s.out_scale = 4  # a fractional ratio -> out_scale 4: the bytes of a context that never left 4
    assert s.out_ratio == 4 and np.array_equal(s.process(img), want4)
    assert s._L.rsr_set_option(s._h, b"out_scale", 3) == R.RSR_E_ARG and s.get_stat("out_scale") == 4
    assert s._L.rsr_set_out_ratio(s._h, 3, 1) == R.RSR_OK and s.out_ratio == 3 and s.get_stat("out_scale") == 0
    assert s.process(img).shape == (141, 183, 3)


# ---- 9. the CLI ------------------------------------------------------------------------------------------------------------------------
def test_cli_out_ratio(ctxs, tmp_path, model_dir):
    from cli_support import CLI, read_png, write_png
    s = ctxs[False]
    s.tilesize = 32
    img = image(8300, 40, 30)
    write_png(tmp_path / "a.png", img)
    r = subprocess.run([CLI, "-i", str(tmp_path / "a.png"), "-o", str(tmp_path / "o.png"), "-m", model_dir, "-t", "32", "-v"],
                       capture_output=True, text=True, env=dict(os.environ, RSR_OUT_SCALE="3/2"), timeout=300)
    assert r.returncode == 0, r.stderr
    assert "output scale 3/2" in r.stderr
    got = read_png(tmp_path / "o.png")
    assert got.shape == (45, 60, 3)
    s.out_ratio = Fraction(3, 2)
    assert np.array_equal(got, s.process(img))
    write_png(tmp_path / "odd.png", image(8301, 41, 30))
    r = subprocess.run([CLI, "-i", str(tmp_path / "odd.png"), "-o", str(tmp_path / "odd_o.png"), "-m", model_dir, "-t", "32"],
                       capture_output=True, text=True, env=dict(os.environ, RSR_OUT_SCALE="3/2"), timeout=300)
    assert r.returncode != 0 and not (tmp_path / "odd_o.png").exists()
