"""Option "out_scale" on the GPU (run with -m gpu): the x2 / x1 output, box-reduced on the device (include/realsr_hip.h).

The contract is exact: the F32 output at out_scale s is box_reduce (tests/box_reduce.py: float32, the stated order of summation) of the
F32 output the same context gives at out_scale 4, bit for bit; F16 is that rounded once; uint8 is floor(d * 255 + 0.5), compared
against the exact evaluation except where it lies within 2^-14 of an integer (an fma contraction may move those: the rule and the
1e-3 cap of tests/test_gpu_tensor_io.py); alpha is within 1 of the real-valued mean of the x4 alpha bytes (<= 0.5 from the rounding
of the inputs, <= 0.5 from the output's).  Every entry point gives the same bytes.  Outputs are pre-filled with NaN / 0xCD."""
import os
import subprocess
import threading

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

import gpu_support as G
from box_reduce import box_reduce, u8_expected
from gpu_support import context_fixtures, filled, paths, untouched  # noqa: F401
from pixfmt_ref import F16, F32, U8, bits, halfs, u8_image as image

pytestmark = pytest.mark.gpu
# (w, h, tilesize) of tests/test_gpu_tensor_batch.py: partial last tiles | a folded last column | the same at tile 100 | smaller than a tile
GEOS = [(61, 47, 32), (53, 47, 32), (121, 110, 100), (40, 30, 100)]


ctxs, back_to_defaults = context_fixtures(autouse=True)


def run(s, x, in_fmt, out_fmt, scale):
    """One synchronous rsr_process_device_fmt call at out_scale `scale` on the packed numpy image x; the result as a numpy array."""
    s.out_scale = scale
    assert s.get_stat("out_scale") == scale
    return G.run(s, x, in_fmt, out_fmt, nan=True)


def check_u8(got, d):
    """got: uint8 HWC at out_scale s; d: the float32 box means, planar."""
    want, near = u8_expected(d)
    assert near.mean() <= 1e-3, near.mean()
    g = got.transpose(2, 0, 1)
    print("uint8: %d elements, %d left out (within 2^-14 of a rounding boundary), %d differ" % (g.size, near.sum(), ((g != want) & ~near).sum()))
    assert np.array_equal(g[~near], want[~near])
    assert (np.abs(g.astype(int) - want.astype(int))[near] <= 1).all()


# ---- 1. - 3. the three formats against the x4 output of the same context ------------------------------------------------------------
@pytest.mark.parametrize("precise", [0, 1], ids=["fp16", "precise"])
@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
@pytest.mark.parametrize("geo", GEOS, ids=["%dx%d-T%d" % g for g in GEOS])
def test_formats_are_the_box_means_of_the_x4_output(ctxs, geo, tta, precise):
    w, h, T = geo
    s = ctxs[tta]
    s.tilesize = T
    s.set_option("precise", precise)
    img = image(9000 + w, w, h)
    hx = halfs(9100 + w, w, h)
    ref = run(s, img, U8, F32, 4)
    ref_h = run(s, hx, F16, F32, 4)
    assert ref.min() >= 0 and ref.max() <= 1 and not np.array_equal(ref, ref_h)
    for scale in (2, 1):
        d = box_reduce(ref, 4 // scale)
        got = run(s, img, U8, F32, scale)
        assert got.shape == (3, h * scale, w * scale)
        nd = int((bits(got) != bits(d)).sum())
        print("out_scale %d: F32 %d of %d elements differ in bits" % (scale, nd, d.size))
        assert nd == 0
        got_h = run(s, hx, F16, F32, scale)
        assert np.array_equal(bits(got_h), bits(box_reduce(ref_h, 4 // scale)))
        got16 = run(s, img, U8, F16, scale)
        assert np.array_equal(bits(got16), bits(d.astype(np.float16)))  # rounded once, to nearest even
        check_u8(run(s, img, U8, U8, scale), d)


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_bgr_swaps_channels_of_the_reduced_image(ctxs, tta):
    w, h, T = 53, 47, 32
    s = ctxs[tta]
    s.tilesize = T
    img = image(9200, w, h)
    planar = np.ascontiguousarray((img.astype(np.float32) * np.float32(1 / 255.0)).transpose(2, 0, 1)).astype(np.float16)
    rgb8, rgbf = run(s, img, U8, U8, 2), run(s, planar, F16, F32, 2)
    s.set_option("bgr", 1)
    bgr8 = run(s, np.ascontiguousarray(img[:, :, ::-1]), U8, U8, 2)
    bgrf = run(s, np.ascontiguousarray(planar[::-1]), F16, F32, 2)
    assert np.array_equal(bgr8[:, :, ::-1], rgb8) and not np.array_equal(bgr8, rgb8)
    assert np.array_equal(bits(np.ascontiguousarray(bgrf[::-1])), bits(rgbf))


# ---- 4. alpha ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tta,precise", [(False, 0), (True, 0), (False, 1)], ids=["plain", "tta", "precise"])
def test_alpha_is_the_box_mean_of_the_x4_alpha(ctxs, tta, precise):
    w, h, T = 53, 47, 32
    s = ctxs[tta]
    s.tilesize = T
    s.set_option("precise", precise)  # (the blob is fp32 then: the kernels' <float, uint8_t, ., true> instances)
    img = image(9300, w, h, 4)
    full = run(s, img, U8, U8, 4)
    for scale in (2, 1):
        k = 4 // scale
        got = run(s, img, U8, U8, scale)
        assert got.shape == (h * scale, w * scale, 4)
        mean = full[:, :, 3].astype(np.float64).reshape(h * scale, k, w * scale, k).mean(axis=(1, 3))
        err = np.abs(got[:, :, 3].astype(np.float64) - mean).max()
        print("out_scale %d: max |alpha - mean of the x4 alpha bytes| = %.4f" % (scale, err))
        assert err <= 1.0
        assert np.array_equal(got[:, :, :3], run(s, np.ascontiguousarray(img[:, :, :3]), U8, U8, scale))  # RGB as without alpha
        for a in (0, 255):
            flat = img.copy()
            flat[:, :, 3] = a
            assert (run(s, flat, U8, U8, scale)[:, :, 3] == a).all(), (scale, a)


# ---- 5. every entry point gives the same bytes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_batch_of_five_equals_lone_calls(ctxs, tta):
    w, h, T = 61, 47, 32
    s = ctxs[tta]
    s.tilesize = T
    for in_fmt, out_fmt in ((U8, U8), (F16, F32)):
        xs = [image(9400 + i, w, h) if in_fmt == U8 else halfs(9400 + i, w, h) for i in range(5)]
        want = [run(s, x, in_fmt, out_fmt, 2) for x in xs]
        d_in = [torch.from_numpy(x).cuda() for x in xs]
        d_out = [filled(want[0].shape, out_fmt) for _ in xs]
        torch.cuda.synchronize()
        g0 = s.get_stat("batch_groups")
        s.process_device_batch([t.data_ptr() for t in d_in], in_fmt, w, h, 3, [t.data_ptr() for t in d_out], out_fmt)
        torch.cuda.synchronize()
        assert s.get_stat("batch_groups") == g0 + 1  # ONE merged group
        for i in range(5):
            assert np.array_equal(d_out[i].cpu().numpy().view(np.uint8), want[i].view(np.uint8)), (in_fmt, i)


def test_sixteen_threads_of_mixed_sizes_merge(ctxs):
    s = ctxs[False]
    s.tilesize = 32
    sizes = [(61, 47), (53, 47), (40, 30), (33, 21)]
    imgs = [image(9500 + i, *sizes[i % 4]) for i in range(16)]
    s.out_scale = 2
    s.set_option("merge", 1)
    lone = [s.process(im) for im in imgs]
    s.set_option("merge", 16)
    assert lone[0].shape == (94, 122, 3)
    m0, x0 = s.get_stat("merged_batches"), s.get_stat("merged_mixed")
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
    nb, nm = s.get_stat("merged_batches") - m0, s.get_stat("merged_mixed") - x0
    print("16 images of 4 sizes at out_scale 2 in %d batches, %d of them mixed" % (nb, nm))
    assert nb < 16 and nm >= 1  # (the bounds of tests/test_gpu_merge.py)
    for i in range(16):
        assert np.array_equal(got[i], lone[i]), i
    # one caller thread, many images: the same
    many = s.process_many(imgs)
    for i in range(16):
        assert np.array_equal(many[i], lone[i]), i


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_host_entry_points_agree_with_the_device_call(ctxs, tta):
    w, h, T = 61, 47, 32  # 2 x 2 tiles
    s = ctxs[tta]
    s.tilesize = T
    for c in (3, 4):
        img = image(9600 + c, w, h, c)
        for scale in (2, 1):
            want = run(s, img, U8, U8, scale)
            assert np.array_equal(s.process(img), want)                               # pageable in and out
            pin_in, pin_out = R.PinnedArray(img.shape), R.PinnedArray(want.shape)
            pin_in.array[:] = img
            pin_out.array[:] = 0xCD
            assert np.array_equal(s.process(pin_in.array, out=pin_out.array), want)   # pinned in and out
            pin_in.free()
            pin_out.free()
            halves = np.full_like(want, 0xCD)
            s.process_rows(img, halves, 0, 1)
            assert (halves[T * scale:] == 0xCD).all() and np.array_equal(halves[:T * scale], want[:T * scale])
            s.process_rows(img, halves, 1, 2)
            assert np.array_equal(halves, want)
            tiles = np.full_like(want, 0xCD)
            s.process_tiles(img, tiles, 1, 3)  # the tail of tile row 0 and the head of row 1: rectangles
            assert (tiles[:T * scale, :T * scale] == 0xCD).all() and (tiles[T * scale:, T * scale:] == 0xCD).all()
            s.process_tiles(img, tiles, 0, 1)
            s.process_tiles(img, tiles, 3, 4)
            assert np.array_equal(tiles, want)
            assert np.array_equal(R.process_group([s], img), want)
            with pytest.raises(ValueError):
                s.process_rows(img, np.zeros((4 * h, 4 * w, c), np.uint8), 0, 1)  # a x4 buffer at out_scale < 4


# ---- 6. windows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_upscale_a_crop_into_a_2x_window(ctxs, tta):
    s = ctxs[tta]
    s.tilesize = 32
    s.out_scale = 2
    y0, y1, x0, x1 = 5, 52, 3, 56  # a 53 x 47 crop
    for dtype in (torch.float16, torch.float32):
        frame = torch.rand((2, 3, 60, 70), device="cuda").to(dtype)
        want = torch_io.upscale(s, frame[..., y0:y1, x0:x1].contiguous())
        assert tuple(want.shape) == (2, 3, 94, 106)
        canvas = filled((2, 3, 130, 150), F16 if dtype == torch.float16 else F32)
        r = torch_io.upscale(s, frame[..., y0:y1, x0:x1], out=canvas[..., 2 * y0:2 * y1, 2 * x0:2 * x1])
        torch.cuda.synchronize()
        assert r.data_ptr() == canvas[..., 2 * y0:2 * y1, 2 * x0:2 * x1].data_ptr()
        assert torch.equal(r, want) and not torch.isnan(want).any()
        mask = torch.ones_like(canvas, dtype=torch.bool)
        mask[..., 2 * y0:2 * y1, 2 * x0:2 * x1] = False
        assert untouched(canvas[mask])
        with pytest.raises(ValueError):
            torch_io.upscale(s, frame[..., y0:y1, x0:x1], out=canvas[..., 0:4 * (y1 - y0), 0:4 * (x1 - x0)])  # a x4 window
    # uint8 HWC
    frame8 = torch.randint(0, 256, (60, 70, 3), dtype=torch.uint8, device="cuda")
    want8 = torch_io.upscale(s, frame8[y0:y1, x0:x1].contiguous())
    canvas8 = filled((130, 150, 3), U8)
    torch_io.upscale(s, frame8[y0:y1, x0:x1], out=canvas8[2 * y0:2 * y1, 2 * x0:2 * x1])
    torch.cuda.synchronize()
    assert torch.equal(canvas8[2 * y0:2 * y1, 2 * x0:2 * x1], want8)
    mask = torch.ones_like(canvas8, dtype=torch.bool)
    mask[2 * y0:2 * y1, 2 * x0:2 * x1] = False
    assert untouched(canvas8[mask])


def test_row_pitch_is_checked_against_the_reduced_width(ctxs):
    s = ctxs[False]
    s.tilesize = 32
    s.out_scale = 2
    w, h = 40, 30
    d_in = torch.from_numpy(halfs(9700, w, h)).cuda().float()
    d_out = filled((3, 2 * h, 2 * w), F32)
    torch.cuda.synchronize()
    L = s._L

    def call(pitch):
        return L.rsr_process_device_batch(s._h, 1, R._images([d_in.data_ptr()]), F32, w, h, 3, R._images([(d_out.data_ptr(), pitch, 0)]), F32, None)
    g0 = s.get_stat("batch_groups")
    assert call(4 * (2 * w - 1)) == R.RSR_E_ARG  # one element short of a row of the 2x image
    torch.cuda.synchronize()
    assert untouched(d_out) and s.get_stat("batch_groups") == g0
    assert call(4 * 2 * w) == R.RSR_OK  # (far below the 4 * 4 * w bytes of a x4 row)
    torch.cuda.synchronize()
    assert not torch.isnan(d_out).any()


# ---- 7. option hygiene ---------------------------------------------------------------------------------------------------------------
def test_bad_values_are_refused_and_4_is_the_old_path(ctxs, paths):
    s = ctxs[False]
    s.tilesize = 32
    img = image(9800, 61, 47)
    fresh = R.RealSR(0)
    fresh.load(*paths)
    fresh.tilesize = 32
    assert fresh.out_scale == 4 and fresh.get_stat("out_scale") == 4
    want4 = fresh.process(img)
    fresh.close()
    s.out_scale = 2
    two = s.process(img)
    assert two.shape == (94, 122, 3)
    for bad in (0, 3, 8, -1):
        assert s._L.rsr_set_option(s._h, b"out_scale", bad) == R.RSR_E_ARG
        assert s.get_stat("out_scale") == 2
        with pytest.raises(R.RealSRError) as e:
            s.out_scale = bad
        assert e.value.code == R.RSR_E_ARG and s.out_scale == 2
    s.out_scale = 4
    assert np.array_equal(s.process(img), want4)  # 2 -> 4: the bytes of a context that never left 4
    s.out_scale = 2
    assert np.array_equal(s.process(img), two)


def test_set_option_sizes_the_outputs_too(ctxs):
    """"out_scale" set through set_option, as every other option is, and through the property are one value: the binding sizes its
    buffers with what the engine reports, in either order."""
    s = ctxs[False]
    s.tilesize = 32
    img = image(9850, 61, 47)
    x = torch.from_numpy(halfs(9851, 61, 47)).cuda()
    s.out_scale = 2
    two = s.process(img)
    s.set_option("out_scale", 4)  # (a x4 image now: a binding still at 2 would hand out a quarter of the bytes it needs)
    assert s.out_scale == 4
    four = s.process(img)
    assert four.shape == (188, 244, 3)
    assert tuple(torch_io.upscale(s, x).shape) == (3, 188, 244)
    assert [o.shape for o in s.process_many([img, img])] == [(188, 244, 3)] * 2
    s.set_option("out_scale", 2)
    assert s.out_scale == 2
    assert np.array_equal(s.process(img), two)
    y = torch_io.upscale(s, x)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (3, 94, 122)
    s.out_scale = 4
    assert np.array_equal(s.process(img), four)


def test_device_direct_still_counts(ctxs):
    s = ctxs[False]
    s.tilesize = 32
    w, h = 61, 47
    x = halfs(9900, w, h)
    want = run(s, x, F16, F16, 2)  # (upscale returns the dtype it was given)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    n0 = s.get_stat("device_direct")
    with torch.cuda.stream(st):
        y = torch_io.upscale(s, torch.from_numpy(x).cuda())
    st.synchronize()
    assert s.get_stat("device_direct") == n0 + 1  # an idle context: the kernels went onto the caller's stream
    assert y.dtype == torch.float16 and tuple(y.shape) == (3, 2 * h, 2 * w)
    assert np.array_equal(bits(y.cpu().numpy()), bits(want))


def test_cli_out_scale(ctxs, tmp_path, model_dir):
    from cli_support import CLI, read_png, write_png
    s = ctxs[False]
    s.tilesize = 32
    img = image(9950, 40, 30)
    write_png(tmp_path / "a.png", img)
    env = dict(os.environ, RSR_OUT_SCALE="2")
    r = subprocess.run([CLI, "-i", str(tmp_path / "a.png"), "-o", str(tmp_path / "o.png"), "-m", model_dir, "-t", "32", "-v"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "output scale 2" in r.stderr
    got = read_png(tmp_path / "o.png")
    assert got.shape == (60, 80, 3)
    s.out_scale = 2
    assert np.array_equal(got, s.process(img))
    r = subprocess.run([CLI, "-i", str(tmp_path / "a.png"), "-o", str(tmp_path / "o3.png"), "-m", model_dir, "-t", "32"],
                       capture_output=True, text=True, env=dict(os.environ, RSR_OUT_SCALE="3"), timeout=300)
    assert r.returncode != 0 and "RSR_OUT_SCALE" in r.stderr and not (tmp_path / "o3.png").exists()
