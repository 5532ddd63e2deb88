"""rsr_process_device_batch on the GPU (run with -m gpu): tensor batches as merged tile batches, strided inputs and outputs, and
torch_io.upscale on top of them.

Everything here is EXACT: image i of a batch call must receive the very bytes a lone rsr_process_device_fmt call on the tightly packed
image writes -- the kernels, the plan tables of an image and the arithmetic are the same, only the addressing differs -- so no
tolerance appears anywhere.  Outputs are pre-filled with what no call writes (NaN / 0xCD): an element left out, or a byte written
outside a window, shows.  The parity of a lone call against the oracle is tests/test_gpu_parity.py and tests/test_gpu_tensor_io.py.
"""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

from gpu_support import ROUTE_IDS, ROUTES, TORCH, context_fixtures, filled, paths, run, untouched  # noqa: F401
from pixfmt_ref import F16, F32, NP, U8, same_bits, sentinel, u8_image as image

pytestmark = pytest.mark.gpu
# (w, h, tilesize) of tests/test_gpu_tensor_io.py: partial last tiles both ways | a folded last column (kernels.h kFoldBit) | the same at
# tile 100 | an image smaller than a tile
GEOS = [(61, 47, 32), (53, 47, 32), (121, 110, 100), (40, 30, 100)]
PAIRS = [(U8, U8), (F16, F32), (F32, F16), (U8, F16)]
FOLDED = (53, 47, 32)


ctxs, back_to_defaults = context_fixtures(autouse=True)


def as_fmt(img, fmt):
    """The uint8 image itself, or the planar float image whose network input is exactly the uint8 path's."""
    if fmt == U8:
        return img
    x = img.astype(np.float32) * np.float32(1 / 255.0)
    return np.ascontiguousarray(x.transpose(2, 0, 1)).astype(NP[fmt])


def out_buffer(fmt, w, h, c=3):
    return filled((4 * h, 4 * w, c) if fmt == U8 else (3, 4 * h, 4 * w), fmt)


def geometry(x, fmt):
    return (x.shape[1], x.shape[0], x.shape[2]) if fmt == U8 else (x.shape[2], x.shape[1], 3)


def single(s, x, in_fmt, out_fmt):
    """The reference: one synchronous rsr_process_device_fmt call on the packed numpy image x, as raw bytes."""
    got = run(s, x, in_fmt, out_fmt, nan=True)
    assert not same_bits(got, sentinel(out_fmt, got.shape))
    return got.view(np.uint8)


def batch(s, xs, in_fmt, out_fmt, stream=None):
    """One rsr_process_device_batch call on packed numpy images; returns the device outputs (not synchronised when a stream is given)."""
    w, h, c = geometry(xs[0], in_fmt)
    d_in = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]
    d_out = [out_buffer(out_fmt, w, h, c) for _ in xs]
    torch.cuda.synchronize()
    s.process_device_batch([t.data_ptr() for t in d_in], in_fmt, w, h, c, [t.data_ptr() for t in d_out], out_fmt, stream=stream)
    return d_out


def raw(t):
    return t.cpu().numpy().view(np.uint8)


def stats(s, *keys):
    return [s.get_stat(k) for k in keys]


# ---- 1. a batch equals its singles -----------------------------------------------------------------------------------------------
CASES = [(g, tta, precise, PAIRS[(gi + 2 * tta + precise) % 4])
         for gi, g in enumerate(GEOS) for tta in (0, 1) for precise in (0, 1)]  # every pair meets every geometry, mode and storage once


@pytest.mark.parametrize("geo,tta,precise,pair", CASES,
                         ids=["%dx%d-T%d-%s-%s-fmt%d%d" % (g + ("tta" if t else "plain", "precise" if p else "fp16") + f) for g, t, p, f in CASES])
def test_batch_equals_singles(ctxs, geo, tta, precise, pair):
    w, h, T = geo
    s = ctxs[bool(tta)]
    s.tilesize = T
    s.set_option("precise", precise)
    try:
        xs = [as_fmt(image(7000 + 10 * w + i, w, h), pair[0]) for i in range(3)]
        want = [single(s, x, *pair) for x in xs]
        assert not np.array_equal(want[0], want[1])
        g0, m0 = stats(s, "batch_groups", "merged_batches")
        outs = batch(s, xs, *pair)
        torch.cuda.synchronize()
        assert stats(s, "batch_groups", "merged_batches") == [g0 + 1, m0]  # three images, ONE tile batch (narrower than its plan)
        for i in range(3):
            assert np.array_equal(raw(outs[i]), want[i]), i
    finally:
        s.set_option("precise", 0)


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_rgba_batch_equals_singles(ctxs, tta):
    """uint8 RGBA: the unfused route (postproc_tiles writes the image) and the bicubic alpha reads, per image of the batch."""
    w, h, T = FOLDED
    s = ctxs[tta]
    s.tilesize = T
    xs = [image(7100 + i, w, h, 4) for i in range(3)]
    want = [single(s, x, U8, U8) for x in xs]
    outs = batch(s, xs, U8, U8)
    torch.cuda.synchronize()
    for i in range(3):
        assert np.array_equal(raw(outs[i]), want[i]), i


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_bgr_batch_equals_singles(ctxs, tta):
    w, h, T = FOLDED
    s = ctxs[tta]
    s.tilesize = T
    s.set_option("bgr", 1)
    try:
        for pair in ((U8, U8), (F16, F32)):
            xs = [as_fmt(image(7200 + i, w, h), pair[0]) for i in range(3)]
            want = [single(s, x, *pair) for x in xs]
            outs = batch(s, xs, *pair)
            torch.cuda.synchronize()
            for i in range(3):
                assert np.array_equal(raw(outs[i]), want[i]), (pair, i)
    finally:
        s.set_option("bgr", 0)


# ---- 2. group arithmetic ---------------------------------------------------------------------------------------------------------
def test_groups_of_merge_width(ctxs):
    """17 images of 40 x 30 at tile 100 (one tile of 8 work items each: 16 share a batch) are two tile batches, 16 + 1; with "merge" = 1
    seventeen.  Same bytes either way, and the cross-call combiner's counters do not move."""
    s = ctxs[False]
    s.tilesize = 100
    xs = [as_fmt(image(7300 + i, 40, 30), F16) for i in range(17)]
    g0, c0, i0, m0 = stats(s, "batch_groups", "batch_calls", "batch_images", "merged_batches")
    merged = [raw(t) for t in batch(s, xs, F16, F16)]
    assert stats(s, "batch_groups", "batch_calls", "batch_images", "merged_batches") == [g0 + 2, c0 + 1, i0 + 17, m0]
    s.set_option("merge", 1)
    try:
        serial = [raw(t) for t in batch(s, xs, F16, F16)]
        assert stats(s, "batch_groups", "batch_calls", "batch_images", "merged_batches") == [g0 + 19, c0 + 2, i0 + 34, m0]
        lone = [single(s, xs[i], F16, F16) for i in (0, 15, 16)]
    finally:
        s.set_option("merge", 16)
    for i in range(17):
        assert np.array_equal(merged[i], serial[i]), i
    for k, i in enumerate((0, 15, 16)):  # the first and last image of the full group, and the lone one of the second
        assert np.array_equal(merged[i], lone[k]), i
    # n = 1 with a packed descriptor is the rsr_process_device_fmt call
    one = batch(s, xs[:1], F16, F16)
    assert stats(s, "batch_groups", "batch_calls", "batch_images") == [g0 + 20, c0 + 3, i0 + 35]
    assert np.array_equal(raw(one[0]), lone[0])


def lr_items(w, h, T, P=10):
    """Engine::image_items: the 16 x 32 blocks of all padded tiles of a w x h image."""
    n = 0
    for y0 in range(0, h, T):
        for x0 in range(0, w, T):
            th, tw = min(y0 + T, h) - y0 + 2 * P, min(x0 + T, w) - x0 + 2 * P
            n += ((th + 15) // 16) * ((tw + 31) // 32)
    return n


def test_large_images_are_not_merged(ctxs):
    """An image is merged while its work items are at most a quarter of "merge_target_items" (4096).  At tile 32 a full tile is 52 x 52
    padded = 4 x 2 blocks: 11 x 11 tiles are 968 items (four such images fit one batch), 12 x 11 tiles 1056 -- the smallest grid of
    whole tiles that is not merged.  Two images of each: one tile batch, and two."""
    s = ctxs[False]
    s.tilesize = 32
    assert lr_items(352, 352, 32) * 4 <= 4096 < lr_items(384, 352, 32) * 4
    for (w, h), groups in (((352, 352), 1), ((384, 352), 2)):
        xs = [image(7400 + w + i, w, h) for i in range(2)]
        g0 = s.get_stat("batch_groups")
        outs = batch(s, xs, U8, U8)
        torch.cuda.synchronize()
        assert s.get_stat("batch_groups") == g0 + groups, (w, h)
        for i in range(2):
            assert np.array_equal(raw(outs[i]), single(s, xs[i], U8, U8)), (w, h, i)


def test_progress_counts_the_tiles_of_all_images(ctxs):
    s = ctxs[False]
    s.tilesize = 32
    w, h = 61, 47  # 2 x 2 tiles
    seen = []
    CB = C.CFUNCTYPE(None, C.c_int, C.c_int, C.c_void_p)
    cb = CB(lambda done, total, user: seen.append((done, total)))
    assert s._L.rsr_set_progress_callback(s._h, C.cast(cb, C.c_void_p), None) == 0
    try:
        batch(s, [image(7500 + i, w, h) for i in range(5)], U8, U8)
        torch.cuda.synchronize()
    finally:
        assert s._L.rsr_set_progress_callback(s._h, None, None) == 0
    assert seen == [(i, 20) for i in range(1, 21)]


# ---- 3. strided inputs and outputs -----------------------------------------------------------------------------------------------
def crop_and_window(x, fmt, w, h, c=3):
    """x (packed numpy image) placed at odd offsets inside a larger device tensor, and a canvas with a window at odd offsets for its
    result: returns (surface, crop view, canvas, window view).  Row pitch > width, plane pitch > h * row pitch, bases element-aligned."""
    if fmt == U8:
        surface = torch.randint(0, 256, (h + 9, w + 11, c), dtype=torch.uint8, device="cuda")
        crop = surface[5:5 + h, 3:3 + w]
        canvas = filled((4 * h + 7, 4 * w + 9, c), fmt)
        window = canvas[3:3 + 4 * h, 5:5 + 4 * w]
    else:
        surface = torch.rand((3, h + 9, w + 11), device="cuda").to(TORCH[fmt])
        crop = surface[:, 5:5 + h, 3:3 + w]
        canvas = filled((3, 4 * h + 7, 4 * w + 9), fmt)
        window = canvas[:, 3:3 + 4 * h, 5:5 + 4 * w]
    crop.copy_(torch.from_numpy(x).cuda())
    assert not crop.is_contiguous() and not window.is_contiguous()
    return surface, crop, canvas, window


def check_window(canvas, window, want, fmt):
    """The window holds `want` (raw bytes of the packed result) and the canvas around it still holds the fill value."""
    assert np.array_equal(raw(window.contiguous()).reshape(-1), want.reshape(-1))
    mask = torch.ones_like(canvas, dtype=torch.bool)
    if fmt == U8:
        mask[3:3 + window.shape[0], 5:5 + window.shape[1]] = False
    else:
        mask[:, 3:3 + window.shape[1], 5:5 + window.shape[2]] = False
    assert untouched(canvas[mask])


# plain context: the fused store, the per-pixel post kernel, the LDS-staged pre / post kernels (which must cope with, or decline, the
# pitches); TTA context: the default (staged post kernel) and the staged pre kernel too


@pytest.mark.parametrize("fmt", [U8, F16, F32], ids=["u8", "f16", "f32"])
@pytest.mark.parametrize("tta,dbg", ROUTES, ids=ROUTE_IDS)
def test_strided_crop_in_window_out(ctxs, tta, dbg, fmt):
    w, h, T = FOLDED
    s = ctxs[tta]
    s.tilesize = T
    x = as_fmt(image(7600, w, h), fmt)
    want = single(s, x, fmt, fmt)
    surface, crop, canvas, window = crop_and_window(x, fmt, w, h)
    ins, outs = [torch_io.describe(crop)], [torch_io.describe(window)]
    assert ins[0][1] > w * crop.element_size() and outs[0][1] > 4 * w * window.element_size()
    torch.cuda.synchronize()
    s.set_option("dbg", dbg)
    try:
        s.process_device_batch(ins, fmt, w, h, 3, outs, fmt)
        torch.cuda.synchronize()
    finally:
        s.set_option("dbg", 0)
    check_window(canvas, window, want, fmt)


@pytest.mark.parametrize("tta,dbg", ROUTES, ids=ROUTE_IDS)
def test_uint8_row_pitch_of_3w_plus_1(ctxs, tta, dbg):
    """A uint8 row pitch that is no multiple of the pixel size, on both sides, three images in one batch: every pad byte stays."""
    w, h, T = FOLDED
    s = ctxs[tta]
    s.tilesize = T
    xs = [image(7700 + i, w, h) for i in range(3)]
    want = [single(s, x, U8, U8) for x in xs]
    ip, op = 3 * w + 1, 12 * w + 1
    assert R.image_span(U8, w, h, 3, ip) == h * ip - 1
    d_in, d_out = [], []
    for x in xs:
        t = torch.randint(0, 256, (h, ip), dtype=torch.uint8, device="cuda")
        t[:, :3 * w] = torch.from_numpy(x.reshape(h, 3 * w)).cuda()
        d_in.append(t)
        d_out.append(filled((4 * h, op), U8))
    torch.cuda.synchronize()
    s.set_option("dbg", dbg)
    try:
        s.process_device_batch([(t.data_ptr(), ip, 0) for t in d_in], U8, w, h, 3, [(t.data_ptr(), op, 0) for t in d_out], U8)
        torch.cuda.synchronize()
    finally:
        s.set_option("dbg", 0)
    for i in range(3):
        got = d_out[i].cpu().numpy()
        assert np.array_equal(got[:, :12 * w].reshape(-1), want[i].reshape(-1)), i
        assert (got[:, 12 * w] == 0xCD).all(), i


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_rgba_crop_in_window_out(ctxs, tta):
    w, h, T = FOLDED
    s = ctxs[tta]
    s.tilesize = T
    x = image(7800, w, h, 4)
    want = single(s, x, U8, U8)
    surface, crop, canvas, window = crop_and_window(x, U8, w, h, 4)
    torch.cuda.synchronize()
    s.process_device_batch([torch_io.describe(crop)], U8, w, h, 4, [torch_io.describe(window)], U8)
    torch.cuda.synchronize()
    check_window(canvas, window, want, U8)


# ---- 4. streams ------------------------------------------------------------------------------------------------------------------
def test_batch_on_a_torch_stream(ctxs):
    """A batch call on a non-default stream, its inputs made by a torch op on that stream just before, no host synchronisation in
    between.  Engine idle: the kernels go onto the caller's stream (stat device_direct).  Engine busy behind a device-side sleep on
    another stream: the ordered path through the compute stream.  Correct either way once the stream is synchronised."""
    s = ctxs[False]
    s.tilesize = 32
    w, h = 61, 47
    xs = [as_fmt(image(7900 + i, w, h), F16) for i in range(3)]
    want = [single(s, x, F16, F32) for x in xs]
    base = torch.from_numpy(np.stack(xs)).cuda()
    st, other = torch.cuda.Stream(), torch.cuda.Stream()

    def call(x, y, stream):
        s.process_device_batch([t.data_ptr() for t in x], F16, w, h, 3, [t.data_ptr() for t in y], F32, stream=stream.cuda_stream)

    torch.cuda.synchronize()
    n0, g0 = stats(s, "device_direct", "batch_groups")
    with torch.cuda.stream(st):
        x = (base * 2) * 0.5  # exact; produced on `st`
        y = filled((3, 3, 4 * h, 4 * w), F32)
        call(x, y, st)
        y_copy = y.clone()
    st.synchronize()
    assert stats(s, "device_direct", "batch_groups") == [n0 + 1, g0 + 1]
    for i in range(3):
        assert np.array_equal(raw(y_copy[i]), want[i]), i
    torch.cuda.synchronize()
    with torch.cuda.stream(other):
        torch.cuda._sleep(50_000_000)
        y_slow = filled((3, 3, 4 * h, 4 * w), F32)
        call(base, y_slow, other)  # (on its caller's stream or through the compute stream: the compute stream has work pending while the sleep lasts)
    n1 = s.get_stat("device_direct")
    with torch.cuda.stream(st):
        x2 = (base * 2) * 0.5
        y2 = filled((3, 3, 4 * h, 4 * w), F32)
        call(x2, y2, st)  # the ordered path through the compute stream
        y2_copy = y2.clone()
    assert s.get_stat("device_direct") == n1
    st.synchronize()
    other.synchronize()
    for i in range(3):
        assert np.array_equal(raw(y2_copy[i]), want[i]), i
        assert np.array_equal(raw(y_slow[i]), want[i]), i
    torch.cuda.synchronize()


# ---- 5. torch_io -----------------------------------------------------------------------------------------------------------------
def test_upscale_batch_views_and_out(ctxs):
    s = ctxs[False]
    s.tilesize = 32
    w, h, N = 53, 47, 3
    xs = [as_fmt(image(8000 + i, w, h), F32) for i in range(N)]
    want = [single(s, x, F32, F32) for x in xs]
    st = torch.cuda.Stream()
    # an (N, 3, H, W) tensor is ONE batch call
    x = torch.from_numpy(np.stack(xs)).cuda()
    c0, i0, g0 = stats(s, "batch_calls", "batch_images", "batch_groups")
    with torch.cuda.stream(st):
        y = torch_io.upscale(s, x)
    st.synchronize()
    assert stats(s, "batch_calls", "batch_images", "batch_groups") == [c0 + 1, i0 + N, g0 + 1]
    assert tuple(y.shape) == (N, 3, 4 * h, 4 * w) and y.dtype == torch.float32 and y.is_contiguous()
    for i in range(N):
        assert np.array_equal(raw(y[i]), want[i]), i
    # a crop view (of every second image of a larger batch) gives the bytes of its contiguous copy, on the default stream too
    big = torch.rand((2 * N, 3, h + 9, w + 11), device="cuda")
    view = big[::2, :, 5:5 + h, 3:3 + w]
    view.copy_(x)
    assert not view.is_contiguous() and torch_io.describe(view[1]) is not None
    y_view = torch_io.upscale(s, view)
    y_copy = torch_io.upscale(s, view.contiguous())
    torch.cuda.synchronize()
    assert torch.equal(y_view, y_copy) and torch.equal(y_view, y)
    # a single cropped image
    y_one = torch_io.upscale(s, view[1])
    torch.cuda.synchronize()
    assert np.array_equal(raw(y_one), want[1])
    # out=: a window of a canvas, written in place and returned; the canvas around it is untouched
    canvas = filled((N, 3, 4 * h + 7, 4 * w + 9), F32)
    window = canvas[:, :, 3:3 + 4 * h, 5:5 + 4 * w]
    with torch.cuda.stream(st):
        r = torch_io.upscale(s, view, out=window)
    st.synchronize()
    assert r is window
    for i in range(N):
        check_window(canvas[i], window[i], want[i], F32)
    # uint8 HWC: a crop into a window
    x8 = image(8100, w, h)
    want8 = single(s, x8, U8, U8)
    surface, crop, canvas8, window8 = crop_and_window(x8, U8, w, h)
    assert torch_io.upscale(s, crop, out=window8) is window8
    torch.cuda.synchronize()
    check_window(canvas8, window8, want8, U8)
    # a bad `out` is refused before anything is launched
    calls = stats(s, "batch_calls", "device_direct")
    hwc = torch.empty((N, 4 * h, 4 * w, 3), device="cuda").permute(0, 3, 1, 2)  # the right shape in a layout no descriptor fits
    for bad in (window[:, :, :, ::2], canvas, window.double(), window[0], hwc):
        with pytest.raises(ValueError):
            torch_io.upscale(s, view, out=bad)
    assert stats(s, "batch_calls", "device_direct") == calls


# ---- 6. next to calls of every other kind ----------------------------------------------------------------------------------------
def test_batch_calls_next_to_merging_and_format_calls(ctxs):
    """Four threads on one context: two issue batch calls (one strided, f16 -> f32; one uint8), one small synchronous process_device
    calls (these enter the cross-call combiner), one process_device_fmt calls.  Every output equals its lone result."""
    s = ctxs[False]
    s.tilesize = 64
    w, h = 90, 70
    imgs = [image(8200 + i, w, h) for i in range(14)]
    kind = [(F16, F32)] * 4 + [(U8, U8)] * 4 + [(U8, U8)] * 3 + [(F16, F32)] * 3  # batch a | batch b | process_device | process_device_fmt
    src = [as_fmt(im, k[0]) for im, k in zip(imgs, kind)]
    s.set_option("merge", 1)
    lone = [single(s, x, *k) for x, k in zip(src, kind)]
    s.set_option("merge", 16)
    d_out = [out_buffer(k[1], w, h) for k in kind]
    d_in = [torch.from_numpy(x).cuda() for x in src]
    surface = torch.rand((4, 3, h + 3, w + 5), device="cuda").half()  # batch a reads crops of a larger tensor
    crops = surface[:, :, 1:1 + h, 3:3 + w]
    crops.copy_(torch.stack(d_in[:4]))
    torch.cuda.synchronize()
    errs = []

    def work(t):
        try:
            for _ in range(2):
                if t == 0:
                    s.process_device_batch([torch_io.describe(crops[i]) for i in range(4)], F16, w, h, 3, [d_out[i].data_ptr() for i in range(4)], F32)
                elif t == 1:
                    s.process_device_batch([d_in[i].data_ptr() for i in range(4, 8)], U8, w, h, 3, [d_out[i].data_ptr() for i in range(4, 8)], U8)
                elif t == 2:
                    for i in range(8, 11):
                        s.process_device(d_in[i].data_ptr(), w, h, 3, d_out[i].data_ptr())
                else:
                    for i in range(11, 14):
                        s.process_device_fmt(d_in[i].data_ptr(), F16, w, h, 3, d_out[i].data_ptr(), F32)
        except Exception as e:  # noqa: BLE001
            errs.append((t, repr(e)))
    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    torch.cuda.synchronize()
    for i in range(14):
        assert np.array_equal(raw(d_out[i]), lone[i]), i


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing_and_leave_the_context_usable(ctxs, paths):
    s = ctxs[False]
    s.tilesize = 32
    L = s._L
    w, h = 40, 30
    x = as_fmt(image(8300, w, h), F32)
    want = single(s, x, F32, F32)
    d_in = torch.from_numpy(x).cuda()
    d_out = out_buffer(F32, w, h)
    pin, pout = d_in.data_ptr(), d_out.data_ptr()

    def call(n, ins, in_fmt, c, outs, out_fmt, h_=None):
        return L.rsr_process_device_batch(h_ or s._h, n, R._images(ins) if ins is not None else None, in_fmt, w, h, c,
                                          R._images(outs) if outs is not None else None, out_fmt, None)

    ok_in, ok_out = [(pin, 0, 0)], [(pout, 0, 0)]
    bad = [
        (0, ok_in, F32, 3, ok_out, F32), (-1, ok_in, F32, 3, ok_out, F32),              # n < 1
        (1, None, F32, 3, ok_out, F32), (1, ok_in, F32, 3, None, F32),                  # null arrays
        (1, [(0, 0, 0)], F32, 3, ok_out, F32), (1, ok_in, F32, 3, [(0, 0, 0)], F32),    # null data
        (2, ok_in * 2, F32, 3, ok_out + [(0, 0, 0)], F32),                              # ... of a later image
        (1, ok_in, 7, 3, ok_out, F32), (1, ok_in, F32, 3, ok_out, -1),                  # unknown format
        (1, ok_in, F32, 4, ok_out, F32), (1, ok_in, U8, 4, ok_out, F16),                # planar with c != 3
        (1, ok_in, U8, 5, ok_out, U8),
        (1, [(pin, 4 * w - 4, 0)], F32, 3, ok_out, F32),                                # row pitch below a row
        (1, ok_in, F32, 3, [(pout, 16 * w - 4, 0)], F32),
        (1, [(pin, 4 * w + 2, 0)], F32, 3, ok_out, F32),                                # pitches / data that are no element multiples
        (1, ok_in, F32, 3, [(pout, 16 * w, 16 * w * 4 * h + 2)], F32),
        (1, [(pin + 2, 0, 0)], F32, 3, ok_out, F32), (1, ok_in, F32, 3, [(pout + 1, 0, 0)], F32),
        (1, [(pin, -4 * w, 0)], F32, 3, ok_out, F32), (1, ok_in, F32, 3, [(pout, 0, -1)], F32),  # negative
        (2, ok_in * 2, F32, 3, ok_out + [(pout, 16 * w - 4, 0)], F32),                  # the LAST image is bad: the first is not run either
    ]
    for a in bad:
        assert call(*a) == R.RSR_E_ARG, a
    torch.cuda.synchronize()
    assert untouched(d_out)
    g = s.get_stat("batch_groups")
    fresh = R.RealSR(0)
    try:
        assert call(1, ok_in, F32, 3, ok_out, F32, h_=fresh._h) == R.RSR_E_STATE  # before load
    finally:
        fresh.close()
    assert untouched(d_out)
    # a good call afterwards works
    assert call(1, ok_in, F32, 3, ok_out, F32) == R.RSR_OK
    torch.cuda.synchronize()
    assert s.get_stat("batch_groups") == g + 1 and np.array_equal(raw(d_out), want)
