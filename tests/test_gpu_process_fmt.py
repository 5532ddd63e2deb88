"""rsr_process_fmt on the GPU (run with -m gpu): host images of every format pair through one thin entry point -- equal to rsr_process for
uint8, equal to the device call for everything else, from pinned and pageable memory, from several threads at once."""
import threading

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
import rgb16_ref as Z
from gpu_support import context_fixtures, dev, paths  # noqa: F401
from pixfmt_ref import F16, F32, NV12, U8, image

pytestmark = pytest.mark.gpu
U16 = R.RSR_FMT_U16_HWC
W, H, T, P = 36, 25, 16, 10
ctxs, ctx = context_fixtures(T, P)


def device_call(s, x, in_fmt, out_fmt):
    w, h = Z.dims_of(in_fmt, x)
    c = Z.channels_of(in_fmt, x)
    ow, oh = s.out_size_fmt(out_fmt, w, h)
    oshape = Z.shape_of(out_fmt, ow, oh, c)
    d_in, d_out = dev(x), dev(Z.sentinel_bytes(out_fmt, oshape))
    s.process_device_fmt(d_in.data_ptr(), in_fmt, w, h, c, d_out.data_ptr(), out_fmt)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(Z.np_dtype(out_fmt)).reshape(oshape)


@pytest.mark.parametrize("c", [3, 4], ids=["rgb", "rgba"])
@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_u8_to_u8_is_process(ctx, tta, c):
    s = ctx[tta]
    img = image(200 + c, U8, W, H, c)
    want = s.process(img)
    got = s.process_fmt(img, U8, U8)
    assert got.dtype == np.uint8 and got.shape == (4 * H, 4 * W, c) and np.array_equal(got, want)
    s.out_scale = 2
    assert np.array_equal(s.process_fmt(img, U8, U8), s.process(img))


PAIRS = [(U16, U16, 3), (U16, U16, 4), (F32, U16, 3), (U16, F16, 3), (U8, U16, 4), (NV12, U16, 3), (U16, NV12, 3)]


@pytest.mark.parametrize("in_fmt,out_fmt,c", PAIRS, ids=["u16-u16", "u16-u16-rgba", "f32-u16", "u16-f16", "u8-u16-rgba", "nv12-u16", "u16-nv12"])
def test_equals_the_device_call(ctx, in_fmt, out_fmt, c):
    s = ctx[False]
    h = 26 if NV12 in (in_fmt, out_fmt) else H
    if in_fmt == U16:
        x = Z.image16(210, W, h, c)
    elif in_fmt == F32:
        x = Z.as_f32_chw(Z.image16(211, W, h))
    else:
        x = image(212, in_fmt, W, h, c)
    want = device_call(s, x, in_fmt, out_fmt)
    got = s.process_fmt(x, in_fmt, out_fmt)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def test_pinned_and_pageable_buffers(ctx):
    s = ctx[False]
    img = Z.image16(220, W, H)
    want = s.process_fmt(img, U16, U16)  # pageable in, pageable out
    pin_in, pin_out = R.PinnedArray((H, W, 3 * 2)), R.PinnedArray((4 * H, 4 * W, 3 * 2))
    try:
        a_in, a_out = pin_in.array.view(np.uint16).reshape(H, W, 3), pin_out.array.view(np.uint16).reshape(4 * H, 4 * W, 3)
        a_in[:] = img
        a_out[:] = 0xCDCD
        assert s.process_fmt(a_in, U16, U16, out=a_out) is a_out and np.array_equal(a_out, want)  # pinned in, pinned out
        out = np.full_like(want, 0xCDCD)
        assert np.array_equal(s.process_fmt(a_in, U16, U16, out=out), want)                     # pinned in, pageable out
        a_out[:] = 0xCDCD
        assert np.array_equal(s.process_fmt(img, U16, U16, out=a_out), want)                    # pageable in, pinned out
    finally:
        pin_in.free()
        pin_out.free()


def test_pageable_output_in_several_chunks(ctx):
    """chunk_mb 1: the download into pageable memory goes through the two staging slots in chunks of 1 MiB -- a slot is never larger than
    chunk_mb says at the time of the call, whatever staging an earlier call left on the lane (Engine::lane_fetch), and never smaller
    than 1 MiB.  800 x 480 x 6 B = 2.3 MB of 16-bit RGB is three chunks.  The NV12 surface of the same size is 576,000 B, ONE chunk; the
    1200 x 960 surface of a 300 x 240 image is 1.73 MB, two: the boundary, at 1 MiB, lies inside the Y plane of 1.15 MB."""
    s = ctx[False]
    for w, h, out_fmt, chunks in ((200, 120, U16, 3), (200, 120, NV12, 1), (300, 240, NV12, 2)):
        img = Z.image16(270, w, h)
        nbytes = R.image_bytes(out_fmt, 4 * w, 4 * h, 3)
        assert -(-nbytes // (1 << 20)) == chunks and (out_fmt != NV12 or chunks == 1 or 1 << 20 < 4 * w * 4 * h)  # what the docstring says
        pin = R.PinnedArray((nbytes,))
        try:
            spec = s.process_fmt(img, U16, out_fmt)  # chunk_mb 16, pageable: one chunk
            pinned = s.process_fmt(img, U16, out_fmt, out=pin.array.view(spec.dtype).reshape(spec.shape))
            s.set_option("chunk_mb", 1)
            got = s.process_fmt(img, U16, out_fmt, out=np.full_like(spec, 0xCD))
            assert spec.nbytes == nbytes and np.array_equal(got, spec) and np.array_equal(got, pinned)
        finally:
            s.set_option("chunk_mb", 16)
            pin.free()


def test_four_threads_on_one_context(ctx):
    """Four threads, each its own images and format pair, next to one another and next to rsr_process on the same context."""
    s = ctx[False]
    s._push_params()
    jobs = [(Z.image16(230, W, H), U16, U16), (image(231, U8, W, H), U8, U16), (Z.image16(232, 40, 30, 4), U16, U16), (Z.image16(233, W, H), U16, U8)]
    want = [s.process_fmt(x, i, o) for x, i, o in jobs]
    img8 = image(234, U8, W, H)
    want8 = s.process(img8)
    errs = []

    def work(k):
        try:
            x, i, o = jobs[k]
            for _ in range(3):
                if not np.array_equal(s.process_fmt(x, i, o), want[k]):
                    errs.append("thread %d: other bytes" % k)
                if k == 0 and not np.array_equal(s.process(img8, push_params=False), want8):
                    errs.append("rsr_process beside them: other bytes")
        except Exception as e:  # noqa: BLE001
            errs.append("thread %d: %r" % (k, e))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs


def test_progress_callback_fires_per_tile(ctx):
    import ctypes as C
    s = ctx[False]
    seen = []
    cb = C.CFUNCTYPE(None, C.c_int, C.c_int, C.c_void_p)(lambda done, total, user: seen.append((done, total)))
    s._L.rsr_set_progress_callback(s._h, C.cast(cb, C.c_void_p), None)
    try:
        s.process_fmt(Z.image16(240, W, H), U16, U16)
    finally:
        s._L.rsr_set_progress_callback(s._h, None, None)
    assert seen == [(i, 6) for i in range(1, 7)]


def test_argument_errors(ctx):
    s = ctx[False]
    L, h_ = s._L, s._h
    x = Z.image16(250, 8, 8)
    out = np.full((32, 32, 3), 0xCDCD, dtype=np.uint16)

    def rc(in_p, in_fmt, w, h, c, out_p, out_fmt):
        return L.rsr_process_fmt(h_, in_p, in_fmt, w, h, c, out_p, out_fmt)

    pi, po = x.ctypes.data, out.ctypes.data
    assert rc(None, U16, 8, 8, 3, po, U16) == R.RSR_E_ARG
    assert rc(pi, U16, 8, 8, 3, None, U16) == R.RSR_E_ARG
    assert rc(pi, U16, 0, 8, 3, po, U16) == R.RSR_E_ARG
    assert rc(pi, U16, 8, 8, 2, po, U16) == R.RSR_E_ARG
    assert rc(pi, U16, 8, 8, 4, po, F32) == R.RSR_E_ARG
    assert rc(pi, 14, 8, 8, 3, po, U16) == R.RSR_E_ARG
    assert rc(pi, U16, 8, 8, 3, po, 17) == R.RSR_E_ARG
    assert rc(pi, NV12, 7, 8, 3, po, U16) == R.RSR_E_ARG
    assert L.rsr_process_fmt(None, pi, U16, 8, 8, 3, po, U16) == R.RSR_E_ARG
    s.out_ratio = (3, 2)
    assert rc(pi, U16, 7, 8, 3, po, U16) == R.RSR_E_ARG
    assert (out == 0xCDCD).all()
    with pytest.raises(ValueError):
        s.process_fmt(x.view(np.int16), U16, U16)
    with pytest.raises(ValueError):
        s.process_fmt(x, U16, U16, out=np.zeros((32, 32, 3), np.uint8))


def test_state_error_before_load():
    s = R.RealSR(0)
    try:
        with pytest.raises(R.RealSRError) as e:
            s.process_fmt(Z.image16(260, 8, 8), U16, U16)
        assert e.value.code == R.RSR_E_STATE
    finally:
        s.close()
