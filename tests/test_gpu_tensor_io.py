"""Planar fp16 / fp32 device images (rsr_process_device_fmt) and torch_io.upscale on the GPU (run with -m gpu).

Everything here is EXACT: the float formats are tied to the uint8 path bit for bit (the uint8 path's own parity against the oracle is
tests/test_gpu_parity.py), so no tolerance appears anywhere.

    input side    u8 -> u8  ==  f16 -> u8 with x = fp16(float32(k) * float32(1/255))  ==  f32 -> u8 with x = float32(k) * float32(1/255)
    output side   q(u8 -> f32) == u8 -> u8 with q(v) = clip(floor(v * 255 + 0.5), 0, 255);  u8 -> f16 == fp16(u8 -> f32)

In the default non-TTA mode the f32 output is an fp16 value and v * 255 + 0.5 is exact in float32 whether or not the device contracts it
into an fma: every element is compared.  In the TTA and precise modes v is a general float32; there E = float64(v) * 255 + 0.5 is
evaluated exactly on the host and the elements where E lies within 2^-14 of an integer are left out (two float32 roundings at magnitude
< 256 move E by at most 2^-16); the test asserts that this leaves out at most 0.1 % of a frame.
"""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

import gpu_support as G
from gpu_support import context_fixtures, paths  # noqa: F401
from pixfmt_ref import F16, F32, NP, U8, u8_image as image

pytestmark = pytest.mark.gpu
# (w, h, tilesize): smaller than a tile | partial last tiles in both directions at tile 32 | the same with a last tile column of 21 + 2 * 10
# = 41 padded pixels: 9 behind a 32-column block at LR and 4 * 41 = 5 * 32 + 4 at 4x, i.e. folded last columns (kernels.h kFoldBit) |
# tile 100 with partial last tiles both ways and a folded last column (121 = 100 + 21)
GEOS = [(40, 30, 100), (61, 47, 32), (53, 47, 32), (121, 110, 100)]


ctxs, back_to_defaults = context_fixtures(autouse=True)


def as_planar(img, fmt):
    """The planar float image whose network input is exactly the uint8 path's: float32(k) * float32(1/255) [rounded to fp16]."""
    x = img.astype(np.float32) * np.float32(1 / 255.0)
    return np.ascontiguousarray(x.transpose(2, 0, 1)).astype(NP[fmt])


def out_buffer(fmt, w, h, c=3):
    """The destination, pre-filled with what no call writes (NaN / 0xCD): an element the engine leaves out shows."""
    if fmt == U8:
        return torch.full((4 * h, 4 * w, c), 0xCD, dtype=torch.uint8, device="cuda")
    return torch.full((3, 4 * h, 4 * w), float("nan"), dtype=torch.float16 if fmt == F16 else torch.float32, device="cuda")


def run(s, x, in_fmt, out_fmt, stream=None):
    """One synchronous rsr_process_device_fmt call on the numpy image x; returns the output as numpy."""
    return G.run(s, x, in_fmt, out_fmt, nan=True, stream=stream)


def quantise(v):
    return np.clip(np.floor(v.astype(np.float32) * np.float32(255) + np.float32(0.5)), 0, 255).astype(np.uint8)


def check_formats_against_u8(s, img, every_element):
    """Items 1-3 of the module docstring for one image in the context's current mode.  Returns the u8 -> u8 bytes."""
    ref = run(s, img, U8, U8)
    assert not (ref == 0xCD).all()
    # 1. input side
    assert np.array_equal(run(s, as_planar(img, F16), F16, U8), ref)
    assert np.array_equal(run(s, as_planar(img, F32), F32, U8), ref)
    # 2. output side
    v = run(s, img, U8, F32)
    assert v.dtype == np.float32 and v.shape == (3,) + ref.shape[:2]
    assert np.isfinite(v).all() and v.min() >= 0.0 and v.max() <= 1.0
    want = ref.transpose(2, 0, 1)
    if every_element:
        assert np.array_equal(v.astype(np.float16).astype(np.float32), v)  # fp16 values: v * 255 + 0.5 is exact in float32
        assert np.array_equal(quantise(v), want)
    else:
        E = v.astype(np.float64) * 255.0 + 0.5
        near = np.abs(E - np.rint(E)) < 2.0 ** -14
        assert near.mean() <= 1e-3, near.mean()
        assert np.array_equal(np.clip(np.floor(E), 0, 255).astype(np.uint8)[~near], want[~near])
    # 3. the fp16 output is the fp32 output rounded once
    v16 = run(s, img, U8, F16)
    assert v16.dtype == np.float16 and np.array_equal(v16.view(np.uint16), v.astype(np.float16).view(np.uint16))
    return ref


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
@pytest.mark.parametrize("precise", [0, 1], ids=["fp16", "precise"])
@pytest.mark.parametrize("w,h,T", GEOS)
def test_float_formats_equal_the_uint8_path(ctxs, w, h, T, precise, tta):
    s = ctxs[tta]
    s.tilesize = T
    s.set_option("precise", precise)
    try:
        check_formats_against_u8(s, image(w * 1000 + h + T, w, h), every_element=not tta and not precise)
    finally:
        s.set_option("precise", 0)


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_bgr_swaps_planes_like_bytes(ctxs, tta):
    """Option "bgr": plane p of a planar image is byte p of the uint8 pixel, on both sides; and the option does change the result."""
    s = ctxs[tta]
    s.tilesize = 32
    img = image(5, 53, 47)
    rgb = run(s, img, U8, U8)
    s.set_option("bgr", 1)
    try:
        bgr = check_formats_against_u8(s, img, every_element=not tta)
        assert not np.array_equal(bgr, rgb)
        assert np.array_equal(run(s, np.ascontiguousarray(img[:, :, ::-1]), U8, U8)[:, :, ::-1], rgb)
    finally:
        s.set_option("bgr", 0)


@pytest.mark.parametrize("precise", [0, 1], ids=["fp16", "precise"])
def test_unfused_route_gives_the_same_images(ctxs, precise):
    """dbg 8192: conv_last leaves its planar blob and postproc_tiles writes the image (the route TTA always takes), also in its LDS-staged
    form (dbg 65536): same bytes as the fused store, in every format."""
    s = ctxs[False]
    s.tilesize = 32
    img = image(6, 53, 47)
    s.set_option("precise", precise)
    try:
        fused = {f: run(s, img, U8, f) for f in (U8, F16, F32)}
        for dbg in (8192, 8192 | 65536, 8192 | 32768):
            s.set_option("dbg", dbg)
            assert np.array_equal(check_formats_against_u8(s, img, every_element=not precise), fused[U8])
            for f in (F16, F32):
                assert np.array_equal(run(s, img, U8, f).view(np.uint8), fused[f].view(np.uint8)), (dbg, f)
    finally:
        s.set_option("dbg", 0)
        s.set_option("precise", 0)


def test_tta_per_pixel_and_staged_postproc_agree(ctxs):
    """Under TTA the LDS-staged post kernel is the default; the one-thread-per-pixel kernel (dbg 32768) writes the same float images."""
    s = ctxs[True]
    s.tilesize = 32
    img = image(8, 53, 47)
    staged = {f: run(s, img, U8, f) for f in (U8, F16, F32)}
    s.set_option("dbg", 32768)
    try:
        for f in (U8, F16, F32):
            assert np.array_equal(run(s, img, U8, f).view(np.uint8), staged[f].view(np.uint8)), f
    finally:
        s.set_option("dbg", 0)


def test_sub_8_bit_input_really_arrives(ctxs):
    """One image that fits one tile, fp16 values OFF the k/255 grid: f16 -> f16 is the network itself on the reflect-padded image, clamped
    and cropped (same kernels, same summation order).  The same values as float32 with low-order bits below half an fp16 ulp round to
    the same halfs (RNE).  Snapping x to the k/255 grid first gives another output: the test can see the feature."""
    s = ctxs[False]
    s.tilesize = 64
    P = s.prepadding
    rng = np.random.default_rng(11)
    x = (rng.random((3, 37, 45), dtype=np.float32) * 0.98 + 0.01).astype(np.float16)
    grid = (np.rint(x.astype(np.float32) * 255).astype(np.float32) * np.float32(1 / 255.0)).astype(np.float16)
    assert (x != grid).mean() > 0.5
    net = s.net_forward(np.pad(x, ((0, 0), (P, P), (P, P)), mode="reflect"))
    want = np.clip(net, 0, 1)[:, 4 * P:-4 * P, 4 * P:-4 * P]
    got = run(s, x, F16, F16)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint16), want.view(np.uint16))
    # float32 input: rounded to nearest even
    x32 = x.astype(np.float32) + (np.spacing(x).astype(np.float32) * np.float32(0.2) * rng.choice([-1, 1], size=x.shape).astype(np.float32))
    assert (x32 != x.astype(np.float32)).all() and np.array_equal(x32.astype(np.float16).view(np.uint16), x.view(np.uint16))
    assert np.array_equal(run(s, x32, F32, F16).view(np.uint16), got.view(np.uint16))
    assert np.array_equal(run(s, x32, F32, F32), got.astype(np.float32))
    # ties go to the even half: x + exactly half an ulp
    tie = x.astype(np.float32) + np.spacing(x).astype(np.float32) * np.float32(0.5)
    assert np.array_equal(run(s, tie, F32, F16).view(np.uint16), run(s, tie.astype(np.float16), F16, F16).view(np.uint16))
    # the uint8 detour loses it
    snapped = run(s, grid, F16, F16)
    assert not np.array_equal(snapped.view(np.uint16), got.view(np.uint16))
    assert np.array_equal(quantise(snapped), run(s, np.ascontiguousarray(np.rint(x.astype(np.float32) * 255).astype(np.uint8).transpose(1, 2, 0)), U8, U8).transpose(2, 0, 1))


def profile_and_run(s, x, in_fmt, out_fmt):
    s.get_profile(reset=True)
    out = run(s, x, in_fmt, out_fmt)
    return s.get_profile(reset=True), out


@pytest.mark.parametrize("precise", [0, 1], ids=["fp16", "precise"])
@pytest.mark.parametrize("flow_flags", [0, 8], ids=["last3", "generic"])
def test_fusion_is_kept_and_plans_are_shared(ctxs, precise, flow_flags):
    """Non-TTA: the float image leaves conv_last itself -- as many conv launches as the uint8 call, no post kernel -- through both forms of
    conv_last (flow_flags bit 3: the generic path); a float call of a geometry the uint8 path has planned adds no plan; profiling accounts
    the bytes of the formats."""
    s = ctxs[False]
    s.tilesize = 32
    s.set_option("precise", precise)
    s.set_option("flow_flags", flow_flags)
    s.set_option("merge", 1)
    s.set_profiling(True)
    try:
        img = image(21, 61, 47)
        p_u8, ref = profile_and_run(s, img, U8, U8)
        plans = s.get_stat("plans")
        p_a, a = profile_and_run(s, img, U8, F16)
        p_b, b = profile_and_run(s, as_planar(img, F16), F16, F32)
        assert s.get_stat("plans") == plans
        assert p_u8["conv_launches"] == R.NUM_CONVS and p_u8["post_ms"] == 0 and p_u8["post_bytes"] == 0
        for p in (p_a, p_b):
            assert p["conv_launches"] == p_u8["conv_launches"] and p["post_ms"] == 0 and p["post_bytes"] == 0 and p["calls"] == 1
        if not precise:
            assert np.array_equal(quantise(b), ref.transpose(2, 0, 1))
        assert np.array_equal(a.view(np.uint16), b.astype(np.float16).view(np.uint16))
        # per padded-tile pixel the pre kernel reads 3 bytes of a uint8 image or 6 of an fp16 one, and writes 64
        assert p_a["pre_bytes"] == p_u8["pre_bytes"] and p_b["pre_bytes"] == pytest.approx(p_u8["pre_bytes"] * (6 + 64) / (3 + 64))
        # the unfused route: one post launch, whose bytes follow the output format
        s.set_option("dbg", 8192)
        q_u8, _ = profile_and_run(s, img, U8, U8)
        q_f32, _ = profile_and_run(s, img, U8, F32)
        assert q_u8["post_ms"] > 0 and q_f32["post_ms"] > 0 and q_f32["conv_launches"] == q_u8["conv_launches"]
        assert q_f32["post_bytes"] == pytest.approx(q_u8["post_bytes"] * (6 + 12) / (6 + 3))  # per output pixel: the blob read + the image written
        assert s.get_stat("plans") == plans
    finally:
        s.set_profiling(False)
        s.set_option("dbg", 0)
        s.set_option("flow_flags", 0)
        s.set_option("merge", 16)
        s.set_option("precise", 0)


def test_float_calls_next_to_merging_uint8_calls(ctxs):
    """Eight threads on one context, small images: half of them u8 -> u8 through process_device (these merge), half f16 -> f32 (these do
    not); every output equals what the same call gives alone."""
    s = ctxs[False]
    s.tilesize = 64
    w, h = 90, 70
    imgs = [image(400 + i, w, h) for i in range(16)]
    fmt = [(U8, U8) if (i // 2) % 2 == 0 else (F16, F32) for i in range(16)]  # threads 0, 2, 4, 6: uint8; 1, 3, 5, 7: float
    src = [im if f[0] == U8 else as_planar(im, F16) for im, f in zip(imgs, fmt)]
    s.set_option("merge", 1)
    lone = [run(s, x, f[0], f[1]) for x, f in zip(src, fmt)]
    s.set_option("merge", 16)
    d_in = [torch.from_numpy(x).cuda() for x in src]
    d_out = [out_buffer(f[1], w, h) for f in fmt]
    torch.cuda.synchronize()
    errs = []

    def work(t):
        try:
            for i in (2 * t, 2 * t + 1):
                if fmt[i][0] == U8:
                    s.process_device(d_in[i].data_ptr(), w, h, 3, d_out[i].data_ptr())
                else:
                    s.process_device_fmt(d_in[i].data_ptr(), F16, w, h, 3, d_out[i].data_ptr(), F32)
        except Exception as e:  # noqa: BLE001
            errs.append((t, repr(e)))
    th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    torch.cuda.synchronize()
    for i in range(16):
        assert np.array_equal(d_out[i].cpu().numpy().view(np.uint8), lone[i].view(np.uint8)), i
    for i in range(16):  # and the float outputs are the uint8 ones
        if fmt[i][0] != U8:
            assert np.array_equal(quantise(lone[i]), run(s, imgs[i], U8, U8).transpose(2, 0, 1))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_upscale_on_a_torch_stream(ctxs, dtype):
    """torch_io.upscale on a non-default stream, its input made by a torch op on that stream just before, no host synchronisation in
    between: equals the synchronous call.  First with the engine idle (the kernels go onto the caller's stream: stat device_direct), then
    with the engine busy (the ordered path through the context's compute stream)."""
    s = ctxs[False]
    s.tilesize = 32
    w, h = 61, 47
    fmt = F16 if dtype == torch.float16 else F32
    x_np = as_planar(image(31, w, h), fmt)
    want = run(s, x_np, fmt, fmt)
    base = torch.from_numpy(x_np).cuda()
    st, other = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    n0 = s.get_stat("device_direct")
    with torch.cuda.stream(st):
        x = (base * 2) * 0.5  # exact; produced on `st`
        y = torch_io.upscale(s, x)
        y_copy = y.clone()
    st.synchronize()
    assert s.get_stat("device_direct") == n0 + 1
    assert y.dtype == dtype and tuple(y.shape) == (3, 4 * h, 4 * w) and y.is_contiguous()
    assert np.array_equal(y_copy.cpu().numpy().view(np.uint8), want.view(np.uint8))
    # engine busy: a call sits behind a device-side sleep on another stream.  Whether that call itself went onto its caller's stream (then
    # the compute stream waits for its last kernel) or through the compute stream (then its kernels wait there for the sleep) -- streams
    # may share a hardware queue, which makes an idle stream look busy -- the compute stream has work pending while the sleep lasts.
    torch.cuda.synchronize()
    with torch.cuda.stream(other):
        torch.cuda._sleep(50_000_000)
        y_slow = torch_io.upscale(s, base)
    n1 = s.get_stat("device_direct")
    with torch.cuda.stream(st):
        x2 = (base * 2) * 0.5
        y2 = torch_io.upscale(s, x2)  # the ordered path through the compute stream
        y2_copy = y2.clone()
    assert s.get_stat("device_direct") == n1
    st.synchronize()
    other.synchronize()
    assert np.array_equal(y2_copy.cpu().numpy().view(np.uint8), want.view(np.uint8))
    assert np.array_equal(y_slow.cpu().numpy().view(np.uint8), want.view(np.uint8))
    torch.cuda.synchronize()


def test_upscale_layouts(ctxs):
    """(N, 3, H, W) equals N single calls; uint8 (H, W, 4) equals process_device; non-contiguous input is made contiguous; the default
    stream works; under TTA too."""
    s = ctxs[False]
    s.tilesize = 32
    w, h = 45, 33
    imgs = [image(50 + i, w, h) for i in range(3)]
    singles = [run(s, as_planar(im, F32), F32, F32) for im in imgs]
    batch = torch.from_numpy(np.stack([as_planar(im, F32) for im in imgs])).cuda()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        y = torch_io.upscale(s, batch * 1.0)
    st.synchronize()
    assert tuple(y.shape) == (3, 3, 4 * h, 4 * w) and y.dtype == torch.float32
    for i in range(3):
        assert np.array_equal(y[i].cpu().numpy(), singles[i]), i
    # default stream, fp16, non-contiguous (a flipped view and an HWC-stored image seen as CHW)
    x16 = torch.from_numpy(as_planar(imgs[0], F16)).cuda()
    y16 = torch_io.upscale(s, x16)
    torch.cuda.synchronize()
    assert np.array_equal(y16.cpu().numpy().view(np.uint16), singles[0].astype(np.float16).view(np.uint16))
    hwc = x16.permute(1, 2, 0).contiguous()
    view = hwc.permute(2, 0, 1)
    assert not view.is_contiguous()
    y_view = torch_io.upscale(s, view)
    torch.cuda.synchronize()
    assert y_view.is_contiguous() and torch.equal(y_view, y16)
    # uint8 HWC with alpha
    rgba = image(60, w, h, 4)
    d_in = torch.from_numpy(rgba).cuda()
    d_out = out_buffer(U8, w, h, 4)
    s.process_device(d_in.data_ptr(), w, h, 4, d_out.data_ptr())
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        y8 = torch_io.upscale(s, d_in)
    st.synchronize()
    assert y8.dtype == torch.uint8 and tuple(y8.shape) == (4 * h, 4 * w, 4) and torch.equal(y8, d_out)
    # TTA context
    t = ctxs[True]
    t.tilesize = 32
    want = run(t, as_planar(imgs[1], F16), F16, F16)
    with torch.cuda.stream(st):
        yt = torch_io.upscale(t, torch.from_numpy(as_planar(imgs[1], F16)).cuda())
    st.synchronize()
    assert np.array_equal(yt.cpu().numpy().view(np.uint16), want.view(np.uint16))
    # wrong device / dtype / shape: refused before anything is launched
    n = s.get_stat("device_direct")
    for bad in (x16.cpu(), x16.double(), x16[:2], x16.permute(1, 2, 0), d_in.permute(2, 0, 1)):
        with pytest.raises(ValueError):
            torch_io.upscale(s, bad)
    assert s.get_stat("device_direct") == n


def test_errors_leave_the_context_usable(ctxs, paths):
    s = ctxs[False]
    s.tilesize = 32
    L = s._L
    img = image(70, 40, 30)
    ref = run(s, img, U8, U8)
    d_in = torch.from_numpy(as_planar(img, F32)).cuda()
    d_rgba = torch.zeros((30, 40, 4), dtype=torch.uint8, device="cuda")
    d_out = out_buffer(F32, 40, 30)
    d_out4 = torch.zeros((4, 120, 160), dtype=torch.float32, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert L.rsr_process_device_fmt(s._h, vp(d_in), F32, 40, 30, 4, vp(d_out4), F32, None) == R.RSR_E_ARG   # planar + c = 4
    assert L.rsr_process_device_fmt(s._h, vp(d_rgba), U8, 40, 30, 4, vp(d_out4), F16, None) == R.RSR_E_ARG  # ... on the output side
    assert L.rsr_process_device_fmt(s._h, vp(d_in), F16, 40, 30, 4, vp(d_out4), U8, None) == R.RSR_E_ARG    # ... on the input side
    assert L.rsr_process_device_fmt(s._h, vp(d_in), 7, 40, 30, 3, vp(d_out), F32, None) == R.RSR_E_ARG      # unknown format
    assert L.rsr_process_device_fmt(s._h, vp(d_in), F32, 40, 30, 3, vp(d_out), 7, None) == R.RSR_E_ARG
    assert L.rsr_process_device_fmt(s._h, vp(d_in), F32, 40, 30, 3, vp(d_out), -1, None) == R.RSR_E_ARG
    assert L.rsr_process_device_fmt(s._h, vp(d_in), F32, 0, 30, 3, vp(d_out), F32, None) == R.RSR_E_ARG
    assert L.rsr_process_device_fmt(s._h, None, F32, 40, 30, 3, vp(d_out), F32, None) == R.RSR_E_ARG
    assert b"format" in L.rsr_last_error(s._h) or b"image" in L.rsr_last_error(s._h)
    torch.cuda.synchronize()
    assert torch.isnan(d_out).all()  # nothing was written
    fresh = R.RealSR(0)
    try:
        assert L.rsr_process_device_fmt(fresh._h, vp(d_in), F32, 40, 30, 3, vp(d_out), F32, None) == R.RSR_E_STATE  # before load
        st = torch.cuda.Stream()
        assert L.rsr_process_device_fmt(fresh._h, vp(d_in), F32, 40, 30, 3, vp(d_out), F32, C.c_void_p(st.cuda_stream)) == R.RSR_E_STATE
        fresh.load(*paths)
        fresh.tilesize = 32
        assert np.array_equal(quantise(run(fresh, as_planar(img, F32), F32, F32)), ref.transpose(2, 0, 1))
    finally:
        fresh.close()
    # a good call afterwards still works, and rsr_process_device is the U8 / U8 case
    assert np.array_equal(quantise(run(s, as_planar(img, F32), F32, F32)), ref.transpose(2, 0, 1))
    d8 = torch.from_numpy(img).cuda()
    o8 = out_buffer(U8, 40, 30)
    s.process_device(d8.data_ptr(), 40, 30, 3, o8.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(o8.cpu().numpy(), ref)
