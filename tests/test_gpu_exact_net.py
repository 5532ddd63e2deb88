"""The WHOLE network and the whole tile loop held BIT FOR BIT to the two-term exact model (run with -m gpu on the MI355X box).

Every other check of the whole data path against something that is not the engine itself carries a tolerance (+-1 uint8, 3e-3), which a
defect shared by all of the engine's configurations and worth less than a code passes: a bias or a slope held as fp16, a weight packed
into the wrong row, a residual read from the wrong RDB, a TTA variant inverted with the wrong transform.  tests/exact_net.py builds a
model whose accumulators have at most two non-zero terms -- one right answer whatever the summation order -- and restates the rounding
steps in numpy; here the 351 convs in production order, packed weight images, tile batches, trimmed rectangles, folded columns, TTA, the
fused conv_last output, the float formats and the reduced outputs are compared with np.array_equal.  tests/test_exact_net.py (CPU)
shows that the model is healthy on these very inputs and that deliberate sub-code defects of the mirror are seen."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import exact_conv as X
import exact_net as N
import realsr_ncnn_vulkan_amd as R
from area_reduce import area_reduce
from box_reduce import box_reduce
from realsr_ncnn_vulkan_amd import synth, torch_io

pytestmark = pytest.mark.gpu

U8, F16, F32 = R.RSR_FMT_U8_HWC, R.RSR_FMT_F16_CHW, R.RSR_FMT_F32_CHW
COMBOS = ((0, 0, 256), (3, 0, 256), (4, 0, 8), (0, 32, 8))   # (flow_flags, dbg, num_cu): see tests/test_gpu_exact.py
W, H, T = N.FRAME


def _model_dir(root, model):
    d = str(root)
    synth.write_param(os.path.join(d, "x4.param"))
    synth.write_bin(os.path.join(d, "x4.bin"), N.dense_weights(model), "fp16")
    return os.path.join(d, "x4.param"), os.path.join(d, "x4.bin")


@pytest.fixture(scope="module")
def model():
    return N.make_model()


@pytest.fixture(scope="module")
def paths(model, tmp_path_factory):
    return _model_dir(tmp_path_factory.mktemp("exact_net"), model)


@pytest.fixture(scope="module")
def sr(paths):
    s = R.RealSR(0)
    s.load(*paths)
    s.tilesize = T
    yield s
    s.close()


@pytest.fixture(autouse=True)
def back_to_defaults(sr):
    yield
    sr.out_scale = 4
    sr.tilesize = T
    for k, v in (("flow_flags", 0), ("dbg", 0), ("num_cu", 256), ("precise", 0), ("bgr", 0), ("max_workspace_mb", 65536)):
        sr.set_option(k, v)


_refs = {}


def ref_x4(model, key, x16, precise=False):
    """The mirror's x4 image for one input at tile T, computed once per module."""
    if key not in _refs:
        _refs[key] = N.image_x4(model, x16, T, precise=precise)
        _refs[key].setflags(write=False)
    return _refs[key]


def same(got, want, what=""):
    """np.array_equal on the bit patterns (uint8: the bytes); '' or a message with the first mismatch.  Values that differ only in the
    sign of a zero are reported and taken as equal."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.uint8:
        g, w = got, want
    else:
        g, w = (np.ascontiguousarray(a).view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize]) for a in (got, want))
    bad = g != w
    if not bad.any():
        return ""
    if got.dtype != np.uint8 and ((got == 0) & (want == 0))[bad].all():
        print("%s: %d values differ only in the sign of a zero: taken as equal" % (what, int(bad.sum())))
        return ""
    i = tuple(np.argwhere(bad)[0])
    return "%s: %d of %d values differ, first at %s: got %r (0x%x) want %r (0x%x)" % (
        what, int(bad.sum()), g.size, i, got[i].item(), int(g[i]), want[i].item(), int(w[i]))


def hwc(planar_u8):
    return np.ascontiguousarray(planar_u8.transpose(1, 2, 0))


def device_call(s, x, in_fmt, out_fmt):
    """One synchronous rsr_process_device_fmt call on the packed numpy image x at the context's output ratio."""
    w, h = (x.shape[1], x.shape[0]) if in_fmt == U8 else (x.shape[2], x.shape[1])
    ow, oh = s.out_size(w, h)
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if out_fmt == U8:
        d_out = torch.full((oh, ow, 3), 0xCD, dtype=torch.uint8, device="cuda")
    else:
        d_out = torch.full((3, oh, ow), float("nan"), dtype=torch.float16 if out_fmt == F16 else torch.float32, device="cuda")
    torch.cuda.synchronize()   # (the fills above run on torch's null stream, the call on the context's own non-blocking stream)
    s.process_device_fmt(d_in.data_ptr(), in_fmt, w, h, 3, d_out.data_ptr(), out_fmt)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert out_fmt == U8 or not np.isnan(got).any()   # every element was written
    return got


# ---- the network, one tile per call -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", N.TILE_SHAPES)
def test_net_forward_tiles(sr, model, h, w):
    """(20, 44): a folded last block column 12 wide (24 / 48 behind the up-samplings); (33, 35): 3 -> 6 -> 12; (16, 32): exact blocks;
    (17, 65): one row and one column over.  8 x 32 / 4 x 64 waves, weights resident / streamed, rows below the tile skipped / computed."""
    x = N.tile_f16(h, w)
    want = X.f16(N.forward(model, x))
    for flags, dbg, ncu in COMBOS:
        for k, v in (("flow_flags", flags), ("dbg", dbg), ("num_cu", ncu)):
            sr.set_option(k, v)
        msg = same(sr.net_forward(x), want, "net_forward %dx%d" % (h, w))
        assert not msg, ((flags, dbg, ncu), msg)


# ---- process(): the tile loop, uint8 -----------------------------------------------------------------------------------------------
def test_process_rgb(sr, model):
    """50 x 40 at tile 24: 3 x 2 tiles, the last column 2 px wide; in one batch, and in several (a workspace budget of two tiles)."""
    img = N.frame_u8(W, H)
    want = hwc(N.to_u8(ref_x4(model, "u8", N.halfs_of_u8(img))))
    msg = same(sr.process(img), want, "process")
    assert not msg, msg
    assert sr.get_stat("plan_batches") == 1
    sr.set_option("max_workspace_mb", 30)
    got = sr.process(img)
    assert sr.get_stat("plan_batches") > 1
    msg = same(got, want, "process in %d batches" % sr.get_stat("plan_batches"))
    assert not msg, msg


def test_process_rgba(sr, model):
    """The RGB bytes of an RGBA image (its own planar conv_last output and post-processing kernel); alpha is bicubic, not the network's."""
    img = N.frame_u8(W, H, 4)
    want = hwc(N.to_u8(ref_x4(model, "rgba", N.halfs_of_u8(img))))
    got = sr.process(img)
    assert got.shape == (4 * H, 4 * W, 4)
    msg = same(np.ascontiguousarray(got[:, :, :3]), want, "process RGBA")
    assert not msg, msg


def test_process_bgr(sr, model):
    """bgr = 1: the network sees the channels reversed and the output is reversed back."""
    img = N.frame_u8(W, H)
    want = hwc(N.to_u8(ref_x4(model, "bgr", N.halfs_of_u8(img[:, :, ::-1]))))[:, :, ::-1]
    sr.set_option("bgr", 1)
    msg = same(sr.process(img), np.ascontiguousarray(want), "process bgr")
    assert not msg, msg


def test_process_tta(tmp_path_factory):
    """A TTA context on 30 x 26 at tile 16: eight variants per tile, each inverted with its own transform, summed in fp32 in the
    shader's order.  (Its own model: the mean of eight outputs needs a louder conv_last to reach both clamps.)"""
    model = N.make_model(**N.TTA_GAINS)
    s = R.RealSR(0, tta_mode=True)
    try:
        s.load(*_model_dir(tmp_path_factory.mktemp("exact_net_tta"), model))
        s.tilesize = N.TTA_FRAME[2]
        img = N.tta_frame()
        want = hwc(N.to_u8(N.image_x4(model, N.halfs_of_u8(img), N.TTA_FRAME[2], tta=True)))
        msg = same(s.process(img), want, "process TTA")
        assert not msg, msg
    finally:
        s.close()


# ---- the float formats: the network's exact output value, not only its byte ----------------------------------------------------------
def test_float_formats(sr, model):
    """The 50 x 40 frame as general fp16: F16 -> F32, F32 -> F16 (device calls) and fp16 / fp32 tensors through torch_io.upscale."""
    x = N.frame_f16(W, H)
    want = N.to_unit(ref_x4(model, "f16", x))
    assert np.array_equal(want.astype(np.float16).astype(np.float32), want)   # (the default path's value IS an fp16)
    for name, got in (("F16 -> F32", device_call(sr, x, F16, F32)),
                      ("F32 -> F16", device_call(sr, x.astype(np.float32), F32, F16).astype(np.float32)),
                      ("upscale fp16", torch_io.upscale(sr, torch.from_numpy(x).cuda()).cpu().numpy().astype(np.float32)),
                      ("upscale fp32", torch_io.upscale(sr, torch.from_numpy(x.astype(np.float32)).cuda()).cpu().numpy())):
        msg = same(got, want, name)
        assert not msg, msg


# ---- reduced outputs --------------------------------------------------------------------------------------------------------------
def test_out_scale_2(sr, model):
    """uint8 in, F32 out at out_scale 2: tests/box_reduce.py of the mirror's x4 image."""
    img = N.frame_u8(W, H)
    want = box_reduce(ref_x4(model, "u8", N.halfs_of_u8(img)), 2)
    sr.out_scale = 2
    msg = same(device_call(sr, img, U8, F32), want, "out_scale 2")
    assert not msg, msg


def test_out_ratio_3_2(sr, model):
    """uint8 in, F32 out at ratio 3/2 (tile 24 -> 36 output pixels): tests/area_reduce.py of the mirror's x4 image."""
    img = N.frame_u8(W, H)
    want = area_reduce(ref_x4(model, "u8", N.halfs_of_u8(img)), 3, 2)
    sr.out_ratio = Fraction(3, 2)
    msg = same(device_call(sr, img, U8, F32), want, "out_ratio 3/2")
    assert not msg, msg


# ---- precise mode ---------------------------------------------------------------------------------------------------------------
def test_precise_mode(sr, model):
    """Option "precise" = 1: the hi + lo / 2048 residual stream through all 23 RRDBs and conv_last's unrounded fp32 result -- one tile
    through rsr_net_forward_f32, and the 50 x 40 frame to uint8."""
    sr.set_option("precise", 1)
    x = N.tile_f16(*N.TILE_SHAPES[0])
    want = N.forward(model, x, precise=True)
    assert not np.array_equal(X.f16(want), X.f16(N.forward(model, x)))   # (another stream than the default one)
    for flags, dbg, ncu in COMBOS:
        for k, v in (("flow_flags", flags), ("dbg", dbg), ("num_cu", ncu)):
            sr.set_option(k, v)
        msg = same(sr.net_forward_f32(x), want, "net_forward_f32")
        assert not msg, ((flags, dbg, ncu), msg)
    for k, v in (("flow_flags", 0), ("dbg", 0), ("num_cu", 256)):
        sr.set_option(k, v)
    img = N.frame_u8(W, H)
    msg = same(sr.process(img), hwc(N.to_u8(ref_x4(model, "u8 precise", N.halfs_of_u8(img), precise=True))), "process, precise")
    assert not msg, msg
