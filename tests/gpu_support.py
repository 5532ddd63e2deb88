"""What the GPU test modules share beyond tests/pixfmt_ref.py: the contexts and their reset, host <-> device copies of packed numpy images,
one synchronous device call, a profiled call, and the tables several modules parametrise over.  torch and the library are imported here;
the numpy-only helpers live in pixfmt_ref."""
import os

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R

import pixfmt_ref as F

# what a context holds at creation (engine.h): every option a module changes goes back to it around every test
DEFAULTS = (("precise", 0), ("out_scale", 4), ("yuv_matrix", 709), ("yuv_range", 0), ("yuv_siting", 0), ("merge", 16), ("bgr", 0), ("dbg", 0),
            ("max_workspace_mb", 65536))
# (tta, dbg) of the five routes a batch takes: fused, unfused, unfused and staged, TTA, TTA staged
ROUTES = [(False, 0), (False, 8192), (False, 8192 | 65536), (True, 0), (True, 65536)]
ROUTE_IDS = ["fused", "unfused", "unfused-staged", "tta", "tta-staged"]
# (id, fmt, c) of the families rsr_diff_tiles came with
DIFF_FORMATS = [("u8c3", F.U8, 3), ("u8c4", F.U8, 4), ("f16", F.F16, 3), ("f32", F.F32, 3), ("nv12", F.NV12, 3), ("p010", F.P010, 3)]
DIFF_FORMAT_IDS = [f[0] for f in DIFF_FORMATS]
TORCH = {F.U8: torch.uint8, F.F16: torch.float16, F.F32: torch.float32}


@pytest.fixture(scope="module")
def paths(model_dir):
    return os.path.join(model_dir, "x4.param"), os.path.join(model_dir, "x4.bin")


def reset(s, tilesize=None, prepadding=None):
    """Every option back to its default, profiling off; the tile geometry to the module's (None: left as it is)."""
    if tilesize is not None:
        s.tilesize, s.prepadding = tilesize, prepadding
    for key, v in DEFAULTS:
        s.set_option(key, v)
    s.set_profiling(False)
    assert s.yuv_siting == 0


def context_fixtures(tilesize=None, prepadding=10, others=(), autouse=False):
    """The fixtures (ctxs, ctx) of one test module -- assign them to these names in the module, beside the imported `paths`.
    ctxs, per module: one loaded context per TTA setting (it is fixed at creation; everything else is an option of a call) under the keys
    False and True, further plain ones under the keys `others`; closed at teardown.
    ctx, per test (autouse: around every test of the module, asked for or not): ctxs, reset before and after the test."""
    @pytest.fixture(scope="module")
    def ctxs(paths):
        made = {}
        for key in (False, True) + tuple(others):
            made[key] = R.RealSR(0, tta_mode=key is True)
            made[key].load(*paths)
        yield made
        for s in made.values():
            s.close()

    @pytest.fixture(autouse=autouse)
    def ctx(ctxs):
        for s in ctxs.values():
            reset(s, tilesize, prepadding)
        yield ctxs
        for s in ctxs.values():
            reset(s, tilesize, prepadding)

    return ctxs, ctx


def dev(x):
    """The bytes of the packed numpy image x as a flat uint8 device tensor."""
    return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()


def host(t, fmt, shape):
    """The device bytes t as a packed numpy image."""
    return t.cpu().numpy().view(np.uint8).reshape(-1).view(F.NP[fmt]).reshape(shape)


def filled(shape, fmt):
    """A device tensor of what no call writes: 0xCD bytes, NaN for a float format."""
    if fmt == F.U8:
        return torch.full(shape, 0xCD, dtype=torch.uint8, device="cuda")
    return torch.full(shape, float("nan"), dtype=TORCH[fmt], device="cuda")


def untouched(t):
    """Does every element of the tensor still hold its fill value?"""
    return bool((t == 0xCD).all()) if t.dtype == torch.uint8 else bool(torch.isnan(t).all())


def out_dims(s, w, h):
    """(ow, oh) at the context's one output ratio, by the definition: w n / d, h n / d."""
    r = s.out_ratio
    return w * r.numerator // r.denominator, h * r.numerator // r.denominator


def profile_of(s, fn, merge=None):
    """(fn(), the profile of the calls it made) -- merge: with that "merge" option, 16 again afterwards."""
    if merge is not None:
        s.set_option("merge", merge)
    s.set_profiling(True)
    s.get_profile(reset=True)
    try:
        out = fn()
        return out, s.get_profile(reset=True)
    finally:
        s.set_profiling(False)
        if merge is not None:
            s.set_option("merge", 16)


def run(s, x, in_fmt, out_fmt, w=None, h=None, c=None, out_size=None, nan=False, stream=None):
    """One synchronous rsr_process_device_fmt call on the packed numpy image x; the result as a packed numpy image.  The destination is
    sized by s.out_size_fmt (or `out_size`) and pre-filled with 0xCD bytes -- nan: a float destination with NaN, and every element of it
    must have been written."""
    if w is None:
        w, h = F.dims_of(in_fmt, x)
    c = c if c is not None else (x.shape[2] if in_fmt == F.U8 else 3)
    ow, oh = out_size if out_size is not None else s.out_size_fmt(out_fmt, w, h)
    assert x.dtype == F.NP[in_fmt] and x.shape == F.shape_of(in_fmt, w, h, c) and x.nbytes == R.image_bytes(in_fmt, w, h, c)
    oshape = F.shape_of(out_fmt, ow, oh, c)
    d_in = dev(x)
    d_out = dev((F.sentinel if nan else F.sentinel_bytes)(out_fmt, oshape))
    assert d_out.numel() == R.image_bytes(out_fmt, ow, oh, c)
    s.process_device_fmt(d_in.data_ptr(), in_fmt, w, h, c, d_out.data_ptr(), out_fmt, stream=stream)
    torch.cuda.synchronize()
    got = host(d_out, out_fmt, oshape)
    assert not (nan and out_fmt in (F.F16, F.F32) and np.isnan(got).any())
    return got
