"""No output depends on stale workspace bytes, and no kernel writes what it does not own (run with -m gpu on the MI355X box).

The exact tests hold every arithmetic step and every tile geometry to a numpy mirror, but their contexts are fresh or module-scoped: a
new or grown workspace is all zeros (Engine::ensure_planes), and zero is also what convolution padding reads through the plane guards.
A loader, residual fetch or post kernel that reads a pixel its call never wrote sees correct padding there; in production the same bytes
hold an earlier frame.  Such pixels exist by design: an edge tile fills part of a slot, merged and masked batches give every slot a full
tile's capacity, TTA puts transposed tiles into equal slots, dead-output elimination leaves whole blocks of the 2x / 4x planes and of
OUT3 unwritten.  Here:

  1. Option "ws_poison": every call starts from a workspace whose every byte holds a pattern, with only the guards (and IN) zeroed -- the
     worst history there is.  0xFFFF is NaN as fp16, as fp32 and as an e5m2 residue byte: on the sparse exact model 0 * NaN = NaN makes
     EVERY tap of every convolution sensitive, but v_med3 / max / min / the final clamps can swallow a NaN.  0x7BFF is 65504 (fp16),
     57344 and NaN (residue bytes), 2.6e36 (fp32): finite, nothing swallows it, but it needs dense weights to matter.  So: the one-block
     exact model under 0xFFFF against the MIRROR, the dense two-block model under both patterns against a FRESH unpoisoned context.
  2. Natural history, no hook: tiles of equal capacity and other shape, a tiny image, a precise toggle and a self-check on ONE context.
  3. Stat "ws_guard_dirty" == 0 after every call: no guard of the layout and none of IN's channels 3 .. 31 was ever written.

Every comparison is np.array_equal; there is no tolerance in this module.  tests/test_ws_hygiene.py (CPU) proves from COVERAGE below
that every case has slot slack or eliminated blocks, and states what the two patterns decode to."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import depth_ref as D
import exact_conv as X
import exact_net as N
import realsr_ncnn_vulkan_amd as R
import test_gpu_exact_geometry as G
from area_reduce import area_reduce
from box_reduce import box_reduce
from gpu_support import dev, filled, run
from pixfmt_ref import F16, F32, NV12, U8, YUV444P10, same_bits
from realsr_ncnn_vulkan_amd import synth, torch_io
from test_gpu_exact_geometry import nets  # noqa: F401  (the fixture: the committed exact models)

pytestmark = pytest.mark.gpu

U16 = R.RSR_FMT_U16_HWC
NAN, BIG = 0x1FFFF, 0x17BFF          # option values: bit 16 + the pattern
PATTERNS = {"nan": NAN, "big": BIG}
# the mirror's other inputs: exact_net.FRAME (50 x 40 at tile 24: 3 x 2 tiles, the last column 2 px wide) for the output paths, two
# net_forward tiles (folded, odd), the self-check's tiles
FW, FH, FT = N.FRAME
NET_TILES = [(20, 44), (33, 35)]
# the dense model's image (tests/test_gpu_workspace_layout.py): three tiles in a row, the last one 6 px wide, slots of 52 x 40
DW, DH, DT = 70, 20, 32
YW = 68                               # the NV12 call at ratio 3/2: 70 * 3 / 2 is odd, 68 -> 102 (tiles 32, 32, 4)
HISTORY = [(32, 20), (20, 32), (1, 1)]  # natural history at tile 32: padded 52 x 40, 40 x 52 (equal capacity), 21 x 21

# ---- what every case runs, for the CPU module: name -> (kind, w, h, tilesize, prepadding, tta) -----------------------------------------
# kind: "plan" = the image's own plan (capacity: its largest padded tile -- a merged plan has more), "full" = slots of a full tile's
# capacity (merged and masked batches, sequences), "tile" = one untrimmed slot of exactly the tile (net_forward, the self-check)
COVERAGE = {}
for _c in G.CASES:
    COVERAGE["mirror " + G.case_id(_c)] = ("plan",) + _c
for _w, _h in G.MIXED:
    COVERAGE["mirror mixed %dx%d" % (_w, _h)] = ("full", _w, _h, G.MIXED_T, 10, 0)
COVERAGE["mirror outputs %dx%d" % (FW, FH)] = ("plan", FW, FH, FT, 10, 0)
for _h, _w in NET_TILES:
    COVERAGE["mirror net_forward %dx%d" % (_w, _h)] = ("tile", _w, _h, max(_w, _h), 0, 0)
for _h, _w in G.CHECK_TILES[1]:
    COVERAGE["mirror selfcheck %dx%d" % (_w, _h)] = ("tile", _w, _h, max(_w, _h), 0, 0)
COVERAGE["fresh %dx%d" % (DW, DH)] = ("plan", DW, DH, DT, 10, 0)
COVERAGE["fresh tta %dx%d" % (DW, DH)] = ("plan", DW, DH, DT, 10, 1)
COVERAGE["fresh masked / sequence %dx%d" % (DW, DH)] = ("full", DW, DH, DT, 10, 0)
COVERAGE["fresh nv12 %dx%d" % (YW, DH)] = ("plan", YW, DH, DT, 10, 0)
for _w, _h in HISTORY:
    COVERAGE["history %dx%d" % (_w, _h)] = ("plan", _w, _h, 32, 10, 0)


def hwc(planar):
    return np.ascontiguousarray(planar.transpose(1, 2, 0))


def clean(s):
    """The two invariants of the workspace's zeros, after a call."""
    n = s.get_stat("ws_guard_dirty")
    assert n == 0, "%d non-zero bytes among the guards of the layout and IN's channels 3 .. 31" % n


def same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if same_bits(got, want):
        return ""
    g, w = (np.ascontiguousarray(a).view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize]) for a in (got, want))
    bad = np.argwhere(g != w)
    i = tuple(bad[0])
    return "%d of %d values differ, first at %s: got %r want %r; index ranges %s" % (
        len(bad), g.size, i, got[i].item(), want[i].item(), [(int(bad[:, k].min()), int(bad[:, k].max())) for k in range(bad.shape[1])])


# ---- 1a. against the mirror: the one-block exact model under 0xFFFF ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def pctxs(nets):
    """tta -> a context holding the one-block exact model."""
    made = {}
    for tta in (0, 1):
        made[tta] = R.RealSR(0, tta_mode=bool(tta))
        made[tta].load(*nets[1][2:])
    yield made
    for s in made.values():
        s.close()


def reset(s, poison=0):
    s.out_scale = 4
    G.reset(s)
    for k, v in (("bgr", 0), ("alpha_net", 0), ("ws_poison", poison)):
        s.set_option(k, v)


@pytest.fixture
def pctx(pctxs):
    for s in pctxs.values():
        reset(s, NAN)
    yield pctxs
    for s in pctxs.values():
        reset(s)


def poisoned_case(pctx, case):
    w, h, T, P, tta = case
    s = pctx[tta]
    s.tilesize, s.prepadding = T, P
    return s, N.frame_u8(w, h)


# (one test per configuration: a case pays for its mirror reference once, in whichever of them runs first)
@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_poisoned_tile_loop_equals_the_mirror(pctx, nets, case):
    """process() in the default configuration, every geometry of the sweep."""
    s, img = poisoned_case(pctx, case)
    msg = G.same8(s.process(img), G.ref_u8(nets, *case))
    clean(s)
    assert not msg, (case, msg)


@pytest.mark.parametrize("case", [c for c in G.CASES if G.ntiles(c) > 1], ids=G.case_id)
def test_poisoned_tile_loop_in_several_batches_equals_the_mirror(pctx, nets, case):
    """Cases of several tiles under a workspace budget of about two tiles: every batch poisons the workspace again."""
    s, img = poisoned_case(pctx, case)
    T, P, tta = case[2:]
    cap = (T + 2 * P) ** 2 * (8 if tta else 1)
    s.set_option("max_workspace_mb", (2 * cap * G.BYTES_PER_PX >> 20) + 1 if G.ntiles(case) > 2 else 1)
    got = s.process(img)
    clean(s)
    nb = s.get_stat("plan_batches")
    assert nb > 1, (case, nb)
    msg = G.same8(got, G.ref_u8(nets, *case))
    assert not msg, (case, "in %d batches" % nb, msg)


@pytest.mark.parametrize("case", G.PRECISE, ids=G.case_id)
def test_poisoned_tile_loop_precise_equals_the_mirror(pctx, nets, case):
    """The PRECISE cases with option "precise" 1: the residue planes start as NaN bytes too."""
    s, img = poisoned_case(pctx, case)
    s.set_option("precise", 1)
    msg = G.same8(s.process(img), G.ref_u8(nets, *case, precise=True))
    clean(s)
    assert not msg, (case, "precise", msg)


def test_poisoned_merged_batch_of_mixed_sizes_equals_the_mirror(pctx, nets):
    """The MIXED process_many call at tile 16: slots of a full tile's capacity (36 x 36) hold images from 1 x 1 to 40 x 33."""
    s = pctx[0]
    s.tilesize = G.MIXED_T
    outs = s.process_many([N.frame_u8(w, h) for w, h in G.MIXED])
    clean(s)
    for (w, h), got in zip(G.MIXED, outs):
        msg = G.same8(got, G.ref_u8(nets, w, h, G.MIXED_T, 10, 0))
        assert not msg, ((w, h), msg)


_x4 = {}


def x4(nets, key, x16):
    """The mirror's x4 image (fp32, before clamp and conversion) of one FRAME-sized input, computed once and left unchanged."""
    if key not in _x4:
        with D.depth(1):
            _x4[key] = N.image_x4(nets[1][1], x16, FT)
        _x4[key].setflags(write=False)
    return _x4[key]


def test_poisoned_rgba_bgr_and_reduced_outputs_equal_the_mirror(pctx, nets):
    """Where the post kernels read OUT3: an RGBA image (its colour against the mirror), option "bgr", out_scale 2 (tests/box_reduce.py)
    and ratio 3/2 (tests/area_reduce.py) of the mirror's x4 image."""
    s = pctx[0]
    s.tilesize = FT
    img4 = N.frame_u8(FW, FH, 4)
    got = s.process(img4)
    clean(s)
    msg = same(np.ascontiguousarray(got[:, :, :3]), hwc(N.to_u8(x4(nets, "rgba", N.halfs_of_u8(img4)))))
    assert not msg, ("RGBA", msg)
    img = N.frame_u8(FW, FH)
    s.set_option("bgr", 1)
    got = s.process(img)
    clean(s)
    msg = same(got, np.ascontiguousarray(hwc(N.to_u8(x4(nets, "bgr", N.halfs_of_u8(img[:, :, ::-1]))))[:, :, ::-1]))
    assert not msg, ("bgr", msg)
    s.set_option("bgr", 0)
    v = x4(nets, "u8", N.halfs_of_u8(img))
    s.out_scale = 2
    got = run(s, img, U8, F32)
    clean(s)
    msg = same(got, box_reduce(v, 2))
    assert not msg, ("out_scale 2", msg)
    s.out_ratio = Fraction(3, 2)
    got = run(s, img, U8, F32)
    clean(s)
    msg = same(got, area_reduce(v, 3, 2))
    assert not msg, ("out_ratio 3/2", msg)


def test_poisoned_float_formats_equal_the_mirror(pctx, nets):
    s = pctx[0]
    s.tilesize = FT
    x = N.frame_f16(FW, FH)
    want = N.to_unit(x4(nets, "f16", x))
    got = run(s, x, F16, F32)
    clean(s)
    msg = same(got, want)
    assert not msg, ("F16 -> F32", msg)
    got = run(s, x.astype(np.float32), F32, F16)
    clean(s)
    msg = same(got.astype(np.float32), want)
    assert not msg, ("F32 -> F16", msg)


@pytest.mark.parametrize("h,w", NET_TILES)
def test_poisoned_net_forward_equals_the_mirror(pctx, nets, h, w):
    """rsr_net_forward and rsr_net_forward_f32 (precise mode) on a folded and an odd tile: one untrimmed slot, every block computed."""
    s, x = pctx[0], N.tile_f16(h, w)
    with D.depth(1):
        want = X.f16(N.forward(nets[1][1], x))
        want_p = N.forward(nets[1][1], x, precise=True)
    msg = same(s.net_forward(x), want)
    assert not msg, ("net_forward", msg)
    clean(s)
    s.set_option("precise", 1)
    msg = same(s.net_forward_f32(x), want_p)
    assert not msg, ("net_forward_f32", msg)
    clean(s)


@pytest.mark.parametrize("h,w", G.CHECK_TILES[1])
def test_poisoned_selfcheck_equals_the_mirror(pctx, nets, h, w):
    """rsr_selfcheck walks the tile in both storages on a poisoned workspace: every peak as a bit pattern, storage_err, max_byte_diff and
    bytes_differ equal mirror_report.  It leaves the workspace without a layout (-1); the next call lays its own out."""
    s = pctx[0]
    G.check_report(s, nets, 1, N.tile_f16(h, w))
    assert s.get_stat("ws_guard_dirty") == -1
    s.tilesize = 32
    msg = G.same8(s.process(N.frame_u8(5, 3)), G.ref_u8(nets, 5, 3, 32, 10, 0))
    assert not msg, msg
    clean(s)


# ---- 1b. against a fresh context: the dense two-block model under both patterns ---------------------------------------------------------
@pytest.fixture(scope="module")
def dense():
    d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K", 42, nb=2)
    return os.path.join(d, "x4.param"), os.path.join(d, "x4.bin")


def context(dense, tta=False):
    s = R.RealSR(0, tta_mode=tta)
    s.load(*dense)
    s.tilesize, s.prepadding = DT, 10
    return s


@pytest.fixture(scope="module")
def dctxs(dense):
    """tta -> the context that gets poisoned."""
    made = {tta: context(dense, tta) for tta in (False, True)}
    yield made
    for s in made.values():
        s.close()


def masked(s, img):
    """One tile of three selected (the narrow last one, in a slot of a full tile's capacity); the whole destination, sentinels included."""
    d_in, d_out = dev(img), filled((4 * DH, 4 * DW, 3), U8)
    torch.cuda.synchronize()
    s.process_device_masked(d_in.data_ptr(), U8, DW, DH, 3, d_out.data_ptr(), U8, np.array([0, 0, 1], np.uint8))
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def sequence(s, frames):
    """Two frames, the middle tile of the second copied from the first."""
    n = 4 * DH * 4 * DW * 3
    d_in, d_out = [dev(f) for f in frames], filled((2, n), U8)
    torch.cuda.synchronize()
    s.process_device_sequence([t.data_ptr() for t in d_in], U8, DW, DH, 3, [d_out[k].data_ptr() for k in range(2)], U8,
                              np.array([[1, 1, 1], [1, 0, 1]], np.uint8))
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def windows(s, imgs):
    """A tensor batch of two pitched windows: crops of a larger surface in, windows of a larger canvas out; the whole canvas."""
    surface = torch.zeros((2, DH + 9, DW + 11, 3), dtype=torch.uint8, device="cuda")
    canvas = filled((2, 4 * DH + 7, 4 * DW + 9, 3), U8)
    crops = [surface[i, 5:5 + DH, 3:3 + DW] for i in range(2)]
    wins = [canvas[i, 3:3 + 4 * DH, 5:5 + 4 * DW] for i in range(2)]
    for c, im in zip(crops, imgs):
        c.copy_(torch.from_numpy(im).cuda())
    torch.cuda.synchronize()
    s.process_device_batch([torch_io.describe(c) for c in crops], U8, DW, DH, 3, [torch_io.describe(w) for w in wins], U8)
    torch.cuda.synchronize()
    return canvas.cpu().numpy()


def nv12(s, surf):
    s.out_ratio = Fraction(3, 2)
    try:
        return run(s, surf, NV12, NV12)
    finally:
        s.out_scale = 4


def with_options(fn, **opts):
    def call(s, *a):
        for k, v in opts.items():
            s.set_option(k, v)
        try:
            return fn(s, *a)
        finally:
            for k in opts:
                s.set_option(k, 16 if k == "merge" else 0)
    return call


def image16(seed):
    return np.random.default_rng(seed).integers(0, 65536, (DH, DW, 4), dtype=np.uint16)


_rng = np.random.default_rng(7020)
# name -> (tta, the call, its input)
CALLS = {
    "c3": (False, lambda s, x: s.process(x), synth.make_image(14, DW, DH, 3)),
    "c4": (False, lambda s, x: s.process(x), synth.make_image(15, DW, DH, 4)),
    "c3 merge 1": (False, with_options(lambda s, x: s.process(x), merge=1), synth.make_image(14, DW, DH, 3)),
    "tta c3": (True, lambda s, x: s.process(x), synth.make_image(14, DW, DH, 3)),
    "tta c4": (True, lambda s, x: s.process(x), synth.make_image(15, DW, DH, 4)),
    "precise c3": (False, with_options(lambda s, x: s.process(x), precise=1), synth.make_image(14, DW, DH, 3)),
    "precise c4": (False, with_options(lambda s, x: s.process(x), precise=1), synth.make_image(15, DW, DH, 4)),
    "alpha_net u8": (False, with_options(lambda s, x: s.process(x), alpha_net=1), synth.make_image(15, DW, DH, 4)),
    "alpha_net u16": (False, with_options(lambda s, x: s.process_fmt(x, U16, U16), alpha_net=1), image16(16)),
    "masked, one tile": (False, masked, synth.make_image(14, DW, DH, 3)),
    "sequence, one tile copied": (False, sequence, [synth.make_image(14, DW, DH, 3), synth.make_image(17, DW, DH, 3)]),
    "two pitched windows": (False, windows, [synth.make_image(14, DW, DH, 3), synth.make_image(17, DW, DH, 3)]),
    "nv12 at 3/2": (False, nv12, _rng.integers(0, 256, (DH * 3 // 2, YW)).astype(np.uint8)),
    "yuv444p10": (False, lambda s, x: run(s, x, YUV444P10, YUV444P10), _rng.integers(0, 1024, (3, DH, DW)).astype(np.uint16)),
}
_fresh = {}


def fresh(dense, name):
    """The call's output on a context made for it alone, without the hook: the reference (tied to the oracle by the rest of the suite).
    Made once per module and left unchanged."""
    if name not in _fresh:
        tta, fn, x = CALLS[name]
        s = context(dense, tta)
        try:
            assert s.get_stat("ws_poison") == 0
            _fresh[name] = fn(s, x).copy()
            clean(s)
        finally:
            s.close()
        _fresh[name].setflags(write=False)
    return _fresh[name]


@pytest.mark.parametrize("name", list(CALLS))
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_poisoned_call_equals_a_fresh_context(dense, dctxs, pattern, name):
    tta, fn, x = CALLS[name]
    want = fresh(dense, name)
    assert len(np.unique(want)) > 16, name
    s = dctxs[tta]
    s.set_option("ws_poison", PATTERNS[pattern])
    try:
        got = fn(s, x)
        clean(s)
    finally:
        s.set_option("ws_poison", 0)
    msg = same(got, want)
    assert not msg, (name, pattern, msg)


# ---- 2. natural history, no hook; 3. guard integrity -----------------------------------------------------------------------------------
def test_natural_history_equals_fresh_contexts(dense):
    """ONE context, merge 1 (the batch is the image's own plan): a 52 x 40 padded tile, then a 40 x 52 one -- the capacity is equal, so
    nothing is zeroed in between --, then 1 x 1, then the second image in precise mode, a self-check, and the first image again.  Each
    output equals a fresh context's, and no guard is dirty after any call (-1 behind the self-check: no layout)."""
    imgs = [synth.make_image(40 + i, w, h, 3) for i, (w, h) in enumerate(HISTORY)]
    steps = [(0, 0), (1, 0), (2, 0), (1, 1), None, (0, 0)]   # (image, precise) | the self-check
    want = {}
    for st in steps:
        if st is not None and st not in want:
            f = context(dense)
            try:
                f.set_option("merge", 1)
                f.set_option("precise", st[1])
                want[st] = f.process(imgs[st[0]]).copy()
            finally:
                f.close()
    s = context(dense)
    try:
        s.set_option("merge", 1)
        assert s.get_stat("ws_guard_dirty") == -1
        for i, st in enumerate(steps):
            if st is None:
                rep = s.selfcheck(w=44, h=20)
                assert rep["nonfinite"] == 0 and s.get_stat("ws_guard_dirty") == -1
                continue
            s.set_option("precise", st[1])
            got = s.process(imgs[st[0]])
            clean(s)
            msg = same(got, want[st])
            assert not msg, ("step %d: image %d, precise %d" % (i, st[0], st[1]), msg)
    finally:
        s.close()
