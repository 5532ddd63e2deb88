"""Conv and tile GEOMETRY swept bit for bit (run with -m gpu on the MI355X box).

tests/test_gpu_exact.py and tests/test_gpu_exact_net.py / test_gpu_depth.py hold every arithmetic step of the engine to an exact
reference, but at a handful of geometries: 14 plane widths, four tiles, one 50 x 40 frame.  The block, strip, fold and margin arithmetic
of conv3x3_flow and the index arithmetic of the host side (tail_margin, append_block_items, the per-slot dims of transposed TTA
variants) is where this project gets rewritten, and a slip there worth less than one uint8 code passes every toleranced test.  Here:

  A. ONE launch per kernel class on exactly summable operands (tests/exact_conv.py) at every plane width 1 .. 66 and every plane height
     1 .. 36: every residue of w % 32 with 0, 1 and 2 full blocks to its left, both sides of the fold limit kFoldMaxW = 14, every residue
     of h % 16 and of the 4-row groups, a pair of block rows plus an unpaired one.  Every launch runs between red zones (option
     "test_redzone", tests/test_gpu_exact.py launch): no byte outside the buffers is written, and the output starts as NaN, not 0.
  B. The tile loop on the ONE-BLOCK exact model (tests/depth_ref.py; 21 convs, every kernel class present, 56 - 119 us per padded pixel in
     the numpy mirror): images smaller than the halo, single rows and columns, tiles larger than the image, padded widths on both sides
     of a block and of the fold limit, the margin rings of other prepaddings, TTA with non-square edge tiles, several batches, precise
     mode, and a merged batch of mixed sizes -- process() against exact_net.image_x4, byte for byte.
  D. The self-check's device reductions (range_probe, output_compare) against the same model, which knows every stored plane.

Every comparison is np.array_equal on bytes or bit patterns; there is no tolerance in this module.  tests/test_exact_geometry.py (CPU)
proves the coverage claims from the tables below, ties the mirror's halo rule to the oracle and shows the mirror healthy on these inputs."""
import os

import numpy as np
import pytest

import depth_ref as D
import exact_conv as X
import exact_net as N
import realsr_ncnn_vulkan_amd as R
import test_gpu_exact as E
from realsr_ncnn_vulkan_amd import synth

pytestmark = pytest.mark.gpu

# ---- A: the shape set ---------------------------------------------------------------------------------------------------------------
# (h, w) of the OUTPUT plane, in five groups (one test parameter each, so that no test runs longer than a few seconds): 66 widths at
# h = 17 (a second block row of one live row: a folded pair has both strips) and 36 heights at w = 32 (exact blocks), 44 (a folded strip
# of 12) and 47 (a plain remainder of 15) -- 174 shapes.
GROUPS = {
    "w1-33": [(17, w) for w in range(1, 34)],
    "w34-66": [(17, w) for w in range(34, 67)],
    "h1-36@w32": [(h, 32) for h in range(1, 37)],
    "h1-36@w44": [(h, 44) for h in range(1, 37)],
    "h1-36@w47": [(h, 47) for h in range(1, 37)],
}
# The up-sampling class: INPUT shapes; the output plane is twice as large, so only even sizes occur -- widths 2 .. 66 at h = 18, heights
# 2 .. 36 at w = 32, 44 and 48.
UPS_GROUPS = {
    "w1-33": [(9, w) for w in range(1, 18)],
    "w34-66": [(9, w) for w in range(18, 34)],
    "h1-36@w32": [(h, 16) for h in range(1, 19)],
    "h1-36@w44": [(h, 22) for h in range(1, 19)],
    "h1-36@w47": [(h, 24) for h in range(1, 19)],
}
# name -> (cin, cout, form)
CLASSES = {
    "conv_first 3->64": (3, 64, "plain"),
    "dense 64->32": (64, 32, "lrelu"),
    "dense 160->32": (160, 32, "lrelu"),
    "conv5+rrdb 192->64": (192, 64, "res"),
    "conv5+rrdb precise 192->64": (192, 64, "precise"),
    "upconv 64->64 x2": (64, 64, "ups"),
    "conv_last 64->3": (64, 3, "plain"),
}
# (flow_flags, dbg, num_cu) of tests/test_gpu_exact.py: the default, and 4 x 64 waves with the deferred epilogue, rows below the tile
# computed, few workgroups walking many blocks.  The residual entry points have no single member with all of that: the two members
# that carry it between them are run (rows below the tile + few workgroups; 4 x 64 waves [+ few workgroups]).
CFG = ((0, 0, 256), (3, 32, 8))
RES_CFG = ((0, 0, 256), (0, 32, 8), (1, 0, 8))
PREC_CFG = ((0, 0, 256), (0, 32, 8), (1, 0, 256))
assert set(CFG) <= set(E.LAYER_COMBOS) and set(RES_CFG) <= set(E.RES_COMBOS) and set(PREC_CFG) <= set(E.PREC_COMBOS)
S = 0.2   # the network's residual scale, s1 = s2

# ---- B: the case table (w, h, tile, prepadding, tta) ----------------------------------------------------------------------------------
CASES = [
    # image smaller than / equal to / one over the halo, single rows and columns, tile larger than the image
    (1, 1, 32, 10, 0), (1, 47, 33, 10, 0), (61, 1, 35, 10, 0), (5, 3, 32, 10, 0), (10, 11, 32, 10, 0), (11, 10, 16, 10, 0),
    # (4 + 20 = 24: 48 at the 2x level, a remainder of 16 -- the even neighbour of the fold limit there)
    (4, 6, 32, 10, 0),
    # padded tile widths on both sides of a block and of the fold limit (w + 20 = 64, 65 | 46, 47 | 32, 33)
    (44, 12, 200, 10, 0), (45, 13, 200, 10, 0), (26, 30, 26, 10, 0), (27, 18, 27, 10, 0), (12, 16, 12, 10, 0), (13, 33, 13, 10, 0),
    # several tiles, last tile 1 / 2 / 7 px wide or high, interior tiles with real neighbours on four sides
    (65, 20, 32, 10, 0), (49, 17, 48, 10, 0), (33, 50, 16, 10, 0), (58, 22, 19, 10, 0), (40, 40, 13, 10, 0),
    # the margin rings of tail_margin at other crops (crop4 = 0, 4, 8, 12, 20, 28, 48)
    (37, 29, 18, 0, 0), (43, 31, 21, 1, 0), (43, 31, 21, 2, 0), (43, 31, 21, 3, 0), (43, 31, 21, 5, 0), (43, 31, 21, 7, 0), (43, 31, 21, 12, 0),
    # TTA, non-square edge tiles (transposed slots), an image smaller than the halo, other prepaddings
    (30, 26, 16, 10, 1), (23, 9, 12, 10, 1), (9, 21, 32, 3, 1), (19, 19, 8, 5, 1),
]
# also run with option "precise" = 1 against image_x4(..., precise=True): a tiny image, prepaddings 0 and 3, one tile on the fold limit
# and two multi-tile cases
PRECISE = [(5, 3, 32, 10, 0), (37, 29, 18, 0, 0), (43, 31, 21, 3, 0), (13, 33, 13, 10, 0), (65, 20, 32, 10, 0), (40, 40, 13, 10, 0)]
assert set(PRECISE) <= set(CASES) and len(set(CASES)) == len(CASES) == 29
# one process_many call at tile 16: eight sizes between 1 x 1 and 40 x 33 (w, h)
MIXED_T = 16
MIXED = [(1, 1), (40, 33), (5, 3), (17, 16), (16, 17), (33, 9), (12, 31), (26, 22)]
# D: the self-check's tiles (h, w), per model
CHECK_TILES = {1: [(20, 44), (33, 35)], 2: [(20, 44)]}
HOT_TILE = (20, 44)
# the overflow model: conv_last's |w| = 2^15, the largest power of two fp16 holds -- |acc| = 32768 |x| + b leaves fp16 where |x| reaches 2.
# The three HRconv channels conv_last reads stay below 0.23 on this tile (|acc| <= 7,472), so the two up-sampling convs and HRconv are
# four times as loud as well: HRconv stores up to 198 (finite), and 71 % of conv_last's results overflow.
HOT_GAINS = dict(last=(2.0 ** 15,), up=(4.0, 8.0))
BYTES_PER_PX = 6048       # workspace bytes per padded LR pixel in fp16 storage (Engine::bytes_per_px)


def case_id(c):
    return "%dx%d-t%d-p%d%s" % (c[0], c[1], c[2], c[3], "-tta" if c[4] else "")


def ntiles(c):
    return len(N.tile_grid(c[0], c[1], c[2]))


# ---- models and contexts, each made once -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets(tmp_path_factory):
    """key -> (depth, model, x4.param, x4.bin): the committed one- and two-block exact models and the one-block model whose conv_last
    overflows fp16; everything made inside depth(nb)."""
    made = {}
    for key, nb, gains in ((1, 1, {}), (2, 2, {}), ("hot", 1, HOT_GAINS)):
        d = str(tmp_path_factory.mktemp("geometry_%s" % key))
        with D.depth(nb):
            model = D.make_model(nb, **gains)
            pp, bp = os.path.join(d, "x4.param"), os.path.join(d, "x4.bin")
            synth.write_param(pp)
            synth.write_bin(bp, N.dense_weights(model), "fp16")
        made[key] = (nb, model, pp, bp)
    assert synth.NB == N.NB == 23
    return made


OPTIONS = (("flow_flags", 0), ("dbg", 0), ("num_cu", 256), ("precise", 0), ("trim", 1), ("fold", 1), ("merge", 16), ("merge_mixed", 1),
           ("max_workspace_mb", 65536))


def reset(s):
    s.tilesize, s.prepadding = 200, 10
    for k, v in OPTIONS:
        s.set_option(k, v)


@pytest.fixture(scope="module")
def ctxs(nets):
    """tta -> a context holding the one-block model."""
    made = {}
    for tta in (0, 1):
        made[tta] = R.RealSR(0, tta_mode=bool(tta))
        made[tta].load(*nets[1][2:])
    yield made
    for s in made.values():
        s.close()


@pytest.fixture
def ctx(ctxs):
    """Part A runs between red zones (option "test_redzone", tests/test_gpu_exact.py launch): it concerns the one-launch entry points alone."""
    for s in ctxs.values():
        reset(s)
        s.set_option("test_redzone", E.REDZONE)
    yield ctxs
    for s in ctxs.values():
        reset(s)
        s.set_option("test_redzone", 0)


_refs = {}


def ref_u8(nets, w, h, T, P, tta, precise=False):
    """The mirror's bytes (HWC) of frame_u8(w, h) on the one-block model, computed once per module and left unchanged."""
    key = (w, h, T, P, tta, precise)
    if key not in _refs:
        with D.depth(1):
            v = N.image_x4(nets[1][1], N.halfs_of_u8(N.frame_u8(w, h)), T, P=P, tta=bool(tta), precise=precise)
        _refs[key] = np.ascontiguousarray(N.to_u8(v).transpose(1, 2, 0))
        _refs[key].setflags(write=False)
    return _refs[key]


def same8(got, want):
    """np.array_equal on the bytes, with the first mismatch in the message."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, (got.shape, want.shape, got.dtype)
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return ""
    i = tuple(bad[0])
    return "%d of %d bytes differ, first at (y, x, c) = %s: got %d want %d; rows %d..%d, columns %d..%d" % (
        len(bad), got.size, i, got[i], want[i], bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max())


# ---- A: one launch, every width and height class ---------------------------------------------------------------------------------------
_operands = {}


def operands(name):
    """Weights and bias of a class, drawn once and reused for all of its shapes."""
    if name not in _operands:
        cin, cout, _ = CLASSES[name]
        rng = np.random.default_rng([2024, list(CLASSES).index(name)])
        _operands[name] = (X.grid_w(rng, (cout, cin, 3, 3)), X.grid_b(rng, cout))
    return _operands[name]


def shape_rng(name, h, w):
    """Inputs are drawn per shape, from a seed made of the class and the shape."""
    return np.random.default_rng([list(CLASSES).index(name), h, w])


def run_class(sr, name, group):
    cin, cout, form = CLASSES[name]
    wt, b = operands(name)
    for h, w in (UPS_GROUPS if form == "ups" else GROUPS)[group]:
        rng = shape_rng(name, h, w)
        x = X.grid_x(rng, (cin, h, w))
        if form in ("plain", "lrelu", "ups"):
            X.assert_exact(x, wt, b)
            want = X.epi1(X.conv_sum(x, wt, b, ups=form == "ups"), form != "plain")
            for c in E.combos(sr, CFG):
                got = E.launch(sr, sr.conv3x3, x, wt, b, lrelu=form != "plain", upsample2x=form == "ups")
                assert got.shape == want.shape, (name, h, w, c)
                msg = E.same16(got, want)
                assert not msg, (name, (h, w), c, msg)
            continue
        # the residual forms: conv5 (x rides in the accumulator as an identity tap) + the RRDB residual, s1 = s2 = 0.2
        r = X.grid_x(rng, (cout, h, w))
        X.assert_exact(x, wt, b, idt_coef=X.idt_coef(S))
        acc = X.conv_sum(x, wt, b) + X.idt_coef(S) * x[:cout].astype(np.float64)
        if form == "res":
            want = X.epi2(acc, S, r, S)
            for c in E.combos(sr, RES_CFG):
                msg = E.same16(E.launch(sr, sr.conv3x3_res, x, wt, b, S, own_input_residual=True, res=r, s2=S), want)
                assert not msg, (name, (h, w), c, msg)
        else:
            x_lo, r_lo = X.grid_lo(rng, x[:cout]), X.grid_lo(rng, r)
            want_hi, want_lo = X.epi_precise(acc, S, x_lo, r, r_lo, S)
            for c in E.combos(sr, PREC_CFG):
                hi, lo = E.launch(sr, sr.conv3x3_res_precise, x, wt, b, S, own_input_residual=True, x_lo=x_lo, res=r, res_lo=r_lo, s2=S)
                msg = E.same16(hi, want_hi)
                assert not msg, (name, (h, w), c, "hi", msg)
                bad = np.argwhere(lo != want_lo)
                assert len(bad) == 0, (name, (h, w), c, "lo: %d bytes differ, first at %s: got 0x%02x want 0x%02x" % (
                    len(bad), tuple(bad[0]), lo[tuple(bad[0])], want_lo[tuple(bad[0])]))


@pytest.mark.parametrize("group", list(GROUPS))
def test_geometry_conv_first(ctx, group):
    """3 -> 64, no activation: the three input channels share one 16-channel plane."""
    run_class(ctx[0], "conv_first 3->64", group)


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("name", ["dense 64->32", "dense 160->32"])
def test_geometry_dense(ctx, name, group):
    """LeakyReLU: the first and the widest dense conv of an RDB."""
    run_class(ctx[0], name, group)


@pytest.mark.parametrize("group", list(GROUPS))
def test_geometry_conv5_rrdb_residual(ctx, group):
    """192 -> 64 through conv3x3_res: v = fp16(fl32(0.2 acc)), then fp16(fma32(v, 0.2, r)) -- every third conv5 of the network."""
    run_class(ctx[0], "conv5+rrdb 192->64", group)


@pytest.mark.parametrize("group", list(GROUPS))
def test_geometry_conv5_rrdb_residual_precise(ctx, group):
    """The same conv on the hi + lo / 2048 stream (conv3x3_res_precise with x_lo, res and res_lo): both bytes of every element."""
    run_class(ctx[0], "conv5+rrdb precise 192->64", group)


@pytest.mark.parametrize("group", list(UPS_GROUPS))
def test_geometry_upconv(ctx, group):
    """64 -> 64 behind nearest x2, LeakyReLU.  The swept sizes are those of the OUTPUT plane, so only even ones occur: input widths 1 .. 33
    at input height 9 (output 2 .. 66 x 18) and input heights 1 .. 18 at input widths 16, 22 and 24 (output widths 32, 44 and 48)."""
    run_class(ctx[0], "upconv 64->64 x2", group)


@pytest.mark.parametrize("group", list(GROUPS))
def test_geometry_conv_last(ctx, group):
    """64 -> 3, no activation: (dy, cout) share the MFMA's M dimension."""
    run_class(ctx[0], "conv_last 64->3", group)


# ---- B: the tile loop -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_tile_loop(ctx, nets, case):
    """process() to uint8 against hwc(to_u8(image_x4)) of the one-block exact model: the default configuration, option "trim" 0 (every
    margin ring computed) and option "fold" 0 (no folded items) each against the MIRROR, not merely against each other; the PRECISE cases
    also with option "precise" 1; cases of several tiles also under a workspace budget of about two tiles, in several batches."""
    w, h, T, P, tta = case
    s = ctx[tta]
    s.tilesize, s.prepadding = T, P
    img = N.frame_u8(w, h)
    want = ref_u8(nets, w, h, T, P, tta)
    assert want.shape == (4 * h, 4 * w, 3)
    for opt in (None, "trim", "fold"):
        if opt:
            s.set_option(opt, 0)
        msg = same8(s.process(img), want)
        assert not msg, (case, "default" if opt is None else opt + " 0", msg)
        if opt:
            s.set_option(opt, 1)
    if ntiles(case) > 1:
        # two full tiles' worth of slots (a small image runs under the plan of a merged batch, whose slots have a full tile's capacity);
        # two-tile images: the smallest budget there is, which still gives every batch one tile
        cap = (T + 2 * P) ** 2 * (8 if tta else 1)
        s.set_option("max_workspace_mb", (2 * cap * BYTES_PER_PX >> 20) + 1 if ntiles(case) > 2 else 1)
        got = s.process(img)
        nb = s.get_stat("plan_batches")
        assert nb > 1, (case, nb)
        msg = same8(got, want)
        assert not msg, (case, "in %d batches" % nb, msg)
        s.set_option("max_workspace_mb", 65536)
    if case in PRECISE:
        s.set_option("precise", 1)
        msg = same8(s.process(img), ref_u8(nets, w, h, T, P, tta, precise=True))
        assert not msg, (case, "precise", msg)


def test_merged_batch_of_mixed_sizes_against_the_mirror(ctx, nets):
    """Eight images of eight sizes in ONE process_many call at tile 16: every output equals ITS OWN mirror (tests/test_gpu_merge.py ties
    merged batches to lone calls only), and a batch of images of different sizes did form (Engine::enqueue_mixed)."""
    s = ctx[0]
    s.tilesize = MIXED_T
    imgs = [N.frame_u8(w, h) for w, h in MIXED]
    want = [ref_u8(nets, w, h, MIXED_T, 10, 0) for w, h in MIXED]
    b0, m0 = s.get_stat("merged_batches"), s.get_stat("merged_mixed")
    outs = s.process_many(imgs)
    nb, nm = s.get_stat("merged_batches") - b0, s.get_stat("merged_mixed") - m0
    print("8 images of 8 sizes in %d merged batches, %d of them mixed" % (nb, nm))
    for (w, h), got, ref in zip(MIXED, outs, want):
        msg = same8(got, ref)
        assert not msg, ((w, h), msg)
    assert nb < 8 and nm >= 1


# ---- D: the self-check's device reductions, exact --------------------------------------------------------------------------------------
def bits32(v):
    return np.asarray(v, np.float32).view(np.uint32)


def q_post_store(v):
    """post_store(v * 255.f) on values that may lie far outside [0, 1] or be infinite: floor(v * 255 + 0.5), THEN the clamp to 0 .. 255.
    exact_net.to_u8 asks that the floor does not depend on whether the compiler fuses the multiply-add; for the large fp32 values of the
    overflow model it does, but both floors lie beyond the clamp, so here the two are compared behind it."""
    v = np.asarray(v, np.float32)
    two = np.clip(np.floor(v * np.float32(255) + np.float32(0.5)), 0, 255)
    one = np.clip(np.floor((v.astype(np.float64) * 255.0 + 0.5).astype(np.float32)), 0, 255)
    assert np.array_equal(one, two)
    return two.astype(np.uint8)


def mirror_report(nets, key, x, q=N.to_u8):
    """What rsr_selfcheck must report for tile x: per-conv peaks and non-finite counts of the fp16-storage walk, storage_err and the
    byte counts between that walk's output and the precise walk's (q: the uint8 conversion)."""
    nb, model = nets[key][:2]
    with D.depth(nb):
        st = {}
        with np.errstate(over="ignore"):
            acc = N.forward(model, x, stats=st)
            out16 = N.half_out(acc)
        acc_p = N.forward(model, x, precise=True)
    assert np.isfinite(acc_p).all()
    with np.errstate(invalid="ignore"):
        err = np.abs(out16 - acc_p).max()                      # fl32(half_out(acc) - acc_precise), as output_compare forms it
    dq = np.abs(q(out16).astype(int) - q(acc_p).astype(int))
    return np.array(st["conv_peak"], np.float32), np.array(st["conv_nonfinite"], np.int64), np.float32(err), int(dq.max()), int((dq > 0).sum())


def check_report(s, nets, key, x, q=N.to_u8):
    peak, bad, err, qmax, ndiff = mirror_report(nets, key, x, q)
    rep = s.selfcheck(x)
    got_peak, got_bad = s.selfcheck_ranges()
    print("model %s, tile %s: storage_err %.9e (mirror %.9e), max_byte_diff %d (%d), bytes_differ %d (%d), peak %.6g at conv %d, %d non-finite" % (
        key, x.shape[1:], rep["storage_err"], err, rep["max_byte_diff"], qmax, rep["bytes_differ"], ndiff, rep["peak_abs"], rep["peak_conv"], rep["nonfinite"]))
    assert len(got_peak) == len(peak) == 15 * nets[key][0] + 6
    assert np.array_equal(bits32(got_peak), bits32(peak)), [(i, float(a), float(b)) for i, (a, b) in enumerate(zip(got_peak, peak)) if a != b][:5]
    assert np.array_equal(got_bad, bad), (got_bad.tolist(), bad.tolist())
    assert bits32(rep["storage_err"]) == bits32(err)
    assert rep["max_byte_diff"] == qmax and rep["bytes_differ"] == ndiff
    assert bits32(rep["peak_abs"]) == bits32(peak.max()) and rep["peak_conv"] == int(peak.argmax())
    assert rep["nonfinite"] == int(bad.sum())
    return rep, peak, bad


@pytest.mark.parametrize("key,h,w", [(k, h, w) for k, ts in CHECK_TILES.items() for h, w in ts])
def test_selfcheck_report_equals_the_mirror(ctx, nets, key, h, w):
    """selfcheck(tile), then selfcheck_ranges(): every per-conv peak equals the mirror's max |stored fp16| as a float32 bit pattern, every
    non-finite count is 0, storage_err equals max |fl32(half_out(acc) - acc_precise)| bit for bit, and max_byte_diff / bytes_differ equal
    the counts to_u8 gives on the two mirror outputs.  (range_probe is otherwise held to an fp32 walk within 0.28 %.)"""
    s = ctx[0] if key == 1 else R.RealSR(0)
    try:
        if key != 1:
            s.load(*nets[key][2:])
        rep, _, bad = check_report(s, nets, key, N.tile_f16(h, w))
        assert (bad == 0).all() and rep["fp16_overflow"] == 0
    finally:
        if key != 1:
            s.close()


def test_selfcheck_overflow_equals_the_mirror(nets):
    """A one-block exact model whose conv_last has |w| = 2^15 (HOT_GAINS): only conv_last's stored output leaves fp16, and nothing reads
    it again inside the probed walk (no inf x 0 = NaN arises, which the sparse mirror could not model).  The last convolution's non-finite count equals
    the mirror's count of |acc| that round to inf, every other one is 0; its peak is the largest FINITE stored value; fp16_overflow = 1.
    The comparison of the two outputs: output_compare takes d = |fp16 value - fp32 value|, +inf at an overflowed element, and keeps it
    (d == d; only a NaN would be replaced, by +inf as well), so storage_err = +inf.  post_store(v * 255) treats +-inf as any value beyond
    the clamp -- floorf(+-inf + 0.5) = +-inf, fminf(fmaxf(., 0), 255) = 255 or 0 -- and the precise walk's finite value at such an element
    (|acc| >= 65520) clamps to the same byte: the overflowed elements add nothing to max_byte_diff / bytes_differ, and q_post_store
    (floor, then clip) gives the same bytes for +-inf."""
    s = R.RealSR(0)
    try:
        s.load(*nets["hot"][2:])
        x = N.tile_f16(*HOT_TILE)
        rep, peak, bad = check_report(s, nets, "hot", x, q_post_store)
        assert bad[-1] > 0 and (bad[:-1] == 0).all() and 0 < peak[-1] <= 65504 and bad[-1] < 3 * 16 * x[0].size
        assert rep["fp16_overflow"] == 1 and s.get_stat("selfcheck_overflow") == 1
        assert np.isposinf(rep["storage_err"]) and rep["headroom"] == 0
    finally:
        s.close()
