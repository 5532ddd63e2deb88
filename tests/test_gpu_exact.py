"""conv3x3_flow held BIT FOR BIT to a mirror of its rounding steps (run with -m gpu on the MI355X box).

The layer tests of tests/test_gpu_parity.py / test_gpu_precise.py use random normal operands, whose fp32 sums depend on the
summation order: they need a tolerance, and a tolerance lets a kernel that is wrong in a systematic way pass (round toward zero, a
LeakyReLU slope or a bias held as fp16, a product rounded to fp16 in one step instead of through fp32).  Here the operands are chosen
so that every partial sum is exact in fp32 in any order (tests/exact_conv.py): what is left are the epilogues' roundings, which the
mirror restates, and every output is compared with np.array_equal.

The entry points behind these tests size their buffers exactly and used to pre-set the output to 0: a store past the last plane was
invisible, a read just past a plane met the next plane's zero guard, and a store never made left a legal 0.  The module's context
therefore runs them between red zones (option "test_redzone"), and every launch goes through launch() below."""
import os

import numpy as np
import pytest

import exact_conv as X
import realsr_ncnn_vulkan_amd as R

pytestmark = pytest.mark.gpu

# (flow_flags, dbg, num_cu): 8 x 32 / 4 x 64 MFMA waves, inline / deferred epilogue, weights resident / streamed (4), rows below the
# tile skipped / computed (dbg 32), one workgroup per CU / few workgroups walking many blocks (num_cu 8)
LAYER_COMBOS = ((0, 0, 256), (3, 0, 256), (4, 0, 8), (7, 0, 256), (0, 32, 8), (3, 32, 8), (1, 0, 8))
RES_COMBOS = ((0, 0, 256), (1, 0, 256), (0, 0, 8), (1, 0, 8), (0, 32, 8), (4, 0, 8), (5, 0, 256))
PREC_COMBOS = ((0, 0, 256), (0, 0, 8), (0, 32, 8), (4, 0, 8), (1, 0, 256))


REDZONE = 4096   # bytes; the widest swept plane row is 66 px x 32 B = 2112 B, and one store instruction moves 1 KiB


@pytest.fixture(scope="module")
def sr(model_dir):
    """The one-launch entry points run between red zones (option "test_redzone"): input, residual and output buffers lie between 4 KiB
    of NaN and the output starts as NaN, not 0 -- a store that is never made is a certain mismatch, and launch() looks at the zones."""
    s = R.RealSR(0)
    s.load(os.path.join(model_dir, "x4.param"), os.path.join(model_dir, "x4.bin"))
    s.set_option("test_redzone", REDZONE)
    yield s
    s.set_option("test_redzone", 0)
    s.close()


def launch(sr, fn, *args, **kw):
    """sr.conv3x3 / conv3x3_res / conv3x3_res_precise, and no byte of the red zones around its buffers changed."""
    got = fn(*args, **kw)
    assert sr.get_stat("test_redzone") == REDZONE
    dirty = sr.get_stat("test_redzone_dirty")
    assert dirty == 0, "%d red-zone bytes changed: a store outside the buffers" % dirty
    return got


def combos(sr, cs):
    try:
        for flags, dbg, ncu in cs:
            for k, v in (("flow_flags", flags), ("dbg", dbg), ("num_cu", ncu)):
                sr.set_option(k, v)
            yield flags, dbg, ncu
    finally:
        for k, v in (("flow_flags", 0), ("dbg", 0), ("num_cu", 256)):
            sr.set_option(k, v)


def same16(got, want):
    """np.array_equal on the fp16 bit patterns, with the first mismatch in the message."""
    g, w = got.view(np.uint16), want.view(np.uint16)
    if np.array_equal(g, w):
        return ""
    bad = np.argwhere(g != w)
    i = tuple(bad[0])
    return "%d of %d values differ, first at %s: got %r (0x%04x) want %r (0x%04x)" % (
        len(bad), g.size, i, float(got[i]), int(g[i]), float(want[i]), int(w[i]))


# ---- a hardware fact the mirror relies on --------------------------------------------------------------------
def test_accumulator_and_fp16_conversion_round_to_nearest_even(sr):
    """Off the exact grid on purpose: one product p = x*w far below an ulp of the bias, b + p inexact in fp32.  b = 1 + 2^-11 is an fp16
    midpoint, so the fp16 output shows how fl32(b + p) rounded: to nearest even (mirror), toward zero, or not at all (a wider
    accumulator).  The product meets the bias inside the bias's own MFMA (tap (0, 0) of the first step) and in a later one (centre tap)."""
    cin, cout, h, w = 32, 32, 8, 40
    u = 2.0 ** -23                                   # ulp of fp32 at 1
    t = 1.0 + 2.0 ** -11                             # an fp16 tie, exact in fp32
    # (bias, product): per output channel; products = 2^-12 * w, w an fp16-normal weight
    table = [(t, 0.75 * u), (t, 0.25 * u), (t, 0.5 * u), (t, -0.25 * u), (-t, -0.75 * u), (-t, -0.25 * u),
             (t + u, -0.5 * u), (t + u, 0.5 * u), (2.0 - 2.0 ** -11, 0.75 * u), (0.5 + 2.0 ** -12, 0.375 * u)]
    xv = 2.0 ** -12
    x = np.zeros((cin, h, w), np.float16)
    x[0, 3, 3] = xv                                  # centre tap of output (3, 3)
    x[1, 3, 20] = xv                                 # tap (0, 0) of output (4, 21)
    wt = np.zeros((cout, cin, 3, 3), np.float32)
    b = np.full(cout, 0.5, np.float32)
    for o, (bb, p) in enumerate(table):
        wv = p / xv
        assert float(np.float16(wv)) == wv and abs(wv) >= 2.0 ** -14
        wt[o, 0, 1, 1] = wt[o, 1, 0, 0] = wv
        b[o] = bb
    exact = b.astype(np.float64)[:, None, None] + np.zeros((h, w))
    for o, (bb, p) in enumerate(table):
        exact[o, 3, 3] += p
        exact[o, 4, 21] += p
    want = exact.astype(np.float32).astype(np.float16)                       # fl32 to nearest even, then fp16 to nearest even
    rtz = np.where(np.abs(exact.astype(np.float32)) > np.abs(exact), np.nextafter(exact.astype(np.float32), np.float32(0)),
                   exact.astype(np.float32)).astype(np.float16)
    wide = exact.astype(np.float16)                                           # one rounding from the exact sum
    assert not np.array_equal(want.view(np.uint16), rtz.view(np.uint16)) and not np.array_equal(want.view(np.uint16), wide.view(np.uint16))
    for c in combos(sr, LAYER_COMBOS[:2]):
        got = launch(sr, sr.conv3x3, x, wt, b)
        msg = same16(got, want)
        if msg:
            msg += " | equals round-toward-zero: %s, equals a single rounding of the exact sum: %s" % (
                np.array_equal(got.view(np.uint16), rtz.view(np.uint16)), np.array_equal(got.view(np.uint16), wide.view(np.uint16)))
        assert not msg, (c, msg)


def test_fp16_subnormals_are_kept_on_both_sides(sr):
    """The whole-network mirror (tests/exact_net.py) stores a few thousand fp16 SUBNORMAL activations per tile and keeps them, as numpy
    does.  Here: fp16-subnormal inputs (and the smallest normal ones) times weights 1.0 / 2.0 / 0.5, one tap per output channel, plus a
    bias far below fp16's subnormal spacing -- every accumulator is exact in fp32, and its fp16 result is subnormal or just above, with
    and without LeakyReLU.  A kernel that flushed subnormal MFMA inputs, or whose fp32 -> fp16 conversion flushed subnormal results, would
    differ from numpy; the message says which."""
    cin, cout, h, w = 32, 32, 9, 40
    rng = np.random.default_rng(2411)
    k = rng.integers(1, 1024, (cin, h, w))                                     # subnormals: k * 2^-24
    k = np.where(rng.integers(0, 3, (cin, h, w)) == 0, (1024 + k) << rng.integers(0, 3, (cin, h, w)), k)   # a third: [2^-14, 2^-11)
    x = (np.where(rng.integers(0, 2, k.shape) == 1, -k, k) * 2.0 ** -24).astype(np.float16)
    assert (np.abs(x.astype(np.float64)) < X.F16_MIN_NORMAL).mean() > 0.5 and (x != 0).all()
    wt = np.zeros((cout, cin, 3, 3), np.float32)
    for o in range(cout):
        wt[o, (o * 7) % cin, o % 3, (o // 3) % 3] = (1.0, 2.0, 0.5)[o % 3] * (-1.0 if o & 4 else 1.0)
    m = rng.integers(0, 64, cout) * 2 + 1
    b = (np.where(rng.integers(0, 2, cout) == 1, -m, m) * 2.0 ** -27).astype(np.float32)   # odd multiples of 2^-27, |b| < 2^-20
    acc = X.conv_sum(x, wt, b)                                                  # (asserts that the sums are exact in fp32)
    flushed_in = X.conv_sum(np.where(np.abs(x.astype(np.float64)) < X.F16_MIN_NORMAL, 0, x).astype(np.float16), wt, b)
    for lrelu in (False, True):
        want = X.epi1(acc, lrelu)
        sub = (np.abs(want.astype(np.float64)) < X.F16_MIN_NORMAL) & (want != 0)
        assert sub.mean() > 0.3                                                 # subnormal results, and normal ones next to them
        flushed_out = np.where(sub, np.float16(0) * want, want).astype(np.float16)
        for c in combos(sr, LAYER_COMBOS[:2]):
            got = launch(sr, sr.conv3x3, x, wt, b, lrelu=lrelu)
            msg = same16(got, want)
            if msg:
                msg += " | equals subnormal inputs flushed: %s, subnormal results flushed (ignoring the sign of zero): %s" % (
                    np.array_equal(got.view(np.uint16), X.epi1(flushed_in, lrelu).view(np.uint16)), np.array_equal(got, flushed_out))
            assert not msg, (c, lrelu, msg)


# ---- EPI 1 (conv + bias [+ LeakyReLU] -> fp16), every conv shape of the network ------------------------------------
SHAPES = [(64, 32, 20, 40, False), (96, 32, 17, 33, False), (128, 32, 16, 32, False), (160, 32, 33, 65, False), (192, 64, 16, 32, False),
          (3, 64, 9, 70, False), (64, 3, 33, 31, False), (64, 64, 10, 21, True), (64, 64, 1, 1, False),
          (32, 32, 12, 40, False), (3, 32, 9, 70, False)]  # (one 32-channel input pair: fewer half-stages than the deferred epilogue's body)
# production planes: 220 x 220 (a C2 tile), 140 wide (the folded last column of C2's 1920-wide row: 140 = 4 x 32 + 12), the x2 / x4
# levels behind the up-samplings and conv_last's 440 x 440
PROD = [(64, 32, 220, 220, False), (160, 32, 220, 220, False), (192, 64, 220, 220, False), (64, 32, 100, 140, False),
        (160, 32, 100, 140, False), (192, 64, 100, 140, False), (3, 64, 220, 220, False), (64, 64, 220, 220, True),
        (64, 3, 440, 440, False)]


def _layer(sr, cin, cout, h, w, ups, lrelu, cs, seed):
    rng = np.random.default_rng(seed)
    x, wt, b = X.grid_x(rng, (cin, h, w)), X.grid_w(rng, (cout, cin, 3, 3)), X.grid_b(rng, cout)
    X.assert_exact(x, wt, b)
    want = X.epi1(X.conv_sum(x, wt, b, ups=ups), lrelu)
    for c in combos(sr, cs):
        got = launch(sr, sr.conv3x3, x, wt, b, lrelu=lrelu, upsample2x=ups)
        assert got.shape == want.shape
        msg = same16(got, want)
        assert not msg, (c, msg)


@pytest.mark.parametrize("cin,cout,h,w,ups", SHAPES)
@pytest.mark.parametrize("lrelu", [False, True])
def test_exact_layer(sr, cin, cout, h, w, ups, lrelu):
    _layer(sr, cin, cout, h, w, ups, lrelu, LAYER_COMBOS, cin * 1000 + cout + h + lrelu)


@pytest.mark.parametrize("cin,cout,h,w,ups", PROD)
def test_exact_layer_production_planes(sr, cin, cout, h, w, ups):
    _layer(sr, cin, cout, h, w, ups, cout != 3, LAYER_COMBOS[:3] + LAYER_COMBOS[4:5], cin + 7 * cout + h)


# ---- impulses: tap orientation, halo, zero padding, block / strip seams --------------------------------------------
def _seams(h, w):
    """Positions on every seam that matters: plane corners and edges, the 32-column / 16-row block borders, both strips of a folded last
    column (w % 32 in 1..14: rows 0..15 / 16..31 of a block-row pair) and the last 4-row group of the tile."""
    pos = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h // 2, 0), (h - 1, w // 3), (h // 3, w - 1)]
    for bx in range(32, w, 32):
        for by in range(16, h, 16):
            pos += [(by - 1, bx - 1), (by, bx), (by - 1, bx), (by, bx - 1)]
        pos += [(0, bx), (h - 1, bx - 1)]
    if w % 32:
        fx = w - w % 32
        pos += [(5, fx + (w % 32) // 2), (min(20, h - 1), w - 1), (min(31, h - 1), fx), (min(15, h - 1), w - 1), (min(16, h - 1), fx)]
    g = (h - 1) // 4 * 4                       # first row of the last 4-row group
    pos += [(g, 2), (min(g + 3, h - 1), w // 2 + 1), (max(g - 1, 0), w - 3)]
    return sorted(set((min(y, h - 1), min(x, w - 1)) for y, x in pos))


@pytest.mark.parametrize("cin,cout,h,w", [(64, 32, 37, 44), (192, 64, 37, 44), (160, 32, 100, 140), (3, 64, 53, 70), (64, 3, 37, 44)])
def test_impulse_responses(sr, cin, cout, h, w):
    """One-hot inputs of 1.0: the output is act(b) everywhere but the 3 x 3 footprint of each impulse, where it is act(b + w[:, c, 1 - oy,
    1 - ox]) -- no reference arithmetic at all.  The channel of each impulse walks all 16-channel planes."""
    rng = np.random.default_rng(cin * 31 + w)
    wt, b = X.grid_w(rng, (cout, cin, 3, 3)), X.grid_b(rng, cout)
    lrelu = cout != 3
    groups = X.impulse_sets(h, w, _seams(h, w))
    assert sum(len(g) for g in groups) >= 12
    k = 0
    for g in groups:
        hits = []
        for y, x in g:
            hits.append(((k * 37) % cin, y, x))
            k += 1
        xin = X.impulse_input(cin, h, w, hits)
        want = X.epi1(X.impulse_sum(wt, b, h, w, hits), lrelu)
        for c in combos(sr, LAYER_COMBOS[:2] + LAYER_COMBOS[4:6]):
            msg = same16(launch(sr, sr.conv3x3, xin, wt, b, lrelu=lrelu), want)
            assert not msg, (c, hits, msg)


# ---- EPI 2: the residual forms ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,h,w", [(192, 20, 40), (64, 33, 50), (192, 70, 90), (192, 100, 140)])
def test_exact_residual_epilogues(sr, cin, h, w):
    """RDB conv5 v = fp16(fl32(s1 * (conv + b + x * fp16(1/s1)))) (x rides in the accumulator as an identity tap), every third RDB
    v = fp16(fma32(v, s2, r)), trunk_conv v = fp16(fma32(fp16(conv + b), 1, r)) -- at power-of-two scales (only the fp16 stores round)
    and at the network's 0.2 (the fp32 product rounds first)."""
    cout = 64
    rng = np.random.default_rng(cin + h + 5)
    x, wt, b, r = X.grid_x(rng, (cin, h, w)), X.grid_w(rng, (cout, cin, 3, 3)), X.grid_b(rng, cout), X.grid_x(rng, (cout, h, w))
    acc = X.conv_sum(x, wt, b)
    x0 = x[:cout].astype(np.float64)
    forms = {}
    for s1, s2 in ((0.25, 0.5), (0.5, 0.25), (0.2, 0.2)):
        X.assert_exact(x, wt, b, idt_coef=X.idt_coef(s1))
        a = acc + X.idt_coef(s1) * x0
        forms["conv5 s1=%g" % s1] = ((s1, True, None, 1.0), X.epi2(a, s1))
        forms["conv5+rrdb s1=%g s2=%g" % (s1, s2)] = ((s1, True, r, s2), X.epi2(a, s1, r, s2))
    X.assert_exact(x, wt, b)
    forms["trunk"] = ((1.0, False, r, 1.0), X.epi2(acc, 1.0, r, 1.0))
    cs = RES_COMBOS if h * w < 10000 else RES_COMBOS[:2] + RES_COMBOS[4:5]
    for c in combos(sr, cs):
        for name, ((s1, own, rr, s2), want) in forms.items():
            msg = same16(launch(sr, sr.conv3x3_res, x, wt, b, s1, own_input_residual=own, res=rr, s2=s2), want)
            assert not msg, (name, c, msg)


# ---- EPI 4 / 5: the precise residual stream, hi and lo bytes --------------------------------------------------------
@pytest.mark.parametrize("cin,h,w", [(192, 20, 40), (64, 33, 50), (192, 70, 90), (3, 9, 70), (192, 100, 140)])
def test_exact_precise_epilogues(sr, cin, h, w):
    """v = fl32(fl32(s1 * acc) + lo1/2048) [; v = fl32(fma32(v, s2, r_hi) + r_lo/2048)], hi = fp16(v), lo = bf8 RNE of (v - hi) * 2048:
    both bytes of every element against the mirror."""
    cout = 64
    rng = np.random.default_rng(cin * 3 + h)
    xx = X.grid_x(rng, (max(cin, cout), h, w))
    x, x_lo = xx[:cin], X.grid_lo(rng, xx[:cout])
    wt, b = X.grid_w(rng, (cout, cin, 3, 3)), X.grid_b(rng, cout)
    r_hi = X.grid_x(rng, (cout, h, w))
    r_lo = X.grid_lo(rng, r_hi)
    acc = X.conv_sum(x, wt, b)
    forms = {"trunk": ((1.0, False, None, r_hi, r_lo, 1.0), X.epi_precise(acc, 1.0, None, r_hi, r_lo)),
             "trunk, no lo": ((1.0, False, None, r_hi, None, 1.0), X.epi_precise(acc, 1.0, None, r_hi, None))}
    if cin == 3:
        forms["conv_first"] = ((1.0, False, None, None, None, 1.0), X.epi_precise(acc, 1.0))
    if cin >= cout:
        for s1, s2 in ((0.25, 0.5), (0.2, 0.2)):
            X.assert_exact(x, wt, b, idt_coef=X.idt_coef(s1))
            a = acc + X.idt_coef(s1) * xx[:cout].astype(np.float64)
            forms["conv5 s1=%g" % s1] = ((s1, True, x_lo, None, None, 1.0), X.epi_precise(a, s1, x_lo))
            forms["conv5, no lo s1=%g" % s1] = ((s1, True, None, None, None, 1.0), X.epi_precise(a, s1))
            forms["conv5+rrdb s1=%g" % s1] = ((s1, True, x_lo, r_hi, r_lo, s2), X.epi_precise(a, s1, x_lo, r_hi, r_lo, s2))
    cs = PREC_COMBOS if h * w < 10000 else PREC_COMBOS[:1] + PREC_COMBOS[2:3]
    for c in combos(sr, cs):
        for name, ((s1, own, xl, rh, rl, s2), (want_hi, want_lo)) in forms.items():
            hi, lo = launch(sr, sr.conv3x3_res_precise, x, wt, b, s1, own_input_residual=own, x_lo=xl, res=rh, res_lo=rl, s2=s2)
            msg = same16(hi, want_hi)
            assert not msg, (name, c, "hi", msg)
            bad = np.argwhere(lo != want_lo)
            assert len(bad) == 0, (name, c, "lo: %d bytes differ, first at %s: got 0x%02x want 0x%02x" % (
                len(bad), tuple(bad[0]), lo[tuple(bad[0])], want_lo[tuple(bad[0])]))
