"""64-bit image addressing on the GPU (run with -m gpu): every entry point that takes an rsr_image, on surfaces whose rows and planes lie
beyond 2^31 and 2^32 bytes from their data pointer (tests/far_layout.py: layouts R, Pn and M, and the arena).

ONE assertion throughout: a call on far surfaces writes, into its window, the very bytes the same context writes for the same pixels on
tightly packed tensors -- np.array_equal on raw bytes -- and nothing else: once the windows are refilled with 0xCD, every byte of the
output arena and of the input arena holds 0xCD again (far_layout.scan).  No tolerance appears anywhere.  The packed calls are tied to
the exact references by the other GPU modules; here only the addressing differs.  That these comparisons fail for an offset narrowed
to 32 bits is shown on the CPU (tests/test_far_layout.py), and every such offset stays inside the arenas.

The two arenas are module-scoped (13.1 GiB together) and freed at teardown; with less than that + 4 GiB of free device memory the module
skips, naming both figures."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

import far_layout as fl
import sequence_ref
import tile_diff_ref as ref
from far_layout import F16, F32, H, NV12, P010, T, U8, W, P
from gpu_support import DIFF_FORMATS, ROUTE_IDS, ROUTES, context_fixtures, dev, out_dims, paths  # noqa: F401
from pixfmt_ref import paste, sentinel_bytes as sentinel

pytestmark = pytest.mark.gpu
NP = fl.NP
NT = 4  # 2 x 2 tiles


ctxs, ctx = context_fixtures(T, P)


class Arenas:
    def __init__(self):
        self.inp, self.out = fl.new_arena(), fl.new_arena()


@pytest.fixture(scope="module")
def A():
    """The input arena and the output arena of the module."""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    why = fl.memory_skip_reason(free)
    if why:
        pytest.skip(why)
    torch.cuda.reset_peak_memory_stats()
    a = Arenas()
    assert a.inp.numel() == a.out.numel() == fl.arena_bytes()
    torch.cuda.synchronize()
    yield a
    peak = torch.cuda.max_memory_allocated()
    a.inp = a.out = None
    torch.cuda.empty_cache()
    print("\nfar addressing: peak device memory of the module %.2f GiB (two arenas of %.2f GiB; cap %.0f GiB)"
          % (peak / fl.GIB, fl.arena_bytes() / fl.GIB, fl.CAP / fl.GIB))
    assert peak <= fl.CAP


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def filled_bytes(n):
    return torch.full((n,), fl.FILL, dtype=torch.uint8, device="cuda")


def noise(seed, fmt, shape):
    """A numpy image of the format of random BYTES: a previous output no network produces."""
    n = int(np.prod(shape)) * np.dtype(NP[fmt]).itemsize
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).view(NP[fmt]).reshape(shape)


def kind_of(fmt, kind):
    """A uint8 HWC image has no planes: beside a Pn surface it lies in layout R."""
    return "R" if fmt == U8 and kind == "Pn" else kind


def windows(kind, fmt, w, h, c=3, odd=False, n=1):
    return fl.group(kind_of(fmt, kind), fmt, w, h, c, odd and fmt == U8, n=n)


def packed_batch(s, xs, in_fmt, out_fmt, c=3, w=W, h=H):
    """The reference: the batch call on tightly packed tensors, as the packed numpy outputs."""
    ow, oh = out_dims(s, w, h)
    d_in = [dev(x) for x in xs]
    d_out = [filled_bytes(R.image_bytes(out_fmt, ow, oh, c)) for _ in xs]
    torch.cuda.synchronize()
    s.process_device_batch([t.data_ptr() for t in d_in], in_fmt, w, h, c, [t.data_ptr() for t in d_out], out_fmt)
    torch.cuda.synchronize()
    outs = [t.cpu().numpy().view(NP[out_fmt]).reshape(fl.shape_of(out_fmt, ow, oh, c)) for t in d_out]
    for o in outs:
        assert not np.array_equal(fl.raw(o), fl.raw(sentinel(out_fmt, o.shape)))
    return outs


def clean(A, in_wins, out_wins):
    """Refill the windows, then scan both arenas: (first changed byte of the input arena, of the output arena), None = untouched.  An
    arena found changed is filled anew, so that the next test starts clean."""
    found = []
    for arena, wins in ((A.inp, in_wins), (A.out, out_wins)):
        for wn in wins:
            fl.refill(arena, wn)
        bad = fl.scan(arena)
        if bad is not None:
            arena.fill_(fl.FILL)
        found.append(bad)
    torch.cuda.synchronize()
    return tuple(found)


def far_run(A, in_wins, xs, out_wins, wants, call, before=None):
    """xs into the input windows (and `before`, where given, into the output windows), call(), and the one assertion: the output windows
    hold `wants`, the input windows still hold xs, and with the windows refilled both arenas are untouched."""
    got = ins = None
    try:
        for wn, x in zip(in_wins, xs):
            fl.put(A.inp, wn, x)
        for wn, x in zip(out_wins, before or []):
            if x is not None:
                fl.put(A.out, wn, x)
        torch.cuda.synchronize()
        call()
        torch.cuda.synchronize()
        got = [fl.get(A.out, wn) for wn in out_wins]
        ins = [fl.get(A.inp, wn) for wn in in_wins]
    finally:
        bad_in, bad_out = clean(A, in_wins, out_wins)
    for i, (g, want) in enumerate(zip(got, wants)):
        assert np.array_equal(g, fl.raw(want)), ("output window", i, out_wins[i])
    for i, (g, x) in enumerate(zip(ins, xs)):
        assert np.array_equal(g, fl.raw(x)), ("input window", i, in_wins[i])
    assert bad_out is None, "the output arena was written outside the windows, first at byte %d from the image base" % (bad_out - fl.BASE)
    assert bad_in is None, "the input arena was written, first at byte %d from the image base" % (bad_in - fl.BASE)


def batch_case(A, s, kind, in_fmt, out_fmt, c=3, odd=False, n=1, seed=100):
    """n images through rsr_process_device_batch: far on both sides against packed on both sides, at the options in force."""
    ow, oh = out_dims(s, W, H)
    xs = [fl.image(seed + i, in_fmt, W, H, c) for i in range(n)]
    wants = packed_batch(s, xs, in_fmt, out_fmt, c)
    iw, ows = windows(kind, in_fmt, W, H, c, odd, n), windows(kind, out_fmt, ow, oh, c, odd, n)
    far_run(A, iw, xs, ows, wants,
            lambda: s.process_device_batch([wn.desc(A.inp) for wn in iw], in_fmt, W, H, c, [wn.desc(A.out) for wn in ows], out_fmt))


# ---- the instruments themselves -----------------------------------------------------------------------------------------------------------
def test_scan_finds_one_changed_byte_anywhere(A):
    n = A.out.numel()
    assert fl.scan(A.out) is None and fl.scan(A.inp) is None
    for at in (0, 5, fl.SCAN_CHUNK - 1, fl.SCAN_CHUNK, fl.BASE - 1, fl.BASE + fl.B32 + 3, n - 9, n - 1):
        A.out[at] = 0xCC
        found = fl.scan(A.out)
        A.out[at] = fl.FILL
        assert found == at
    assert fl.scan(A.out) is None


@pytest.mark.parametrize("fmt,kind", [(U8, "R"), (F32, "R"), (F32, "Pn"), (P010, "R"), (P010, "Pn"), (U8, "M"), (F16, "M")],
                         ids=["u8-R", "f32-R", "f32-Pn", "p010-R", "p010-Pn", "u8-M", "f16-M"])
def test_views_address_the_stated_bytes(A, fmt, kind):
    """put() and get() go through as_strided views; the library goes through the descriptor.  Every row of an image put into a window
    is found, by a plain slice of the arena, at base + column + plane * plane_pitch + row * row_pitch -- beyond 2^32 too."""
    w, h = fl.m_size(fmt) if kind == "M" else (4 * W, 4 * H)
    wn = fl.group(kind, fmt, w, h)[3]
    x = noise(90, fmt, fl.shape_of(fmt, w, h))
    rows = fl.raw(x).reshape(-1, wn.rowbytes)
    try:
        fl.put(A.out, wn, x)
        assert wn.desc(A.out) == fl.view(A.out, (wn.row_pitch, wn.plane_pitch), fmt, w, h, 3, wn.col)[0]
        assert wn.desc(A.out)[0] == A.out.data_ptr() + fl.BASE + wn.col
        starts = wn.row_starts()
        assert len(starts) == len(rows) and max(o for _, _, o in starts) + wn.rowbytes > fl.B32  # (layout M: the last row ends beyond 2^32)
        picked = [0, len(rows) - 1] + [i for i, (_, _, o) in enumerate(starts) if o < fl.B32 <= o + wn.row_pitch or o < fl.B31 <= o + wn.row_pitch]
        for i in picked:
            at = fl.BASE + wn.col + starts[i][2]
            assert np.array_equal(A.out[at:at + wn.rowbytes].cpu().numpy(), rows[i]), starts[i]
        assert np.array_equal(fl.get(A.out, wn), fl.raw(x))
    finally:
        _, bad = clean(A, [], [wn])
    assert bad is None


# ---- (a) rsr_process_device_batch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("odd", [False, True], ids=["pitch0mod4", "pitch1mod4"])
@pytest.mark.parametrize("tta,dbg", ROUTES, ids=ROUTE_IDS)
def test_u8c3_routes(ctx, A, tta, dbg, odd):
    s = ctx[tta]
    s.set_option("dbg", dbg)
    batch_case(A, s, "R", U8, U8, odd=odd)


@pytest.mark.parametrize("odd", [False, True], ids=["pitch0mod4", "pitch1mod4"])
@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_u8c4_alpha_reads(ctx, A, tta, odd):
    batch_case(A, ctx[tta], "R", U8, U8, c=4, odd=odd, seed=110)


@pytest.mark.parametrize("kind", ["R", "Pn"])
@pytest.mark.parametrize("tta,dbg", [(False, 0), (False, 8192), (True, 0)], ids=["fused", "unfused", "tta"])
@pytest.mark.parametrize("pair", [(F16, F32), (F32, F16)], ids=["f16-f32", "f32-f16"])
def test_planar_routes(ctx, A, pair, tta, dbg, kind):
    s = ctx[tta]
    s.set_option("dbg", dbg)
    batch_case(A, s, kind, *pair, seed=120)


@pytest.mark.parametrize("option", ["bgr", "precise"])
@pytest.mark.parametrize("kind,pair", [("R", (U8, U8)), ("R", (F16, F32)), ("Pn", (F32, F16))], ids=["u8-R", "f16-f32-R", "f32-f16-Pn"])
def test_bgr_and_precise(ctx, A, kind, pair, option):
    s = ctx[False]
    s.set_option(option, 1)
    batch_case(A, s, kind, *pair, seed=130)


@pytest.mark.parametrize("kind,pair,odd", [("R", (U8, U8), True), ("R", (F16, F32), False), ("Pn", (F32, F16), False), ("R", (NV12, NV12), False),
                                            ("Pn", (P010, P010), False)], ids=["u8-R", "f16-f32-R", "f32-f16-Pn", "nv12-R", "p010-Pn"])
def test_merged_batch_of_three(ctx, A, kind, pair, odd):
    """Three images, each in its own window of the shared arenas, in ONE tile batch: the pitches and plane offsets of images 1 and 2."""
    s = ctx[False]
    g0 = s.get_stat("batch_groups")
    batch_case(A, s, kind, *pair, odd=odd, n=3, seed=140)
    assert s.get_stat("batch_groups") == g0 + 2  # the packed call and the far one: one tile batch each


@pytest.mark.parametrize("kind", ["R", "Pn"])
@pytest.mark.parametrize("siting", [0, 1, 2])
@pytest.mark.parametrize("fmt", [NV12, P010], ids=["nv12", "p010"])
def test_yuv_surfaces(ctx, A, fmt, siting, kind):
    s = ctx[False]
    s.set_option("yuv_siting", siting)
    batch_case(A, s, kind, fmt, fmt, seed=150)


@pytest.mark.parametrize("kind", ["R", "Pn"])
@pytest.mark.parametrize("pair", [(U8, NV12), (NV12, F16)], ids=["u8-nv12", "nv12-f16"])
def test_yuv_on_one_side(ctx, A, pair, kind):
    batch_case(A, ctx[False], kind, *pair, seed=160)


REDUCED = ([(Fraction(r), fmt, 0, k) for r in (2, 1) for fmt, k in ((U8, "R"), (F32, "R"), (F32, "Pn"), (NV12, "R"), (NV12, "Pn"))] +
           [(Fraction(3, 2), fmt, st, k) for fmt, st, k in ((U8, 0, "R"), (F16, 0, "R"), (F16, 0, "Pn"), (NV12, 0, "R"), (NV12, 2, "Pn"), (P010, 0, "Pn"),
                                                           (P010, 2, "R"))])


@pytest.mark.parametrize("ratio,fmt,siting,kind", REDUCED, ids=["x%s-f%d-s%d-%s" % (str(r).replace("/", "_"), f, st, k) for r, f, st, k in REDUCED])
def test_reduced_outputs(ctx, A, ratio, fmt, siting, kind):
    s = ctx[False]
    s.set_option("yuv_siting", siting)
    s.out_ratio = ratio
    assert out_dims(s, W, H) in fl.SIZES
    batch_case(A, s, kind, fmt, fmt, odd=(ratio == 1), seed=170)


@pytest.mark.parametrize("ratio,fmt,kind", [(Fraction(2), U8, "R"), (Fraction(3, 2), F32, "Pn")], ids=["box-u8-R", "area-f32-Pn"])
def test_reduced_outputs_under_tta(ctx, A, ratio, fmt, kind):
    s = ctx[True]
    s.out_ratio = ratio
    batch_case(A, s, kind, fmt, fmt, seed=180)


# ---- (b) rsr_process_device_masked --------------------------------------------------------------------------------------------------------
FAR3 = [(U8, "R"), (F32, "R"), (F32, "Pn"), (NV12, "R"), (NV12, "Pn")]
FAR3_IDS = ["u8-R", "f32-R", "f32-Pn", "nv12-R", "nv12-Pn"]


@pytest.mark.parametrize("fmt,kind", FAR3, ids=FAR3_IDS)
def test_masked_tiles_1_and_2(ctx, A, fmt, kind):
    """Tiles 1 and 2 of the 2 x 2 grid: their output rectangles equal the packed plain call's, and the other two -- whose rows lie on both
    sides of 2^31 and 2^32 as well -- still hold 0xCD, like everything around the window."""
    s = ctx[False]
    mask = [0, 1, 1, 0]
    x = fl.image(200, fmt)
    plain = packed_batch(s, [x], fmt, fmt)[0]
    want = sentinel(fmt, plain.shape)
    for t in (1, 2):
        paste(fmt, want, plain, ref.out_rect(W, H, T, t))
    assert not np.array_equal(fl.raw(want), fl.raw(plain))
    iw, ow = windows(kind, fmt, W, H), windows(kind, fmt, 4 * W, 4 * H)
    far_run(A, iw, [x], ow, [want], lambda: s.process_device_masked(iw[0].desc(A.inp), fmt, W, H, 3, ow[0].desc(A.out), fmt, mask))


# ---- (c) rsr_process_device_sequence ------------------------------------------------------------------------------------------------------
SEQ_MASKS = [[1, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]]


def test_the_sequence_masks_copy_far_rows_at_every_alignment():
    """The condition on the inputs of the test below: the rectangles of tiles 2 and 3 -- output rows 128 .. 175, row 170
    the first beyond 2^32 -- are copied previous output -> frame 0 (windows co-aligned to 16 bytes), frame 0 or the previous output ->
    frame 1 (agreeing modulo 4 only) and frame 1 -> frame 2 (modulo the element size only)."""
    src = sequence_ref.sources(np.array(SEQ_MASKS), True)
    assert src.tolist() == [[0, 0, -1, -1], [0, 0, 1, -1], [0, 0, 1, -1]]
    assert ref.out_rect(W, H, T, 2)[1] == 128 < 170 < ref.out_rect(W, H, T, 2)[3] == 176 and fl.far_row_pitch(U8, 176) * 170 >= fl.B32


@pytest.mark.parametrize("fmt,kind", FAR3, ids=FAR3_IDS)
def test_sequence_of_three_frames_and_a_previous_output(ctx, A, fmt, kind):
    """Three frames and the previous output, all in far windows: previous output in window 0 of the output arena, the frames' outputs in
    windows 1 .. 3.  Every rectangle comes from the packed result of the frame tests/sequence_ref.py names, or from the previous output."""
    s = ctx[False]
    xs = [fl.image(210 + k, fmt) for k in range(3)]
    plains = packed_batch(s, xs, fmt, fmt)
    prev = noise(219, fmt, plains[0].shape)
    src = sequence_ref.sources(np.array(SEQ_MASKS), True)
    wants = []
    for k in range(3):
        e = sentinel(fmt, prev.shape)
        for t in range(NT):
            paste(fmt, e, prev if src[k, t] < 0 else plains[src[k, t]], ref.out_rect(W, H, T, t))
        wants.append(e)
    iw, ow = windows(kind, fmt, W, H, n=3), windows(kind, fmt, 4 * W, 4 * H, n=4)
    far_run(A, iw, xs, ow, [prev] + wants,
            lambda: s.process_device_sequence([wn.desc(A.inp) for wn in iw], fmt, W, H, 3, [wn.desc(A.out) for wn in ow[1:]], fmt,
                                              np.array(SEQ_MASKS, dtype=np.uint8), prev_out=ow[0].desc(A.out)),
            before=[prev])


# ---- (d) rsr_diff_tiles and rsr_diff_tiles_sequence ---------------------------------------------------------------------------------------
def flipped(x, byte):
    """x with one bit of byte `byte` of its packed form changed."""
    b = fl.raw(x).copy()
    b[byte] ^= 1
    return b.view(x.dtype).reshape(x.shape)


def planted(fmt, x, w, h, c):
    """x itself; x with the last byte of the last row of plane 0 -- the last row of the last tile -- changed; and x with a byte of the last
    row of plane 2 or of the UV plane changed (uint8 HWC has one plane: the first byte of its last row)."""
    rb = fl.rowbytes(fmt, w, c)
    second = (h - 1) * rb if fmt == U8 else fl.raw(x).size - 1 - rb // 2
    return [x, flipped(x, h * rb - 1), flipped(x, second)]


def runs(idx):
    """The sorted unique positions idx as (start, end) runs of consecutive ones."""
    idx = np.unique(idx)
    cut = np.nonzero(np.diff(idx) != 1)[0] + 1
    return [(int(r[0]), int(r[-1]) + 1) for r in np.split(idx, cut)] if idx.size else []


def narrowed_positions(wn):
    """Arena indices of every narrowed offset of the window's bytes that is no byte of the window itself."""
    far, rest = wn.offsets()
    true = far + rest
    al = np.concatenate([a[a != true] for a in fl.alias32(far, rest)])
    return runs(np.setdiff1d(al, true) + wn.col + fl.BASE)


def diff_mask(s, a, b, fmt, w, h, c, n=None, prev=None):
    """rsr_diff_tiles (n None) or rsr_diff_tiles_sequence (a = the list of frames) into a mask pre-filled with 0xCD."""
    nx, ny = ref.tile_count(w, h, T)
    d_m = filled_bytes(nx * ny * (n or 1))
    torch.cuda.synchronize()
    if n is None:
        s.diff_tiles(a, b, fmt, w, h, c, d_m.data_ptr())
    else:
        s.diff_tiles_sequence(a, prev, fmt, w, h, c, d_m.data_ptr())
    torch.cuda.synchronize()
    m = d_m.cpu().numpy()
    assert set(m.tolist()) <= {0, 1}, m
    return m.reshape(n or 1, nx * ny)


DIFF_CASES = [(f, k) for f in DIFF_FORMATS for k in fl.KINDS if not (k == "Pn" and f[1] == U8)]


@pytest.mark.parametrize("fmtcase,kind", DIFF_CASES, ids=["%s-%s" % (f[0], k) for f, k in DIFF_CASES])
def test_diff_of_far_operands(ctx, A, fmtcase, kind):
    """a in the input arena, b in the output arena (co-aligned to 16 bytes, and at the column that agrees modulo the element size only),
    and either against a packed copy of the other: the mask is tests/tile_diff_ref.py's for equal frames and for a byte planted in the
    last row of the last tile, then in plane 2 / the UV plane -- a narrowed read misses the planted byte.  The converse: equal frames, and
    the bytes at every narrowed offset made to differ between the two arenas: the mask stays zero."""
    _, fmt, c = fmtcase
    s = ctx[False]
    w, h = fl.m_size(fmt) if kind == "M" else (W, H)
    x = fl.image(300, fmt, w, h, c)
    g = fl.group(kind, fmt, w, h, c)
    wa = g[0]
    d_x = dev(x)
    got, poked = [], []
    try:
        fl.put(A.inp, wa, x)
        for wb in (g[1], g[3]):
            for b in planted(fmt, x, w, h, c):
                want = ref.diff_mask(fmt, x, b, T, P).tolist()
                fl.put(A.out, wb, b)
                d_b = dev(b)
                got.append((want, diff_mask(s, wa.desc(A.inp), wb.desc(A.out), fmt, w, h, c)[0].tolist(), "far | far", wb.col))
                got.append((want, diff_mask(s, wa.desc(A.inp), d_b.data_ptr(), fmt, w, h, c)[0].tolist(), "far | packed", wb.col))
                got.append((want, diff_mask(s, d_x.data_ptr(), wb.desc(A.out), fmt, w, h, c)[0].tolist(), "packed | far", wb.col))
            # the converse
            fl.put(A.out, wb, x)
            for arena, wn, v in ((A.inp, wa, 0x11), (A.out, wb, 0x22)):
                for r0, r1 in narrowed_positions(wn):
                    arena[r0:r1].fill_(v)
                    poked.append((arena, r0, r1))
            got.append(([0] * len(want), diff_mask(s, wa.desc(A.inp), wb.desc(A.out), fmt, w, h, c)[0].tolist(), "narrowed offsets differ", wb.col))
            for arena, r0, r1 in poked:
                arena[r0:r1].fill_(fl.FILL)
            poked = []
            fl.refill(A.out, wb)
    finally:
        for arena, r0, r1 in poked:
            arena[r0:r1].fill_(fl.FILL)
        bad_in, bad_out = clean(A, [wa], [g[1], g[3]])
    wants = [ref.diff_mask(fmt, x, b, T, P).tolist() for b in planted(fmt, x, w, h, c)]
    assert wants[0] == [0] * len(wants[0]) and wants[1][-1] == 1 and any(wants[2])
    for want, m, what, col in got:
        assert m == want, (what, col)
    assert bad_in is None and bad_out is None, (bad_in, bad_out)


@pytest.mark.parametrize("fmtcase,kind", DIFF_CASES, ids=["%s-%s" % (f[0], k) for f, k in DIFF_CASES])
def test_diff_sequence_of_far_frames(ctx, A, fmtcase, kind):
    """prev and three frames in the four windows of the input arena: frame 0 = prev, frame 1 differs in the last byte of the last row of
    plane 0, frame 2 from frame 1 in a byte of plane 2 / the UV plane.  Row k of the mask is tests/tile_diff_ref.py's for the pair."""
    _, fmt, c = fmtcase
    s = ctx[False]
    w, h = fl.m_size(fmt) if kind == "M" else (W, H)
    x = fl.image(310, fmt, w, h, c)
    _, b1, _ = planted(fmt, x, w, h, c)
    b2 = planted(fmt, b1, w, h, c)[2]
    frames = [x, x, b1, b2]
    want = [ref.diff_mask(fmt, frames[k], frames[k + 1], T, P).tolist() for k in range(3)]
    nt = len(want[0])
    assert nt == (2 if kind == "M" else NT) and want[0] == [0] * nt and want[1][-1] == 1 and any(want[2])
    g = fl.group(kind, fmt, w, h, c)
    try:
        for wn, f in zip(g, frames):
            fl.put(A.inp, wn, f)
        got = diff_mask(s, [wn.desc(A.inp) for wn in g[1:]], None, fmt, w, h, c, n=3, prev=g[0].desc(A.inp)).tolist()
        first = diff_mask(s, [wn.desc(A.inp) for wn in g[1:]], None, fmt, w, h, c, n=3, prev=None).tolist()
    finally:
        bad_in, bad_out = clean(A, g, [])
    assert got == want and first == [[1] * nt] + want[1:]
    assert bad_in is None and bad_out is None, (bad_in, bad_out)


# ---- (e) inputs at the admitted maximum ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
@pytest.mark.parametrize("fmt,c", [(U8, 3), (U8, 4), (F16, 3), (F32, 3)], ids=["u8c3", "u8c4", "f16", "f32"])
def test_inputs_at_the_largest_row_pitch(ctx, A, fmt, c, tta):
    """Layout M: a 52 x 3 input whose row pitch is the largest admitted (2^31 - 1, or 2^31 - 4 for the float formats), so that row 2 starts
    below 2^32 and ends beyond it; the output is packed, with 4 KiB of 0xCD on either side."""
    s = ctx[tta]
    w, h = fl.m_size(fmt)
    x = fl.image(400, fmt, w, h, c)
    want = packed_batch(s, [x], fmt, fmt, c, w, h)[0]
    n = fl.raw(want).size
    d_out = filled_bytes(n + 8192)
    iw = fl.group("M", fmt, w, h, c, n=1)
    far_run(A, iw, [x], [], [], lambda: s.process_device_batch([iw[0].desc(A.inp)], fmt, w, h, c, [d_out.data_ptr() + 4096], fmt))
    got = d_out.cpu().numpy()
    assert np.array_equal(got[4096:4096 + n], fl.raw(want))
    assert (got[:4096] == fl.FILL).all() and (got[4096 + n:] == fl.FILL).all()


# ---- (f) torch_io -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,kind", [(U8, "R"), (F16, "R"), (F16, "Pn")], ids=["u8-R", "f16-R", "f16-Pn"])
def test_upscale_of_as_strided_views(ctx, A, fmt, kind):
    """torch_io.upscale(sr, crop, out=window) on as_strided views of the arenas: describe() yields the far descriptors -- the views' own
    data_ptr and pitches, so no .contiguous() copy stands in for either -- and the window receives the packed result."""
    s = ctx[False]
    x = fl.image(500, fmt)
    want = packed_batch(s, [x], fmt, fmt)[0]
    iw, ow = fl.group(kind, fmt, W, H, n=2)[1], fl.group(kind, fmt, 4 * W, 4 * H, n=3)[2]
    d_in, crop = fl.view(A.inp, (iw.row_pitch, iw.plane_pitch), fmt, W, H, 3, iw.col)
    d_out, window = fl.view(A.out, (ow.row_pitch, ow.plane_pitch), fmt, 4 * W, 4 * H, 3, ow.col)
    assert d_in == iw.desc(A.inp) and d_out == ow.desc(A.out)
    plane = (lambda wn: 0 if fmt == U8 else wn.plane_pitch)
    assert torch_io.describe(crop) == (crop.data_ptr(), iw.row_pitch, plane(iw)) == (d_in[0], d_in[1], plane(iw))
    assert torch_io.describe(window) == (window.data_ptr(), ow.row_pitch, plane(ow)) == (d_out[0], d_out[1], plane(ow))
    assert not crop.is_contiguous() and not window.is_contiguous()
    returned = []
    far_run(A, [iw], [x], [ow], [want], lambda: returned.append(torch_io.upscale(s, crop, out=window)))
    assert returned[0] is window
