"""Masked tile processing and the device frame diff on the GPU (run with -m gpu): rsr_diff_tiles, rsr_process_device_masked and
torch_io.upscale_delta.  Every comparison is EXACT: a masked call must write, for the tiles it runs, the bytes the plain call writes, and
nothing else; the diff must mark exactly the tiles tests/tile_diff_ref.py marks.

The base case is 70 x 50 at tile 32, prepadding 10: a 3 x 2 grid whose last tiles are 6 wide and 18 high, every source rectangle clipped
at some image edge, the halos of neighbours overlapping (tile 0 reads columns [0, 42), tile 1 [22, 70), tile 2 [54, 70)).  Outputs are
pre-filled with 0xCD bytes (NaN for the float formats)."""
import ctypes as C
import threading
from fractions import Fraction

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

import tile_diff_ref as ref
from gpu_support import DIFF_FORMATS, context_fixtures, dev, out_dims, paths, profile_of  # noqa: F401
from pixfmt_ref import F16, F32, NP, NV12, NV16, P010, P210, P444, S420, S422, U8, YUV444P, YUV444P10, image_at, paste, same_bits, sentinel, shape_of

pytestmark = pytest.mark.gpu
W, H, T, P = 70, 50, 32, 10
NT = 6
CHECKER = [1, 0, 1, 0, 1, 0]
MASKS = [[int(i == t) for i in range(NT)] for t in range(NT)] + [CHECKER, [1 - m for m in CHECKER]]


ctxs, ctx = context_fixtures(T, P)
image = image_at(W, H)


def call(s, x, in_fmt, out_fmt, mask, w=W, h=H, c=3, into=None):
    """One synchronous call on the packed numpy image x: the plain n = 1 batch call (mask None) or the masked one.  The destination is
    `into` (a numpy image as a previous call left it) or a sentinel."""
    ow, oh = out_dims(s, w, h)
    oshape = shape_of(out_fmt, ow, oh, c)
    d_in = dev(x)
    d_out = dev(into if into is not None else sentinel(out_fmt, oshape))
    if mask is None:
        s.process_device_batch([d_in.data_ptr()], in_fmt, w, h, c, [d_out.data_ptr()], out_fmt)
    else:
        s.process_device_masked(d_in.data_ptr(), in_fmt, w, h, c, d_out.data_ptr(), out_fmt, mask)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(NP[out_fmt]).reshape(oshape)


def expected(s, fmt, plain, mask, w=W, h=H, base=None):
    """What a masked call must leave: `base` (default: the sentinel) with the output rectangles of the marked tiles from the plain result."""
    e = sentinel(fmt, plain.shape) if base is None else base.copy()
    r = s.out_ratio
    for t, m in enumerate(mask):
        if m:
            paste(fmt, e, plain, ref.out_rect(w, h, s.tilesize, t, r.numerator, r.denominator))
    return e


# (id, in_fmt, out_fmt, c, yuv_siting, takes ratio 3/2)
FORMATS = [("u8c3", U8, U8, 3, 0, True), ("u8c4", U8, U8, 4, 0, False), ("f16", F16, F16, 3, 0, False), ("f32", F32, F32, 3, 0, True),
           ("nv12-s0", NV12, NV12, 3, 0, False), ("nv12-s2", NV12, NV12, 3, 2, False), ("p010-s0", P010, P010, 3, 0, False),
           ("p010-s2", P010, P010, 3, 2, False), ("u8-nv12", U8, NV12, 3, 0, False)]


@pytest.mark.parametrize("fmtcase", FORMATS, ids=[f[0] for f in FORMATS])
@pytest.mark.parametrize("mode", ["default", "tta", "precise", "bgr"])
def test_masked_equals_plain_rectangle_by_rectangle(ctx, mode, fmtcase):
    _, in_fmt, out_fmt, c, siting, ratio = fmtcase
    s = ctx[mode == "tta"]
    s.set_option("precise", int(mode == "precise"))
    s.set_option("bgr", int(mode == "bgr"))
    s.set_option("yuv_siting", siting)
    x = image(11, in_fmt, c=c)
    for scale in [4, 2, 1] + ([Fraction(3, 2)] if ratio else []):
        s.out_ratio = scale
        assert out_dims(s, W, H) == ((105, 75) if scale == Fraction(3, 2) else (W * scale, H * scale))
        plain = call(s, x, in_fmt, out_fmt, None, c=c)
        assert not same_bits(plain, sentinel(out_fmt, plain.shape))
        for mask in MASKS:
            got = call(s, x, in_fmt, out_fmt, mask, c=c)
            assert same_bits(got, expected(s, out_fmt, plain, mask)), (scale, mask)
        # the complement, run into the buffer the checkerboard left, completes the frame
        half = call(s, x, in_fmt, out_fmt, CHECKER, c=c)
        full = call(s, x, in_fmt, out_fmt, [1 - m for m in CHECKER], c=c, into=half)
        assert same_bits(full, plain), scale


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_all_ones_is_the_plain_call_and_zero_launches_nothing(ctx, tta):
    s = ctx[tta]
    x = image(12, U8)
    plain = call(s, x, U8, U8, None)
    stats = {k: s.get_stat(k) for k in ("masked_calls", "masked_tiles_run", "masked_tiles_skipped", "masked_batches")}
    got, p = profile_of(s, lambda: call(s, x, U8, U8, [1] * NT))
    assert same_bits(got, plain) and p["conv_launches"] == R.NUM_CONVS and p["calls"] == 1 and p["tiles"] == NT * (8 if tta else 1)
    got, p = profile_of(s, lambda: call(s, x, U8, U8, [3, 0, 0, 0, 0, 255]))  # (any non-zero byte marks a tile)
    assert same_bits(got, expected(s, U8, plain, [1, 0, 0, 0, 0, 1])) and p["conv_launches"] == R.NUM_CONVS and p["tiles"] == 2 * (8 if tta else 1)
    got, p = profile_of(s, lambda: call(s, x, U8, U8, [0] * NT))
    assert same_bits(got, sentinel(U8, plain.shape)) and p["conv_launches"] == 0 and p["tiles"] == 0
    assert s.get_stat("masked_calls") == stats["masked_calls"] + 3
    assert s.get_stat("masked_tiles_run") == stats["masked_tiles_run"] + NT + 2
    assert s.get_stat("masked_tiles_skipped") == stats["masked_tiles_skipped"] + (NT - 2) + NT
    assert s.get_stat("masked_batches") == stats["masked_batches"] + 1  # (only the partial mask builds batches of its own)


def test_progress_is_reported_once_per_selected_tile(ctx):
    s = ctx[False]
    seen = []
    cb = C.CFUNCTYPE(None, C.c_int, C.c_int, C.c_void_p)(lambda done, total, user: seen.append((done, total)))
    L = R.lib()
    assert L.rsr_set_progress_callback(s._h, C.cast(cb, C.c_void_p), None) == 0
    try:
        call(s, image(13, U8), U8, U8, CHECKER)
    finally:
        assert L.rsr_set_progress_callback(s._h, None, None) == 0
    assert seen == [(1, 3), (2, 3), (3, 3)]


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_several_batches(ctx, tta):
    """A slot of the frame's largest tile, 52 x 52 padded pixels, is 16.4 MB of workspace: under a budget of 40 MB a batch takes two
    slots (under TTA one tile's eight, the least there is), so four marked tiles need at least two batches."""
    s = ctx[tta]
    x = image(14, U8)
    plain = call(s, x, U8, U8, None)
    mask = [1, 1, 0, 1, 1, 0]
    s.set_option("max_workspace_mb", 40)
    before = s.get_stat("masked_batches")
    got = call(s, x, U8, U8, mask)
    batches = s.get_stat("masked_batches") - before
    assert batches == (4 if tta else 2)
    assert same_bits(got, expected(s, U8, plain, mask))
    s.set_option("max_workspace_mb", 65536)
    assert same_bits(call(s, x, U8, U8, None), plain) and s.get_stat("ws_clamp_mb") == -1


def test_pitched_images_and_windows(ctx):
    s = ctx[False]
    mask = [0, 1, 1, 1, 0, 0]
    # uint8: a crop at an odd byte offset inside a larger frame, into a window of a canvas
    x = image(15, U8)
    plain = call(s, x, U8, U8, None)
    frame = np.random.default_rng(1).integers(0, 256, size=(64, 101, 3), dtype=np.uint8)
    frame[9:9 + H, 6:6 + W] = x
    canvas = np.full((260, 400, 3), 0xCD, dtype=np.uint8)
    d_frame, d_canvas = dev(frame), dev(canvas)
    src = (d_frame.data_ptr() + (9 * 101 + 6) * 3, 101 * 3, 0)
    dst = (d_canvas.data_ptr() + (31 * 400 + 47) * 3, 400 * 3, 0)
    assert src[0] % 2 == 1
    s.process_device_masked(src, U8, W, H, 3, dst, U8, mask)
    torch.cuda.synchronize()
    want = canvas.copy()
    want[31:31 + 4 * H, 47:47 + 4 * W] = expected(s, U8, plain, mask)
    assert same_bits(d_canvas.cpu().numpy().reshape(canvas.shape), want)
    # float: a crop view of a larger planar tensor into a window of a planar canvas
    xf = image(16, F32)
    plain_f = call(s, xf, F32, F32, None)
    big = np.random.default_rng(2).uniform(0, 1, size=(3, 60, 90)).astype(np.float32)
    big[:, 4:4 + H, 13:13 + W] = xf
    canvas_f = np.full((3, 230, 300), np.nan, dtype=np.float32)
    d_big, d_cf = dev(big), dev(canvas_f)
    src = (d_big.data_ptr() + (4 * 90 + 13) * 4, 90 * 4, 60 * 90 * 4)
    dst = (d_cf.data_ptr() + (17 * 300 + 9) * 4, 300 * 4, 230 * 300 * 4)
    s.process_device_masked(src, F32, W, H, 3, dst, F32, mask)
    torch.cuda.synchronize()
    want = canvas_f.copy()
    want[:, 17:17 + 4 * H, 9:9 + 4 * W] = expected(s, F32, plain_f, mask)
    assert same_bits(d_cf.cpu().numpy().view(np.float32).reshape(canvas_f.shape), want)


# ---- the diff ---------------------------------------------------------------------------------------------------------------------------
def gpu_mask(s, a, b, fmt, w, h, c=3, place_b=None):
    """rsr_diff_tiles on the numpy images a and b, synchronously; the mask buffer is pre-filled with 0xCD.  place_b = (offset, row pitch,
    plane pitch) in bytes puts b inside a larger allocation (a is packed)."""
    nx, ny = ref.tile_count(w, h, s.tilesize)
    d_a = dev(a)
    if place_b is None:
        d_b = dev(b)
        desc_b = d_b.data_ptr()
    else:
        off, row, plane = place_b
        es = b.dtype.itemsize
        rowbytes = w * es * (c if fmt == U8 else 1)
        planar = fmt in (F16, F32) + P444
        host = np.random.default_rng(3).integers(0, 256, size=off + R.image_span(fmt, w, h, c, row, plane) + 64, dtype=np.uint8)
        raw = np.ascontiguousarray(b).view(np.uint8).reshape(-1, rowbytes)  # rows of every plane, in order
        if fmt == U8:
            starts = [off + y * row for y in range(h)]
        elif planar:
            starts = [off + q * plane + y * row for q in range(3) for y in range(h)]
        else:
            starts = [off + y * row for y in range(h)] + [off + plane + y * row for y in range(h if fmt in S422 else h // 2)]
        for r_, st in zip(raw, starts):
            host[st:st + rowbytes] = r_
        d_b = torch.from_numpy(host).cuda()
        desc_b = (d_b.data_ptr() + off, row, plane)
    d_m = torch.full((nx * ny,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the fill runs on torch's null stream, the diff on the context's non-blocking one: without this wait the fill may land behind the diff's memset)
    s.diff_tiles(d_a.data_ptr(), desc_b, fmt, w, h, c, d_m.data_ptr())
    m = d_m.cpu().numpy()
    assert set(m.tolist()) <= {0, 1}, m
    # rsr_diff_tiles IS the sequence of the one pair (prev = a, frames = [b]): row 0 of its masks
    d_m.fill_(0xCD)
    torch.cuda.synchronize()
    s.diff_tiles_sequence([desc_b], d_a.data_ptr(), fmt, w, h, c, d_m.data_ptr())
    assert d_m.cpu().numpy().tolist() == m.tolist()
    return m


def poke(fmt, x, px, py, ch=0, chroma=None, h=H):
    """x with ONE sample changed by one bit: luma / element (px, py) of channel ch, or, chroma = 0 / 1, the U / V of chroma pair (px, py)."""
    y = x.copy()
    v = y.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[y.dtype.itemsize])
    if fmt == U8:
        v[py, px, ch] ^= 1
    elif fmt in (F16, F32) + P444:
        v[ch, py, px] ^= 1
    elif chroma is None:
        v[py, px] ^= 1  # (P010: one of the low 6 bits)
    else:
        v[h + py, 2 * px + chroma] ^= 1
    return y


# (id, fmt, c, w, h, tile): the families the feature came with on the base case; the later ones at 35 x 25 (4:4:4) and 36 x 26 (4:2:2) with
# tile 16 -- a 3 x 2 grid again, the smallest with an interior tile, an edge tile, an odd chroma boundary and a clipped halo
DIFF_CASES = [f + (W, H, T) for f in DIFF_FORMATS] + [("nv16", NV16, 3, 36, 26, 16), ("p210", P210, 3, 36, 26, 16), ("yuv444p", YUV444P, 3, 35, 25, 16),
                                                      ("yuv444p10", YUV444P10, 3, 35, 25, 16)]
DIFF_IDS = [f[0] for f in DIFF_CASES]


@pytest.mark.parametrize("name,fmt,c,w,h,tile", DIFF_CASES, ids=DIFF_IDS)
def test_diff_against_the_reference(ctx, name, fmt, c, w, h, tile):
    s = ctx[False]
    s.tilesize = tile
    base = (w, h, tile) == (W, H, T)
    a = image(21, fmt, w, h, c)
    assert gpu_mask(s, a, a, fmt, w, h, c).tolist() == [0] * NT
    last = c - 1 if fmt == U8 else 2  # (c == 4: the alpha byte)
    for t in (0, 4):
        x0, y0, x1, y1 = ref.source_rect(w, h, tile, P, t)
        inside = [(x0, y0), (x1 - 1, y0), (x0, y1 - 1), (x1 - 1, y1 - 1)]
        outside = [(x0 - 1, y0), (x1, y0), (x0, y0 - 1), (x0, y1), (x1, y1 - 1)]
        for px, py in inside + [q for q in outside if 0 <= q[0] < w and 0 <= q[1] < h]:
            b = poke(fmt, a, px, py, ch=last, h=h)
            want = ref.diff_mask(fmt, a, b, tile, P)
            assert want[t] == int((px, py) in inside) and want.any()
            assert gpu_mask(s, a, b, fmt, w, h, c).tolist() == want.tolist(), (t, px, py)
    # the last column of tile 0's rectangle lies in its right neighbours' too, the one behind it in theirs only (the base case: column 41
    # is inside tile 0's [0, 42) and tile 1's [22, 70); column 42 in tile 1's only)
    x1 = ref.source_rect(w, h, tile, P, 0)[2]
    for px, want0 in ((x1 - 1, 1), (x1, 0)):
        b = poke(fmt, a, px, 5, ch=last, h=h)
        want = ref.diff_mask(fmt, a, b, tile, P).tolist()
        assert want[0] == want0 and want[1] == 1 and want[3:] == [0, 0, 0] and (not base or (px, want) == (42 - want0, [want0, 1, 0, 0, 0, 0]))
        assert gpu_mask(s, a, b, fmt, w, h, c).tolist() == want
    if fmt in S420 + S422:
        # the chroma pair one sample beyond tile 0's luma columns [0, x1) (its own pairs are 0 .. x1 / 2 - 1) is compared all the same; the
        # next one not (the base case: pairs 21 and 22)
        for cx, want0 in ((x1 // 2, 1), (x1 // 2 + 1, 0)):
            for uv in (0, 1):
                b = poke(fmt, a, cx, 3, chroma=uv, h=h)
                want = ref.diff_mask(fmt, a, b, tile, P)
                assert want[0] == want0 and gpu_mask(s, a, b, fmt, w, h, c).tolist() == want.tolist(), (cx, uv)
    if fmt in S420:
        # chroma row 21 against tile 0's luma rows [0, 42), likewise
        b = poke(fmt, a, 2, 21, chroma=1, h=h)
        want = ref.diff_mask(fmt, a, b, tile, P)
        assert want.tolist() == [1, 0, 0, 1, 0, 0] and gpu_mask(s, a, b, fmt, w, h, c).tolist() == want.tolist()
    if fmt in S422:
        # a UV row per Y row, nothing beyond: tile row 1 reads rows [6, 26), so chroma row 5 is tile row 0's alone and row 6 both rows'
        # (pair 0: of the tiles of a row, only the first reads it)
        for cy, want3 in ((5, 0), (6, 1)):
            b = poke(fmt, a, 0, cy, chroma=1, h=h)
            want = ref.diff_mask(fmt, a, b, tile, P)
            assert want.tolist() == [1, 0, 0, want3, 0, 0] and gpu_mask(s, a, b, fmt, w, h, c).tolist() == want.tolist()
    if fmt == F32:
        z = a.copy()
        z[1, 30, 30] = 0.0
        n = z.copy()
        n[1, 30, 30] = -0.0
        assert z[1, 30, 30] == n[1, 30, 30]
        want = ref.diff_mask(fmt, z, n, tile, P)
        assert want.tolist() == [1, 1, 0, 1, 1, 0] and gpu_mask(s, z, n, fmt, w, h, c).tolist() == want.tolist()


@pytest.mark.parametrize("name,fmt,c,w,h,tile", DIFF_CASES, ids=DIFF_IDS)
def test_diff_of_pitched_against_packed_operands(ctx, name, fmt, c, w, h, tile):
    """b inside a larger allocation: at offsets and pitches that agree with the packed a modulo 16, modulo 4 only, and not at all (uint8
    and the 8-bit surfaces; the wider elements as far as their alignment lets them)."""
    s = ctx[False]
    s.tilesize = tile
    a = image(22, fmt, w, h, c)
    es = a.dtype.itemsize
    rowbytes = w * es * (c if fmt == U8 else 1)
    rows = h if fmt != U8 else 0
    for off, pad in ((0, 0), (16, 32), (4, 12), (8 if es == 4 else 2, 4 if es == 4 else 6)) + (((3, 7), (1, 0)) if es == 1 else ()):
        row = rowbytes + pad
        plane = (rows + 3) * row if fmt != U8 else 0
        for b in (a, poke(fmt, a, min(41, w - 2), min(41, h - 2), ch=1, h=h), poke(fmt, a, w - 1, h - 1, ch=2, h=h), poke(fmt, a, 0, 0, h=h)):
            want = ref.diff_mask(fmt, a, b, tile, P)
            assert gpu_mask(s, a, b, fmt, w, h, c, place_b=(off, row, plane)).tolist() == want.tolist(), (off, pad)


@pytest.mark.parametrize("name,fmt,c", [f[:3] for f in DIFF_CASES])
def test_diff_of_a_row_longer_than_a_workgroup_pass(ctx, name, fmt, c):
    """230 x 36 at tile 200: tile 0's rectangle is 210 pixels wide -- 840 bytes of RGBA or fp32, 210 of luma --, more than 64 lanes cover in
    one step of 4-byte or 1-byte pieces; the change sits at the far end of the row.  Every family at this one geometry: a row this long
    is what the test is about."""
    s = ctx[False]
    s.tilesize = 200
    w, h = 230, 36
    a = image(23, fmt, w, h, c)
    es = a.dtype.itemsize
    rowbytes = w * es * (c if fmt == U8 else 1)
    for off, pad in ((0, 0), (4, 4)) + (((1, 0),) if es == 1 else ()):
        row = rowbytes + pad
        plane = (h + 1) * row if fmt != U8 else 0
        for px, want in ((209, [1, 1]), (210, [0, 1]), (189, [1, 0]), (190, [1, 1]), (229, [0, 1])):
            b = poke(fmt, a, px, h - 1, ch=2, h=h)
            assert ref.diff_mask(fmt, a, b, 200, P).tolist() == want
            assert gpu_mask(s, a, b, fmt, w, h, c, place_b=(off, row, plane)).tolist() == want, (off, px)


# ---- soundness: the point of the feature ----------------------------------------------------------------------------------------------------
EDGE_X, EDGE_Y = [21, 22, 41, 42, 53, 54], [21, 22, 41, 42]


def next_frame(fmt, a, seed):
    """Frame a with 1 .. 3 random samples changed: half of them on the columns / rows where a source rectangle begins or ends, and for a
    surface a third of them chroma-only."""
    rng = np.random.default_rng(1000 + seed)
    b = a
    for _ in range(int(rng.integers(1, 4))):
        px = int(rng.choice(EDGE_X)) if rng.integers(2) else int(rng.integers(W))
        py = int(rng.choice(EDGE_Y)) if rng.integers(2) else int(rng.integers(H))
        if fmt == NV12 and rng.integers(3) == 0:
            b = poke(fmt, b, px // 2, py // 2, chroma=int(rng.integers(2)))
        else:
            b = poke(fmt, b, px, py, ch=int(rng.integers(3)))
    return b


SOUND = [("u8", U8, 0), ("f16", F16, 0), ("nv12-s0", NV12, 0), ("nv12-s1", NV12, 1), ("nv12-s2", NV12, 2)]
SEEDS = range(20)


def test_the_seeds_leave_most_frames_mostly_unchanged():
    """The condition on the inputs of the test below, counted on the CPU: in at least half of the seeds fewer than all 6 tiles change."""
    assert R.tile_count(W, H, T) == (3, 2) and ref.tile_count(W, H, T) == (3, 2)
    for _, fmt, _ in SOUND:
        a = image(31, fmt)
        counts = [int(ref.diff_mask(fmt, a, next_frame(fmt, a, seed), T, P).sum()) for seed in SEEDS]
        assert min(counts) >= 1 and sum(n < NT for n in counts) * 2 >= len(counts), counts


@pytest.mark.parametrize("name,fmt,siting", SOUND, ids=[f[0] for f in SOUND])
def test_upscale_delta_equals_upscale(ctx, name, fmt, siting):
    s = ctx[False]
    s.set_option("yuv_siting", siting)
    up = torch_io.upscale_yuv if fmt == NV12 else torch_io.upscale
    a = image(31, fmt)
    ta = torch.from_numpy(a).cuda()
    ya = up(s, ta)
    few = 0
    for seed in SEEDS:
        b = next_frame(fmt, a, seed)
        want_mask = ref.diff_mask(fmt, a, b, T, P)
        tb = torch.from_numpy(b).cuda()
        want = up(s, tb)
        y = ya.clone()
        out, n = torch_io.upscale_delta(s, tb, ta, y)
        torch.cuda.synchronize()
        assert out is y and n == int(want_mask.sum()), (seed, n, want_mask)
        assert torch.equal(out.view(torch.uint8), want.view(torch.uint8)), seed
        few += n < NT
    assert few * 2 >= len(SEEDS)
    # without a previous frame every tile runs; another `out` first receives prev_y
    y = torch.zeros_like(ya)
    out, n = torch_io.upscale_delta(s, ta, None, y)
    torch.cuda.synchronize()
    assert n == NT and torch.equal(out.view(torch.uint8), ya.view(torch.uint8))
    other = torch.zeros_like(ya)
    out, n = torch_io.upscale_delta(s, ta, ta, ya, out=other)
    torch.cuda.synchronize()
    assert out is other and n == 0 and torch.equal(other.view(torch.uint8), ya.view(torch.uint8))


def undescribable(fmt, x):
    """The numpy image x on the device as a view no rsr_image describes -- uint8: a permuted CHW tensor; fp16: every second column of a
    tensor twice as wide; NV12: a (y, uv) pair whose uv lies BELOW y in memory -- so that upscale_delta has to pack it first."""
    if fmt == U8:
        v = torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1))).cuda().permute(1, 2, 0)
        assert torch_io.describe(v) is None
    elif fmt == F16:
        wide = torch.zeros((3, H, 2 * W), dtype=torch.float16, device="cuda")
        wide[:, :, ::2] = torch.from_numpy(x).cuda()
        v = wide[:, :, ::2]
        assert torch_io.describe(v) is None
    else:
        buf = torch.zeros((H * 3 // 2, W), dtype=torch.uint8, device="cuda")
        t = torch.from_numpy(x).cuda()
        buf[:H // 2], buf[H // 2:] = t[H:], t[:H]
        v = (buf[H // 2:], buf[:H // 2])
        assert torch_io._describe_yuv(*v) is None
    return v


@pytest.mark.parametrize("name,fmt", [("u8", U8), ("f16", F16), ("nv12", NV12)])
def test_upscale_delta_of_views_that_must_be_packed_on_the_default_stream(ctx, name, fmt):
    """x and prev_x are views no descriptor fits, and torch's current stream is the default one: both packed copies are made on that
    stream, the diff and the masked call run on a side stream behind them.  The allocator hands the copies memory that held other frames
    a moment ago, so a diff that ran ahead of a copy would compare stale bytes."""
    s = ctx[False]
    assert torch.cuda.current_stream().cuda_stream == 0
    up = torch_io.upscale_yuv if fmt == NV12 else torch_io.upscale
    a = image(33, fmt)
    ta = torch.from_numpy(a).cuda()
    ya = up(s, ta)
    for seed in SEEDS:
        b = next_frame(fmt, a, seed)
        want = up(s, torch.from_numpy(b).cuda())
        y = ya.clone()
        churn = [torch.from_numpy(b).cuda().clone() for _ in range(4)]  # (freed below: what the packed copies are then made in)
        del churn
        prev_y = (y[:4 * H], y[4 * H:]) if fmt == NV12 else y  # (a pair of views in, a pair of views of the result)
        out, n = torch_io.upscale_delta(s, undescribable(fmt, b), undescribable(fmt, a), prev_y)
        torch.cuda.synchronize()
        assert out is prev_y and n == int(ref.diff_mask(fmt, a, b, T, P).sum()), seed
        assert torch.equal(y.view(torch.uint8), want.view(torch.uint8)), seed


# ---- errors and concurrency ---------------------------------------------------------------------------------------------------------------
def test_a_refused_workspace_halves_this_call_and_leaves_no_clamp(ctx):
    """Test hook ws_fail_above_mb: four marked tiles want 4 slots of 16.4 MB; workspaces above 40 MB are refused, so the call halves its
    batches to two slots, runs, and plants no ws_clamp for later calls.  With every workspace refused the call fails with RSR_E_NOMEM,
    writes nothing and counts nothing."""
    s = ctx[False]
    x = image(43, U8)
    plain = call(s, x, U8, U8, None)
    mask = [1, 1, 0, 1, 1, 0]
    keys = ("masked_calls", "masked_tiles_run", "masked_tiles_skipped", "masked_batches", "ws_failures")
    try:
        s.set_option("ws_fail_above_mb", 40)
        before = {k: s.get_stat(k) for k in keys}
        got = call(s, x, U8, U8, mask)
        assert same_bits(got, expected(s, U8, plain, mask))
        assert s.get_stat("ws_failures") == before["ws_failures"] + 1 and s.get_stat("masked_batches") == before["masked_batches"] + 2
        assert s.get_stat("ws_clamp_mb") == -1
        assert s.get_stat("masked_calls") == before["masked_calls"] + 1 and s.get_stat("masked_tiles_run") == before["masked_tiles_run"] + 4
        s.set_option("ws_fail_above_mb", 0)
        before = {k: s.get_stat(k) for k in keys}
        d_in = dev(x)
        d_out = torch.full((16 * W * H * 3,), 0xCD, dtype=torch.uint8, device="cuda")
        with pytest.raises(R.RealSRError) as e:
            s.process_device_masked(d_in.data_ptr(), U8, W, H, 3, d_out.data_ptr(), U8, mask)
        torch.cuda.synchronize()
        assert e.value.code == R.RSR_E_NOMEM and bool((d_out == 0xCD).all()) and s.get_stat("ws_clamp_mb") == -1
        for k in keys[:4]:
            assert s.get_stat(k) == before[k], k
    finally:
        s.set_option("ws_fail_above_mb", -1)
    assert same_bits(call(s, x, U8, U8, None), plain) and s.get_stat("plan_batches") == 1 and s.get_stat("ws_clamp_mb") == -1
    assert same_bits(call(s, x, U8, U8, mask), expected(s, U8, plain, mask))


def test_errors_leave_out_untouched(ctx):
    s = ctx[False]
    x = image(41, U8)
    d_in = dev(x)
    d_out = torch.full((16 * W * H * 3,), 0xCD, dtype=torch.uint8, device="cuda")

    def refused(fn):
        with pytest.raises(R.RealSRError) as e:
            fn()
        assert e.value.code == R.RSR_E_ARG
        torch.cuda.synchronize()
        assert bool((d_out == 0xCD).all())

    refused(lambda: s.process_device_masked(d_in.data_ptr(), U8, W, H, 3, d_out.data_ptr(), U8, [1] * (NT - 1)))
    refused(lambda: s.process_device_masked(d_in.data_ptr(), U8, W, H, 3, d_out.data_ptr(), U8, [1] * (NT + 1)))
    refused(lambda: s.process_device_masked(d_in.data_ptr(), U8, W, H, 3, d_out.data_ptr(), U8, None))
    refused(lambda: s.process_device_masked(d_in.data_ptr(), U8, W, H, 3, d_out.data_ptr(), U8, (0, NT)))
    refused(lambda: s.process_device_masked(d_in.data_ptr(), NV12, W - 1, H, 3, d_out.data_ptr(), NV12, [1] * NT))   # an odd-width NV12
    refused(lambda: s.process_device_masked(d_in.data_ptr(), F16, W, H, 4, d_out.data_ptr(), F16, [1] * NT))         # planar with c == 4
    refused(lambda: s.process_device_masked((d_in.data_ptr(), W * 3 - 1, 0), U8, W, H, 3, d_out.data_ptr(), U8, [1] * NT))  # pitch below a row
    s.out_ratio = Fraction(3, 2)
    refused(lambda: s.process_device_masked(d_in.data_ptr(), U8, W - 1, H, 3, d_out.data_ptr(), U8, [1] * NT))       # 69 * 3 / 2 is no pixel count
    s.out_ratio = 4
    # rsr_diff_tiles: format against c, an unknown format, an odd-width NV12, P010 at an odd address, a null mask; the mask stays as it was
    d_m = torch.full((NT,), 0xCD, dtype=torch.uint8, device="cuda")
    for args in ((F32, W, H, 4), (F16, W, H, 4), (3, W, H, 3), (NV12, W - 1, H, 3), (U8, W, H, 2), (U8, 0, H, 3)):
        refused(lambda: s.diff_tiles(d_in.data_ptr(), d_in.data_ptr(), args[0], args[1], args[2], args[3], d_m.data_ptr()))
    refused(lambda: s.diff_tiles(d_in.data_ptr(), d_in.data_ptr() + 1, P010, 34, 24, 3, d_m.data_ptr()))
    refused(lambda: s.diff_tiles(d_in.data_ptr(), (d_in.data_ptr(), 2 * 34 + 1, 0), P010, 34, 24, 3, d_m.data_ptr()))
    refused(lambda: s.diff_tiles(d_in.data_ptr(), d_in.data_ptr(), U8, W, H, 3, 0))
    torch.cuda.synchronize()
    assert bool((d_m == 0xCD).all())


def test_masked_calls_next_to_small_process_calls(ctx):
    s = ctx[False]
    x = image(42, U8)
    plain = call(s, x, U8, U8, None)
    smalls = [image(50 + i, U8, 24 + i, 20) for i in range(8)]
    wants = [s.process(im) for im in smalls]
    bad, masked = [], []

    def worker(i):
        try:
            for _ in range(4):
                if not np.array_equal(s.process(smalls[i]), wants[i]):
                    bad.append(i)
        except Exception as e:  # noqa: BLE001
            bad.append((i, repr(e)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for k in range(6):
        mask = MASKS[k % len(MASKS)]
        masked.append((mask, call(s, x, U8, U8, mask)))
    for t in threads:
        t.join()
    assert bad == []
    for mask, got in masked:
        assert same_bits(got, expected(s, U8, plain, mask)), mask
