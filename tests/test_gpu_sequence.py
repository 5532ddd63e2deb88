"""Frame sequences on the GPU (run with -m gpu): rsr_diff_tiles_sequence, rsr_process_device_sequence and torch_io.upscale_sequence.
Every comparison is EXACT.  A sequence call must leave, in every output rectangle, the bytes the plain call writes there for the frame
tests/sequence_ref.py names as the rectangle's source, or the bytes of the previous output; the diff must write, row by row, what
rsr_diff_tiles and tests/tile_diff_ref.py give for the pair.

The base case is that of tests/test_gpu_tile_mask.py: 70 x 50 at tile 32, prepadding 10, a 3 x 2 grid with partial last tiles, a folded
narrow last column and overlapping halos; n = 4 frames.  Outputs are pre-filled with 0xCD bytes (NaN for the float formats); the
previous output holds a pattern no network produces (negative floats, P010 words with their low bits set), so a rectangle of source -1
shows that it was copied verbatim."""
import ctypes as C
import threading
from fractions import Fraction

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

import sequence_ref
import tile_diff_ref as ref
from gpu_support import DIFF_FORMATS, context_fixtures, dev, out_dims, paths, profile_of  # noqa: F401
from pixfmt_ref import F16, F32, NP, NV12, P010, U8, image_at, paste, pattern, same_bits, sentinel, shape_of

pytestmark = pytest.mark.gpu
W, H, T, P = 70, 50, 32, 10
NT, N = 6, 4
CHECKER = [1, 0, 1, 0, 1, 0]
ZERO, ONE = [0] * NT, [1] * NT
# single tiles, a checkerboard, all zero, all one -- with a previous output (row 0 may have zeros) and without (row 0 all ones)
MASKS_PREV = [[0, 0, 0, 0, 1, 0], CHECKER, ZERO, ONE]
MASKS_PREV2 = [ZERO, [0, 1, 0, 0, 0, 0], [1 - m for m in CHECKER], [0, 0, 0, 0, 0, 7]]
MASKS_FIRST = [ONE, ZERO, [0, 0, 1, 0, 0, 0], [1 - m for m in CHECKER]]
SEQ_STATS = ("seq_calls", "seq_frames", "seq_tiles_run", "seq_tiles_copied", "seq_batches")
MASKED_STATS = ("masked_calls", "masked_tiles_run", "masked_tiles_skipped", "masked_batches")


ctxs, ctx = context_fixtures(T, P)
image = image_at(W, H)


def plain_call(s, x, in_fmt, out_fmt, w=W, h=H, c=3):
    """The plain n = 1 batch call on the packed numpy image x into a sentinel, synchronously."""
    ow, oh = out_dims(s, w, h)
    oshape = shape_of(out_fmt, ow, oh, c)
    d_in, d_out = dev(x), dev(sentinel(out_fmt, oshape))
    s.process_device_batch([d_in.data_ptr()], in_fmt, w, h, c, [d_out.data_ptr()], out_fmt)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(NP[out_fmt]).reshape(oshape)
    assert not same_bits(got, sentinel(out_fmt, oshape))
    return got


def seq_call(s, xs, in_fmt, out_fmt, masks, prev=None, w=W, h=H, c=3, in_place=False):
    """One synchronous sequence call on the packed numpy frames xs into sentinels.  prev: the numpy previous output (None: there is
    none); in_place: it IS out[0].  Returns the numpy outputs; a separate previous output must come back unchanged."""
    ow, oh = out_dims(s, w, h)
    oshape = shape_of(out_fmt, ow, oh, c)
    d_ins = [dev(x) for x in xs]
    d_outs = [dev(sentinel(out_fmt, oshape)) for _ in xs]
    d_prev = None
    if prev is not None:
        d_prev = dev(prev)
        if in_place:
            d_outs[0] = d_prev
    s.process_device_sequence([d.data_ptr() for d in d_ins], in_fmt, w, h, c, [d.data_ptr() for d in d_outs], out_fmt, np.asarray(masks, dtype=np.uint8),
                              prev_out=d_prev.data_ptr() if d_prev is not None else None)
    torch.cuda.synchronize()
    if prev is not None and not in_place:
        assert same_bits(d_prev.cpu().numpy().view(NP[out_fmt]).reshape(oshape), prev)
    return [d.cpu().numpy().view(NP[out_fmt]).reshape(oshape) for d in d_outs]


def expected(s, fmt, plains, masks, prev, w=W, h=H):
    """What a sequence call must leave in every output: rectangle t of frame k from the plain result of frame src[k][t], or from prev."""
    masks = np.asarray(masks).reshape(len(plains), -1)
    src = sequence_ref.sources(masks, prev is not None)
    r = s.out_ratio
    outs = []
    for k in range(len(plains)):
        e = sentinel(fmt, plains[0].shape)
        for t in range(masks.shape[1]):
            paste(fmt, e, prev if src[k, t] < 0 else plains[src[k, t]], ref.out_rect(w, h, s.tilesize, t, r.numerator, r.denominator))
        outs.append(e)
    return outs


def all_same(got, want):
    return len(got) == len(want) and all(same_bits(g, w_) for g, w_ in zip(got, want))


# ---- 1. composition -----------------------------------------------------------------------------------------------------------------------
# (id, in_fmt, out_fmt, c, yuv_siting, takes ratio 3/2)
FORMATS = [("u8c3", U8, U8, 3, 0, True), ("u8c4", U8, U8, 4, 0, False), ("f16", F16, F16, 3, 0, True), ("f32", F32, F32, 3, 0, False),
           ("nv12-s0", NV12, NV12, 3, 0, False), ("nv12-s1", NV12, NV12, 3, 1, False), ("nv12-s2", NV12, NV12, 3, 2, False),
           ("p010-s0", P010, P010, 3, 0, False), ("p010-s1", P010, P010, 3, 1, False), ("p010-s2", P010, P010, 3, 2, False),
           ("nv12-f16", NV12, F16, 3, 0, False), ("u8-nv12", U8, NV12, 3, 0, False)]


@pytest.mark.parametrize("fmtcase", FORMATS, ids=[f[0] for f in FORMATS])
@pytest.mark.parametrize("mode", ["default", "tta", "precise", "bgr"])
def test_every_rectangle_comes_from_its_source(ctx, mode, fmtcase):
    _, in_fmt, out_fmt, c, siting, ratio = fmtcase
    s = ctx[mode == "tta"]
    s.set_option("precise", int(mode == "precise"))
    s.set_option("bgr", int(mode == "bgr"))
    s.set_option("yuv_siting", siting)
    xs = [image(60 + k, in_fmt, c=c) for k in range(N)]
    for scale in [4, 2, 1] + ([Fraction(3, 2)] if ratio else []):
        s.out_ratio = scale
        assert out_dims(s, W, H) == ((105, 75) if scale == Fraction(3, 2) else (W * scale, H * scale))
        plains = [plain_call(s, x, in_fmt, out_fmt, c=c) for x in xs]
        prev = pattern(out_fmt, plains[0].shape)
        for masks, pv in ((MASKS_PREV, prev), (MASKS_PREV2, prev), (MASKS_FIRST, None), (MASKS_FIRST, prev)):
            got = seq_call(s, xs, in_fmt, out_fmt, masks, prev=pv, c=c)
            assert all_same(got, expected(s, out_fmt, plains, masks, pv)), (scale, masks)


# ---- 2. the diff --------------------------------------------------------------------------------------------------------------------------
def poke(fmt, x, px, py, ch=0, chroma=None, h=H):
    """x with ONE sample changed by one bit: luma / element (px, py) of channel ch, or, chroma = 0 / 1, the U / V of chroma pair (px, py)."""
    y = x.copy()
    v = y.view(np.uint8) if fmt == NV12 else (y.view(np.uint16) if fmt in (F16, P010) else (y.view(np.uint32) if fmt == F32 else y))
    if fmt == U8:
        v[py, px, ch] ^= 1
    elif fmt in (F16, F32):
        v[ch, py, px] ^= 1
    elif chroma is None:
        v[py, px] ^= 1
    else:
        v[h + py, 2 * px + chroma] ^= 1
    return y


def placed(b, fmt, w, h, c, off, row, plane):
    """The numpy image b on the device inside a larger allocation of random bytes: (tensor, descriptor)."""
    rowbytes = w * b.dtype.itemsize * (c if fmt == U8 else 1)
    host = np.random.default_rng(3).integers(0, 256, size=off + R.image_span(fmt, w, h, c, row, plane) + 64, dtype=np.uint8)
    raw = np.ascontiguousarray(b).view(np.uint8).reshape(-1, rowbytes)  # rows of every plane, in order
    if fmt == U8:
        starts = [off + y * row for y in range(h)]
    elif fmt in (F16, F32):
        starts = [off + q * plane + y * row for q in range(3) for y in range(h)]
    else:
        starts = [off + y * row for y in range(h)] + [off + plane + y * row for y in range(h // 2)]
    for r_, st in zip(raw, starts):
        host[st:st + rowbytes] = r_
    d = torch.from_numpy(host).cuda()
    return d, (d.data_ptr() + off, row, plane)


def video(fmt, seed, n, c=3):
    """n + 1 frames: frame 0 random, every next one the one before with one sample poked -- alternately in the interior of a tile (one
    tile changes) and in a halo that two or four tiles share; for a surface every third poke is chroma-only.  Frames 6 and 7 are equal."""
    spots = [(5, 5), (41, 5), (60, 45), (30, 30), (22, 41), (69, 0), None, (10, 40), (53, 20), (41, 41)]
    frames = [image(seed, fmt, c=c)]
    for k in range(n):
        sp = spots[k % len(spots)]
        if sp is None:
            frames.append(frames[-1].copy())
        elif fmt in (NV12, P010) and k % 3 == 2:
            frames.append(poke(fmt, frames[-1], sp[0] // 2, sp[1] // 2, chroma=k % 2))
        else:
            frames.append(poke(fmt, frames[-1], sp[0], sp[1], ch=(c - 1 if fmt == U8 else k % 3)))
    return frames


@pytest.mark.parametrize("name,fmt,c", DIFF_FORMATS, ids=[f[0] for f in DIFF_FORMATS])
def test_diff_rows_equal_the_reference_and_the_single_diff(ctx, name, fmt, c):
    s = ctx[False]
    frames = video(fmt, 70, 8, c=c)  # frames[0] serves as prev
    want = [ref.diff_mask(fmt, frames[k], frames[k + 1], T, P) for k in range(8)]
    counts = [int(m.sum()) for m in want]
    assert 0 in counts and 1 in counts and max(counts) >= 2, counts  # an unchanged frame, interior pokes, halo pokes
    es = frames[0].dtype.itemsize
    rowbytes = W * es * (c if fmt == U8 else 1)
    # packed operands, then pitched ones at offsets that agree with their neighbours modulo 16, modulo 4 only, and (bytes) not at all
    layouts = [None, (16, 32), (4, 12), (8 if es == 4 else 2, 4 if es == 4 else 6)] + ([(3, 7), (1, 0)] if es == 1 else [])
    keep, descs = [], []
    for k, f in enumerate(frames):
        lay = layouts[k % len(layouts)]
        if lay is None:
            d = dev(f)
            keep.append(d), descs.append(d.data_ptr())
        else:
            row = rowbytes + lay[1]
            d, desc = placed(f, fmt, W, H, c, lay[0], row, (H + 3) * row if fmt != U8 else 0)
            keep.append(d), descs.append(desc)
    for with_prev in (True, False):
        d_m = torch.full((8 * NT + 16,), 0xCD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # (the fill runs on torch's null stream, the diff on the context's non-blocking one: without this wait the fill may land behind the diff's memset)
        s.diff_tiles_sequence(descs[1:], descs[0] if with_prev else None, fmt, W, H, c, d_m.data_ptr())
        got = d_m.cpu().numpy()
        assert (got[8 * NT:] == 0xCD).all()
        got = got[:8 * NT].reshape(8, NT)
        assert got[0].tolist() == (want[0].tolist() if with_prev else ONE)
        for k in range(1, 8):
            assert got[k].tolist() == want[k].tolist(), (with_prev, k)
    # ... and what rsr_diff_tiles writes for every pair
    for k in range(8):
        d_1 = torch.full((NT,), 0xCD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        s.diff_tiles(descs[k], descs[k + 1], fmt, W, H, c, d_1.data_ptr())
        assert d_1.cpu().numpy().tolist() == want[k].tolist(), k
    # sixteen pairs in one launch
    d_m = torch.full((16 * NT,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s.diff_tiles_sequence([descs[1 + k % 8] for k in range(16)], None, fmt, W, H, c, d_m.data_ptr())
    got = d_m.cpu().numpy().reshape(16, NT)
    assert got[0].tolist() == ONE and got[8].tolist() == ref.diff_mask(fmt, frames[8], frames[1], T, P).tolist()
    assert all(got[k].tolist() == want[k % 8].tolist() for k in range(1, 16) if k != 8)


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------------------
SOUND = [("u8", U8, 0), ("f16", F16, 0), ("nv12-s1", NV12, 1)]


@pytest.mark.parametrize("name,fmt,siting", SOUND, ids=[f[0] for f in SOUND])
def test_upscale_sequence_equals_upscale_of_every_frame(ctx, name, fmt, siting):
    s = ctx[False]
    s.set_option("yuv_siting", siting)
    up = torch_io.upscale_yuv if fmt == NV12 else torch_io.upscale
    frames = video(fmt, 80, 18)  # 19 frames: two windows
    masks = [ref.diff_mask(fmt, frames[k], frames[k + 1], T, P) for k in range(18)]
    counts = [int(m.sum()) for m in masks]
    assert 0 in counts and 1 in counts and max(counts) >= 2
    ts = [torch.from_numpy(f).cuda() for f in frames]
    wants = [up(s, t) for t in ts]
    torch.cuda.synchronize()
    assert torch.cuda.current_stream().cuda_stream == 0  # (the null stream: the work goes through the side stream)

    def check(ys, lo=0):
        torch.cuda.synchronize()
        for k, y in enumerate(ys):
            assert torch.equal(y.view(torch.uint8), wants[lo + k].view(torch.uint8)), k

    if fmt == NV12:
        ys, n = torch_io.upscale_sequence(s, ts)  # (surfaces come as a list)
        assert isinstance(ys, list)
    else:
        ys, n = torch_io.upscale_sequence(s, torch.stack(ts))
        assert isinstance(ys, torch.Tensor) and ys.shape[0] == 19
    check(ys)
    assert len(ys) == 19 and n == NT + sum(counts)
    # a list, on a stream of the caller's
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ys, n = torch_io.upscale_sequence(s, ts)
    side.synchronize()
    check(ys)
    assert isinstance(ys, list) and n == NT + sum(counts)
    # prev_x / prev_y rolling from call to call, each call two windows wide or less; out= given
    before = s.get_stat("seq_calls")
    outs = [torch.zeros_like(wants[0]) for _ in range(17)]
    ya, na = torch_io.upscale_sequence(s, ts[1:18], prev_x=ts[0], prev_y=wants[0], out=outs)
    assert ya is outs and len(ya) == 17 and na == sum(counts[:17])
    check(ya, 1)
    yb, nb = torch_io.upscale_sequence(s, ts[18:], prev_x=ts[17], prev_y=ya[-1])
    assert len(yb) == 1 and nb == counts[17]
    check(yb, 18)
    assert s.get_stat("seq_calls") == before + 3
    if fmt == NV12:
        pairs = [(t[:H], t[H:]) for t in ts]
        yp, n = torch_io.upscale_sequence(s, pairs[1:5], prev_x=pairs[0], prev_y=(wants[0][:4 * H], wants[0][4 * H:]))
        torch.cuda.synchronize()
        assert n == sum(counts[:4])
        for k, (y, uv) in enumerate(yp):
            assert torch.equal(torch.cat([y, uv]), wants[1 + k]), k


# ---- 4. alignment of the copy ---------------------------------------------------------------------------------------------------------------
def test_copies_between_windows_at_different_alignments(ctx):
    """uint8 RGB windows of 840 bytes a row inside canvases of pitch 1001 bytes (no multiple of 3, 4 or 16), each starting at its own
    byte offset: out[0] and out[2] agree modulo 16, out[3] agrees with them modulo 4 only, out[1] and the previous output with nobody."""
    s = ctx[False]
    xs = [image(90 + k, U8) for k in range(N)]
    plains = [plain_call(s, x, U8, U8) for x in xs]
    prev = pattern(U8, plains[0].shape)
    pitch, rows = 1001, 4 * H + 6
    offs = [3 * pitch + 15, 3 * pitch + 16, 3 * pitch + 31, 3 * pitch + 19]
    off_prev = 3 * pitch + 5
    assert pitch % 3 and pitch % 4 and (offs[0] - offs[2]) % 16 == 0 and (offs[0] - offs[3]) % 16 and (offs[0] - offs[3]) % 4 == 0 and (offs[1] - offs[0]) % 4

    def canvas(img, off):
        cv = np.full(rows * pitch, 0xCD, dtype=np.uint8)
        if img is not None:
            for y in range(4 * H):
                cv[off + y * pitch:off + y * pitch + 4 * W * 3] = img[y].reshape(-1)
        return cv

    for masks in (MASKS_PREV, MASKS_PREV2, [ZERO] * N, MASKS_FIRST):
        d_ins = [dev(x) for x in xs]
        d_cv = [torch.from_numpy(canvas(None, 0)).cuda() for _ in range(N)]
        d_pv = torch.from_numpy(canvas(prev, off_prev)).cuda()
        s.process_device_sequence([d.data_ptr() for d in d_ins], U8, W, H, 3, [(d.data_ptr() + o, pitch, 0) for d, o in zip(d_cv, offs)], U8,
                                  np.asarray(masks, dtype=np.uint8), prev_out=(d_pv.data_ptr() + off_prev, pitch, 0))
        torch.cuda.synchronize()
        want = expected(s, U8, plains, masks, prev)
        for k in range(N):
            assert np.array_equal(d_cv[k].cpu().numpy(), canvas(want[k], offs[k])), (masks, k)  # the window, and sentinels all around it
        assert np.array_equal(d_pv.cpu().numpy(), canvas(prev, off_prev))


def test_copies_of_an_f16_ratio_window_at_an_odd_element_offset(ctx):
    s = ctx[False]
    s.out_ratio = Fraction(3, 2)
    xs = [image(95 + k, F16) for k in range(N)]
    plains = [plain_call(s, x, F16, F16) for x in xs]
    assert plains[0].shape == (3, 75, 105)
    prev = pattern(F16, plains[0].shape)
    ch, cw = 90, 131
    at = [(7, 3), (5, 4), (6, 11), (4, 8)]  # (row, column) of the window in its canvas: odd and even element offsets
    at_prev = (3, 6)

    def canvas(img, pos):
        cv = np.full((3, ch, cw), np.nan, dtype=np.float16)
        if img is not None:
            cv[:, pos[0]:pos[0] + 75, pos[1]:pos[1] + 105] = img
        return cv

    def desc(d, pos):
        return (d.data_ptr() + (pos[0] * cw + pos[1]) * 2, cw * 2, ch * cw * 2)

    for masks in (MASKS_PREV, MASKS_PREV2):
        d_ins = [dev(x) for x in xs]
        d_cv = [dev(canvas(None, None)) for _ in range(N)]
        d_pv = dev(canvas(prev, at_prev))
        s.process_device_sequence([d.data_ptr() for d in d_ins], F16, W, H, 3, [desc(d, p) for d, p in zip(d_cv, at)], F16, np.asarray(masks, dtype=np.uint8),
                                  prev_out=desc(d_pv, at_prev))
        torch.cuda.synchronize()
        want = expected(s, F16, plains, masks, prev)
        for k in range(N):
            assert same_bits(d_cv[k].cpu().numpy().view(np.float16).reshape(3, ch, cw), canvas(want[k], at[k])), (masks, k)


# ---- 5. several batches and n = 16 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_sixteen_frames_in_several_batches(ctx, tta):
    """A slot of the frame's largest tile, 52 x 52 padded pixels, is 16.4 MB of workspace: under a budget of 40 MB a batch takes two
    slots (under TTA one tile's eight, the least there is), so 16 frames with one tile set in each need 8 batches (16 under TTA)."""
    s = ctx[tta]
    xs = [image(100 + k, U8) for k in range(16)]
    plains = [plain_call(s, x, U8, U8) for x in xs]
    prev = pattern(U8, plains[0].shape)
    masks = [[int(t == k % NT) for t in range(NT)] for k in range(16)]
    s.set_option("max_workspace_mb", 40)
    before = {k: s.get_stat(k) for k in SEQ_STATS}
    got = seq_call(s, xs, U8, U8, masks, prev=prev)
    batches = s.get_stat("seq_batches") - before["seq_batches"]
    assert batches >= 3 and batches == (16 if tta else 8)
    assert all_same(got, expected(s, U8, plains, masks, prev))
    assert s.get_stat("seq_tiles_run") == before["seq_tiles_run"] + 16 and s.get_stat("seq_tiles_copied") == before["seq_tiles_copied"] + 16 * NT - 16
    assert s.get_stat("seq_frames") == before["seq_frames"] + 16
    s.set_option("max_workspace_mb", 65536)
    assert same_bits(plain_call(s, xs[0], U8, U8), plains[0]) and s.get_stat("ws_clamp_mb") == -1


def test_a_refused_workspace_halves_this_call_and_leaves_no_clamp(ctx):
    """Test hook ws_fail_above_mb: four set tiles want 4 slots of 16.4 MB; workspaces above 40 MB are refused, so the call halves its
    batches to two slots, runs, and plants no ws_clamp for later calls.  With every workspace refused the call fails with RSR_E_NOMEM,
    writes nothing and counts nothing."""
    s = ctx[False]
    xs = [image(110 + k, U8) for k in range(2)]
    plains = [plain_call(s, x, U8, U8) for x in xs]
    prev = pattern(U8, plains[0].shape)
    masks = [[1, 1, 0, 0, 0, 0], [0, 0, 0, 1, 1, 0]]
    keys = SEQ_STATS + ("ws_failures",)
    try:
        s.set_option("ws_fail_above_mb", 40)
        before = {k: s.get_stat(k) for k in keys}
        got = seq_call(s, xs, U8, U8, masks, prev=prev)
        assert all_same(got, expected(s, U8, plains, masks, prev))
        assert s.get_stat("ws_failures") == before["ws_failures"] + 1 and s.get_stat("seq_batches") == before["seq_batches"] + 2
        assert s.get_stat("ws_clamp_mb") == -1
        assert s.get_stat("seq_calls") == before["seq_calls"] + 1 and s.get_stat("seq_tiles_run") == before["seq_tiles_run"] + 4
        s.set_option("ws_fail_above_mb", 0)
        before = {k: s.get_stat(k) for k in keys}
        d_ins = [dev(x) for x in xs]
        d_outs = [torch.full((16 * W * H * 3,), 0xCD, dtype=torch.uint8, device="cuda") for _ in xs]
        d_prev = dev(prev)
        with pytest.raises(R.RealSRError) as e:
            s.process_device_sequence([d.data_ptr() for d in d_ins], U8, W, H, 3, [d.data_ptr() for d in d_outs], U8, np.asarray(masks, dtype=np.uint8),
                                      prev_out=d_prev.data_ptr())
        torch.cuda.synchronize()
        assert e.value.code == R.RSR_E_NOMEM and all(bool((d == 0xCD).all()) for d in d_outs) and s.get_stat("ws_clamp_mb") == -1
        for k in SEQ_STATS:
            assert s.get_stat(k) == before[k], k
    finally:
        s.set_option("ws_fail_above_mb", -1)
    assert same_bits(plain_call(s, xs[0], U8, U8), plains[0]) and s.get_stat("plan_batches") == 1 and s.get_stat("ws_clamp_mb") == -1
    assert all_same(seq_call(s, xs, U8, U8, masks, prev=prev), expected(s, U8, plains, masks, prev))


# ---- 6. in place and the degenerate cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_in_place_degenerate_cases_stats_and_progress(ctx, tta):
    s = ctx[tta]
    per = 8 if tta else 1
    xs = [image(120 + k, U8) for k in range(N)]
    plains = [plain_call(s, x, U8, U8) for x in xs]
    prev = pattern(U8, plains[0].shape)
    before = {k: s.get_stat(k) for k in SEQ_STATS + MASKED_STATS + ("batch_calls",)}
    # the previous output IS out[0]: frame 0 is updated in place, the later frames still read its untouched rectangles
    for masks in (MASKS_PREV, MASKS_PREV2):
        got = seq_call(s, xs, U8, U8, masks, prev=prev, in_place=True)
        assert all_same(got, expected(s, U8, plains, masks, prev)), masks
    run = sum(1 for m in MASKS_PREV + MASKS_PREV2 for v in m if v)
    in_place_skipped = MASKS_PREV[0].count(0) + MASKS_PREV2[0].count(0)
    assert s.get_stat("seq_calls") == before["seq_calls"] + 2 and s.get_stat("seq_frames") == before["seq_frames"] + 2 * N
    assert s.get_stat("seq_tiles_run") == before["seq_tiles_run"] + run
    assert s.get_stat("seq_tiles_copied") == before["seq_tiles_copied"] + 2 * N * NT - run - in_place_skipped
    assert s.get_stat("seq_batches") == before["seq_batches"] + 2 and s.get_stat("batch_calls") == before["batch_calls"] + 2
    # n = 1 in place is the masked call: the same rectangles written, every other byte untouched
    d_in, d_out = dev(xs[0]), dev(prev)
    s.process_device_masked(d_in.data_ptr(), U8, W, H, 3, d_out.data_ptr(), U8, CHECKER)
    torch.cuda.synchronize()
    masked = d_out.cpu().numpy().reshape(prev.shape)
    (got,), p = profile_of(s, lambda: seq_call(s, xs[:1], U8, U8, [CHECKER], prev=prev, in_place=True))
    assert same_bits(got, masked) and same_bits(got, expected(s, U8, plains[:1], [CHECKER], prev)[0])
    assert p["conv_launches"] == R.NUM_CONVS and p["calls"] == 1 and p["tiles"] == 3 * per
    # n = 1, not in place: the masked rectangles plus a copy of all the others
    (got,), p = profile_of(s, lambda: seq_call(s, xs[:1], U8, U8, [CHECKER], prev=prev))
    assert same_bits(got, masked) and p["conv_launches"] == R.NUM_CONVS and p["calls"] == 1
    # no tile set anywhere: only the copy launch runs ...
    got, p = profile_of(s, lambda: seq_call(s, xs, U8, U8, [ZERO] * N, prev=prev))
    assert all(same_bits(g, prev) for g in got) and p["conv_launches"] == 0 and p["tiles"] == 0 and p["calls"] == 1
    # ... and with n = 1 in place nothing at all is launched
    calls = s.get_stat("batch_calls")
    (got,), p = profile_of(s, lambda: seq_call(s, xs[:1], U8, U8, [ZERO], prev=prev, in_place=True))
    assert same_bits(got, prev) and p["conv_launches"] == 0 and p["tiles"] == 0 and p["calls"] == 0 and p["total_ms"] == 0
    assert s.get_stat("batch_calls") == calls
    assert s.get_stat("seq_calls") == before["seq_calls"] + 6
    for k in MASKED_STATS:
        assert s.get_stat(k) == before[k] + (1 if k == "masked_calls" else (3 if k in ("masked_tiles_run", "masked_tiles_skipped") else 1)), k
    # progress: one callback per computed tile
    seen = []
    cb = C.CFUNCTYPE(None, C.c_int, C.c_int, C.c_void_p)(lambda done, total, user: seen.append((done, total)))
    L = R.lib()
    assert L.rsr_set_progress_callback(s._h, C.cast(cb, C.c_void_p), None) == 0
    try:
        seq_call(s, xs, U8, U8, MASKS_PREV2, prev=prev)
    finally:
        assert L.rsr_set_progress_callback(s._h, None, None) == 0
    assert seen == [(i, 5) for i in range(1, 6)]


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_every_output_untouched(ctx):
    s = ctx[False]
    xs = [image(130 + k, U8) for k in range(17)]
    d_ins = [dev(x) for x in xs]
    d_outs = [torch.full((16 * W * H * 3,), 0xCD, dtype=torch.uint8, device="cuda") for _ in xs]
    d_prev = torch.full((16 * W * H * 3,), 0xCD, dtype=torch.uint8, device="cuda")
    ins, outs = [d.data_ptr() for d in d_ins], [d.data_ptr() for d in d_outs]
    before = {k: s.get_stat(k) for k in SEQ_STATS}

    def refused(fn):
        with pytest.raises(R.RealSRError) as e:
            fn()
        assert e.value.code == R.RSR_E_ARG
        torch.cuda.synchronize()
        assert all(bool((d == 0xCD).all()) for d in d_outs + [d_prev])

    def seq(n, masks, prev=d_prev.data_ptr(), in_fmt=U8, out_fmt=U8, w=W, h=H, c=3, ins_=None, outs_=None):
        return lambda: s.process_device_sequence((ins_ or ins)[:n], in_fmt, w, h, c, (outs_ or outs)[:n], out_fmt, masks, prev_out=prev)

    refused(seq(17, [1] * (17 * NT)))                                    # n beyond RSR_SEQ_MAX
    refused(seq(0, [1] * NT))                                            # no frame at all
    refused(seq(4, [1] * (4 * NT - 1)))                                  # nmask != n * nx * ny
    refused(seq(4, [1] * (4 * NT + 1)))
    refused(seq(4, [1] * (3 * NT)))
    refused(seq(4, None))                                                # a null mask
    refused(seq(4, (0, 4 * NT)))
    refused(seq(4, [1] * NT + [0] * (3 * NT), ins_=ins[:3] + [0]))        # a null data pointer
    refused(seq(4, [1] * NT + [0] * (3 * NT), outs_=outs[:2] + [0, outs[3]]))
    refused(seq(4, [1, 1, 1, 1, 1, 0] + [1] * (3 * NT), prev=None))       # row 0 has a zero byte and there is no previous output
    refused(seq(4, [0] * (4 * NT), prev=None))
    refused(seq(4, [0] * (4 * NT), prev=(d_prev.data_ptr(), 4 * W * 3 - 1, 0)))  # the previous output fails the checks of an output image
    refused(seq(4, [0] * (4 * NT), prev=(0, 0, 0)))
    refused(seq(4, [1] * (4 * NT), out_fmt=F16, prev=d_prev.data_ptr() + 1))     # ... its alignment to the element included
    refused(seq(4, [1] * (4 * NT), in_fmt=NV12, out_fmt=NV12, w=W - 1))          # everything the batch call refuses: an odd-width NV12,
    refused(seq(4, [1] * (4 * NT), in_fmt=F16, out_fmt=F16, c=4))                # planar with c == 4,
    refused(seq(4, [1] * (4 * NT), ins_=[(ins[0], W * 3 - 1, 0)] + ins[1:]))     # a pitch below a row,
    s.out_ratio = Fraction(3, 2)
    refused(seq(4, [1] * (4 * NT), w=W - 1))                                     # 69 * 3 / 2 is no pixel count,
    refused(seq(4, [1] * (4 * NT), in_fmt=NV12, out_fmt=NV12))                   # a YUV output at ratio 3 / 2
    refused(seq(4, [1] * (4 * NT), out_fmt=NV12))
    s.out_ratio = 4
    for k in SEQ_STATS:
        assert s.get_stat(k) == before[k], k
    # rsr_diff_tiles_sequence: n, null pointers, and for every descriptor what rsr_diff_tiles refuses; the masks stay as they were
    d_m = torch.full((17 * NT,), 0xCD, dtype=torch.uint8, device="cuda")
    refused(lambda: s.diff_tiles_sequence(ins[:17], None, U8, W, H, 3, d_m.data_ptr()))
    refused(lambda: s.diff_tiles_sequence([], None, U8, W, H, 3, d_m.data_ptr()))
    refused(lambda: s.diff_tiles_sequence(ins[:4], None, U8, W, H, 3, 0))
    refused(lambda: s.diff_tiles_sequence(ins[:3] + [0], None, U8, W, H, 3, d_m.data_ptr()))
    refused(lambda: s.diff_tiles_sequence(ins[:4], 0, U8, W, H, 3, d_m.data_ptr()))
    for args in ((F32, W, H, 4), (3, W, H, 3), (NV12, W - 1, H, 3), (U8, W, H, 2), (U8, 0, H, 3)):
        refused(lambda: s.diff_tiles_sequence(ins[:4], ins[4], args[0], args[1], args[2], args[3], d_m.data_ptr()))
    refused(lambda: s.diff_tiles_sequence(ins[:2] + [ins[2] + 1], None, P010, 34, 24, 3, d_m.data_ptr()))
    refused(lambda: s.diff_tiles_sequence(ins[:2], (ins[2], 2 * 34 + 1, 0), P010, 34, 24, 3, d_m.data_ptr()))
    torch.cuda.synchronize()
    assert bool((d_m == 0xCD).all())


# ---- 8. next to other calls -------------------------------------------------------------------------------------------------------------------
def test_sequence_calls_on_a_user_stream_next_to_small_process_calls(ctx):
    s = ctx[False]
    xs = [image(140 + k, U8) for k in range(N)]
    plains = [plain_call(s, x, U8, U8) for x in xs]
    prev = pattern(U8, plains[0].shape)
    smalls = [image(150 + i, U8, 24 + i, 20) for i in range(8)]
    wants = [s.process(im) for im in smalls]
    bad, results = [], []

    def worker(i):
        try:
            for _ in range(4):
                if not np.array_equal(s.process(smalls[i]), wants[i]):
                    bad.append(i)
        except Exception as e:  # noqa: BLE001
            bad.append((i, repr(e)))

    st = torch.cuda.Stream()
    d_ins = [dev(x) for x in xs]
    d_prev = dev(prev)
    torch.cuda.synchronize()
    threads = [threading.Thread(target=worker, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for k in range(6):
        masks = (MASKS_PREV, MASKS_PREV2, MASKS_FIRST)[k % 3]
        with torch.cuda.stream(st):
            d_outs = [dev(sentinel(U8, plains[0].shape)) for _ in xs]
            s.process_device_sequence([d.data_ptr() for d in d_ins], U8, W, H, 3, [d.data_ptr() for d in d_outs], U8, np.asarray(masks, dtype=np.uint8),
                                      prev_out=d_prev.data_ptr(), stream=st.cuda_stream)
        results.append((masks, d_outs))
    for t in threads:
        t.join()
    st.synchronize()
    torch.cuda.synchronize()
    assert bad == []
    for masks, d_outs in results:
        got = [d.cpu().numpy().reshape(plains[0].shape) for d in d_outs]
        assert all_same(got, expected(s, U8, plains, masks, prev)), masks
