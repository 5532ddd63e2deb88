"""NV16 / P210 device images on the GPU (run with -m gpu): RSR_FMT_NV16 / RSR_FMT_P210 -- YUV 4:2:2, chroma halved horizontally only -- on
either side of every device entry point that takes NV12 / P010, and torch_io's chroma=422.

Everything here is EXACT, no tolerance anywhere: np.array_equal on bytes against tests/yuv422_ref.py, the numpy float32 restatement of
"YUV 4:2:2" in include/realsr_hip.h, tied to the planar fp32 format of the same context as tests/test_gpu_yuv.py ties NV12 / P010:

    input side    yuv -> f32  ==  f32 -> f32 with x = yuv422_ref.decode(surface)
    output side   x -> yuv    ==  yuv422_ref.encode(x -> f32)
    end to end    yuv -> yuv  ==  yuv422_ref.encode(f32 -> f32 with x = yuv422_ref.decode(surface))

Destinations are pre-filled with 0xCD.  The baseline image is 36 x 25 at tile 16, prepadding 10: 3 x 2 tiles, partial tiles on both
edges, an odd height (no 4:2:0 surface has one), reflect halos wider than a chroma sample."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

import tile_diff_ref as ref
import yuv422_ref
import yuv_ref
import yuv_siting_ref
from gpu_support import context_fixtures, dev, paths, run  # noqa: F401
from pixfmt_ref import BITS, F16, F32, NP, NV12, NV16, P210, U8, image_at, lift, paste, place, same_bits

pytestmark = pytest.mark.gpu
W, H, T, P = 36, 25, 16, 10
CFGS = [(709, 0), (601, 1), (2020, 0), (709, 1), (601, 0), (2020, 1)]  # (yuv_matrix, yuv_range)
SENTINEL = 0xCD
ctxs, ctx = context_fixtures(T, P)
surface = rgb_image = image_at(W, H)


def set_cfg(s, cfg):
    s.set_option("yuv_matrix", cfg[0])
    s.set_option("yuv_range", cfg[1])


def want422(d, fmt, cfg=(709, 0), siting=0, tile_w=0):
    return yuv422_ref.join(*yuv422_ref.encode(d, cfg[0], cfg[1], BITS[fmt], siting, tile_w), BITS[fmt])


# ---- 1. input tie ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [NV16, P210], ids=["nv16", "p210"])
@pytest.mark.parametrize("mode", ["default", "tta", "precise"])
def test_input_tie(ctx, mode, fmt):
    s = ctx[mode == "tta"]
    s.set_option("precise", int(mode == "precise"))
    surf = surface(11 + fmt, fmt)
    y, uv = yuv422_ref.split(surf, BITS[fmt])
    seen = []
    for cfg in CFGS:
        set_cfg(s, cfg)
        per_siting = []
        for siting in (0, 1, 2):
            s.yuv_siting = siting
            ref = yuv422_ref.decode(y, uv, cfg[0], cfg[1], BITS[fmt], siting)
            assert (ref == 0).any() and (ref == 1).any() and len(np.unique(ref)) > 100  # the clamp acts, and not everywhere
            got = run(s, surf, fmt, F32)
            assert got.shape == (3, 4 * H, 4 * W) and not (got.view(np.uint8) == SENTINEL).all()
            assert same_bits(got, run(s, ref, F32, F32)), (cfg, siting)
            per_siting.append(got)
        assert same_bits(per_siting[2], per_siting[1]) and not np.array_equal(per_siting[0], per_siting[1])  # top-left IS left here
        seen.append(per_siting[0])
    assert not any(np.array_equal(seen[i], seen[j]) for i in range(len(seen)) for j in range(i))  # every matrix and range is a different image


# ---- 2. output tie -----------------------------------------------------------------------------------------------------------------
CASES = [(tta, precise, os_) for tta in (False, True) for precise in (0, 1) for os_ in (4, 2, 1)]


@pytest.mark.parametrize("case", range(len(CASES)), ids=["%s-%s-x%d" % ("tta" if t else "plain", "precise" if p else "fp16", o) for t, p, o in CASES])
def test_output_tie(ctx, case):
    """out_scale 4 / 2 / 1 (tile 16 is even), sitings 0 / 1 / 2: 36 x 25 gives 144 x 100, 72 x 50 and 36 x 25 -- an odd number of rows."""
    tta, precise, os_ = CASES[case]
    s = ctx[tta]
    s.set_option("precise", precise)
    s.out_scale = os_
    for src in (U8, F16):
        x = rgb_image(20 + case + src, src)
        s.yuv_siting = 0
        d = run(s, x, src, F32)
        assert d.shape == (3, H * os_, W * os_) and np.isfinite(d).all() and len(np.unique(d)) > 16
        for fmt in (NV16, P210):
            cfg = CFGS[(case + fmt + src) % 6]
            set_cfg(s, cfg)
            outs = []
            for siting in (0, 1, 2):
                s.yuv_siting = siting
                want = want422(d, fmt, cfg, siting, T * os_)
                assert want.shape == (2 * H * os_, W * os_) and len(np.unique(want)) > 16  # an image, not a constant
                outs.append(run(s, x, src, fmt))
                assert same_bits(outs[-1], want), (src, fmt, cfg, siting)
            assert same_bits(outs[2], outs[1])
            # the clamp at tile-first columns shows: the unclamped [1 2 1] filter gives another sample somewhere, and only in those columns
            free = want422(d, fmt, cfg, 1, 0)
            differ = np.argwhere(free != outs[1])
            assert len(differ) > 0 and (differ[:, 0] >= H * os_).all() and (differ[:, 1] // 2 * 2 % (T * os_) == 0).all() and (differ[:, 1] > 0).all()


@pytest.mark.parametrize("tta,precise", [(False, 0), (True, 0), (False, 1)], ids=["plain", "tta", "precise"])
def test_output_tie_at_3_2(ctx, tta, precise):
    """36 x 26 at 3/2 and tile 16: 54 x 39 -- an odd output height and tile rectangles of 24 x 24 whose last row of tiles has 15 rows; NV12
    refuses it, a 4:2:2 surface takes it."""
    s = ctx[tta]
    s.set_option("precise", precise)
    s.out_ratio = Fraction(3, 2)
    assert s.out_size_fmt(NV16, 36, 26) == (54, 39) == s.out_size_fmt(F32, 36, 26)
    with pytest.raises(ValueError, match="YUV"):
        s.out_size_fmt(NV12, 36, 26)
    x = rgb_image(300 + tta, U8, 36, 26)
    with pytest.raises(R.RealSRError):
        run_into(s, x, U8, NV12, 36, 26, 54 * 40 * 2)
    d = run(s, x, U8, F32, 36, 26)
    assert d.shape == (3, 39, 54)
    for fmt in (NV16, P210):
        for siting in (0, 1):
            s.yuv_siting = siting
            got = run(s, x, U8, fmt, 36, 26)
            assert same_bits(got, want422(d, fmt, (709, 0), siting, 24)), (fmt, siting)
        assert not same_bits(got, want422(d, fmt, (709, 0), 1, 0))  # (the clamp at columns 24 and 48 shows)


def run_into(s, x, in_fmt, out_fmt, w, h, nbytes):
    """A call that is expected to be refused: the destination must come back untouched."""
    d_in = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
    d_out = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    try:
        s.process_device_fmt(d_in.data_ptr(), in_fmt, w, h, 3, d_out.data_ptr(), out_fmt)
    finally:
        torch.cuda.synchronize()
        assert (d_out == SENTINEL).all()


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_output_tie_at_a_pair(ctx, tta):
    """48 x 28 at (8/3, 9/4) and tile 24: tile rectangles 64 x 54, output 128 x 63 -- odd rows, 5-tap footprints down the columns."""
    s = ctx[tta]
    s.tilesize = 24
    s.out_ratio_xy = (Fraction(8, 3), Fraction(9, 4))
    assert s.out_size_fmt(P210, 48, 28) == (128, 63)
    x = rgb_image(310, F16, 48, 28)
    d = run(s, x, F16, F32, 48, 28)
    assert d.shape == (3, 63, 128)
    for fmt, siting, cfg in ((NV16, 0, CFGS[1]), (NV16, 1, CFGS[2]), (P210, 2, CFGS[3]), (P210, 0, CFGS[4])):
        s.yuv_siting = siting
        set_cfg(s, cfg)
        assert same_bits(run(s, x, F16, fmt, 48, 28), want422(d, fmt, cfg, siting, 64)), (fmt, siting)


# ---- 3. end to end, cross-format ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tta,precise,os_,siting", [(False, 0, 4, 0), (True, 0, 2, 1), (False, 1, 1, 2)], ids=["plain-x4", "tta-x2-left", "precise-x1-topleft"])
def test_end_to_end_and_cross_format(ctx, tta, precise, os_, siting):
    s = ctx[tta]
    s.set_option("precise", precise)
    s.out_scale = os_
    s.yuv_siting = siting
    cfg = CFGS[os_ % 6]
    set_cfg(s, cfg)
    for fmt in (NV16, P210):
        surf = surface(60 + fmt, fmt)
        d = run(s, yuv422_ref.decode(*yuv422_ref.split(surf, BITS[fmt]), cfg[0], cfg[1], BITS[fmt], siting), F32, F32)
        assert same_bits(run(s, surf, fmt, fmt), want422(d, fmt, cfg, siting, T * os_)), fmt
    # the two sides are independent.  NV16 -> NV12 needs an even height: 36 x 26
    surf = surface(70, NV16, 36, 26)
    d = run(s, yuv422_ref.decode(*yuv422_ref.split(surf, 8), cfg[0], cfg[1], 8, siting), F32, F32, 36, 26)
    want = yuv_ref.join(*yuv_siting_ref.encode(d, siting, T * os_, cfg[0], cfg[1], 8), 8)
    assert same_bits(run(s, surf, NV16, NV12, 36, 26), want)
    surf = surface(71, NV12, 36, 26)
    d = run(s, yuv_siting_ref.decode(*yuv_ref.split(surf, 8), siting, cfg[0], cfg[1], 8), F32, F32, 36, 26)
    assert same_bits(run(s, surf, NV12, P210, 36, 26), want422(d, P210, cfg, siting, T * os_))


# ---- 4. batches, masks, sequences -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [NV16, P210], ids=["nv16", "p210"])
@pytest.mark.parametrize("tta,os_", [(False, 4), (True, 2), (False, 1)], ids=["plain-x4", "tta-x2", "plain-x1"])
def test_batch_of_three_pitched_windows(ctx, tta, os_, fmt):
    """Three surfaces in ONE rsr_process_device_batch call, each inside a larger allocation (row pitch > w, UV plane farther than
    h * pitch behind Y, NV16 at odd addresses), each into a window of a sentinel-filled canvas: every window holds what the lone call
    gives, every other byte of the canvases its sentinel."""
    s = ctx[tta]
    s.out_scale = os_
    s.yuv_siting = 1
    es = NP[fmt]().itemsize
    surfs = [surface(70 + i, fmt) for i in range(3)]
    lone = [run(s, x, fmt, fmt) for x in surfs]
    ipitch, iplane, ioff = (W + 5) * es, (H + 3) * (W + 5) * es, 3 * es
    opitch, oplane, ooff = (W * os_ + 7) * es, (H * os_ + 2) * (W * os_ + 7) * es + 6 * es, 5 * es
    ispan, ospan = R.image_span(fmt, W, H, 3, ipitch, iplane), R.image_span(fmt, W * os_, H * os_, 3, opitch, oplane)
    assert ospan == oplane + (H * os_ - 1) * opitch + W * os_ * es
    ins, outs, keep = [], [], []
    for x in surfs:
        canvas = np.full(ioff + ispan + 64, 0x5A, dtype=np.uint8)
        place(canvas, ioff, ipitch, iplane, x, fmt)
        d_in = torch.from_numpy(canvas).cuda()
        d_out = torch.full((ooff + ospan + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        keep.append((d_in, d_out))
        ins.append((d_in.data_ptr() + ioff, ipitch, iplane))
        outs.append((d_out.data_ptr() + ooff, opitch, oplane))
    calls = s.get_stat("batch_calls")
    s.process_device_batch(ins, fmt, W, H, 3, outs, fmt)
    torch.cuda.synchronize()
    assert s.get_stat("batch_calls") == calls + 1
    for (_, d_out), want in zip(keep, lone):
        got = d_out.cpu().numpy()
        assert same_bits(lift(got, ooff, opitch, oplane, fmt, W * os_, H * os_), want)
        inside = place(np.zeros_like(got), ooff, opitch, oplane, want, fmt)
        assert (got[~inside] == SENTINEL).all()  # no byte outside the Y and UV windows is touched
        assert inside.sum() == want.nbytes


@pytest.mark.parametrize("fmt,ratio", [(NV16, None), (P210, Fraction(3, 2))], ids=["nv16-x4", "p210-x3_2"])
def test_masked_tiles(ctx, fmt, ratio):
    """A partial mask: the marked tiles' rectangles hold the full call's bytes, the unmarked ones the sentinel -- Y and UV alike."""
    s = ctx[False]
    w, h = (W, H) if ratio is None else (36, 26)
    r = Fraction(4) if ratio is None else ratio
    if ratio is not None:
        s.out_ratio = ratio
    s.yuv_siting = 1
    surf = surface(90 + fmt, fmt, w, h)
    full = run(s, surf, fmt, fmt, w, h)
    nx, ny = s.tile_count(w, h)
    assert (nx, ny) == (3, 2)
    mask = np.array([1, 0, 1, 0, 1, 0], dtype=np.uint8)
    d_in, d_out = dev(surf), torch.full((full.nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    s.process_device_masked(d_in.data_ptr(), fmt, w, h, 3, d_out.data_ptr(), fmt, mask)
    torch.cuda.synchronize()
    want = np.full(full.shape, SENTINEL | (SENTINEL << 8) if BITS[fmt] == 10 else SENTINEL, dtype=NP[fmt])
    for t in np.flatnonzero(mask):
        paste(fmt, want, full, ref.out_rect(w, h, T, t, r.numerator, r.denominator))
    got = d_out.cpu().numpy().view(NP[fmt]).reshape(full.shape)
    assert same_bits(got, want) and not same_bits(got, full)


@pytest.mark.parametrize("fmt", [NV16, P210], ids=["nv16", "p210"])
def test_sequence_of_three_frames_with_prev_out(ctx, fmt):
    """Three frames and a previous output: a rectangle nobody computed is copied from the frame that computed it last or from prev_out --
    its Y rows and, in full, its UV rows (36 x 25: tile rows of 64 and 36 output rows)."""
    s = ctx[False]
    frames = [surface(100 + i + fmt, fmt) for i in range(3)]
    full = [run(s, x, fmt, fmt) for x in frames]
    prev = surface(110, fmt, 4 * W, 4 * H)
    masks = np.array([[1, 0, 0, 0, 1, 0],
                      [0, 1, 0, 0, 0, 0],
                      [0, 0, 0, 1, 1, 0]], dtype=np.uint8)
    d_ins = [dev(x) for x in frames]
    d_outs = [torch.full((full[0].nbytes,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in frames]
    d_prev = dev(prev)
    s.process_device_sequence([t.data_ptr() for t in d_ins], fmt, W, H, 3, [t.data_ptr() for t in d_outs], fmt, masks.reshape(-1), prev_out=d_prev.data_ptr())
    torch.cuda.synchronize()
    state = prev.copy()
    for k in range(3):
        for t in np.flatnonzero(masks[k]):
            paste(fmt, state, full[k], ref.out_rect(W, H, T, t))
        got = d_outs[k].cpu().numpy().view(NP[fmt]).reshape(full[k].shape)
        assert same_bits(got, state), k
    assert same_bits(d_prev.cpu().numpy().view(NP[fmt]).reshape(prev.shape), prev)


# ---- 5. the frame diff -------------------------------------------------------------------------------------------------------------
def flips(w, h):
    """(row of the (2h, w) surface, column) of single samples to change: in Y, in U and in V, each at a corner of a source rectangle, one
    chroma column beyond the rectangle's own and one more (not compared by that tile), and one row below / above it."""
    out = []
    for tile in (0, 4):
        x0, y0, x1, y1 = ref.source_rect(w, h, T, P, tile)
        c1 = min(((x1 - 1) >> 1) + 1, w // 2 - 1)
        out += [(y0, x0), (y1 - 1, x1 - 1)]
        if x1 < w:
            out += [(y1 - 1, x1), (y1 - 1, x1 + 1)]
        if y1 < h:
            out += [(y1, x0), (h + y1, 2 * c1), (h + y1, 2 * c1 + 1)]
        if y0 > 0:
            out += [(y0 - 1, x0), (h + y0 - 1, 2 * c1), (h + y0 - 1, 2 * c1 + 1)]
        for q in (0, 1):  # U, V
            out += [(h + y0, 2 * max((x0 >> 1) - 1, 0) + q), (h + y1 - 1, 2 * c1 + q)]
            if c1 + 1 < w // 2:
                out += [(h + y1 - 1, 2 * (c1 + 1) + q)]
    return out


@pytest.mark.parametrize("fmt", [NV16, P210], ids=["nv16", "p210"])
def test_diff_tiles_and_sequence(ctx, fmt):
    s = ctx[False]
    a = surface(120 + fmt, fmt)
    d_a = dev(a)
    nt = 6
    seen = set()
    pos = flips(W, H)
    assert len(pos) >= 16
    for i, (r, c) in enumerate(pos):
        b = a.copy()
        b[r, c] ^= 1 if (BITS[fmt] == 8 or i % 2) else 0x40  # (P210: a bit below the code differs as well -- whole words are compared)
        want = ref.diff_mask(fmt, a, b, T, P)
        d_mask = torch.full((nt,), SENTINEL, dtype=torch.uint8, device="cuda")
        s.diff_tiles(d_a.data_ptr(), dev(b).data_ptr(), fmt, W, H, 3, d_mask.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_mask.cpu().numpy(), want), (r, c, want)
        seen.add(tuple(want))
    assert len(seen) >= 4 and any(sum(m) == 1 for m in seen) and any(sum(m) > 1 for m in seen)
    # the sequence form: row k is the diff of the pair (frame k - 1, frame k), row 0 against prev; without a prev every tile of row 0 is set
    frames = [a.copy() for _ in range(3)]
    frames[1][pos[1]] ^= 1
    frames[2][pos[1]] ^= 1
    frames[2][pos[-1]] ^= 1
    d_f = [dev(x) for x in frames]
    for prev in (a, None):
        d_masks = torch.full((3 * nt,), SENTINEL, dtype=torch.uint8, device="cuda")
        s.diff_tiles_sequence([t.data_ptr() for t in d_f], d_a.data_ptr() if prev is not None else None, fmt, W, H, 3, d_masks.data_ptr())
        torch.cuda.synchronize()
        want = np.stack([ref.diff_mask(fmt, p, q, T, P) for p, q in zip([a] + frames[:2], frames)])
        if prev is None:
            want[0] = 1
        assert np.array_equal(d_masks.cpu().numpy().reshape(3, nt), want)
        assert want[1].any() and want[2].any()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_before_launch(ctx):
    s = ctx[False]
    buf = torch.full((1 << 18,), SENTINEL, dtype=torch.uint8, device="cuda")
    p, q = buf.data_ptr(), buf.data_ptr() + (1 << 17)

    def refused(*a, batch=False, yuv=False):
        with pytest.raises(R.RealSRError) as e:
            (s.process_device_batch if batch else s.process_device_fmt)(*a)
        assert e.value.code == R.RSR_E_ARG, a
        assert not yuv or "YUV" in str(e.value), str(e.value)

    for fmt in (NV16, P210):
        refused(p, fmt, 7, 8, 3, q, F16, yuv=True)                   # an odd w of a 4:2:2 input
        refused([p], fmt, 7, 8, 3, [q], F16, batch=True, yuv=True)
        refused(p, fmt, 8, 8, 4, q, U8)                              # c = 4
        refused(p, U8, 8, 8, 4, q, fmt)
    refused(p + 1, P210, 8, 8, 3, q, F16)                            # P210: an odd address, an odd pitch -- on either side
    refused(p, F16, 8, 8, 3, q + 1, P210)
    refused([(p + 1, 0, 0)], P210, 8, 8, 3, [q], F16, batch=True)
    refused([(p, 17, 0)], P210, 8, 8, 3, [q], F16, batch=True)
    refused([(p, 0, 8 * 16 + 1)], P210, 8, 8, 3, [q], F16, batch=True)
    refused([p], F16, 8, 8, 3, [(q, 65, 0)], P210, batch=True)
    s.tilesize = 30
    s.out_ratio = Fraction(3, 2)                                     # 3/2 at tile 30: 45 columns
    for fmt in (NV16, P210):
        refused(p, U8, 36, 26, 3, q, fmt, yuv=True)
        with pytest.raises(ValueError, match="YUV"):
            s.out_size_fmt(fmt, 36, 26)
    assert s.out_size_fmt(F32, 36, 26) == (54, 39)
    s.tilesize = 33
    s.out_scale = 1                                                  # out_scale 1 at tile 33
    for fmt in (NV16, P210):
        refused(p, U8, 36, 25, 3, q, fmt, yuv=True)
    s.tilesize = 16
    refused(p, U8, 35, 25, 3, q, NV16, yuv=True)                     # out_scale 1 and an odd width: no 4:2:2 surface of that size
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()                                   # nothing was launched
    s.out_scale = 4
    assert run(s, surface(130, NV16, 8, 5), NV16, NV16, 8, 5).shape == (40, 32)  # (the context is as usable as before; any h is taken)


# ---- 7. 64-bit addressing: a UV plane beyond 2^32 bytes ---------------------------------------------------------------------------------
FAR = (1 << 32) + (1 << 20) + 6  # plane pitch of the far surfaces (even: P210)
ARENA = (1 << 32) + (3 << 27)    # ~ 4.4 GiB, a whole number of 8-byte words


@pytest.fixture(scope="module")
def arena():
    a = torch.full((ARENA,), SENTINEL, dtype=torch.uint8, device="cuda")
    yield a
    del a
    torch.cuda.empty_cache()


def arena_clean(arena):
    words = arena.view(torch.int64)
    fill = int(np.array([SENTINEL] * 8, dtype=np.uint8).view(np.int64)[0])
    return int(words.min()) == fill and int(words.max()) == fill


@pytest.mark.parametrize("fmt", [NV16, P210], ids=["nv16", "p210"])
def test_far_uv_plane_on_either_side(ctx, arena, fmt):
    """The UV plane FAR > 2^32 bytes behind Y(0,0), inside one arena of 0xCD: as an input the call gives the packed call's bytes; as an
    output the two windows hold the packed call's bytes and the rest of the arena stays 0xCD (checked on the device)."""
    s = ctx[False]
    s.yuv_siting = 1
    es = NP[fmt]().itemsize
    assert ARENA % 8 == 0 and arena_clean(arena)
    # input side
    surf = surface(140 + fmt, fmt)
    want = run(s, surf, fmt, F32)
    off, pitch = 4096 + 2 * es, (W + 9) * es
    assert R.image_span(fmt, W, H, 3, pitch, FAR) == FAR + (H - 1) * pitch + W * es < ARENA - off
    rows = torch.from_numpy(surf.view(np.uint8).reshape(2 * H, -1)).cuda()
    for r in range(2 * H):
        o = off + r * pitch if r < H else off + FAR + (r - H) * pitch
        arena[o:o + W * es] = rows[r]
    d_out = torch.full((want.nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    s.process_device_batch([(arena.data_ptr() + off, pitch, FAR)], fmt, W, H, 3, [d_out.data_ptr()], F32)
    torch.cuda.synchronize()
    assert same_bits(d_out.cpu().numpy().view(np.float32).reshape(want.shape), want)
    for r in range(2 * H):
        o = off + r * pitch if r < H else off + FAR + (r - H) * pitch
        assert torch.equal(arena[o:o + W * es], rows[r])
        arena[o:o + W * es] = SENTINEL
    assert arena_clean(arena)
    # output side
    x = rgb_image(150 + fmt, U8)
    want = run(s, x, U8, fmt)
    ow, oh = 4 * W, 4 * H
    opitch = (ow + 11) * es
    assert R.image_span(fmt, ow, oh, 3, opitch, FAR) < ARENA - off
    s.process_device_batch([dev(x).data_ptr()], U8, W, H, 3, [(arena.data_ptr() + off, opitch, FAR)], fmt)
    torch.cuda.synchronize()
    wrows = torch.from_numpy(want.view(np.uint8).reshape(2 * oh, -1)).cuda()
    for r in range(2 * oh):
        o = off + r * opitch if r < oh else off + FAR + (r - oh) * opitch
        assert torch.equal(arena[o:o + ow * es], wrows[r]), r
        arena[o:o + ow * es] = SENTINEL
    assert arena_clean(arena)


# ---- 8. torch_io, chroma=422 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16], ids=["nv16", "p210"])
def test_torch_upscale_yuv_422(ctx, dtype):
    s = ctx[False]
    s.out_scale = 2
    fmt = NV16 if dtype == torch.uint8 else P210
    surf = surface(160, fmt)
    want = run(s, surf, fmt, fmt)
    as_t = lambda a: torch.from_numpy(a.view(np.int16) if fmt == P210 else a).cuda()  # noqa: E731
    back = lambda t: t.cpu().numpy().view(NP[fmt])  # noqa: E731
    x = as_t(surf)
    y = torch_io.upscale_yuv(s, x, chroma=422)
    torch.cuda.synchronize()
    assert y.dtype == dtype and tuple(y.shape) == (H * 4, W * 2) and same_bits(back(y), want)
    # a (y, uv) pair of views into a padded surface, written into a pair of views of a canvas
    big = torch.zeros(2 * H + 9, W + 12, dtype=dtype, device="cuda")
    big[4:4 + H, 2:2 + W], big[H + 7:2 * H + 7, 2:2 + W] = x[:H], x[H:]
    fill = 0x4D4D if fmt == P210 else 0x4D
    canvas = torch.full((H * 4 + 8, W * 2 + 6), fill, dtype=dtype, device="cuda")
    oy, ouv = canvas[1:1 + 2 * H, 4:4 + 2 * W], canvas[2 * H + 5:4 * H + 5, 4:4 + 2 * W]
    got = torch_io.upscale_yuv(s, (big[4:4 + H, 2:2 + W], big[H + 7:2 * H + 7, 2:2 + W]), out=(oy, ouv), chroma=422)
    torch.cuda.synchronize()
    assert got[0] is oy and got[1] is ouv
    assert same_bits(back(torch.cat([oy, ouv]).contiguous()), want)
    untouched = torch.ones_like(canvas, dtype=torch.bool)
    untouched[1:1 + 2 * H, 4:4 + 2 * W] = False
    untouched[2 * H + 5:4 * H + 5, 4:4 + 2 * W] = False
    assert (canvas[untouched] == fill).all()


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16], ids=["nv16", "p210"])
def test_torch_delta_and_sequence_422(ctx, dtype):
    """upscale_delta and upscale_sequence with chroma=422 give, frame by frame, the bytes of the lone C-level call."""
    s = ctx[False]
    fmt = NV16 if dtype == torch.uint8 else P210
    as_t = lambda a: torch.from_numpy(a.view(np.int16) if fmt == P210 else a).cuda()  # noqa: E731
    back = lambda t: t.cpu().numpy().view(NP[fmt])  # noqa: E731
    frames = [surface(170, fmt)]
    for k, (r, c) in enumerate(((3, 5), (H + 20, 30))):  # frame 1: one Y sample of tile 0; frame 2: one chroma sample of the last tile row
        f = frames[-1].copy()
        f[r, c] ^= 0x80
        frames.append(f)
    want = [run(s, f, fmt, fmt) for f in frames]
    xs = [as_t(f) for f in frames]
    y0 = torch_io.upscale_yuv(s, xs[0], chroma=422)
    out, n = torch_io.upscale_delta(s, xs[1], xs[0], y0.clone(), chroma=422)
    torch.cuda.synchronize()
    assert 0 < n < 6 and same_bits(back(out), want[1])
    ys, n = torch_io.upscale_sequence(s, xs, chroma=422)
    torch.cuda.synchronize()
    assert 6 < n < 18 and all(tuple(y.shape) == (8 * H, 4 * W) for y in ys)
    for y, w_ in zip(ys, want):
        assert same_bits(back(y), w_)
