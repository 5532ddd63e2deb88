"""GPU tests added in rounds 2 and 3 (run with -m gpu on the MI355X box): concurrency of rsr_process on one context, the
workspace guard invariant, the BASELINE configurations that had no oracle check (C3, C5, the edge-tile classes of C2),
a raw-fp32 x4.bin, pinned-memory I/O, blob validation, the bench's multi-rank control flow on one GPU.

Everything goes through the C-ABI; the oracle is only the checker."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import oracle
import oracle_pool
import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import synth
from gpu_support import paths  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sr(paths):
    s = R.RealSR(0)
    s.load(*paths)
    yield s
    s.close()


def padded_tile(img, x0, y0, tw, th, P=10):
    """The padded network input of the tile whose un-padded origin is (x0, y0): reflect-101 at the image border
    (realsr.cpp:613 copy_make_border type 2 == numpy 'reflect'), real neighbours elsewhere.  CHW float32 in [0,1]."""
    big = np.pad(img, ((P, P), (P, P), (0, 0)), mode="reflect")
    t = big[y0:y0 + th + 2 * P, x0:x0 + tw + 2 * P, :3]
    return t.astype(np.float32).transpose(2, 0, 1) * np.float32(1 / 255.0)


def quantise(ref, P=10):
    """realsr.cpp:804,820-831: crop the halo, v*255 + 0.5, truncate, clamp."""
    r = ref[:, 4 * P:-4 * P, 4 * P:-4 * P]
    return np.clip((r * 255.0 + 0.5).astype(np.int32), 0, 255).transpose(1, 2, 0)


def check_tile(out, img, net, x0, y0, tw, th):
    ref8 = quantise(net.forward(padded_tile(img, x0, y0, tw, th)))
    got = out[4 * y0:4 * (y0 + th), 4 * x0:4 * (x0 + tw)].astype(int)
    d = np.abs(got - ref8)
    assert d.max() <= 1, "tile at (%d,%d) %dx%d: max diff %d" % (x0, y0, tw, th, d.max())
    return (d > 0).mean()


# ---- concurrency -----------------------------------------------------------------------------------------------
def test_concurrent_process_on_one_context(sr):
    """The reference runs jobs_proc threads through ONE RealSR (main.cpp:811-828).  6 threads push images of 5 different
    sizes (different plans, growing lane buffers, pageable and pinned destinations) through one context, 60 calls in all:
    every result must be byte-identical to the serial result of the same image."""
    sr.tilesize = 32
    sizes = [(50, 43, 3), (70, 20, 3), (33, 64, 3), (37, 20, 4), (120, 90, 3)]
    imgs = [synth.make_image(100 + i, w, h, c) for i, (w, h, c) in enumerate(sizes)]
    sr._push_params()
    want = [sr.process(im, push_params=False) for im in imgs]
    errors = []

    def worker(tid):
        try:
            pin = None
            for it in range(10):
                k = (tid * 3 + it) % len(imgs)
                if (tid + it) % 3 == 0:  # every third call writes into pinned memory
                    pin = R.PinnedArray(want[k].shape)
                    got = sr.process(imgs[k], out=pin.array, push_params=False)
                else:
                    got = sr.process(imgs[k], push_params=False)
                if not (got == want[k]).all():
                    errors.append("thread %d iteration %d image %d: %d bytes differ" % (tid, it, k, int((got != want[k]).sum())))
                if pin is not None:
                    pin.free()
                    pin = None
        except Exception as e:  # noqa: BLE001
            errors.append("thread %d: %r" % (tid, e))

    ts = [threading.Thread(target=worker, args=(t,)) for t in range(6)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors[:5]


def test_concurrent_large_frames_share_the_workspace(sr):
    """Two threads, full-HD-sized tiles (tile 200): the calls share one workspace and one compute stream; uploads and
    downloads overlap the other call's kernels.  Results identical to the serial ones."""
    sr.tilesize = 200
    a, b = synth.make_image(31, 640, 420), synth.make_image(32, 500, 610)
    sr._push_params()
    wa, wb = sr.process(a, push_params=False), sr.process(b, push_params=False)
    out, errs = {}, []

    def run(name, img, want):
        for _ in range(4):
            got = sr.process(img, push_params=False)
            if not (got == want).all():
                errs.append(name)
        out[name] = True

    ts = [threading.Thread(target=run, args=("a", a, wa)), threading.Thread(target=run, args=("b", b, wb))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs and len(out) == 2


def test_pinned_buffers_equal_pageable(sr):
    sr.tilesize = 32
    img = synth.make_image(5, 61, 47)
    want = sr.process(img)
    pin_in, pin_out = R.PinnedArray(img.shape), R.PinnedArray(want.shape)
    pin_in.array[:] = img
    got = sr.process(pin_in.array, out=pin_out.array)
    assert (got == want).all()
    sr.set_option("chunk_mb", 1)  # pageable download in several chunks
    try:
        big = synth.make_image(6, 300, 260)
        sr.tilesize = 200
        w1 = sr.process(big)
        p2 = R.PinnedArray(w1.shape)
        assert (sr.process(big, out=p2.array) == w1).all()
    finally:
        sr.set_option("chunk_mb", 16)


# ---- workspace guard invariant (every conv-input plane has a zero guard in front, whatever ran before) --------------------
def test_guards_stay_zero_across_layout_and_slot_changes(paths):
    """A large image lays the workspace out for many slots; a small-cap image re-lays it out with 2 slots; a third image
    with the SAME slot capacity but more slots must not find stale activations where its guards are (conv zero padding
    reads them).  Compared with a fresh context, byte for byte."""
    imgs = [synth.make_image(41, 150, 120), synth.make_image(42, 40, 20), synth.make_image(43, 100, 20)]
    a = R.RealSR(0)
    a.load(*paths)
    a.tilesize = 32
    seq = [a.process(im) for im in imgs]
    # and back to the first layout
    again = a.process(imgs[0])
    a.close()
    for im, got in zip(imgs, seq):
        f = R.RealSR(0)
        f.load(*paths)
        f.tilesize = 32
        want = f.process(im)
        f.close()
        assert (got == want).all(), "image %s differs from a fresh context" % (im.shape,)
    assert (again == seq[0]).all()


# ---- BASELINE configs that had no oracle check ----------------------------------------------------------------------------
def test_c2_tiles_against_oracle(sr, paths):
    """C2 (1920x1080, tile 200): 45 x 220x220, 9 x 220x100 (last tile row), 5 x 140x220 (last column), the 140x100 corner.
    ALL 60 tiles against the committed strided oracle samples (tests/golden/frame_c2.npz: the oracle's frame on a lattice of every
    8th output row / column, 540 k samples), +-1 uint8; then 6 tiles -- the corner, a 140x220, two 220x100, two interior ones,
    rotating from day to day -- in full against the LIVE oracle (RSR_SLOW_TESTS=1: all 60, ~4 min of CPU).  Tile loop:
    realsr.cpp:541-553."""
    sr.tilesize = 200
    img = synth.make_image(1235, 1920, 1080)
    out = sr.process(img)
    assert sr.get_stat("plan_batches") == 1 and sr.get_stat("plan_slots_per_batch") == 60
    n, frac = oracle_pool.check_frame_golden(out, "c2", img, paths[1], 200)
    assert n == 60 and frac < 0.15
    print("C2: 60 of 60 tiles within +-1 of the golden oracle samples, %.2f %% of the samples differ" % (100 * frac))
    tiles = None if os.environ.get("RSR_SLOW_TESTS") == "1" else oracle_pool.rotating_tiles(10, 6)
    n, frac = oracle_pool.check_frame_tiles(out, img, *paths, T=200, tiles=tiles)
    assert n == (60 if tiles is None else 6) and frac < 0.15
    print("C2: %d tiles %s in full within +-1 of the live oracle, %.2f %% of the bytes differ" % (n, tiles or "(all)", 100 * frac))


def test_c3_tiles_against_oracle_and_batching(sr, paths):
    """C3 (3840x2160, tile 400: 10 x 6 tiles -- 45 x 420x420, 9 x 420x180 (last row), 5 x 260x420 (last column), the 260x180
    corner; every tile ends in a 4-pixel block column = folded work items).  Under the default 64 GiB workspace budget the 60 slots
    of 176,400 px x 6,048 B = 64.0 GB form ONE batch (asserted).  ALL 60 tiles against the committed strided oracle samples
    (tests/golden/frame_c3.npz, 2.1 M samples), +-1 uint8; 6 rotating tiles (corner, a 260x420, two 420x180, two 420x420) in full
    against the live oracle.  Then the frame again with a 32 GiB budget = 2 batches of 32 + 28 slots (asserted): byte-identical
    -- batches are an implementation detail."""
    sr.tilesize = 400
    img = synth.make_image(1236, 3840, 2160)
    out = sr.process(img)
    assert out.shape == (8640, 15360, 3)
    assert sr.get_stat("plan_batches") == 1 and sr.get_stat("plan_slots_per_batch") == 60
    n, frac = oracle_pool.check_frame_golden(out, "c3", img, paths[1], 400)
    assert n == 60 and frac < 0.15
    print("C3: 60 of 60 tiles within +-1 of the golden oracle samples, %.2f %% of the samples differ" % (100 * frac))
    tiles = oracle_pool.rotating_tiles(10, 6)
    n, frac = oracle_pool.check_frame_tiles(out, img, *paths, T=400, tiles=tiles)
    assert n == 6 and frac < 0.15
    print("C3: %d tiles %s in full within +-1 of the live oracle, %.2f %% of the bytes differ" % (n, tiles, 100 * frac))
    sr.set_option("max_workspace_mb", 32 * 1024)
    try:
        two = sr.process(img)
        assert sr.get_stat("plan_batches") == 2 and sr.get_stat("plan_slots_per_batch") == 32  # 32 x 1.067 GB <= 32 GiB
    finally:
        sr.set_option("max_workspace_mb", 65536)
    assert (two == out).all()
    assert (sr.process(img) == out).all()  # determinism


def test_c5_tta_against_oracle():
    """C5 = BASELINE.json configs[4]: models-DF2K_JPEG (the synthetic stand-in: seed 43, as bench.py's C5 leg), 1080p, tile 200,
    -x.  TTA x8 -- 4 + 4 transposed-shape slots for the non-square edge tiles (engine.cpp / realsr.cpp:251-258, scatter
    realsr.cpp:617-650, gather :707-724).  A 260x230 image whose grid has all four tile shapes against the oracle's own TTA path
    (whole image), then the real 1080p frame: ALL 60 tiles against the committed strided oracle samples
    (tests/golden/frame_c5.npz: 480 oracle network evaluations, made once by tests/golden/make_frames.py), and 4 rotating tiles --
    the corner, a 140x220, two 220x100 -- in full against an independent live statement of the 8 dihedral passes (all 60 with
    RSR_SLOW_TESTS=1)."""
    d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K_JPEG", 43)
    jp = (os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
    s = R.RealSR(0, tta_mode=True)
    s.load(*jp)
    s.tilesize = 200
    img = synth.make_image(1239, 260, 230)
    got = s.process(img)
    ref = oracle.OracleNet(*jp).process(img, 200, tta=True)
    d = np.abs(got.astype(int) - ref.astype(int))
    assert d.max() <= 1
    assert (d > 0).mean() < 0.15
    big = synth.make_image(1239, 1920, 1080)
    out = s.process(big)
    s.close()
    n, frac = oracle_pool.check_frame_golden(out, "c5", big, jp[1], 200)
    assert n == 60 and frac < 0.15
    print("C5 (models-DF2K_JPEG, TTA): 60 of 60 tiles within +-1 of the golden oracle samples, %.2f %% of the samples differ" % (100 * frac))
    tiles = None if os.environ.get("RSR_SLOW_TESTS") == "1" else oracle_pool.rotating_tiles(10, 6, k=4)
    n, frac = oracle_pool.check_frame_tiles(out, big, *jp, T=200, tiles=tiles, tta=True)
    assert n == (60 if tiles is None else 4) and frac < 0.15
    print("C5 (models-DF2K_JPEG, TTA): %d tiles %s in full within +-1 of the live oracle, %.2f %% of the bytes differ" % (n, tiles or "(all)", 100 * frac))


def test_rgba_frame_at_baseline_size(sr, paths):
    """no BASELINE config has an alpha channel.  The C2 frame with one added: 1920x1080 RGBA at tile 200 through the
    alpha path (alpha kept un-normalised next to the RGB planes, ncnn-flavoured bicubic x4 of every tile's UN-PADDED alpha rectangle in
    postproc_tiles -- realsr_preproc.comp:79-88, realsr.cpp:128-140,431-442, realsr_postproc.comp:58-61 -- so the planar conv_last /
    postproc launch instead of the fused uint8 epilogue).  The RGB channels must satisfy the committed C2 oracle samples (all 60
    tiles, +-1: the alpha channel must not disturb them), and the alpha channel the oracle's bicubic, tile by tile, +0.5, saturate
    (+-1; every tile shape: 200x200, 200x80, 120x200, 120x80)."""
    sr.tilesize = 200
    rgb = synth.make_image(1235, 1920, 1080)
    yy, xx = np.mgrid[0:1080, 0:1920]
    alpha = ((np.sin(xx / 37.0) * np.cos(yy / 23.0) * 0.5 + 0.5) * 255).astype(np.uint8)
    alpha[300:420, 500:900] = 0      # hard edges, also across tile borders (x = 600, 800; y = 400)
    alpha[390:410, 100:1800] = 255
    img = np.concatenate([rgb, alpha[:, :, None]], axis=2)
    out = sr.process(img)
    assert out.shape == (4320, 7680, 4)
    n, frac = oracle_pool.check_frame_golden(out, "c2", rgb, paths[1], 200)
    assert n == 60
    worst, ndiff, total = 0, 0, 0
    for y0 in range(0, 1080, 200):
        for x0 in range(0, 1920, 200):
            th, tw = min(y0 + 200, 1080) - y0, min(x0 + 200, 1920) - x0
            ref = oracle.bicubic(alpha[y0:y0 + th, x0:x0 + tw].astype(np.float32), 4 * th, 4 * tw)
            ref8 = np.clip((ref + 0.5).astype(np.int32), 0, 255)
            d = np.abs(out[4 * y0:4 * (y0 + th), 4 * x0:4 * (x0 + tw), 3].astype(int) - ref8)
            assert d.max() <= 1, "alpha of the tile at (%d,%d): max diff %d" % (x0, y0, d.max())
            worst, ndiff, total = max(worst, int(d.max())), ndiff + int((d > 0).sum()), total + d.size
    print("RGBA 1080p: RGB 60 of 60 tiles within +-1 of the golden C2 samples (%.2f %% differ); alpha 60 of 60 tiles within +-1 of the oracle's bicubic (max %d, %.3f %% differ)" % (
        100 * frac, worst, 100.0 * ndiff / total))


def test_baseline_tiles_against_an_independent_pytorch_graph(sr, weights):
    """A second checker that shares NOTHING with oracle/realsr_oracle.c: the canonical ESRGAN RRDBNet(3, 3, 64, 23, gc = 32) assembled
    from torch.nn.functional (tests/torch_ref.py: conv2d / leaky_relu 0.2 / cat / nearest x2, fp32 on the CPU), fed with the seeded
    weights as synth.make_weights() produces them (not as any .bin reader parsed them) and with tiles cut by numpy (reflect-101 halo
    of 10, realsr.cpp:613; crop 40, v * 255 + 0.5, truncate, clamp, realsr.cpp:804,820-831).  Tiles of the C2 frame -- the first
    (220x220), a 220x100, the 140x100 corner -- and the 260x180 corner of the C3 frame (folded last block column) must be within +-1
    uint8 of it (~35 s of PyTorch-CPU time; a first run with six tiles incl. an interior C2 tile and a 420x180 C3 tile: profiles/r05_gpu_tests.txt): the same bar as against the oracle, by an independent route (SURVEY 8(c):
    "independent cross-check available in-container: PyTorch CPU")."""
    import torch_ref
    wl = [(np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)) for W, b in weights]
    try:
        for name, iseed, w, h, T, tiles in (("C2", 1235, 1920, 1080, 200, [(0, 0), (4, 5), (9, 5)]),
                                            ("C3", 1236, 3840, 2160, 400, [(9, 5)])):
            sr.tilesize = T
            img = synth.make_image(iseed, w, h)
            out = sr.process(img)
            worst, ndiff, total = 0, 0, 0
            for xi, yi in tiles:
                x0, y0 = xi * T, yi * T
                tw, th = min(x0 + T, w) - x0, min(y0 + T, h) - y0
                ref = torch_ref.net_forward_np(wl, oracle_pool.padded_tile(img, x0, y0, tw, th))
                ref8 = quantise(ref)
                got = out[4 * y0:4 * (y0 + th), 4 * x0:4 * (x0 + tw)].astype(int)
                d = np.abs(got - ref8)
                assert d.max() <= 1, "%s tile (%d,%d): max diff %d vs the PyTorch graph" % (name, xi, yi, d.max())
                worst, ndiff, total = max(worst, int(d.max())), ndiff + int((d > 0).sum()), total + d.size
            print("%s: %d tiles %s within +-1 of the independent PyTorch graph, %.2f %% of the bytes differ" % (name, len(tiles), tiles, 100.0 * ndiff / total))
    finally:
        sr.tilesize = 200


def test_engine_options_do_not_change_the_bytes(paths, sr):
    """Scheduling / staging knobs (include/realsr_hip.h: rsr_set_option) are implementation details: tail launch groups,
    work-item order, one lane, single-threaded staging copies, small download chunks, no dead-output elimination, rows below
    the tile computed, small tile batches, the one-thread-per-pixel / the LDS-staged pre and post kernels forced (dbg 32768 / 65536;
    with 8192 the RGB path runs postproc_tiles too) -- every one must reproduce the default configuration's bytes, RGB, RGBA and TTA."""
    imgs = [synth.make_image(61, 150, 100), synth.make_image(62, 70, 90, 4)]
    sr.tilesize = 32
    want = [sr.process(im) for im in imgs]
    t = R.RealSR(0, tta_mode=True)
    t.load(*paths)
    t.tilesize = 32
    want_tta = t.process(imgs[0])
    knobs = [("tail_group", 1, 0), ("tail_group", 3, 0), ("alternate_order", 0, 1), ("xcd_order", 0, 1), ("max_lanes", 1, 4), ("copy_threads", 1, 4), ("chunk_mb", 1, 16),
             ("trim", 0, 1), ("fold", 0, 1), ("dbg", 32, 0), ("dbg", 8192, 0), ("dbg", 16384, 0), ("dbg", 32768, 0), ("dbg", 65536, 0), ("dbg", 8192 | 65536, 0), ("flow_flags", 3, 0), ("flow_flags", 4, 0), ("max_workspace_mb", 64, 65536), ("num_cu", 64, 256)]
    try:
        for key, val, default in knobs:
            for ctx, ims, refs in ((sr, imgs, want), (t, imgs[:1], [want_tta])):
                ctx.set_option(key, val)
                try:
                    for im, ref in zip(ims, refs):
                        assert (ctx.process(im) == ref).all(), (key, val, im.shape, ctx.tta_mode)
                finally:
                    ctx.set_option(key, default)
    finally:
        t.close()


@pytest.mark.parametrize("w,h,T", [(240, 50, 120), (250, 40, 240), (400, 45, 400), (130, 150, 120)])
def test_folded_last_column_of_baseline_tile_widths(paths, sr, w, h, T):
    """Padded tile widths 140 / 260 / 420 (BASELINE C2's edge tiles, C3's edge and interior tiles; realsr.cpp:170-181) end in a block
    column of 12 / 4 / 4 pixels that the engine computes with folded work items; their 2x-level widths 280 / 520 / 840 fold too (840,
    520: 8 pixels).  Whole images with such tiles: option "fold" 0 must reproduce the bytes, with and without dead-output
    elimination (a folded pair of block rows never starts inside the top margin: engine.cpp append_block_items), RGB and TTA; and
    the default configuration stays within +-1 of the oracle (the last case, 130 x 150 at tile 120: 140- and 30-wide tiles)."""
    img = synth.make_image(400 + w, w, h)
    t = R.RealSR(0, tta_mode=True)
    t.load(*paths)
    try:
        for ctx in (sr, t):
            ctx.tilesize = T
            want = ctx.process(img)
            for trim in (1, 0):
                ctx.set_option("trim", trim)
                ctx.set_option("fold", 0)
                got = ctx.process(img)
                ctx.set_option("fold", 1)
                assert (got == want).all(), (ctx.tta_mode, trim)
                assert (ctx.process(img) == want).all(), (ctx.tta_mode, trim)
            ctx.set_option("trim", 1)
            if w == 130 and ctx is sr:
                ref = oracle.OracleNet(*paths).process(img, T)
                assert np.abs(want.astype(int) - ref.astype(int)).max() <= 1
    finally:
        sr.set_option("trim", 1)
        sr.set_option("fold", 1)
        sr.tilesize = 200
        t.close()


def test_lds_staged_pre_post_kernels_equal_the_per_pixel_ones(paths, sr):
    """preproc_tiles_lds / postproc_tiles_lds (rows staged in LDS, dword loads, 1-KiB stores, transposed TTA variants through an
    LDS tile; forced with dbg 65536, by default only the TTA gather runs staged) against the one-thread-per-pixel kernels (dbg
    32768) -- same arithmetic, so the same BYTES: RGB through the
    two-kernel path (dbg 8192), RGBA (alpha bicubic), TTA, BGR order; widths that are not multiples of 4 (unaligned source rows),
    images smaller than the halo (every column reflected), tiles of 1 / 31 / 33 pixels, 200-pixel tiles."""
    t = R.RealSR(0, tta_mode=True)
    t.load(*paths)
    cases = [(50, 43, 3, 32), (37, 41, 4, 32), (5, 3, 3, 32), (1, 1, 4, 32), (33, 65, 3, 31), (131, 67, 4, 33), (301, 215, 3, 200), (97, 203, 4, 200)]
    try:
        for eng, extra in ((sr, 8192), (sr, 0), (t, 0)):
            for (w, h, c, T) in cases:
                if eng is t and (c == 4 or T == 200):
                    continue
                eng.tilesize = T
                img = synth.make_image(300 + w, w, h, c)
                for bgr in (0, 1):
                    eng.set_option("bgr", bgr)
                    try:
                        eng.set_option("dbg", extra | 65536)
                        new = eng.process(img)
                        eng.set_option("dbg", extra | 32768)
                        old = eng.process(img)
                        eng.set_option("dbg", extra)
                        dflt = eng.process(img)
                    finally:
                        eng.set_option("dbg", 0)
                        eng.set_option("bgr", 0)
                    assert (new == old).all(), (w, h, c, T, bgr, eng.tta_mode, int((new != old).sum()))
                    assert (dflt == old).all(), (w, h, c, T, bgr, eng.tta_mode)
        t.tilesize = 200
        img = synth.make_image(77, 260, 230)  # all four tile shapes, transposed-shape slots
        new = t.process(img)                  # default under TTA: the LDS-staged gather
        t.set_option("dbg", 32768)
        assert (t.process(img) == new).all()
        t.set_option("dbg", 65536)
        assert (t.process(img) == new).all()
    finally:
        t.close()
        sr.set_option("dbg", 0)


def test_dead_output_elimination_at_other_prepaddings(sr):
    """engine.cpp tail_margin: the ring arithmetic behind `trim` ((crop4 - 3) >> 1, (m - 1) >> 1, one ring per conv) is general
    in prepadding, but BASELINE only ever runs 10.  trim = 0 (every padded-tile pixel computed at every layer) against the default
    for prepadding 1 / 3 / 7 / 10 on images whose tile heights are NOT multiples of 4 (81 + 2P rows, a 37-row last tile row) --
    the kept bytes must be the same."""
    img = synth.make_image(63, 113, 118)
    try:
        for P, T in ((1, 81), (3, 81), (7, 81), (10, 81), (3, 32)):
            sr.tilesize, sr.prepadding = T, P
            want = sr.process(img)
            sr.set_option("trim", 0)
            try:
                full = sr.process(img)
            finally:
                sr.set_option("trim", 1)
            assert (full == want).all(), (P, T, int((full != want).sum()))
    finally:
        sr.prepadding = 10


def test_raw_fp32_bin_with_unrepresentable_weights(tmp_path):
    """A raw-fp32 x4.bin (tag 0) whose weights are NOT fp16-representable: the packer rounds them to
    fp16 (what ncnn's Vulkan fp16-storage path does), the oracle keeps fp32.  Stated tolerance: +-1 uint8 on >= 99.9 % of
    the bytes, never more than 2 (weight rounding adds ~2^-11 relative error per product)."""
    d = synth.make_model_dir(str(tmp_path), "models-raw32", 44, encoding="fp32", round_fp16=False)
    pp, bp = os.path.join(d, "x4.param"), os.path.join(d, "x4.bin")
    assert R.model_info(pp, bp)["bin_encoding"] == 0
    net = oracle.OracleNet(pp, bp)
    w0 = net.conv(5)["weight"]
    assert (w0.astype(np.float16).astype(np.float32) != w0).mean() > 0.5  # really not fp16 values
    s = R.RealSR(0)
    s.load(pp, bp)
    s.tilesize = 64
    img = synth.make_image(77, 90, 70)
    got = s.process(img)
    # pre-quantise error of one tile, for the record
    x = padded_tile(img, 0, 0, 64, 64)
    e = np.abs(s.net_forward(x.astype(np.float16)).astype(np.float32) - net.forward(x.astype(np.float16).astype(np.float32)))
    print("raw-fp32 weights: pre-quantise max %.3e p99.9 %.3e" % (e.max(), np.quantile(e, 0.999)))
    s.close()
    ref = net.process(img, 64)
    dd = np.abs(got.astype(int) - ref.astype(int))
    assert dd.max() <= 2 and (dd > 1).mean() <= 1e-3
    assert e.max() <= 6e-3


# ---- memory policy: the tile batch follows the memory that is really free ---------------------------------------------
def test_weight_statistics_headroom_hot_model(tmp_path):
    """The real models-DF2K / DF2K_JPEG blobs are absent (/root/reference/.MISSING_LARGE_BLOBS), so what their statistics could do
    to an fp16-storage engine is shown as headroom: a second synthetic model (seed 44) whose conv_first is 32 x larger and conv_last
    32 x smaller -- every feature map in between is 32 x the stand-in's: trunk activations peak at ~6e3 (asserted >= 1e3, a tenth of
    fp16's 65,504) -- and whose output saturates on >= 5 % of the pixels (both clamps of realsr.cpp:804,820-831 busy).  BASELINE C1
    (256x256, tile 128) and one C2 tile (200x200 -> a 220x220 padded tile) must still be within +-1 of the oracle, whose
    intermediates are fp32.  (Past 65,504 the model is refused by tools/check_real_model.py: tests/test_model_io.py.)"""
    import importlib.util
    d = synth.make_model_dir(str(tmp_path), "models-hot32", 44, hot=32.0, last_gain=0.15)
    pp, bp = os.path.join(d, "x4.param"), os.path.join(d, "x4.bin")
    net = oracle.OracleNet(pp, bp)
    spec = importlib.util.spec_from_file_location("check_real_model", os.path.join(ROOT, "tools", "check_real_model.py"))
    crm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(crm)
    probe = synth.make_image(1234, 64, 64)
    tile = np.pad(probe, ((10, 10), (10, 10), (0, 0)), mode="reflect")[:, :, :3].astype(np.float32).transpose(2, 0, 1) * np.float32(1 / 255.0)
    peaks, _ = crm.activation_ranges(net, np.ascontiguousarray(tile))
    top = max(v for _, v in peaks)
    assert 1e3 <= top < 65504, top
    s = R.RealSR(0)
    s.load(pp, bp)
    try:
        for name, img, T in (("C1", synth.make_image(1234, 256, 256), 128), ("one C2 tile", synth.make_image(1235, 200, 200), 200)):
            s.tilesize = T
            got = s.process(img)
            ref = net.process(img, T)
            dd = np.abs(got.astype(int) - ref.astype(int))
            sat = float(((ref == 0) | (ref == 255)).mean())
            print("hot model (trunk peak %.0f), %s: max |diff| %d, %.2f %% of the bytes differ, %.1f %% of the output saturated" % (top, name, dd.max(), 100 * (dd > 0).mean(), 100 * sat))
            assert dd.max() <= 1, name
            assert sat >= 0.05, (name, sat)
    finally:
        s.close()


def test_weight_statistics_channel_spread_model(tmp_path):
    """Trained ESRGAN weights are not i.i.d. filters: a few loud output channels, many quiet ones.  A third stand-in (seed 45, synth
    chan_sigma = 1: log-normal per-output-channel gains, unit RMS per conv, ~50x between the loudest and the quietest channel of a conv;
    trunk peaks ~7e2).  (1) With the base model's output swing (last_gain 0.12) BASELINE C1 holds +-1 against the oracle.  (2) With a
    1.7x larger output swing (last_gain 0.2: fp32 output -0.56 .. 1.79) the fp16 STORAGE noise itself reaches one uint8 step (max
    pre-quantise error 4.3e-3 vs 1 / 255 = 3.9e-3) and ONE byte of the 3.1 M of the C1 frame differs by 2 (measured, round 5) -- that
    is the format the reference's Vulkan path shares (realsr.cpp:44-46), not this engine's arithmetic: on a tile of that model the
    engine's deviation from the fp32 oracle must equal, statistically, that of a PyTorch emulation of fp16 storage / fp32 arithmetic
    (tests/torch_ref.py rrdbnet_forward_fp16_storage: mean within 10 %, p99.9 within 25 %), and the engine must be CLOSER to that
    emulation than either is to the oracle.  DESIGN.md section 3 states the bar accordingly."""
    import torch_ref
    img = synth.make_image(1234, 256, 256)
    d = synth.make_model_dir(str(tmp_path), "models-spread", 45, chan_sigma=1.0, last_gain=0.12)
    pp, bp = os.path.join(d, "x4.param"), os.path.join(d, "x4.bin")
    s = R.RealSR(0)
    s.load(pp, bp)
    try:
        s.tilesize = 128
        got = s.process(img)
    finally:
        s.close()
    ref = oracle.OracleNet(pp, bp).process(img, 128)
    dd = np.abs(got.astype(int) - ref.astype(int))
    print("channel-spread model, C1: max |diff| %d, %.2f %% of the bytes differ" % (dd.max(), 100 * (dd > 0).mean()))
    assert dd.max() <= 1
    d = synth.make_model_dir(str(tmp_path), "models-spread-wide", 45, chan_sigma=1.0, last_gain=0.2)
    pp, bp = os.path.join(d, "x4.param"), os.path.join(d, "x4.bin")
    net = oracle.OracleNet(pp, bp)
    wl = [(c["weight"], c["bias"]) for c in (net.conv(i) for i in range(net.num_convs))]
    tile = np.ascontiguousarray(oracle_pool.padded_tile(img, 0, 0, 128, 128))
    a = net.forward(tile)
    b = torch_ref.net_forward_fp16_storage_np(wl, tile)
    s = R.RealSR(0)
    s.load(pp, bp)
    try:
        c = s.net_forward(tile.astype(np.float16)).astype(np.float32)
    finally:
        s.close()
    e_eng, e_emu, e_x = np.abs(c - a), np.abs(b - a), np.abs(c - b)
    print("wide-swing spread model, one 148x148 tile: engine vs oracle mean %.3e p99.9 %.3e max %.3e | fp16-storage emulation vs oracle mean %.3e p99.9 %.3e max %.3e | "
          "engine vs emulation mean %.3e" % (e_eng.mean(), np.quantile(e_eng, 0.999), e_eng.max(), e_emu.mean(), np.quantile(e_emu, 0.999), e_emu.max(), e_x.mean()))
    assert abs(e_eng.mean() / e_emu.mean() - 1) < 0.10
    assert abs(np.quantile(e_eng, 0.999) / np.quantile(e_emu, 0.999) - 1) < 0.25
    assert e_x.mean() < e_eng.mean() and e_x.mean() < e_emu.mean()


def test_workspace_budget_follows_free_memory(paths):
    """The reference bounds device memory through the tile size (main.cpp:761-774); here all tiles of an image form one batch
    whose workspace (17.6 GB for a 1080p frame at tile 200) must fit.  With all but ~8 GB of the device taken by somebody else
    the engine has to plan smaller batches on its own (90 % of free memory; a batch that still fails to allocate is halved and
    re-planned) and produce the same bytes as the unconstrained run -- not RSR_E_NOMEM."""
    import torch
    img = synth.make_image(71, 1920, 1080)
    a = R.RealSR(0)
    a.load(*paths)
    a.tilesize = 200
    want = a.process(img)
    a.close()
    torch.cuda.empty_cache()
    free_mb, total_mb = R.device_memory(0)
    try:
        hog = torch.empty(max(0, free_mb - 8 * 1024) << 20, dtype=torch.uint8, device="cuda")
    except RuntimeError as e:  # the allocator could not hand out one block that large: nothing to test against
        pytest.skip("cannot fill the device: %s" % str(e)[:80])
    try:
        left_mb, _ = R.device_memory(0)
        assert left_mb < 12 * 1024, "the test needs a nearly full device (%d MiB free)" % left_mb
        b = R.RealSR(0)
        b.load(*paths)
        b.tilesize = 200
        got = b.process(img)
        prof_calls = b.get_profile()["calls"]
        b.close()
    finally:
        del hog
        torch.cuda.empty_cache()
    assert (got == want).all()
    assert prof_calls == 0  # (profiling was off; the call simply must have succeeded in several batches)


def test_workspace_clamp_is_dropped_when_memory_returns(paths):
    """What one failed workspace allocation leaves behind (ws_clamp, enqueue_image's retry) must not halve the tile batches of
    this context for ever: the next call that finds the device with room for twice the clamped size plans without it.  The
    clamp is planted through its test hook (1 GiB = 3 tiles of 220 x 220 per batch): the first call afterwards already sees a
    nearly empty 288 GB device and runs the frame in one batch; a clamp the device can NOT satisfy twice over stays."""
    s = R.RealSR(0)
    s.load(*paths)
    s.tilesize = 200
    img = synth.make_image(72, 1000, 600)  # 5 x 3 tiles
    want = s.process(img)
    assert s.get_stat("plan_batches") == 1 and s.get_stat("ws_clamp_mb") == -1
    s.set_option("ws_clamp_mb", 1024)
    assert s.get_stat("ws_clamp_mb") == 1024
    assert (s.process(img) == want).all()
    assert s.get_stat("ws_clamp_mb") == -1 and s.get_stat("plan_batches") == 1
    free_mb, _ = R.device_memory(0)
    s.set_option("ws_clamp_mb", free_mb)  # "twice that much" is not there: the clamp holds, and so does the result
    assert (s.process(img) == want).all()
    assert s.get_stat("ws_clamp_mb") == free_mb
    s.close()


# ---- blob validation (a failed load must leave the loaded model intact) ------------------------------------------------------
def test_persistent_workspace_failure_backs_off(paths):
    """ADVICE r04 (engine.cpp enqueue_image): when the CAUSE of a failed workspace allocation does not go away (fragmentation,
    hipMemGetInfo overstating what one hipMalloc can get) the "device has room for twice the clamp again" test is true on every
    call; without a back-off every frame would re-plan at full size, fail, drain the stream and rebuild the workspace.  With the
    test hook "ws_fail_above_mb" (workspaces above 2 GiB are refused, every time) 13 calls must see only the first failure and the
    attempts at full size the back-off allows (after 4, then 8 calls) -- and the frames stay byte-identical.  When the cause is
    gone the next scheduled attempt brings the single batch back."""
    s = R.RealSR(0)
    s.load(*paths)
    s.tilesize = 200
    img = synth.make_image(72, 1000, 600)  # 5 x 3 tiles = 4.4 GB of workspace in one batch, 7 tiles = 1.95 GiB
    try:
        want = s.process(img)
        assert s.get_stat("plan_batches") == 1
        s.set_option("ws_fail_above_mb", 2048)
        s.set_option("max_workspace_mb", 65536)  # (drops the plans: the next call plans afresh, at full size)
        for _ in range(13):
            assert (s.process(img) == want).all()
        assert s.get_stat("plan_batches") == 3 and s.get_stat("plan_slots_per_batch") == 7
        assert s.get_stat("ws_failures") == 3, s.get_stat("ws_failures")  # call 1, then the attempts of calls 5 and 13
        assert s.get_stat("clamp_backoff") == 16
        s.set_option("ws_fail_above_mb", -1)
        for i in range(17):
            assert (s.process(img) == want).all()
            if s.get_stat("ws_clamp_mb") == -1:
                break
        assert s.get_stat("ws_clamp_mb") == -1 and s.get_stat("plan_batches") == 1 and s.get_stat("ws_failures") == 3
        assert s.get_stat("clamp_backoff") == 4
    finally:
        s.close()


def test_corrupt_blob_is_refused_and_state_survives(paths, sr):
    sr.tilesize = 32
    img = synth.make_image(8, 40, 30)
    want = sr.process(img)
    blob = R.model_pack(*paths)
    rec = np.dtype([("cin", "<u4"), ("cout", "<u4"), ("act", "<u4"), ("nplanes", "<u4"), ("nt", "<u4"),
                    ("slope", "<f4"), ("b_off", "<u8"), ("w16_off", "<u8"), ("aux_off", "<u8")])
    assert rec.itemsize == 48
    for field, value in (("w16_off", blob.size - 256), ("cin", 128), ("nt", 2), ("b_off", blob.size + 4096), ("aux_off", 4096)):
        bad = blob.copy()
        table = bad[24:24 + 351 * 48].view(rec)
        table[field][7] = value
        with pytest.raises(R.RealSRError) as e:
            sr.load_packed(bad)
        assert e.value.code == R.RSR_E_FORMAT, field
        assert (sr.process(img) == want).all(), "a refused blob must not disturb the loaded model"
    old_version = blob.copy()
    old_version[4:8].view("<u4")[0] = 4  # a blob of the previous layout (with the round-1 weight images) is refused, not misread
    with pytest.raises(R.RealSRError) as e:
        sr.load_packed(old_version)
    assert e.value.code == R.RSR_E_FORMAT
    # the blob itself loads and gives the same bytes as rsr_load
    s2 = R.RealSR(0)
    s2.load_packed(blob)
    s2.tilesize = 32
    assert (s2.process(img) == want).all()
    s2.close()


def test_fused_conv_last_is_bit_identical_to_postproc_kernel(sr):
    """Non-TTA RGB: conv_last applies realsr_postproc.comp:62-83 itself and writes the uint8 image (no planar fp16 blob, no
    postproc launch).  dbg 8192 switches back to conv_last -> planar blob -> postproc_tiles: the bytes must be the same,
    incl. partial tiles, images smaller than a tile, and a 1080p frame at tile 200."""
    for (w, h, T) in [(50, 43, 32), (5, 3, 32), (130, 70, 64), (1920, 1080, 200)]:
        sr.tilesize = T
        img = synth.make_image(90 + w, w, h)
        fused = sr.process(img)
        sr.set_option("dbg", 8192)
        try:
            two = sr.process(img)
        finally:
            sr.set_option("dbg", 0)
        assert (fused == two).all(), (w, h, T, int((fused != two).sum()))


def test_bgr_pixel_order(sr, paths):
    """BGR(A) images (the reference's Windows/WIC path, realsr_preproc.comp:17-21 `bgr` specialisation):
    processing a channel-swapped image with bgr=1 gives the channel-swapped result, RGB and RGBA, fused and TTA paths."""
    sr.tilesize = 32
    t = R.RealSR(0, tta_mode=True)
    t.load(*paths)
    t.tilesize = 32
    try:
        for eng, (w, h, c) in ((sr, (50, 43, 3)), (sr, (37, 20, 4)), (t, (40, 33, 3))):
            img = synth.make_image(7 + c, w, h, c)
            want = eng.process(img)
            swapped = img.copy()
            swapped[..., [0, 2]] = img[..., [2, 0]]
            eng.set_option("bgr", 1)
            try:
                got = eng.process(swapped)
            finally:
                eng.set_option("bgr", 0)
            back = got.copy()
            back[..., [0, 2]] = got[..., [2, 0]]
            assert (back == want).all(), (w, h, c)
    finally:
        t.close()


# ---- several GPUs: group creation, tile-row sharding of one image ------------------------------------------------------
def test_tile_rows_and_group_processing_equal_the_full_image(paths):
    """one large image split over contexts.  Two contexts (both on GPU 0 here) each process a disjoint range of
    tile rows / of tiles into ONE output buffer; rsr_process_group deals the TILES (contiguous row-major ranges of equal
    load, rectangles fetched with 2-D copies) on its own threads.  Bytes identical to one call for 2 / 3 / 5 / 8 shares --
    ranges that start and end in the middle of a tile row included."""
    a, b = R.RealSR(0), R.RealSR(0)
    for s in (a, b):
        s.load(*paths)
        s.tilesize = 32
    img = synth.make_image(55, 70, 150)  # 3 x 5 tiles
    want = a.process(img)
    out = np.zeros_like(want)
    a.process_rows(img, out, 0, 2)
    assert (out[:2 * 32 * 4] == want[:2 * 32 * 4]).all() and (out[2 * 32 * 4:] == 0).all()
    b.process_rows(img, out, 2, 5)
    assert (out == want).all()
    # tile ranges: [0,4) = row 0 + the first tile of row 1; [4,5) one tile in the middle of a row; [5,13) tail of row 1, rows 2-3,
    # head of row 4; [13,15) the rest.  Every call may only touch the rectangles of its own tiles.
    out = np.zeros_like(want)
    mask = np.zeros(want.shape[:2], dtype=bool)
    for (t0, t1), ctx in zip(((4, 5), (0, 4), (13, 15), (5, 13)), (a, b, a, b)):
        ctx.process_tiles(img, out, t0, t1)
        for t in range(t0, t1):
            yi, xi = divmod(t, 3)
            mask[yi * 128:min((yi + 1) * 32, 150) * 4, xi * 128:min((xi + 1) * 32, 70) * 4] = True
        assert (out[mask] == want[mask]).all() and (out[~mask] == 0).all(), (t0, t1)
    assert mask.all()
    pinned = R.PinnedArray(want.shape)
    pinned.array[:] = 0
    b.process_tiles(img, pinned.array, 2, 11)  # rectangles into pinned memory
    a.process_tiles(img, pinned.array, 0, 2)
    a.process_tiles(img, pinned.array, 11, 15)
    assert (pinned.array == want).all()
    pinned.free()
    for parts in (1, 2, 3, 5, 8, 20):
        ctxs = [(a, b)[i % 2] for i in range(parts)]
        assert (R.process_group(ctxs, img) == want).all(), parts
    # a member allocates the output ROWS of its tile range, not the frame: a fresh context that only ever ran tiles [11, 15)
    # (tail of tile row 3 + row 4 = output rows 384..599 of 600) holds 216 rows
    cnew = R.RealSR(0)
    cnew.load(*paths)
    cnew.tilesize = 32
    part = np.zeros_like(want)
    cnew.process_tiles(img, part, 11, 15)
    assert abs(cnew.get_stat("lane_out_mb") * 1048576 - (600 - 384) * 280 * 3) < 1 and (part[384:] == want[384:])[:, 2 * 128:].all()
    cnew.set_option("chunk_mb", 1)
    big = synth.make_image(59, 900, 500)  # rectangles wider than a staging chunk row budget: several chunks per rectangle
    cnew.tilesize = 200
    wbig = cnew.process(big)
    pbig = np.zeros_like(wbig)
    for t0, t1 in ((0, 3), (3, 7), (7, 15)):
        cnew.process_tiles(big, pbig, t0, t1)
    assert (pbig == wbig).all()
    cnew.close()
    rgba = synth.make_image(56, 40, 100, 4)
    assert (R.process_group([a, b, a], rgba) == a.process(rgba)).all()
    for bad in ((3, 9), (7, 7), (-1, 2)):
        with pytest.raises(R.RealSRError) as e:
            (a.process_rows if bad == (3, 9) else a.process_tiles)(img, out, *bad)
        assert e.value.code == R.RSR_E_ARG
    b.tilesize = 48  # members that disagree about the tile grid would write rectangles twice / never: refused
    with pytest.raises(R.RealSRError) as e:
        R.process_group([a, b], img)
    assert e.value.code == R.RSR_E_ARG
    a.close()
    b.close()


def test_tile_ranges_under_tta_and_rgba(paths):
    """Tile ranges with the other output paths: TTA contexts (8 slots per tile, the LDS-staged gather writing dword rows into a
    device buffer that holds only the range's rows) and RGBA (alpha bicubic reads the INPUT image around the tile): every split
    of the tile grid gives the bytes of one call."""
    a, b = R.RealSR(0, tta_mode=True), R.RealSR(0, tta_mode=True)
    for s in (a, b):
        s.load(*paths)
        s.tilesize = 32
    try:
        for img in (synth.make_image(64, 70, 110), synth.make_image(65, 45, 100, 4)):
            want = a.process(img)
            for parts in (2, 3, 7):
                assert (R.process_group([(a, b)[i % 2] for i in range(parts)], img) == want).all(), (img.shape, parts)
            out = np.zeros_like(want)
            nt = -(-img.shape[1] // 32) * -(-img.shape[0] // 32)
            cuts = [0, 1, nt // 2, nt - 1, nt]
            for t0, t1 in zip(cuts, cuts[1:]):
                if t1 > t0:
                    b.process_tiles(img, out, t0, t1)
            assert (out == want).all(), img.shape
    finally:
        a.close()
        b.close()


def test_group_of_eight_under_concurrent_callers_and_a_failing_member(paths):
    """First contact with an 8-GPU node, rehearsed on one device: rsr_process_group over EIGHT contexts (all on device 0:
    rsr_create_group itself refuses duplicate ids) from FOUR caller threads at once -- 28 shares in flight on the process-wide worker
    pool (grown on demand), two lanes per context (callers wait for lanes), different image sizes per caller (the reference's proc
    threads share one RealSR per GPU the same way, main.cpp:811-828).  Every frame must equal the single-context bytes.  Then one
    member refuses every workspace (test hook ws_fail_above_mb = 0): the call reports RSR_E_NOMEM naming the share, the other
    members' shares complete, nobody hangs, and the group works again once the member recovers."""
    srs = []
    try:
        for _ in range(8):
            s = R.RealSR(0)
            s.load(*paths)
            s.tilesize = 32
            s.set_option("max_lanes", 2)
            s.set_option("max_workspace_mb", 2048)
            srs.append(s)
        imgs = [synth.make_image(500 + i, w, h) for i, (w, h) in enumerate([(200, 130), (90, 260), (257, 65), (128, 128)])]
        want = [srs[0].process(im) for im in imgs]
        bad = []

        def caller(k):
            try:
                for _ in range(3):
                    if not (R.process_group(srs, imgs[k]) == want[k]).all():
                        bad.append((k, "bytes differ"))
            except Exception as e:  # noqa: BLE001
                bad.append((k, repr(e)))

        ths = [threading.Thread(target=caller, args=(k,)) for k in range(4)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(300)
        assert not any(t.is_alive() for t in ths), "a group call hangs"
        assert not bad, bad
        assert srs[0].get_stat("pool_workers") >= 7
        srs[5].set_option("ws_fail_above_mb", 0)
        with pytest.raises(R.RealSRError) as e:
            R.process_group(srs, imgs[0])
        assert e.value.code == R.RSR_E_NOMEM and "gpu share 5" in str(e.value), str(e.value)
        srs[5].set_option("ws_fail_above_mb", -1)
        for t in [threading.Thread(target=caller, args=(k,)) for k in range(4)]:
            t.start()
            t.join(300)
        assert not bad, bad
    finally:
        for s in srs:
            s.close()


def test_group_share_runs_inline_when_no_worker_thread_can_be_started(paths):
    """std::thread creation failing inside rsr_process_group (thread limit, no memory) must neither throw across the C
    boundary nor leave a queued share without anybody to run it: the share runs on the calling thread.  Fresh process (an empty pool),
    thread creation refused through the RSR_POOL_NO_THREADS test hook."""
    code = (
        "import os, sys, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "os.environ['RSR_POOL_NO_THREADS'] = '1'\n"
        "import realsr_ncnn_vulkan_amd as R\n"
        "from realsr_ncnn_vulkan_amd import synth\n"
        "srs = []\n"
        "for _ in range(3):\n"
        "    s = R.RealSR(0); s.load(%r, %r); s.tilesize = 32; srs.append(s)\n"
        "img = synth.make_image(9, 120, 70)\n"
        "want = srs[0].process(img)\n"
        "got = R.process_group(srs, img)\n"
        "assert (got == want).all()\n"
        "print('inline', int(srs[0].get_stat('pool_inline_runs')), 'workers', int(srs[0].get_stat('pool_workers')))\n"
    ) % (ROOT, paths[0], paths[1])
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    assert "inline 2 workers 0" in r.stdout, r.stdout


def test_create_group(paths, monkeypatch):
    """rsr_create_group: parse + pack once, one context per GPU (one GPU here: no collective needed); a duplicate id and a
    missing device are argument / device errors and leave no context behind."""
    monkeypatch.delenv("RSR_GROUP_FORCE_RCCL", raising=False)
    srs, transport = R.create_group([0], *paths)
    assert len(srs) == 1 and transport.startswith("host")
    srs[0].tilesize = 32
    img = synth.make_image(57, 40, 30)
    ref = R.RealSR(0)
    ref.load(*paths)
    ref.tilesize = 32
    assert (srs[0].process(img) == ref.process(img)).all()
    ref.close()
    srs[0].close()
    with pytest.raises(R.RealSRError) as e:
        R.create_group([0, 0], *paths)
    assert e.value.code == R.RSR_E_ARG
    import torch
    if torch.cuda.device_count() == 1:
        with pytest.raises(R.RealSRError) as e:
            R.create_group([0, 1], *paths)
        assert e.value.code == R.RSR_E_DEVICE
    else:  # a multi-GPU box: the real thing, weights by RCCL broadcast
        srs, transport = R.create_group([0, 1], *paths)
        assert transport == "rccl", transport
        for s in srs:
            s.tilesize = 32
        big = synth.make_image(58, 70, 150)
        one = srs[0].process(big)
        assert (srs[1].process(big) == one).all()
        assert (R.process_group(srs, big) == one).all()
        for s in srs:
            s.close()


def test_create_group_through_rccl_on_one_gpu(paths, monkeypatch):
    """The RCCL branch of rsr_create_group (group.cpp: dlopen librccl, ncclCommInitAll, one grouped ncclBroadcast of the 33.5 MB
    packed model, stream sync, ncclCommDestroy, load from the DEVICE copy) executed on the one GPU this box has:
    RSR_GROUP_FORCE_RCCL=1 makes n == 1 take it with a communicator of one rank and an in-place broadcast.  The transport must
    say "rccl" (a failure anywhere falls back to "host (rccl unavailable: ...)" and fails this test) and the context must give
    the bytes of a context loaded from the files.  Reference semantics: one RealSR + load per GPU id, main.cpp:778-791."""
    assert R.rccl_probe() is None
    monkeypatch.setenv("RSR_GROUP_FORCE_RCCL", "1")
    srs, transport = R.create_group([0], *paths)
    assert transport == "rccl", transport
    ref = R.RealSR(0)
    ref.load(*paths)
    img = synth.make_image(57, 90, 70)
    for T in (32, 64):
        srs[0].tilesize = ref.tilesize = T
        assert (srs[0].process(img) == ref.process(img)).all()
    # and the single-image split over "several" members created that way (the same GPU twice is refused by create_group:
    # the second member is a plain context)
    srs[0].tilesize = ref.tilesize = 32
    assert (R.process_group([srs[0], ref, srs[0]], img) == ref.process(img)).all()
    ref.close()
    srs[0].close()


def test_real_model_harness_gpu_legs(model_dir, tmp_path):
    """tools/check_real_model.py on the synthetic stand-in (the real x4.bin is absent from the reference checkout,
    /root/reference/.MISSING_LARGE_BLOBS): encoding by size, pack, fp16 activation-range guard, pre-quantise error, BASELINE C1
    whole frame +-1 against the oracle, the C2 bench leg -- the path a user-supplied models-DF2K/x4.bin takes."""
    out = tmp_path / "rep.json"
    env = {k: v for k, v in os.environ.items() if k != "RSR_NO_TORCH"}  # (the in-process oracle pool sets it for CPU-only children)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_real_model.py"), model_dir, "--json", str(out)],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "RESULT: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    rep = json.loads(out.read_text())
    assert rep["c1"]["max_diff"] <= 1 and rep["pre_quantise"]["max"] <= 3.0e-3 and rep["c2_bench"]["mpix_per_s"] > 50
    assert rep["recommended_mode"] == "default" and rep["pre_quantise"]["headroom"] >= 1.5


def test_real_model_harness_recommends_precise_mode_for_wide_swing_weights(tmp_path):
    """The stand-in fp16 storage cannot hold the bar on (log-normal channel gains, output swing -0.56 .. 1.79: one byte of C1 off by 2,
    profiles/r05_fp16_storage.txt): the harness measures a headroom below 1.5, switches the engine to precise mode, and passes C1 +-1 there."""
    d = synth.make_model_dir(str(tmp_path), "models-spread-wide", 45, chan_sigma=1.0, last_gain=0.2)
    out = tmp_path / "rep.json"
    env = {k: v for k, v in os.environ.items() if k != "RSR_NO_TORCH"}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_real_model.py"), d, "--json", str(out), "--no-bench"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "RESULT: ok" in r.stdout and "switching to PRECISE mode" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    rep = json.loads(out.read_text())
    assert rep["recommended_mode"] == "precise" and rep["pre_quantise"]["headroom"] < 1.5 and rep["pre_quantise_precise"]["headroom"] >= 1.5
    assert rep["c1"]["max_diff"] <= 1


# ---- bench.py's multi-rank control flow, executed on ONE gpu (the driver's 8-GPU run is the first real one otherwise) ----------
def test_bench_multirank_control_flow_on_one_gpu(tmp_path):
    """`python bench.py --gpus 2` with no torch.distributed environment (the driver's command shape) must start two ranks itself
    and report n_gpus == 2; RSR_BENCH_SAME_GPU puts both on cuda:0 over gloo.  Behind the rank run, rank 0 runs the product's
    own multi-GPU path (group mode: contexts + proc threads on a shared queue + rsr_process_group) in a child process."""
    env = dict(os.environ, RSR_BENCH_SAME_GPU="1", RSR_BENCH_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    j = json.loads(line)
    assert j["n_gpus"] == 2 and j["steps"] == 2 and j["value"] > 0 and j["scaling"] == "weak"
    assert "2 ranks" in j["config"]["parallelism"]
    g = j["group_mode"]
    assert g.get("value"), g
    assert g["n_gpus"] == 2 and sum(g["config"]["frames_per_gpu"]) == g["frames"]
    assert g["single_image_over_group"]["bytes_equal_single_context"] is True
    # the driver's own launch shape (torch.distributed.run around the script) still works, and a world size that does not match
    # --gpus is refused instead of being reported as something else
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29517", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1",
           "--no-cpu-baseline", "--no-host", "--no-group"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["n_gpus"] == 2


@pytest.mark.gpu
def test_device_memory_query_feeds_the_tile_policy():
    """rsr_device_memory = the heap budget behind the CLI's automatic tile size (main.cpp:761-774): an MI355X reports its
    288 GB, far above the 1900 MB that selects tile 200; a device that does not exist is an error, not a crash."""
    free_mb, total_mb = R.device_memory(0)
    assert total_mb > 200 * 1024 and 1900 < free_mb <= total_mb
    with pytest.raises(R.RealSRError):
        R.device_memory(97)
