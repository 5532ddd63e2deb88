"""The host video session on the GPU (run with -m gpu): R.Video -- rsr_video_open / send / ready / receive / flush / reset / info / close.

Everything is EXACT.  The definition of output frame k is

    planes_ref.unpack(rsr_process_device_fmt(planes_ref.pack(frame k)))

in the context's current mode, whatever the window size and whatever came before; the reference is computed with the plain call of
tests/gpu_support.py (run), once per distinct frame.  The frames are 36 x 26 at tile 16, prepadding 10: 3 x 2 tiles.  The script is a
random frame, a repeat, one luma sample changed, one chroma sample changed, a repeat, an all-new frame, a repeat -- at window 3 that is
runs of 3, 3 and a flushed 1."""
from fractions import Fraction

import numpy as np
import pytest

import realsr_ncnn_vulkan_amd as R

import pixfmt_ref as F
import planes_ref as P
import tile_diff_ref as ref
from gpu_support import context_fixtures, paths, run  # noqa: F401

pytestmark = pytest.mark.gpu
W, H, T, PAD = 36, 26, 16, 10
NT = 6
ctxs, ctx = context_fixtures(T, PAD)


def script(fmt, w=W, h=H, seed=0):
    """The seven frames, each a (y, u, v) triple."""
    a = P.frame(seed + 1, fmt, w, h)
    b = tuple(p.copy() for p in a)
    b[0][h - 3, w - 2] ^= 1  # one luma sample, in the last tile
    c = tuple(p.copy() for p in b)
    c[1][0, 0] ^= 1          # one chroma sample, in the first tile
    d = P.frame(seed + 2, fmt, w, h)
    return [a, a, b, c, c, d, d]


class Definition:
    """unpack(plain call(pack(frame))) on the context as it stands, computed once per distinct frame."""

    def __init__(self, s, fmt, w, h):
        self.s, self.fmt, self.w, self.h, self.seen = s, fmt, w, h, {}
        self.ow, self.oh = s.out_size_fmt(fmt, w, h)

    def __call__(self, frame):
        key = b"".join(p.tobytes() for p in frame)
        if key not in self.seen:
            out = run(self.s, P.pack(self.fmt, *frame), self.fmt, self.fmt)
            self.seen[key] = P.unpack(self.fmt, out, self.ow, self.oh)
        return self.seen[key]


def expected_runs(fmt, frames, window, first=None):
    """Tiles run per window: the masks of tests/tile_diff_ref.py over the packed surfaces, all tiles where a frame has no predecessor."""
    runs, prev = [], first
    for k0 in range(0, len(frames), window):
        n = 0
        for f in frames[k0:k0 + window]:
            cur = P.pack(fmt, *f)
            n += NT if prev is None else int(ref.diff_mask(fmt, prev, cur, T, PAD).sum())
            prev = cur
        runs.append(n)
    return runs


def play(s, v, frames, window):
    """Send the frames, receive every window when it is ready, flush the rest: (outputs, tiles run per window)."""
    outs, runs = [], []

    def drain(before):
        assert v.ready == min(window, len(frames) - len(outs))
        while v.ready:
            outs.append(v.receive())
        runs.append(int(s.get_stat("video_tiles_run")) - before)

    before = int(s.get_stat("video_tiles_run"))
    for k, f in enumerate(frames):
        assert v.ready == 0
        v.send(*f)
        if (k + 1) % window == 0:
            drain(before)
            before = int(s.get_stat("video_tiles_run"))
    if len(frames) % window:
        assert v.ready == 0
        v.flush()
        drain(before)
    v.flush()  # nothing pending: RSR_OK
    return outs, runs


def same(got, want):
    return len(got) == 3 and all(g.dtype == w_.dtype and np.array_equal(g, w_) for g, w_ in zip(got, want))


@pytest.mark.parametrize("fmt,w,h", [(F.NV12, W, H), (F.P010, W, H), (F.NV16, W, H), (F.YUV444P10, W, H), (F.YUV444P, 35, 25)],
                         ids=["nv12", "p010", "nv16", "yuv444p10", "yuv444p-35x25"])
def test_the_script_at_window_3(ctx, fmt, w, h):
    s = ctx[False]
    frames, want = script(fmt, w, h, seed=fmt), Definition(s, fmt, w, h)
    stats0 = {k: int(s.get_stat(k)) for k in ("video_frames", "video_windows", "video_tiles_run", "video_tiles_skipped")}
    v = R.Video(s, fmt, w, h, window=3)
    try:
        assert v.window == 3 and v.out_size == (4 * w, 4 * h)
        outs, runs = play(s, v, frames, 3)
    finally:
        v.close()
    assert len(outs) == 7 and all(same(o, want(f)) for o, f in zip(outs, frames))
    assert len(want.seen) == 4 and len(np.unique(outs[0][0])) > 16
    assert not same(outs[4], outs[5])
    # the luma sample lies in the halo of several tiles, the chroma sample in one tile alone; a repeat runs nothing
    assert runs == expected_runs(fmt, frames, 3) and NT < runs[0] < 2 * NT and runs[1] == 1 + NT and runs[2] == 0
    got = {k: int(s.get_stat(k)) - n for k, n in stats0.items()}
    assert got == {"video_frames": 7, "video_windows": 3, "video_tiles_run": sum(runs), "video_tiles_skipped": 7 * NT - sum(runs)}


def test_every_window_size_gives_the_same_bytes(ctx):
    s = ctx[False]
    frames, want = script(F.NV12), Definition(s, F.NV12, W, H)
    for window in (1, 3, 16):
        v = R.Video(s, F.NV12, W, H, window=window)
        try:
            assert v.window == window
            outs, runs = play(s, v, frames, window)
        finally:
            v.close()
        assert all(same(o, want(f)) for o, f in zip(outs, frames)), window
        assert runs == expected_runs(F.NV12, frames, window) and sum(runs) == sum(expected_runs(F.NV12, frames, 1)), window
    v = R.Video(s, F.NV12, W, H)  # window 0 means 8
    assert v.window == 8
    v.close()
    for bad in (-1, 17):
        with pytest.raises(R.RealSRError) as e:
            R.Video(s, F.NV12, W, H, window=bad)
        assert e.value.code == R.RSR_E_ARG
    for bad_fmt in (F.U8, F.F16, 3, 14):
        with pytest.raises(R.RealSRError) as e:
            R.Video(s, bad_fmt, W, H)
        assert e.value.code == R.RSR_E_ARG
    with pytest.raises(R.RealSRError) as e:
        R.Video(s, F.NV12, W - 1, H)  # the parity rule of the input
    assert e.value.code == R.RSR_E_ARG


def test_reset_runs_all_tiles_and_a_plain_call_between_windows_changes_nothing(ctx):
    s = ctx[False]
    frames, want = script(F.P010), Definition(s, F.P010, W, H)
    v = R.Video(s, F.P010, W, H, window=2)
    try:
        t0 = int(s.get_stat("video_tiles_run"))
        v.send(*frames[0])
        v.send(*frames[1])
        a = [v.receive(), v.receive()]
        assert int(s.get_stat("video_tiles_run")) - t0 == NT
        other = run(s, F.u8_image(3, 40, 30), F.U8, F.U8)  # a plain call of another geometry between two windows
        v.send(*frames[1])
        v.send(*frames[2])
        b = [v.receive(), v.receive()]
        changed = int(ref.diff_mask(F.P010, P.pack(F.P010, *frames[1]), P.pack(F.P010, *frames[2]), T, PAD).sum())
        assert 0 < changed < NT and int(s.get_stat("video_tiles_run")) - t0 == NT + changed
        assert np.array_equal(other, run(s, F.u8_image(3, 40, 30), F.U8, F.U8))
        v.reset()
        v.send(*frames[2])  # the frame the session saw last: after a reset it is compared with nothing
        v.flush()
        c = v.receive()
        assert int(s.get_stat("video_tiles_run")) - t0 == 2 * NT + changed
    finally:
        v.close()
    assert same(a[0], want(frames[0])) and same(a[1], want(frames[1])) and same(b[0], want(frames[1])) and same(b[1], want(frames[2])) and same(c, want(frames[2]))


@pytest.mark.parametrize("mode", ["out_scale2", "ratio3/2", "tta", "precise"])
def test_modes(ctx, mode):
    s = ctx[mode == "tta"]
    w, h = W, H
    if mode == "out_scale2":
        s.out_scale = 2
    elif mode == "precise":
        s.set_option("precise", 1)
    elif mode == "ratio3/2":
        s.out_ratio = Fraction(3, 2)
        with pytest.raises(R.RealSRError) as e:  # 26 * 3 / 2 = 39 rows: no 4:2:0 surface
            R.Video(s, F.NV12, 36, 26, window=3)
        assert e.value.code == R.RSR_E_ARG and "YUV" in str(e.value)
        h = 28
    try:
        frames, want = script(F.NV12, w, h, seed=7)[:4], Definition(s, F.NV12, w, h)
        v = R.Video(s, F.NV12, w, h, window=3)
        try:
            assert v.out_size == {"out_scale2": (72, 52), "ratio3/2": (54, 42)}.get(mode, (4 * w, 4 * h))
            outs, runs = play(s, v, frames, 3)
        finally:
            v.close()
        assert all(same(o, want(f)) for o, f in zip(outs, frames))
        assert runs == expected_runs(F.NV12, frames, 3) and runs[1] == 1
    finally:
        s.out_scale = 4


def canvas_planes(fmt, w, h, fill, pinned, keep):
    """Three planes as views into larger arrays of `fill` -- pageable, or pinned (rsr_host_alloc): (views, backing arrays)."""
    dt = np.dtype(F.NP[fmt])
    (yh, yw), (ch, cw), _ = P.plane_shapes(fmt, w, h)

    def backing(shape):
        if not pinned:
            return np.full(shape, fill, dtype=dt)
        m = R.PinnedArray((int(np.prod(shape)) * dt.itemsize,))
        keep.append(m)
        a = m.array.view(dt).reshape(shape)
        a[...] = fill
        return a

    by, bc = backing((yh + 2, yw + 5)), backing((2, ch + 3, cw + 3))
    return (by[1:yh + 1, 2:yw + 2], bc[0, 1:ch + 1, 3:cw + 3], bc[1, 1:ch + 1, 3:cw + 3]), (by, bc)


@pytest.mark.parametrize("fmt", [F.NV12, F.P210], ids=["nv12", "p210"])
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_pitched_host_planes_on_both_sides(ctx, fmt, pinned):
    s = ctx[False]
    frames, want = script(fmt, seed=11)[:3], Definition(s, fmt, W, H)
    fill = 0xCD if F.ES[fmt] == 1 else 0xCDCD
    keep = []
    v = R.Video(s, fmt, W, H, window=3)
    try:
        for f in frames:
            views, _ = canvas_planes(fmt, W, H, fill, pinned, keep)
            assert views[0].strides[0] % 16 and not views[0].flags.c_contiguous
            for dst, src in zip(views, f):
                dst[...] = src
            v.send(*views)
        for f in frames:
            views, backs = canvas_planes(fmt, v.out_size[0], v.out_size[1], fill, pinned, keep)
            got = v.receive(views)
            assert all(g is x for g, x in zip(got, views)) and same(got, want(f))
            for x in views:  # nothing but the rows of the planes was written
                x[...] = fill
            assert all((b == fill).all() for b in backs)
    finally:
        v.close()
        for m in keep:
            m.free()


def test_state_errors(ctx):
    s = ctx[False]
    frames = script(F.NV12)
    v = R.Video(s, F.NV12, W, H, window=2)
    try:
        def state(fn, *a):
            with pytest.raises(R.RealSRError) as e:
                fn(*a)
            assert e.value.code == R.RSR_E_STATE
        state(v.receive)                  # none ready
        v.flush()                         # nothing pending: fine
        v.send(*frames[0])
        state(v.receive)                  # one pending, none ready
        state(v.reset)                    # frames are pending
        v.send(*frames[1])
        assert v.ready == 2
        state(v.send, *frames[2])         # ready frames remain
        first = v.receive()
        state(v.send, *frames[2])
        v.receive()
        state(v.receive)
        with pytest.raises(ValueError):
            v.send(frames[0][0], frames[0][1], frames[0][2][:, :-1])
        with pytest.raises(ValueError):
            v.send(*(p.astype(np.uint16) for p in frames[0]))
        assert v.ready == 0
        s.out_scale = 2                   # the output size changes under the session
        state(v.send, *frames[2])
        s.out_scale = 4
        v.send(*frames[2])
        s.tilesize = 32
        state(v.flush)
        s.tilesize = T
        v.flush()
        assert v.ready == 1 and first[0].shape == (4 * H, 4 * W)
    finally:
        s.tilesize = T
        v.close()
    with pytest.raises(R.RealSRError) as e:
        v.send(*frames[0])
    assert e.value.code == R.RSR_E_STATE


@pytest.mark.parametrize("option,value", [("yuv_matrix", 601), ("yuv_range", 1), ("precise", 1), ("yuv_siting", 1)])
def test_a_mode_change_between_windows_carries_nothing_over(ctx, option, value):
    """Unchanged tiles are copied from the output of the window before -- unless that was computed in another mode: then the window's first
    frame is compared with nothing, and every frame is again what the plain call makes of it in the mode its window runs in."""
    s = ctx[False]
    frames = script(F.NV12, seed=21)
    v = R.Video(s, F.NV12, W, H, window=2)
    try:
        old = Definition(s, F.NV12, W, H)
        v.send(*frames[0])
        v.send(*frames[1])
        a = [v.receive(), v.receive()]
        assert same(a[0], old(frames[0])) and same(a[1], old(frames[1]))
        t0 = int(s.get_stat("video_tiles_run"))
        s.set_option(option, value)
        new = Definition(s, F.NV12, W, H)
        v.send(*frames[1])  # a repeat of the last frame: nothing would run
        v.send(*frames[2])
        b = [v.receive(), v.receive()]
        changed = int(ref.diff_mask(F.NV12, P.pack(F.NV12, *frames[1]), P.pack(F.NV12, *frames[2]), T, PAD).sum())
        assert int(s.get_stat("video_tiles_run")) - t0 == NT + changed
        assert same(b[0], new(frames[1])) and same(b[1], new(frames[2]))
        assert option == "yuv_siting" or not same(b[0], a[1])  # (the mode shows in the bytes)
    finally:
        v.close()


def test_closing_the_context_closes_its_sessions(paths):
    s = R.RealSR(0)
    s.load(*paths)
    s.tilesize, s.prepadding = T, PAD
    v = R.Video(s, F.NV12, W, H, window=2)
    v.send(*script(F.NV12)[0])
    s.close()
    assert v._h is None
    v.close()
    with pytest.raises(R.RealSRError):
        v.flush()
