"""The conditions on the inputs of tests/test_gpu_far_addressing.py, checked where there is no GPU: every far layout (tests/far_layout.py) is
admitted by the library with the span the helper computes, crosses 2^31 and 2^32 where a tile rectangle is in the middle of its rows, and
keeps every 32-bit narrowing of every byte offset inside the arena and away from the byte itself -- so that a kernel with a dropped cast
fails a comparison instead of faulting -- and the module's memory stays under its cap.  The last test is a numpy model of a gather and
a scatter through the narrowed offsets: the proof that the GPU comparisons can fail.

What does NOT hold, and is therefore not asserted: that a narrowed offset never falls on a byte of a window.  With the pitches used here
(h - 6) * P - 2^32 is small (32 .. 424 bytes for the pitches that are multiples of 4), so the wrapped offset of a byte of row y >= h - 6 lies in row y - (h - 6) of the same window, that
many bytes to the right; plane 2 of a Pn layout wraps into plane 0, the UV plane into Y, row 2 of layout M into row 0.  What holds, and
is asserted: such a byte belongs to another row or plane than the one it was meant for, i.e. to other pixels of a seeded random image.
The model shows that the compared bytes change either way."""
import numpy as np
import pytest

import realsr_ncnn_vulkan_amd as R

import far_layout as fl
from far_layout import B31, B32, BASE, F16, F32, NV12, P010, U8

GROUPS = fl.catalogue()
IDS = ["%s-f%dc%d%s-%dx%d" % (g[0].kind, g[0].fmt, g[0].c, "odd" if g[0].odd else "", g[0].w, g[0].h) for g in GROUPS]
ARENA = fl.arena_bytes()


def test_the_pitches_are_the_stated_ones():
    assert fl.SIZES == [(208, 176), (104, 88), (78, 66), (52, 44)]
    assert [fl.far_row_pitch(U8, h) for h in (176, 88, 66, 44)] == [25264516, 52377652, 71582792, 113025456]
    for h, (r31, r32) in zip((176, 88, 66, 44), ((85, 170), (41, 82), (30, 60), (19, 38))):
        p = fl.far_row_pitch(U8, h)
        assert (r31 - 1) * p < B31 <= r31 * p and (r32 - 1) * p < B32 <= r32 * p and (h - 6) * p >= B32 > (h - 6) * (p - 4)
    for c in (3, 4):
        for h in (176, 88, 66, 44):
            p = fl.far_row_pitch(U8, h, c, odd=True)
            assert p % 4 == 1 and p % c and (h - 6) * p >= B32 and p - fl.far_row_pitch(U8, h) < 12
    for fmt in (F16, F32, P010):
        for h in (176, 88, 66, 44):
            assert fl.far_row_pitch(fmt, h) % fl.ES[fmt] == 0 and (h - 6) * fl.far_row_pitch(fmt, h) >= B32
    assert fl.layout("Pn", F32, 208, 176) == (208 * 4 + 16, B31 + 4096) and fl.layout("Pn", NV12, 52, 44) == (52 + 16, B32 + 4096)
    assert fl.layout("M", U8, 52, 3)[0] == B31 - 1 and fl.layout("M", F16, 52, 3)[0] == B31 - 4 and fl.layout("M", F32, 52, 3)[0] == B31 - 4
    spans = [wn.span for g in GROUPS if g[0].kind == "R" for wn in g[:1]]
    assert 4.1 * fl.GIB <= min(spans) and max(spans) <= 4.65 * fl.GIB, (min(spans) / fl.GIB, max(spans) / fl.GIB)  # 4.12 .. 4.53 GiB
    # windows 0 | 1 co-aligned to 16 bytes; 1 | 2 agree modulo 4 only; 2 | 3 modulo the element size only
    for fmt in (U8, F16, F32):
        for kind in ("R", "Pn"):
            c = fl.cols(fmt, kind)
            assert (c[1] - c[0]) % 16 == 0 and (c[2] - c[1]) % 16 == 4 and (c[3] - c[2]) % 4 == fl.ES[fmt] % 4 and all(v % fl.ES[fmt] == 0 for v in c)


@pytest.mark.parametrize("g", GROUPS, ids=IDS)
def test_the_library_admits_the_layout_with_the_helpers_span(g):
    for wn in g:
        assert R.image_span(wn.fmt, wn.w, wn.h, wn.c, wn.row_pitch, wn.plane_pitch) == wn.span == fl.span(wn.fmt, wn.w, wn.h, wn.c, wn.row_pitch, wn.plane_pitch)
        far, rest = wn.offsets()
        assert far.size == wn.nbytes and int((far + rest).max()) + 1 == wn.span and int((far + rest).min()) == 0
        assert int((far + rest).max()) >= B32  # every window has bytes beyond 2^32


def inside_not_first(y, spans):
    """Does row y lie inside one of the rectangles' row spans, and on the first row of none that holds it?"""
    holds = [s for s in spans if s[0] <= y < s[1]]
    return bool(holds) and all(y != s[0] for s in holds)


@pytest.mark.parametrize("g", GROUPS, ids=IDS)
def test_the_crossings_lie_inside_tile_rectangles(g):
    """The first row, plane or UV row beyond 2^31 and beyond 2^32 exists; a row lies inside a tile rectangle and is not its first row
    (layout M: the crossing is inside row 2, and inside row 1).  One exception, asserted as such: the UV plane of the 44-row surface in
    layout R crosses 2^32 at chroma row 16, the first of the lower x1 OUTPUT rectangles [16, 22); it is the sixth row of the lower source
    rectangle [11, 22), so the surface as an input -- and its Y row 38 on either side -- still answers."""
    wn = g[0]
    found = fl.crossings(wn)
    assert {B for B, _, _, _ in found} == {B31, B32}, found
    if wn.kind == "M":
        last = (1, 0) if fl.is_yuv(wn.fmt) else (0, 2)
        assert (B32, "mid") + last in found and (B31, "mid", 0, 1) in found
        return
    if wn.kind == "Pn":
        want = {(B31, "plane", 1, 0), (B32, "plane", 1, 0)} if fl.is_yuv(wn.fmt) else {(B31, "plane", 1, 0), (B32, "plane", 2, 0)}
        assert want <= set(found), found
        return
    rows = [f for f in found if f[1] == "row"]
    assert {(B, q) for B, _, q, _ in rows} >= ({(B31, 0), (B32, 0), (B32, 1)} if fl.is_yuv(wn.fmt) else {(B31, 0), (B32, 0)}), found
    assert not [f for f in found if f[1] == "mid"]
    for B, _, q, y in rows:
        spans = fl.rect_rows(wn.h)
        if fl.is_yuv(wn.fmt) and q == 1:
            spans = [(a // 2, b // 2) for a, b in spans]
        if fl.is_yuv(wn.fmt) and q == 1 and wn.h == fl.H and B == B32:
            assert y == 16 and not inside_not_first(y, spans) and inside_not_first(y, spans[2:]) and spans[3] == (11, 22)
        else:
            assert inside_not_first(y, spans), (B, q, y, spans)


@pytest.mark.parametrize("g", GROUPS, ids=IDS)
def test_every_narrowed_offset_stays_inside_the_arena_and_off_its_byte(g):
    true = []
    for wn in g:
        far, rest = wn.offsets()
        true.append(far + rest + wn.col)
        assert wn.col + wn.span <= ARENA - BASE - 4096
    for k, wn in enumerate(g):
        far, rest = wn.offsets()
        total = far + rest
        zext, sext, prod = fl.alias32(far, rest)
        for a in (zext, sext, prod):
            at = a + wn.col  # from the arena's image base
            assert int(at.min()) >= -BASE and int(at.max()) < ARENA - BASE - 4096
        assert np.array_equal(zext != total, total >= B32) and np.array_equal(sext != total, total >= B31) and np.array_equal(prod != total, far >= B31)
        assert np.all(np.abs(zext - total) % B32 == 0) and np.all(np.abs(sext - total) % B32 == 0) and np.all(np.abs(prod - total) % B32 == 0)
        # A narrowed offset that falls on a byte of a window of the arena falls into another row or plane than its own (see the module's
        # docstring): no two bytes of one row, of this window or of the same row of a neighbour, lie a multiple of 2^32 apart.
        row_id = np.repeat(np.arange(len(wn.row_starts())), wn.rowbytes)
        for a in (zext, sext, prod):
            moved = a != total
            for j, other in enumerate(true):
                hit = np.isin(a[moved] + wn.col, other)
                if hit.any():  # (packed order is address order only within a row: look the row up through a sorted copy)
                    order = np.argsort(other, kind="stable")
                    landed_row = row_id[order[np.searchsorted(other[order], (a[moved] + wn.col)[hit])]]
                    assert np.all(landed_row != row_id[moved][hit]), (k, j)


def test_the_memory_cap_holds():
    assert ARENA % 4096 == 0 and ARENA >= BASE + B32 + 4096
    assert fl.held_bytes() == 2 * ARENA + fl.TEMPORARIES <= fl.CAP
    assert fl.memory_skip_reason(fl.held_bytes() + fl.HEADROOM) is None
    why = fl.memory_skip_reason(8 * fl.GIB)
    assert why and "8.00 GiB" in why and "%.2f GiB" % ((fl.held_bytes() + fl.HEADROOM) / fl.GIB) in why
    # the largest temporary of scan(): the comparison result of one chunk
    assert fl.SCAN_CHUNK <= 256 << 20 and fl.SCAN_CHUNK // 8 + 3 * 4 * 208 * 176 * 4 <= fl.TEMPORARIES


def test_alias32():
    assert fl.alias32(5) == (5, 5, 5)
    assert fl.alias32(B31) == (B31, -B31, -B31) and fl.alias32(B31 - 1, 1) == (B31, -B31, B31)
    assert fl.alias32(B32 + 7) == (7, 7, 7) and fl.alias32(B32 - 2, 5) == (3, 3, 3) and fl.alias32(3 * B31 + 9, 1) == (B31 + 10, -B31 + 10, -B31 + 10)


# ---- the model: a gather and a scatter through narrowed offsets -----------------------------------------------------------------------------
MODEL = [g for g in GROUPS if (g[0].w, g[0].h) in ((fl.W, fl.H), (208, 176), fl.m_size(g[0].fmt)) and (g[0].fmt, g[0].c) in ((U8, 3), (F32, 3), (NV12, 3))]


@pytest.mark.parametrize("g", MODEL, ids=[i for i, g in zip(IDS, GROUPS) if g in MODEL])
def test_a_narrowed_gather_or_scatter_changes_the_compared_bytes(g):
    """Two windows of a sparse arena hold two seeded random images.  A correct gather returns the image and a correct scatter leaves it in
    the window and 0xCD everywhere else: the GPU module's one assertion.  With the offsets of window 0 narrowed in any of the three ways
    the gathered bytes differ from the image, and the scattered image is missing from its window or has left 0xCD changed outside it."""
    x = [fl.raw(fl.image(40 + k, wn.fmt, wn.w, wn.h, wn.c)) for k, wn in enumerate(g[:2])]
    offs = [wn.offsets() for wn in g[:2]]
    true = [far + rest + wn.col for (far, rest), wn in zip(offs, g[:2])]
    every = np.concatenate(true)

    def filled():
        a = fl.SparseArena(ARENA)
        for t, v in zip(true, x):
            a.write(t, v)
        return a

    a = filled()
    assert np.array_equal(a.read(true[0]), x[0]) and np.array_equal(a.read(true[1]), x[1]) and a.untouched_outside(every)
    far, rest = offs[0]
    for form, narrowed in zip(("zext", "sext", "prod"), fl.alias32(far, rest)):
        at = narrowed + g[0].col
        assert not np.array_equal(filled().read(at), x[0]), form  # the gather
        a = fl.SparseArena(ARENA)
        a.write(true[1], x[1])
        a.write(at, x[0])  # the scatter
        got = [a.read(t) for t in true]
        assert not (np.array_equal(got[0], x[0]) and np.array_equal(got[1], x[1])), form
        assert np.count_nonzero(got[0] != x[0]) >= np.count_nonzero(narrowed != far + rest) * 9 // 10, form  # (a byte in 256 may agree by chance)
