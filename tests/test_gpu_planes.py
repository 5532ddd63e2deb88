"""rsr_pack_planes / rsr_unpack_planes on the GPU (run with -m gpu): the three planes of a yuv420p / yuv422p / yuv444p frame (8 and 10
bits) to the surface of an RSR_FMT_* and back, against tests/planes_ref.py.  Everything is EXACT: np.array_equal on whole byte canvases,
so a byte written outside the rows of a destination fails a test as surely as a wrong sample.

Widths 2, 4, 18, 34, 66, 130 give chroma rows of 1, 2, 9, 17, 33, 65 samples: below, at and beyond a 16-byte piece and a 64-lane step.
Every geometry runs in four layouts, which between them take every access width of the kernels:
  packed     tight planes and surfaces at the allocator's alignment, pitches passed as 0: 16-byte pieces
  offset     everything at byte offset 1 (8-bit) / 2 (16-bit) with pitches that are no multiple of 16: single samples for the UV rows
  coaligned  addresses that agree modulo 16 (Y) and, halved, modulo 8 (UV against U and V) but sit 4 bytes off: 16-byte pieces with a head
  mid        addresses that agree modulo 4 / 2 only: 4-byte pieces"""
import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

import planes_ref as P
from gpu_support import context_fixtures, dev, paths, run  # noqa: F401
import pixfmt_ref as F

pytestmark = pytest.mark.gpu
T, PAD = 16, 10
ctxs, ctx = context_fixtures(T, PAD)
WIDTHS, HEIGHTS = (2, 4, 18, 34, 66, 130), (2, 26, 3)
LAYOUTS = ("packed", "offset", "coaligned", "mid")
IDS = {F.NV12: "nv12", F.P010: "p010", F.NV16: "nv16", F.P210: "p210", F.YUV444P: "yuv444p", F.YUV444P10: "yuv444p10"}
SLACK = 48  # sentinel bytes behind the last row of every canvas


def up(n, m):
    return (n + m - 1) // m * m


def geometry(fmt, w, h, layout):
    """(surface offset, row pitch, plane pitch; y offset, y pitch; u offset, v offset, chroma pitch) in bytes -- and the pitches as they
    are passed: 0 where the layout is the packed one."""
    es = F.ES[fmt]
    cw, ch = P.chroma_dims(fmt, w, h)
    yrow, crow = w * es, cw * es
    if layout == "packed":
        return dict(so=0, sp=yrow, spl=h * yrow, yo=0, yp=yrow, uo=0, vo=0, cp=crow, passed=(0, 0, 0, 0))
    if layout == "offset":
        odd16 = lambda n: n + 6 if (n + 6) % 16 else n + 10
        sp = odd16(yrow)
        g = dict(so=es, sp=sp, spl=h * sp + 10, yo=es, yp=odd16(yrow + 4), uo=es, vo=es, cp=odd16(crow))
    elif layout == "coaligned":
        sp = up(yrow, 16) + 16
        g = dict(so=4, sp=sp, spl=h * sp + 32, yo=20, yp=up(yrow, 16) + 32, uo=2, vo=10, cp=up(crow, 8) + 8)
    else:
        sp = up(yrow, 16) + 16
        g = dict(so=4, sp=sp, spl=h * sp + 32, yo=8, yp=up(yrow, 16) + 32, uo=4, vo=6, cp=up(crow, 8) + 8)
    g["passed"] = (g["sp"], g["spl"], g["yp"], g["cp"])
    return g


def plane_canvas(rows, off, pitch):
    return np.full(off + rows * pitch + SLACK, 0xCD, dtype=np.uint8)


def put(canvas, off, pitch, plane):
    rows = np.ascontiguousarray(plane).view(np.uint8).reshape(plane.shape[0], -1)
    for r, row in enumerate(rows):
        canvas[off + r * pitch:off + r * pitch + row.size] = row
    return canvas


class Frame:
    """One frame of one geometry and layout: the canvases of its three planes and of its surface, on the host and on the device."""

    def __init__(self, seed, fmt, w, h, layout, pack):
        self.fmt, self.w, self.h, self.g = fmt, w, h, geometry(fmt, w, h, layout)
        g, (cw, ch) = self.g, P.chroma_dims(fmt, w, h)
        self.planes = P.frame(seed, fmt, w, h, dirty=True)
        self.surface = P.pack(fmt, *self.planes) if pack else F.image(seed, fmt, w, h) | (F.ES[fmt] == 2 and 0x15)  # (low bits set: no codes)
        if not pack:
            self.surface = self.surface.astype(F.NP[fmt])
            self.planes = P.unpack(fmt, self.surface, w, h)
        self.offs = (g["yo"], g["uo"], g["vo"])
        self.pitches = (g["yp"], g["cp"], g["cp"])
        rows = (h, ch, ch)
        nplanes = 3 if F.TABLE[fmt].kind == F.PLANAR else 2
        span = g["so"] + (nplanes - 1) * g["spl"] + F.plane_rows(fmt, h)[-1] * g["sp"] + SLACK
        self.want_planes = [put(plane_canvas(r, o, p), o, p, pl) for r, o, p, pl in zip(rows, self.offs, self.pitches, self.planes)]
        self.want_surface = np.full(span, 0xCD, dtype=np.uint8)
        F.place(self.want_surface, g["so"], g["sp"], g["spl"], self.surface, fmt)
        # the sources hold the data, the destinations 0xCD
        self.d_planes = [dev(c if pack else np.full_like(c, 0xCD)) for c in self.want_planes]
        self.d_surface = dev(np.full_like(self.want_surface, 0xCD) if pack else self.want_surface)

    def planes_arg(self):
        sp, spl, yp, cp = self.g["passed"]
        return tuple(d.data_ptr() + o for d, o in zip(self.d_planes, self.offs)) + (yp, cp)

    def surface_arg(self):
        sp, spl, yp, cp = self.g["passed"]
        return (self.d_surface.data_ptr() + self.g["so"], sp, spl)

    def check(self, pack, note):
        if pack:
            assert np.array_equal(self.d_surface.cpu().numpy(), self.want_surface), note
        else:
            for q, (d, want) in enumerate(zip(self.d_planes, self.want_planes)):
                assert np.array_equal(d.cpu().numpy(), want), (note, "plane %d" % q)


def move(s, frames, pack, stream=None):
    fmt, w, h = frames[0].fmt, frames[0].w, frames[0].h
    if pack:
        s.pack_planes([f.planes_arg() for f in frames], [f.surface_arg() for f in frames], fmt, w, h, stream=stream)
    else:
        s.unpack_planes([f.surface_arg() for f in frames], [f.planes_arg() for f in frames], fmt, w, h, stream=stream)
    torch.cuda.synchronize()


def sizes(fmt):
    return [(w, h) for w in WIDTHS for h in HEIGHTS if P.admits(fmt, w, h)]


@pytest.mark.parametrize("pack", [True, False], ids=["pack", "unpack"])
@pytest.mark.parametrize("fmt", P.FORMATS, ids=[IDS[f] for f in P.FORMATS])
def test_every_width_height_and_layout(ctx, fmt, pack):
    s = ctx[False]
    assert len(sizes(fmt)) == (12 if fmt in F.S420 else 18)  # heights 2 and 26, and 3 where the format has no vertical parity rule
    for i, (w, h) in enumerate(sizes(fmt)):
        for j, layout in enumerate(LAYOUTS):
            f = Frame(100 * i + j + fmt, fmt, w, h, layout, pack)
            if layout == "offset":  # what the issue of this feature asks for, spelled out
                g = f.g
                assert g["so"] == g["yo"] == g["uo"] == F.ES[fmt] and all(g[k] % 16 for k in ("sp", "yp", "cp"))
            move(s, [f], pack)
            f.check(pack, (w, h, layout))


@pytest.mark.parametrize("pack", [True, False], ids=["pack", "unpack"])
@pytest.mark.parametrize("fmt", P.FORMATS, ids=[IDS[f] for f in P.FORMATS])
def test_three_frames_in_one_call_on_a_stream(ctx, fmt, pack):
    s = ctx[False]
    frames = [Frame(7 + k + fmt, fmt, 34, 26, layout, pack) for k, layout in enumerate(("offset", "packed", "coaligned"))]
    assert not np.array_equal(frames[0].planes[0], frames[1].planes[0])
    st = torch.cuda.Stream()
    move(s, frames, pack, stream=st.cuda_stream)
    for k, f in enumerate(frames):
        f.check(pack, k)


def test_ten_bit_words(ctx):
    """What the planar words hold above bit 9 never reaches a P010 / P210 surface; what a surface word holds below bit 6 never reaches
    the planes; YUV444P10 words travel as they are."""
    s = ctx[False]
    for fmt in (F.P010, F.P210):
        f = Frame(1, fmt, 18, 26, "packed", True)
        assert any((p >> 10).any() for p in f.planes)
        move(s, [f], True)
        got = f.d_surface.cpu().numpy()[:f.surface.nbytes].view(np.uint16)
        assert not (got & 63).any() and np.array_equal(got.reshape(f.surface.shape) >> 6, P.pack(fmt, *f.planes) >> 6)
        f = Frame(2, fmt, 18, 26, "packed", False)
        assert (f.surface & 63).any() and max(p.max() for p in f.planes) == 1023
        move(s, [f], False)
        f.check(False, fmt)
    f = Frame(3, F.YUV444P10, 18, 3, "packed", True)
    assert (f.surface >> 10).any()
    move(s, [f], True)
    f.check(True, "444p10")


def bad_calls(f):
    """(name, planes entry, surface entry, fmt, w, h) of calls that must be refused, from the good frame f (NV12 or P010, 36 x 26)."""
    y, u, v, yp, cp = f.planes_arg()
    d, sp, spl = f.surface_arg()
    fmt, w, h, es = f.fmt, f.w, f.h, F.ES[f.fmt]
    out = [("null-y", (0, u, v, yp, cp), (d, sp, spl), fmt, w, h), ("null-u", (y, 0, v, yp, cp), (d, sp, spl), fmt, w, h),
           ("null-v", (y, u, 0, yp, cp), (d, sp, spl), fmt, w, h), ("null-surface", (y, u, v, yp, cp), (0, sp, spl), fmt, w, h),
           ("odd-w", (y, u, v, yp, cp), (d, sp, spl), fmt, w - 1, h), ("odd-h", (y, u, v, yp, cp), (d, sp, spl), fmt, w, h - 1),
           ("odd-w-422", (y, u, v, yp, cp), (d, sp, spl), fmt + 4, w - 1, h),
           ("zero-w", (y, u, v, yp, cp), (d, sp, spl), fmt, 0, h), ("zero-h", (y, u, v, yp, cp), (d, sp, spl), fmt, w, 0),
           ("y-pitch-short", (y, u, v, w * es - es, cp), (d, sp, spl), fmt, w, h),
           ("c-pitch-short", (y, u, v, yp, w // 2 * es - es), (d, sp, spl), fmt, w, h),
           ("c-pitch-short-444", (y, u, v, yp, w // 2 * es), (d, sp, spl), F.YUV444P if es == 1 else F.YUV444P10, w, h),
           ("y-pitch-negative", (y, u, v, -yp, cp), (d, sp, spl), fmt, w, h), ("c-pitch-negative", (y, u, v, yp, -cp), (d, sp, spl), fmt, w, h),
           ("row-pitch-short", (y, u, v, yp, cp), (d, w * es - es, spl), fmt, w, h),
           ("row-pitch-negative", (y, u, v, yp, cp), (d, -sp, spl), fmt, w, h),
           ("plane-pitch-negative", (y, u, v, yp, cp), (d, sp, -spl), fmt, w, h),
           ("row-pitch-2^31", (y, u, v, yp, cp), (d, 1 << 31, spl), fmt, w, h)]
    out += [("fmt-%d" % bad, (y, u, v, yp, cp), (d, sp, spl), bad, w, h) for bad in (F.U8, F.F16, F.F32, 3, 6, 7, 10, 11, 14, -1)]
    if es == 2:
        out += [("odd-y", (y + 1, u, v, yp, cp), (d, sp, spl), fmt, w, h), ("odd-v", (y, u, v + 1, yp, cp), (d, sp, spl), fmt, w, h),
                ("odd-y-pitch", (y, u, v, yp + 1, cp), (d, sp, spl), fmt, w, h), ("odd-c-pitch", (y, u, v, yp, cp + 1), (d, sp, spl), fmt, w, h),
                ("odd-surface", (y, u, v, yp, cp), (d + 1, sp, spl), fmt, w, h), ("odd-row-pitch", (y, u, v, yp, cp), (d, sp + 1, spl), fmt, w, h),
                ("odd-plane-pitch", (y, u, v, yp, cp), (d, sp, spl + 1), fmt, w, h)]
    return out


@pytest.mark.parametrize("pack", [True, False], ids=["pack", "unpack"])
@pytest.mark.parametrize("fmt", [F.NV12, F.P010], ids=["nv12", "p010"])
def test_every_refusal_leaves_the_destination_untouched(ctx, fmt, pack):
    s = ctx[False]
    f = Frame(9, fmt, 36, 26, "offset", pack)
    good = Frame(10, fmt, 36, 26, "offset", pack)
    call = s.pack_planes if pack else s.unpack_planes
    order = (lambda p, im: (p, im)) if pack else (lambda p, im: (im, p))
    cases = bad_calls(f)
    assert len(cases) == (28 if fmt == F.NV12 else 35)
    for name, planes, surf, bfmt, w, h in cases:
        for entries in ([planes], [good.planes_arg(), planes]):  # alone, and behind a good frame: nothing of the call may have run
            surfs = [surf] if len(entries) == 1 else [good.surface_arg(), surf]
            with pytest.raises(R.RealSRError) as e:
                call(*order(entries, surfs), bfmt, w, h)
            assert e.value.code == R.RSR_E_ARG, name
    with pytest.raises(R.RealSRError) as e:
        call([], [], fmt, 36, 26)  # n < 1
    assert e.value.code == R.RSR_E_ARG
    with pytest.raises(R.RealSRError) as e:
        call(*order([f.planes_arg()] * (R.RSR_SEQ_MAX + 1), [f.surface_arg()] * (R.RSR_SEQ_MAX + 1)), fmt, 36, 26)
    assert e.value.code == R.RSR_E_ARG and "n must be" in str(e.value)
    null = R.lib().rsr_pack_planes if pack else R.lib().rsr_unpack_planes
    assert null(s._h, 1, None, None, fmt, 36, 26, None) == R.RSR_E_ARG
    torch.cuda.synchronize()
    dests = [f.d_surface, good.d_surface] if pack else f.d_planes + good.d_planes
    assert all(bool((d == 0xCD).all()) for d in dests)
    move(s, [f, good], pack)  # ... and the same frames, asked for properly, are moved
    f.check(pack, "after the refusals")
    good.check(pack, "after the refusals")


def as_torch(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16 if a.dtype == np.uint16 else a.dtype)).cuda()


@pytest.mark.parametrize("fmt,chroma,w,h", [(F.NV12, 420, 36, 26), (F.P010, 420, 36, 26), (F.P210, 422, 36, 25), (F.YUV444P10, 444, 35, 25)],
                         ids=["nv12", "p010", "p210", "yuv444p10"])
def test_planes_through_upscale_yuv(ctx, fmt, chroma, w, h):
    """unpack(upscale_yuv(pack(planes))) through torch_io is the definition around the plain call, byte for byte."""
    s = ctx[False]
    planes = P.frame(31 + fmt, fmt, w, h)
    ty, tu, tv = (as_torch(p) for p in planes)
    surf = torch_io.pack_planes(s, ty, tu, tv, chroma=chroma)
    assert tuple(surf.shape) == F.shape_of(fmt, w, h)
    assert np.array_equal(surf.cpu().numpy().view(F.NP[fmt]), P.pack(fmt, *planes))
    big = torch_io.upscale_yuv(s, surf, chroma=chroma)
    got = torch_io.unpack_planes(s, big, chroma=chroma)
    want_surface = run(s, P.pack(fmt, *planes), fmt, fmt)
    assert np.array_equal(big.cpu().numpy().view(F.NP[fmt]), want_surface)
    want = P.unpack(fmt, want_surface, 4 * w, 4 * h)
    assert [tuple(t.shape) for t in got] == [p.shape for p in want] and len(np.unique(want[0])) > 16
    assert all(np.array_equal(t.cpu().numpy().view(F.NP[fmt]), p) for t, p in zip(got, want))
    # pitched views in, given planes out: a crop of a padded frame, planes inside a larger canvas
    pad = torch.full((h + 3, w + 7), 0x4D, dtype=ty.dtype, device="cuda")
    pad[1:h + 1, 3:w + 3] = ty
    surf2 = torch_io.pack_planes(s, pad[1:h + 1, 3:w + 3], tu, tv, chroma=chroma, out=torch.empty_like(surf))
    assert torch.equal(surf2, surf)
    oy = torch.full((4 * h + 2, 4 * w + 9), 0x4D, dtype=ty.dtype, device="cuda")
    ou, ov = torch.empty_like(got[1]), torch.empty_like(got[2])
    back = torch_io.unpack_planes(s, big, chroma=chroma, out=(oy[1:4 * h + 1, 5:4 * w + 5], ou, ov))
    assert torch.equal(back[0], got[0]) and torch.equal(ou, got[1]) and torch.equal(ov, got[2])
    oy[1:4 * h + 1, 5:4 * w + 5] = 0x4D
    assert bool((oy == 0x4D).all())
