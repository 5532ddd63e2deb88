"""The definition of rsr_pack_planes / rsr_unpack_planes (include/realsr_hip.h "Three-plane YUV frames"), restated in numpy on the format
table of tests/pixfmt_ref.py: the three planes Y, U, V of a frame as a software decoder holds it (yuv420p / yuv422p / yuv444p and their
10-bit little-endian forms, the code in the LOW bits) against the packed surface of an RSR_FMT_* the engine takes.

  8-bit            bytes move unchanged; UV[r][2X] = U[r][X], UV[r][2X + 1] = V[r][X]; Y row by row
  P010 / P210      pack: every surface word is (plane word & 1023) << 6, Y included; unpack: every plane word is surface word >> 6
  YUV444P10        words are copied verbatim both ways (both layouts hold the code low)
numpy only; nothing here asks the library."""
import numpy as np

import pixfmt_ref as F

FORMATS = F.SEMIS + F.P444  # the six YUV formats


def chroma_dims(fmt, w, h):
    """(cw, ch) of the U and the V plane of a w x h frame."""
    t = F.TABLE[fmt]
    return w >> t.sx, h >> t.sy


def plane_shapes(fmt, w, h):
    cw, ch = chroma_dims(fmt, w, h)
    return (h, w), (ch, cw), (ch, cw)


def admits(fmt, w, h):
    """The parity rule of the format (rsr_image_bytes states it)."""
    t = F.TABLE[fmt]
    return w >= 1 and h >= 1 and not (w & t.sx) and not (h & t.sy)


def frame(seed, fmt, w, h, dirty=False):
    """Seeded random planes (y, u, v) over the whole code range -- dirty: 10-bit words with random bits above bit 9 as well, which are no
    part of the code."""
    rng, dirt = np.random.default_rng(seed), np.random.default_rng(seed + 1000003)  # (the codes of a seed are the same, dirty or not)
    t = F.TABLE[fmt]
    out = []
    for shape in plane_shapes(fmt, w, h):
        p = rng.integers(0, 1 << t.bits, size=shape)
        if dirty and t.bits == 10:
            p = p | (dirt.integers(0, 64, size=shape) << 10)
        out.append(p.astype(t.dtype))
    return tuple(out)


def pack(fmt, y, u, v):
    """The packed surface (pixfmt_ref.shape_of) of the planes."""
    t = F.TABLE[fmt]
    h, w = y.shape
    assert admits(fmt, w, h) and all(p.dtype == t.dtype for p in (y, u, v)) and (u.shape, v.shape) == plane_shapes(fmt, w, h)[1:]
    if t.kind == F.PLANAR:
        return np.stack([y, u, v])  # verbatim, the bits above the code included
    uv = np.stack([u, v], axis=-1).reshape(u.shape[0], w)
    s = np.concatenate([y, uv], axis=0)
    if t.high:
        s = ((s.astype(np.uint32) & 1023) << 6).astype(t.dtype)
    assert s.shape == F.shape_of(fmt, w, h)
    return s


def unpack(fmt, s, w, h):
    """The planes (y, u, v) of the packed surface s."""
    t = F.TABLE[fmt]
    assert s.dtype == t.dtype and s.shape == F.shape_of(fmt, w, h)
    if t.kind == F.PLANAR:
        return s[0].copy(), s[1].copy(), s[2].copy()
    if t.high:
        s = s >> 6
    uv = s[h:].reshape(h >> t.sy, w >> 1, 2)
    return s[:h].copy(), uv[..., 0].copy(), uv[..., 1].copy()
