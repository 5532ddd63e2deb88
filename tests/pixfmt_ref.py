"""What a pixel format is, restated once for the tests from include/realsr_hip.h ("pixel formats"): the numpy layout of a packed image of
every RSR_FMT_*, and the helpers that need nothing but that layout -- shapes, seeded random images, sentinels, tile rectangles pasted from
one image into another, images placed into and lifted out of pitched byte canvases.  numpy only; nothing here asks the library (the tie
between the two is tests/test_pixfmt_ref.py).

A packed image is
  HWC      uint8 (h, w, c), c in {3, 4}
  PLANAR   (3, h, w): the float formats and YUV 4:4:4
  SEMI     a surface (h + (h >> sy), w): h rows of Y, then the rows of interleaved (U, V) pairs, one pair per 2 luma columns (sx is 1) and
           one row per 1 << sy luma rows -- 4:2:0 (3h / 2, w), 4:2:2 (2h, w)."""
from collections import namedtuple

import numpy as np

U8, F16, F32, NV12, P010, NV16, P210, YUV444P, YUV444P10 = 0, 1, 2, 4, 5, 8, 9, 12, 13
HWC, PLANAR, SEMI = "hwc", "planar", "semi"
# dtype; bits of a YUV code (0: RGB); layout; log2 of the luma samples per chroma sample along x and y; the 10-bit code sits in the HIGH bits
Fmt = namedtuple("Fmt", "dtype bits kind sx sy high")
TABLE = {
    U8: Fmt(np.uint8, 0, HWC, 0, 0, False),
    F16: Fmt(np.float16, 0, PLANAR, 0, 0, False),
    F32: Fmt(np.float32, 0, PLANAR, 0, 0, False),
    NV12: Fmt(np.uint8, 8, SEMI, 1, 1, False),
    P010: Fmt(np.uint16, 10, SEMI, 1, 1, True),
    NV16: Fmt(np.uint8, 8, SEMI, 1, 0, False),
    P210: Fmt(np.uint16, 10, SEMI, 1, 0, True),
    YUV444P: Fmt(np.uint8, 8, PLANAR, 0, 0, False),
    YUV444P10: Fmt(np.uint16, 10, PLANAR, 0, 0, False),
}
FORMATS = tuple(TABLE)
NP = {f: t.dtype for f, t in TABLE.items()}
ES = {f: np.dtype(t.dtype).itemsize for f, t in TABLE.items()}  # bytes of one element
BITS = {f: t.bits for f, t in TABLE.items() if t.bits}
S420, S422 = tuple(f for f in FORMATS if TABLE[f].kind == SEMI and TABLE[f].sy), tuple(f for f in FORMATS if TABLE[f].kind == SEMI and not TABLE[f].sy)
P444 = tuple(f for f in FORMATS if TABLE[f].kind == PLANAR and TABLE[f].bits)
SEMIS = S420 + S422


def is_yuv(fmt):
    return TABLE[fmt].bits > 0


def plane_rows(fmt, h):
    """Rows of every plane of an h-row image: one (uint8 HWC), three (planar), Y and UV (a surface)."""
    t = TABLE[fmt]
    return [h] if t.kind == HWC else ([h, h, h] if t.kind == PLANAR else [h, h >> t.sy])


def shape_of(fmt, w, h, c=3):
    t = TABLE[fmt]
    return (h, w, c) if t.kind == HWC else ((3, h, w) if t.kind == PLANAR else (h + (h >> t.sy), w))


def dims_of(fmt, x):
    """(w, h) of the packed numpy image x."""
    t = TABLE[fmt]
    if t.kind == HWC:
        return x.shape[1], x.shape[0]
    if t.kind == PLANAR:
        return x.shape[2], x.shape[1]
    return x.shape[1], (x.shape[0] * 2 // 3 if t.sy else x.shape[0] // 2)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def image(seed, fmt, w, h, c=3):
    """A seeded random packed image: uint8 bytes; floats in [0, 1); YUV codes over the whole code range -- most of them outside the RGB
    gamut, so the decoder's clamp acts."""
    rng = np.random.default_rng(seed)
    t = TABLE[fmt]
    if t.kind == HWC:
        return rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)
    if not t.bits:
        return rng.uniform(0, 1, size=(3, h, w)).astype(t.dtype)
    return (rng.integers(0, 1 << t.bits, size=shape_of(fmt, w, h)) << (6 if t.high else 0)).astype(t.dtype)


def u8_image(seed, w, h, c=3):
    return image(seed, U8, w, h, c)


def halfs(seed, w, h):
    """A planar fp16 image with values the uint8 path cannot make."""
    return np.random.default_rng(seed).random((3, h, w), dtype=np.float32).astype(np.float16)


def bits(a):
    """A float array as the unsigned integers of its elements."""
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def image_at(w0, h0):
    """image() with a module's base size as the default w and h."""
    def image_(seed, fmt, w=w0, h=h0, c=3):
        return image(seed, fmt, w, h, c)
    return image_


def sentinel_bytes(fmt, shape):
    """A numpy image of the format, every byte 0xCD."""
    return np.full(int(np.prod(shape)) * ES[fmt], 0xCD, dtype=np.uint8).view(NP[fmt]).reshape(shape)


def sentinel(fmt, shape):
    """A numpy image of the format, filled with 0xCD bytes -- the float formats with NaN."""
    return np.full(shape, np.nan, dtype=NP[fmt]) if fmt in (F16, F32) else sentinel_bytes(fmt, shape)


def pattern(fmt, shape):
    """An image that is recognisably NOT a network output: negative floats, 16-bit words with the low six bits set, a byte ramp of period
    251."""
    i = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    if fmt in (F16, F32):
        return (-2.0 - (i % 977)).astype(NP[fmt])
    if ES[fmt] == 2:
        return (((i % 1021) << 6) | 0x2B).astype(np.uint16)
    return (i % 251).astype(np.uint8)


def paste(fmt, dst, src, rect):
    """The output rectangle `rect` = (x0, y0, x1, y1) of src into dst (packed numpy images of format fmt): of a surface, the Y rectangle and
    the rows of UV pairs that belong to it."""
    x0, y0, x1, y1 = rect
    t = TABLE[fmt]
    if t.kind == HWC:
        dst[y0:y1, x0:x1] = src[y0:y1, x0:x1]
    elif t.kind == PLANAR:
        dst[:, y0:y1, x0:x1] = src[:, y0:y1, x0:x1]
    else:
        oh = dims_of(fmt, dst)[1]
        dst[y0:y1, x0:x1] = src[y0:y1, x0:x1]
        dst[oh + (y0 >> t.sy):oh + (y1 >> t.sy), x0:x1] = src[oh + (y0 >> t.sy):oh + (y1 >> t.sy), x0:x1]


def row_starts(fmt, h, off, pitch, plane):
    """Byte offsets of the rows of a pitched image, in the order of the packed image: rows `pitch` bytes apart from `off`, plane q (a
    surface: the UV rows) q * `plane` bytes behind the first."""
    return [off + q * plane + r * pitch for q, n in enumerate(plane_rows(fmt, h)) for r in range(n)]


def place(canvas, off, pitch, plane, img, fmt):
    """Write the packed image `img` into the byte canvas as a pitched image.  Returns the mask of the bytes that belong to it."""
    starts = row_starts(fmt, dims_of(fmt, img)[1], off, pitch, plane)
    rows = np.ascontiguousarray(img).view(np.uint8).reshape(len(starts), -1)
    mask = np.zeros(canvas.shape, dtype=bool)
    for o, row in zip(starts, rows):
        canvas[o:o + row.size] = row
        mask[o:o + row.size] = True
    return mask


def lift(canvas, off, pitch, plane, fmt, w, h, c=3):
    """The packed image of the pitched image inside the byte canvas."""
    nb = w * ES[fmt] * (c if fmt == U8 else 1)
    return np.stack([canvas[o:o + nb] for o in row_starts(fmt, h, off, pitch, plane)]).view(NP[fmt]).reshape(shape_of(fmt, w, h, c))
