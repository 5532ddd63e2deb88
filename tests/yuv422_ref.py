"""The NV16 / P210 definition of include/realsr_hip.h ("YUV 4:2:2", "The definition, exact") restated in numpy float32 on top of
tests/yuv_ref.py, whose constants it shares.  A helper, not a test.  Written from the header text, not from the kernels: every numpy
operation is one float32 operation rounded by itself, in the order the header writes, so the device results must equal these bit for bit.

A surface travels here as (y, uv): y an integer array (h, w) of CODES, uv (h, w / 2, 2) of (U, V) codes -- one chroma row per luma row;
split() / join() convert from and to the (2h, w) array (uint8, or uint16 words with the 10-bit code in their high bits).  Chroma is
halved horizontally only, so a siting has a horizontal meaning alone: 0 = centre, 1 = left (co-sited with the even luma column), and 2
(top-left) IS 1."""
import numpy as np

import yuv_ref

F = np.float32


def split(surface, bits):
    """(2h, w) surface -> (y, uv) codes."""
    s = np.asarray(surface)
    s = s.view(np.uint16) if s.dtype == np.int16 else s
    assert s.dtype == (np.uint8 if bits == 8 else np.uint16) and s.ndim == 2 and s.shape[0] % 2 == 0 and s.shape[1] % 2 == 0
    h, w = s.shape[0] // 2, s.shape[1]
    codes = s.astype(np.int64) >> (0 if bits == 8 else 6)
    return codes[:h], codes[h:].reshape(h, w // 2, 2)


def join(y, uv, bits):
    """(y, uv) codes -> the (2h, w) surface: uint8, or uint16 holding code << 6."""
    h, w = y.shape
    s = np.concatenate([y, uv.reshape(h, w)], axis=0)
    return s.astype(np.uint8) if bits == 8 else (s << 6).astype(np.uint16)


def upsample_x(p, siting):
    """Chroma samples p (float32, (h, w / 2)) -> one value per luma column: the centre rule (3 * c_near + c_far) * 0.25f, or the co-sited
    rule c[n] for x = 2n, (c[n] + c[min(n + 1, w/2 - 1)]) * 0.5f for x = 2n + 1.  No vertical filter: the chroma row is the pixel's own."""
    half = p.shape[1]
    x = np.arange(2 * half)
    n = x >> 1
    if siting == 0:
        far = np.clip(n + np.where(x & 1, 1, -1), 0, half - 1)
        out = (F(3) * p[:, n] + p[:, far]) * F(0.25)
    else:
        odd = (p[:, n] + p[:, np.minimum(n + 1, half - 1)]) * F(0.5)
        out = np.where((x & 1)[None, :] == 1, odd, p[:, n])
    assert out.dtype == np.float32
    return out


def decode(y, uv, matrix=709, full=0, bits=8, siting=0):
    """(y, uv) codes -> float32 (3, h, w): R, G, B clamped to [0, 1] and rounded to fp16 (nearest even) -- the network input."""
    c = yuv_ref.constants(matrix, full, bits)
    assert siting in (0, 1, 2) and uv.shape == (y.shape[0], y.shape[1] // 2, 2)
    ch = [upsample_x(uv[..., q].astype(F), siting) for q in range(2)]
    yn = (y.astype(F) - c["yoff"]) * c["ys"]
    cb, cr = (ch[0] - c["coff"]) * c["cs"], (ch[1] - c["coff"]) * c["cs"]
    r = yn + c["rv"] * cr
    g = (yn - c["gu"] * cb) - c["gv"] * cr
    b = yn + c["bu"] * cb
    rgb = np.clip(np.stack([r, g, b]), F(0), F(1))
    assert rgb.dtype == np.float32
    return rgb.astype(np.float16).astype(np.float32)


def before(n, tile_w):
    """Per even column 2X of n output columns: xl = 2X - 1, or 2X itself where 2X is the first column of a tile's output rectangle (a
    multiple of tile_w; tile_w = 0: no tile grid, the image's first column only -- the unclamped filter a test compares against)."""
    e = np.arange(0, n, 2)
    first = (e % tile_w == 0) if tile_w else (e == 0)
    return np.where(first, e, e - 1)


def encode(d, matrix=709, full=0, bits=8, siting=0, tile_w=0):
    """float32 (3, H, W), W even, any H -- what RSR_FMT_F32_CHW holds -- -> (y, uv) codes, uv (H, W / 2, 2).
    tile_w = the width of a tile's output rectangle (tilesize * nx / dx: rectangles start at its multiples); 0 = no tile grid."""
    c = yuv_ref.constants(matrix, full, bits)
    d = np.asarray(d)
    assert d.dtype == np.float32 and d.shape[0] == 3 and d.shape[2] % 2 == 0 and siting in (0, 1, 2) and tile_w % 2 == 0

    def luma(v):
        return (c["kr"] * v[0] + c["kg"] * v[1]) + c["kb"] * v[2]

    def code(v, scale, add):
        return np.clip(np.floor(v * scale + add), F(0), c["maxcode"]).astype(np.int64)

    y = code(luma(d), c["yscale"], c["yadd"])  # per pixel, independent of the siting
    if siting == 0:
        m = (d[:, :, 0::2] + d[:, :, 1::2]) * F(0.5)
    else:
        xl = before(d.shape[2], tile_w)
        hs = (d[:, :, xl] + d[:, :, 1::2]) + (d[:, :, 0::2] + d[:, :, 0::2])
        m = hs * F(0.25)
    assert m.dtype == np.float32
    ym = luma(m)
    cb, cr = (m[2] - ym) * c["icb"], (m[0] - ym) * c["icr"]
    return y, np.stack([code(cb, c["cscale"], c["cadd"]), code(cr, c["cscale"], c["cadd"])], axis=-1)
