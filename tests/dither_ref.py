"""Option "dither" of include/realsr_hip.h ("dither": position-keyed ordered dither for integer outputs) restated in numpy float32: the
threshold, the RGB quantiser, and the YUV encodes of tests/yuv_ref.py, yuv_siting_ref.py, yuv422_ref.py and yuv444_ref.py with the
threshold in the place of their 0.5 -- those four have the 0.5 inside their constant yadd / cadd, so the encodes are written out again here
on top of their constants, joins and tile-first index helper.  A helper, not a test.  Written from the header text, not from the kernels:
every numpy operation is one float32 operation rounded by itself, in the order the header writes, so the device results must equal these
bit for bit.

theta(w, h)[y, x] is the threshold of the sample at column x, row y of its own plane of the OUTPUT image; a subsampled plane asks for
theta at its own size."""
import numpy as np

import pixfmt_ref as P
import yuv422_ref
import yuv444_ref
import yuv_ref

F = np.float32
CX, CY = 0xC13FA9A9, 0x91E10DA5


def theta(w, h):
    """float32 (h, w): h = (x * CX + y * CY) mod 2^32, k = h >> 25, theta = (2k + 1) * 2^-8.  uint64 arithmetic masked to 32 bits (x, y
    below 2^20: no product leaves 64 bits)."""
    x = np.arange(w, dtype=np.uint64)[None, :]
    y = np.arange(h, dtype=np.uint64)[:, None]
    hh = (x * np.uint64(CX) + y * np.uint64(CY)) & np.uint64(0xFFFFFFFF)
    k = (hh >> np.uint64(25)).astype(np.int64)
    assert k.min() >= 0 and k.max() <= 127
    return (2 * k + 1).astype(F) * F(2.0 ** -8)


def quantise_rgb(d, M):
    """float32 (3, h, w) in [0, 1] -- what RSR_FMT_F32_CHW holds -- -> the HWC image (h, w, 3), uint8 (M = 255) or uint16 (M = 65535):
    floor(add_rn(mul_rn(d, M), theta)), the three samples of a pixel against the pixel's one threshold.  No clamp: none can act."""
    d = np.asarray(d)
    assert d.dtype == np.float32 and d.ndim == 3 and d.shape[0] == 3 and d.min() >= 0 and d.max() <= 1 and M in (255, 65535)
    q = np.floor(d * F(M) + theta(d.shape[2], d.shape[1])[None])
    assert q.dtype == np.float32 and q.min() >= 0 and q.max() <= M
    return np.ascontiguousarray(q.transpose(1, 2, 0)).astype(np.uint8 if M == 255 else np.uint16)


def _code(v, scale, off, th, maxcode):
    """floor(add_rn(mul_rn(v, scale), add_rn(off, theta))) clamped to [0, maxcode]"""
    q = v * scale + (off + th)
    assert q.dtype == np.float32
    return np.clip(np.floor(q), F(0), maxcode).astype(np.int64)


def _luma(c, v):
    return (c["kr"] * v[0] + c["kg"] * v[1]) + c["kb"] * v[2]


def _chroma_codes(c, m):
    """(U, V) codes (h, w, 2) of the chroma values m (3, h, w): the two of a sample share theta at the sample's own indices."""
    ym = _luma(c, m)
    cb, cr = (m[2] - ym) * c["icb"], (m[0] - ym) * c["icr"]
    th = theta(m.shape[2], m.shape[1])
    return np.stack([_code(cb, c["cscale"], c["coff"], th, c["maxcode"]), _code(cr, c["cscale"], c["coff"], th, c["maxcode"])], axis=-1)


def _luma_codes(c, d):
    return _code(_luma(c, d), c["yscale"], c["yoff"], theta(d.shape[2], d.shape[1]), c["maxcode"])


def encode420(d, siting=0, tile_out=0, matrix=709, full=0, bits=8):
    """float32 (3, H, W), H and W even -> (y, uv) codes of an NV12 / P010 surface, uv (H / 2, W / 2, 2).  The chroma values are those of
    yuv_ref.encode (siting 0) and yuv_siting_ref.encode (1 = left, 2 = top-left; tile_out = the size of a tile's output rectangle, whose
    first column / row clamps the sited filter; 0 = no tile grid)."""
    c = yuv_ref.constants(matrix, full, bits)
    d = np.asarray(d)
    assert d.dtype == np.float32 and d.shape[0] == 3 and d.shape[1] % 2 == 0 and d.shape[2] % 2 == 0 and tile_out % 2 == 0
    H, W = d.shape[1:]
    if siting == 0:
        m = ((d[:, 0::2, 0::2] + d[:, 0::2, 1::2]) + (d[:, 1::2, 0::2] + d[:, 1::2, 1::2])) * F(0.25)
    else:
        xl = yuv422_ref.before(W, tile_out)
        hs = (d[:, :, xl] + d[:, :, 1::2]) + (d[:, :, 0::2] + d[:, :, 0::2])
        if siting == 1:
            m = (hs[:, 0::2] + hs[:, 1::2]) * F(0.125)
        else:
            yu = yuv422_ref.before(H, tile_out)
            m = ((hs[:, yu] + hs[:, 1::2]) + (hs[:, 0::2] + hs[:, 0::2])) * F(0.0625)
    assert m.dtype == np.float32 and m.shape == (3, H // 2, W // 2)
    return _luma_codes(c, d), _chroma_codes(c, m)


def encode422(d, siting=0, tile_w=0, matrix=709, full=0, bits=8):
    """float32 (3, H, W), W even, any H -> (y, uv) codes of an NV16 / P210 surface, uv (H, W / 2, 2): the chroma values of
    yuv422_ref.encode (siting 2 is 1)."""
    c = yuv_ref.constants(matrix, full, bits)
    d = np.asarray(d)
    assert d.dtype == np.float32 and d.shape[0] == 3 and d.shape[2] % 2 == 0 and tile_w % 2 == 0
    if siting == 0:
        m = (d[:, :, 0::2] + d[:, :, 1::2]) * F(0.5)
    else:
        xl = yuv422_ref.before(d.shape[2], tile_w)
        m = ((d[:, :, xl] + d[:, :, 1::2]) + (d[:, :, 0::2] + d[:, :, 0::2])) * F(0.25)
    assert m.dtype == np.float32
    return _luma_codes(c, d), _chroma_codes(c, m)


def encode444(d, matrix=709, full=0, bits=8):
    """float32 (3, H, W), any H and W -> (y, u, v) codes of a YUV444P / YUV444P10 image: m = d, the three codes of a pixel share theta."""
    c = yuv_ref.constants(matrix, full, bits)
    d = np.asarray(d)
    assert d.dtype == np.float32 and d.ndim == 3 and d.shape[0] == 3
    uv = _chroma_codes(c, d)
    return _luma_codes(c, d), uv[..., 0], uv[..., 1]


def encode(fmt, d, cfg=(709, 0), siting=0, tile_out=0):
    """The packed image of format fmt (every integer format of tests/pixfmt_ref.py; 16 = RSR_FMT_U16_HWC) the dithered call writes for d."""
    if fmt == P.U8:
        return quantise_rgb(d, 255)
    if fmt == 16:
        return quantise_rgb(d, 65535)
    bits = P.BITS[fmt]
    if fmt in P.S420:
        return yuv_ref.join(*encode420(d, siting, tile_out, cfg[0], cfg[1], bits), bits)
    if fmt in P.S422:
        return yuv422_ref.join(*encode422(d, siting, tile_out, cfg[0], cfg[1], bits), bits)
    return yuv444_ref.join(*encode444(d, cfg[0], cfg[1], bits), bits)
