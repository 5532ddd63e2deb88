"""The chroma sitings of the NV12 / P010 definition (include/realsr_hip.h, "Chroma siting, exact": option "yuv_siting" 1 = left,
2 = top-left) restated in numpy float32 on top of tests/yuv_ref.py.  A helper, not a test.  Written from the header text, not from the
kernels: every numpy operation is one float32 operation rounded by itself, in the order the header writes, so the device results must
equal these bit for bit.  Siting 0 (centre) IS yuv_ref: decode / encode delegate to it.

An axis on which chroma is co-sited with the even luma index is "cos": siting 1 is cos horizontally and centre vertically, siting 2 is cos
on both axes."""
import numpy as np

import yuv_ref

F = np.float32
COS_AXES = {1: (True, False), 2: (True, True)}  # siting -> (horizontal is cos, vertical is cos)


def upsample_axis(p, axis, cos):
    """Chroma samples p (float32) -> one value per luma index along `axis` (twice as many): the centre rule (3 * near + far) * 0.25f, or
    the cos rule c[n] for an even index, (c[n] + c[min(n + 1, N/2 - 1)]) * 0.5f for an odd one."""
    p = np.moveaxis(p, axis, 0)
    half = p.shape[0]
    i = np.arange(2 * half)
    n = i >> 1
    if cos:
        odd = (p[n] + p[np.minimum(n + 1, half - 1)]) * F(0.5)
        out = np.where((i & 1).reshape((-1,) + (1,) * (p.ndim - 1)) == 1, odd, p[n])
    else:
        far = np.clip(n + np.where(i & 1, 1, -1), 0, half - 1)
        out = (F(3) * p[n] + p[far]) * F(0.25)
    assert out.dtype == np.float32
    return np.moveaxis(out, 0, axis)


def decode(y, uv, siting, matrix=709, full=0, bits=8):
    """(y, uv) codes -> float32 (3, h, w): R, G, B clamped to [0, 1] and rounded to fp16 -- the network input -- at chroma siting `siting`."""
    if siting == 0:
        return yuv_ref.decode(y, uv, matrix, full, bits)
    hcos, vcos = COS_AXES[siting]
    c = yuv_ref.constants(matrix, full, bits)
    ch = [upsample_axis(upsample_axis(uv[..., q].astype(F), 1, hcos), 0, vcos) for q in range(2)]  # horizontally first, then vertically
    yn = (y.astype(F) - c["yoff"]) * c["ys"]
    cb, cr = (ch[0] - c["coff"]) * c["cs"], (ch[1] - c["coff"]) * c["cs"]
    r = yn + c["rv"] * cr
    g = (yn - c["gu"] * cb) - c["gv"] * cr
    b = yn + c["bu"] * cb
    rgb = np.clip(np.stack([r, g, b]), F(0), F(1))
    assert rgb.dtype == np.float32
    return rgb.astype(np.float16).astype(np.float32)


def _before(n, tile_out):
    """Per even index 2X of an axis of n output pixels: the index in front of it, 2X - 1 -- or 2X itself where 2X is the first pixel of a
    tile's rectangle (a multiple of tile_out; tile_out = 0: no tile grid, the image's first pixel only)."""
    e = np.arange(0, n, 2)
    first = (e % tile_out == 0) if tile_out else (e == 0)
    return np.where(first, e, e - 1)


def encode(d, siting, tile_out, matrix=709, full=0, bits=8):
    """float32 (3, H, W), H and W even -- what RSR_FMT_F32_CHW holds -- -> (y, uv) codes at chroma siting `siting`.
    tile_out = tilesize * out_scale: a tile's rectangle starts at its multiples; 0 = no tile grid."""
    if siting == 0:
        return yuv_ref.encode(d, matrix, full, bits)
    c = yuv_ref.constants(matrix, full, bits)
    d = np.asarray(d)
    assert d.dtype == np.float32 and d.shape[0] == 3 and d.shape[1] % 2 == 0 and d.shape[2] % 2 == 0
    assert tile_out % 2 == 0
    H, W = d.shape[1:]
    y, _ = yuv_ref.encode(d, matrix, full, bits)  # luma is unchanged
    xl = _before(W, tile_out)
    hs = (d[:, :, xl] + d[:, :, 1::2]) + (d[:, :, 0::2] + d[:, :, 0::2])  # Hs(y) for every row y: (3, H, W / 2)
    if siting == 1:
        m = (hs[:, 0::2] + hs[:, 1::2]) * F(0.125)
    else:
        yu = _before(H, tile_out)
        m = ((hs[:, yu] + hs[:, 1::2]) + (hs[:, 0::2] + hs[:, 0::2])) * F(0.0625)
    assert m.dtype == np.float32

    def code(v):
        return np.clip(np.floor(v * c["cscale"] + c["cadd"]), F(0), c["maxcode"]).astype(np.int64)

    ym = (c["kr"] * m[0] + c["kg"] * m[1]) + c["kb"] * m[2]
    cb, cr = (m[2] - ym) * c["icb"], (m[0] - ym) * c["icr"]
    return y, np.stack([code(cb), code(cr)], axis=-1)
