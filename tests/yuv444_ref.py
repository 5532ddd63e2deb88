"""The YUV444P / YUV444P10 definition of include/realsr_hip.h ("YUV 4:4:4", "The definition, exact") restated in numpy float32 on top of
tests/yuv_ref.py, whose constants it shares.  A helper, not a test.  Written from the header text, not from the kernels: every numpy
operation is one float32 operation rounded by itself, in the order the header writes, so the device results must equal these bit for bit.

An image travels here as (y, u, v): three integer arrays (h, w) of CODES; split() / join() convert from and to the (3, h, w) array
(uint8, or uint16 words with the 10-bit code in their LOW bits -- yuv444p10le; what a producer left above bit 9 is not part of the code).
Nothing is subsampled: there is no chroma filter, no siting, no parity rule and no tile grid in any of this."""
import numpy as np

import yuv_ref

F = np.float32


def split(image, bits):
    """(3, h, w) image -> (y, u, v) codes (10 bits: word & 1023)."""
    s = np.asarray(image)
    s = s.view(np.uint16) if s.dtype == np.int16 else s
    assert s.dtype == (np.uint8 if bits == 8 else np.uint16) and s.ndim == 3 and s.shape[0] == 3
    codes = s.astype(np.int64) & ((1 << bits) - 1)
    return codes[0], codes[1], codes[2]


def join(y, u, v, bits):
    """(y, u, v) codes -> the (3, h, w) image: uint8, or uint16 holding the code itself (the high six bits 0)."""
    s = np.stack([y, u, v])
    assert s.min() >= 0 and s.max() < (1 << bits)
    return s.astype(np.uint8 if bits == 8 else np.uint16)


def decode(y, u, v, matrix=709, full=0, bits=8):
    """(y, u, v) codes -> float32 (3, h, w): R, G, B clamped to [0, 1] and rounded to fp16 (nearest even) -- the network input."""
    c = yuv_ref.constants(matrix, full, bits)
    assert y.shape == u.shape == v.shape
    yn = (y.astype(F) - c["yoff"]) * c["ys"]
    cb, cr = (u.astype(F) - c["coff"]) * c["cs"], (v.astype(F) - c["coff"]) * c["cs"]
    r = yn + c["rv"] * cr
    g = (yn - c["gu"] * cb) - c["gv"] * cr
    b = yn + c["bu"] * cb
    rgb = np.clip(np.stack([r, g, b]), F(0), F(1))
    assert rgb.dtype == np.float32
    return rgb.astype(np.float16).astype(np.float32)


def encode(d, matrix=709, full=0, bits=8):
    """float32 (3, H, W), any H and W -- what RSR_FMT_F32_CHW holds -- -> (y, u, v) codes: the 4:2:0 rule with m = d."""
    c = yuv_ref.constants(matrix, full, bits)
    d = np.asarray(d)
    assert d.dtype == np.float32 and d.ndim == 3 and d.shape[0] == 3

    def code(val, scale, add):
        return np.clip(np.floor(val * scale + add), F(0), c["maxcode"]).astype(np.int64)

    yl = (c["kr"] * d[0] + c["kg"] * d[1]) + c["kb"] * d[2]
    cb, cr = (d[2] - yl) * c["icb"], (d[0] - yl) * c["icr"]
    assert yl.dtype == cb.dtype == cr.dtype == np.float32
    return code(yl, c["yscale"], c["yadd"]), code(cb, c["cscale"], c["cadd"]), code(cr, c["cscale"], c["cadd"])
