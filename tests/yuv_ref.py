"""The NV12 / P010 definition of include/realsr_hip.h ("The definition, exact") restated in numpy float32: constants, decode, encode.
A helper, not a test.  Written from the definition, not from the kernels: every numpy operation below is one float32 operation rounded
by itself, in the order the header writes them, so the device results must equal these bit for bit.

A surface travels here as (y, uv): y an integer array (h, w) of CODES, uv (h / 2, w / 2, 2) of (U, V) codes; split() / join() convert
from and to the (3h / 2, w) array a decoder yields (uint8, or uint16 words with the 10-bit code in their high bits)."""
import numpy as np

F = np.float32
KR_KB = {709: (0.2126, 0.0722), 601: (0.299, 0.114), 2020: (0.2627, 0.0593)}
# the order of rsr_yuv_constants
NAMES = ("yoff", "ys", "coff", "cs", "rv", "gu", "gv", "bu", "kr", "kg", "kb", "yscale", "yadd", "cscale", "cadd", "icb", "icr", "maxcode")


def constants(matrix=709, full=0, bits=8):
    """Every constant computed in double from Kr and Kb and rounded once to float32."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    k, top = float(1 << (bits - 8)), float((1 << bits) - 1)
    yoff, coff = (0.0 if full else 16.0 * k), float(1 << (bits - 1))
    yscale, cscale = (top, top) if full else (219.0 * k, 224.0 * k)
    c = dict(yoff=F(yoff), ys=F(1.0 / yscale), coff=F(coff), cs=F(1.0 / cscale),
             rv=F(2.0 * (1.0 - kr)), gu=F(2.0 * kb * (1.0 - kb) / kg), gv=F(2.0 * kr * (1.0 - kr) / kg), bu=F(2.0 * (1.0 - kb)),
             kr=F(kr), kg=F(kg), kb=F(kb), yscale=F(yscale), yadd=F(yoff) + F(0.5), cscale=F(cscale), cadd=F(coff) + F(0.5),
             icb=F(1.0 / (2.0 * (1.0 - kb))), icr=F(1.0 / (2.0 * (1.0 - kr))), maxcode=F(top))
    assert all(v.dtype == np.float32 for v in c.values())
    return c


def split(surface, bits):
    """(3h / 2, w) surface -> (y, uv) codes."""
    s = np.asarray(surface)
    s = s.view(np.uint16) if s.dtype == np.int16 else s
    assert s.dtype == (np.uint8 if bits == 8 else np.uint16) and s.ndim == 2 and s.shape[0] % 3 == 0 and s.shape[1] % 2 == 0
    h, w = s.shape[0] * 2 // 3, s.shape[1]
    codes = s.astype(np.int64) >> (0 if bits == 8 else 6)
    return codes[:h], codes[h:].reshape(h // 2, w // 2, 2)


def join(y, uv, bits):
    """(y, uv) codes -> the (3h / 2, w) surface: uint8, or uint16 holding code << 6."""
    h, w = y.shape
    s = np.concatenate([y, uv.reshape(h // 2, w)], axis=0)
    return s.astype(np.uint8) if bits == 8 else (s << 6).astype(np.uint16)


def _near_far(n):
    """Per luma index: its own chroma sample and the next one on its side, clamped at the edge (centre siting)."""
    i = np.arange(n)
    near = i >> 1
    return near, np.clip(near + np.where(i & 1, 1, -1), 0, n // 2 - 1)


def decode(y, uv, matrix=709, full=0, bits=8):
    """(y, uv) codes -> float32 (3, h, w): R, G, B clamped to [0, 1] and rounded to fp16 (nearest even) -- the network input."""
    c = constants(matrix, full, bits)
    h, w = y.shape
    xn, xf = _near_far(w)
    yn_, yf = _near_far(h)
    ch = []
    for q in range(2):
        p = uv[..., q].astype(F)
        hz = (F(3) * p[:, xn] + p[:, xf]) * F(0.25)     # horizontally first
        ch.append((F(3) * hz[yn_] + hz[yf]) * F(0.25))  # then vertically
    yn = (y.astype(F) - c["yoff"]) * c["ys"]
    cb, cr = (ch[0] - c["coff"]) * c["cs"], (ch[1] - c["coff"]) * c["cs"]
    r = yn + c["rv"] * cr
    g = (yn - c["gu"] * cb) - c["gv"] * cr
    b = yn + c["bu"] * cb
    rgb = np.clip(np.stack([r, g, b]), F(0), F(1))
    assert rgb.dtype == np.float32
    return rgb.astype(np.float16).astype(np.float32)


def encode(d, matrix=709, full=0, bits=8):
    """float32 (3, H, W), H and W even -- what RSR_FMT_F32_CHW holds -- -> (y, uv) codes."""
    c = constants(matrix, full, bits)
    d = np.asarray(d)
    assert d.dtype == np.float32 and d.shape[0] == 3 and d.shape[1] % 2 == 0 and d.shape[2] % 2 == 0

    def luma(v):
        return (c["kr"] * v[0] + c["kg"] * v[1]) + c["kb"] * v[2]

    def code(v, scale, add):
        return np.clip(np.floor(v * scale + add), F(0), c["maxcode"]).astype(np.int64)

    y = code(luma(d), c["yscale"], c["yadd"])
    m = ((d[:, 0::2, 0::2] + d[:, 0::2, 1::2]) + (d[:, 1::2, 0::2] + d[:, 1::2, 1::2])) * F(0.25)
    ym = luma(m)
    cb, cr = (m[2] - ym) * c["icb"], (m[0] - ym) * c["icr"]
    uv = np.stack([code(cb, c["cscale"], c["cadd"]), code(cr, c["cscale"], c["cadd"])], axis=-1)
    return y, uv
