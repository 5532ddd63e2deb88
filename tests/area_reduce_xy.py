"""The numpy reference of rsr_set_out_ratio_xy (include/realsr_hip.h, "a ratio per axis"): the definition of tests/area_reduce.py with the
horizontal taps and weights from (nx, dx) and the vertical ones from (ny, dy), and the sited NV12 / P010 encode of tests/yuv_siting_ref.py
with a tile rectangle per axis.  Shared by tests/test_out_ratio_xy.py and tests/test_gpu_out_ratio_xy.py.  A helper, not a test: float32,
every operation rounded by itself, in the stated order."""
import math

import numpy as np

import yuv_ref
import yuv_siting_ref
from area_reduce import RATIOS, _along_x, taps  # noqa: F401  (taps: one axis is one axis, whatever the other does)
from tile_diff_ref import out_rect

F32 = np.float32

# every ratio rsr_set_out_ratio_xy takes on an axis, in lowest terms: d in 1..8, 1 <= n / d <= 4
AXIS_RATIOS = [(n, d) for d in range(1, 9) for n in range(d, 4 * d + 1) if math.gcd(n, d) == 1]


def admitted(n, d):
    """(n, d) reduced where rsr_set_out_ratio_xy takes n / d on an axis, else None."""
    if n < 1 or d < 1:
        return None
    g = math.gcd(n, d)
    n, d = n // g, d // g
    return (n, d) if d <= 8 and d <= n <= 4 * d else None


def out_size_xy(rx, ry, T, w, h, yuv=False):
    """(ow, oh), or None where the call-time rule refuses w, h or the tile size T (rx, ry reduced)."""
    (nx, dx), (ny, dy) = rx, ry
    if w * nx % dx or T * nx % dx or h * ny % dy or T * ny % dy:
        return None
    if yuv and ((w | h) & 1 or (w * nx // dx | T * nx // dx | h * ny // dy | T * ny // dy) & 1):
        return None
    return w * nx // dx, h * ny // dy


def area_reduce_xy(v, rx, ry, top=1.0):
    """v: float32 (..., 4h, 4w), the x4 image; rx = (nx, dx) along the last axis, ry = (ny, dy) along the one before, each in lowest terms.
    Returns the float32 (..., h ny / dy, w nx / dx) array of min(V * fp32(1 / (16 dx dy)), top): c = min(max(v, 0), top), horizontally
    first with the taps of (nx, dx), then vertically with those of (ny, dy)."""
    (nx, dx), (ny, dy) = rx, ry
    v = np.asarray(v)
    assert v.dtype == np.float32 and math.gcd(nx, dx) == 1 and math.gcd(ny, dy) == 1
    c = np.minimum(np.maximum(v, F32(0)), F32(top))
    H = _along_x(c, nx, dx)
    V = np.swapaxes(_along_x(np.ascontiguousarray(np.swapaxes(H, -1, -2)), ny, dy), -1, -2)
    m = np.minimum(V * F32(1.0 / (16.0 * dx * dy)), F32(top))
    assert m.dtype == np.float32
    return np.ascontiguousarray(m)


def exact_area_mean_xy(v, rx, ry, top=1.0):
    """The same average in float64 with exact rational weights."""
    c = np.clip(np.asarray(v, dtype=np.float64), 0.0, top)

    def along(a, n, d):
        out = np.zeros(a.shape[:-1] + (a.shape[-1] * n // (4 * d),))
        for X in range(out.shape[-1]):
            for i, g in taps(X, n, d):
                out[..., X] += g * a[..., i]
        return out
    (nx, dx), (ny, dy) = rx, ry
    return np.swapaxes(along(np.swapaxes(along(c, nx, dx), -1, -2), ny, dy), -1, -2) / (16.0 * dx * dy)


def encode_xy(d, siting, tile_out_x, tile_out_y, matrix=709, full=0, bits=8):
    """yuv_siting_ref.encode with a tile rectangle of tile_out_x columns and tile_out_y rows: float32 (3, H, W) -> (y, uv) codes.  The
    left / top-left filters clamp at the first column of every tile rectangle (multiples of tile_out_x) and, top-left, at its first row
    (multiples of tile_out_y); 0 = no tile grid on that axis."""
    if siting == 0:
        return yuv_ref.encode(d, matrix, full, bits)
    c = yuv_ref.constants(matrix, full, bits)
    d = np.asarray(d)
    assert d.dtype == np.float32 and d.shape[0] == 3 and d.shape[1] % 2 == 0 and d.shape[2] % 2 == 0
    assert tile_out_x % 2 == 0 and tile_out_y % 2 == 0
    H, W = d.shape[1:]
    y, _ = yuv_ref.encode(d, matrix, full, bits)  # luma is unchanged
    xl = yuv_siting_ref._before(W, tile_out_x)
    hs = (d[:, :, xl] + d[:, :, 1::2]) + (d[:, :, 0::2] + d[:, :, 0::2])
    if siting == 1:
        m = (hs[:, 0::2] + hs[:, 1::2]) * F32(0.125)
    else:
        yu = yuv_siting_ref._before(H, tile_out_y)
        m = ((hs[:, yu] + hs[:, 1::2]) + (hs[:, 0::2] + hs[:, 0::2])) * F32(0.0625)
    assert m.dtype == np.float32

    def code(v):
        return np.clip(np.floor(v * c["cscale"] + c["cadd"]), F32(0), c["maxcode"]).astype(np.int64)

    ym = (c["kr"] * m[0] + c["kg"] * m[1]) + c["kb"] * m[2]
    cb, cr = (m[2] - ym) * c["icb"], (m[0] - ym) * c["icr"]
    return y, np.stack([code(cb), code(cr)], axis=-1)


def out_rect_xy(w, h, T, tile, rx, ry):
    """(x0, y0, x1, y1) of the tile's output rectangle at the pair (rx, ry)."""
    return out_rect(w, h, T, tile, *rx, *ry)
