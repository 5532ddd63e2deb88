"""numpy restatement of the tile geometry and of rsr_diff_tiles (include/realsr_hip.h "masked tiles and a device frame diff"): the tile
grid, a tile's source rectangle, and, for every pixel format, the mask of tiles whose compared bytes differ between two frames.  Plain
loops over tiles; nothing here shares code with the library."""
import numpy as np

from pixfmt_ref import F16, F32, NP, NV12, NV16, P010, P210, U8, YUV444P, YUV444P10, dims_of  # noqa: F401  (the formats: tests/pixfmt_ref.py)


def tile_count(w, h, T):
    return -(-w // T), -(-h // T)


def source_rect(w, h, T, P, tile):
    """(x0, y0, x1, y1), half-open: the padded rectangle of tile `tile` (row-major) clipped to the image."""
    nx, ny = tile_count(w, h, T)
    assert 0 <= tile < nx * ny
    yi, xi = divmod(tile, nx)
    return (max(xi * T - P, 0), max(yi * T - P, 0), min(min((xi + 1) * T, w) + P, w), min(min((yi + 1) * T, h) + P, h))


def reflect101(v, n):
    """The index the preprocessing reads for position v of an axis of n pixels: one reflection about either edge, then the clamp for
    images narrower than the halo (oracle/realsr_oracle.c reflect_pad, kernels.hip reflect101)."""
    v = np.abs(np.asarray(v))
    v = np.where(v > n - 1, (n - 1) - (v - (n - 1)), v)
    return np.clip(v, 0, n - 1)


def sampled(w, h, T, P, tile):
    """The sets of image columns and rows the padded tile samples."""
    nx, _ = tile_count(w, h, T)
    yi, xi = divmod(tile, nx)
    tw, th = min((xi + 1) * T, w) - xi * T + 2 * P, min((yi + 1) * T, h) - yi * T + 2 * P
    return set(reflect101(xi * T - P + np.arange(tw), w).tolist()), set(reflect101(yi * T - P + np.arange(th), h).tolist())


def chroma_span(s0, s1, n):
    """Chroma indices [c0, c1] inclusive a luma span [s0, s1) of an axis of n luma samples compares: its own and one beyond."""
    return max((s0 >> 1) - 1, 0), min(((s1 - 1) >> 1) + 1, n // 2 - 1)


def compared(fmt, w, h, T, P, tile, a, b):
    """The pairs of arrays rsr_diff_tiles compares for one tile of the frames a and b (numpy images in the library's layouts: uint8
    (h, w, c); float and planar 4:4:4 (3, h, w); 4:2:0 surfaces (3h / 2, w); 4:2:2 surfaces (2h, w))."""
    x0, y0, x1, y1 = source_rect(w, h, T, P, tile)
    if fmt == U8:
        return [(a[y0:y1, x0:x1, :], b[y0:y1, x0:x1, :])]
    if fmt in (F16, F32, YUV444P, YUV444P10):
        return [(a[:, y0:y1, x0:x1], b[:, y0:y1, x0:x1])]
    cx0, cx1 = chroma_span(x0, x1, w)
    if fmt in (NV16, P210):  # a UV row per Y row: the rectangle's own rows
        return [(a[y0:y1, x0:x1], b[y0:y1, x0:x1]), (a[h + y0:h + y1, 2 * cx0:2 * cx1 + 2], b[h + y0:h + y1, 2 * cx0:2 * cx1 + 2])]
    cy0, cy1 = chroma_span(y0, y1, h)
    return [(a[y0:y1, x0:x1], b[y0:y1, x0:x1]), (a[h + cy0:h + cy1 + 1, 2 * cx0:2 * cx1 + 2], b[h + cy0:h + cy1 + 1, 2 * cx0:2 * cx1 + 2])]


def diff_mask(fmt, a, b, T, P):
    """mask[t] = 1 where any compared BYTE of tile t differs between a and b, else 0 (uint8, nx * ny)."""
    assert a.shape == b.shape and a.dtype == b.dtype == NP[fmt]
    w, h = dims_of(fmt, a)
    nx, ny = tile_count(w, h, T)
    mask = np.zeros(nx * ny, dtype=np.uint8)
    for t in range(nx * ny):
        for pa, pb in compared(fmt, w, h, T, P, t, a, b):
            if not np.array_equal(np.ascontiguousarray(pa).view(np.uint8), np.ascontiguousarray(pb).view(np.uint8)):
                mask[t] = 1
    return mask


def out_rect(w, h, T, tile, num=4, den=1, num_y=None, den_y=None):
    """(x0, y0, x1, y1) of the tile's output rectangle at output ratio num / den -- along y at num_y / den_y where given."""
    if num_y is None:
        num_y, den_y = num, den
    nx, _ = tile_count(w, h, T)
    yi, xi = divmod(tile, nx)
    return (xi * T * num // den, yi * T * num_y // den_y, min((xi + 1) * T, w) * num // den, min((yi + 1) * T, h) * num_y // den_y)
