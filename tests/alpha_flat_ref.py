"""numpy restatement of the rule of option "alpha_adaptive" (include/realsr_hip.h "alpha_adaptive"): a tile is FLAT when all alpha samples
of its source rectangle are equal, compared at the image's own depth.  Plain loops over tiles on top of tests/tile_diff_ref.py; nothing
here shares code with the library."""
import numpy as np

from tile_diff_ref import out_rect, source_rect, tile_count


def varies(img, T, P):
    """flag[t] = 1 where the alpha of tile t's source rectangle holds more than one value, else 0 (uint8, nx * ny, row-major).
    img: (h, w, 4) uint8 or uint16."""
    assert img.ndim == 3 and img.shape[2] == 4 and img.dtype in (np.uint8, np.uint16)
    h, w = img.shape[:2]
    nx, ny = tile_count(w, h, T)
    flags = np.zeros(nx * ny, dtype=np.uint8)
    for t in range(nx * ny):
        x0, y0, x1, y1 = source_rect(w, h, T, P, t)
        a = img[y0:y1, x0:x1, 3]
        flags[t] = int((a != a[0, 0]).any())
    return flags


def select(flags, flat_img, net_img, w, h, T, num=4, den=1, num_y=None, den_y=None):
    """The image the option promises: the output rectangles of flat tiles from flat_img (the "alpha_net" 0 image), all others from net_img
    (the "alpha_net" 1 image)."""
    assert flat_img.shape == net_img.shape
    out = net_img.copy()
    for t in np.flatnonzero(flags == 0):
        x0, y0, x1, y1 = out_rect(w, h, T, int(t), num, den, num_y, den_y)
        out[y0:y1, x0:x1] = flat_img[y0:y1, x0:x1]
    return out
