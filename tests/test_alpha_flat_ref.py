"""tests/alpha_flat_ref.py against the brute-force form of its rule (no GPU): a tile varies when the alpha samples its padded tile actually
READS -- tile_diff_ref.sampled, the reflect-101 halo resolved pixel by pixel -- are not all equal.  The source rectangle is exactly that set
of pixels, so both must agree on every image; and the literal counts tests/test_gpu_alpha_adaptive.py asks of the library."""
import numpy as np
import pytest

import alpha_flat_ref as AF
import tile_diff_ref as ref

T, P, W, H = 16, 10, 83, 44


def brute(img, T, P):
    h, w = img.shape[:2]
    nx, ny = ref.tile_count(w, h, T)
    flags = np.zeros(nx * ny, dtype=np.uint8)
    for t in range(nx * ny):
        xs, ys = ref.sampled(w, h, T, P, t)
        vals = {int(img[y, x, 3]) for y in ys for x in xs}
        flags[t] = int(len(vals) > 1)
    return flags


def sparse(w, h, dtype, seed, n):
    """Constant alpha with n seeded samples changed: most tiles flat, some not."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(h, w, 4)).astype(dtype)
    img[:, :, 3] = 200
    for _ in range(n):
        img[rng.integers(0, h), rng.integers(0, w), 3] = 199
    return img


@pytest.mark.parametrize("w,h,t,p", [(83, 44, 16, 10), (84, 44, 16, 10), (36, 28, 24, 10), (35, 25, 16, 10), (7, 9, 16, 10), (3, 50, 16, 10),
                                     (1, 1, 16, 10), (40, 1, 16, 10), (1, 40, 16, 10), (33, 17, 16, 0), (48, 32, 16, 3)])
def test_varies_is_the_brute_force_rule(w, h, t, p):
    """The geometries of the GPU module, images narrower than the halo, single rows and columns, no halo, a tile-aligned image."""
    for seed, n in ((1, 0), (2, 1), (3, 2), (4, 5)):
        for dtype in (np.uint8, np.uint16):
            img = sparse(w, h, dtype, seed, n)
            got = AF.varies(img, t, p)
            assert got.dtype == np.uint8 and np.array_equal(got, brute(img, t, p)), (seed, n, dtype)
            if n == 0:
                assert not got.any()
    # every single pixel of a small image, one at a time
    if w * h <= 64:
        for y in range(h):
            for x in range(w):
                img = sparse(w, h, np.uint8, 9, 0)
                img[y, x, 3] = 1
                assert np.array_equal(AF.varies(img, t, p), brute(img, t, p))


def test_low_byte_alone_counts():
    """Two uint16 values that share a high byte are different."""
    img = sparse(W, H, np.uint16, 5, 0)
    img[:, :, 3] = 0x8000
    img[20, 40, 3] = 0x8001
    got = AF.varies(img, T, P)
    assert got.sum() > 0 and np.array_equal(got, brute(img, T, P))
    assert not AF.varies((img >> 8).astype(np.uint8), T, P).any()


@pytest.mark.parametrize("x,y,count", [(5, 5, 1), (6, 5, 2), (25, 0, 3), (26, 0, 2), (82, 43, 2), (69, 43, 2)])
def test_single_pixel_counts(x, y, count):
    """83 x 44 at tile 16, prepadding 10: the source rectangles begin at 0, 6, 22, 38, 54, 70 and end at 26, 42, 58, 74, 83, 83 along x, and
    at 0, 6, 22 / 26, 42, 44 along y: an off-by-one at either end changes one of these counts."""
    img = sparse(W, H, np.uint8, 6, 0)
    img[y, x, 3] = 7
    got = AF.varies(img, T, P)
    assert int(got.sum()) == count and np.array_equal(got, brute(img, T, P))


def test_select_takes_whole_rectangles():
    flags = np.array([0, 1, 1, 0, 0, 0] * 3, dtype=np.uint8)
    a, b = np.zeros((4 * H, 4 * W, 4), np.uint8), np.ones((4 * H, 4 * W, 4), np.uint8)
    got = AF.select(flags, a, b, W, H, T)
    assert (got[:, 64:192] == 1).all() and (got[:, :64] == 0).all() and (got[:, 192:] == 0).all()


def test_binding_exposes_alpha_adaptive():
    """A property of RealSR like alpha_net, and the header names the option and its stats."""
    import os

    import realsr_ncnn_vulkan_amd as R
    assert isinstance(R.RealSR.__dict__["alpha_adaptive"], property) and R.RealSR.alpha_adaptive.fset is not None
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "realsr_hip.h")) as fh:
        text = fh.read()
    assert '"alpha_adaptive"' in text and '"alpha_tiles_flat"' in text
