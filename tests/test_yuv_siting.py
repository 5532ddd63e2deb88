"""Chroma siting of the NV12 / P010 formats (option "yuv_siting": 0 centre, 1 left, 2 top-left): what can be said without a GPU -- the
numpy restatement the device tests compare against (tests/yuv_siting_ref.py) is checked against tests/yuv_ref.py (siting 0), against a
float64 restatement of the interpolation rules, and for sense: a surface written at one siting is read back best at that siting.  The
device side is tests/test_gpu_yuv_siting.py."""
import os

import numpy as np
import pytest

import realsr_ncnn_vulkan_amd as R

import yuv_ref
import yuv_siting_ref as ref

F = np.float32


def codes(seed, bits, w=36, h=26):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << bits, size=(h, w)), rng.integers(0, 1 << bits, size=(h // 2, w // 2, 2))


def test_header_documents_the_option():
    text = open(os.path.join(R.INCLUDE_DIR, "realsr_hip.h")).read()
    for needle in ('"yuv_siting"', "Chroma siting, exact", "(c[n] + c[min(n + 1, N/2 - 1)]) * 0.5f", "Hs(y) = (d(xl, y) + d(2X+1, y)) + (d(2X, y) + d(2X, y))",
                   "m = (Hs(2Y) + Hs(2Y+1)) * 0.125f", "m = ((Hs(yu) + Hs(2Y+1)) + (Hs(2Y) + Hs(2Y))) * 0.0625f", "chroma_sample_loc_type"):
        assert needle in text, needle


@pytest.mark.parametrize("bits", [8, 10])
def test_siting_0_is_yuv_ref(bits):
    y, uv = codes(1 + bits, bits)
    for matrix, full in ((709, 0), (2020, 1)):
        assert np.array_equal(ref.decode(y, uv, 0, matrix, full, bits).view(np.uint32), yuv_ref.decode(y, uv, matrix, full, bits).view(np.uint32))
        d = np.random.default_rng(3).uniform(0, 1, size=(3, 26, 36)).astype(F)
        for tile_out in (0, 16):
            got, want = ref.encode(d, 0, tile_out, matrix, full, bits), yuv_ref.encode(d, matrix, full, bits)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def upsample64(p, cos):
    """The interpolation rules along axis 0 in float64, written as weights: centre 3/4 - 1/4, cos 1 or 1/2 - 1/2."""
    half = p.shape[0]
    out = np.empty((2 * half,) + p.shape[1:], dtype=np.float64)
    for i in range(2 * half):
        n = i // 2
        if cos:
            out[i] = p[n] if i % 2 == 0 else 0.5 * p[n] + 0.5 * p[min(n + 1, half - 1)]
        else:
            out[i] = 0.75 * p[n] + 0.25 * p[min(max(n + (1 if i % 2 else -1), 0), half - 1)]
    return out


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("siting", [1, 2])
def test_decode_interpolation_is_exact(siting, bits):
    """Both rules are exact in float32 for 8- and 10-bit codes: the float32 result equals the float64 one, in either order of the axes."""
    _, uv = codes(10 * siting + bits, bits, 64, 48)
    hcos, vcos = ref.COS_AXES[siting]
    for q in range(2):
        p = uv[..., q]
        got = ref.upsample_axis(ref.upsample_axis(p.astype(F), 1, hcos), 0, vcos)
        want = upsample64(upsample64(p.astype(np.float64).T, hcos).T, vcos)
        other = upsample64(upsample64(p.astype(np.float64), vcos).T, hcos).T
        assert got.dtype == np.float32 and got.shape == (48, 64)
        assert np.array_equal(got.astype(np.float64), want) and np.array_equal(want, other)
        assert np.array_equal(got[0::2, 0::2], p) if siting == 2 else np.array_equal(got[:, 0::2], ref.upsample_axis(p.astype(F), 0, False))


def test_encode_luma_and_tile_grid():
    """Luma never depends on the siting; the tile grid changes chroma on tile-first columns (siting 2: and rows) only."""
    d = np.random.default_rng(5).uniform(0, 1, size=(3, 40, 64)).astype(F)
    y0, uv0 = yuv_ref.encode(d)
    for siting in (1, 2):
        y, uv = ref.encode(d, siting, 0)
        yg, uvg = ref.encode(d, siting, 16)
        assert np.array_equal(y, y0) and np.array_equal(yg, y0) and not np.array_equal(uv, uv0)
        diff = (uv != uvg).any(axis=-1)
        on_grid = np.zeros_like(diff)
        on_grid[:, 8::8] = True
        if siting == 2:
            on_grid[8::8, :] = True
        assert diff.any() and not (diff & ~on_grid).any()
        assert not diff[0, 0] and (siting == 2 or not diff[:, 0].any())  # (the image's first column / row is clamped with and without a grid)


def pattern(w=96, h=64):
    """A smooth coloured pattern: sinusoids of a few dozen pixels' period, another phase and direction per channel."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ch = [0.5 + 0.45 * np.sin(2 * np.pi * (xx / px + yy / py) + ph) for px, py, ph in ((31.0, 47.0, 0.0), (-37.0, 29.0, 1.0), (23.0, -41.0, 2.0))]
    return np.stack(ch).astype(F)


def test_round_trip_prefers_the_matching_siting():
    """A surface encoded at one siting and decoded at each of the three: the matching decoder has the smallest max RGB error (interior
    pixels: the edge clamps of the filters are not the point)."""
    d = pattern()
    err = {}
    for enc in (0, 1, 2):
        y, uv = ref.encode(d, enc, 0, 709, 1, 10)
        for dec in (0, 1, 2):
            back = ref.decode(y, uv, dec, 709, 1, 10)
            err[enc, dec] = float(np.abs(back - d)[:, 4:-4, 4:-4].max())
    print({k: round(v, 3) for k, v in err.items()})
    for enc in (0, 1, 2):
        others = [err[enc, dec] for dec in (0, 1, 2) if dec != enc]
        assert err[enc, enc] < min(others), (enc, err)
