"""GPU tests of the workspace layout (csrc/workspace.h): what the engine allocates for a tile batch, to the byte, and that switching the
storage mode on a live context -- same slot capacity, other planes per slot -- changes no output.

The image is 70 x 20 at tilesize 32: three tiles in one row, the third narrower than the first two, so the three slots (capacity: the
largest padded tile, 52 x 40 = 2080 px at prepadding 10) hold tiles of different sizes.  merge = 1: the batch is the image's own plan."""
import os

import numpy as np
import pytest

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import synth

pytestmark = pytest.mark.gpu

W, H, TILE = 70, 20, 32
# per slot: guarded 16-channel planes (64 B guard + 32 B per pixel) of IN, FEA, 3 x RDB, UP1 (2x), UP2 and HR (4x), written out by hand;
# precise mode adds two residue planes to FEA and to each RDB buffer; the planar output has 3 x 16 halfs (floats) per LR pixel
PLANES = ((2, 1), (4, 1), (12, 1), (12, 1), (12, 1), (4, 4), (4, 16), (4, 16))  # (hi planes, pixels per LR pixel)
EXTRA_PRECISE = (0, 2, 2, 2, 2, 0, 0, 0)


def context(model_dir, precise):
    s = R.RealSR(0)
    s.load(os.path.join(model_dir, "x4.param"), os.path.join(model_dir, "x4.bin"))
    s.tilesize = TILE
    s.set_option("merge", 1)
    s.set_option("precise", precise)
    return s


def expected_bytes(s, precise):
    nx, ny = -(-W // s.tilesize), -(-H // s.tilesize)
    cap = (min(W, s.tilesize) + 2 * s.prepadding) * (min(H, s.tilesize) + 2 * s.prepadding)
    per_slot = sum((n + (e if precise else 0)) * (cap * level * 32 + 64) for (n, level), e in zip(PLANES, EXTRA_PRECISE))
    return nx * ny * (per_slot + cap * (192 if precise else 96))


@pytest.fixture(scope="module")
def fresh(model_dir):
    """Per channel count and storage mode: the output of a fresh context, and the workspace bytes it held after that one call."""
    out = {}
    for c in (3, 4):
        img = synth.make_image(11 + c, W, H, c)
        for precise in (0, 1):
            s = context(model_dir, precise)
            try:
                got = s.process(img)
                out[c, precise] = (img, got, round(s.get_stat("workspace_mb") * 1048576), expected_bytes(s, precise))
            finally:
                s.close()
    return out


@pytest.mark.parametrize("precise", [0, 1])
def test_workspace_allocation_to_the_byte(fresh, precise):
    """Three slots of 2080 px: 3 * (2080 * 6048 + 54 * 64) bytes in fp16 storage, 3 * (2080 * 6400 + 62 * 64) in precise mode."""
    _, _, held, want = fresh[3, precise]
    print("precise %d: workspace %d B, expected %d B" % (precise, held, want))
    assert want == (39947904 if precise else 37749888)
    assert held == want


@pytest.mark.parametrize("c", [3, 4])
def test_precise_toggle_changes_no_output(model_dir, fresh, c):
    """fp16, precise, fp16, precise on ONE context: every output equals the one of a fresh context in that mode (c = 4: the planar output
    blob and the post-processing launch)."""
    img = fresh[c, 0][0]
    s = context(model_dir, 0)
    try:
        got = []
        for precise in (0, 1, 0, 1):
            s.set_option("precise", precise)
            got.append(s.process(img).copy())
    finally:
        s.close()
    assert got[0].shape == (4 * H, 4 * W, c)
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[3])
    for i, precise in enumerate((0, 1, 0, 1)):
        assert np.array_equal(got[i], fresh[c, precise][1]), "call %d (precise %d) differs from a fresh context" % (i, precise)
