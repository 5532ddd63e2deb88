"""The CPU side of tests/test_gpu_exact_geometry.py: what that module's bit-for-bit matches rest on, checked without the engine.

  1. The mirror's halo rule (exact_net.padded_tile: ONE reflection per end, then clamped) equals oracle.preproc on images smaller than,
     equal to and one over the halo -- where numpy's multi-bounce "reflect", which the mirror used before, differs.
  2. The coverage the GPU module claims follows from its tables: a table edit that loses a width class, a height class, a side of the
     fold limit or a crop fails HERE, not silently on the GPU.
  3. The one-block exact model is healthy on every case of the table: conditions on the reference alone.
  4. A halo defect is visible: a zero or an edge-replicated halo changes kept bytes of the mirror's output.
  5. The per-convolution peaks exact_net.forward hands to `stats` are those of the stored tensors."""
import os
import re

import numpy as np
import pytest

import depth_ref as D
import exact_conv as X
import exact_net as N
import oracle
import test_gpu_exact_geometry as G   # the tables (importing it runs nothing on a GPU)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fold_max():
    """kFoldMaxW as the kernels hold it."""
    src = open(os.path.join(ROOT, "realsr-ncnn-vulkan_amd", "csrc", "kernels.h")).read()
    return int(re.search(r"constexpr int kFoldMaxW = (\d+);", src).group(1))


# ---- 1. the halo rule -----------------------------------------------------------------------------------------------------------------
def numpy_reflect_tile(x16, x0, y0, tw, th, P=10):
    """The halo as the mirror built it before: numpy's "reflect" bounces as often as needed."""
    big = np.pad(x16, ((0, 0), (P, P), (P, P)), mode="reflect")
    return big[:, y0:y0 + th + 2 * P, x0:x0 + tw + 2 * P]


def other_halo(mode):
    def pad(x16, x0, y0, tw, th, P=10):
        big = np.pad(x16, ((0, 0), (P, P), (P, P)), mode=mode)
        return big[:, y0:y0 + th + 2 * P, x0:x0 + tw + 2 * P]
    return pad


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (10, 11), (11, 10)])
def test_padded_tile_equals_the_oracles_preproc(w, h):
    """Every tile at tile sizes 32 and 4 and prepaddings 10 and 3, cut as the reference cuts its row bands (realsr.cpp:401-404): the
    halfs of oracle.preproc -- fp16(k * (1 / 255.f)), the same as halfs_of_u8 -- bit for bit."""
    img = N.frame_u8(w, h)
    x16 = N.halfs_of_u8(img)
    for T in (32, 4):
        for P in (10, 3):
            for x0, y0, tw, th in N.tile_grid(w, h, T):
                b0, b1 = max(y0 - P, 0), min(y0 + T + P, h)
                want = oracle.preproc(np.ascontiguousarray(img[b0:b1]), tw + 2 * P, th + 2 * P, P, P, x0, min(y0, P))
                got = N.padded_tile(x16, x0, y0, tw, th, P)
                assert got.shape == want.shape and np.array_equal(got.view(np.uint16), want.view(np.uint16)), (T, P, x0, y0)


def test_halo_rules_differ_only_below_the_halo_size():
    """reflect101(-10, 5) = 0, numpy's reflect gives 2: the two rules part where the halo is as wide as the image or wider (P >= n), and
    agree on every image the mirror was used for before (the 50 x 40 and 30 x 26 frames)."""
    assert N.reflect101(-10, 5) == 0 and np.pad(np.arange(5), (10, 10), mode="reflect")[0] == 2
    x = N.halfs_of_u8(N.frame_u8(5, 3))
    assert not np.array_equal(N.padded_tile(x, 0, 0, 5, 3), numpy_reflect_tile(x, 0, 0, 5, 3))
    x = N.halfs_of_u8(N.frame_u8(10, 11))                      # P = n: the last halo column alone (9 - 10 clamps to 0, numpy bounces to 1)
    d = N.padded_tile(x, 0, 0, 10, 11) != numpy_reflect_tile(x, 0, 0, 10, 11)
    assert d[:, :, -1].any() and not d[:, :, :-1].any()
    for (w, h, T) in (N.FRAME, N.TTA_FRAME, (11, 11, 16), (12, 11, 8)):
        x = N.halfs_of_u8(N.frame_u8(w, h))
        for x0, y0, tw, th in N.tile_grid(w, h, T):
            assert np.array_equal(N.padded_tile(x, x0, y0, tw, th), numpy_reflect_tile(x, x0, y0, tw, th)), (w, h, T)


# ---- 2. the coverage claims, from the tables ------------------------------------------------------------------------------------------
def test_part_a_covers_every_width_and_height_class():
    shapes = [s for g in G.GROUPS.values() for s in g]
    assert len(shapes) == 174 and len(set(shapes)) == 171   # (17 x 32, 17 x 44 and 17 x 47 lie in both sweeps)
    assert list(G.GROUPS) == list(G.UPS_GROUPS)
    fm = fold_max()
    ws = {w for h, w in shapes if h == 17}
    assert ws == set(range(1, 67))
    for full in (0, 1):                                   # every residue of w % 32 with no and with one full block to its left
        assert {w % 32 for w in ws if w // 32 == full} == set(range(32))  - ({0} if full == 0 else set())
    assert {w % 32 for w in ws if w // 32 == 2} == {0, 1, 2}
    for full in (0, 1):                                   # the folded band on both sides of its limit
        assert {fm, fm + 1} <= {w % 32 for w in ws if w // 32 == full}
    for wd, rem in ((32, 0), (44, 12), (47, 15)):         # exact blocks, a folded strip, a plain remainder
        hs = {h for h, w in shapes if w == wd}
        assert hs == set(range(1, 37)) and wd % 32 == rem and (rem == 0 or (rem <= fm) == (wd == 44))
        assert {h % 16 for h in hs} == set(range(16)) and {h % 4 for h in hs} == set(range(4))
        assert max(hs) > 32                               # a pair of block rows plus an unpaired one
    # the up-sampling class: the OUTPUT plane takes the even sizes of the same sweep
    ups = [(2 * h, 2 * w) for g in G.UPS_GROUPS.values() for h, w in g]
    assert len(ups) == 87 and len(set(ups)) == 84
    assert {w for h, w in ups if h == 18} == set(range(2, 67, 2))
    assert {fm, fm + 2} <= {w % 32 for h, w in ups if h == 18 and w < 32} and {fm, fm + 2} <= {w % 32 for h, w in ups if h == 18 and w > 32}
    for wd in (32, 44, 48):
        assert {h for h, w in ups if w == wd} == set(range(2, 37, 2))
    for name, (cin, cout, form) in G.CLASSES.items():
        assert form in ("plain", "lrelu", "res", "precise", "ups"), name
    assert {(c[0], c[1]) for c in G.CLASSES.values()} == {(3, 64), (64, 32), (160, 32), (192, 64), (64, 64), (64, 3)}


def test_part_b_covers_both_sides_of_the_fold_limit_at_every_level_and_every_crop():
    fm = fold_max()
    assert fm == 14, "the case table was chosen for kFoldMaxW = 14: choose its neighbours again"
    nearest = {0: (14, 15), 1: (14, 16), 2: (12, 16)}     # the remainders next to the limit that a width << lvl can have
    for lvl in range(3):
        rems = set()
        for w, h, T, P, tta in G.CASES:
            for x0, y0, tw, th in N.tile_grid(w, h, T):
                rems.update(((a + 2 * P) << lvl) % 32 for a in ((tw, th) if tta else (tw,)))   # (TTA: the transposed slots are th wide)
        assert set(nearest[lvl]) <= rems, (lvl, sorted(rems))
        assert nearest[lvl][0] <= fm < nearest[lvl][1] and 0 in rems
    assert {4 * c[3] for c in G.CASES} == {0, 4, 8, 12, 20, 28, 40, 48}
    small = [c for c in G.CASES if min(c[0], c[1]) <= c[3]]                     # an image no larger than the halo, on either axis
    assert {(1, 1), (5, 3), (10, 11), (11, 10)} <= {(c[0], c[1]) for c in small}
    assert any(c[0] == 1 and c[1] > c[2] for c in G.CASES) and any(c[1] == 1 and c[0] > c[2] for c in G.CASES)   # one column / row, tiled
    assert any(c[2] > max(c[0], c[1]) for c in G.CASES)
    # several tiles: a last tile 1, 2 and 7 px wide or high, and a tile with real neighbours on all four sides
    multi = [c for c in G.CASES if G.ntiles(c) > 1]
    last = {(c[0] - 1) % c[2] + 1 for c in multi} | {(c[1] - 1) % c[2] + 1 for c in multi}
    assert {1, 2, 7} <= last
    assert any(c[0] > 2 * c[2] and c[1] > 2 * c[2] for c in multi)
    # TTA: a non-square edge tile (its transposed slots differ in shape from the upright ones), a tiny image, other prepaddings
    tta = [c for c in G.CASES if c[4]]
    assert len(tta) >= 4 and any(tw != th for c in tta for _, _, tw, th in N.tile_grid(c[0], c[1], c[2]))
    assert any(min(c[0], c[1]) < 10 for c in tta) and {c[3] for c in tta} >= {3, 5, 10}
    # precise: a tiny image, a prepadding other than 10, a multi-tile case
    assert len(G.PRECISE) == 6 and not any(c[4] for c in G.PRECISE)
    assert any(c[0] * c[1] <= 15 for c in G.PRECISE) and any(c[3] != 10 for c in G.PRECISE) and any(G.ntiles(c) > 1 for c in G.PRECISE)
    # the merged batch: eight different sizes between 1 x 1 and 40 x 33
    assert len(set(G.MIXED)) == 8 and (1, 1) in G.MIXED and (40, 33) in G.MIXED and all(w <= 40 and h <= 33 for w, h in G.MIXED)


# ---- 3. health of the mirror on the table's inputs ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    with D.depth(1):
        return D.make_model(1)


_x4 = {}


def x4(model, case, pad=None, key=None):
    """The mirror's x4 image of a case (and its stats), computed once."""
    k = (case, key)
    if k not in _x4:
        w, h, T, P, tta = case
        st = {}
        with D.depth(1):
            v = N.image_x4(model, N.halfs_of_u8(N.frame_u8(w, h)), T, P=P, tta=bool(tta), pad=pad, stats=st)
        v.setflags(write=False)
        _x4[k] = (v, st)
    return _x4[k]


def test_the_mirror_is_healthy_on_every_case(model):
    """No non-finite stored value; per case of at least 2,000 output samples both clamps are reached by at least 1 % of the samples
    (1 x 1, 48 samples, never reaches the upper one, 5 x 3 has 720 and 4 x 6 1,152: they count in the pooled condition only); pooled over the table at
    least 200 distinct uint8 codes.  Measured: 15 - 34 % below 0, 12 - 26 % above 1, 123 - 222 codes per case of that size."""
    codes = set()
    for case in G.CASES:
        v, st = x4(model, case)
        lo, hi, u = (v < 0).mean(), (v > 1).mean(), N.to_u8(v)
        print("%-22s %6d samples, %4.1f %% below 0, %4.1f %% above 1, %3d codes, peak %.1f" % (G.case_id(case), v.size, 100 * lo, 100 * hi, len(np.unique(u)), st["peak"]))
        assert st["nonfinite"] == 0 and np.isfinite(v).all() and sum(st["conv_nonfinite"]) == 0, case
        if v.size >= 2000:
            assert lo >= 0.01 and hi >= 0.01, case
        codes.update(np.unique(u).tolist())
    assert sorted(c for c in G.CASES if 3 * 16 * c[0] * c[1] < 2000) == [(1, 1, 32, 10, 0), (4, 6, 32, 10, 0), (5, 3, 32, 10, 0)]
    print("%d distinct uint8 codes over the table" % len(codes))
    assert len(codes) >= 200


# ---- 4. a halo defect is visible --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(5, 3, 32, 10, 0), (13, 33, 13, 10, 0), (43, 31, 21, 3, 0)], ids=G.case_id)
def test_a_wrong_halo_changes_kept_bytes(model, case):
    """The mirror run with a zero halo and with an edge-replicated one (both agree with reflect-101 on the image itself and differ from
    the first halo pixel on) changes bytes of the kept rectangle: an engine with such a halo would not pass as equal.  The one-block
    model carries a change about two LR pixels far, so numpy's multi-bounce halo -- which on 5 x 3 differs from the engine's only five
    and more pixels out -- is told apart at the tile (test_halo_rules_differ_only_below_the_halo_size), not at the bytes; its count is
    printed."""
    want = N.to_u8(x4(model, case)[0])
    for mode in ("constant", "edge"):
        n = int((N.to_u8(x4(model, case, other_halo(mode), mode)[0]) != want).sum())
        print("%s: a %s halo changes %d of %d kept bytes" % (G.case_id(case), mode, n, want.size))
        assert n > 0, (case, mode)
    if case[0] <= 5:
        n = int((N.to_u8(x4(model, case, numpy_reflect_tile, "reflect")[0]) != want).sum())
        print("%s: numpy's multi-bounce halo changes %d of %d kept bytes" % (G.case_id(case), n, want.size))


# ---- 5. the per-convolution peaks of forward() ---------------------------------------------------------------------------------------
def test_forward_reports_the_peak_of_every_stored_tensor(model):
    """stats["conv_peak"] / ["conv_nonfinite"]: one entry per conv in .bin order, the largest over them is stats["peak"] (conv_last's
    fp16(acc) included when it is the largest), the existing keys are what they were, and the model of the GPU module's overflow test
    overflows in conv_last alone -- some of its outputs, not all -- while the precise walk's fp32 output stays finite."""
    x = N.tile_f16(*G.HOT_TILE)
    with D.depth(1):
        st, plain = {}, {}
        acc = N.forward(model, x, stats=st)
        N.forward(model, x, stats=plain)
        assert len(st["conv_peak"]) == len(st["conv_nonfinite"]) == 21 and sum(st["conv_nonfinite"]) == 0
        assert max(st["conv_peak"][:-1]) == st["peak"] == plain["peak"] and st["stored"] == plain["stored"]
        assert st["conv_peak"][-1] == float(np.abs(X.f16(acc).astype(np.float64)).max())
        twice = dict(st)
        N.forward(model, x[:, ::-1].copy(), stats=twice)          # a second call with the same dict: element-wise maxima
        assert all(b >= a for a, b in zip(st["conv_peak"], twice["conv_peak"])) and twice["conv_peak"] != st["conv_peak"]
        hot = D.make_model(1, **G.HOT_GAINS)
        hs = {}
        with np.errstate(over="ignore"):
            hacc = N.forward(hot, x, stats=hs)
            inf = int(np.isinf(X.f16(hacc)).sum())
        assert hs["conv_nonfinite"][:-1] == [0] * 20 and hs["conv_nonfinite"][-1] == inf and 0 < inf < hacc.size
        assert hs["conv_peak"][:-4] == st["conv_peak"][:-4] and max(hs["conv_peak"][:-1]) < 2.0 ** 12 and 0 < hs["conv_peak"][-1] <= 65504
        assert np.isfinite(hacc).all() and np.isfinite(N.forward(hot, x, precise=True)).all()
