"""The CPU side of tests/test_gpu_ws_hygiene.py: what its poisoned runs rest on, checked without the engine.

  1. 0 * NaN is NaN in numpy's fp16 and fp32 -- the arithmetic of the mirror -- so on the sparse exact model a stale NaN under ANY tap of a
     convolution reaches the output, not only one under its single non-zero weight.
  2. The two patterns decode to what the GPU module says: 0xFFFF is NaN as fp16, as fp32 and as an e5m2 residue byte; 0x7BFF is 65504 as
     fp16, 57344 and NaN as residue bytes, 2.6e36 as fp32.
  3. From the workspace table (csrc/workspace.h, restated here and held to the header's text): every case of the GPU module has a slot
     whose tile fills less than its capacity, or a block that dead-output elimination leaves unwritten -- bytes of the workspace that
     the call may read only by mistake.  The cases that have neither are single tiles that fill their slot exactly; they are listed by name."""
import os
import re

import numpy as np

import exact_net as N
import test_gpu_ws_hygiene as H   # the tables (importing it runs nothing on a GPU)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realsr-ncnn-vulkan_amd", "csrc")

# csrc/workspace.h kWsTable: (name, pixels per padded LR pixel, guarded hi planes, lo pair planes of precise mode, zeroed as a whole)
WS_TABLE = [("IN", 1, 2, 0, True), ("FEA", 1, 4, 2, False), ("RDB0", 1, 12, 2, False), ("RDB1", 1, 12, 2, False), ("RDB2", 1, 12, 2, False),
            ("UP1", 4, 4, 0, False), ("UP2", 16, 4, 0, False), ("HR", 16, 4, 0, False), ("OUT3", 16, 0, 0, False)]
BLK_H, BLK_W = 16, 32   # a work item's block (kernels.h kBlkH, kBlkW)


# ---- 1., 2. the poison ------------------------------------------------------------------------------------------------------------------
def test_zero_times_nan_is_nan_in_the_mirrors_arithmetic():
    for t in (np.float16, np.float32):
        nan = np.array([np.nan], t)
        with np.errstate(invalid="ignore"):
            assert np.isnan(np.zeros(1, t) * nan).all() and np.isnan(np.zeros(1, t) * nan + np.ones(1, t)).all()
            assert np.isnan(np.dot(np.zeros(9, t), np.full(9, np.nan, t)))
    # ... while the operations the kernels clamp with may swallow it: why the finite pattern is run as well
    assert np.fmax(np.float32(np.nan), np.float32(0)) == 0 and np.fmin(np.float32(np.nan), np.float32(1)) == 1


def e5m2(byte):
    """A residue byte (bf8 = e5m2) is the high byte of an fp16."""
    return np.array([byte << 8], np.uint16).view(np.float16)[0]


def test_the_patterns_decode_to_what_the_gpu_module_says():
    assert H.NAN == 0x10000 | 0xFFFF and H.BIG == 0x10000 | 0x7BFF and set(H.PATTERNS.values()) == {H.NAN, H.BIG}
    words = {k: np.array([v & 0xFFFF] * 2, np.uint16) for k, v in H.PATTERNS.items()}
    assert np.isnan(words["nan"].view(np.float16)).all() and np.isnan(words["nan"].view(np.float32)).all()
    assert np.isnan(e5m2(0xFF))                                    # both bytes of 0xFFFF
    assert (words["big"].view(np.float16) == np.float16(65504)).all() and np.isfinite(words["big"].view(np.float16)).all()
    assert e5m2(0x7B) == 57344 and np.isnan(e5m2(0xFF))            # the bytes of 0x7BFF
    f = words["big"].view(np.float32)[0]
    assert np.isfinite(f) and 2.6e36 < f < 2.7e36 and words["big"].view(np.uint32)[0] == 0x7BFF7BFF


# ---- 3. every case has bytes it must not read -------------------------------------------------------------------------------------------
def test_the_restated_table_is_the_headers():
    src = open(os.path.join(CSRC, "workspace.h")).read()
    names = [n.strip().replace("kWs", "").upper() for n in re.search(r"enum WsBuf \{([^}]*)\}", src).group(1).split(",")][:-1]
    assert names == [r[0] for r in WS_TABLE]
    rdb = re.search(r"kWsRdbRow = \{(\d+), (\d+), (\d+), (true|false)", src).groups()
    body = re.search(r"kWsTable\[kWsCount\] = \{(.*?)\n\};", src, re.S).group(1)
    rows = []
    for line in body.splitlines():
        for m in re.finditer(r"\{(\d+), (\d+), (\d+), (true|false), \{[^}]*\}\}|kWsRdbRow", line.split("//")[0]):
            rows.append(rdb if m.group(0) == "kWsRdbRow" else m.groups())
    assert [(int(a), int(b), int(c), d == "true") for a, b, c, d in rows] == [r[1:] for r in WS_TABLE]
    assert [r[0] for r in WS_TABLE if r[4]] == ["IN"]              # the one buffer whose slack a change of layout zeroes
    ks = open(os.path.join(CSRC, "kernels.h")).read()
    assert tuple(int(v) for v in re.search(r"constexpr int kBlkH = (\d+), kBlkW = (\d+);", ks).groups()) == (BLK_H, BLK_W)


def tail_margin(crop4, which):
    """engine.cpp tail_margin: 2 = upconv2 (the smallest margin of the 4x level), 3 = upconv1 (of the 2x level)."""
    if crop4 <= 0:
        return 0
    return max(crop4 - which if which <= 2 else crop4 // 2 - 2, 0)


def eliminated_blocks(th, tw, P):
    """Blocks of the 2x and 4x planes of one padded tile that append_block_items leaves out (block granularity; a folded last column is
    counted as the plain column it replaces)."""
    n = 0
    for lvl, which in ((1, 3), (2, 2)):
        Hh, Ww, m = th << lvl, tw << lvl, tail_margin(4 * P, which)
        for y0 in range(0, Hh, BLK_H):
            for x0 in range(0, Ww, BLK_W):
                n += y0 + BLK_H <= m or y0 >= Hh - m or x0 + BLK_W <= m or x0 >= Ww - m
    return n


def unwritten(kind, w, h, T, P, tta):
    """(slots with slack, eliminated blocks, tiles) of a case.  A slot's capacity is at least the largest padded tile of the image (its own
    plan; under TTA the transposed slots have the area of the upright ones) and a full tile's in a merged or masked batch; the one-tile
    hooks run one untrimmed slot of exactly the tile."""
    if kind == "tile":
        return 0, 0, 1
    tiles = [(tw + 2 * P, th + 2 * P) for _, _, tw, th in N.tile_grid(w, h, T)]
    cap = (T + 2 * P) ** 2 if kind == "full" else max(a * b for a, b in tiles)
    assert all(a * b <= cap for a, b in tiles)
    return sum(a * b < cap for a, b in tiles), sum(eliminated_blocks(b, a, P) for a, b in tiles), len(tiles)


# the cases with neither: one tile that fills its slot exactly, and no margin wide enough to free a block (the one-tile hooks trim
# nothing; at prepadding 3 the margins are 4 and 10 pixels)
NEITHER = ["mirror 9x21-t32-p3-tta", "mirror net_forward 44x20", "mirror net_forward 35x33", "mirror selfcheck 44x20", "mirror selfcheck 35x33"]


def test_every_case_has_slot_slack_or_eliminated_blocks():
    assert len(H.COVERAGE) >= len(H.G.CASES) + len(H.G.MIXED) + 10
    neither = []
    for name, (kind, w, h, T, P, tta) in H.COVERAGE.items():
        slack, dead, ntiles = unwritten(kind, w, h, T, P, tta)
        print("%-40s %2d tiles, %2d slots with slack, %4d eliminated blocks" % (name, ntiles, slack, dead))
        if not slack and not dead:
            assert ntiles == 1, name
            neither.append(name)
    assert neither == NEITHER
    # what the module's own geometries were chosen for
    for name in ("fresh %dx%d" % (H.DW, H.DH), "fresh nv12 %dx%d" % (H.YW, H.DH), "mirror outputs %dx%d" % (H.FW, H.FH)):
        slack, dead, ntiles = unwritten(*H.COVERAGE[name])
        assert ntiles >= 3 and slack >= 1 and dead >= 1, name
    a, b, c = ((w + 20) * (h + 20) for w, h in H.HISTORY)
    assert a == b and H.HISTORY[0] != H.HISTORY[1] and c < a       # equal capacity, other shape; then a smaller layout
    assert all(unwritten("full", w, h, H.G.MIXED_T, 10, 0)[0] >= 1 for w, h in H.G.MIXED)
