"""Far image layouts for the 64-bit addressing tests (tests/test_far_layout.py on the CPU, tests/test_gpu_far_addressing.py on the GPU):
surfaces whose rows or planes lie beyond 2^31 and 2^32 bytes from their data pointer, and the arena they live in.

Pure Python and numpy; torch is imported only inside the functions that allocate or touch device memory.

One image serves every case: 52 x 44 at tile 32, prepadding 10 -- 2 x 2 tiles with partial last tiles both ways, a padded last column of
40 (a folded column of 8), and every reduced size even: x4 208 x 176, x2 104 x 88, 3/2 78 x 66 (tile rectangles of 48), x1 52 x 44.

A layout is (row_pitch, plane_pitch) in bytes for a surface of `h` rows:
  R   far rows.    row_pitch P = the smallest admissible pitch with (h - 6) * P >= 2^32 (a multiple of the element size; uint8: P = 0 mod 4,
                   or the `odd` variant P = 1 mod 4 that is no multiple of the pixel size).  Planar planes sit side by side inside the
                   pitch (plane_pitch 1 MiB + 64 elements); the UV plane of NV12 / P010 starts at (h / 2) * P + 4096, so its rows cross
                   2^32 themselves.
  Pn  far planes.  row_pitch = the bytes of a row + 16; plane_pitch 2^31 + 4096 (planar: plane 1 lies beyond 2^31, plane 2 beyond 2^32)
                   or 2^32 + 4096 (the UV plane of NV12 / P010).  A uint8 HWC image has no planes: no Pn layout.
  M   the admitted maximum, for inputs and diff operands: row_pitch 2^31 - 1 (one-byte elements) or 2^31 - 4, the image 52 x 3 (a
                   surface: 52 x 2, whose UV row takes the place of row 2): row 1 crosses 2^31 and row 2 crosses 2^32 in mid-row.

An arena is ONE uint8 device tensor filled with 0xCD; the image base lies 2^31 bytes in, and behind the base the arena is as long as the
longest window, and at least 2^32 + a row, + 4096.  An offset narrowed to 32 bits -- its low 32 bits zero-extended, the same
sign-extended, or an `int` product added to a correct 64-bit rest -- lands in [data - 2^31, data + 2^32 + a row): inside the arena,
whatever the layout.  A defect then shows as a failed comparison or a byte that is no longer 0xCD, never as an access outside the
allocation.  Several windows share an arena at different byte columns (COLS); one input and one output arena are all the GPU module holds.
"""
import numpy as np

from pixfmt_ref import ES, F16, F32, NP, NV12, P010, U8, image_at, is_yuv, plane_rows, shape_of  # noqa: F401  (the formats: tests/pixfmt_ref.py)

W, H, T, P = 52, 44, 32, 10
MH = 3  # rows of a layout-M image (a surface: 2)
B31, B32 = 1 << 31, 1 << 32
BASE = B31  # byte offset of the image base inside an arena
FILL = 0xCD
SIDE = 1 << 20  # planes side by side inside a far row pitch: SIDE + 64 elements apart
GIB = 1 << 30
CAP = 14 * GIB  # the most the GPU module may hold
HEADROOM = 4 * GIB  # ... and what must stay free beside it
SCAN_CHUNK = 256 << 20
TEMPORARIES = 512 << 20  # packed images, results, index tensors and scan()'s comparison results: far less than this
# (ow, oh) of the image at every output ratio the GPU module uses, as (numerator, denominator)
RATIOS = [(4, 1), (2, 1), (3, 2), (1, 1)]
SIZES = [(W * n // d, H * n // d) for n, d in RATIOS]
KINDS = ("R", "Pn", "M")


def rowbytes(fmt, w, c=3):
    return w * (c if fmt == U8 else ES[fmt])


def cols(fmt, kind="R"):
    """Byte columns of the (up to four) windows that share an arena.  Window 1 is co-aligned with window 0 to 16 bytes, window 2 agrees
    with window 1 modulo 4 only, window 3 with window 2 modulo the element size only.  The rows of a Pn window follow each other tightly,
    so there the windows lie a further MiB apart (a plane is at most 176 rows of 848 bytes)."""
    base = (0, 8192, 16404, 24596 + ES[fmt])
    return tuple(k * SIDE + b for k, b in enumerate(base)) if kind == "Pn" else base


def far_row_pitch(fmt, h, c=3, odd=False):
    """Layout R: the smallest admissible row pitch P with (h - 6) * P >= 2^32."""
    p = -(-B32 // (h - 6))
    if ES[fmt] == 1:
        while p % 4 != (1 if odd else 0) or (odd and p % c == 0):
            p += 1
        return p
    assert not odd
    return -(-p // ES[fmt]) * ES[fmt]


def layout(kind, fmt, w, h, c=3, odd=False):
    """(row_pitch, plane_pitch) in bytes; plane_pitch 0 for uint8 HWC."""
    es = ES[fmt]
    if kind == "R":
        rp = far_row_pitch(fmt, h, c, odd)
        return rp, (0 if fmt == U8 else ((h // 2) * rp + 4096 if is_yuv(fmt) else SIDE + 64 * es))
    assert not odd
    if kind == "Pn":
        assert fmt != U8
        return rowbytes(fmt, w, c) + 16, (B32 if is_yuv(fmt) else B31) + 4096
    assert kind == "M"
    rp = B31 - 1 if es == 1 else B31 - 4
    return rp, (0 if fmt == U8 else (h * rp if is_yuv(fmt) else SIDE + 64 * es))


def span(fmt, w, h, c, row_pitch, plane_pitch):
    """Bytes from the data pointer to one past the last byte of the image (what rsr_image_span returns)."""
    last = rowbytes(fmt, w, c)
    if is_yuv(fmt):
        return plane_pitch + (h // 2 - 1) * row_pitch + last
    return (0 if fmt == U8 else 2 * plane_pitch) + (h - 1) * row_pitch + last


class Window:
    """An image of one layout at a byte column of an arena.  Offsets count from the arena's image base (BASE bytes into the tensor)."""

    def __init__(self, kind, fmt, w, h, c=3, odd=False, col=0):
        self.kind, self.fmt, self.w, self.h, self.c, self.odd, self.col = kind, fmt, w, h, c, odd, col
        self.row_pitch, self.plane_pitch = layout(kind, fmt, w, h, c, odd)
        self.rowbytes = rowbytes(fmt, w, c)
        self.span = span(fmt, w, h, c, self.row_pitch, self.plane_pitch)
        self.nbytes = sum(plane_rows(fmt, h)) * self.rowbytes  # of the packed image

    def __repr__(self):
        return "Window(%s fmt %d %dx%dx%d%s col %d: pitches %d, %d)" % (self.kind, self.fmt, self.w, self.h, self.c, " odd" if self.odd else "",
                                                                        self.col, self.row_pitch, self.plane_pitch)

    def row_starts(self):
        """[(plane, row, offset from this window's data pointer)] of every row, in the order of the packed image."""
        return [(q, y, q * self.plane_pitch + y * self.row_pitch) for q, n in enumerate(plane_rows(self.fmt, self.h)) for y in range(n)]

    def offsets(self):
        """(far, rest): int64 arrays over every byte of the image in packed order; the byte lies at data + far + rest, where far is the
        64-bit part of the address arithmetic (plane * plane_pitch + row * row_pitch) and rest the byte inside its row."""
        far = np.repeat(np.array([o for _, _, o in self.row_starts()], dtype=np.int64), self.rowbytes)
        rest = np.tile(np.arange(self.rowbytes, dtype=np.int64), len(far) // self.rowbytes)
        return far, rest

    def tail(self):
        """How far behind the image base an arena must reach for this window: its bytes, and every narrowed offset of them."""
        return self.col + max(self.span, B32 + self.rowbytes)

    def desc(self, arena):
        """The rsr_image descriptor (ptr, row_pitch, plane_pitch) of the window inside the device tensor `arena`."""
        return (arena.data_ptr() + BASE + self.col, self.row_pitch, self.plane_pitch)


def group(kind, fmt, w, h, c=3, odd=False, n=4):
    """n windows of one layout that share an arena, at the columns cols()."""
    return [Window(kind, fmt, w, h, c, odd, col) for col in cols(fmt, kind)[:n]]


def alias32(off, rest=0):
    """The three wrapped forms of the byte offset off + rest (Python ints or int64 arrays), where off is what a kernel must form in 64
    bits: the low 32 bits of the sum zero-extended; the same sign-extended; off wrapped to an `int` and added to the correct rest."""
    total = off + rest
    zext = total & 0xFFFFFFFF
    sext = ((total + B31) & 0xFFFFFFFF) - B31
    prod = ((off + B31) & 0xFFFFFFFF) - B31 + rest
    return zext, sext, prod


# ---- the catalogue: every window the GPU module uses, so that the CPU module can check them all -------------------------------------------
def formats():
    """(fmt, c, odd) of every surface format and uint8 pitch variant."""
    return [(U8, 3, False), (U8, 3, True), (U8, 4, False), (U8, 4, True), (F16, 3, False), (F32, 3, False), (NV12, 3, False), (P010, 3, False)]


def m_size(fmt):
    return (W, 2) if is_yuv(fmt) else (W, MH)


def catalogue():
    """Every group of windows sharing an arena: layout x format x size.  Layout M comes at its own size only and has no odd variant."""
    out = []
    for fmt, c, odd in formats():
        for w, h in SIZES:
            out.append(group("R", fmt, w, h, c, odd))
            if fmt != U8:
                out.append(group("Pn", fmt, w, h, c))
        if not odd:
            out.append(group("M", fmt, *m_size(fmt), c=c))
    return out


def arena_bytes(groups=None):
    """Bytes of an arena that holds any group of the catalogue: BASE in front of the image base, the longest tail + 4096 behind it,
    rounded up to 4 KiB (a whole number of every element, so that typed views of the tensor exist)."""
    tail = max(wn.tail() for g in (groups if groups is not None else catalogue()) for wn in g)
    return -(-(BASE + tail + 4096) // 4096) * 4096


def held_bytes():
    """What the GPU module holds at most: the input arena, the output arena and its temporaries."""
    return 2 * arena_bytes() + TEMPORARIES


def memory_skip_reason(free):
    """None, or why the GPU module cannot run with `free` bytes of device memory: it names both figures."""
    need = held_bytes() + HEADROOM
    if free >= need:
        return None
    return "far addressing needs %.2f GiB of free device memory (%.2f GiB held + 4 GiB headroom), %.2f GiB are free" % (need / GIB, held_bytes() / GIB, free / GIB)


# ---- where a surface crosses 2^31 and 2^32 ------------------------------------------------------------------------------------------------
def rect_rows(rows):
    """The (first, end) row spans of the tile rectangles a surface of `rows` rows of the 52 x 44 image is read or written by: the output
    rectangles at the ratio rows / 44, and for the image's own size the (overlapping) source rectangles too."""
    ny = -(-H // T)
    n_d = [r for r, s in zip(RATIOS, SIZES) if s[1] == rows]
    assert n_d, rows
    n, d = n_d[0]
    spans = [(yi * T * n // d, min((yi + 1) * T, H) * n // d) for yi in range(ny)]
    if rows == H:
        spans += [(max(yi * T - P, 0), min(min((yi + 1) * T, H) + P, H)) for yi in range(ny)]
    return spans


def crossings(win):
    """For B in (2^31, 2^32): where the window's bytes first lie beyond B, as a list of (B, what, plane, row):
    "row"   the first row of a plane whose rows start on both sides of B;
    "plane" a plane that starts beyond B while the plane in front of it starts below B;
    "mid"   a row that starts below B and ends beyond it."""
    found = []
    starts = win.row_starts()
    for B in (B31, B32):
        for q, n in enumerate(plane_rows(win.fmt, win.h)):
            rows = [o for qq, _, o in starts if qq == q]
            if q > 0 and rows[0] >= B > [o for qq, _, o in starts if qq == q - 1][0]:
                found.append((B, "plane", q, 0))
            for y in range(n):
                if rows[y] < B < rows[y] + win.rowbytes:
                    found.append((B, "mid", q, y))
                elif y > 0 and rows[y - 1] + win.rowbytes <= B <= rows[y]:
                    found.append((B, "row", q, y))
    return found


# ---- images -------------------------------------------------------------------------------------------------------------------------------
image = image_at(W, H)  # a seeded random image in the library's packed layout


def raw(x):
    """The bytes of a packed numpy image, flat."""
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1)


# ---- a sparse arena for the CPU model -----------------------------------------------------------------------------------------------------
class SparseArena:
    """An arena as a dict of 4 KiB rows of bytes, each created full of 0xCD when first written: reads and writes at arrays of byte offsets
    from the image base (negative ones included), refused outside [-BASE, nbytes - BASE)."""
    ROW = 4096

    def __init__(self, nbytes):
        self.nbytes, self.rows = nbytes, {}

    def _check(self, addr):
        assert addr.size == 0 or (addr.min() >= -BASE and addr.max() < self.nbytes - BASE), "outside the arena"

    def write(self, addr, values):
        addr = np.asarray(addr, dtype=np.int64)
        self._check(addr)
        values = np.broadcast_to(np.asarray(values, dtype=np.uint8), addr.shape)
        key, at = (addr + BASE) // self.ROW, (addr + BASE) % self.ROW
        for k in np.unique(key):
            sel = key == k
            self.rows.setdefault(int(k), np.full(self.ROW, FILL, dtype=np.uint8))[at[sel]] = values[sel]  # (a later write to a byte wins)

    def read(self, addr):
        addr = np.asarray(addr, dtype=np.int64)
        self._check(addr)
        out = np.full(addr.shape, FILL, dtype=np.uint8)
        key, at = (addr + BASE) // self.ROW, (addr + BASE) % self.ROW
        for k in np.unique(key):
            if int(k) in self.rows:
                sel = key == k
                out[sel] = self.rows[int(k)][at[sel]]
        return out

    def untouched_outside(self, addr):
        """Does every byte that is not one of `addr` still hold 0xCD?"""
        mine = set((np.asarray(addr, dtype=np.int64) + BASE).tolist())
        for k, row in self.rows.items():
            for i in np.nonzero(row != FILL)[0]:
                if k * self.ROW + int(i) not in mine:
                    return False
        return True


# ---- device side (torch) ------------------------------------------------------------------------------------------------------------------
def new_arena(nbytes=None):
    import torch
    return torch.full((nbytes if nbytes is not None else arena_bytes(),), FILL, dtype=torch.uint8, device="cuda")


def byte_views(arena, win):
    """The window's planes as uint8 (rows, rowbytes) as_strided views of the arena, in the order of the packed image."""
    return [arena.as_strided((n, win.rowbytes), (win.row_pitch, 1), BASE + win.col + q * win.plane_pitch)
            for q, n in enumerate(plane_rows(win.fmt, win.h))]


def view(arena, lay, fmt, w, h, c=3, col=0):
    """The image of layout lay = (row_pitch, plane_pitch) at byte column `col` of the arena: its (ptr, row_pitch, plane_pitch) descriptor
    and an as_strided view of the arena -- uint8 (h, w, c); float (3, h, w); a surface: the pair (y (h, w), uv (h / 2, w)), P010 as int16."""
    import torch
    rp, pp = lay
    es = ES[fmt]
    assert (BASE + col) % es == 0 and rp % es == 0 and pp % es == 0
    d = (arena.data_ptr() + BASE + col, rp, pp)
    if fmt == U8:
        return d, arena.as_strided((h, w, c), (rp, c, 1), BASE + col)
    typed = arena.view({F16: torch.float16, F32: torch.float32, NV12: torch.uint8, P010: torch.int16}[fmt])
    at = (BASE + col) // es
    if is_yuv(fmt):
        return d, (typed.as_strided((h, w), (rp // es, 1), at), typed.as_strided((h // 2, w), (rp // es, 1), at + pp // es))
    return d, typed.as_strided((3, h, w), (pp // es, rp // es, 1), at)


def put(arena, win, x):
    """The packed numpy image x into the window."""
    import torch
    b = raw(x)
    assert b.size == win.nbytes
    at = 0
    for v in byte_views(arena, win):
        v.copy_(torch.from_numpy(b[at:at + v.numel()].reshape(v.shape).copy()).cuda())
        at += v.numel()


def get(arena, win):
    """The window's bytes in the order of the packed image, as a flat numpy uint8 array."""
    import torch
    return torch.cat([v.reshape(-1) for v in byte_views(arena, win)]).cpu().numpy()


def refill(arena, win):
    for v in byte_views(arena, win):
        v.fill_(FILL)


def scan(arena):
    """None where every byte of the arena holds 0xCD, else the index of the first one that does not.  Chunks of at most 256 MiB compared
    as int64: the largest temporary is a chunk's 32 MiB of comparison results."""
    import torch
    n = arena.numel()
    word = int(np.array([FILL] * 8, dtype=np.uint8).view(np.int64)[0])
    for o in range(0, n, SCAN_CHUNK):
        part = arena[o:min(o + SCAN_CHUNK, n)]
        m = part.numel() & ~7
        bad = part[:m].view(torch.int64) != word
        if bool(bad.any()):
            first = int(bad.to(torch.uint8).argmax()) * 8
            return o + first + int((part[first:first + 8] != FILL).to(torch.uint8).argmax())
        rest = part[m:] != FILL
        if bool(rest.any()):
            return o + m + int(rest.to(torch.uint8).argmax())
    return None
