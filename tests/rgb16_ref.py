"""RSR_FMT_U16_HWC restated for the tests from include/realsr_hip.h ("16-bit RGB(A)"): the decode in front of the network, the encode behind
it, the alpha rule of the four depth pairs, and the packed-image helpers of tests/pixfmt_ref.py extended by the one format that module's
table does not hold.  numpy only; nothing here asks the library (the tie between the two is tests/test_rgb16_ref.py).

Every float32 operation below is one numpy operation on float32 arrays: rounded by itself, as the header demands."""
import numpy as np

import pixfmt_ref as F

U16 = 16
U8 = F.U8
NORM16 = np.float32(1) / np.float32(65535)  # fp32(1/65535): the constant of the decode
NORM8 = np.float32(1) / np.float32(255)
INV257 = np.float32(1) / np.float32(257)
TRAPS = (0, 1, 255, 256, 257, 32767, 32768, 65534, 65535)  # sign and byte-order traps of a 16-bit word


# ---- layout ---------------------------------------------------------------------------------------------------------------------------
def np_dtype(fmt):
    return np.dtype(np.uint16) if fmt == U16 else np.dtype(F.NP[fmt])


def shape_of(fmt, w, h, c=3):
    return (h, w, c) if fmt == U16 else F.shape_of(fmt, w, h, c)


def dims_of(fmt, x):
    return (x.shape[1], x.shape[0]) if fmt == U16 else F.dims_of(fmt, x)


def channels_of(fmt, x):
    return x.shape[2] if fmt in (U8, U16) else 3


def sentinel_bytes(fmt, shape):
    """A numpy image of the format, every byte 0xCD."""
    dt = np_dtype(fmt)
    return np.full(int(np.prod(shape)) * dt.itemsize, 0xCD, dtype=np.uint8).view(dt).reshape(shape)


def image16(seed, w, h, c=3, traps=True):
    """A seeded random uint16 HWC image over the whole code range; with `traps`, its first pixels carry TRAPS in every channel."""
    img = np.random.default_rng(seed).integers(0, 65536, size=(h, w, c), dtype=np.uint16)
    if traps:
        flat = img.reshape(-1, c)
        for i, k in enumerate(TRAPS):
            flat[i, :] = k
            flat[len(TRAPS) + i, i % c] = k  # ... and once more in one channel alone
    return img


def widen(img8):
    """An 8-bit image widened by x257: the same network input."""
    return (img8.astype(np.uint16) * np.uint16(257)).astype(np.uint16)


# ---- decode / encode --------------------------------------------------------------------------------------------------------------------
def decode(k):
    """uint16 samples -> the network's fp16 input: fp16_rn(float(k) * fp32(1/65535)), k unsigned."""
    k = np.asarray(k)
    assert k.dtype == np.uint16
    return (k.astype(np.float32) * NORM16).astype(np.float16)


def decode8(b):
    """uint8 samples -> the network's fp16 input (kernels.hip preproc_tiles; tests/exact_net.py)."""
    b = np.asarray(b)
    assert b.dtype == np.uint8
    return (b.astype(np.float32) * NORM8).astype(np.float16)


def as_f32_chw(img16):
    """The planar float32 image whose F32 -> X result a U16 -> X result must equal: k * fp32(1/65535), alpha dropped."""
    return np.ascontiguousarray((img16[:, :, :3].astype(np.float32) * NORM16).transpose(2, 0, 1))


def encode(d):
    """What RSR_FMT_F32_CHW holds (float32 in [0, 1], any shape) -> uint16 samples: floor(fl(fl(d * 65535) + 0.5))."""
    d = np.asarray(d)
    assert d.dtype == np.float32 and d.min() >= 0 and d.max() <= 1
    return np.floor(d * np.float32(65535) + np.float32(0.5)).astype(np.uint16)


# ---- alpha ----------------------------------------------------------------------------------------------------------------------------
def alpha_units(v, src_fmt, dst_fmt):
    """The bicubic sum v (float32, in the units of the source's samples) in the units of the destination's: one multiplication where the
    depths differ."""
    v = np.asarray(v, dtype=np.float32)
    if src_fmt == dst_fmt:
        return v
    return v * np.float32(257) if dst_fmt == U16 else v * INV257


def alpha_max(fmt):
    return 65535.0 if fmt == U16 else 255.0


def cubic_coeffs(w, outw, dx):
    """kernels.hip cubic_coeffs, statement for statement (ncnn's Interp bicubic, A = -0.75): (sx, the four float32 coefficients).  At x4
    every intermediate is a short dyadic number, so the float32 evaluation is exact whatever the order."""
    f = np.float32
    scale = f(w) / f(outw)
    fx = (f(dx) + f(0.5)) * scale - f(0.5)
    sx = int(np.floor(fx))
    fx = f(fx - f(sx))
    A = f(-0.75)
    fx0, fx1, fx2 = f(fx + f(1)), fx, f(f(1) - fx)
    c = [A * fx0 * fx0 * fx0 - f(5) * A * fx0 * fx0 + f(8) * A * fx0 - f(4) * A,
         (A + f(2)) * fx1 * fx1 * fx1 - (A + f(3)) * fx1 * fx1 + f(1),
         (A + f(2)) * fx2 * fx2 * fx2 - (A + f(3)) * fx2 * fx2 + f(1), None]
    c[3] = f(1) - c[0] - c[1] - c[2]
    z = f(0)
    if sx <= -1:
        sx, c = 1, [f(1) - c[3], c[3], z, z]
    if sx == 0:
        sx, c = 1, [c[0] + c[1], c[2], c[3], z]
    if sx == w - 2:
        sx, c = w - 3, [z, c[0], c[1], c[2] + c[3]]
    if sx >= w - 1:
        sx, c = w - 3, [z, z, c[0], f(1) - c[0]]
    return sx, [float(v) for v in c]


def bicubic_x4(a):
    """The bicubic x4 value of ONE tile's un-padded alpha rectangle a (h, w) integers, in float64 -- exact: samples below 2^16, coefficient
    products multiples of 2^-22, sixteen terms.  kernels.hip alpha_bicubic without its rounding: tap indices clamped to the rectangle."""
    h, w = a.shape
    a = a.astype(np.float64)
    out = np.zeros((4 * h, 4 * w), dtype=np.float64)
    cxs = [cubic_coeffs(w, 4 * w, x) for x in range(4 * w)]
    cys = [cubic_coeffs(h, 4 * h, y) for y in range(4 * h)]
    X = np.zeros((4 * w, w))
    for x, (bx, c) in enumerate(cxs):
        for i in range(4):
            X[x, min(max(bx - 1 + i, 0), w - 1)] += c[i]
    Y = np.zeros((4 * h, h))
    for y, (by, c) in enumerate(cys):
        for j in range(4):
            Y[y, min(max(by - 1 + j, 0), h - 1)] += c[j]
    out[:] = Y @ a @ X.T  # (every partial product and sum is exact in float64: 16 + 11 + 11 bits and a few carries)
    return out


def _fma(a, b, c):
    """fl32(a * b + c) with one rounding.  Exact here through float64: a product of a 24-bit and a 12-bit number and an addend on the grid of
    2^-22 below 2^18 fit 53 bits."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _dot4(p, c, chain):
    """p[0] c[0] + p[1] c[1] + p[2] c[2] + p[3] c[3] in float32 as the compiler lays the expression out -- chain "fma": the first product
    becomes the multiplicand of an fma whose addend is the second product, the others are folded in one by one
    (fma(p3, c3, fma(p2, c2, fma(p0, c0, p1 c1)))); "seq": fma(p3, c3, fma(p2, c2, fma(p1, c1, p0 c0))); "none": nothing is contracted."""
    if chain == "none":
        return ((p[0] * c[0] + p[1] * c[1]) + p[2] * c[2]) + p[3] * c[3]
    t = _fma(p[0], c[0], p[1] * c[1]) if chain == "fma" else _fma(p[1], c[1], p[0] * c[0])
    return _fma(p[3], c[3], _fma(p[2], c[2], t))


def bicubic_x4_f32(a, chain="fma"):
    """bicubic_x4 as kernels.hip alpha_bicubic evaluates it in float32: four rows of four taps, then the four rows (_dot4)."""
    h, w = a.shape
    af = a.astype(np.float32)
    cxs = [cubic_coeffs(w, 4 * w, x) for x in range(4 * w)]
    cys = [cubic_coeffs(h, 4 * h, y) for y in range(4 * h)]
    ix = np.array([[min(max(bx - 1 + i, 0), w - 1) for i in range(4)] for bx, _ in cxs])      # (4w, 4)
    iy = np.array([[min(max(by - 1 + j, 0), h - 1) for j in range(4)] for by, _ in cys])      # (4h, 4)
    cx = np.array([c for _, c in cxs], dtype=np.float32)
    cy = np.array([c for _, c in cys], dtype=np.float32)
    rows = []
    for j in range(4):
        src = af[iy[:, j]]  # (4h, w): the source row of every output row's tap row j
        rows.append(_dot4([src[:, ix[:, i]] for i in range(4)], [np.broadcast_to(cx[:, i], (4 * h, 4 * w)) for i in range(4)], chain))
    return _dot4(rows, [np.broadcast_to(cy[:, j:j + 1], (4 * h, 4 * w)) for j in range(4)], chain)


def alpha_x4(img_alpha, T, f32=None):
    """The x4 alpha in source units of every tile's un-padded rectangle of the alpha plane (h, w) at tile size T: exact in float64
    (bicubic_x4), or -- f32 = a chain of _dot4 -- as the kernel's float32 evaluation gives it."""
    h, w = img_alpha.shape
    out = np.empty((4 * h, 4 * w), dtype=np.float64 if f32 is None else np.float32)
    for y0 in range(0, h, T):
        for x0 in range(0, w, T):
            y1, x1 = min(y0 + T, h), min(x0 + T, w)
            out[4 * y0:4 * y1, 4 * x0:4 * x1] = bicubic_x4(img_alpha[y0:y1, x0:x1]) if f32 is None else bicubic_x4_f32(img_alpha[y0:y1, x0:x1], f32)
    return out


def alpha_chain(src_fmt):
    """The _dot4 chain of the kernel for a source format: a uint16 source's sums are pinned by the definition ("none": every operation
    rounded by itself); a uint8 source runs the uint8 path's own expression as the compiler contracts it ("fma" -- a sum of four 20-bit
    products is exact, so only the last of the five sums can tell the chains apart)."""
    return "none" if src_fmt == U16 else "fma"


def box_mean(c, k):
    """The mean of every k x k box of c (float32 (H, W), already clamped) in the order of option "out_scale": pairs along x, then pairs of
    rows (tests/box_reduce.py without its clamp to [0, 1])."""
    h, w = c.shape
    b = c.reshape(h // k, k, w // k, k)
    at = lambda y, x: b[:, y, :, x]  # noqa: E731
    if k == 2:
        return ((at(0, 0) + at(0, 1)) + (at(1, 0) + at(1, 1))) * np.float32(0.25)
    s = [(at(j, 0) + at(j, 1)) + (at(j, 2) + at(j, 3)) for j in range(4)]
    return ((s[0] + s[1]) + (s[2] + s[3])) * np.float32(0.0625)


def alpha_store(v, fmt):
    """floor(v + 0.5) clamped to the sample range of fmt (v float32, in the units of fmt)."""
    return np.clip(np.floor(np.asarray(v, dtype=np.float32) + np.float32(0.5)), 0, alpha_max(fmt)).astype(np_dtype(fmt))
