"""A two-term exact model of the WHOLE network and a numpy mirror of it (tests/test_exact_net.py, tests/test_gpu_exact_net.py).

tests/exact_conv.py makes ONE conv launch exactly summable with operands on a dyadic grid.  That grid does not survive the graph: the
residual scale is 0.2, so behind the first RDB every activation is a general fp16 value and a sum of several products needs more than
24 bits.  What does survive: an accumulator with AT MOST TWO non-zero terms is the exact sum of the two rounded once to fp32, in any
order (a + b = b + a; every other term is an exact zero), and that the hardware rounds such a sum to nearest even is a pinned fact
(test_gpu_exact.py test_accumulator_and_fp16_conversion_round_to_nearest_even).  So in this model

  * every output channel of every conv has exactly ONE non-zero weight, +-2^k at a seeded (input channel, ky, kx);
  * the second term is the bias (an odd multiple of 2^-14 that fp16 cannot hold) -- or, for the 69 RDB conv5s, whose bias is 0, the
    identity tap fp16(1 / 0.2f) * x = 5 * x the engine adds to carry the RDB's own input;
  * a conv5's weight for output channel o never reads the 32-channel input pair o lies in: the two products never meet in one MFMA.

The data is still real: every conv, tap position, 16-channel plane, residual and both up-samplings move position-dependent values, and
one changed input pixel changes hundreds of output pixels.  The mirror restates the rounding steps with exact_conv's epilogues; the
engine is right when its output equals the mirror's BIT FOR BIT.  No GPU code here.

What this model does not cover: the accumulation of many terms (that is test_gpu_exact.py's dyadic grid, one launch at a time).
"""
import numpy as np

import exact_conv as X
from realsr_ncnn_vulkan_amd import synth

NB = synth.NB
F32 = np.float32
IDT = F32(X.idt_coef(0.2))   # the identity tap's coefficient: fp16(1 / 0.2f) = 5
CLASSES = ("first", "dense", "conv5", "trunk", "up", "last")
# committed seed and gains (|w| is drawn from the pair): chosen so that the mirror alone meets the health conditions of
# tests/test_exact_net.py on the inputs the GPU tests use
SEED = 31
GAINS = dict(first=(0.25, 0.5), dense=(0.5, 1.0), conv5=(0.25, 0.5), trunk=(2.0 ** -5, 2.0 ** -4), up=(1.0, 2.0), last=(2.0, 4.0))


def conv_class(i):
    """Class of conv i in .bin order."""
    if i == 0:
        return "first"
    if i <= NB * 15:
        return "conv5" if (i - 1) % 5 == 4 else "dense"
    return ("trunk", "up", "up", "up", "last")[i - NB * 15 - 1]   # trunk_conv, upconv1, upconv2, HRconv, conv_last


class Layer:
    """The sparse description of one conv: output channel o reads wv[o] * x[c[o]] at tap (ky[o], kx[o]), plus b[o]."""

    def __init__(self, cin, c, ky, kx, wv, b):
        self.cin, self.c, self.ky, self.kx = cin, c, ky, kx
        self.wv, self.b = wv.astype(F32), b.astype(F32)

    def dense(self):
        w = np.zeros((len(self.c), self.cin, 3, 3), F32)
        w[np.arange(len(self.c)), self.c, self.ky, self.kx] = self.wv
        return w, self.b.copy()


def _odd_bias(rng, n, lo, hi):
    """Odd multiples of 2^-14 with lo <= |b| < hi, random sign."""
    m = rng.integers(int(lo * 2 ** 13), int(hi * 2 ** 13), n) * 2 + 1
    return np.where(rng.integers(0, 2, n) == 1, -m, m) / 2.0 ** 14


def make_model(seed=SEED, **gains):
    """The 351 Layers in .bin order.  gains: |w| choices per conv class (GAINS).  dense_weights(model) gives the (W, b) pairs for
    synth.write_bin(path, ..., "fp16")."""
    g = dict(GAINS, **gains)
    assert set(g) == set(CLASSES)
    rng = np.random.default_rng(seed)
    model = []
    for i, (cin, cout, _) in enumerate(synth.conv_specs()):
        cls = conv_class(i)
        c = rng.integers(0, cin, cout)
        ky, kx = rng.integers(0, 3, cout), rng.integers(0, 3, cout)
        if cls == "conv5":   # never the 32-channel input pair the identity tap of output channel o lies in
            c = rng.integers(0, cin - 32, cout)
            c = np.where(c >= np.arange(cout) // 32 * 32, c + 32, c)
            b = np.zeros(cout)
        elif cls == "last":  # (dy, cout) share the MFMA's M dimension: the three outputs take three rows, columns and planes
            ky, kx = rng.permutation(3), rng.permutation(3)
            c = rng.permutation(4)[:3] * 16 + rng.integers(0, 16, 3)
            b = 0.5 + _odd_bias(rng, cout, 2.0 ** -8, 2.0 ** -3)
        else:                # |b| >= 2^-3: fp16's ulp there is 2^-13 or more, an odd multiple of 2^-14 never fits
            b = _odd_bias(rng, cout, 2.0 ** -3, 2.0 ** -2)
        sign = np.where(rng.integers(0, 2, cout) == 1, 1.0, -1.0)
        if cls == "last":    # HRconv's output is mostly positive (LeakyReLU): one weight of each sign reaches both clamps
            sign[:2] = rng.permutation([1.0, -1.0])
        wv = rng.choice(g[cls], cout) * sign
        m, e = np.frexp(wv)
        assert (np.abs(m) == 0.5).all() and (e > -13).all(), "weights are +-2^k, fp16-normal"
        assert (b == 0).all() or (b.astype(np.float16).astype(np.float64) != b).all(), "a bias fp16 can hold"
        model.append(Layer(cin, c, ky, kx, wv, b))
    return model


def dense_weights(model):
    return [L.dense() for L in model]


# ---- the mirror ----------------------------------------------------------------------------------------------------------------
def taps(x16, L, ups=False):
    """x16 fp16 [n][cin][h][w] -> (fp16 [n][cout][h'][w'] with element o = x[c[o]] shifted by tap (ky[o], kx[o]), zero padded; the conv's
    input, up-sampled nearest x2 first with ups)."""
    if ups:
        x16 = x16.repeat(2, axis=2).repeat(2, axis=3)
    n, cin, h, w = x16.shape
    assert cin == L.cin
    xp = np.zeros((n, cin, h + 2, w + 2), np.float16)
    xp[:, :, 1:-1, 1:-1] = x16
    t = np.empty((n, len(L.c), h, w), np.float16)
    for ky in range(3):
        for kx in range(3):
            idx = np.nonzero((L.ky == ky) & (L.kx == kx))[0]
            if idx.size:
                t[:, idx] = xp[:, L.c[idx], ky:ky + h, kx:kx + w]
    return t, x16


def accumulate(L, t16, other, slow=False):
    """fl32(w * x_tap + other), ONE rounding, to nearest even.  w = +-2^k, so w * x_tap is exact in fp32 and the fp32 addition is that one
    rounding; slow = True computes the same through exact_conv.fma32 (float64 TwoSum) instead."""
    wv = L.wv[None, :, None, None]
    if slow:
        with np.errstate(invalid="ignore"):   # (fma32 checks its product by a division that is 0 / 0 where both factors are zero)
            return X.fma32(np.broadcast_to(wv, t16.shape), t16.astype(F32), np.broadcast_to(other, t16.shape))
    p = t16.astype(F32) * wv
    return p + other.astype(F32)


def forward(model, x16, slow=False, stats=None, fault=None, precise=False):
    """conv_last's fp32 accumulator [n][3][4h][4w] for the fp16 input x16 [n][3][h][w] (or [3][h][w] -> [3][4h][4w]): every stored
    activation rounded as conv3x3_flow's epilogues round it (exact_conv epi1 / epi2).  What the default path makes of the accumulator
    is fp16(acc) (half_out).
    precise: option "precise" = 1 -- the trunk's 64-channel tensors (conv_first, every RDB output) are kept as hi + lo / 2048 and rounded
    once per conv (exact_conv.epi_precise, conv_flow.hip EPI 4 / 5); the convs read the hi planes; conv_last's accumulator is what is
    converted (no fp16 rounding in between).
    stats: a dict that receives peak |activation|, the non-finite count and the fp16-subnormal count of the stored activations, and per
    convolution, in .bin order, "conv_peak" (the largest finite |stored fp16|; conv_last's entry is that of fp16(acc)) and
    "conv_nonfinite" (the stored values that are not finite) -- what the self-check's range probe reports; over several calls with one
    dict the lists hold the element-wise maximum and sum.
    fault: None, or a deliberate defect of the MIRROR (tests/test_exact_net.py shows that each one is seen):
      "slope16" the LeakyReLU slope held as fp16, "tap_x" the taps of ONE dense conv mirrored in x, "res_rrdb" one conv5's identity tap
      read from the RRDB's input instead of the RDB's."""
    x16 = np.asarray(x16, np.float16)
    single = x16.ndim == 3
    if single:
        x16 = x16[None]
    it = iter(enumerate(model))
    conv_peak, conv_bad = [], []

    def per_conv(a):
        fin = np.isfinite(a)
        conv_peak.append(float(a[fin].max()) if fin.any() else 0.0)
        conv_bad.append(int((~fin).sum()))

    def keep(v16):
        if stats is not None:
            a = np.abs(v16.astype(np.float64))
            per_conv(a)
            stats["peak"] = max(stats.get("peak", 0.0), float(a.max()))
            stats["nonfinite"] = stats.get("nonfinite", 0) + int((~np.isfinite(a)).sum())
            stats["subnormal"] = stats.get("subnormal", 0) + int(((a > 0) & (a < X.F16_MIN_NORMAL)).sum())
            stats["stored"] = stats.get("stored", 0) + a.size
        return v16

    def conv(x, ups=False, idt=None):
        i, L = next(it)
        if fault == "tap_x" and i == 172:
            L = Layer(L.cin, L.c, L.ky, 2 - L.kx, L.wv, L.b)
        t, xin = taps(x, L, ups)
        if idt is None:
            other = L.b[None, :, None, None]
        else:
            assert (L.b == 0).all()
            other = IDT * (idt if fault == "res_rrdb" and i == 175 else xin)[:, :len(L.c)].astype(F32)   # 3 + 11 bits: exact
        return accumulate(L, t, other, slow)

    def act(acc):
        if fault == "slope16":
            return X.f16(np.maximum(acc, acc * F32(np.float16(0.2))))
        return X.epi1(acc, True)

    if precise:
        assert fault is None
        fea, fea_lo = X.epi_precise(conv(x16), 1.0)
        cur, cur_lo = keep(fea), fea_lo
    else:
        fea = cur = keep(X.epi1(conv(x16), False))
    for _ in range(NB):
        rrdb_in, rrdb_lo = cur, cur_lo if precise else None
        for j in range(3):
            feats = cur
            for _ in range(4):
                feats = np.concatenate([feats, keep(act(conv(feats)))], axis=1)
            acc = conv(feats, idt=rrdb_in)
            if precise:
                cur, cur_lo = X.epi_precise(acc, 0.2, cur_lo, rrdb_in, rrdb_lo, 0.2) if j == 2 else X.epi_precise(acc, 0.2, cur_lo)
                keep(cur)
            else:
                cur = keep(X.epi2(acc, 0.2, rrdb_in, 0.2) if j == 2 else X.epi2(acc, 0.2))
    if precise:
        s = keep(X.epi_precise(conv(cur), 1.0, None, fea, fea_lo)[0])   # (only upconv1 reads it: no lo planes)
    else:
        s = keep(X.epi2(conv(cur), 1.0, fea, 1.0))
    s = keep(act(conv(s, ups=True)))
    s = keep(act(conv(s, ups=True)))
    s = keep(act(conv(s)))
    acc = conv(s)
    assert next(it, None) is None
    if stats is not None:
        with np.errstate(over="ignore"):   # (a model made to overflow: the cast to fp16 gives the infinities the engine stores)
            per_conv(np.abs(X.f16(acc).astype(np.float64)))
        assert len(conv_peak) == len(model)
        stats["conv_peak"] = [max(p) for p in zip(stats.get("conv_peak", conv_peak), conv_peak)]
        stats["conv_nonfinite"] = [a + b for a, b in zip(stats.get("conv_nonfinite", [0] * len(model)), conv_bad)]
    return acc[0] if single else acc


def half_out(acc):
    """What the default path makes of conv_last's accumulator: the reference's fp16 `output` blob, as fp32 (conv_flow.hip store3)."""
    return X.f16(acc).astype(F32)


# ---- images ---------------------------------------------------------------------------------------------------------------------
def halfs_of_u8(img):
    """uint8 HWC (RGB first) -> the network's fp16 input, planar: fp16(fl32(k * (1 / 255.f))) (kernels.hip preproc_tiles)."""
    return (np.asarray(img)[:, :, :3].astype(F32) * F32(1 / 255.0)).astype(np.float16).transpose(2, 0, 1)


def tile_grid(w, h, T):
    return [(x0, y0, min(x0 + T, w) - x0, min(y0 + T, h) - y0) for y0 in range(0, h, T) for x0 in range(0, w, T)]


def reflect101(v, n):
    """The engine's halo index (kernels.hip reflect101, after realsr_preproc.comp:59-62): ONE reflection at each end of 0 .. n - 1, then
    clamped -- where the halo is wider than the image (n <= P) the shader's single bounce leaves the image, and the engine and the
    oracle clamp.  numpy's "reflect" bounces as often as needed instead: the two agree while |v| and v - (n - 1) stay below n."""
    v = np.abs(np.asarray(v))
    v = (n - 1) - np.abs(v - (n - 1))
    return np.clip(v, 0, n - 1)


def padded_tile(x16, x0, y0, tw, th, P=10):
    """The padded network input of the tile at (x0, y0): reflect101 at the image border, real neighbours elsewhere."""
    _, h, w = x16.shape
    ys = reflect101(np.arange(y0 - P, y0 + th + P), h)
    xs = reflect101(np.arange(x0 - P, x0 + tw + P), w)
    return x16[:, ys[:, None], xs[None, :]]


def tta_variants(t):
    """The eight inputs preproc_tiles writes for the tile t [3][th][tw]: variant k holds t(gy, gx) at (oy, ox)."""
    _, th, tw = t.shape
    gy, gx = np.mgrid[0:th, 0:tw]
    maps = [(gy, gx, 0), (gy, tw - 1 - gx, 0), (th - 1 - gy, tw - 1 - gx, 0), (th - 1 - gy, gx, 0),
            (gx, gy, 1), (gx, th - 1 - gy, 1), (tw - 1 - gx, th - 1 - gy, 1), (tw - 1 - gx, gy, 1)]
    out = []
    for oy, ox, tr in maps:
        v = np.empty((3, tw, th) if tr else (3, th, tw), t.dtype)
        v[:, oy, ox] = t
        out.append(v)
    return out


def tta_merge(b):
    """postproc_tiles on the eight x4 outputs b[k] (fp32 [3][h][w], or [3][w][h] for k >= 4): (v0 + v1 + ... + v7) * 0.125f in fp32, in
    this order."""
    _, h, w = b[0].shape
    sy, sx = np.mgrid[0:h, 0:w]
    v = [b[0][:, sy, sx], b[1][:, sy, w - 1 - sx], b[2][:, h - 1 - sy, w - 1 - sx], b[3][:, h - 1 - sy, sx],
         b[4][:, sx, sy], b[5][:, sx, h - 1 - sy], b[6][:, w - 1 - sx, h - 1 - sy], b[7][:, w - 1 - sx, sy]]
    s = v[0].astype(F32)
    for t in v[1:]:
        s = s + t.astype(F32)
    return s * F32(0.125)


def image_x4(model, x16, T, P=10, tta=False, precise=False, pad=None, **kw):
    """The x4 image [3][4h][4w] as fp32, BEFORE the clamp and the conversion to the output format, for the fp16 image x16 [3][h][w] at
    tile size T: per tile the padded tile through forward(), the halo cropped.  Default: the fp16-rounded value; tta: the fp32 mean
    of the eight fp16 outputs; precise: conv_last's fp32 accumulator itself.  pad: another halo rule than padded_tile, same signature
    (tests/test_exact_geometry.py shows that a wrong one changes kept bytes)."""
    out_of = (lambda a: np.asarray(a, F32)) if precise else half_out
    kw["precise"] = precise
    _, h, w = x16.shape
    out = np.empty((3, 4 * h, 4 * w), F32)
    for x0, y0, tw, th in tile_grid(w, h, T):
        t = (pad or padded_tile)(x16, x0, y0, tw, th, P)
        if tta:
            vs = tta_variants(t)
            y = [out_of(a) for k in (0, 4) for a in forward(model, np.stack(vs[k:k + 4]), **kw)]
            v = tta_merge(y)
        else:
            v = out_of(forward(model, t, **kw))
        out[:, 4 * y0:4 * (y0 + th), 4 * x0:4 * (x0 + tw)] = v[:, 4 * P:4 * (P + th), 4 * P:4 * (P + tw)]
    return out


def to_u8(v):
    """floor(v * 255.f + 0.5f) clamped to 0..255 (post_store), planar.  The compiler may or may not fuse the multiply-add: the value must
    not depend on it (for an fp16-representable v both are exact)."""
    v = np.asarray(v, F32)
    two = np.floor(v * F32(255) + F32(0.5))
    one = np.floor((v.astype(np.float64) * 255.0 + 0.5).astype(F32))
    assert np.array_equal(one, two), "%d bytes depend on whether v * 255 + 0.5 is fused" % int((one != two).sum())
    return np.clip(two, 0, 255).astype(np.uint8)


def to_unit(v):
    """The planar float outputs: the value clamped to [0, 1] (post_store_planar / store3)."""
    return np.minimum(np.maximum(np.asarray(v, F32), F32(0)), F32(1))


# ---- the inputs the tests use (seeded; the CPU tests check the model's health on the very same ones) --------------------------------
TILE_SHAPES = [(20, 44), (33, 35), (16, 32), (17, 65)]   # (h, w) of the net_forward tiles
FRAME = (50, 40, 24)      # (w, h, tilesize): 3 x 2 tiles, the last column 2 px wide
TTA_FRAME = (30, 26, 16)  # the TTA context's image
TTA_GAINS = dict(last=(4.0, 8.0))  # the mean of eight variants is tamer than one output: a model with a louder conv_last reaches both clamps


def tile_f16(h, w):
    """General fp16 values in [0, 1]."""
    return np.random.default_rng(1000 * h + w).random((3, h, w), dtype=np.float32).astype(np.float16)


def frame_u8(w, h, c=3, seed=None):
    return np.random.default_rng(77 * w + h if seed is None else seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def tta_frame():
    return frame_u8(TTA_FRAME[0], TTA_FRAME[1], seed=5)


def frame_f16(w, h):
    return np.random.default_rng(99 * w + h).random((3, h, w), dtype=np.float32).astype(np.float16)
