"""CPU tests of the two-term exact model and its mirror (tests/exact_net.py): the model keeps its promises, the sparse mirror equals a
dense twin built on torch's conv2d, deliberate defects of the mirror are seen, and the model is healthy on the inputs of
tests/test_gpu_exact_net.py -- so that a bit-for-bit match with the engine there means something."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_conv as X
import exact_net as N

F32 = np.float32


@pytest.fixture(scope="module")
def model():
    return N.make_model()


@pytest.fixture(scope="module")
def dense(model):
    return N.dense_weights(model)


# ---- the model ------------------------------------------------------------------------------------------------------------------
def test_model_invariants(model, dense):
    """From the DENSE arrays: one non-zero weight per output channel, fp16-exact; with the bias or the identity tap at most two terms per
    accumulator; the conv5 rule; every conv class uses all nine taps and all of its 16-channel input planes."""
    specs = N.synth.conv_specs()
    assert len(dense) == len(specs) == 351
    used = {}
    for i, ((w, b), (cin, cout, _)) in enumerate(zip(dense, specs)):
        cls = N.conv_class(i)
        assert w.shape == (cout, cin, 3, 3) and b.shape == (cout,) and w.dtype == np.float32 and b.dtype == np.float32
        assert ((w != 0).reshape(cout, -1).sum(axis=1) == 1).all(), i
        assert np.array_equal(w.astype(np.float16).astype(np.float32), w), i
        o, c, ky, kx = np.nonzero(w)
        assert np.array_equal(o, np.arange(cout))
        m, _ = np.frexp(w[o, c, ky, kx])
        assert (np.abs(m) == 0.5).all(), "weights are powers of two: w * x is exact"
        if cls == "conv5":
            assert (b == 0).all() and (c // 32 != o // 32).all(), i   # terms: the product and the identity tap 5 * x[o]
        else:
            b64 = b.astype(np.float64)
            assert (b64 * 2 ** 14 % 2 == 1).all(), "biases are odd multiples of 2^-14"
            assert (b.astype(np.float16).astype(np.float32) != b).all(), "a bias fp16 can hold: rounding it would not show"
        key = cin if cls in ("first", "dense", "conv5") else "tail"
        t, p = used.setdefault(key, (set(), set()))
        t.update(zip(ky.tolist(), kx.tolist()))
        p.update((c // 16).tolist())
    assert set(used) == {3, 64, 96, 128, 160, 192, "tail"}
    for key, (t, p) in used.items():
        cin = 64 if key == "tail" else key
        assert len(t) == 9 and p == set(range((cin + 15) // 16)), key
    b_last = dense[-1][1]
    assert (np.abs(b_last - 0.5) < 0.125).all()
    assert len(set(np.nonzero(dense[-1][0])[2])) == 3 and (dense[-1][0] > 0).any() and (dense[-1][0] < 0).any()


# ---- the dense twin ---------------------------------------------------------------------------------------------------------------
def round_sum32(p, c):
    """The exact p + c (float64 values) rounded ONCE to fp32, to nearest even: TwoSum carries the exact sum as s + e, and e decides where
    s falls on an fp32 midpoint."""
    p, c = np.broadcast_arrays(np.asarray(p, np.float64), np.asarray(c, np.float64))
    s = p + c
    bp = s - c
    e = (p - bp) + (c - (s - bp))
    r = s.astype(F32)
    r64 = r.astype(np.float64)
    other = np.nextafter(r, np.where(s > r64, F32(np.inf), F32(-np.inf)).astype(F32))
    tie = (s != r64) & (np.abs(s - r64) == np.abs(other.astype(np.float64) - s))
    away = tie & (e != 0) & (np.sign(other.astype(np.float64) - s) == np.sign(e))
    return np.where(away, other, r).astype(F32)


def dense_forward(dense, x16):
    """The same rounding steps on the dense OIHW arrays with torch's conv2d in float64 (one non-zero product per output: exact)."""
    it = iter(dense)

    def conv(x, ups=False, idt=False):
        w, b = next(it)
        xt = torch.from_numpy(x.astype(np.float64))[None]
        if ups:
            xt = xt.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        p = F.conv2d(xt, torch.from_numpy(w.astype(np.float64)), padding=1)[0].numpy()
        other = 5.0 * x[:w.shape[0]].astype(np.float64) if idt else b.astype(np.float64)[:, None, None]
        return round_sum32(p, other)

    fea = X.epi1(conv(x16), False)
    cur = fea
    for _ in range(N.NB):
        rrdb_in = cur
        for j in range(3):
            feats = cur
            for _ in range(4):
                feats = np.concatenate([feats, X.epi1(conv(feats), True)])
            acc = conv(feats, idt=True)
            cur = X.epi2(acc, 0.2, rrdb_in, 0.2) if j == 2 else X.epi2(acc, 0.2)
    s = X.epi2(conv(cur), 1.0, fea, 1.0)
    s = X.epi1(conv(s, ups=True), True)
    s = X.epi1(conv(s, ups=True), True)
    s = X.epi1(conv(s), True)
    return conv(s)


@pytest.fixture(scope="module")
def twin(dense):
    x = N.tile_f16(20, 44)
    return x, dense_forward(dense, x)


def bits(a):
    return np.ascontiguousarray(a).view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def test_sparse_mirror_equals_the_dense_twin(model, twin):
    """Tap orientation, padding, the up-sampling and the graph's wiring against torch's definition, independently of the engine; the fast
    accumulate (an fp32 addition) against exact_conv.fma32."""
    x, want = twin
    assert X.idt_coef(0.2) == 5.0
    got = N.forward(model, x)
    assert got.shape == (3, 80, 176) and np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(N.forward(model, x, slow=True)), bits(want))
    pair = N.forward(model, np.stack([x, x[:, ::-1].copy()]))      # the batch dimension
    assert np.array_equal(bits(pair[0]), bits(want)) and not np.array_equal(bits(pair[1]), bits(want))


@pytest.mark.parametrize("fault", ["slope16", "tap_x", "res_rrdb"])
def test_a_broken_mirror_is_seen(model, twin, fault):
    """The evidence that a bit-for-bit comparison sees sub-code defects: a LeakyReLU slope held as fp16, the taps of ONE conv mirrored in x,
    ONE conv5 residual read from the RRDB's input -- each changes the fp16 output and the uint8 bytes of the dense twin's tile."""
    x, want = twin
    got = N.forward(model, x, fault=fault)
    nh = int((bits(X.f16(got)) != bits(X.f16(want))).sum())
    nb = int((N.to_u8(N.half_out(got)) != N.to_u8(N.half_out(want))).sum())
    print("%s: %d fp16 values, %d bytes of %d differ" % (fault, nh, nb, want.size))
    assert nh > 0 and nb > 0


def test_tta_transforms_invert_each_other():
    """tta_merge undoes tta_variants: with nearest x4 as the 'network' all eight terms are the same value."""
    t = N.tile_f16(5, 7)
    up = lambda v: v.astype(F32).repeat(4, axis=1).repeat(4, axis=2)   # noqa: E731
    vs = N.tta_variants(t)
    assert [v.shape for v in vs] == [(3, 5, 7)] * 4 + [(3, 7, 5)] * 4 and len({v.tobytes() for v in vs}) == 8
    assert np.array_equal(N.tta_merge([up(v) for v in vs]), up(t))


# ---- health: conditions on the model alone, on the inputs the GPU tests use ---------------------------------------------------------
def _spread(model, x16, th, tw):
    """Bounding box of the output pixels one changed input pixel (centre of the un-padded tile, +-0.25) changes."""
    t = N.padded_tile(x16, 0, 0, tw, th)
    t2 = t.copy()
    cy, cx = t.shape[1] // 2, t.shape[2] // 2
    t2[1, cy, cx] = np.float16(float(t[1, cy, cx]) + (0.25 if t[1, cy, cx] < 0.5 else -0.25))
    a, b = N.forward(model, np.stack([t, t2]))
    ys, xs = np.nonzero((bits(X.f16(a)) != bits(X.f16(b))).any(axis=0))
    return ys.max() - ys.min() + 1, xs.max() - xs.min() + 1


# The share of samples whose v * 255 lies within 2^-11 of a k + 0.5 boundary.  A value the conversion rounds (not clamps) is an fp16
# m * 2^-(11 + e) in [2^-(e + 1), 2^-e): 255 m mod 2^(11 + e) is uniform over the mantissas, and 2^(e + 1) + 1 of its 2^(11 + e) values lie
# within 2^e of the middle -- between 2^-10 and 3 / 2048 = 0.146 % of the samples, whatever conv_last's gain is (a gain moves values
# between binades, not within one); the fp32 mean under TTA is finer still (2 * 2^-11).  A larger share only comes from samples far
# outside [0, 1], where fp16 is coarse and the clamp decides the byte -- they are not counted here.  Half the lower figure is asked for.
NEAR_MIN = 0.5 * 2.0 ** -10


def check_health(model, x16, T, tta, u8):
    st = {}
    v = N.image_x4(model, x16, T, tta=tta, stats=st)
    n = v.size
    print("peak %.1f, %d subnormals of %d stored, below 0: %.2f %%, above 1: %.2f %%" % (
        st["peak"], st["subnormal"], st["stored"], 100 * (v < 0).mean(), 100 * (v > 1).mean()))
    assert st["nonfinite"] == 0 and np.isfinite(v).all()
    assert st["peak"] < 2.0 ** 12
    assert (v < 0).sum() >= 0.01 * n and (v > 1).sum() >= 0.01 * n, "both clamps"
    codes = len(np.unique(N.to_u8(v)))
    print("%d distinct uint8 codes" % codes)
    assert codes >= 100
    for q in range(3):
        assert ((v[q] >= 0) & (v[q] <= 1)).mean() >= 0.3, "channel %d is mostly clamped: its roundings would not show" % q
    if u8:
        e = v.astype(np.float64) * 255.0
        inr = (v >= 0) & (v <= 1)
        near = (np.abs(e - np.floor(e) - 0.5) <= 2.0 ** -11) & inr
        print("within 2^-11 of a k + 0.5 boundary: %.3f %% of the %d samples in [0, 1]" % (100 * near.sum() / inr.sum(), inr.sum()))
        assert near.sum() >= NEAR_MIN * inr.sum()
    return v


def test_health_uint8_frame(model):
    w, h, T = N.FRAME
    x16 = N.halfs_of_u8(N.frame_u8(w, h))
    check_health(model, x16, T, False, True)
    sy, sx = _spread(model, x16, T, T)
    print("one input pixel changes a %d x %d output region" % (sy, sx))
    assert sy >= 20 and sx >= 20


def test_health_bgr_and_rgba_frames(model):
    w, h, T = N.FRAME
    check_health(model, N.halfs_of_u8(N.frame_u8(w, h)[:, :, ::-1]), T, False, True)
    check_health(model, N.halfs_of_u8(N.frame_u8(w, h, 4)), T, False, True)


def test_health_fp16_frame(model):
    w, h, T = N.FRAME
    check_health(model, N.frame_f16(w, h), T, False, False)


def test_health_tta_frame():
    check_health(N.make_model(**N.TTA_GAINS), N.halfs_of_u8(N.tta_frame()), N.TTA_FRAME[2], True, True)


@pytest.mark.parametrize("h,w", N.TILE_SHAPES)
def test_health_tiles(model, h, w):
    st = {}
    v = N.forward(model, N.tile_f16(h, w), stats=st)
    assert st["nonfinite"] == 0 and np.isfinite(v).all() and st["peak"] < 2.0 ** 12
    assert (v < 0).mean() >= 0.01 and (v > 1).mean() >= 0.01 and len(np.unique(X.f16(v))) >= 100
