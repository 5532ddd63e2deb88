"""rsr_model_blend, the host restatement of network interpolation (CPU, no GPU): whole blobs byte for byte against the numpy rule of
tests/blend_ref.py, the copies at t = 0 and t = 1, a hand-made pair of models at the edges of fp16, and every refusal."""
import ctypes as C
import os

import numpy as np
import pytest

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import synth

import blend_ref as BR


def _paths(d):
    return os.path.join(d, "x4.param"), os.path.join(d, "x4.bin")


@pytest.fixture(scope="module")
def blobs(tmp_path_factory):
    """(nb -> (blob A, blob B)) of the synthetic 1- and 2-block models, seeds 42 / 43, and "x" -> the hand-made extreme pair."""
    tmp = tmp_path_factory.mktemp("blend_models")
    out = {}
    for nb in (1, 2):
        out[nb] = tuple(R.model_pack(*_paths(synth.make_model_dir(str(tmp), "models-DF2K-s%d" % seed, seed, nb=nb))) for seed in (42, 43))
    out["x"] = tuple(R.model_pack(*_paths(d)) for d in BR.extreme_pair(tmp, synth))
    return out


def _raw(a, b, t, cap=None, want_dst=True):
    """(rc, need, dst) of one rsr_model_blend call on numpy uint8 arrays."""
    L = R.lib()
    need = C.c_size_t(0)
    dst = np.full(a.size if cap is None else cap, 0xCD, dtype=np.uint8) if want_dst else None
    rc = L.rsr_model_blend(a.ctypes.data_as(C.c_void_p), a.size, b.ctypes.data_as(C.c_void_p), b.size, C.c_float(t),
                           dst.ctypes.data_as(C.c_void_p) if want_dst else None, 0 if dst is None else dst.size, C.byref(need))
    return rc, need.value, dst


@pytest.mark.parametrize("key", [1, 2, "x"], ids=["nb1", "nb2", "extreme"])
@pytest.mark.parametrize("t", BR.T_VALUES, ids=BR.T_IDS)
def test_blend_equals_the_numpy_rule_byte_for_byte(blobs, key, t):
    a, b = blobs[key]
    got = np.frombuffer(R.model_blend(a, b, t), dtype=np.uint8)
    want = BR.blend_ref(a, b, t)
    assert got.size == a.size
    assert np.array_equal(got, want), "first differing byte at %d of %d" % (int(np.flatnonzero(got != want)[0]), a.size)
    if t == 0.0:
        assert np.array_equal(got, a)
    if t == 1.0:
        assert np.array_equal(got, b)


def test_the_extreme_pair_holds_what_it_is_made_for(blobs):
    """The hand-made pair does carry its cases into the packed blobs: the largest fp16 on both sides, subnormals, both zeros -- in the
    first conv, a dense conv and conv_last's aux image -- and its blends stay finite where both sides agree."""
    a, b = blobs["x"]
    segs = BR.segments(a)
    assert sum(1 for s in segs if s[2] == np.float16) == 21 + 1  # one w16 image per conv + conv_last's aux image
    aux = [s for s in segs if s[2] == np.float16][-1]
    first = [s for s in segs if s[2] == np.float16][0]
    for off, n, dt in (first, aux):
        ha, hb = a[off:off + n].view(np.uint16), b[off:off + n].view(np.uint16)
        assert (ha == 0x7BFF).any() and (hb == 0xFBFF).any()          # +-65504
        assert ((ha & 0x7C00) == 0).any() and ((ha & 0x7FFF) != 0).any() and (((ha & 0x7C00) == 0) & ((ha & 0x3FF) != 0)).any()  # subnormals
        assert ((ha == 0x0000) & (hb == 0x8000)).any() and ((ha == 0x8000) & (hb == 0x0000)).any()  # +0 against -0 and back
    c = np.frombuffer(R.model_blend(a, b, 0.5), dtype=np.uint8)
    off, n, dt = first
    hc = c[off:off + n].view(np.uint16)
    ha, hb = a[off:off + n].view(np.uint16), b[off:off + n].view(np.uint16)
    both_top = (ha == 0x7BFF) & (hb == 0x7BFF)
    assert both_top.any() and (hc[both_top] == 0x7BFF).all()          # 65504 with 65504 stays 65504 (no overflow to inf)
    assert (hc[(ha == 0x0000) & (hb == 0x8000)] == 0x0000).all()      # +0 with -0 is +0 under round to nearest
    assert (hc[(ha == 0x8000) & (hb == 0x8000)] == 0x8000).all()      # -0 with -0 stays -0
    neg = (ha ^ hb) == 0x8000
    assert neg.any() and ((hc[neg] & 0x7FFF) == 0).all()              # a = -b blends to zero at one half


def test_need_is_reported_without_a_destination(blobs):
    a, b = blobs[1]
    rc, need, _ = _raw(a, b, 0.3, want_dst=False)
    assert rc == R.RSR_OK and need == a.size


def test_destination_too_small_is_refused_and_left_alone(blobs):
    a, b = blobs[1]
    rc, need, dst = _raw(a, b, 0.3, cap=a.size - 1)
    assert rc == R.RSR_E_ARG and need == a.size
    assert (dst == 0xCD).all()


def test_depth_mismatch_is_a_graph_error(blobs):
    with pytest.raises(R.RealSRError) as e:
        R.model_blend(blobs[1][0], blobs[2][1], 0.5)
    assert e.value.code == R.RSR_E_GRAPH and "depth" in str(e.value) and "1 and 2" in str(e.value)


def test_differing_slope_names_the_convolution_and_the_field(blobs):
    a, b = blobs[2]
    b = b.copy()
    off = BR.HEADER.size + 7 * BR.ENTRY.size + 20   # the slope of convolution 7
    b[off:off + 4] = np.frombuffer(np.float32(0.1).tobytes(), dtype=np.uint8)
    with pytest.raises(R.RealSRError) as e:
        R.model_blend(a, b, 0.5)
    assert e.value.code == R.RSR_E_GRAPH and "convolution 7" in str(e.value) and "slope" in str(e.value)
    with pytest.raises(R.RealSRError) as e:   # ... whichever side carries it, and at the ends too: the copies are checked like the arithmetic
        R.model_blend(b, a, 1.0)
    assert e.value.code == R.RSR_E_GRAPH and "convolution 7" in str(e.value)


@pytest.mark.parametrize("cut", ["less1", "less256", "table", "header", "10bytes"])
@pytest.mark.parametrize("side", [0, 1])
def test_truncated_blobs_are_refused(blobs, cut, side):
    a, b = blobs[1]
    keep = {"less1": a.size - 1, "less256": a.size - 256, "table": BR.table_bytes(a), "header": BR.HEADER.size, "10bytes": 10}[cut]
    pair = [a, b]
    pair[side] = pair[side][:keep].copy()
    rc, need, dst = _raw(pair[0], pair[1], 0.5, cap=a.size)
    assert rc == R.RSR_E_FORMAT
    assert (dst == 0xCD).all()


@pytest.mark.parametrize("t", [float("nan"), -0.1, 1.5, float("inf"), -float("inf")], ids=["nan", "-0.1", "1.5", "inf", "-inf"])
def test_strengths_outside_the_unit_interval_are_refused(blobs, t):
    a, b = blobs[1]
    rc, need, dst = _raw(a, b, t)
    assert rc == R.RSR_E_ARG
    assert (dst == 0xCD).all()


def test_null_blobs_are_refused(blobs):
    a, b = blobs[1]
    L = R.lib()
    need = C.c_size_t(0)
    assert L.rsr_model_blend(None, a.size, b.ctypes.data_as(C.c_void_p), b.size, C.c_float(0.5), None, 0, C.byref(need)) == R.RSR_E_ARG
    assert L.rsr_model_blend(a.ctypes.data_as(C.c_void_p), a.size, None, b.size, C.c_float(0.5), None, 0, None) == R.RSR_E_ARG


def test_a_blend_is_a_loadable_blob(blobs):
    """What the blend returns passes the blob check again: blending it once more with B is accepted (header and table are A's)."""
    a, b = blobs[2]
    c = R.model_blend(a, b, 0.3)
    d = np.frombuffer(R.model_blend(c, b, 0.5), dtype=np.uint8)
    assert np.array_equal(d, BR.blend_ref(c, b, 0.5))
