"""Network interpolation on the device (rsr_load_second, rsr_set_blend, rsr_model_export): the active blob byte for byte against the numpy
rule of tests/blend_ref.py, the outputs of a blended context against a context that loaded the expected blob, the call order, and the
whole of it once more under the workspace hook "ws_poison" (the active blob is then allocated over the hook's pattern, and the export
covers every byte of it: a stray or a missing store shows as a byte that differs from the rule).

1- and 2-block synthetic models (seeds 42 / 43), a 20 x 12 image at tile 16: two tiles."""
import os

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import synth

import blend_ref as BR
import gpu_support as G
import pixfmt_ref as F

pytestmark = pytest.mark.gpu

W, H, TILE, PAD = 20, 12, 16, 10
POISON = {"plain": 0, "poisoned": 0x1FFFF}   # option "ws_poison": off, every byte 0xFF (fp16 NaN)
T03 = float(np.float32(0.3))


def _paths(d):
    return os.path.join(d, "x4.param"), os.path.join(d, "x4.bin")


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """key -> ((dir A, dir B), (blob A, blob B)): the 1- and 2-block synthetic models and, under "x", the hand-made extreme pair."""
    tmp = tmp_path_factory.mktemp("gpu_blend_models")
    out = {}
    for nb in (1, 2):
        dirs = tuple(synth.make_model_dir(str(tmp), "models-DF2K-s%d" % seed, seed, nb=nb) for seed in (42, 43))
        out[nb] = (dirs, tuple(R.model_pack(*_paths(d)) for d in dirs))
    dirs = tuple(BR.extreme_pair(tmp, synth))
    out["x"] = (dirs, tuple(R.model_pack(*_paths(d)) for d in dirs))
    return out


_expected = {}


def expected(models, key, t):
    """blend_ref of the pair `key` at t: computed once per module, shared, read-only."""
    if (key, t) not in _expected:
        _expected[key, t] = BR.blend_ref(models[key][1][0], models[key][1][1], t)
        _expected[key, t].setflags(write=False)
    return _expected[key, t]


def context(poison=0, tta=False):
    s = R.RealSR(0, tta_mode=tta)
    s.tilesize, s.prepadding = TILE, PAD
    if poison:
        s.set_option("ws_poison", poison)
    return s


def load_second(s, models, key, source):
    dirs, blobs = models[key]
    if source == "files":
        s.load_second(*_paths(dirs[1]))
    elif source == "host":
        s.load_second_packed(blobs[1])
    else:
        d = G.dev(blobs[1])
        s.load_second_packed(d.numel(), device_ptr=d.data_ptr())
        del d   # the context keeps a copy of its own


def first_diff(got, want):
    got = np.frombuffer(got, dtype=np.uint8)
    assert got.size == want.size, (got.size, want.size)
    bad = np.flatnonzero(got != want)
    return "" if bad.size == 0 else "%d of %d bytes differ, first at %d: got %d want %d" % (bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


# ---- 1. the exported blob after a blend ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", list(POISON))
@pytest.mark.parametrize("source", ["files", "host", "device"])
@pytest.mark.parametrize("key", [1, 2, "x"], ids=["nb1", "nb2", "extreme"])
def test_export_after_blend_equals_the_rule(models, key, source, poison):
    s = context(POISON[poison])
    try:
        s.load(*_paths(models[key][0][0]))
        load_second(s, models, key, source)
        assert s.get_stat("second_loaded") == 1 and s.blend == 0.0
        msg = first_diff(s.export_model(), expected(models, key, 0.0))   # the copy of A the second load made
        assert not msg, ("after load_second", msg)
        for t in BR.T_VALUES + [0.5]:   # (and once more a strength that was already set: from 'below 1' back to the middle)
            s.blend = t
            assert s.blend == t
            msg = first_diff(s.export_model(), expected(models, key, t))
            assert not msg, (t, msg)
    finally:
        s.close()


# ---- 2. the exported blob of a plain load ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 2])
def test_export_of_a_plain_load_equals_model_pack(models, nb):
    s = context()
    try:
        s.load(*_paths(models[nb][0][0]))
        assert s.get_stat("second_loaded") == 0 and s.blend == 0.0
        assert not first_diff(s.export_model(), models[nb][1][0])
        s.load_packed(models[nb][1][1])
        assert not first_diff(s.export_model(), models[nb][1][1])
    finally:
        s.close()


# ---- 3. outputs ------------------------------------------------------------------------------------------------------------------------
IMG = synth.make_image(11, W, H)
IMG4 = synth.make_image(12, W, H, 4)


def _u8(s, x):
    return G.run(s, x, F.U8, F.U8)


def _f32(s, x):
    return G.run(s, (x.transpose(2, 0, 1).astype(np.float32) / np.float32(255)).copy(), F.F32, F.F32, nan=True)


def _precise(s, x):
    s.set_option("precise", 1)
    try:
        return s.process(x)
    finally:
        s.set_option("precise", 0)


def _half(s, x):
    s.out_scale = 2
    try:
        return s.process(x)
    finally:
        s.out_scale = 4


def _rgba_net(s, x):
    s.alpha_net = 1
    try:
        return s.process(IMG4)
    finally:
        s.alpha_net = 0


def _masked(s, x):
    """Tile 1 alone of the two: the other rectangle keeps the destination's fill."""
    d_in, d_out = G.dev(x), torch.full((4 * H, 4 * W, 3), 0xCD, dtype=torch.uint8, device="cuda")
    s.process_device_masked(d_in.data_ptr(), F.U8, W, H, 3, d_out.data_ptr(), F.U8, np.array([0, 1], dtype=np.uint8))
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


CALLS = [("process", lambda s, x: s.process(x)), ("device_u8", _u8), ("device_f32", _f32), ("precise", _precise), ("out_scale2", _half),
         ("rgba_alpha_net", _rgba_net), ("masked", _masked)]


def outputs(s, tta=False):
    """name -> bytes of every call of CALLS on the context (under TTA: process alone -- the other routes are no different there)."""
    return {name: np.ascontiguousarray(fn(s, IMG)).copy() for name, fn in (CALLS[:1] if tta else CALLS)}


def same_outputs(got, want):
    assert got.keys() == want.keys()
    return [name for name in got if got[name].shape != want[name].shape or not np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8))]


@pytest.mark.parametrize("poison", list(POISON))
@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
@pytest.mark.parametrize("nb", [1, 2])
def test_blended_context_computes_what_the_loaded_blend_computes(models, nb, tta, poison):
    dirs, blobs = models[nb]
    made = []

    def ctx():
        made.append(context(POISON[poison], tta))
        return made[-1]

    try:
        refs = {}
        for t, blob in ((0.0, blobs[0]), (1.0, blobs[1]), (T03, expected(models, nb, T03))):
            r = ctx()
            r.load_packed(blob)
            refs[t] = outputs(r, tta)
            r.close()
        for name, o in refs[T03].items():   # the three models do differ in what they compute, and none computes a flat image
            assert len(np.unique(o)) > 16, name
            assert not np.array_equal(o, refs[0.0][name]) and not np.array_equal(o, refs[1.0][name]), name
        s = ctx()
        s.load(*_paths(dirs[0]))
        s.load_second(*_paths(dirs[1]))
        assert same_outputs(outputs(s, tta), refs[0.0]) == []           # a second model alone changes nothing: strength 0 is A
        for t in (T03, 0.0, T03, 1.0):                                  # 0.3 -> 0 -> 0.3 reproduces the bytes; 1 is B
            s.blend = t
            assert s.get_stat("blend") == t and s.blend == t
            assert same_outputs(outputs(s, tta), refs[t]) == [], t
        assert s.get_stat("ws_guard_dirty") == 0
    finally:
        for c in made:
            c.close()


# ---- 4. state --------------------------------------------------------------------------------------------------------------------------
def test_call_order_and_refusals(models):
    dirs, blobs = models[1]
    s = context()
    try:
        with pytest.raises(R.RealSRError) as e:
            s.load_second(*_paths(dirs[1]))
        assert e.value.code == R.RSR_E_STATE
        with pytest.raises(R.RealSRError) as e:
            s.load_second_packed(blobs[1])
        assert e.value.code == R.RSR_E_STATE
        with pytest.raises(R.RealSRError) as e:
            s.blend = 0.5
        assert e.value.code == R.RSR_E_STATE
        with pytest.raises(R.RealSRError) as e:
            s.export_model()
        assert e.value.code == R.RSR_E_STATE
        s.load(*_paths(dirs[0]))
        with pytest.raises(R.RealSRError) as e:   # a first model alone: still nothing to blend with
            s.blend = 0.5
        assert e.value.code == R.RSR_E_STATE
        s.load_second_packed(blobs[1])
        for t in (float("nan"), -0.1, 1.5):
            with pytest.raises(R.RealSRError) as e:
                s.blend = t
            assert e.value.code == R.RSR_E_ARG
        assert s.blend == 0.0
        assert not first_diff(s.export_model(), blobs[0])
    finally:
        s.close()


@pytest.mark.parametrize("source", ["files", "host", "device"])
def test_second_model_of_another_depth_is_refused_and_changes_nothing(models, source):
    dirs, blobs = models[1]
    s, r = context(), context()
    try:
        r.load(*_paths(dirs[0]))
        want = r.process(IMG)
        s.load(*_paths(dirs[0]))
        with pytest.raises(R.RealSRError) as e:
            load_second(s, models, 2, source)
        assert e.value.code == R.RSR_E_GRAPH and "depth" in str(e.value)
        assert s.get_stat("second_loaded") == 0
        assert np.array_equal(s.process(IMG), want)
        # ... and with a pair in place: the pair stays, at its strength
        s.load_second_packed(blobs[1])
        s.blend = T03
        with pytest.raises(R.RealSRError) as e:
            load_second(s, models, 2, source)
        assert e.value.code == R.RSR_E_GRAPH
        with pytest.raises(R.RealSRError) as e:   # a blob cut short is no model at all
            s.load_second_packed(blobs[1][:-256])
        assert e.value.code == R.RSR_E_FORMAT
        assert s.get_stat("second_loaded") == 1 and s.blend == T03
        assert not first_diff(s.export_model(), expected(models, 1, T03))
    finally:
        s.close()
        r.close()


def test_a_new_first_model_drops_the_second_and_a_new_second_keeps_the_strength(models):
    dirs, blobs = models[2]
    s = context()
    try:
        s.load(*_paths(dirs[0]))
        s.load_second(*_paths(dirs[1]))
        s.blend = T03
        s.load_second_packed(blobs[0])          # another second model (A itself): the strength stays and the blend is made again
        assert s.blend == T03 and s.get_stat("second_loaded") == 1
        assert not first_diff(s.export_model(), BR.blend_ref(blobs[0], blobs[0], T03))
        s.load_second_packed(blobs[1])
        assert not first_diff(s.export_model(), expected(models, 2, T03))
        s.load(*_paths(dirs[1]))                # a new first model
        assert s.get_stat("second_loaded") == 0 and s.blend == 0.0
        assert not first_diff(s.export_model(), blobs[1])
        with pytest.raises(R.RealSRError) as e:
            s.blend = 0.5
        assert e.value.code == R.RSR_E_STATE
        s.load_second_packed(blobs[0])
        s.blend = 0.25
        s.load_packed(models[1][1][0])          # ... of another depth, from a blob
        assert s.get_stat("second_loaded") == 0 and s.blend == 0.0 and s.num_blocks == 1
        assert not first_diff(s.export_model(), models[1][1][0])
    finally:
        s.close()


def test_a_selfcheck_report_does_not_outlive_a_blend(models):
    dirs, blobs = models[1]
    s = context()
    try:
        s.load(*_paths(dirs[0]))
        s.load_second_packed(blobs[1])
        s.selfcheck()
        assert s.get_stat("selfcheck_headroom") != -1.0
        s.selfcheck_ranges()
        s.blend = T03
        assert s.get_stat("selfcheck_headroom") == -1.0
        with pytest.raises(R.RealSRError) as e:
            s.selfcheck_ranges()
        assert e.value.code == R.RSR_E_STATE
        s.selfcheck()                            # ... and describes the blended model when it runs again
        assert s.get_stat("selfcheck_headroom") != -1.0
        s.blend = T03                            # the same strength once more: still a model that changed hands
        assert s.get_stat("selfcheck_headroom") == -1.0
    finally:
        s.close()


def test_group_members_must_agree_on_the_blend(models):
    dirs, blobs = models[1]
    a, b = context(), context()
    try:
        for s in (a, b):
            s.load(*_paths(dirs[0]))
        want = R.process_group([a, b], IMG)
        a.load_second_packed(blobs[1])
        with pytest.raises(R.RealSRError) as e:   # one member with a second model, one without
            R.process_group([a, b], IMG)
        assert e.value.code == R.RSR_E_ARG
        b.load_second_packed(blobs[1])
        assert np.array_equal(R.process_group([a, b], IMG), want)   # both at strength 0: A
        a.blend, b.blend = T03, float(np.nextafter(np.float32(T03), np.float32(1)))
        with pytest.raises(R.RealSRError) as e:   # one ulp apart
            R.process_group([a, b], IMG)
        assert e.value.code == R.RSR_E_ARG and "blend" in str(e.value)
        b.blend = T03
        r = context()
        r.load_packed(expected(models, 1, T03))
        try:
            assert np.array_equal(R.process_group([a, b], IMG), r.process(IMG))
        finally:
            r.close()
    finally:
        a.close()
        b.close()
