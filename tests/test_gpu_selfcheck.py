"""Device self-check of a loaded model (rsr_selfcheck, option "precise_auto"; run with -m gpu on the MI355X box).

The self-check walks ONE tile through the network in fp16 storage (a range-probe launch behind every convolution) and in precise mode,
and compares the two results on the device.  Checked here: the report equals what the public entry points already say (exactly); the
estimate storage_err = max |default - precise| is a safe stand-in for e16 = max |default - fp32 oracle|; the decision; the option end
to end; that the check leaves no trace; the range probe against an fp32 walk; overflow; two contexts; the CLI.

Five stand-in models (profiles/selfcheck.txt), two tiles: the padded 148 x 148 tile of the C1 frame (synth.make_image(1234, 256, 256),
as tests/test_gpu_precise.py) and the built-in tile.  Figures are printed before they are asserted (pytest -s)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "realsr-ncnn-vulkan_amd", "bin", "realsr-hip")
STEP = 1.0 / 255.0

MODELS = {
    "42": (42, {}),
    "43": (43, {}),
    "44hot": (44, {"hot": 32.0, "last_gain": 0.15}),
    "45base": (45, {"chan_sigma": 1.0, "last_gain": 0.12}),
    "45wide": (45, {"chan_sigma": 1.0, "last_gain": 0.2}),
}


def model_paths(key):
    seed, kw = MODELS[key]
    d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K_sc_" + key, seed, **kw)  # (the CLI wants "models-DF2K" in the name)
    return os.path.join(d, "x4.param"), os.path.join(d, "x4.bin")


def c1_image():
    return synth.make_image(1234, 256, 256)


def tiles():
    big = np.pad(c1_image(), ((10, 10), (10, 10), (0, 0)), mode="reflect")
    photo = (big[:148, :148, :3].astype(np.float32).transpose(2, 0, 1) * np.float32(1 / 255.0)).astype(np.float16)
    return {"photo": np.ascontiguousarray(photo), "builtin": R.selfcheck_tile()}


_oracle_cache = {}


def oracle_forward(key, tname):
    """fp32 oracle on the very tile the engine gets (the fp16 values, widened)."""
    if (key, tname) not in _oracle_cache:
        net = oracle.OracleNet(*model_paths(key))
        _oracle_cache[(key, tname)] = net.forward(tiles()[tname].astype(np.float32))
    return _oracle_cache[(key, tname)]


_c1_cache = {}


def oracle_c1(key):
    if key not in _c1_cache:
        _c1_cache[key] = oracle.OracleNet(*model_paths(key)).process(c1_image(), 128)
    return _c1_cache[key]


def q_engine(v):
    """The engine's uint8 conversion (kernels.hip post_store(v * 255)): floor(v * 255 + 0.5), saturated -- the q of tests/test_gpu_precise.py,
    with the product and the sum rounded ONCE to fp32, as the device's fused multiply-add does (v * 255 + 0.5 is exact in float64 for
    an fp32 v).  For fp16 values the product is exact in fp32 and the two agree."""
    return np.clip(np.floor((v.astype(np.float64) * 255.0 + 0.5).astype(np.float32)), 0, 255)


def q_plain(v):
    return np.clip(np.floor(v * 255.0 + 0.5), 0, 255)  # tests/test_gpu_precise.py, every operation rounded to fp32


def open_model(key, **options):
    s = R.RealSR(0)
    for k, v in options.items():
        s.set_option(k, v)
    s.load(*model_paths(key))
    return s


def both_modes(s, tile):
    """(rsr_net_forward in fp16 storage as fp32, rsr_net_forward_f32 in precise mode); the context is left in fp16 storage."""
    s.set_option("precise", 0)
    a = s.net_forward(tile).astype(np.float32)
    s.set_option("precise", 1)
    b = s.net_forward_f32(tile)
    s.set_option("precise", 0)
    return a, b


# ---- 4. the report is what the public entry points already say ----------------------------------------------------------------
@pytest.mark.parametrize("key", ["42", "45wide"])
def test_report_equals_the_public_entry_points_exactly(key):
    s = open_model(key)
    try:
        for tname, tile in tiles().items():
            rep = s.selfcheck(tile if tname == "photo" else None)
            a, b = both_modes(s, tile)
            err = np.abs(a - b).max()
            qa, qb = q_engine(a), q_engine(b)
            dq = np.abs(qa - qb)
            plain = np.abs(q_plain(a) - q_plain(b))
            print("model %s, %s tile: storage_err report %.9e host %.9e | max_byte_diff %d / %d | bytes_differ %d / %d (q rounded per operation: %d) | %.2f ms" % (
                key, tname, rep["storage_err"], err, rep["max_byte_diff"], dq.max(), rep["bytes_differ"], (dq > 0).sum(), (plain > 0).sum(), rep["elapsed_ms"]))
            assert (rep["tile_w"], rep["tile_h"]) == (148, 148)
            assert np.float32(rep["storage_err"]).view(np.uint32) == np.float32(err).view(np.uint32)  # no tolerance: the same kernels, the same differences
            assert rep["max_byte_diff"] == int(dq.max())
            assert rep["bytes_differ"] == int((dq > 0).sum())
            assert np.float32(rep["headroom"]) == (np.float32(1.0) / np.float32(255.0)) / np.float32(rep["storage_err"])
            assert rep["recommend_precise"] == int(rep["headroom"] < 1.5)
            assert s.get_stat("selfcheck_headroom") == rep["headroom"] and s.get_stat("selfcheck_ms") == rep["elapsed_ms"]
        assert s.get_stat("selfcheck_runs") == 2
    finally:
        s.close()


# ---- 5. + 6. the estimator is safe; the decision --------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(MODELS))
def test_estimator_is_safe_and_the_decision(key):
    """storage_err >= (2/3) e16, e16 = max |rsr_net_forward - fp32 oracle| on the same tile.  Why 2/3: auto leaves a model in fp16 storage
    only when (1/255) / storage_err >= 1.5; with storage_err >= (2/3) e16 that implies (1/255) / e16 >= 1 -- the +-1 bar holds on the
    tile.  Decision: the wide-swing model goes to precise, models 42 and 43 stay; 44hot and 45base (near the threshold) are printed only."""
    s = open_model(key)
    try:
        for tname, tile in tiles().items():
            ref = oracle_forward(key, tname)
            rep = s.selfcheck(tile)
            a, b = both_modes(s, tile)
            e16, eP = float(np.abs(a - ref).max()), float(np.abs(b - ref).max())
            print("TABLE %-7s %-6s e16 %.3e (headroom %.2f)  eP %.3e  storage_err %.3e (est. headroom %.2f)  est/e16 %.3f  recommend_precise %d  peak %.4g @conv %d  %.2f ms" % (
                tname, key, e16, STEP / e16, eP, rep["storage_err"], rep["headroom"], rep["storage_err"] / e16, rep["recommend_precise"], rep["peak_abs"],
                rep["peak_conv"], rep["elapsed_ms"]))
            assert rep["storage_err"] >= (2.0 / 3.0) * e16
            assert rep["nonfinite"] == 0 and rep["fp16_overflow"] == 0
            if key == "45wide":
                assert rep["recommend_precise"] == 1
            if key in ("42", "43"):
                assert rep["recommend_precise"] == 0
    finally:
        s.close()


# ---- 7. end to end, nothing set but the new option ------------------------------------------------------------------------------
def test_precise_auto_end_to_end_on_the_wide_swing_model():
    img, want = c1_image(), oracle_c1("45wide")
    pp, bp = model_paths("45wide")
    plain = R.RealSR(0)
    plain.load(pp, bp)
    plain.tilesize = 128
    plain_bytes = plain.process(img)
    assert plain.get_stat("precise_active") == 0 and plain.get_stat("selfcheck_runs") == 0
    plain.close()
    print("45wide, C1 in fp16 storage: max |d| vs oracle = %d" % np.abs(plain_bytes.astype(int) - want.astype(int)).max())
    outs = []
    for how in ("option before load", "option after load", "load_packed"):
        s = R.RealSR(0)
        try:
            if how == "option after load":
                s.load(pp, bp)
                assert s.get_stat("precise_active") == 0
                s.set_option("precise_auto", 1)
            elif how == "option before load":
                s.set_option("precise_auto", 1)
                assert s.get_stat("selfcheck_runs") == 0
                s.load(pp, bp)
            else:
                s.set_option("precise_auto", 1)
                s.load_packed(R.model_pack(pp, bp))
            assert s.get_stat("precise_active") == 1 and s.get_stat("selfcheck_runs") == 1 and s.get_stat("selfcheck_overflow") == 0
            s.tilesize = 128
            got = s.process(img)
            d = np.abs(got.astype(int) - want.astype(int))
            print("45wide, precise_auto (%s): C1 max |d| vs oracle = %d, %.2f %% differ; headroom %.2f, %.2f ms" % (
                how, d.max(), 100 * (d > 0).mean(), s.get_stat("selfcheck_headroom"), s.get_stat("selfcheck_ms")))
            assert d.max() <= 1
            outs.append(got)
            if how == "option after load":  # an explicit "precise" afterwards wins
                s.set_option("precise", 0)
                assert s.get_stat("precise_active") == 0
                assert np.array_equal(s.process(img), plain_bytes)
        finally:
            s.close()
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


def test_precise_auto_leaves_the_base_model_in_fp16_storage_with_the_same_bytes():
    img = c1_image()
    pp, bp = model_paths("42")
    plain = R.RealSR(0)
    plain.load(pp, bp)
    plain.tilesize = 128
    want = plain.process(img)
    plain.close()
    s = R.RealSR(0)
    try:
        s.set_option("precise_auto", 1)
        s.load(pp, bp)
        assert s.get_stat("precise_active") == 0 and s.get_stat("selfcheck_runs") == 1
        s.tilesize = 128
        assert np.array_equal(s.process(img), want)
        s.set_option("precise_auto", 0)  # off: the mode stays where it is, nothing runs
        assert s.get_stat("precise_active") == 0 and s.get_stat("selfcheck_runs") == 1
    finally:
        s.close()


# ---- 8. the check leaves no trace ------------------------------------------------------------------------------------------------
def test_selfcheck_leaves_no_trace():
    img = c1_image()
    imgs = [img, synth.make_image(77, 90, 70)]
    fresh = open_model("42")
    fresh.tilesize = 128
    want = [fresh.process(i) for i in imgs]
    fresh.set_option("precise", 1)
    wantp = [fresh.process(i) for i in imgs]
    fresh.close()
    s = open_model("42")
    try:
        s.tilesize = 128
        reps = []
        for mode, ref in ((0, want), (1, wantp)):
            s.set_option("precise", mode)
            assert all(np.array_equal(s.process(i), r) for i, r in zip(imgs, ref))
            plans = s.get_stat("plans")
            reps.append(s.selfcheck())
            assert s.get_stat("plans") == plans and s.get_stat("precise_active") == mode
            assert all(np.array_equal(s.process(i), r) for i, r in zip(imgs, ref))
            reps.append(s.selfcheck(tiles()["photo"]))  # another tile, again between two calls
            assert all(np.array_equal(s.process(i), r) for i, r in zip(imgs, ref))
            assert s.get_stat("plans") == plans and s.get_stat("precise_active") == mode
            # a tile of the check's own size right behind it (same slot capacity, the other storage's layout before)
            t = tiles()["photo"]
            x = s.net_forward(t)
            s.selfcheck()
            assert np.array_equal(s.net_forward(t).view(np.uint16), x.view(np.uint16))
        # the report does not depend on the mode the context is in
        for k in ("storage_err", "max_byte_diff", "bytes_differ", "peak_abs", "peak_conv", "nonfinite"):
            assert reps[0][k] == reps[2][k] and reps[1][k] == reps[3][k], k
    finally:
        s.close()


# ---- 9. the range probe against an fp32 walk ---------------------------------------------------------------------------------------
def stored_peaks_fp32(key, tile):
    """max |v| of what every convolution of x4.param STORES, from an fp32 walk of the canonical graph (the shape of
    tools/check_real_model.py activation_ranges, per convolution): conv_first; x1..x4 after LeakyReLU; conv5 stores 0.2 * x5 + x, every
    third one 0.2 * (0.2 * x5 + x) + rrdb_in; trunk_conv stores fea + conv; the up convs after LeakyReLU; conv_last as it is."""
    import torch
    import torch.nn.functional as F
    net = oracle.OracleNet(*model_paths(key))
    it = iter([(c["weight"], c["bias"]) for c in (net.conv(i) for i in range(net.num_convs))])
    peaks = []

    def conv(t, act):
        W, b = next(it)
        y = F.conv2d(t, torch.from_numpy(np.ascontiguousarray(W)), torch.from_numpy(np.ascontiguousarray(b)), padding=1)
        return F.leaky_relu(y, 0.2) if act else y

    def st(t):
        peaks.append(float(t.abs().max()))
        return t

    with torch.no_grad():
        x = torch.from_numpy(tile.astype(np.float32))[None]
        fea = st(conv(x, False))
        cur = fea
        for _ in range(23):
            rin = cur
            for j in range(3):
                xx = cur
                x1 = st(conv(xx, True))
                x2 = st(conv(torch.cat((xx, x1), 1), True))
                x3 = st(conv(torch.cat((xx, x1, x2), 1), True))
                x4 = st(conv(torch.cat((xx, x1, x2, x3), 1), True))
                v = conv(torch.cat((xx, x1, x2, x3, x4), 1), False) * 0.2 + xx
                if j == 2:
                    v = v * 0.2 + rin
                cur = st(v)
        t = st(conv(cur, False) + fea)
        t = st(conv(F.interpolate(t, scale_factor=2, mode="nearest"), True))
        t = st(conv(F.interpolate(t, scale_factor=2, mode="nearest"), True))
        t = st(conv(t, True))
        st(conv(t, False))
    assert len(peaks) == R.NUM_CONVS
    return np.array(peaks)


# Worst relative deviation of a convolution's device peak (fp16 storage) from the fp32 walk's, measured on MI355X on the built-in tile
# (profiles/selfcheck.txt): 1.403e-3 on model 42 (conv 340), 1.345e-3 on 44hot (conv 307).  The bound is twice the measured worst and never
# above 5 %: the probe has to tell 6e3 from 65,504, and a probe that read the wrong planes would be off by far more than a per cent.
PEAK_DEVIATION_BOUND = min(2 * 1.403e-3, 0.05)


def test_range_probe_against_an_fp32_walk():
    tile = tiles()["builtin"]
    dev = {}
    for key in ("44hot", "42"):
        s = open_model(key)
        try:
            rep = s.selfcheck()
            peak, bad = s.selfcheck_ranges()
        finally:
            s.close()
        ref = stored_peaks_fp32(key, tile)
        rel = np.abs(peak - ref) / ref
        worst = int(rel.argmax())
        print("model %s: range probe vs fp32 walk, worst relative deviation %.3e at conv %d (device %.6g, fp32 %.6g); peak_abs %.6g at conv %d; conv 0 %.5g; conv_last %.5g" % (
            key, rel.max(), worst, peak[worst], ref[worst], rep["peak_abs"], rep["peak_conv"], peak[0], peak[-1]))
        assert bad.sum() == 0 and rep["nonfinite"] == 0 and rep["fp16_overflow"] == 0
        assert peak[rep["peak_conv"]] == np.float32(rep["peak_abs"]) == peak.max()
        assert abs(ref[rep["peak_conv"]] / ref.max() - 1) <= PEAK_DEVIATION_BOUND  # ... and it is (all but) the fp32 walk's largest too
        assert rel.max() <= PEAK_DEVIATION_BOUND
        dev[key] = peak
    print("conv 0 peaks: 44hot %.5g, 42 %.5g (x%.1f)" % (dev["44hot"][0], dev["42"][0], dev["44hot"][0] / dev["42"][0]))
    assert dev["44hot"][0] >= 20 * dev["42"][0]  # conv_first is 32 x larger by construction


# ---- 10. overflow is seen -----------------------------------------------------------------------------------------------------------
def test_overflow_is_reported_not_raised():
    """hot = 512 (the model tools/check_real_model.py refuses): the trunk passes 65,504.  The load succeeds, the self-check returns RSR_OK
    with fp16_overflow set, and a context holding model 42 on the same device gives its usual bytes afterwards.  (inf / NaN arithmetic in
    ordinary kernels; run once.)"""
    img = synth.make_image(7, 50, 43)
    base = open_model("42")
    try:
        base.tilesize = 32
        want = base.process(img)
        d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K_sc_44hot512", 44, hot=512.0, last_gain=0.15)
        s = R.RealSR(0)
        try:
            s.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
            r = R.SelfcheckReport()
            assert s._L.rsr_selfcheck(s._h, None, 0, 0, C.byref(r)) == R.RSR_OK
            peak, bad = s.selfcheck_ranges()
            print("hot = 512: peak_abs %.6g at conv %d, %d non-finite values in %d convolutions, storage_err %g, recommend_precise %d" % (
                r.peak_abs, r.peak_conv, r.nonfinite, int((bad > 0).sum()), r.storage_err, r.recommend_precise))
            assert r.fp16_overflow == 1 and (r.nonfinite > 0 or r.peak_abs >= 65504)
            assert r.nonfinite == bad.sum() and s.get_stat("selfcheck_overflow") == 1
        finally:
            s.close()
        assert np.array_equal(base.process(img), want)
    finally:
        base.close()


def test_cli_warns_about_overflow_without_verbose(tmp_path):
    """RSR_PRECISE_AUTO=1 without -v: silent on a healthy model (test_cli_precise_auto), ONE warning line per GPU when the activations
    overflow fp16; the run itself is not refused (the decision is the caller's)."""
    from cli_support import write_png
    d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K_sc_44hot512", 44, hot=512.0, last_gain=0.15)
    write_png(tmp_path / "in.png", synth.make_image(7, 50, 43))
    env = {k: v for k, v in os.environ.items() if k not in ("RSR_PRECISE", "RSR_PRECISE_AUTO")}
    r = subprocess.run([CLI, "-i", str(tmp_path / "in.png"), "-o", str(tmp_path / "out.png"), "-m", d, "-t", "32"], capture_output=True, text=True,
                       env=dict(env, RSR_PRECISE_AUTO="1"))
    warn = [ln for ln in r.stderr.splitlines() if "warning" in ln]
    print("\n".join(warn))
    assert r.returncode == 0 and len(warn) == 1 and "overflow fp16" in warn[0] and "non-finite" in warn[0], r.stderr[-2000:]
    assert os.path.exists(tmp_path / "out.png")


# ---- 11. two contexts agree ---------------------------------------------------------------------------------------------------------
def test_two_contexts_and_a_group_member_agree(monkeypatch):
    pp, bp = model_paths("45wide")
    a, b = open_model("45wide"), open_model("45wide")
    monkeypatch.setenv("RSR_GROUP_FORCE_RCCL", "1")
    srs, transport = R.create_group([0], pp, bp)
    try:
        ra, rb = a.selfcheck(), b.selfcheck()
        for k in ra:
            if k != "elapsed_ms":
                assert ra[k] == rb[k], k
        assert np.float32(ra["storage_err"]).view(np.uint32) == np.float32(rb["storage_err"]).view(np.uint32)
        assert transport == "rccl", transport
        g = srs[0]  # comes back loaded: the option decides at once, per member
        g.set_option("precise_auto", 1)
        a.set_option("precise_auto", 1)
        assert g.get_stat("precise_active") == a.get_stat("precise_active") == ra["recommend_precise"] == 1
        assert g.get_stat("selfcheck_headroom") == a.get_stat("selfcheck_headroom") == ra["headroom"]
    finally:
        for s in (a, b, srs[0]):
            s.close()


# ---- 12. CLI -------------------------------------------------------------------------------------------------------------------------
def test_cli_precise_auto(tmp_path):
    from cli_support import read_png, write_png
    img, want = c1_image(), oracle_c1("45wide")
    mdir = os.path.dirname(model_paths("45wide")[0])
    write_png(tmp_path / "in.png", img)
    env = {k: v for k, v in os.environ.items() if k not in ("RSR_PRECISE", "RSR_PRECISE_AUTO")}
    r = subprocess.run([CLI, "-i", str(tmp_path / "in.png"), "-o", str(tmp_path / "auto.png"), "-m", mdir, "-t", "128", "-v"], capture_output=True, text=True,
                       env=dict(env, RSR_PRECISE_AUTO="1"))
    lines = [ln for ln in r.stderr.splitlines() if "self-check" in ln]
    print("\n".join(lines))
    assert r.returncode == 0 and len(lines) == 1, r.stderr[-2000:]
    assert "148x148" in lines[0] and "storage_err" in lines[0] and "headroom" in lines[0] and "non-finite" in lines[0] and "precise residual trunk" in lines[0]
    d = np.abs(read_png(tmp_path / "auto.png").astype(int) - want.astype(int))
    print("CLI, RSR_PRECISE_AUTO=1: C1 on 45wide max |d| vs oracle = %d" % d.max())
    assert d.max() <= 1
    r0 = subprocess.run([CLI, "-i", str(tmp_path / "in.png"), "-o", str(tmp_path / "forced.png"), "-m", mdir, "-t", "128", "-v"], capture_output=True, text=True,
                        env=dict(env, RSR_PRECISE_AUTO="1", RSR_PRECISE="0"))
    lines0 = [ln for ln in r0.stderr.splitlines() if "self-check" in ln]
    assert r0.returncode == 0 and len(lines0) == 1 and "fp16 storage" in lines0[0] and "precise residual trunk" not in lines0[0], r0.stderr[-2000:]
    # without -v and without overflow: silent
    rq = subprocess.run([CLI, "-i", str(tmp_path / "in.png"), "-o", str(tmp_path / "quiet.png"), "-m", mdir, "-t", "128"], capture_output=True, text=True,
                        env=dict(env, RSR_PRECISE_AUTO="1"))
    assert rq.returncode == 0 and "self-check" not in rq.stderr and "warning" not in rq.stderr, rq.stderr[-2000:]
    assert np.array_equal(read_png(tmp_path / "quiet.png"), read_png(tmp_path / "auto.png"))
