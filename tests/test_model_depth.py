"""RRDBNet x4 models of any depth, 1 .. RSR_MAX_RRDB blocks (CPU: the loader, the packer, the synthetic models, the exact model).

The loader derives the depth from the graph's node count and holds everything else to the canonical graph of that depth; the packed
blob carries the depth as its conv count, 15 nb + 6.  Here: models of five depths load, pack and agree with the oracle's own reader;
the default depth still produces the bytes it produced before depths existed (tests/golden/depth_default.json, recorded at the commit
before this feature); graphs that are not an RRDBNet of a depth in range are refused with RSR_E_GRAPH and a message; a .bin of another
depth than its .param ends in a clean error; and the exact model of tests/exact_net.py, driven at other depths through
tests/depth_ref.py, equals its dense twin bit for bit and is healthy on the inputs tests/test_gpu_depth.py uses."""
import ctypes as C
import hashlib
import json
import os
import struct

import numpy as np
import pytest

import depth_ref as D
import exact_net as N
import oracle
import realsr_ncnn_vulkan_amd as R
import test_exact_net as TE   # the health conditions and the dense twin, as the default depth is held to them
from realsr_ncnn_vulkan_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_default.json")


# ---- five depths load and pack ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 2, 6, 16, 64])
def test_model_of_depth_loads_packs_and_agrees_with_the_oracle(nb, tmp_path):
    d = synth.make_model_dir(str(tmp_path), nb=nb)
    assert os.path.basename(d) == "models-DF2K-nb%d" % nb   # (never the directory the default-depth model is cached in)
    pp, bp = os.path.join(d, "x4.param"), os.path.join(d, "x4.bin")
    try:
        nconv = 15 * nb + 6
        assert len(synth.conv_specs(nb)) == nconv
        info = R.model_info(pp, bp)
        assert info["n_convs"] == nconv
        blob = R.model_pack(pp, bp)
        magic, version, hconv, flags, total = struct.unpack("<4sIIIQ", blob[:24].tobytes())
        assert (magic, version, hconv, flags, total) == (b"RSRP", 6, nconv, 0, blob.size)
        assert oracle.OracleNet(pp, bp).num_convs == nconv
    finally:
        os.remove(bp)   # (93 MB at 64 blocks)


def test_default_depth_is_byte_identical_to_the_commit_before_depths():
    """sha256 and size of synth.param_text(), the seed-42 x4.bin and its packed blob against the values recorded before the feature."""
    want = json.load(open(GOLDEN))
    root = os.environ.get("RSR_MODELS", "/tmp/rsr_models")
    d = synth.make_model_dir(root, "models-DF2K", 42)
    pp, bp = os.path.join(d, "x4.param"), os.path.join(d, "x4.bin")
    got = {"param_text": synth.param_text().encode(), "x4_bin_seed42": open(bp, "rb").read(), "packed_blob_seed42": R.model_pack(pp, bp).tobytes()}
    assert open(pp, "rb").read() == got["param_text"]
    for k, b in got.items():
        assert {"sha256": hashlib.sha256(b).hexdigest(), "size": len(b)} == want[k], k
    assert synth.param_text(23) == synth.param_text() and len(synth.conv_specs()) == R.NUM_CONVS == 351


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def gen_param(nb, rdbs=lambda i: 3, drop_rrdb_add=None, narrow=None, interps=2):
    """A local writer of the x4 graph (names of its own: the validator compares operator types and parameters, never names), with the
    defects the refusal tests need: rdbs(i) dense blocks in RRDB i, RRDB drop_rrdb_add without its Eltwise, conv number `narrow` with 48
    instead of 64 output channels, `interps` up-sampling stages.  Splits are inserted from the consumer counts, so a defect never leaves
    a dangling blob behind."""
    layers, n, nconv = [], [0], [0]

    def add(typ, ins, params="", out=None):
        n[0] += 1
        out = out or "b%d" % n[0]
        layers.append((typ, "L%d" % n[0], list(ins), out, params))
        return out

    def conv(src, cin, cout, lrelu, out=None):
        if narrow == nconv[0]:
            cout = 48
        nconv[0] += 1
        p = "0=%d 1=3 4=1 5=1 6=%d" % (cout, cin * cout * 9) + (" 9=2 -23310=1,2.000000e-01" if lrelu else "")
        return add("Convolution", [src], p, out)

    def axpy(a, b):
        return add("Eltwise", [a, b], "0=1 -23301=2,2.000000e-01,1.000000e+00")

    fea = cur = conv(add("Input", [], out="data"), 3, 64, False)
    for i in range(nb):
        rrdb_in = cur
        for _ in range(rdbs(i)):
            x, feats = cur, [cur]
            for k in range(4):
                feats.append(conv(x if k == 0 else add("Concat", feats), 64 + 32 * k, 32, True))
            cur = axpy(conv(add("Concat", feats), 192, 64, False), x)
        if i != drop_rrdb_add:
            cur = axpy(cur, rrdb_in)
    s = add("BinaryOp", [fea, conv(cur, 64, 64, False)])
    for _ in range(interps):
        s = conv(add("Interp", [s], "0=1 1=2.0 2=2.0"), 64, 64, True)
    conv(conv(s, 64, 64, True), 64, 3, False, out="output")

    uses = {}
    for li, (_, _, ins, _, _) in enumerate(layers):
        for k, b in enumerate(ins):
            uses.setdefault(b, []).append((li, k))
    out, rename, nblobs = [], {}, 0
    for li, (typ, name, ins, top, p) in enumerate(layers):
        out.append((typ, name, [rename.get((li, k), b) for k, b in enumerate(ins)], [top], p))
        nblobs += 1
        if len(uses.get(top, [])) > 1:
            tops = ["%s_s%d" % (top, i) for i in range(len(uses[top]))]
            rename.update(zip(uses[top], tops))
            out.append(("Split", "S" + name, [top], tops, ""))
            nblobs += len(tops)
    lines = ["7767517", "%d %d" % (len(out), nblobs)]
    lines += [" ".join([typ, name, str(len(ins)), str(len(tops))] + ins + tops + ([p] if p else [])) for typ, name, ins, tops, p in out]
    return "\n".join(lines) + "\n"


def test_the_local_generator_writes_loadable_graphs(tmp_path):
    """... so that a refusal below is the defect's, not the generator's: its sound nb = 2 graph loads with synth's weights."""
    p = tmp_path / "x4.param"
    p.write_text(gen_param(2))
    bp = tmp_path / "x4.bin"
    synth.write_bin(str(bp), synth.make_weights(3, nb=2))
    assert R.model_info(p, bp)["n_convs"] == 36


REFUSED = {
    "nb = 0": (dict(nb=0), "0 RRDB"),
    "nb = 65": (dict(nb=65), "65 RRDB"),
    "an RRDB with two RDBs": (dict(nb=2, rdbs=lambda i: 2 if i == 1 else 3), "node"),
    "an RRDB with four RDBs": (dict(nb=2, rdbs=lambda i: 4 if i == 0 else 3), "node"),
    "an RRDB-level Eltwise missing": (dict(nb=2, drop_rrdb_add=0), "node"),
    "a conv of 64 -> 48": (dict(nb=2, narrow=10), "48,3,3"),
    "a third Interp stage": (dict(nb=2, interps=3), "node"),
    "one Interp stage": (dict(nb=2, interps=1), "node"),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_graphs_that_are_no_rrdbnet_of_a_depth_in_range_are_refused(what, tmp_path):
    kw, word = REFUSED[what]
    p = tmp_path / "x4.param"
    p.write_text(gen_param(**kw))
    bp = tmp_path / "x4.bin"
    bp.write_bytes(b"\0" * 64)   # (never read: the graph is validated first)
    L = R.lib()
    rc = L.rsr_model_info(str(p).encode(), str(bp).encode(), None, None, None, None, None)
    msg = L.rsr_last_error(None).decode()
    print("%s: %d %s" % (what, rc, msg))
    assert rc == R.RSR_E_GRAPH and msg and word in msg
    need = C.c_size_t(0)
    assert L.rsr_model_pack(str(p).encode(), str(bp).encode(), None, 0, C.byref(need)) == R.RSR_E_GRAPH


def test_a_bin_of_another_depth_ends_in_a_clean_error(tmp_path):
    """The reader walks the .param's convolutions through the .bin.  A .bin of 6 blocks beside a .param of 2 is LONG: 36 convolutions
    are read and bytes remain -> RSR_E_FORMAT ("trailing bytes").  A .bin of 2 beside a .param of 6 is SHORT: the file ends inside
    convolution 36 -> RSR_E_IO ("truncated")."""
    d2, d6 = synth.make_model_dir(str(tmp_path), nb=2), synth.make_model_dir(str(tmp_path), nb=6)
    L = R.lib()
    for pdir, bdir, want, word in ((d2, d6, R.RSR_E_FORMAT, "trailing"), (d6, d2, R.RSR_E_IO, "truncated")):
        rc = L.rsr_model_info(os.path.join(pdir, "x4.param").encode(), os.path.join(bdir, "x4.bin").encode(), None, None, None, None, None)
        msg = L.rsr_last_error(None).decode()
        assert rc == want and word in msg, (rc, msg)


# ---- synthetic weights ------------------------------------------------------------------------------------------------------------
def test_trunk_gain_follows_the_depth():
    """make_weights scales trunk_conv by 1.2 ** (23 - nb): its weights at nb = 6 have 1.2 ** 17 times the RMS of the default depth's."""
    rms = {nb: float(np.sqrt(np.mean(synth.make_weights(5, nb=nb)[15 * nb + 1][0].astype(np.float64) ** 2))) for nb in (6, 23)}
    assert abs(rms[6] / rms[23] / 1.2 ** 17 - 1) < 0.05   # (64 * 64 * 9 samples each: the ratio of two RMS estimates is good to ~1 %)


# ---- the exact model at other depths ----------------------------------------------------------------------------------------------
def test_depth_restores_both_globals_also_behind_an_exception():
    assert synth.NB == N.NB == 23
    with pytest.raises(ZeroDivisionError):
        with D.depth(2):
            assert synth.NB == N.NB == 2 and len(synth.conv_specs()) == 36
            1 / 0
    assert synth.NB == N.NB == 23 and len(synth.conv_specs()) == 351


@pytest.mark.parametrize("nb", [1, 2, 6])
def test_sparse_mirror_equals_the_dense_twin_at_depth(nb):
    with D.depth(nb):
        model = D.make_model(nb)
        assert len(model) == 15 * nb + 6
        x = N.tile_f16(20, 44)
        want = TE.dense_forward(N.dense_weights(model), x)
        got = N.forward(model, x)
        assert got.shape == (3, 80, 176) and np.array_equal(TE.bits(got), TE.bits(want))
    assert synth.NB == N.NB == 23


@pytest.mark.parametrize("nb", [1, 2, 6])
def test_health_at_depth(nb):
    """The committed (seed, gains) of the depth meet the conditions the default depth's model is held to, on the frame and on the four
    net_forward tiles, and one changed input pixel changes an output region of at least 16 x 16."""
    with D.depth(nb):
        model = D.make_model(nb)
        w, h, T = N.FRAME
        x16 = N.halfs_of_u8(N.frame_u8(w, h))
        TE.check_health(model, x16, T, False, True)
        sy, sx = TE._spread(model, x16, T, T)
        print("nb = %d: one input pixel changes a %d x %d output region" % (nb, sy, sx))
        assert sy >= D.MIN_SPREAD and sx >= D.MIN_SPREAD
        for th, tw in N.TILE_SHAPES:
            TE.test_health_tiles(model, th, tw)


def test_health_of_the_two_block_model_on_every_frame_the_gpu_tests_use():
    with D.depth(2):
        model = D.make_model(2)
        w, h, T = N.FRAME
        TE.check_health(model, N.halfs_of_u8(N.frame_u8(w, h)[:, :, ::-1]), T, False, True)
        TE.check_health(model, N.halfs_of_u8(N.frame_u8(w, h, 4)), T, False, True)
        TE.check_health(model, N.frame_f16(w, h), T, False, False)
        TE.check_health(model, N.halfs_of_u8(N.tta_frame()), N.TTA_FRAME[2], True, True)
