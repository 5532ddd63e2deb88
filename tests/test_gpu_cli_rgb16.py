"""The command line tool with RSR_DEPTH on the GPU (run with -m gpu): a directory of a 16-bit RGB PNG, a 16-bit RGBA PNG and an 8-bit PNG
at -t 32 under RSR_DEPTH=auto, RSR_DEPTH=16 and without the variable, every output equal to the library's own call on the decoded samples;
and the two refusals that come before any GPU work."""
import os
import subprocess

import numpy as np
import pytest

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import synth

import rgb16_ref as Z
from cli_support import CLI, write_png
from png16_ref import read_png, write_png16

pytestmark = pytest.mark.gpu
U8, U16 = R.RSR_FMT_U8_HWC, R.RSR_FMT_U16_HWC


def cli(env, *args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True, env=dict({k: v for k, v in os.environ.items() if k != "RSR_DEPTH"}, **env))


@pytest.fixture(scope="module")
def images():
    return {"a": Z.image16(900, 40, 30), "b": Z.image16(901, 33, 21, 4), "c": synth.make_image(902, 36, 28)}


@pytest.fixture(scope="module")
def indir(tmp_path_factory, images):
    d = tmp_path_factory.mktemp("rgb16_in")
    write_png16(d / "a.png", images["a"], 0)
    write_png16(d / "b.png", images["b"], 2)
    write_png(d / "c.png", images["c"])
    return d


@pytest.fixture(scope="module")
def sr(model_dir):
    s = R.RealSR(0)
    s.load(os.path.join(model_dir, "x4.param"), os.path.join(model_dir, "x4.bin"))
    s.tilesize = 32
    yield s
    s.close()


def test_depth_auto(tmp_path, model_dir, indir, images, sr):
    r = cli({"RSR_DEPTH": "auto"}, "-i", str(indir), "-o", str(tmp_path), "-m", model_dir, "-t", "32", "-j", "2:3:2", "-v")
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["a.png", "b.png", "c.png"]
    assert "a.png: 16-bit route" in r.stderr and "b.png: 16-bit route" in r.stderr and "c.png: 8-bit route" in r.stderr
    for n in ("a", "b"):
        got, depth = read_png(tmp_path / (n + ".png"))
        assert depth == 16 and np.array_equal(got, sr.process_fmt(images[n], U16, U16)), n
    got, depth = read_png(tmp_path / "c.png")
    assert depth == 8 and np.array_equal(got, sr.process(images["c"]))
    lines = r.stderr.splitlines()  # progress lines as ever, one per tile: 2 x 1 tiles each
    assert lines.count("0.00%") == 3 and lines.count("50.00%") == 3, r.stderr


def test_depth_16_widens_an_8_bit_source(tmp_path, model_dir, indir, images, sr):
    r = cli({"RSR_DEPTH": "16", "RSR_PRECISE": "1"}, "-i", str(indir), "-o", str(tmp_path), "-m", model_dir, "-t", "32", "-v")
    assert r.returncode == 0, r.stderr
    assert "c.png: 16-bit route (8-bit source widened by x257)" in r.stderr
    sr.set_option("precise", 1)
    try:
        got, depth = read_png(tmp_path / "c.png")
        assert depth == 16 and np.array_equal(got, sr.process_fmt(Z.widen(images["c"]), U16, U16))
        got, depth = read_png(tmp_path / "a.png")
        assert depth == 16 and np.array_equal(got, sr.process_fmt(images["a"], U16, U16))
    finally:
        sr.set_option("precise", 0)


def test_depth_unset_is_the_8_bit_route(tmp_path, model_dir, indir, images, sr):
    for env in ({}, {"RSR_DEPTH": "8"}):
        out = tmp_path / ("o%d" % len(env))
        out.mkdir()
        r = cli(env, "-i", str(indir), "-o", str(out), "-m", model_dir, "-t", "32")
        assert r.returncode == 0, r.stderr
        for n in ("a", "b"):  # a 16-bit source is reduced to its high bytes, as ever
            got, depth = read_png(out / (n + ".png"))
            assert depth == 8 and np.array_equal(got, sr.process((images[n] >> 8).astype(np.uint8))), n
        got, depth = read_png(out / "c.png")
        assert depth == 8 and np.array_equal(got, sr.process(images["c"]))


def test_refusals_before_any_gpu_work(tmp_path, model_dir, indir):
    """A jpg output under RSR_DEPTH=16 and an unknown RSR_DEPTH end the tool before a model is looked for: the model path given does not
    exist, and no word about it is said."""
    nowhere = str(tmp_path / "models-DF2K-nowhere")
    one = str(indir / "a.png")
    r = cli({"RSR_DEPTH": "16"}, "-i", one, "-o", str(tmp_path / "x.jpg"), "-m", nowhere)
    assert r.returncode != 0 and "RSR_DEPTH=16" in r.stderr and ".png" in r.stderr and "model" not in r.stderr
    r = cli({"RSR_DEPTH": "16"}, "-i", str(indir), "-o", str(tmp_path), "-m", nowhere, "-f", "webp")
    assert r.returncode != 0 and "RSR_DEPTH=16" in r.stderr and ".png" in r.stderr and "model" not in r.stderr
    r = cli({"RSR_DEPTH": "12"}, "-i", one, "-o", str(tmp_path / "x.png"), "-m", nowhere)
    assert r.returncode != 0 and "invalid RSR_DEPTH '12'" in r.stderr and "model" not in r.stderr
    assert not os.path.exists(tmp_path / "x.jpg") and not os.path.exists(tmp_path / "x.png")
    assert cli({}, "-h").stderr.count("RSR_DEPTH") >= 1
