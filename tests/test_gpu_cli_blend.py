"""RSR_BLEND of the command line tool on the GPU (run with -m gpu): -m <dir A> with RSR_BLEND=<dir B>:<t> runs on the weights
(1 - t) * A + t * B, exactly the library's rsr_load_second + rsr_set_blend; unset, the tool is what it was; a value that cannot be meant,
a directory that holds no model or a model of another depth is refused before any GPU work."""
import os
import subprocess

import numpy as np
import pytest

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import synth
from cli_support import CLI, read_png, write_png

pytestmark = pytest.mark.gpu
T = 32
W, H = 20, 12


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    """The 2-block synthetic models of seeds 42 and 43, and a 1-block one: (A, B, shallow)."""
    tmp = str(tmp_path_factory.mktemp("cli_blend_models"))
    return (synth.make_model_dir(tmp, "models-DF2K-s42", 42, nb=2), synth.make_model_dir(tmp, "models-DF2K-s43", 43, nb=2),
            synth.make_model_dir(tmp, "models-DF2K-s43", 43, nb=1))


@pytest.fixture(scope="module")
def image():
    return synth.make_image(21, W, H)


def cli(tmp_path, model_dir, blend=None, verbose=True, tag="x"):
    env = {k: v for k, v in os.environ.items() if k != "RSR_BLEND"}
    if blend is not None:
        env["RSR_BLEND"] = blend
    out = tmp_path / ("out_%s.png" % tag)
    r = subprocess.run([CLI, "-i", str(tmp_path / "in.png"), "-o", str(out), "-m", model_dir, "-t", str(T)] + (["-v"] if verbose else []),
                       capture_output=True, text=True, env=env, timeout=240)
    return r, out


def paths(d):
    return os.path.join(d, "x4.param"), os.path.join(d, "x4.bin")


def test_blend_equals_the_library_and_unset_is_the_plain_tool(tmp_path, dirs, image):
    a, b, _ = dirs
    write_png(tmp_path / "in.png", image)
    r, out = cli(tmp_path, a, b + ":0.3", tag="blend")
    assert r.returncode == 0, r.stderr
    assert "blend 0.3 of %s (2 blocks)" % b in r.stderr
    r0, out0 = cli(tmp_path, a, None, tag="plain")
    assert r0.returncode == 0, r0.stderr
    assert "blocks)" not in r0.stderr and "RSR_BLEND" not in r0.stderr   # (no blend line)
    s = R.RealSR(0)
    try:
        s.load(*paths(a))
        s.tilesize = T
        plain = s.process(image)
        s.load_second(*paths(b))
        s.blend = float(np.float32(0.3))
        want = s.process(image)
    finally:
        s.close()
    assert want.shape == (4 * H, 4 * W, 3) and not np.array_equal(want, plain) and len(np.unique(want)) > 16
    assert np.array_equal(read_png(out), want)
    assert np.array_equal(read_png(out0), plain)


@pytest.mark.parametrize("value", ["0.3", ":0.3", "DIR", "DIR:", "DIR:abc", "DIR:1.5", "DIR:-0.1", "DIR:nan", "DIR:1e-1", "DIR: 0.3", "DIR:0.3x", "DIR:0..3", "DIR:."])
def test_malformed_values_are_refused_before_any_gpu_work(tmp_path, dirs, image, value):
    a, b, _ = dirs
    write_png(tmp_path / "in.png", image)
    r, out = cli(tmp_path, a, value.replace("DIR", b))
    assert r.returncode != 0 and "RSR_BLEND" in r.stderr and not out.exists()
    assert "gpu 0:" not in r.stderr and "%" not in r.stderr   # no context was created, no tile ran


def test_a_missing_directory_and_another_depth_are_refused_before_any_gpu_work(tmp_path, dirs, image):
    a, b, shallow = dirs
    write_png(tmp_path / "in.png", image)
    for value, word in ((str(tmp_path / "models-nowhere") + ":0.3", "no such directory"), (str(tmp_path) + ":0.3", "x4.param"), (shallow + ":0.3", "depth")):
        r, out = cli(tmp_path, a, value)
        assert r.returncode != 0 and "RSR_BLEND" in r.stderr and word in r.stderr and not out.exists(), (value, r.stderr)
        assert "gpu 0:" not in r.stderr and "%" not in r.stderr
