"""RSR_ALPHA of the command line tool on the GPU (run with -m gpu): net = the alpha of an RGBA image through the network (engine option
"alpha_net"), except for a fully opaque image, which keeps the bicubic alpha and its one pass."""
import os
import subprocess

import numpy as np
import pytest

import realsr_ncnn_vulkan_amd as R
from cli_support import CLI, read_png, write_png

pytestmark = pytest.mark.gpu
T = 32


def cli(tmp_path, name, model_dir, alpha=None, verbose=False):
    env = {k: v for k, v in os.environ.items() if k != "RSR_ALPHA"}
    if alpha is not None:
        env["RSR_ALPHA"] = alpha
    out = tmp_path / ("out_%s_%s.png" % (name, alpha))
    r = subprocess.run([CLI, "-i", str(tmp_path / (name + ".png")), "-o", str(out), "-m", model_dir, "-t", str(T)] + (["-v"] if verbose else []),
                       capture_output=True, text=True, env=env, timeout=240)
    return r, out


@pytest.fixture(scope="module")
def images():
    rng = np.random.default_rng(5)
    cut = rng.integers(0, 256, size=(37, 45, 4), dtype=np.uint8)
    cut[:, :, 3] = (np.arange(45) * 255 // 44)[None, :]
    cut[10:20, 5:30, 3] = 0
    cut[20:30, 5:30, 3] = 255
    opaque = cut.copy()
    opaque[:, :, 3] = 255
    return {"cut": cut, "opaque": opaque}


def test_rgba_png_under_net_equals_the_library(tmp_path, model_dir, images):
    write_png(tmp_path / "cut.png", images["cut"])
    r, out = cli(tmp_path, "cut", model_dir, "net", verbose=True)
    assert r.returncode == 0, r.stderr
    assert "alpha through the network" in r.stderr
    got = read_png(out)
    s = R.RealSR(0)
    try:
        s.load(os.path.join(model_dir, "x4.param"), os.path.join(model_dir, "x4.bin"))
        s.tilesize = T
        bicubic = s.process(images["cut"])
        s.alpha_net = 1
        want = s.process(images["cut"])
    finally:
        s.close()
    assert got.shape == want.shape == (148, 180, 4)
    assert np.array_equal(got, want) and not np.array_equal(want[:, :, 3], bicubic[:, :, 3])
    r0, out0 = cli(tmp_path, "cut", model_dir, "bicubic")
    assert r0.returncode == 0 and np.array_equal(read_png(out0), bicubic)


def test_opaque_rgba_png_keeps_its_alpha_and_one_pass(tmp_path, model_dir, images):
    write_png(tmp_path / "opaque.png", images["opaque"])
    r, out = cli(tmp_path, "opaque", model_dir, "net", verbose=True)
    assert r.returncode == 0, r.stderr
    assert "fully opaque" in r.stderr
    r0, out0 = cli(tmp_path, "opaque", model_dir, None)
    assert r0.returncode == 0, r0.stderr
    got, plain = read_png(out), read_png(out0)
    assert got.shape == (148, 180, 4) and np.array_equal(got, plain) and (got[:, :, 3] == 255).all()


def test_bad_value_is_refused_before_any_gpu_work(tmp_path, model_dir, images):
    write_png(tmp_path / "cut.png", images["cut"])
    r, out = cli(tmp_path, "cut", model_dir, "foo", verbose=True)
    assert r.returncode != 0 and "RSR_ALPHA" in r.stderr and not out.exists()
    assert "model:" not in r.stderr and "%" not in r.stderr   # no context was created, no tile ran
