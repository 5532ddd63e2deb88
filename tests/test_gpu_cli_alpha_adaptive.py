"""RSR_ALPHA=adaptive of the command line tool on the GPU (run with -m gpu): engine options "alpha_net" 1 and "alpha_adaptive" 1 for the
whole run -- the alpha pass on the tiles whose alpha varies, the bicubic alpha on the others; a fully opaque image keeps its alpha."""
import os
import subprocess

import numpy as np
import pytest

import alpha_flat_ref as AF
import realsr_ncnn_vulkan_amd as R
from cli_support import CLI, read_png, write_png

pytestmark = pytest.mark.gpu
T, P, W, H = 32, 10, 100, 70


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
    """cut: opaque left of x = 45, transparent from there on -- of the 4 x 3 tiles only the second column sees both values."""
    rng = np.random.default_rng(6)
    cut = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    cut[:, :45, 3] = 255
    cut[:, 45:, 3] = 0
    opaque = cut.copy()
    opaque[:, :, 3] = 255
    return {"cut": cut, "opaque": opaque}


def test_cutout_png_equals_the_library(tmp_path, model_dir, images):
    img = images["cut"]
    flags = AF.varies(img, T, P)
    assert flags.size == 12 and int(flags.sum()) == 3
    write_png(tmp_path / "cut.png", img)
    r, out = cli(tmp_path, "cut", model_dir, "adaptive", verbose=True)
    assert r.returncode == 0, r.stderr
    assert "3 of 12 tiles ran the alpha pass" in r.stderr
    got = read_png(out)
    s = R.RealSR(0)
    try:
        s.load(os.path.join(model_dir, "x4.param"), os.path.join(model_dir, "x4.bin"))
        s.tilesize = T
        bicubic = s.process(img)
        s.alpha_net = 1
        net = s.process(img)
        s.alpha_adaptive = 1
        want = s.process(img)
        assert s.get_stat("alpha_tiles") == 12 + 3 and s.get_stat("alpha_tiles_flat") == 9
    finally:
        s.close()
    assert got.shape == want.shape == (4 * H, 4 * W, 4)
    assert np.array_equal(got, want) and np.array_equal(want, AF.select(flags, bicubic, net, W, H, T))
    assert not np.array_equal(want, net) and not np.array_equal(want, bicubic)


def test_opaque_png_equals_the_plain_run(tmp_path, model_dir, images):
    write_png(tmp_path / "opaque.png", images["opaque"])
    r, out = cli(tmp_path, "opaque", model_dir, "adaptive", verbose=True)
    assert r.returncode == 0, r.stderr
    assert "0 of 12 tiles ran the alpha pass" in r.stderr
    r0, out0 = cli(tmp_path, "opaque", model_dir, None)
    assert r0.returncode == 0, r0.stderr
    got, plain = read_png(out), read_png(out0)
    assert got.shape == (4 * H, 4 * W, 4) and np.array_equal(got, plain) and (got[:, :, 3] == 255).all()
