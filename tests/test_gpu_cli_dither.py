"""RSR_DITHER of the command line tool on the GPU (run with -m gpu): engine option "dither" 1 for the whole run, on the image route and
on the Y4M route; a value other than 0 / 1 is refused before any GPU work.  Few process launches."""
import os
import subprocess

import numpy as np
import pytest

import realsr_ncnn_vulkan_amd as R

import dither_ref as D
import pixfmt_ref as F
import planes_ref as P
from cli_support import CLI, read_png, write_png

pytestmark = pytest.mark.gpu
T, W, H = 32, 44, 37  # 2 x 2 tiles: a pattern keyed to the tile would show


def cli(model_dir, args, dither, data=None):
    env = {k: v for k, v in os.environ.items() if k not in ("RSR_DITHER", "RSR_OUT_SCALE", "RSR_DEPTH", "RSR_PRECISE", "RSR_PRECISE_AUTO", "RSR_ALPHA",
                                                            "RSR_YUV_RANGE", "RSR_YUV_SITING", "RSR_VIDEO_WINDOW")}
    if dither is not None:
        env["RSR_DITHER"] = dither
    return subprocess.run([CLI, "-m", model_dir, "-t", str(T)] + args, input=data, capture_output=True, env=env, timeout=240)


@pytest.fixture()
def sr(model_dir):
    s = R.RealSR(0)
    s.load(os.path.join(model_dir, "x4.param"), os.path.join(model_dir, "x4.bin"))
    s.tilesize = T
    yield s
    s.close()


def test_png_equals_the_library_and_the_rule(tmp_path, model_dir, sr):
    img = np.random.default_rng(8).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    write_png(tmp_path / "in.png", img)
    r = cli(model_dir, ["-i", str(tmp_path / "in.png"), "-o", str(tmp_path / "out.png"), "-v"], "1")
    assert r.returncode == 0, r.stderr[-800:]
    assert b"ordered dither of the integer outputs (RSR_DITHER)" in r.stderr
    got = read_png(tmp_path / "out.png")
    plain = sr.process(img)
    d = sr.process_fmt(img, F.U8, F.F32)
    sr.dither = 1
    want = sr.process(img)
    assert got.shape == (4 * H, 4 * W, 3) and np.array_equal(got, want) and np.array_equal(want, D.quantise_rgb(d, 255))
    assert not np.array_equal(want, plain)
    # RSR_DITHER=0 and no variable at all: the plain run
    for val in ("0", None):
        r = cli(model_dir, ["-i", str(tmp_path / "in.png"), "-o", str(tmp_path / "out0.png")], val)
        assert r.returncode == 0 and np.array_equal(read_png(tmp_path / "out0.png"), plain), val


def write_stream(frames):
    head = b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420jpeg\n" % (40, 30)
    return head + b"".join(b"FRAME\n" + b"".join(p.tobytes() for p in f) for f in frames)


def parse_stream(data, w, h):
    head, body = data.split(b"\n", 1)
    shapes = P.plane_shapes(F.NV12, w, h)
    frames, pos = [], 0
    while pos < len(body):
        assert body[pos:pos + 6] == b"FRAME\n"
        pos += 6
        planes = []
        for s in shapes:
            n = int(np.prod(s))
            planes.append(np.frombuffer(body[pos:pos + n], dtype=np.uint8).reshape(s))
            pos += n
        frames.append(tuple(planes))
    assert pos == len(body)
    return head, frames


def library(s, frames):
    v = R.Video(s, F.NV12, 40, 30, window=2)
    outs = []
    try:
        for f in frames:
            v.send(*f)
            while v.ready:
                outs.append(v.receive())
        v.flush()
        while v.ready:
            outs.append(v.receive())
    finally:
        v.close()
    return outs


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(p, q) for x, y in zip(a, b) for p, q in zip(x, y))


def test_y4m_equals_the_library(model_dir, sr):
    """Three frames, the second a repeat of the first: the session copies its tiles from the frame before, and the static pattern makes
    that the bytes a fresh computation gives."""
    a, b = P.frame(4, F.NV12, 40, 30), P.frame(5, F.NV12, 40, 30)
    frames = [a, a, b]
    r = cli(model_dir, ["-i", "-", "-o", "-"], "1", data=write_stream(frames))
    assert r.returncode == 0, r.stderr[-800:]
    head, got = parse_stream(r.stdout, 160, 120)
    assert head.startswith(b"YUV4MPEG2 W160 H120")
    plain = library(sr, frames)
    sr.dither = 1
    want = library(sr, frames)
    assert len(got) == 3 and same(got, want) and not same(want, plain)
    assert same(want[:1], want[1:2])


def test_a_bad_value_is_refused_before_gpu_work(tmp_path, model_dir):
    img = np.zeros((8, 8, 3), np.uint8)
    write_png(tmp_path / "in.png", img)
    for bad in ("2", "on", "-1", "0.5"):
        # (a model directory that does not exist: the refusal comes before the tool looks for it, let alone for a device)
        r = cli(str(tmp_path / "no_such_model"), ["-i", str(tmp_path / "in.png"), "-o", str(tmp_path / "out.png")], bad)
        assert r.returncode != 0 and b"invalid RSR_DITHER" in r.stderr and bad.encode() in r.stderr, bad
        assert not (tmp_path / "out.png").exists()
