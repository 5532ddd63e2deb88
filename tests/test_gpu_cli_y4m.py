"""The CLI's video mode on the GPU (run with -m gpu): `realsr-hip -i in.y4m -o out.y4m` runs a YUV4MPEG2 stream through one rsr_video
session.  Streams are written and parsed by numpy here; 40 x 30 frames at -t 32 (2 x 1 tiles), 5 frames with repeats.  Every frame the
CLI writes equals, byte for byte, what the library's session (R.Video) makes of the same planes with the options the C tag and the X
tags map to.  Few process launches, several checks per run."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import realsr_ncnn_vulkan_amd as R

import pixfmt_ref as F
import planes_ref as P
from gpu_support import context_fixtures, paths  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "realsr-ncnn-vulkan_amd", "bin", "realsr-hip")
W, H, T = 40, 30, 32
ctxs, ctx = context_fixtures(T, 10)
FMT = {"420jpeg": F.NV12, "420mpeg2": F.NV12, "420p10": F.P010, "444": F.YUV444P, "mono": F.NV12, "420p12": F.P010}


def frames_of(fmt, seed):
    a, b = P.frame(seed, fmt, W, H), P.frame(seed + 1, fmt, W, H)
    c = tuple(p.copy() for p in b)
    c[0][3, 3] ^= 1
    return [a, a, b, c, c]  # repeats: windows with tiles to skip


def write_stream(tag, frames, tags=b" F25:1 Ip A1:1", xtags=b""):
    head = b"YUV4MPEG2 W%d H%d" % (W, H) + tags + b" C" + tag.encode() + xtags + b"\n"
    return head + b"".join(b"FRAME\n" + b"".join(p.astype(p.dtype.newbyteorder("<")).tobytes() for p in f) for f in frames)


def parse_stream(data, fmt):
    head, body = data.split(b"\n", 1)
    tok = head.split(b" ")
    assert tok[0] == b"YUV4MPEG2"
    w, h = int([t for t in tok if t[:1] == b"W"][0][1:]), int([t for t in tok if t[:1] == b"H"][0][1:])
    shapes, dt = P.plane_shapes(fmt, w, h), np.dtype(F.NP[fmt]).newbyteorder("<")
    frames, pos = [], 0
    while pos < len(body):
        assert body[pos:pos + 6] == b"FRAME\n"
        pos += 6
        planes = []
        for s in shapes:
            n = int(np.prod(s)) * dt.itemsize
            planes.append(np.frombuffer(body[pos:pos + n], dtype=dt).astype(F.NP[fmt]).reshape(s))
            pos += n
        frames.append(tuple(planes))
    assert pos == len(body)
    return head, (w, h), frames


def cli(model_dir, args, env=None, data=None):
    e = dict(os.environ)
    for k in ("RSR_OUT_SCALE", "RSR_YUV_MATRIX", "RSR_YUV_RANGE", "RSR_YUV_SITING", "RSR_VIDEO_WINDOW", "RSR_PRECISE", "RSR_PRECISE_AUTO"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([CLI, "-m", model_dir, "-t", str(T)] + args, input=data, capture_output=True, env=e, timeout=120)


def library(s, fmt, frames, siting=0, range_=0):
    s.set_option("yuv_siting", siting)
    s.set_option("yuv_range", range_)
    v = R.Video(s, fmt, W, H, window=2)
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
    return len(a) == len(b) and all(np.array_equal(p, q) and p.dtype == q.dtype for x, y in zip(a, b) for p, q in zip(x, y))


def test_files_sitings_and_the_verbose_lines(ctx, model_dir, tmp_path):
    s = ctx[False]
    for tag, siting in (("420jpeg", 0), ("420mpeg2", 1)):
        frames = frames_of(FMT[tag], 3)
        (tmp_path / "in.y4m").write_bytes(write_stream(tag, frames))
        r = cli(model_dir, ["-i", str(tmp_path / "in.y4m"), "-o", str(tmp_path / "out.y4m"), "-v"], env={"RSR_VIDEO_WINDOW": "2"})
        assert r.returncode == 0, r.stderr[-800:]
        head, size, got = parse_stream((tmp_path / "out.y4m").read_bytes(), FMT[tag])
        assert head == b"YUV4MPEG2 W160 H120 F25:1 Ip A1:1 C" + tag.encode() and size == (160, 120)
        assert same(got, library(s, FMT[tag], frames, siting)), tag
        err = r.stderr.decode()
        windows = [ln for ln in err.splitlines() if ln.startswith("window:")]
        assert len(windows) == 3 and "%" not in err  # one line per window, no per-tile percent lines
        assert windows[0] == "window: 2 frames, 2 tiles run, 2 skipped" and windows[2].startswith("window: 1 frames, 0 tiles run")
    assert not same(got, library(s, F.NV12, frames, 0))  # (the siting shows in the bytes)


def test_stdin_to_stdout_ten_bits_and_out_scale_2(ctx, model_dir):
    s = ctx[False]
    frames = frames_of(F.P010, 5)
    r = cli(model_dir, ["-i", "-", "-o", "-"], env={"RSR_OUT_SCALE": "2"}, data=write_stream("420p10", frames, tags=b" F30000:1001 Ip A10:11", xtags=b" XFOO=bar"))
    assert r.returncode == 0, r.stderr[-800:]
    head, size, got = parse_stream(r.stdout, F.P010)
    assert head == b"YUV4MPEG2 W80 H60 F30000:1001 Ip A10:11 C420p10 XFOO=bar"
    s.out_scale = 2
    assert same(got, library(s, F.P010, frames, 1))
    assert max(int(p.max()) for f in got for p in f) < 1024  # codes in the low bits, as they came


def test_444_full_range_and_a_ratio_per_axis(ctx, model_dir, tmp_path):
    s = ctx[False]
    frames = frames_of(F.YUV444P, 7)
    (tmp_path / "in.y4m").write_bytes(write_stream("444", frames, tags=b" F25:1 Ip A4:3", xtags=b" XCOLORRANGE=FULL XYSCSS=444"))
    r = cli(model_dir, ["-i", str(tmp_path / "in.y4m"), "-o", str(tmp_path / "out.y4m")], env={"RSR_OUT_SCALE": "2,4"})
    assert r.returncode == 0, r.stderr[-800:]
    head, size, got = parse_stream((tmp_path / "out.y4m").read_bytes(), F.YUV444P)
    assert head == b"YUV4MPEG2 W80 H120 F25:1 Ip A8:3 C444 XCOLORRANGE=FULL XYSCSS=444"  # 4 * 4 * 1 : 3 * 2 * 1
    s.out_ratio_xy = (Fraction(2), Fraction(4))
    want = library(s, F.YUV444P, frames, 0, 1)
    assert same(got, want)
    s.out_ratio_xy = (Fraction(2), Fraction(4))
    assert not same(got, library(s, F.YUV444P, frames, 0, 0))  # (XCOLORRANGE shows in the bytes)
    # RSR_YUV_RANGE overrides the header
    r = cli(model_dir, ["-i", str(tmp_path / "in.y4m"), "-o", str(tmp_path / "out2.y4m")], env={"RSR_OUT_SCALE": "2,4", "RSR_YUV_RANGE": "0"})
    s.out_ratio_xy = (Fraction(2), Fraction(4))
    assert r.returncode == 0 and same(parse_stream((tmp_path / "out2.y4m").read_bytes(), F.YUV444P)[2], library(s, F.YUV444P, frames, 0, 0))


def test_refusals_and_a_stream_cut_inside_frame_4(ctx, model_dir, tmp_path):
    frames = frames_of(F.NV12, 9)
    good = write_stream("420jpeg", frames)
    for data, word in ((write_stream("420jpeg", frames, tags=b" F25:1 It"), "'It'"), (write_stream("mono", frames), "'Cmono'"), (write_stream("420p12", frames), "'C420p12'")):
        (tmp_path / "bad.y4m").write_bytes(data)
        r = cli(model_dir, ["-i", str(tmp_path / "bad.y4m"), "-o", str(tmp_path / "bad_out.y4m")])
        assert r.returncode != 0 and word in r.stderr.decode(), word
        assert not (tmp_path / "bad_out.y4m").exists() or (tmp_path / "bad_out.y4m").read_bytes() == b""
    (tmp_path / "in.y4m").write_bytes(good)
    r = cli(model_dir, ["-i", str(tmp_path / "in.y4m"), "-o", str(tmp_path / "out.png")])
    assert r.returncode != 0 and ".y4m" in r.stderr.decode() and not (tmp_path / "out.png").exists()
    per = (len(good) - good.index(b"\n") - 1) // 5
    (tmp_path / "cut.y4m").write_bytes(good[:good.index(b"\n") + 1 + 3 * per + per // 2])
    r = cli(model_dir, ["-i", str(tmp_path / "cut.y4m"), "-o", str(tmp_path / "cut_out.y4m")])
    assert r.returncode != 0 and "inside a frame" in r.stderr.decode()
    head, size, got = parse_stream((tmp_path / "cut_out.y4m").read_bytes(), F.NV12)
    assert len(got) == 3 and same(got, library(ctx[False], F.NV12, frames[:3], 0))
