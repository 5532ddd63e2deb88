"""csrc/y4m_io.h, the YUV4MPEG2 reader and writer of the CLI's video mode, under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU:
a stand-alone g++ harness (its own main, nothing preloaded; the pattern of tests/test_loader_sanitized.py) parses a stream and re-emits
it at ratio 1.  Every C tag the CLI takes comes back bit for bit; the tags it refuses are refused by name; then 240 seeded MUTATED
streams -- truncations, flipped bytes, wild W / H / F, a missing newline, an overlong header, a broken FRAME magic -- must each end in a
clean code within a timeout: a sanitizer report, a crash or a hang fails the test, and at least half of them must be refused."""
import os
import subprocess

import numpy as np
import pytest

import pixfmt_ref as F
import planes_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realsr-ncnn-vulkan_amd", "csrc")

HARNESS = r'''
#include <cstdio>
#include <string>
#include <vector>
#include "y4m_io.h"
// usage: harness <in.y4m> <out.y4m>     prints "ok <frames> <fmt> <siting> <range>" or "refused <frames written> <message>"; exit code 0 either way
int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* fi = std::fopen(argv[1], "rb");
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    y4m::Header hd;
    std::string line, err;
    const int lrc = y4m::read_line(fi, line);
    err = lrc == 0 ? y4m::parse_header(line, hd) : std::string(lrc == 1 ? "empty input" : "header line without a newline within 256 bytes");
    long long frames = 0;
    if (err.empty())
    {
        const std::string head = y4m::format_header(hd, hd.w, hd.h, 1, 1, 1, 1);
        std::fwrite(head.data(), 1, head.size(), fo);
        std::vector<unsigned char> buf;
        for (;;)
        {
            std::string params;
            const int rc = y4m::read_frame(fi, hd, buf, params, err);
            if (rc <= 0) break;
            if (!y4m::write_frame(fo, params, buf.data(), buf.size())) return 2;
            frames++;
        }
    }
    std::fclose(fi);
    std::fclose(fo);
    if (err.empty()) std::printf("ok %lld %d %d %d\n", frames, hd.fmt, hd.siting, hd.range);
    else std::printf("refused %lld %s\n", frames, err.c_str());
    if (argc > 3)
    { // the output header at another pair of ratios: harness in out nx dx ny dy
        const int nx = std::atoi(argv[3]), dx = std::atoi(argv[4]), ny = std::atoi(argv[5]), dy = std::atoi(argv[6]);
        std::printf("%s", y4m::format_header(hd, hd.w * nx / dx, hd.h * ny / dy, nx, dx, ny, dy).c_str());
    }
    return 0;
}
'''

# C tag -> (format, yuv_siting), as the CLI maps them; None: no tag at all
TAGS = {None: (F.NV12, 0), "420": (F.NV12, 0), "420jpeg": (F.NV12, 0), "420mpeg2": (F.NV12, 1), "420paldv": (F.NV12, 2), "420p10": (F.P010, 1),
        "422": (F.NV16, 1), "422p10": (F.P210, 1), "444": (F.YUV444P, -1), "444p10": (F.YUV444P10, -1)}
REFUSED_TAGS = ["mono", "411", "444alpha", "420p12", "422p12", "444p12", "420p14", "444p14", "420p16", "444p16", "mono16", "420P10", ""]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("y4m")
    src = d / "harness.cpp"
    src.write_text(HARNESS)
    exe = str(d / "harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, str(src)])
    return exe


def run(exe, data, tmp_path, *ratios):
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    src.write_bytes(data)
    r = subprocess.run([exe, str(src), str(dst)] + [str(x) for x in ratios], capture_output=True, timeout=20,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in err and "runtime error" not in err, (r.returncode, err[-1500:])
    lines = r.stdout.decode(errors="replace").splitlines()
    return lines[0].split(" ", 2), dst.read_bytes(), lines[1:]


def stream(tag, w, h, nframes, seed, extra=b" F30000:1001 Ip A1:1", xtags=b""):
    fmt = TAGS[tag][0]
    head = b"YUV4MPEG2 W%d H%d" % (w, h) + extra + (b" C" + tag.encode() if tag is not None else b"") + xtags + b"\n"
    body = b""
    for k in range(nframes):
        planes = P.frame(seed + k, fmt, w, h)
        body += (b"FRAME\n" if k % 2 == 0 else b"FRAME Ip\n") + b"".join(p.astype(p.dtype.newbyteorder("<")).tobytes() for p in planes)
    return head + body


@pytest.mark.parametrize("tag", list(TAGS), ids=[str(t) for t in TAGS])
def test_every_tag_parses_and_comes_back_bit_for_bit(harness, tmp_path, tag):
    w, h = (40, 30) if TAGS[tag][0] not in F.P444 else (35, 25)
    for xtags, rng_ in ((b"", -1), (b" XYSCSS=420JPEG XCOLORRANGE=FULL", 1), (b" XCOLORRANGE=LIMITED Xanything", 0)):
        data = stream(tag, w, h, 3, 5, xtags=xtags)
        (status, n, rest), out, _ = run(harness, data, tmp_path)
        assert status == "ok" and int(n) == 3 and [int(x) for x in rest.split()] == [TAGS[tag][0], TAGS[tag][1], rng_]
        assert out == data
    assert len(data) == len(data.split(b"\n", 1)[0]) + 1 + 3 * 6 + 3 + R_bytes(TAGS[tag][0], w, h) * 3  # (two plain FRAME lines, one with parameters)


def R_bytes(fmt, w, h):
    return sum(int(np.prod(s)) for s in P.plane_shapes(fmt, w, h)) * F.ES[fmt]


def test_refused_tags_are_named_and_interlaced_streams_refused(harness, tmp_path):
    for tag in REFUSED_TAGS:
        data = b"YUV4MPEG2 W40 H30 F25:1 Ip C" + tag.encode() + b"\nFRAME\n" + bytes(1800)
        (status, n, msg), out, _ = run(harness, data, tmp_path)
        assert status == "refused" and int(n) == 0 and "'C%s'" % tag in msg and out == b"", tag
    for i in ("t", "b", "m"):
        (status, _, msg), _, _ = run(harness, stream("420", 40, 30, 1, 1, extra=b" F25:1 I" + i.encode()), tmp_path)
        assert status == "refused" and "interlaced" in msg and "'I%s'" % i in msg
    for head, word in ((b"YUV4MPEG2 W65537 H30", "W65537"), (b"YUV4MPEG2 W40 H0", "H0"), (b"YUV4MPEG2 W40", "no W or no H"), (b"YUV4MPEG W40 H30", "YUV4MPEG2"),
                       (b"YUV4MPEG2 W41 H30", "odd"), (b"YUV4MPEG2 W40 H31", "odd"), (b"YUV4MPEG2 W40 H30 Q1", "'Q1'"), (b"YUV4MPEG2 W40 H30 F25", "'F25'"),
                       (b"YUV4MPEG2 W40 H30 " + b"X" * 240, "newline")):
        (status, _, msg), _, _ = run(harness, head + b"\nFRAME\n" + bytes(1800), tmp_path)
        assert status == "refused" and word in msg, (head, msg)
    # odd sizes are fine where the format has no such axis
    assert run(harness, stream("422", 40, 31, 1, 1), tmp_path)[0][0] == "ok" and run(harness, stream("444", 41, 31, 1, 1), tmp_path)[0][0] == "ok"


def test_a_cut_stream_keeps_its_whole_frames_and_the_header_is_rewritten(harness, tmp_path):
    data = stream("420mpeg2", 40, 30, 5, 9)
    head = len(data.split(b"\n", 1)[0]) + 1
    per = (len(data) - head) // 5  # (6- and 9-byte FRAME lines alternate: cut well inside frame 4)
    (status, n, msg), out, _ = run(harness, data[:head + 3 * per + 700], tmp_path)
    assert status == "refused" and int(n) == 3 and "inside a frame" in msg and out == data[:len(out)] and len(out) > head + 3 * (per - 2)
    (status, n, msg), out, _ = run(harness, data.replace(b"FRAME Ip\n", b"FRAMF Ip\n", 1), tmp_path)
    assert status == "refused" and int(n) == 1 and "FRAME" in msg
    # W, H and A for another size; F, I, C and X copied; 0:0 stays; the ratio reduced
    src = stream("420p10", 40, 30, 1, 1, extra=b" F30000:1001 Ip A10:11", xtags=b" XCOLORRANGE=FULL XFOO")
    assert run(harness, src, tmp_path, 2, 1, 2, 1)[2] == ["YUV4MPEG2 W80 H60 F30000:1001 Ip A10:11 C420p10 XCOLORRANGE=FULL XFOO"]
    assert run(harness, src, tmp_path, 8, 3, 9, 4)[2] == ["YUV4MPEG2 W106 H67 F30000:1001 Ip A135:176 C420p10 XCOLORRANGE=FULL XFOO"]  # 10 * 9 * 3 : 11 * 8 * 4
    assert run(harness, stream("420", 40, 30, 1, 1, extra=b" A0:0"), tmp_path, 3, 2, 1, 1)[2] == ["YUV4MPEG2 W60 H30 A0:0 C420"]
    assert run(harness, stream(None, 40, 30, 1, 1, extra=b""), tmp_path, 4, 1, 4, 1)[2] == ["YUV4MPEG2 W160 H120"]


def test_mutated_streams_end_cleanly_under_asan_ubsan(harness, tmp_path):
    rng = np.random.default_rng(2027)
    tags = [t for t in TAGS if t is not None]
    counts = {"ok": 0, "refused": 0}
    wild = [b"0", b"-1", b"65537", b"99999999", b"999999999999", b"4294967297", b"1e3", b"", b"40x"]
    for i in range(240):
        tag = tags[i % len(tags)]
        data = bytearray(stream(tag, 24, 18, 3, i))
        head = data.index(b"\n") + 1
        kind = i % 8
        if kind == 0:    # truncation anywhere
            data = data[:int(rng.integers(0, len(data)))]
        elif kind == 1:  # flipped bytes in the header
            for _ in range(int(rng.integers(1, 4))):
                data[int(rng.integers(0, head))] = int(rng.integers(0, 256))
        elif kind == 2:  # flipped bytes anywhere (mostly samples: most of these stay valid)
            for _ in range(int(rng.integers(1, 6))):
                data[int(rng.integers(0, len(data)))] = int(rng.integers(0, 256))
        elif kind == 3:  # wild W / H / F
            which = [b"W24", b"H18", b"F30000:1001"][int(rng.integers(0, 3))]
            data = data.replace(which, which[:1] + wild[int(rng.integers(0, len(wild)))], 1)
        elif kind == 4:  # the header's newline is missing
            data = data[:head - 1] + data[head:]
        elif kind == 5:  # an overlong header
            data = data[:head - 1] + b" X" + b"y" * int(rng.integers(230, 4000)) + data[head - 1:]
        elif kind == 6:  # a broken FRAME magic, in one of the three frames
            k = int(rng.integers(0, 3))
            pos = [j for j in range(len(data)) if data.startswith(b"FRAME", j)][k]
            data[pos + int(rng.integers(0, 5))] ^= 1 << int(rng.integers(0, 7))
        else:            # sizes that do not fit the body: a larger frame than the stream holds, or a huge one
            data = data.replace(b"W24", [b"W26", b"W4096", b"W65536"][int(rng.integers(0, 3))], 1).replace(b"H18", [b"H18", b"H65536"][int(rng.integers(0, 2))], 1)
        (status, n, _), out, _ = run(harness, bytes(data), tmp_path)
        assert status in counts and 0 <= int(n) <= 3 and (int(n) == 0 or out), (i, kind, status)
        counts[status] += 1
    print("240 mutated streams:", counts)
    assert counts["refused"] >= 120
