"""The 16-bit codecs of the command line tool (image_io.h: is_16bit, load_image16, save_png16) as stand-alone programs, without a GPU:
16-bit PNGs of every colour type and P5 / P6 files with maxval 65535 go through load_image16 -> save_png16 and are read back, sample for
sample, by a numpy + zlib reader (tests/png16_ref.py; Pillow reduces 16-bit RGB, so it is not the judge); a second build under ASan + UBSan
runs the loader over mutated and truncated files."""
import os
import subprocess

import numpy as np
import pytest

from cli_support import ROOT, write_png
from png16_ref import png16_bytes, read_png, write_png16

CSRC = os.path.join(ROOT, "realsr-ncnn-vulkan_amd", "csrc")
LIB = os.path.join(ROOT, "realsr-ncnn-vulkan_amd", "lib")

ROUNDTRIP = r'''
#include "image_io.h"
int main(int c, char** v)
{
    std::vector<uint8_t> f;
    if (!imgio::read_file(v[1], f)) return 3;
    const bool deep = imgio::is_16bit(f);
    Image im;
    std::string e = imgio::load_image16(v[1], im);
    if (!e.empty()) { printf("%d\n", int(deep)); fprintf(stderr, "%s\n", e.c_str()); return 1; }
    e = imgio::save_png16(v[2], im);
    if (!e.empty()) { fprintf(stderr, "%s\n", e.c_str()); return 2; }
    printf("%d %d %d %d %d\n", int(deep), im.w, im.h, im.elempack, im.depth);
    return 0;
}
'''

# No HIP: the two functions of the library that Image calls are malloc and free here.
FUZZ = r'''
#include "image_io.h"
extern "C" void* rsr_host_alloc(size_t n) { return malloc(n); }
extern "C" void rsr_host_free(void* p) { free(p); }
int main(int c, char** v)
{
    int ok = 0, bad = 0;
    for (int i = 1; i < c; i++)
    {
        std::vector<uint8_t> f;
        if (!imgio::read_file(v[i], f)) return 3;
        Image im, im8;
        const bool deep = imgio::is_16bit(f);
        const std::string e = imgio::load_image16(f, im);
        if (e.empty() && (!deep || im.depth != 16 || im.empty() || im.size_bytes() != size_t(im.w) * im.h * im.elempack * 2)) return 4;
        if (e.empty())
        { // every sample is readable
            unsigned long long s = 0;
            for (size_t k = 0; k < size_t(im.w) * im.h * im.elempack; k++) s += im.data16()[k];
            if (s == 0xffffffffffffffffull) return 5;
        }
        (void)imgio::load_image(v[i], im8); // the 8-bit loader over the same bytes
        e.empty() ? ok++ : bad++;
    }
    printf("%d %d\n", ok, bad);
    return 0;
}
'''


def build(d, name, text, flags, libs):
    src = d / (name + ".cpp")
    src.write_text(text)
    exe = d / name
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + flags + ["-I", CSRC, "-o", str(exe), str(src)] + libs + ["-lz", "-ldl"])
    return str(exe)


@pytest.fixture(scope="module")
def roundtrip(tmp_path_factory):
    return build(tmp_path_factory.mktemp("png16"), "t_png16", ROUNDTRIP, [], ["-L", LIB, "-lrealsr_hip", "-Wl,-rpath," + LIB])


@pytest.fixture(scope="module")
def fuzz(tmp_path_factory):
    return build(tmp_path_factory.mktemp("png16_san"), "t_png16_san", FUZZ, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], [])


def image(shape, seed):
    img = np.random.default_rng(seed).integers(0, 65536, shape).astype(np.uint16)
    img.reshape(-1)[:6] = [0, 1, 255, 256, 32768, 65535]  # byte-order and sign traps
    return img


def expanded(img):
    """gray -> RGB, gray+alpha -> RGBA, as the 8-bit loader expands them."""
    if img.ndim == 2:
        return np.repeat(img[:, :, None], 3, 2)
    if img.shape[2] == 2:
        return np.concatenate([np.repeat(img[:, :, :1], 3, 2), img[:, :, 1:]], 2)
    return img


SHAPES = {"gray": (11, 7), "gray-alpha": (6, 5, 2), "rgb": (13, 17, 3), "rgba": (9, 20, 4)}


@pytest.mark.parametrize("filt", [0, 2])
@pytest.mark.parametrize("kind", list(SHAPES))
def test_png16_roundtrip(roundtrip, tmp_path, kind, filt):
    img = image(SHAPES[kind], len(kind) + filt)
    write_png16(tmp_path / "in.png", img, filt)
    out = subprocess.check_output([roundtrip, str(tmp_path / "in.png"), str(tmp_path / "out.png")]).decode().split()
    want = expanded(img)
    assert [int(v) for v in out] == [1, want.shape[1], want.shape[0], want.shape[2], 16]
    got, depth = read_png(tmp_path / "out.png")
    assert depth == 16 and got.dtype == np.uint16 and np.array_equal(got, want)


@pytest.mark.parametrize("filt", [0, 2])
def test_png16_rgb_with_a_colour_key(roundtrip, tmp_path, filt):
    """RGB + tRNS: RGBA with alpha 0 exactly on the keyed pixels and 65535 elsewhere (stb's rule, at 16 bits)."""
    img = image((10, 12, 3), 5)
    key = (513, 40000, 65535)
    img[2:4, 3:6] = key
    write_png16(tmp_path / "k.png", img, filt, trns=key)
    out = subprocess.check_output([roundtrip, str(tmp_path / "k.png"), str(tmp_path / "k2.png")]).decode().split()
    assert [int(v) for v in out] == [1, 12, 10, 4, 16]
    got, depth = read_png(tmp_path / "k2.png")
    keyed = (img == np.array(key, dtype=np.uint16)).all(axis=2)
    assert depth == 16 and np.array_equal(got[:, :, :3], img) and np.array_equal(got[:, :, 3], np.where(keyed, 0, 65535)) and keyed.sum() >= 6


@pytest.mark.parametrize("magic,c", [(b"P6", 3), (b"P5", 1)])
def test_pnm16(roundtrip, tmp_path, magic, c):
    img = image((5, 4, c), 9 + c)
    with open(tmp_path / "a.pnm", "wb") as f:
        f.write(magic + b"\n# 16 bits\n4 5\n65535\n" + img.astype(">u2").tobytes())
    out = subprocess.check_output([roundtrip, str(tmp_path / "a.pnm"), str(tmp_path / "o.png")]).decode().split()
    assert [int(v) for v in out] == [1, 4, 5, 3, 16]
    got, depth = read_png(tmp_path / "o.png")
    assert depth == 16 and np.array_equal(got, np.repeat(img, 3, 2) if c == 1 else img)


def test_what_is_not_16_bit(roundtrip, tmp_path):
    """is_16bit says no to an 8-bit PNG, an 8-bit PNM and a PNM with another maxval above 255, and load_image16 refuses them."""
    write_png(tmp_path / "e.png", np.zeros((4, 4, 3), np.uint8))
    (tmp_path / "e.ppm").write_bytes(b"P6\n2 2\n255\n" + bytes(12))
    (tmp_path / "m.ppm").write_bytes(b"P6\n2 2\n1023\n" + bytes(24))
    (tmp_path / "t.ppm").write_bytes(b"P6\n2 2\n65535\n" + bytes(23))  # one byte short
    for name, deep in (("e.png", 0), ("e.ppm", 0), ("m.ppm", 0), ("t.ppm", 1)):
        r = subprocess.run([roundtrip, str(tmp_path / name), str(tmp_path / "o.png")], capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout.split() == [str(deep)], (name, r.stdout, r.stderr)


def test_loader_over_mutated_files_under_sanitizers(fuzz, tmp_path):
    """ASan + UBSan (no recovery) over at least 200 truncated and mutated 16-bit files: every one is decoded or refused, none trips a check."""
    rng = np.random.default_rng(77)
    seeds = [png16_bytes(image(s, 3), f) for s in SHAPES.values() for f in (0, 2)]
    seeds.append(png16_bytes(image((6, 6, 3), 4), 0, trns=(1, 2, 3)))
    seeds += [m + b"\n7 5\n65535\n" + image((5, 7, c), 6).astype(">u2").tobytes() for m, c in ((b"P6", 3), (b"P5", 1))]
    files = []
    for k, good in enumerate(seeds):
        variants = [good]
        variants += [good[:n] for n in sorted(set(int(v) for v in rng.integers(0, len(good), 8)) | {1, 8, 26, 33, len(good) - 1})]
        for _ in range(12):
            b = bytearray(good)
            for at in rng.integers(0, len(b), int(rng.integers(1, 4))):
                b[at] = int(rng.integers(0, 256))
            variants.append(bytes(b))
        for j in (16, 17, 18, 19, 20, 21, 22, 23, 24, 25):  # the IHDR / header fields, byte by byte: sizes, depth, colour type
            b = bytearray(good)
            if j < len(b):
                b[j] = 0xFF if b[j] != 0xFF else 0x7F
                variants.append(bytes(b))
        for i, v in enumerate(variants):
            p = tmp_path / ("f%02d_%03d" % (k, i))
            p.write_bytes(v)
            files.append(str(p))
    assert len(files) >= 200
    env = dict(os.environ, ASAN_OPTIONS="allocator_may_return_null=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([fuzz] + files, capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-3000:])
    ok, bad = (int(v) for v in r.stdout.split())
    assert ok + bad == len(files) and ok >= len(seeds) and bad >= 50
