"""Network interpolation on the host under AddressSanitizer + UndefinedBehaviorSanitizer (CPU; a stand-alone g++ program with its own
main, as tests/test_loader_depth_sanitized.py builds one -- nothing is loaded into Python, nothing is preloaded).

blend_packed (the function behind rsr_model_blend) reads two blobs through offsets that came from outside and writes a third.  The
harness loads and packs the 1- and 2-block synthetic models (seeds 42 / 43) and hands it
  * the honest pairs of either depth at a rounded strength and at both ends, and the two depths against each other;
  * truncated copies of either side;
  * a hundred and four pairs whose table was hit by byte flips, wild 64-bit values (offsets among them) or wild 32-bit values: on one side
    alone, or on BOTH sides alike -- the tables then agree, and wherever the blob check passes the arithmetic runs over the moved segments.
Every blob handed over is a heap copy of exactly the advertised length, and so is the destination: one access past either is an ASan
report.  Every call must end in 0 or a clean negative code; the honest pairs return 0 and their bytes hash to what tests/blend_ref.py
computes -- this build is another compiler's than the library's, and the rule is the same."""
import os
import subprocess

import numpy as np
import pytest

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import synth

import blend_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realsr-ncnn-vulkan_amd", "csrc")
T = float(np.float32(0.3))

HARNESS = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>
#include "model.h"
using namespace rsr;

static std::vector<unsigned char> packed(const char* param, const char* bin)
{
    Model m;
    std::string e;
    if (load_model(param, bin, m, e) != 0) { std::printf("load failed: %s\n", e.c_str()); std::exit(1); }
    std::vector<unsigned char> blob(packed_size(m));
    if (pack_model(m, blob.data(), blob.size(), e) != 0) { std::printf("pack failed: %s\n", e.c_str()); std::exit(1); }
    return blob;
}

// blend_packed on heap copies of EXACTLY na / nb bytes of a / b into a heap buffer of exactly the size it reports; *hash: FNV-1a of the result
static int blend(const std::vector<unsigned char>& a, size_t na, const std::vector<unsigned char>& b, size_t nb, float t, unsigned long long* hash)
{
    std::unique_ptr<unsigned char[]> ha(new unsigned char[na ? na : 1]), hb(new unsigned char[nb ? nb : 1]);
    std::memcpy(ha.get(), a.data(), na);
    std::memcpy(hb.get(), b.data(), nb);
    std::string e;
    size_t need = 0;
    int rc = blend_packed(ha.get(), na, hb.get(), nb, t, nullptr, 0, &need, e);
    if (rc != 0) return rc;
    std::unique_ptr<unsigned char[]> dst(new unsigned char[need ? need : 1]);
    rc = blend_packed(ha.get(), na, hb.get(), nb, t, dst.get(), need, &need, e);
    if (rc == 0 && hash)
    {
        unsigned long long h = 1469598103934665603ull;
        for (size_t i = 0; i < need; i++) h = (h ^ dst[i]) * 1099511628211ull;
        *hash = h;
    }
    return rc;
}

static void mutate(std::vector<unsigned char>& b, std::mt19937_64& rng, int kind, size_t table, size_t total)
{
    if (kind == 0)
        for (int k = 0, n = 1 + int(rng() % 5); k < n; k++) b[rng() % table] = (unsigned char)(rng() & 255);
    else if (kind == 1)
    { // a wild 64-bit value over an aligned 8 bytes: the offsets of a table entry among them
        const unsigned long long wild[8] = {0ull, 1ull << 63, ~0ull, total, total - 1, 1ull << 32, total - 256, (unsigned long long)((table + 255) & ~size_t(255))};
        const size_t off = (rng() % (table - 8)) / 8 * 8;
        std::memcpy(b.data() + off, &wild[rng() % 8], 8);
    }
    else
    { // a wild 32-bit value over a field of the header or of an entry
        const uint32_t wild[5] = {0u, ~0u, 1u << 31, 966u, 967u};
        const size_t off = (rng() % (table - 4)) / 4 * 4;
        std::memcpy(b.data() + off, &wild[rng() % 5], 4);
    }
}

// usage: harness <t> <param a1> <bin a1> <param b1> <bin b1> <param a2> <bin a2> <param b2> <bin b2>
int main(int argc, char** argv)
{
    if (argc != 10) return 2;
    const float t = std::strtof(argv[1], nullptr);
    std::vector<unsigned char> blob[4];
    for (int i = 0; i < 4; i++) blob[i] = packed(argv[2 + 2 * i], argv[3 + 2 * i]);
    for (int d = 0; d < 2; d++)
    {
        const std::vector<unsigned char>&a = blob[2 * d], &b = blob[2 * d + 1];
        const float ts[3] = {t, 0.f, 1.f};
        for (float tt : ts)
        {
            unsigned long long h = 0;
            const int rc = blend(a, a.size(), b, b.size(), tt, &h);
            std::printf("honest %d %.9g %d %llu\n", d + 1, double(tt), rc, h);
        }
        const size_t cuts[5] = {a.size() - 1, a.size() - 256, packed_table_bytes(uint32_t(num_convs(d + 1))), sizeof(PackedHeader), 10};
        for (size_t c : cuts)
        {
            std::printf("cut %d a %zu %d\n", d + 1, c, blend(a, c, b, b.size(), t, nullptr));
            std::printf("cut %d b %zu %d\n", d + 1, c, blend(a, a.size(), b, c, t, nullptr));
        }
    }
    std::printf("depths %d %d\n", blend(blob[0], blob[0].size(), blob[3], blob[3].size(), t, nullptr), blend(blob[2], blob[2].size(), blob[1], blob[1].size(), t, nullptr));
    std::mt19937_64 rng(2026);
    const size_t total = blob[2].size(), table = packed_table_bytes(uint32_t(num_convs(2)));
    for (int i = 0; i < 104; i++)
    {
        std::vector<unsigned char> a = blob[2], b = blob[3];
        const int who = i % 4; // 0: A alone, 1: B alone, 2 and 3: both alike
        std::mt19937_64 twin = rng;
        if (who != 1) mutate(a, rng, (i / 4) % 3, table, total);
        if (who >= 2) rng = twin;
        if (who != 0) mutate(b, rng, (i / 4) % 3, table, total);
        std::printf("mut %d %d %d\n", i, who, blend(a, total, b, total, t, nullptr));
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("san_blend")
    src = d / "harness.cpp"
    src.write_text(HARNESS)
    exe = str(d / "harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           "-o", exe, str(src), os.path.join(CSRC, "model.cpp")])
    return exe


def _fnv(data):
    h = 1469598103934665603
    for chunk in np.array_split(np.frombuffer(data, dtype=np.uint8), max(1, len(data) // 65536)):
        for v in chunk.tolist():
            h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_blend_packed_survives_hostile_blobs_under_asan_ubsan(harness, tmp_path):
    dirs = [synth.make_model_dir(str(tmp_path), "models-DF2K-s%d" % seed, seed, nb=nb) for nb in (1, 2) for seed in (42, 43)]
    args = [p for d in dirs for p in (os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))]
    r = subprocess.run([harness, repr(T)] + args, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
    lines = [ln.split() for ln in r.stdout.splitlines()]
    honest = [ln for ln in lines if ln[0] == "honest"]
    assert len(honest) == 6
    for ln in honest:
        nb, t, rc, h = int(ln[1]), float(ln[2]), int(ln[3]), int(ln[4])
        assert rc == 0
        if nb == 1:  # (hashing a blob byte by byte in Python: the small depth)
            a, b = (R.model_pack(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin")) for d in dirs[:2])
            assert h == _fnv(BR.blend_ref(a, b, t).tobytes()), (nb, t)
    cuts = [ln for ln in lines if ln[0] == "cut"]
    assert len(cuts) == 20 and all(int(ln[4]) == R.RSR_E_FORMAT for ln in cuts), cuts
    assert [ln for ln in lines if ln[0] == "depths"] == [["depths", str(R.RSR_E_GRAPH), str(R.RSR_E_GRAPH)]]
    muts = [(int(ln[2]), int(ln[3])) for ln in lines if ln[0] == "mut"]
    assert len(muts) == 104
    assert all(rc in (R.RSR_OK, R.RSR_E_FORMAT, R.RSR_E_GRAPH) for _, rc in muts), muts
    one_sided = [rc for who, rc in muts if who < 2]
    print("104 mutated pairs: %d refused; of the 52 one-sided %d" % (sum(rc < 0 for _, rc in muts), sum(rc < 0 for rc in one_sided)))
    assert sum(rc < 0 for rc in one_sided) >= 45   # a one-sided change is refused unless it wrote the byte that was there
    assert any(rc == R.RSR_E_GRAPH for rc in one_sided) and any(rc == R.RSR_E_FORMAT for rc in one_sided)
    assert any(rc == R.RSR_OK for who, rc in muts if who >= 2)   # a change on both sides that the blob check passes is blended
