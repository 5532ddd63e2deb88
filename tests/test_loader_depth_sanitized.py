"""The packed-blob check at any depth under AddressSanitizer + UndefinedBehaviorSanitizer (CPU; a stand-alone g++ program with its own
main, as tests/test_loader_sanitized.py builds one -- nothing is loaded into Python, nothing is preloaded).

Since a blob's header names its own conv count, check_packed sizes its walk by a number that came from outside.  The harness loads and
packs the 1- and 2-block synthetic models, then hands check_packed
  * headers whose nconv is rewritten to counts around every bound (0, 5, 6, 20, 21, 22, 36, 351, 352, 966, 967, 981, 2^32 - 1), each with
    three lengths of the buffer it may read: the true table, the advertised table (where the blob is that long), the bare header;
  * a hundred byte-flip / wild-offset mutations of the 2-block table.
Every buffer handed over is a heap copy of exactly head_bytes bytes, so one read past it is an ASan report.  Every input must end in
0 or a clean negative code; only the unmutated headers with their whole table in reach return 0."""
import os
import subprocess

import pytest

from realsr_ncnn_vulkan_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realsr-ncnn-vulkan_amd", "csrc")
NCONVS = [0, 5, 6, 20, 21, 22, 36, 351, 352, 966, 967, 981, 2 ** 32 - 1]

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

// check_packed on a heap copy of EXACTLY head_bytes bytes of `blob`
static int check(const std::vector<unsigned char>& blob, size_t head_bytes, size_t total)
{
    std::unique_ptr<unsigned char[]> h(new unsigned char[head_bytes ? head_bytes : 1]);
    std::memcpy(h.get(), blob.data(), head_bytes);
    std::string e;
    return check_packed(h.get(), head_bytes, total, e);
}

// usage: harness <param> <bin> <nb> <nconv>...      prints "sweep <nconv> <which> <rc>", "mut <i> <rc>", "ok <nb>"
int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    Model m;
    std::string e;
    int rc = load_model(argv[1], argv[2], m, e);
    const int nb = std::atoi(argv[3]);
    if (rc != 0 || m.nb != nb || int(m.convs.size()) != num_convs(nb)) { std::printf("load failed: %d %s\n", rc, e.c_str()); return 1; }
    std::vector<unsigned char> blob(packed_size(m));
    rc = pack_model(m, blob.data(), blob.size(), e);
    if (rc != 0) { std::printf("pack failed: %d %s\n", rc, e.c_str()); return 1; }
    const size_t total = blob.size(), table = packed_table_bytes(uint32_t(m.convs.size()));
    if (check(blob, total, total) != 0 || check(blob, table, total) != 0) { std::printf("the unmutated blob is refused\n"); return 1; }
    std::printf("ok %d nconv %zu table %zu total %zu\n", nb, m.convs.size(), table, total);
    for (int a = 4; a < argc; a++)
    {
        const uint32_t nconv = uint32_t(std::strtoull(argv[a], nullptr, 10));
        std::vector<unsigned char> b = blob;
        std::memcpy(b.data() + offsetof(PackedHeader, nconv), &nconv, 4);
        const unsigned long long adv = sizeof(PackedHeader) + (unsigned long long)nconv * sizeof(PackedConv); // (64-bit: 2^32 - 1 entries do not wrap)
        std::printf("sweep %u true %d\n", nconv, check(b, table, total));
        if (adv <= total) std::printf("sweep %u advertised %d\n", nconv, check(b, size_t(adv), total));
        std::printf("sweep %u header %d\n", nconv, check(b, sizeof(PackedHeader), total));
    }
    if (nb == 2)
    {
        std::mt19937_64 rng(2026);
        for (int i = 0; i < 102; i++)
        {
            std::vector<unsigned char> b = blob;
            if (i % 3 == 0)
                for (int k = 0, n = 1 + int(rng() % 5); k < n; k++) b[rng() % table] = (unsigned char)(rng() & 255);
            else if (i % 3 == 1)
            { // a wild 64-bit value over an aligned 8 bytes: the offsets of a table entry among them
                const unsigned long long wild[6] = {0ull, 1ull << 63, ~0ull, total, total - 1, 1ull << 32};
                const size_t off = (rng() % (table - 8)) / 8 * 8;
                std::memcpy(b.data() + off, &wild[rng() % 6], 8);
            }
            else
            { // a wild 32-bit value over a field of the header or of an entry
                const uint32_t wild[5] = {0u, ~0u, 1u << 31, 966u, 967u};
                const size_t off = (rng() % (table - 4)) / 4 * 4;
                std::memcpy(b.data() + off, &wild[rng() % 5], 4);
            }
            std::printf("mut %d %d\n", i, check(b, table, total));
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("san_depth")
    src = d / "harness.cpp"
    src.write_text(HARNESS)
    exe = str(d / "harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           "-o", exe, str(src), os.path.join(CSRC, "model.cpp")])
    return exe


@pytest.mark.parametrize("nb", [1, 2])
def test_check_packed_survives_rewritten_conv_counts_under_asan_ubsan(harness, nb, tmp_path):
    d = synth.make_model_dir(str(tmp_path), nb=nb)
    r = subprocess.run([harness, os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"), str(nb)] + [str(n) for n in NCONVS],
                       capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert lines[0][:2] == ["ok", str(nb)]   # the unmutated header returned 0 (with the whole blob and with the table alone in reach)
    true_nconv = 15 * nb + 6
    sweep = [(int(ln[1]), ln[2], int(ln[3])) for ln in lines if ln[0] == "sweep"]
    assert {n for n, _, _ in sweep} == set(NCONVS)
    assert {w for _, w, _ in sweep} == {"true", "advertised", "header"}
    for n, which, rc in sweep:
        # 0 only where nothing was changed and the whole table is in reach; everything else is RSR_E_FORMAT
        want = 0 if (n == true_nconv and which != "header") else -3
        assert rc == want, (n, which, rc)
    assert sum(1 for n, w, _ in sweep if w == "advertised") >= len(NCONVS) - 1   # (only 2^32 - 1 entries are longer than the blob)
    muts = [int(ln[2]) for ln in lines if ln[0] == "mut"]
    assert len(muts) == (102 if nb == 2 else 0)
    assert all(rc <= 0 for rc in muts)
    if nb == 2:
        print("102 mutated tables: %d refused" % sum(rc < 0 for rc in muts))
        assert sum(rc < 0 for rc in muts) >= 60   # the mutations do bite (a flip inside padding or to the same value leaves the table valid)
