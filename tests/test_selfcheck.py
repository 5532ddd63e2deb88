"""Model self-check (rsr_selfcheck*, option "precise_auto"): what can be said without a GPU -- the built-in tile, the C ABI, argument
and call-order errors, the CLI's usage exit.  The device side is tests/test_gpu_selfcheck.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import realsr_ncnn_vulkan_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "realsr-ncnn-vulkan_amd", "bin", "realsr-hip")
NEW_SYMBOLS = ("rsr_selfcheck", "rsr_selfcheck_tile", "rsr_selfcheck_ranges")


def test_builtin_tile_is_deterministic_host_only_and_made_of_byte_levels():
    """rsr_selfcheck_tile needs no device.  Two calls give the same bytes; every value is fp16(k / 255) for an integer k -- both as the
    preprocessing computes it (float32(k) * float32(1 / 255), rounded to fp16) and as the plain quotient -- levels 0 and 255 are used,
    and the tile has what the storage error depends on: flat areas, smooth ramps, hard edges and fine texture."""
    a, b = R.selfcheck_tile(), R.selfcheck_tile(148, 148)
    assert a.shape == (3, 148, 148) and a.dtype == np.float16
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))
    k = np.arange(256)
    lut = (k.astype(np.float32) * np.float32(1 / 255.0)).astype(np.float16)
    assert np.array_equal(lut.view(np.uint16), (k / 255.0).astype(np.float16).view(np.uint16))
    assert np.isin(a.view(np.uint16), lut.view(np.uint16)).all()
    assert a.min() == 0.0 and a.max() == 1.0 and np.isfinite(a).all()
    lvl = np.searchsorted(lut.astype(np.float32), a.astype(np.float32)).astype(int)  # the byte level of every pixel (lut is increasing)
    assert np.array_equal(lut[lvl].view(np.uint16), a.view(np.uint16))
    assert len(np.unique(lvl)) >= 200  # covers 0 .. 1, not a few levels
    dx = np.abs(np.diff(lvl, axis=2))
    assert (dx == 0).mean() > 0.05      # flat runs
    assert ((dx >= 1) & (dx <= 3)).mean() > 0.1  # ramps: gentle steps on a good part of the smooth half of the tile
    assert (dx >= 100).mean() > 0.01    # hard edges
    # fine texture: somewhere a 16 x 16 window whose horizontal differences change sign on more than half of the pixels
    sgn = np.sign(np.diff(lvl[0].astype(int), axis=1))
    flips = (sgn[:, 1:] * sgn[:, :-1] < 0)
    assert max(flips[y:y + 16, x:x + 16].mean() for y in range(0, 130, 8) for x in range(0, 128, 8)) > 0.5
    # other sizes: deterministic too
    c = R.selfcheck_tile(40, 24)
    assert c.shape == (3, 24, 40) and np.array_equal(c.view(np.uint16), R.selfcheck_tile(40, 24).view(np.uint16))
    assert np.isin(c.view(np.uint16), lut.view(np.uint16)).all()


def test_selfcheck_argument_and_state_errors_without_a_device():
    """NULL context / NULL destination / bad sizes: RSR_E_ARG, reached without touching a device."""
    L = R.lib()
    rep = R.SelfcheckReport()
    assert L.rsr_selfcheck(None, None, 0, 0, C.byref(rep)) == R.RSR_E_ARG
    assert L.rsr_selfcheck_ranges(None, None, None, 351) == R.RSR_E_ARG
    assert L.rsr_selfcheck_tile(None, 148, 148) == R.RSR_E_ARG
    buf = np.zeros(3 * 8 * 8, dtype=np.uint16)
    assert L.rsr_selfcheck_tile(buf.ctypes.data_as(C.c_void_p), -1, 8) == R.RSR_E_ARG
    assert L.rsr_selfcheck_tile(buf.ctypes.data_as(C.c_void_p), 0, 8) == R.RSR_E_ARG
    assert L.rsr_selfcheck_tile(buf.ctypes.data_as(C.c_void_p), 8, 8) == R.RSR_OK and buf.any()
    assert L.rsr_set_option(None, b"precise_auto", 1) == R.RSR_E_ARG


def test_python_mirror_declares_the_new_entry_points():
    assert set(NEW_SYMBOLS) <= set(R.EXPORTS)
    L = R.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s), s
    assert C.sizeof(R.SelfcheckReport) == 64  # the C struct: 2 int, 2 float, int (+ pad), long long, float, int, long long, 2 int, float (+ pad)
    assert b"gfx950" in L.rsr_version()


def test_header_with_the_selfcheck_api_is_plain_c_and_a_c_host_reaches_it(tmp_path):
    """include/realsr_hip.h still compiles as C99 -pedantic; a host written in C links against the three new symbols, lays the report
    struct out as the Python mirror does, and gets the built-in tile and the argument errors without a GPU."""
    src = tmp_path / "host.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "realsr_hip.h"
static uint16_t tile[3 * 148 * 148], again[3 * 148 * 148];
int main(void)
{
    rsr_selfcheck_report rep;
    size_t i;
    int lo = 0, hi = 0, same = 1;
    int rc_tile = rsr_selfcheck_tile(tile, 0, 0), rc2 = rsr_selfcheck_tile(again, 148, 148);
    int rc_null = rsr_selfcheck(NULL, NULL, 0, 0, &rep), rc_rng = rsr_selfcheck_ranges(NULL, NULL, NULL, 351);
    for (i = 0; i < sizeof tile / sizeof tile[0]; i++)
    {
        lo |= tile[i] == 0;
        hi |= tile[i] == 0x3c00;
        same &= tile[i] == again[i];
    }
    printf("tile %d %d lo %d hi %d same %d null %d ranges %d size %d off %d %d\n", rc_tile, rc2, lo, hi, same, rc_null, rc_rng, (int)sizeof rep,
           (int)offsetof(rsr_selfcheck_report, bytes_differ), (int)offsetof(rsr_selfcheck_report, elapsed_ms));
    return 0;
}
''')
    lib = os.path.join(ROOT, "realsr-ncnn-vulkan_amd", "lib")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(inc, "realsr_hip.h")])
    exe = str(tmp_path / "host")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", inc, "-o", exe, str(src), "-L", lib, "-lrealsr_hip", "-Wl,-rpath," + lib])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tile 0 0 lo 1 hi 1 same 1 null -1 ranges -1 size %d off %d %d" % (
        C.sizeof(R.SelfcheckReport), R.SelfcheckReport.bytes_differ.offset, R.SelfcheckReport.elapsed_ms.offset) in r.stdout, r.stdout
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(lib, "librealsr_hip.so")], text=True)
    for s in NEW_SYMBOLS:
        assert " T %s\n" % s in out, s


def test_selfcheck_before_load_is_a_state_error():
    """Call order: a context that holds no model answers RSR_E_STATE (rsr_selfcheck) and keeps "precise_auto" for the next load.  A context
    needs a device, so without one the creation's loud failure is all there is to see."""
    import torch
    if not torch.cuda.is_available():
        try:
            R.RealSR(0)
        except R.RealSRError as e:
            assert e.code < 0
            return
        raise AssertionError("a context was created without a device")
    s = R.RealSR(0)
    try:
        rep = R.SelfcheckReport()
        assert s._L.rsr_selfcheck(s._h, None, 0, 0, C.byref(rep)) == R.RSR_E_STATE
        assert s._L.rsr_selfcheck_ranges(s._h, None, None, 351) == R.RSR_E_STATE
        s.set_option("precise_auto", 1)  # remembered, nothing to check yet
        assert s.get_stat("selfcheck_runs") == 0 and s.get_stat("selfcheck_ms") == -1 and s.get_stat("precise_active") == 0
    finally:
        s.close()


def test_cli_usage_exit_is_unchanged():
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert r.returncode != 0 and "Usage:" in r.stderr and "-j load:proc:save" in r.stderr
