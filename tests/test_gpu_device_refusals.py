"""What the descriptor-taking device entry points REFUSE (run with -m gpu): rsr_process_device_batch, rsr_process_device_masked,
rsr_process_device_sequence, rsr_diff_tiles and rsr_diff_tiles_sequence against one table of bad descriptors.  Every call must return
RSR_E_ARG on the host, before anything is launched: the output and mask buffers keep their 0xCD bytes and no counter of rsr_get_stat moves.

The geometry is 40 x 36 at tile 32, prepadding 10: a 2 x 2 tile grid whose last column is 8 wide and whose last row is 4 high; the forms
that take several images get three.  A fault of ONE descriptor is placed in the first and in the last image of every array the entry
point takes (inputs, outputs, the previous output / frame); a fault of the call's format or size applies to all of them at once."""
import ctypes as C

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R

pytestmark = pytest.mark.gpu
U8, F16, F32, NV12, P010 = R.RSR_FMT_U8_HWC, R.RSR_FMT_F16_CHW, R.RSR_FMT_F32_CHW, R.RSR_FMT_NV12, R.RSR_FMT_P010
ES = {U8: 3, F16: 2, F32: 4, NV12: 1, P010: 2}  # bytes of one element of a row (uint8 HWC with c == 3: of one pixel)
W, H, T, P = 40, 36, 32, 10
NT, N = 4, 3
COUNTERS = ("device_direct", "batch_calls", "batch_images", "batch_groups", "masked_calls", "masked_tiles_run", "masked_tiles_skipped",
            "masked_batches", "masked_table_us", "seq_calls", "seq_frames", "seq_tiles_run", "seq_tiles_copied", "seq_batches",
            "merged_batches", "merged_images", "merged_mixed", "plans", "ws_failures", "workspace_mb")

# One bad descriptor: (id, format of the call, what becomes of a good (ptr, 0, 0) descriptor of a w-wide image of that format)
DESCRIPTOR_FAULTS = [
    ("null-data", U8, lambda p, w: (0, 0, 0)),
    ("row-pitch-one-below-packed", U8, lambda p, w: (p, w * ES[U8] - 1, 0)),
    ("negative-plane-pitch", F32, lambda p, w: (p, 0, -1)),
    ("f16-at-odd-address", F16, lambda p, w: (p + 1, 0, 0)),
    ("pitch-no-element-multiple", F16, lambda p, w: (p, w * ES[F16] + 1, 0)),
]
# A bad call: (id, format, w, c) -- every descriptor of it is a good packed one
CALL_FAULTS = [
    ("odd-w-nv12", NV12, W + 1, 3),
    ("w-beyond-2^24", U8, (1 << 24) + 1, 3),
    ("unknown-format", 7, W, 3),
    ("planar-with-c4", F16, W, 4),
]


@pytest.fixture(scope="module")
def rig(model_dir):
    """A loaded context at the test's tile size, three input buffers, three output buffers and a previous output (each large enough for
    any format of the table at x4, the outputs filled with 0xCD), and a device mask buffer of N * NT sentinel bytes."""
    import os
    s = R.RealSR(0)
    s.load(os.path.join(model_dir, "x4.param"), os.path.join(model_dir, "x4.bin"))
    s.tilesize, s.prepadding = T, P
    s._push_params()
    nin = (W + 2) * H * 12 + 64
    ins = [torch.zeros(nin, dtype=torch.uint8, device="cuda") for _ in range(N)]
    outs = [torch.full((16 * nin,), 0xCD, dtype=torch.uint8, device="cuda") for _ in range(N + 1)]
    mask = torch.full((N * NT,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    yield s, ins, outs[:N], outs[N], mask
    s.close()


def good(bufs):
    return [(b.data_ptr(), 0, 0) for b in bufs]


def variants(arr, fault, w):
    """`arr` with the fault in its first and in its last descriptor (one variant where it has one descriptor)."""
    for i in sorted({0, len(arr) - 1}):
        yield i, arr[:i] + [fault(arr[i][0], w)] + arr[i + 1:]


def entry_calls(s, ins, outs, prev, mask, fmt, w, c, fault=None):
    """(label, thunk) of every call of the table row: each thunk returns the entry point's return code.  fault None: all descriptors good."""
    L, h_, vp = s._L, s._h, C.c_void_p
    ones = np.ones(N * NT, dtype=np.uint8)
    part = np.array([1, 0, 0, 1], dtype=np.uint8)  # a masked call that builds tables of its own
    im = R._images

    def batch(i, o):
        return lambda: L.rsr_process_device_batch(h_, len(i), im(i), fmt, w, H, c, im(o), fmt, None)

    def masked(i, o):
        return lambda: L.rsr_process_device_masked(h_, im(i), fmt, w, H, c, im(o), fmt, part.ctypes.data_as(vp), NT, None)

    def sequence(i, o, p):
        return lambda: L.rsr_process_device_sequence(h_, len(i), im(i), fmt, w, H, c, im(o), fmt, im(p) if p else None, ones.ctypes.data_as(vp), N * NT, None)

    def diff(a, b):
        return lambda: L.rsr_diff_tiles(h_, im(a), im(b), fmt, w, H, c, vp(mask.data_ptr()), None)

    def diff_seq(f, p):
        return lambda: L.rsr_diff_tiles_sequence(h_, len(f), im(f), im(p) if p else None, fmt, w, H, c, vp(mask.data_ptr()), None)

    gi, go, gp = good(ins), good(outs), good([prev])
    if fault is None:
        return [("batch", batch(gi, go)), ("masked", masked(gi[:1], go[:1])), ("sequence", sequence(gi, go, None)), ("sequence+prev", sequence(gi, go, gp)),
                ("diff", diff(gi[:1], gi[1:2])), ("diff_seq", diff_seq(gi, None)), ("diff_seq+prev", diff_seq(gi, gp))]
    ow = w * 4  # (the output descriptors are checked against the x4 width)
    calls = []
    for k, bad in variants(gi, fault, w):
        calls += [("batch in[%d]" % k, batch(bad, go)), ("sequence in[%d]" % k, sequence(bad, go, gp)), ("diff_seq frames[%d]" % k, diff_seq(bad, gp))]
    for k, bad in variants(go, fault, ow):
        calls += [("batch out[%d]" % k, batch(gi, bad)), ("sequence out[%d]" % k, sequence(gi, bad, None))]
    calls += [("masked in", masked([fault(gi[0][0], w)], go[:1])), ("masked out", masked(gi[:1], [fault(go[0][0], ow)])),
              ("sequence prev_out", sequence(gi, go, [fault(gp[0][0], ow)])),
              ("diff a", diff([fault(gi[0][0], w)], gi[1:2])), ("diff b", diff(gi[:1], [fault(gi[1][0], w)])),
              ("diff_seq prev", diff_seq(gi, [fault(gp[0][0], w)]))]
    return calls


def untouched(outs, prev, mask):
    torch.cuda.synchronize()
    return all(bool((b == 0xCD).all()) for b in list(outs) + [prev, mask])


def refused(rig, calls):
    s, ins, outs, prev, mask = rig
    before = {k: s.get_stat(k) for k in COUNTERS}
    for label, thunk in calls:
        assert thunk() == R.RSR_E_ARG, label
    assert untouched(outs, prev, mask)
    for k in COUNTERS:
        assert s.get_stat(k) == before[k], k


@pytest.mark.parametrize("name,fmt,fault", DESCRIPTOR_FAULTS, ids=[f[0] for f in DESCRIPTOR_FAULTS])
def test_a_bad_descriptor_is_refused_by_every_entry_point(rig, name, fmt, fault):
    s, ins, outs, prev, mask = rig
    calls = entry_calls(s, ins, outs, prev, mask, fmt, W, 3, fault)
    assert len(calls) == 3 * 2 + 2 * 2 + 6
    refused(rig, calls)


@pytest.mark.parametrize("name,fmt,w,c", CALL_FAULTS, ids=[f[0] for f in CALL_FAULTS])
def test_a_bad_format_or_size_is_refused_by_every_entry_point(rig, name, fmt, w, c):
    s, ins, outs, prev, mask = rig
    refused(rig, entry_calls(s, ins, outs, prev, mask, fmt, w, c))


def test_two_faults_at_once_the_same_one_is_named(rig):
    """Which refusal a call with two faults gets.  Recorded on the commit before the host call skeleton was folded into one:
      * an output ratio the image does not take (4/3 of 40 x 36) AND a null data pointer: the ratio is named ("output ratio 4/3: w, h and
        tilesize times 4 must be multiples of 3 ..."), by the batch, the masked and the sequence form alike -- the ratio is looked at before
        any descriptor;
      * a null data pointer AND a row pitch below a row, in one descriptor or in two of one array: the null pointer of the first image is
        named ("image 0: null data pointer")."""
    s, ins, outs, prev, mask = rig
    L = s._L
    null = lambda p, w: (0, 0, 0)
    null_and_pitch = lambda p, w: (0, w * ES[U8] - 1, 0)
    short = lambda p, w: (p, w * ES[U8] - 1, 0)
    before = {k: s.get_stat(k) for k in COUNTERS}

    def messages(calls, want):
        for label, thunk in calls:
            assert thunk() == R.RSR_E_ARG, label
            assert want in L.rsr_last_error(s._h).decode(), (label, L.rsr_last_error(s._h).decode())

    process_forms = ("batch", "masked", "sequence")
    s.out_ratio = (4, 3)
    try:
        calls = [c for c in entry_calls(s, ins, outs, prev, mask, U8, W, 3, null) if c[0].startswith(process_forms)]
        assert len(calls) == 11
        messages(calls, "output ratio 4/3")
    finally:
        s.out_ratio = 4
    gi, go, gp = good(ins), good(outs), good([prev])
    im = R._images
    ones = np.ones(N * NT, dtype=np.uint8)
    for first in (null_and_pitch, null):  # both in the first descriptor; the null pointer in the first, the short pitch in the last
        bad = [first(gi[0][0], W)] + gi[1:-1] + [short(gi[-1][0], W)]
        messages([("batch", lambda: L.rsr_process_device_batch(s._h, N, im(bad), U8, W, H, 3, im(go), U8, None)),
                  ("sequence", lambda: L.rsr_process_device_sequence(s._h, N, im(bad), U8, W, H, 3, im(go), U8, im(gp), ones.ctypes.data_as(C.c_void_p), N * NT, None)),
                  ("diff_seq", lambda: L.rsr_diff_tiles_sequence(s._h, N, im(bad), im(gp), U8, W, H, 3, C.c_void_p(mask.data_ptr()), None))],
                 "image 0: null data pointer")
    assert untouched(outs, prev, mask)
    for k in COUNTERS:
        assert s.get_stat(k) == before[k], k


def test_process_device_fmt_does_not_ask_for_float_alignment(rig, model_dir):
    """rsr_process_device_fmt takes raw pointers and checks less than the descriptor forms: the header asks only P010 data to be aligned to
    its samples there.  Recorded on the commit before the fold: an F32 pointer at base + 2 (and an F16 pointer at base + 1) passes the
    argument checks -- on a context without a model the call gets as far as RSR_E_STATE ("process before load"), the refusal that follows
    them --, while a P010 pointer at base + 1 is RSR_E_ARG there.  The context has no model so that no kernel ever runs on a misaligned
    float pointer in this test."""
    s, ins, outs, prev, mask = rig
    vp = C.c_void_p
    fresh = R.RealSR(0)
    try:
        L, pin, pout = fresh._L, ins[0].data_ptr(), outs[0].data_ptr()
        assert L.rsr_process_device_fmt(fresh._h, vp(pin + 2), F32, W, H, 3, vp(pout), F32, None) == R.RSR_E_STATE
        assert "before load" in L.rsr_last_error(fresh._h).decode()
        assert L.rsr_process_device_fmt(fresh._h, vp(pin), F32, W, H, 3, vp(pout + 2), F32, None) == R.RSR_E_STATE
        assert L.rsr_process_device_fmt(fresh._h, vp(pin + 1), F16, W, H, 3, vp(pout + 1), F16, None) == R.RSR_E_STATE
        assert L.rsr_process_device_fmt(fresh._h, vp(pin + 1), P010, W, H, 3, vp(pout), P010, None) == R.RSR_E_ARG
        assert L.rsr_process_device_fmt(fresh._h, vp(pin), P010, W, H, 3, vp(pout + 1), P010, None) == R.RSR_E_ARG
        assert L.rsr_process_device_fmt(fresh._h, vp(pin), P010, W, H, 3, vp(pout), P010, None) == R.RSR_E_STATE
    finally:
        fresh.close()
    assert untouched(outs, prev, mask)


def test_the_good_calls_of_the_table_run(rig):
    """The table's good descriptors are good: the same calls without a fault return RSR_OK (so a refusal above is the fault's doing)."""
    s, ins, outs, prev, mask = rig
    scratch = [torch.full_like(o, 0xCD) for o in outs] + [torch.full_like(prev, 0xCD)]
    m = torch.full_like(mask, 0xCD)
    for label, thunk in entry_calls(s, ins, scratch[:N], scratch[N], m, U8, W, 3):
        assert thunk() == R.RSR_OK, label
    torch.cuda.synchronize()
    assert bool((m[:NT] <= 1).all())
