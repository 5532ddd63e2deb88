"""Network interpolation of two packed blobs, restated in numpy from the rule of include/realsr_hip.h ("network interpolation"):
u = fp32(1) - t; every fp16 weight c = fp16_rne((u * float(a)) + (t * float(b))), every fp32 bias c = (u * a) + (t * b), every operation
rounded by itself in fp32 (numpy's float32 ufuncs: one rounding each, no fused multiply-add); t == 0 / t == 1 are A's / B's bytes; every
byte outside the segments is A's.  The segments come from the conv table this module parses itself."""
import struct

import numpy as np

HEADER = struct.Struct("<4IQ")    # magic, version, nconv, flags, total_bytes
ENTRY = struct.Struct("<5If3Q")   # cin, cout, act, nplanes, nt, slope, b_off, w16_off, aux_off
# the strengths the tests blend at: the ends (copies), a half and a quarter (exact products), 0.3 and 1e-3 (rounded ones), the last float below 1
T_VALUES = [0.0, 1.0, 0.5, 0.25, float(np.float32(0.3)), float(np.float32(1e-3)), float(np.nextafter(np.float32(1), np.float32(0)))]
T_IDS = ["0", "1", "0.5", "0.25", "0.3", "1e-3", "below1"]


def as_bytes(blob):
    return np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)


def table(blob):
    """(header tuple, [entry tuples]) of a packed blob."""
    blob = as_bytes(blob)
    head = HEADER.unpack_from(blob, 0)
    return head, [ENTRY.unpack_from(blob, HEADER.size + i * ENTRY.size) for i in range(head[2])]


def table_bytes(blob):
    return HEADER.size + table(blob)[0][2] * ENTRY.size


def segments(blob):
    """[(byte offset, byte count, dtype)] of everything in the blob that is a number: per conv the fp32 biases, the fp16 w16 image, and
    the fp16 aux image where the conv has one."""
    out = []
    for cin, cout, act, nplanes, nt, slope, b_off, w16_off, aux_off in table(blob)[1]:
        out.append((b_off, nt * 32 * 4, np.float32))
        out.append((w16_off, 2 * nplanes * 9 * nt * 32 * 32, np.float16))
        if aux_off:
            out.append((aux_off, 2 * nplanes * 3 * 32 * 32, np.float16))
    return out


def blend_ref(blob_a, blob_b, t):
    a, b = as_bytes(blob_a), as_bytes(blob_b)
    n = table_bytes(a)
    assert a.size == b.size and np.array_equal(a[:n], b[:n]), "the rule is defined for byte-identical headers and tables"
    t = np.float32(t)
    assert 0 <= t <= 1
    if t == 0:
        return a.copy()
    if t == 1:
        return b.copy()
    u = np.float32(1) - t
    c = a.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for off, nbytes, dt in segments(a):
            x = a[off:off + nbytes].view(dt).astype(np.float32)
            y = b[off:off + nbytes].view(dt).astype(np.float32)
            p = u * x
            q = t * y
            c[off:off + nbytes] = (p + q).astype(dt).view(np.uint8)
    return c


def extreme_pair(tmp, synth):
    """Two hand-made 1-block model directories whose weights hold, in conv_first, in a dense conv, in conv_last (the aux image) and in
    the biases: +-65504 on both sides, a = -b, fp16 subnormals, +0 against -0.  Returns (dir_a, dir_b)."""
    import os
    wa, wb = synth.make_weights(42, nb=1), synth.make_weights(43, nb=1)
    sub = np.float32(2.0 ** -24)  # the smallest fp16 subnormal
    # (a, b) per slot of a conv's first output channel, first input channel, taps 0..8; then of its second output channel
    taps = [(65504.0, 65504.0), (-65504.0, -65504.0), (65504.0, -65504.0), (sub, 3 * sub), (sub, 0.0), (-5 * sub, 1023 * sub), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0)]
    for i in (0, 3, len(wa) - 1):
        for k, (x, y) in enumerate(taps):
            wa[i][0][0, 0, k // 3, k % 3], wb[i][0][0, 0, k // 3, k % 3] = x, y
        wb[i][0][1] = -wa[i][0][1]                       # a whole output channel with a = -b
        wa[i][0][2, 1:] = 65504.0                        # ... one at the top of the range on both sides
        wb[i][0][2, 1:] = 65504.0
        wa[i][0][2, 0] = np.float32(2.0 ** -14)          # the smallest normal against the largest subnormal
        wb[i][0][2, 0] = 1023 * sub
        ba, bb = wa[i][1], wb[i][1]
        ba[0], bb[0] = 65504.0, 65504.0
        ba[1], bb[1] = -65504.0, 65504.0
        ba[2], bb[2] = sub, 3 * sub
        if ba.size > 4:
            ba[3], bb[3] = 0.0, -0.0
            ba[4], bb[4] = -0.0, 0.0
            ba[5], bb[5] = np.float32(1e-40), np.float32(-3e-39)  # fp32 subnormals
            ba[6], bb[6] = np.float32(3.0e38), np.float32(3.0e38)
    dirs = []
    for name, ws in (("a", wa), ("b", wb)):
        d = os.path.join(str(tmp), "extreme-" + name)
        os.makedirs(d, exist_ok=True)
        synth.write_param(os.path.join(d, "x4.param"), 1)
        synth.write_bin(os.path.join(d, "x4.bin"), ws, "fp16")
        dirs.append(d)
    return dirs
