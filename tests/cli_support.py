"""What the tests of the command line tool share: where the built tool is, and a PNG writer and reader that owe nothing to the tool's own
codecs (numpy + zlib)."""
import os
import struct
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "realsr-ncnn-vulkan_amd", "bin", "realsr-hip")


def write_png(path, img, filt=0):
    """Independent PNG writer (numpy + zlib): 8-bit RGB/RGBA/gray, given filter type per row (0 or 2)."""
    h, w = img.shape[:2]
    c = 1 if img.ndim == 2 else img.shape[2]
    ctype = {1: 0, 2: 4, 3: 2, 4: 6}[c]
    rows = img.reshape(h, w * c).astype(np.uint8)
    if filt == 2:
        up = np.vstack([np.zeros((1, w * c), np.uint8), rows[:-1]])
        rows = (rows.astype(np.int16) - up).astype(np.uint8)
    raw = b"".join(bytes([filt]) + r.tobytes() for r in rows)

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def read_png(path):
    """Independent PNG reader for what save_png emits (8-bit RGB/RGBA, any filter)."""
    d = open(path, "rb").read()
    assert d[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat = 8, b""
    while pos < len(d):
        n, t = struct.unpack(">I4s", d[pos:pos + 8])
        body = d[pos + 8:pos + 8 + n]
        if t == b"IHDR":
            w, h, depth, ctype = struct.unpack(">IIBB", body[:10])
        elif t == b"IDAT":
            idat += body
        pos += 12 + n
    c = {2: 3, 6: 4}[ctype]
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, w * c + 1)
    out = np.zeros((h, w * c), np.uint8)
    for y in range(h):
        ft, row = raw[y, 0], raw[y, 1:].astype(np.int32)
        if ft == 0:
            out[y] = row
        elif ft == 1:
            for i in range(c):
                out[y, i::c] = np.cumsum(row[i::c]) & 255
        elif ft == 2:
            out[y] = (row + (out[y - 1] if y else 0)) & 255
        else:
            raise AssertionError("unexpected filter %d" % ft)
    return out.reshape(h, w, c)
