"""A PNG writer and reader for 16-bit samples that owe nothing to the tool's codecs (numpy + zlib): what tests/cli_support.py is for 8 bits.
The reader undoes all five filter types, for either depth; samples come back as uint16 (depth 16) or uint8 in the file's own channel count."""
import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"
CTYPE = {1: 0, 2: 4, 3: 2, 4: 6}


def chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)


def png16_bytes(img, filt=0, trns=None):
    """The file of a uint16 image (h, w) gray, (h, w, 2) gray+alpha, (h, w, 3) RGB or (h, w, 4) RGBA: depth 16, big-endian samples, filter
    type 0 or 2 on every row.  trns: the colour key of a tRNS chunk (one value for gray, three for RGB)."""
    assert img.dtype == np.uint16
    h, w = img.shape[:2]
    c = 1 if img.ndim == 2 else img.shape[2]
    rows = img.reshape(h, w * c).astype(">u2").view(np.uint8).reshape(h, w * c * 2)
    if filt == 2:
        up = np.vstack([np.zeros((1, rows.shape[1]), np.uint8), rows[:-1]])
        rows = (rows.astype(np.int16) - up).astype(np.uint8)
    raw = b"".join(bytes([filt]) + r.tobytes() for r in rows)
    out = SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, CTYPE[c], 0, 0, 0))
    if trns is not None:
        out += chunk(b"tRNS", b"".join(struct.pack(">H", v) for v in trns))
    return out + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b"")


def write_png16(path, img, filt=0, trns=None):
    with open(path, "wb") as f:
        f.write(png16_bytes(img, filt, trns))


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def read_png(path):
    """(samples, depth): the image as (h, w, c) uint8 or uint16, c the file's channel count; colour types 0, 2, 4, 6, no interlace."""
    d = open(path, "rb").read()
    assert d[:8] == SIG
    pos, idat = 8, b""
    while pos < len(d):
        n, t = struct.unpack(">I4s", d[pos:pos + 8])
        body = d[pos + 8:pos + 8 + n]
        assert zlib.crc32(t + body) & 0xffffffff == struct.unpack(">I", d[pos + 8 + n:pos + 12 + n])[0], t
        if t == b"IHDR":
            w, h, depth, ctype, comp, flt, lace = struct.unpack(">IIBBBBB", body)
            assert depth in (8, 16) and (comp, flt, lace) == (0, 0, 0)
        elif t == b"IDAT":
            idat += body
        pos += 12 + n
    c = {0: 1, 2: 3, 4: 2, 6: 4}[ctype]
    bpp, stride = c * depth // 8, w * c * depth // 8
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, stride + 1)
    out = np.zeros((h, stride), np.int32)
    for y in range(h):
        ft, row = int(raw[y, 0]), raw[y, 1:].astype(np.int32)
        prev = out[y - 1] if y else np.zeros(stride, np.int32)
        if ft == 0:
            out[y] = row
        elif ft == 2:
            out[y] = (row + prev) & 255
        elif ft == 1:
            for i in range(bpp):
                out[y, i::bpp] = np.cumsum(row[i::bpp]) & 255
        elif ft in (3, 4):
            cur = out[y]
            for i in range(stride):
                a = cur[i - bpp] if i >= bpp else 0
                b = prev[i]
                cc = prev[i - bpp] if i >= bpp else 0
                cur[i] = (row[i] + ((a + b) >> 1 if ft == 3 else _paeth(int(a), int(b), int(cc)))) & 255
        else:
            raise AssertionError("filter type %d" % ft)
    by = out.astype(np.uint8)
    if depth == 16:
        return by.reshape(h, w * c, 2).copy().view(">u2").astype(np.uint16).reshape(h, w, c), 16
    return by.reshape(h, w, c), 8
