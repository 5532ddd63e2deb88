"""Generates tests/golden/format_rules.json: what the library's host-only format functions answer over a grid of formats, sizes, pitches,
tile sizes and output ratios -- return value, ow, oh and, where the call is refused, the rsr_last_error text.

    python tests/golden/make_format_rules.py          # needs the built library only: no GPU is touched

tests/test_format_rules.py replays the same grid (cases() below) against the current build and compares answer by answer, texts
included: the record of what a pixel format IS to the host code, taken before that knowledge moved into one table (kernels.h PixFmt).

Layout of the file: {"args_sha256": of the grid, "messages": [text, ...], "answers": {entry point: run-length list}}.  One answer is an
int (rsr_image_bytes / rsr_image_span accepted: the value), [ow, oh] (a size function accepted) or {"no": [rc, message index]} (refused;
a size function adds ow, oh: what the call left in its outputs, -1 = untouched); a run is [count, answer]."""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "format_rules.json")

VALID = (0, 1, 2, 4, 5, 8, 9, 12, 13)
FORMATS = VALID + (-1, 3, 6, 7, 10, 11, 14)
CS = (1, 3, 4)
WS = (1, 2, 3, 35, 36)
HS = (1, 2, 25, 26)
TILES = (3, 6, 16, 32)
RATIOS = ((4, 1), (2, 1), (1, 1), (3, 2), (4, 3), (9, 4), (3, 1), (6, 4), (5, 1), (1, 2), (0, 1))
PAIRS = (((8, 3), (9, 4)), ((3, 2), (1, 1)), ((9, 8), (3, 2)), ((9, 8), (9, 8)), ((1, 1), (17, 9)))
XY = tuple((r, r) for r in RATIOS) + PAIRS  # what the per-axis functions are asked: every single ratio on both axes, then the pairs
SAMPLE = {0: 1, 1: 2, 2: 4, 4: 1, 5: 2, 8: 1, 9: 2, 12: 1, 13: 2}  # bytes of one sample ("element"); an invalid format counts as 1


def pitches(fmt, w, h, c):
    """The (row pitch, plane pitch) pairs one image is described with: 0, packed, packed -+ 1, packed + element, -1, 2^31 for the rows;
    0, h * row, that + 1, + element, -1 for the planes (row: the pitch in force, the packed one where the row pitch is 0 or negative)."""
    e = SAMPLE.get(fmt, 1)
    packed = w * (c if fmt == 0 else e)
    for row in (0, packed, packed - 1, packed + 1, packed + e, -1, 1 << 31):
        r = row if row > 0 else packed
        for plane in (0, h * r, h * r + 1, h * r + e, -1):
            yield row, plane


def cases():
    """(entry point, argument tuple) in the order of the file."""
    for fmt, c, w, h in itertools.product(FORMATS, CS, WS, HS):
        yield "rsr_image_bytes", (fmt, w, h, c)
    for fmt, c, w, h in itertools.product(FORMATS, CS, WS, HS):
        for row, plane in pitches(fmt, w, h, c):
            yield "rsr_image_span", (fmt, w, h, c, row, plane)
    for name in ("rsr_out_size", "rsr_out_size_yuv"):
        for (n, d), T, w, h in itertools.product(RATIOS, TILES, WS, HS):
            yield name, (n, d, T, w, h)
    for name in ("rsr_out_size_xy", "rsr_out_size_yuv_xy"):
        for ((nx, dx), (ny, dy)), T, w, h in itertools.product(XY, TILES, WS, HS):
            yield name, (nx, dx, ny, dy, T, w, h)
    for fmt, ((nx, dx), (ny, dy)), T, w, h in itertools.product(FORMATS, XY, TILES, WS, HS):
        yield "rsr_out_size_fmt", (fmt, nx, dx, ny, dy, T, w, h)


def ask(L, name, args):
    """One call: the value, (rc, ow, oh), or for a refusal (rc, text[, ow, oh])."""
    if name in ("rsr_image_bytes", "rsr_image_span"):
        v = getattr(L, name)(*args)
        return v if v >= 0 else (v, L.rsr_last_error(None).decode())
    ow, oh = C.c_int(-1), C.c_int(-1)
    rc = getattr(L, name)(*args, C.byref(ow), C.byref(oh))
    return (rc, ow.value, oh.value) if rc == 0 else (rc, L.rsr_last_error(None).decode(), ow.value, oh.value)


def record(L):
    """{"args_sha256", "messages", "answers"} of the library L over cases()."""
    messages, answers, sha = [], {}, hashlib.sha256()
    for name, args in cases():
        sha.update(repr((name, args)).encode())
        a = ask(L, name, args)
        if isinstance(a, tuple) and isinstance(a[1], str):
            if a[1] not in messages:
                messages.append(a[1])
            a = {"no": [a[0], messages.index(a[1])] + list(a[2:])}
        elif isinstance(a, tuple):
            a = list(a[1:])
        runs = answers.setdefault(name, [])
        if runs and runs[-1][1] == a:
            runs[-1][0] += 1
        else:
            runs.append([1, a])
    return {"args_sha256": sha.hexdigest(), "messages": messages, "answers": answers}


def expand(rec):
    """The answers of a record, one per case, in the order of cases(): value, [ow, oh] or {"no": [rc, text, ...]}."""
    its = {name: itertools.chain.from_iterable(itertools.repeat(a, k) for k, a in runs) for name, runs in rec["answers"].items()}
    for name, _ in cases():
        a = next(its[name])
        yield {"no": [a["no"][0], rec["messages"][a["no"][1]]] + a["no"][2:]} if isinstance(a, dict) else a


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import realsr_ncnn_vulkan_amd as R
    rec = record(R.lib())
    with open(OUT, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d cases, %d messages, %d bytes" % (OUT, sum(1 for _ in cases()), len(rec["messages"]), os.path.getsize(OUT)))
