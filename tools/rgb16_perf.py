"""C2 frame (1920 x 1080, tile 200), device-resident, as a 16-bit RGB image in and out (RSR_FMT_U16_HWC) -- and the detour through planar
floats a caller needed before the format existed:

    u16->u16     RSR_FMT_U16_HWC in and out (torch_io.upscale on an (H, W, 3) int16 tensor), at out_scale 4 and 2
    detour u16   torch: widen to float, permute to CHW  ->  torch_io.upscale f32 -> f32  ->  torch: quantise, permute back
    u8->u8       uint8 HWC in and out, the same run (what the default path costs on this board)
    f16->f16     planar fp16 in and out, the same run

All variants alternate inside every repetition, on ONE torch stream, each timed with HIP events around `frames` back-to-back frames.  The
gate is printed per line: the native path must not be slower than its detour by more than the detour's own spread over the repetitions.
Then, reported without a gate: post_ms of the U16 launch next to the unfused uint8 launch (engine option "dbg" 8192) and the F16 one, with
one / two pixels per thread forced (engine option "dbg" 32768 / 65536), the same under TTA (C5), the host call rsr_process_fmt U16 -> U16
from pinned buffers next to rsr_process u8 (and either into a pageable array; every host row is max(reps, 20) calls behind 3 warm-up passes --
the two pinned rows of profiles/rgb16.txt are from `reps` calls behind one), and the command line tool on one 1080p 16-bit PNG end to end.
    python tools/rgb16_perf.py [reps=5] [frames=4] [out=profiles/rgb16.txt]
"""
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import realsr_ncnn_vulkan_amd as R  # noqa: E402
from realsr_ncnn_vulkan_amd import synth, torch_io  # noqa: E402

reps, frames, out_path = 5, 4, None
for kv in sys.argv[1:]:
    k, v = kv.split("=")
    if k == "reps":
        reps = int(v)
    elif k == "frames":
        frames = int(v)
    elif k == "out":
        out_path = v

d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K", 42)
pp, bp = os.path.join(d, "x4.param"), os.path.join(d, "x4.bin")
sr = R.RealSR(0)
sr.load(pp, bp)
sr.tilesize = 200
w, h = 1920, 1080
U8, U16 = R.RSR_FMT_U8_HWC, R.RSR_FMT_U16_HWC

img8 = synth.make_image(3, w, h)
rng = np.random.default_rng(3)
img16 = (img8.astype(np.uint16) * 257 + rng.integers(-128, 129, size=img8.shape)).clip(0, 65535).astype(np.uint16)  # the picture, with low bytes of its own
x8 = torch.from_numpy(img8).cuda()
x16 = torch.from_numpy(img16.view(np.int16)).cuda()  # (int16: the words, read unsigned by the engine)
x16a = torch.cat([x16, x16[:, :, :1]], dim=2).contiguous()  # RGBA: the red words once more as alpha
xf16 = (torch.from_numpy(np.ascontiguousarray(img8.transpose(2, 0, 1))).cuda().float() / 255).half()
st = torch.cuda.Stream()


def detour(x):
    """What a caller did with 16-bit words before RSR_FMT_U16_HWC: floats in planar form in, floats out, quantised by torch."""
    f = ((x.to(torch.int32) & 0xFFFF).float() * (1.0 / 65535.0)).permute(2, 0, 1).contiguous()
    y = torch_io.upscale(sr, f)
    return (y * 65535.0 + 0.5).floor_().to(torch.int32).permute(1, 2, 0).contiguous().to(torch.int16)


def at(scale, f, dbg=0, ctx=None):
    c = ctx or sr

    def g():
        c.out_scale = scale
        c.set_option("dbg", dbg)
        try:
            return f()
        finally:
            c.set_option("dbg", 0)
    return g


def alternate(variants):
    """Every variant once per repetition, `frames` back-to-back frames between two HIP events: ms per frame, per repetition; and what each
    variant returned in the first warm-up pass."""
    times = {n: [] for n, _ in variants}
    with torch.cuda.stream(st):
        outs = {n: f() for n, f in variants}  # warm-up: plans, workspace, torch's kernels and allocator
        for n, f in variants:
            f()
        st.synchronize()
        for rep in range(reps):
            for n, f in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(frames):
                    y = f()
                e1.record(st)
                e1.synchronize()
                del y
                times[n].append(e0.elapsed_time(e1) / frames)
    st.synchronize()
    return times, outs


variants = []
for s_ in (4, 2):
    variants.append(("u16->u16 x%d" % s_, at(s_, lambda: torch_io.upscale(sr, x16))))
    variants.append(("detour u16 x%d" % s_, at(s_, lambda: detour(x16))))
    variants.append(("u8->u8 x%d" % s_, at(s_, lambda: torch_io.upscale(sr, x8))))
    variants.append(("f16->f16 x%d" % s_, at(s_, lambda: torch_io.upscale(sr, xf16))))
times, outs = alternate(variants)
assert tuple(outs["u16->u16 x2"].shape) == (2 * h, 2 * w, 3)


def profiled(c, shapes):
    """post_ms / pre_ms of three profiled frames each (after a warm-up frame of the same shape): the frame with the least post_ms."""
    prof = {}
    c.set_profiling(True)
    with torch.cuda.stream(st):
        for n, f in shapes:
            f()
            st.synchronize()
            for _ in range(3):
                c.get_profile(reset=True)
                f()
                st.synchronize()
                p = c.get_profile(reset=True)
                if n not in prof or p["post_ms"] < prof[n]["post_ms"]:
                    prof[n] = p
    c.set_profiling(False)
    return prof


shapes = []
for s_ in (4, 2):
    shapes.append(("u16->u16 x%d" % s_, at(s_, lambda: torch_io.upscale(sr, x16))))
    shapes.append(("u8->u16 x%d" % s_, at(s_, lambda: torch_io.upscale(sr, x8, out_dtype=torch.int16))))
    if s_ == 4:  # either thread shape of the x4 launch forced: one pixel, two neighbouring pixels per thread (RGB and RGBA)
        for px, dbg in ((1, 32768), (2, 65536)):
            shapes.append(("u16->u16 x4, %d px/thread" % px, at(4, lambda: torch_io.upscale(sr, x16), dbg)))
            shapes.append(("u16->u16 x4 rgba, %d px/thread" % px, at(4, lambda: torch_io.upscale(sr, x16a), dbg)))
    shapes.append(("u8->u8 x%d unfused (dbg 8192)" % s_, at(s_, lambda: torch_io.upscale(sr, x8), 8192)))
    shapes.append(("f16->f16 x%d unfused (dbg 8192)" % s_, at(s_, lambda: torch_io.upscale(sr, xf16), 8192)))
prof = profiled(sr, shapes)

tta = R.RealSR(0, tta_mode=True)  # C5: the same frame under TTA (the eight variants merged by the post-processing launch)
tta.load(pp, bp)
tta.tilesize = 200
tta_shapes = [("tta u16->u16 x4", at(4, lambda: torch_io.upscale(tta, x16), ctx=tta)),
              ("tta u16->u16 x4, 1 px/thread", at(4, lambda: torch_io.upscale(tta, x16), 32768, ctx=tta)),
              ("tta u16->u16 x4, 2 px/thread", at(4, lambda: torch_io.upscale(tta, x16), 65536, ctx=tta)),
              ("tta u8->u8 x4", at(4, lambda: torch_io.upscale(tta, x8), ctx=tta)), ("tta f16->f16 x4", at(4, lambda: torch_io.upscale(tta, xf16), ctx=tta))]
tta_prof = profiled(tta, tta_shapes)
tta.close()

# host -> host from pinned buffers: rsr_process_fmt U16 -> U16 (12.4 MB up, 199 MB down) next to rsr_process u8 (half of each)
sr.out_scale = 4
sr.set_option("dbg", 0)
pins = [R.PinnedArray(s) for s in ((h, w, 6), (4 * h, 4 * w, 6), (h, w, 3), (4 * h, 4 * w, 3))]
a16, o16 = pins[0].array.view(np.uint16).reshape(h, w, 3), pins[1].array.view(np.uint16).reshape(4 * h, 4 * w, 3)
a8, o8 = pins[2].array, pins[3].array
a16[:], a8[:] = img16, img8
p16, p8 = np.empty_like(o16), np.empty_like(o8)  # pageable destinations: the download goes through the lane's two staging slots
host_calls = (("process_fmt u16->u16", lambda: sr.process_fmt(a16, U16, U16, out=o16)), ("process u8", lambda: sr.process(a8, out=o8)),
              ("process_fmt u16->u16, pageable out", lambda: sr.process_fmt(a16, U16, U16, out=p16)), ("process u8, pageable out", lambda: sr.process(a8, out=p8)))
host = {n: [] for n, _ in host_calls}
host_warm, host_reps = 3, max(reps, 20)
for rep in range(host_warm + host_reps):
    for n, f in host_calls:
        t0 = time.perf_counter()
        f()
        if rep >= host_warm:  # (the first passes warm the lanes up and touch the pageable arrays)
            host[n].append((time.perf_counter() - t0) * 1e3)
same_as_device = bool(np.array_equal(o16.view(np.int16), outs["u16->u16 x4"].cpu().numpy()))
pageable_same = bool(np.array_equal(p16, o16) and np.array_equal(p8, o8))
for p in pins:
    p.free()


def png16(path, img):
    hh, ww, c = img.shape
    rows = img.astype(">u2").view(np.uint8).reshape(hh, ww * c * 2)
    raw = b"".join(b"\0" + r.tobytes() for r in rows)

    def chunk(t, body):
        return struct.pack(">I", len(body)) + t + body + struct.pack(">I", zlib.crc32(t + body) & 0xffffffff)
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", ww, hh, 16, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 1)) + chunk(b"IEND", b""))


cli = os.path.join(ROOT, "realsr-ncnn-vulkan_amd", "bin", "realsr-hip")
cli_lines = []
with tempfile.TemporaryDirectory() as td:
    png16(os.path.join(td, "in.png"), img16)
    for depth in ("auto", "8"):
        t0 = time.perf_counter()
        r = subprocess.run([cli, "-i", os.path.join(td, "in.png"), "-o", os.path.join(td, "out_%s.png" % depth), "-m", d], capture_output=True, text=True,
                           env=dict(os.environ, RSR_DEPTH=depth))
        dt = time.perf_counter() - t0
        size = os.path.getsize(os.path.join(td, "out_%s.png" % depth)) if r.returncode == 0 else 0
        cli_lines.append("realsr-hip, one 1920 x 1080 16-bit PNG, RSR_DEPTH=%-4s: exit %d, %.2f s wall clock (process start, model load, decode, frame, encode), output %.1f MB"
                         % (depth, r.returncode, dt, size / 1e6))

lines = ["C2 frame 1920 x 1080, tile 200, device-resident, %d repetitions x %d frames per variant, alternating, HIP events on one stream" % (reps, frames),
         "device: %s" % torch.cuda.get_device_name(0),
         "%-20s %9s %9s %9s   %s" % ("variant", "median ms", "min ms", "max ms", "per repetition")]
met = []
for n, _ in variants:
    t = times[n]
    line = "%-20s %9.2f %9.2f %9.2f   %s" % (n, np.median(t), min(t), max(t), " ".join("%.2f" % v for v in t))
    if n.startswith("u16"):
        scale = n.split()[-1]
        dt = times["detour u16 %s" % scale]
        spread = max(dt) - min(dt)
        ok = bool(np.median(t) <= np.median(dt) + spread)
        met.append(ok)
        code = lambda a: a.to(torch.int32) & 0xFFFF  # noqa: E731
        diff = int((code(outs[n]) - code(outs["detour u16 %s" % scale])).abs().max())
        line += "   gate: <= detour %.2f + its spread %.2f ms: %s (%+.2f %%); max code difference to the detour %d" % (
            np.median(dt), spread, "met" if ok else "NOT MET", (np.median(t) / np.median(dt) - 1) * 100, diff)
    lines.append(line)
lines.append("gates met: %d of %d" % (sum(met), len(met)))
lines.append("post_ms / pre_ms of a profiled frame (the least post_ms of three; no gate).  The U16 launch at x4: postproc_tiles (one pixel per thread, sample")
lines.append("stores) or postproc_tiles_u16x2 (two pixels: three dword stores per RGB pair, two 8-byte stores per RGBA pair) -- at its default and with either forced:")
for n, _ in shapes:
    lines.append("%-34s pre_ms %.3f post_ms %.3f post_bytes %.1f MB" % (n, prof[n]["pre_ms"], prof[n]["post_ms"], prof[n]["post_bytes"] / 1e6))
lines.append("C5: the same frame under TTA (no gate):")
for n, _ in tta_shapes:
    lines.append("%-34s pre_ms %.3f post_ms %.3f" % (n, tta_prof[n]["pre_ms"], tta_prof[n]["post_ms"]))
lines.append("host -> host from a pinned input, into a pinned or a pageable output, wall clock per call, %d calls each after %d warm-up passes, alternating (no gate);" % (host_reps, host_warm))
lines.append("process_fmt moves twice the bytes over PCIe:")
for n, t in host.items():
    lines.append("%-34s median %.2f ms, min %.2f, max %.2f" % (n, np.median(t), min(t), max(t)))
lines.append("process_fmt u16->u16 equals the device call byte for byte: %s; the pageable outputs equal the pinned ones: %s" % (same_as_device, pageable_same))
lines += cli_lines
text = "\n".join(lines)
print(text)
if out_path:
    with open(out_path, "w") as fh:
        fh.write(text + "\n")
sr.close()
