"""C2 frame (1920 x 1080, tile 200), device-resident, with engine option "dither" on and off:

    u8->u8 dither 1          the planar blob and one dithering postproc_tiles launch
    u8->u8 dither 0 unfused  the same route without the dither (engine option "dbg" 8192: conv_last never writes the image itself)
    u8->u8 dither 0          the default: conv_last's fused store (what leaving the fused epilogue costs; reported, not gated)
    nv12->nv12 dither 1 / 0  the same post launch with and without the dither (a YUV output is never fused)

All variants alternate inside every repetition, on ONE torch stream, each timed with HIP events around `frames` back-to-back frames.
Gate (a), printed per line: a dithered frame must not be slower than the same call at dither 0 on the unfused route by more than that
call's own spread over the repetitions.  Then, without a gate: post_ms of every dithered launch beside its undithered sibling, from
profiled frames -- uint8, uint16, NV12, P010, out_scale 2, and uint8 under TTA (C5).
    python tools/dither_perf.py [reps=5] [frames=4] [out=profiles/dither.txt]
"""
import os
import sys

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

img8 = synth.make_image(3, w, h)
x8 = torch.from_numpy(img8).cuda()
rng = np.random.default_rng(3)
nv12 = torch.from_numpy(rng.integers(16, 236, size=(h * 3 // 2, w), dtype=np.uint8)).cuda()
p010 = (nv12.to(torch.int32) << 8).to(torch.int16)  # (the 8-bit codes as 10-bit ones in the high bits)
st = torch.cuda.Stream()


def at(f, dither, dbg=0, scale=4, ctx=None):
    c = ctx or sr

    def g():
        c.out_scale = scale
        c.dither = dither
        c.set_option("dbg", dbg)
        try:
            return f(c)
        finally:
            c.set_option("dbg", 0)
            c.dither = 0
    return g


def rgb(c):
    return torch_io.upscale(c, x8)


def rgb16(c):
    return torch_io.upscale(c, x8, out_dtype=torch.int16)


def yuv8(c):
    return torch_io.upscale_yuv(c, nv12)


def yuv10(c):
    return torch_io.upscale_yuv(c, p010)


def alternate(variants):
    """Every variant once per repetition, `frames` back-to-back frames between two HIP events: ms per frame, per repetition."""
    times = {n: [] for n, _ in variants}
    with torch.cuda.stream(st):
        for _ in range(2):  # warm-up: plans, workspace, torch's allocator
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
    return times


variants = [("u8->u8 dither 1", at(rgb, 1)), ("u8->u8 dither 0 unfused", at(rgb, 0, 8192)), ("u8->u8 dither 0", at(rgb, 0)),
            ("nv12->nv12 dither 1", at(yuv8, 1)), ("nv12->nv12 dither 0", at(yuv8, 0))]
times = alternate(variants)
GATES = {"u8->u8 dither 1": "u8->u8 dither 0 unfused", "nv12->nv12 dither 1": "nv12->nv12 dither 0"}


def profiled(c, shapes):
    """post_ms of three profiled frames each (after a warm-up frame of the same shape): the frame with the least post_ms."""
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


pairs = [("u8->u8 x4", rgb, 8192, 4), ("u8->u16 x4", rgb16, 0, 4), ("nv12->nv12 x4", yuv8, 0, 4), ("p010->p010 x4", yuv10, 0, 4),
         ("u8->u8 x2", rgb, 0, 2), ("nv12->nv12 x2", yuv8, 0, 2)]
shapes = []
for n, f, dbg0, scale in pairs:
    shapes.append((n + " dither 0", at(f, 0, dbg0, scale)))
    shapes.append((n + " dither 1", at(f, 1, 0, scale)))
prof = profiled(sr, shapes)

tta = R.RealSR(0, tta_mode=True)  # C5: the same frame under TTA (the staged uint8 kernel merges the eight variants and dithers)
tta.load(pp, bp)
tta.tilesize = 200
tta_shapes = [("tta u8->u8 x4 dither 0", at(rgb, 0, ctx=tta)), ("tta u8->u8 x4 dither 1", at(rgb, 1, ctx=tta))]
tta_prof = profiled(tta, tta_shapes)
tta.close()

lines = ["C2 frame 1920 x 1080, tile 200, device-resident, %d repetitions x %d frames per variant, alternating, HIP events on one stream" % (reps, frames),
         "device: %s" % torch.cuda.get_device_name(0),
         "%-26s %9s %9s %9s   %s" % ("variant", "median ms", "min ms", "max ms", "per repetition")]
met = []
for n, _ in variants:
    t = times[n]
    line = "%-26s %9.2f %9.2f %9.2f   %s" % (n, np.median(t), min(t), max(t), " ".join("%.2f" % v for v in t))
    if n in GATES:
        bt = times[GATES[n]]
        spread = max(bt) - min(bt)
        ok = bool(np.median(t) <= np.median(bt) + spread)
        met.append(ok)
        line += "   gate (a): <= '%s' %.2f + its spread %.2f ms: %s (%+.2f %%)" % (GATES[n], np.median(bt), spread, "met" if ok else "NOT MET",
                                                                                   (np.median(t) / np.median(bt) - 1) * 100)
    lines.append(line)
lines.append("gates met: %d of %d" % (sum(met), len(met)))
fused, dith = np.median(times["u8->u8 dither 0"]), np.median(times["u8->u8 dither 1"])
lines.append("the price of leaving the fused epilogue (no gate): u8->u8 dither 1 %.2f ms against the fused default %.2f ms: %+.2f ms (%+.2f %%)"
             % (dith, fused, dith - fused, (dith / fused - 1) * 100))
lines.append("post_ms of a profiled frame (the least of three; no gate), every dithered launch under its undithered sibling (u8->u8 x4 dither 0: dbg 8192):")
for n, _ in shapes:
    lines.append("%-30s post_ms %.3f post_bytes %.1f MB" % (n, prof[n]["post_ms"], prof[n]["post_bytes"] / 1e6))
lines.append("C5: the same frame under TTA (no gate):")
for n, _ in tta_shapes:
    lines.append("%-30s post_ms %.3f" % (n, tta_prof[n]["post_ms"]))
text = "\n".join(lines)
print(text)
if out_path:
    with open(out_path, "w") as fh:
        fh.write(text + "\n")
sr.close()
