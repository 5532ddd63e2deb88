"""Option "out_scale" (x2 / x1 output, box-reduced on the device) against out_scale 4 and against the detour a user had to take before
(x4, then torch.nn.functional.avg_pool2d over the x4 image):

    A  C2 device-resident   1920 x 1080, tile 200: u8 -> u8 and f16 -> f16 at out_scale 4, 2, 1, and x4 + avg_pool2d (2, 4)
    B  C2 host -> host      the same frame from and into pinned buffers (rsr_process) at out_scale 4 and 2
    C  C5 (TTA)             f16 -> f16 at out_scale 4 and 2, and x4 + avg_pool2d(2)
    D  post_ms              of rsr_get_profile for each device-resident variant, from a separate profiled pass

All variants of a section alternate inside every repetition, on ONE torch stream (B: wall clock around the synchronous call), medians
over the repetitions after a warm-up.  The synthetic model has the real model's shapes, hence its timing.
    python tools/out_scale_perf.py [reps=7] [out=profiles/out_scale.txt]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import realsr_ncnn_vulkan_amd as R  # noqa: E402
from realsr_ncnn_vulkan_amd import synth, torch_io  # noqa: E402

reps, out_path = 7, None
for kv in sys.argv[1:]:
    k, v = kv.split("=")
    if k == "reps":
        reps = int(v)
    elif k == "out":
        out_path = v

W, H, T = 1920, 1080, 200
d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K", 42)
st = torch.cuda.Stream()
lines = ["option out_scale: 1920 x 1080 frame, tile 200, %d repetitions per variant, alternating, after a warm-up" % reps,
         "device: %s" % torch.cuda.get_device_name(0)]
frame8 = synth.make_image(1235, W, H)
x8 = torch.from_numpy(frame8).cuda()
x16 = torch.from_numpy(np.ascontiguousarray((frame8.astype(np.float32) * np.float32(1 / 255.0)).transpose(2, 0, 1))).cuda().half()


def context(tta):
    sr = R.RealSR(0, tta_mode=tta)
    sr.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
    sr.tilesize = T
    return sr


def at(sr, scale, x):
    def f():
        sr.out_scale = scale
        return torch_io.upscale(sr, x)
    return f


def detour(sr, k, x):
    """What a user does today: the x4 image out of the library, then a pass over it."""
    def f():
        sr.out_scale = 4
        y = torch_io.upscale(sr, x)
        if y.dtype == torch.uint8:  # (avg_pool2d has no uint8 kernel: HWC bytes -> planar float -> pool -> bytes)
            p = torch.nn.functional.avg_pool2d(y.permute(2, 0, 1).float()[None], k)[0]
            return (p + 0.5).floor().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()
        return torch.nn.functional.avg_pool2d(y[None], k)[0]
    return f


def table(title, times, base):
    lines.append("")
    lines.append(title)
    lines.append("%-24s %9s %9s %9s   %s" % ("variant", "median ms", "min ms", "max ms", "per repetition"))
    bmed = float(np.median(times[base]))
    for n, t in times.items():
        lines.append("%-24s %9.3f %9.3f %9.3f   %s   (%+.2f %% vs %s)" % (n, np.median(t), min(t), max(t), " ".join("%.3f" % v for v in t),
                                                                        (np.median(t) / bmed - 1) * 100, base))
    spread = max(times[base]) - min(times[base])
    lines.append("spread of %s over the repetitions: %.3f ms (max - min)" % (base, spread))
    return bmed, spread


def measure(title, variants):
    """variants: [(name, f)], the first is out_scale 4; HIP events on one stream."""
    times = {n: [] for n, _ in variants}
    with torch.cuda.stream(st):
        for _ in range(2):  # warm-up: plans, workspace, torch's kernels and allocator
            for n, f in variants:
                f()
        st.synchronize()
        for rep in range(reps):
            for n, f in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                y = f()
                e1.record(st)
                e1.synchronize()
                del y
                times[n].append(e0.elapsed_time(e1))
    st.synchronize()
    bmed, spread = table(title, times, variants[0][0])
    return {n: float(np.median(t)) for n, t in times.items()}, spread


def gate(what, ok):
    lines.append("gate: %-86s %s" % (what, "met" if ok else "MISSED"))


def post_ms(sr, variants):
    """A separate profiled pass: the post-processing launches' share (rsr_get_profile; profiling turns merging off and adds events)."""
    out = []
    sr.set_profiling(True)
    try:
        for n, f in variants:
            with torch.cuda.stream(st):
                f()
                st.synchronize()
                sr.get_profile(reset=True)
                for _ in range(3):
                    f()
                st.synchronize()
            p = sr.get_profile(reset=True)
            out.append("%-24s post %.3f ms, pre %.3f ms, conv %.3f ms, total %.3f ms per frame" % (n, p["post_ms"] / 3, p["pre_ms"] / 3, p["conv_ms"] / 3, p["total_ms"] / 3))
    finally:
        sr.set_profiling(False)
    return out


sr = context(False)
prof_lines = []
for name, x in (("u8 -> u8", x8), ("f16 -> f16", x16)):
    v = [("out_scale 4", at(sr, 4, x)), ("out_scale 2", at(sr, 2, x)), ("out_scale 1", at(sr, 1, x)),
         ("x4 + avg_pool2d(2)", detour(sr, 2, x)), ("x4 + avg_pool2d(4)", detour(sr, 4, x))]
    med, spread = measure("A  C2 device-resident, %s" % name, v)
    gate("C2 %s: out_scale 2 <= out_scale 4 + its spread (%.3f <= %.3f + %.3f ms)" % (name, med["out_scale 2"], med["out_scale 4"], spread),
         med["out_scale 2"] <= med["out_scale 4"] + spread)
    gate("C2 %s: out_scale 2 faster than x4 + avg_pool2d(2) (%.3f < %.3f ms)" % (name, med["out_scale 2"], med["x4 + avg_pool2d(2)"]),
         med["out_scale 2"] < med["x4 + avg_pool2d(2)"])
    gate("C2 %s: out_scale 1 faster than x4 + avg_pool2d(4) (%.3f < %.3f ms)" % (name, med["out_scale 1"], med["x4 + avg_pool2d(4)"]),
         med["out_scale 1"] < med["x4 + avg_pool2d(4)"])
    prof_lines += ["C2 %s:" % name] + post_ms(sr, v[:3])

# ---- B: host -> host from pinned buffers ----
pin_in = R.PinnedArray(frame8.shape)
pin_in.array[:] = frame8
outs = {s: R.PinnedArray((H * s, W * s, 3)) for s in (4, 2)}
times = {"out_scale 4": [], "out_scale 2": []}
for rep in range(reps + 1):
    for s in (4, 2):
        sr.out_scale = s
        t0 = time.perf_counter()
        sr.process(pin_in.array, out=outs[s].array)
        if rep:
            times["out_scale %d" % s].append((time.perf_counter() - t0) * 1e3)
table("B  C2 host -> host, pinned buffers (rsr_process, wall clock)", times, "out_scale 4")
m4, m2 = float(np.median(times["out_scale 4"])), float(np.median(times["out_scale 2"]))
gate("C2 host -> host: out_scale 2 faster than out_scale 4 (%.3f < %.3f ms)" % (m2, m4), m2 < m4)
for p in outs.values():
    p.free()
pin_in.free()
sr.close()

# ---- C: TTA ----
sr = context(True)
v = [("out_scale 4", at(sr, 4, x16)), ("out_scale 2", at(sr, 2, x16)), ("x4 + avg_pool2d(2)", detour(sr, 2, x16))]
med, spread = measure("C  C5 (TTA x8) device-resident, f16 -> f16", v)
gate("C5: out_scale 2 <= out_scale 4 + its spread (%.3f <= %.3f + %.3f ms)" % (med["out_scale 2"], med["out_scale 4"], spread),
     med["out_scale 2"] <= med["out_scale 4"] + spread)
gate("C5: out_scale 2 faster than x4 + avg_pool2d(2) (%.3f < %.3f ms)" % (med["out_scale 2"], med["x4 + avg_pool2d(2)"]),
     med["out_scale 2"] < med["x4 + avg_pool2d(2)"])
prof_lines += ["C5 f16 -> f16:"] + post_ms(sr, v[:2])
sr.close()

lines += ["", "D  profiled pass (rsr_get_profile), three frames per variant"] + prof_lines
text = "\n".join(lines)
print(text)
if out_path:
    with open(out_path, "w") as fh:
        fh.write(text + "\n")
