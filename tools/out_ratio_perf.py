"""Rational output scales (rsr_set_out_ratio: x3/2, x9/4, x3, x4/3, area-averaged on the device) against out_scale 4 and 2 of the same run
and against the detour a user had to take before (x4 out of the library, then torch.nn.functional.interpolate(mode="area") to the same
size -- a timing comparator only: its arithmetic differs):

    A  C2 device-resident   1920 x 1080, u8 -> u8 and f16 -> f16: ratios 3/2, 9/4, 3/1 at tile 200, 4/3 at tile 201 (x4 and x2 at that tile)
    B  C2 host -> host      the same frame from and into pinned buffers (rsr_process) at out_scale 4 and ratio 3/2
    C  C5 (TTA)             f16 -> f16 at out_scale 4 and ratio 3/2, and the detour
    D  post_ms              of rsr_get_profile per ratio, plain (C2) and TTA (C5), from a separate profiled pass

All variants of a section alternate inside every repetition, on ONE torch stream (B: wall clock around the synchronous call); a
repetition of a variant is 4 frames back to back, its time the mean per frame; medians over the repetitions after a warm-up.
Gates, per ratio: the native median is not above the detour's; and it is not above the same run's out_scale 4 median by more than that
run's own spread (max - min of out_scale 4) plus the difference of the two post_ms -- the network work is identical.
    python tools/out_ratio_perf.py [reps=5] [frames=4] [out=profiles/out_ratio.txt] [append=0]
"""
import os
import sys
import time
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import realsr_ncnn_vulkan_amd as R  # noqa: E402
from realsr_ncnn_vulkan_amd import synth, torch_io  # noqa: E402

reps, frames, out_path, append = 5, 4, None, 0
for kv in sys.argv[1:]:
    k, v = kv.split("=")
    if k == "reps":
        reps = int(v)
    elif k == "frames":
        frames = int(v)
    elif k == "out":
        out_path = v
    elif k == "append":
        append = int(v)

W, H = 1920, 1080
d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K", 42)
st = torch.cuda.Stream()
lines = ["rsr_set_out_ratio: 1920 x 1080 frame, %d repetitions of %d frames per variant, alternating, after a warm-up" % (reps, frames),
         "device: %s" % torch.cuda.get_device_name(0)]
frame8 = synth.make_image(1235, W, H)
x8 = torch.from_numpy(frame8).cuda()
x16 = torch.from_numpy(np.ascontiguousarray((frame8.astype(np.float32) * np.float32(1 / 255.0)).transpose(2, 0, 1))).cuda().half()


def context(tta):
    sr = R.RealSR(0, tta_mode=tta)
    sr.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
    return sr


def name_of(r):
    r = Fraction(r)
    return "out_scale %d" % r if r in (1, 2, 4) else "ratio %d/%d" % (r.numerator, r.denominator)


def at(sr, ratio, x):
    def f():
        sr.out_ratio = ratio
        return torch_io.upscale(sr, x)
    return f


def detour(sr, ratio, x):
    """What a user does today: the x4 image out of the library, then a resampling pass over it."""
    def f():
        sr.out_ratio = 4
        y = torch_io.upscale(sr, x)
        if y.dtype == torch.uint8:  # (no uint8 kernel: HWC bytes -> planar float -> area -> bytes)
            size = (x.shape[0] * ratio.numerator // ratio.denominator, x.shape[1] * ratio.numerator // ratio.denominator)
            p = torch.nn.functional.interpolate(y.permute(2, 0, 1).float()[None], size=size, mode="area")[0]
            return (p + 0.5).floor().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()
        size = (x.shape[-2] * ratio.numerator // ratio.denominator, x.shape[-1] * ratio.numerator // ratio.denominator)
        return torch.nn.functional.interpolate(y[None], size=size, mode="area")[0]
    return f


def table(title, times, base):
    lines.append("")
    lines.append(title)
    lines.append("%-26s %9s %9s %9s   %s" % ("variant", "median ms", "min ms", "max ms", "per repetition (ms per frame)"))
    bmed = float(np.median(times[base]))
    for n, t in times.items():
        lines.append("%-26s %9.3f %9.3f %9.3f   %s   (%+.2f %% vs %s)" % (n, np.median(t), min(t), max(t), " ".join("%.3f" % v for v in t),
                                                                          (np.median(t) / bmed - 1) * 100, base))
        if n.startswith("x4 + area"):
            lines.append("%-26s spread of the comparator over the repetitions: %.3f ms (max - min)" % ("", max(t) - min(t)))
    spread = max(times[base]) - min(times[base])
    lines.append("spread of %s over the repetitions: %.3f ms (max - min)" % (base, spread))
    return spread


def measure(title, variants):
    """variants: [(name, f)], the first is out_scale 4; HIP events on one stream around `frames` calls."""
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
                for _ in range(frames):
                    y = f()
                e1.record(st)
                e1.synchronize()
                del y
                times[n].append(e0.elapsed_time(e1) / frames)
    st.synchronize()
    spread = table(title, times, variants[0][0])
    return {n: float(np.median(t)) for n, t in times.items()}, spread


def gate(what, ok):
    lines.append("gate: %-100s %s" % (what, "met" if ok else "MISSED"))


def post_ms(sr, variants):
    """A separate profiled pass: the post-processing launches' share (rsr_get_profile; profiling turns merging off and adds events)."""
    out = {}
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
            out[n] = p["post_ms"] / 3
            lines.append("%-26s post %.3f ms, pre %.3f ms, conv %.3f ms, total %.3f ms per frame" % (n, p["post_ms"] / 3, p["pre_ms"] / 3, p["conv_ms"] / 3, p["total_ms"] / 3))
    finally:
        sr.set_profiling(False)
    return out


def section(sr, title, x, tile, ratios, with_2=True):
    """One alternating run at one tile size: out_scale 4 [, 2], the ratios and their detours; then the profiled pass and the gates."""
    sr.tilesize = tile
    v = [(name_of(4), at(sr, 4, x))] + ([(name_of(2), at(sr, 2, x))] if with_2 else [])
    for r in ratios:
        v += [(name_of(r), at(sr, r, x)), ("x4 + area -> %d/%d" % (r.numerator, r.denominator), detour(sr, r, x))]
    med, spread = measure("%s, tile %d" % (title, tile), v)
    lines.append("profiled pass (rsr_get_profile), three frames per variant:")
    post = post_ms(sr, [(n, f) for n, f in v if not n.startswith("x4 + area")])
    for r in ratios:
        n, dn = name_of(r), "x4 + area -> %d/%d" % (r.numerator, r.denominator)
        gate("%s: %s <= the detour (%.3f <= %.3f ms)" % (title, n, med[n], med[dn]), med[n] <= med[dn])
        margin = spread + (post[n] - post[name_of(4)])
        gate("%s: %s <= out_scale 4 + its spread + the post_ms difference (%.3f <= %.3f + %.3f + %.3f ms)" % (
            title, n, med[n], med[name_of(4)], spread, post[n] - post[name_of(4)]), med[n] <= med[name_of(4)] + margin)
    return {r: post[name_of(r)] - post[name_of(4)] for r in ratios}


sr = context(False)
for name, x in (("u8 -> u8", x8), ("f16 -> f16", x16)):
    diff = section(sr, "A  C2 device-resident, %s" % name, x, 200, [Fraction(3, 2), Fraction(9, 4), Fraction(3, 1)])
    if x is x8:
        POST_DIFF_32 = diff[Fraction(3, 2)]  # (section B runs the same u8 -> u8 frame through the host entry point)
    section(sr, "A  C2 device-resident, %s" % name, x, 201, [Fraction(4, 3)])

# ---- B: host -> host from pinned buffers ----
sr.tilesize = 200
pin_in = R.PinnedArray(frame8.shape)
pin_in.array[:] = frame8
outs = {4: R.PinnedArray((H * 4, W * 4, 3)), Fraction(3, 2): R.PinnedArray((H * 3 // 2, W * 3 // 2, 3))}
times = {name_of(r): [] for r in outs}
for rep in range(reps + 1):
    for r in outs:
        sr.out_ratio = r
        t0 = time.perf_counter()
        for _ in range(frames):
            sr.process(pin_in.array, out=outs[r].array)
        if rep:
            times[name_of(r)].append((time.perf_counter() - t0) * 1e3 / frames)
table("B  C2 host -> host, pinned buffers (rsr_process, wall clock)", times, name_of(4))
m4, m32 = float(np.median(times[name_of(4)])), float(np.median(times[name_of(Fraction(3, 2))]))
hspread = max(times[name_of(4)]) - min(times[name_of(4)])
# (at x4 the download of the first output rows runs under the second half of the network -- the split tail, which needs conv_last to
#  write the image itself --, so moving 14 % of the bytes does not have to make 3/2 faster: the gate is the one of section A)
gate("C2 host -> host: ratio 3/2 <= out_scale 4 + its spread + the post_ms difference (%.3f <= %.3f + %.3f + %.3f ms)" % (m32, m4, hspread, POST_DIFF_32),
     m32 <= m4 + hspread + POST_DIFF_32)
for p in outs.values():
    p.free()
pin_in.free()
sr.close()

# ---- C: TTA ----
sr = context(True)
section(sr, "C  C5 (TTA x8) device-resident, f16 -> f16", x16, 200, [Fraction(3, 2)], with_2=False)
sr.close()

text = "\n".join(lines)
print(text)
if out_path:
    with open(out_path, "a" if append else "w") as fh:
        fh.write(text + "\n")
