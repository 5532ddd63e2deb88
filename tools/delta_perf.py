"""Masked tile processing and the device frame diff (rsr_process_device_masked, rsr_diff_tiles) on the C2 frame: 1920 x 1080 at tile 200,
60 tiles, device-resident, u8 -> u8.

    A  masked call      0, 1, 6, 15, 30 and 60 tiles set, against the plain rsr_process_device_fmt frame of the same run: time per frame,
                        time per run tile, and the tile count at which a masked call stops being cheaper than the plain frame
    B  tables           host time spent building and uploading the tile tables of a masked call (stat "masked_table_us"), and the host
                        time of the whole call
    C  rsr_diff_tiles   U8, NV12 and F32 frames: time and effective GB/s (both frames read once); beside it pre_ms / pre_bytes of a
                        profiled plain frame of the same run: the rate an existing image-reading launch reaches on this board

All variants of a section alternate inside every repetition, on ONE torch stream; a repetition of a variant is `frames` calls back to
back, its time the mean per call (HIP events); medians over the repetitions after a warm-up.  Nothing here is a gate: the numbers are
reported.  (profiles/delta.txt carries two more sections that this tool does not write, each with its command: D, bench.py of the parent
commit against this one, and E, the compiler's resource report of the diff kernel.)
    python tools/delta_perf.py [reps=5] [frames=4] [out=profiles/delta.txt] [append=0]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import realsr_ncnn_vulkan_amd as R  # noqa: E402
from realsr_ncnn_vulkan_amd import synth  # noqa: E402

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

W, H, TILE = 1920, 1080, 200
U8, F32, NV12 = R.RSR_FMT_U8_HWC, R.RSR_FMT_F32_CHW, R.RSR_FMT_NV12
d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K", 42)
st = torch.cuda.Stream()
lines = ["rsr_process_device_masked / rsr_diff_tiles: 1920 x 1080 frame at tile 200 (60 tiles), %d repetitions of %d calls per variant, "
         "alternating, after a warm-up" % (reps, frames), "device: %s" % torch.cuda.get_device_name(0)]
sr = R.RealSR(0)
sr.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
sr.tilesize = TILE
nx, ny = sr.tile_count(W, H)
NT = nx * ny
frame8 = synth.make_image(1235, W, H)
x8 = torch.from_numpy(frame8).cuda()
y8 = torch.empty((4 * H, 4 * W, 3), dtype=torch.uint8, device="cuda")
order = np.random.default_rng(7).permutation(NT)  # which tiles a mask of k tiles sets: the first k of one shuffle


def mask_of(k):
    m = np.zeros(NT, dtype=np.uint8)
    m[order[:k]] = 1
    return m


def plain():
    sr.process_device_fmt(x8.data_ptr(), U8, W, H, 3, y8.data_ptr(), U8, stream=st.cuda_stream)


def masked(m):
    return lambda: sr.process_device_masked(x8.data_ptr(), U8, W, H, 3, y8.data_ptr(), U8, m, stream=st.cuda_stream)


def measure(variants, n_calls):
    """variants: [(name, f)]; HIP events on the stream around n_calls calls; ms per call, per repetition."""
    times = {n: [] for n, _ in variants}
    with torch.cuda.stream(st):
        for _ in range(2):
            for _, f in variants:
                f()
        st.synchronize()
        for _ in range(reps):
            for n, f in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(n_calls):
                    f()
                e1.record(st)
                e1.synchronize()
                times[n].append(e0.elapsed_time(e1) / n_calls)
    return times


# ---- A: the masked call against the plain frame ----
KS = [0, 1, 6, 15, 30, 60]
variants = [("plain frame", plain)] + [("masked, %2d tiles" % k, masked(mask_of(k))) for k in KS]
times = measure(variants, frames)
pm = float(np.median(times["plain frame"]))
lines += ["", "A  masked call against the plain rsr_process_device_fmt frame (u8 -> u8)",
          "%-18s %9s %9s %9s %12s   %s" % ("variant", "median ms", "min ms", "max ms", "ms per tile", "per repetition (ms per call)")]
med = {}
for (n, _), k in zip(variants, [None] + KS):
    t = times[n]
    med[k] = float(np.median(t))
    per = "%12.3f" % (med[k] / k) if k else "%12s" % "-"
    lines.append("%-18s %9.3f %9.3f %9.3f %s   %s   (%+.1f %% vs the plain frame)" % (n, med[k], min(t), max(t), per, " ".join("%.3f" % v for v in t),
                                                                                     (med[k] / pm - 1) * 100))
lines.append("spread of the plain frame over the repetitions: %.3f ms (max - min)" % (max(times["plain frame"]) - min(times["plain frame"])))
ks = np.array([k for k in KS if 0 < k < NT], dtype=np.float64)
slope, icpt = np.polyfit(ks, np.array([med[int(k)] for k in ks]), 1)
lines.append("partial masks, least squares over %s tiles: %.3f ms + %.3f ms per tile" % (", ".join("%d" % k for k in ks), icpt, slope))
cross = (pm - icpt) / slope  # tiles at which the line reaches the plain frame
if cross >= NT:
    lines.append("a masked call stops being cheaper than the plain frame (%.3f ms): never for a partial mask, by this fit (the line reaches it at "
                 "%.1f tiles, the frame has %d); with every tile set it IS the plain call (%.3f ms)" % (pm, cross, NT, med[NT]))
else:
    lines.append("a masked call stops being cheaper than the plain frame (%.3f ms) from %d of %d tiles on, by this fit; with every tile set it IS "
                 "the plain call (%.3f ms)" % (pm, int(np.ceil(cross)), NT, med[NT]))

# ---- B: host time of the tables ----
lines += ["", "B  host time of a masked call (the engine idle, the call asynchronous on the stream), mean of %d calls" % (reps * frames),
          "%-18s %14s %16s" % ("variant", "whole call us", "of it tables us")]
for k in [None] + KS:
    f = plain if k is None else masked(mask_of(k))
    tab0, wall = sr.get_stat("masked_table_us"), 0.0
    for _ in range(reps * frames):
        st.synchronize()
        t0 = time.perf_counter()
        f()
        wall += time.perf_counter() - t0
    st.synchronize()
    lines.append("%-18s %14.1f %16.1f" % ("plain frame" if k is None else "masked, %2d tiles" % k, wall * 1e6 / (reps * frames),
                                          (sr.get_stat("masked_table_us") - tab0) / (reps * frames)))
lines.append("(0 and 60 tiles build no tables: nothing is launched / the cached plan of the plain call runs)")

# ---- C: the diff ----
rng = np.random.default_rng(8)
lines += ["", "C  rsr_diff_tiles, two frames that differ in 3 samples, %d calls per repetition" % (5 * frames),
          "%-8s %10s %10s %10s %12s   %s" % ("format", "median us", "min us", "max us", "GB/s", "per repetition (us per call)")]
d_mask = torch.empty(NT, dtype=torch.uint8, device="cuda")
for name, fmt, nbytes in (("U8", U8, W * H * 3), ("NV12", NV12, W * H * 3 // 2), ("F32", F32, W * H * 12)):
    a = torch.from_numpy(rng.integers(0, 256, size=nbytes, dtype=np.uint8)).cuda()
    b = a.clone()
    b[::nbytes // 3] ^= 1
    t = measure([(name, lambda: sr.diff_tiles(a.data_ptr(), b.data_ptr(), fmt, W, H, 3, d_mask.data_ptr(), stream=st.cuda_stream))], 5 * frames)[name]
    m = float(np.median(t))
    lines.append("%-8s %10.1f %10.1f %10.1f %12.1f   %s   (%d of %d tiles marked)" % (name, m * 1e3, min(t) * 1e3, max(t) * 1e3, 2 * nbytes / (m * 1e-3) / 1e9,
                                                                                    " ".join("%.1f" % (v * 1e3) for v in t), int(d_mask.sum().item()), NT))
lines.append("(GB/s: both frames once, without the fifth that overlapping halos add)")
sr.set_profiling(True)
with torch.cuda.stream(st):
    plain()
    st.synchronize()
    sr.get_profile(reset=True)
    for _ in range(3):
        plain()
    st.synchronize()
p = sr.get_profile(reset=True)
sr.set_profiling(False)
lines.append("preproc_tiles of a profiled plain frame of this run: pre_ms %.3f for pre_bytes %.1f MB per frame = %.1f GB/s (one frame read, "
             "the network's input planes written)" % (p["pre_ms"] / 3, p["pre_bytes"] / 3 / 1e6, p["pre_bytes"] / (p["pre_ms"] * 1e-3) / 1e9))
sr.close()

text = "\n".join(lines)
print(text)
if out_path:
    with open(out_path, "a" if append else "w") as fh:
        fh.write(text + "\n")
