"""Frame sequences (rsr_diff_tiles_sequence, rsr_process_device_sequence, torch_io.upscale_sequence) on the C2 frame: 1920 x 1080 at tile
200, 60 tiles, device-resident, u8 -> u8.

    A  a window        8 frames with 1, 6 and 30 changed tiles per frame: ONE upscale_sequence call against the loop of 8
                       upscale_delta(out=...) calls on the same frames, into the same 8 distinct outputs.  Wall time of the whole window, the
                       host waits included (they are part of what is compared).
                       gate: the sequence is faster than the loop by more than the loop's own spread at 1 and at 6 tiles per frame, and
                       at 30 not slower by more than that spread
    B  propagate_rects the copy launch alone -- a sequence call with n = 1 and no tile set: all 60 rectangles of the x4 frame, from a
                       previous output elsewhere -- against torch's whole-frame copy_ of the same bytes (HIP events): 10 calls back to
                       back, and the launch by itself (the engine's profile brackets it with events; copy_ bracketed the same way)
                       gate: the launch alone within that copy's spread
    C  the diff        rsr_diff_tiles_sequence of 8 pairs against 8 rsr_diff_tiles calls (HIP events); reported

All variants of a section alternate inside every repetition; medians over the repetitions after a warm-up; spread = max - min.  Every
gate is stated on its own line with the numbers that decide it.  (profiles/sequence.txt carries two more sections that this tool does
not write, each with its command: D, bench.py of the parent commit against this one, and E, the compiler's resource report of the two new
kernels.)
    python tools/sequence_perf.py [reps=5] [out=profiles/sequence.txt] [append=0]
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

reps, out_path, append = 5, None, 0
for kv in sys.argv[1:]:
    k, v = kv.split("=")
    if k == "reps":
        reps = int(v)
    elif k == "out":
        out_path = v
    elif k == "append":
        append = int(v)

W, H, TILE, NF = 1920, 1080, 200, 8
CAP_MB = 7700  # 30 slots of a 210 x 210 tile at 6048 B per pixel are 7631 MiB
U8 = R.RSR_FMT_U8_HWC
d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K", 42)
st = torch.cuda.Stream()
lines = ["rsr_process_device_sequence / rsr_diff_tiles_sequence: 1920 x 1080 frames at tile 200 (60 tiles), windows of %d frames, medians of %d "
         "repetitions, alternating, after a warm-up" % (NF, reps), "device: %s" % torch.cuda.get_device_name(0)]
sr = R.RealSR(0)
sr.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
sr.tilesize = TILE
nx, ny = sr.tile_count(W, H)
NT = nx * ny
base = torch.from_numpy(synth.make_image(1235, W, H)).cuda()
order = np.random.default_rng(7).permutation(NT)  # which tiles change: the first k of one shuffle


def video(k):
    """NF + 1 frames; every frame differs from the one before in the centre pixel of k tiles (far from every halo: one tile each)."""
    frames = [base]
    for j in range(NF):
        f = frames[-1].clone()
        for t in order[:k]:
            yi, xi = divmod(int(t), nx)
            cy, cx = min(yi * TILE + TILE // 2, H - 1 - 20), min(xi * TILE + TILE // 2, W - 1 - 20)
            f[cy, cx, 0] += 1 + j
        frames.append(f)
    return frames


def stats(t):
    return float(np.median(t)), min(t), max(t)


def gate(text, met):
    lines.append("gate: %-100s %s" % (text, "met" if met else "NOT MET"))


# ---- A: one window against the loop of masked frames ----
lines += ["", "A  a window of %d frames into %d distinct outputs, prev_x / prev_y given: upscale_sequence against the loop of upscale_delta(out=...)" % (NF, NF),
          "%-26s %10s %9s %9s %9s   %s" % ("variant", "median ms", "min ms", "max ms", "spread", "per repetition (ms per window)")]
outs_a = [torch.empty((4 * H, 4 * W, 3), dtype=torch.uint8, device="cuda") for _ in range(NF)]
outs_b = [torch.empty((4 * H, 4 * W, 3), dtype=torch.uint8, device="cuda") for _ in range(NF)]
with torch.cuda.stream(st):
    y0 = torch_io.upscale(sr, base)
    st.synchronize()
    for k in (1, 6, 30):
        frames = video(k)
        st.synchronize()

        def loop():
            py, n = y0, 0
            for j in range(NF):
                py, m = torch_io.upscale_delta(sr, frames[j + 1], frames[j], py, out=outs_a[j])
                n += m
            return n

        def window():
            return torch_io.upscale_sequence(sr, frames[1:], prev_x=frames[0], prev_y=y0, out=outs_b)[1]

        def window_capped():  # (not gated: the same window cut into tile batches no larger than the loop's, by the workspace budget)
            sr.set_option("max_workspace_mb", CAP_MB)
            try:
                return window()
            finally:
                sr.set_option("max_workspace_mb", 65536)

        variants = (("loop", loop), ("sequence", window)) + ((("capped", window_capped),) if k == 30 else ())
        times = {name: [] for name, _ in variants}
        for rep in range(reps + 1):  # (the first round is the warm-up)
            for name, f in variants:
                st.synchronize()
                t0 = time.perf_counter()
                n = f()
                st.synchronize()
                if rep:
                    times[name].append((time.perf_counter() - t0) * 1e3)
                assert n == NF * k, (name, n)
        same = all(torch.equal(a, b) for a, b in zip(outs_a, outs_b))
        (lm, l0, l1), (sm, s0, s1) = stats(times["loop"]), stats(times["sequence"])
        for key, name, (m, lo, hi) in (("loop", "8 upscale_delta", (lm, l0, l1)), ("sequence", "upscale_sequence", (sm, s0, s1))):
            lines.append("%2d tiles  %-16s %10.3f %9.3f %9.3f %9.3f   %s" % (k, name, m, lo, hi, hi - lo, " ".join("%.3f" % v for v in times[key])))
        if k == 30:
            m, lo, hi = stats(times["capped"])
            lines.append("%2d tiles  %-16s %10.3f %9.3f %9.3f %9.3f   %s   (not gated: max_workspace_mb %d, batches of <= 30 tiles)"
                         % (k, "sequence, capped", m, lo, hi, hi - lo, " ".join("%.3f" % v for v in times["capped"]), CAP_MB))
        lines.append("%2d tiles  the window costs %.3f ms less than the loop (%.1f %%); the 8 outputs of both are bit-identical: %s" % (k, lm - sm, (1 - sm / lm) * 100, same))
        if k < 30:
            gate("%d tiles per frame: loop - sequence = %.3f ms > spread of the loop %.3f ms" % (k, lm - sm, l1 - l0), lm - sm > l1 - l0 and same)
        else:
            gate("%d tiles per frame: sequence - loop = %.3f ms <= spread of the loop %.3f ms" % (k, sm - lm, l1 - l0), sm - lm <= l1 - l0 and same)


def timed(variants, n_calls):
    """HIP events on the stream around n_calls calls; ms per call, per repetition; the first round is the warm-up."""
    times = {n: [] for n, _ in variants}
    with torch.cuda.stream(st):
        for rep in range(reps + 1):
            for n, f in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(n_calls):
                    f()
                e1.record(st)
                e1.synchronize()
                if rep:
                    times[n].append(e0.elapsed_time(e1) / n_calls)
    return times


# ---- B: the copy launch alone ----
nbytes = 16 * W * H * 3
prev = torch.randint(0, 256, (4 * H, 4 * W, 3), dtype=torch.uint8, device="cuda")
dst = torch.empty_like(prev)
zero = np.zeros(NT, dtype=np.uint8)
copied0 = sr.get_stat("seq_tiles_copied")


def propagate():
    sr.process_device_sequence([base.data_ptr()], U8, W, H, 3, [dst.data_ptr()], U8, zero, prev_out=prev.data_ptr(), stream=st.cuda_stream)


def torch_copy():
    dst.copy_(prev)


t = timed([("torch copy_", torch_copy), ("propagate_rects", propagate)], 10)
copied_per_call = int(sr.get_stat("seq_tiles_copied") - copied0) // ((reps + 1) * 10)
with torch.cuda.stream(st):
    dst.zero_()
    propagate()
    st.synchronize()
    same = torch.equal(dst, prev)
# the launch by itself: the engine's profile brackets it with HIP events (post_ms), torch's copy_ bracketed the same way, one call at a time
t1 = timed([("torch copy_", torch_copy)], 1)["torch copy_"]
sr.set_profiling(True)
alone = []
with torch.cuda.stream(st):
    propagate()
    sr.get_profile(reset=True)
    for _ in range(reps):
        propagate()
        alone.append(sr.get_profile(reset=True)["post_ms"])
sr.set_profiling(False)
(cm, c0, c1), (pm, p0, p1) = stats(t["torch copy_"]), stats(t["propagate_rects"])
lines += ["", "B  propagate_rects alone: the %d rectangles of the x4 frame (%.1f MB) from a previous output elsewhere, against torch's copy_ of the frame, 10 calls per repetition" % (NT, nbytes / 1e6),
          "%-18s %10s %9s %9s %9s %9s   %s" % ("variant", "median us", "min us", "max us", "spread", "GB/s", "per repetition (us per call)")]
for name, (m, lo, hi) in (("torch copy_", (cm, c0, c1)), ("propagate_rects", (pm, p0, p1))):
    lines.append("%-18s %10.1f %9.1f %9.1f %9.1f %9.1f   %s" % (name, m * 1e3, lo * 1e3, hi * 1e3, (hi - lo) * 1e3, 2 * nbytes / (m * 1e-3) / 1e9, " ".join("%.1f" % (v * 1e3) for v in t[name])))
lines.append("(GB/s: the frame read once and written once; the sequence call's time includes its 2.4 KB table upload; %d tiles copied per call by stat "
             "\"seq_tiles_copied\"; output equal to the source: %s)" % (copied_per_call, same))
(am, a0, a1), (bm, b0, b1) = stats(alone), stats(t1)
lines.append("one call between two events:  torch copy_ median %.1f us (%.1f .. %.1f; %.1f GB/s)   propagate_rects, the launch alone (profile post_ms) median %.1f us "
             "(%.1f .. %.1f; %.1f GB/s)" % (bm * 1e3, b0 * 1e3, b1 * 1e3, 2 * nbytes / (bm * 1e-3) / 1e9, am * 1e3, a0 * 1e3, a1 * 1e3, 2 * nbytes / (am * 1e-3) / 1e9))
lines.append("(10 calls back to back take %.1f us each where the launch alone takes %.1f: the rest is the call -- its checks, the table's asynchronous copy in front of "
             "the launch, the events that guard the table buffer and order the streams; a window pays it once)" % (pm * 1e3, am * 1e3))
gate("the launch alone, one at a time: propagate_rects - copy_ = %.1f us <= spread of copy_ %.1f us" % ((am - bm) * 1e3, (b1 - b0) * 1e3), am - bm <= b1 - b0 and same)

# ---- C: the diff of 8 pairs ----
frames = video(6)
ptrs = [f.data_ptr() for f in frames]
d_seq = torch.empty(NF * NT, dtype=torch.uint8, device="cuda")
d_one = torch.empty(NF * NT, dtype=torch.uint8, device="cuda")


def diff_seq():
    sr.diff_tiles_sequence(ptrs[1:], ptrs[0], U8, W, H, 3, d_seq.data_ptr(), stream=st.cuda_stream)


def diff_loop():
    for j in range(NF):
        sr.diff_tiles(ptrs[j], ptrs[j + 1], U8, W, H, 3, d_one.data_ptr() + j * NT, stream=st.cuda_stream)


t = timed([("8 rsr_diff_tiles", diff_loop), ("diff_tiles_sequence", diff_seq)], 10)
st.synchronize()
same = torch.equal(d_seq, d_one)
lines += ["", "C  the masks of 8 pairs of U8 frames (6 tiles differ per pair): ONE rsr_diff_tiles_sequence against 8 rsr_diff_tiles calls, 10 windows per repetition",
          "%-20s %10s %9s %9s %9s   %s" % ("variant", "median us", "min us", "max us", "GB/s", "per repetition (us per window)")]
for name in ("8 rsr_diff_tiles", "diff_tiles_sequence"):
    m, lo, hi = stats(t[name])
    lines.append("%-20s %10.1f %9.1f %9.1f %9.1f   %s" % (name, m * 1e3, lo * 1e3, hi * 1e3, NF * 2 * W * H * 3 / (m * 1e-3) / 1e9, " ".join("%.1f" % (v * 1e3) for v in t[name])))
lines.append("(GB/s: both frames of every pair once; the masks of both variants are identical: %s, %d of %d bytes set)" % (same, int(d_seq.sum().item()), NF * NT))
sr.close()

text = "\n".join(lines)
print(text)
if out_path:
    with open(out_path, "a" if append else "w") as fh:
        fh.write(text + "\n")
