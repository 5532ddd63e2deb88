"""Model depth (rsr_load takes RRDBNet x4 graphs of 1 .. 64 blocks) measured on one board.

    A  6 blocks against 23: the C2 frame (1920 x 1080, tile 200), device-resident, u8 -> u8, synthetic models, two contexts in this
       process, alternating (HIP events on one torch stream, `frames` back-to-back frames per timing, medians over `reps` repetitions
       after a warm-up), each line with its own spread.  Next to the measured 6-block value a PREDICTION from one profiled 23-block frame
       (rsr_get_conv_times, rsr_get_profile): the time of its 345 trunk convolutions x 6 / 23, plus its six other convolutions, plus pre
       and post.  There is no gate on the ratio: the file records what it is.
    B  the default path: bench.py --gpus 1, parent commit against this commit, alternating, `rounds` times each: the same checksum, and
       this commit's median ms_per_step no further above the parent's than the parent's own spread over its runs.  Needs parent=DIR, a
       built checkout of the parent commit; without it B is reported as not measured.
    C  the compiler's resource report (hipcc -Rpass-analysis=kernel-resource-usage) of conv_flow.hip and kernels.hip: registers, scratch
       and occupancy per kernel, and -- with parent=DIR -- whether any differs from the parent's.  Needs no GPU: resources=only does
       nothing else, and append=FILE puts a report made that way behind A and B.

    python tools/depth_perf.py [reps=5] [frames=4] [rounds=3] [steps=10] [warmup=3] [parent=DIR] [resources=0|1|only] [append=FILE] [out=profiles/depth.txt]
"""
import json
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = dict(kv.split("=", 1) for kv in sys.argv[1:])
reps, frames, rounds = int(args.get("reps", 5)), int(args.get("frames", 4)), int(args.get("rounds", 3))
steps, warmup = int(args.get("steps", 10)), int(args.get("warmup", 3))
parent, out_path, resources = args.get("parent"), args.get("out"), args.get("resources", "0")
parent = os.path.abspath(parent) if parent else None
lines, gates = [], []


def gate(text, ok):
    gates.append("gate: %-110s %s" % (text, "met" if ok else "MISSED"))


def emit():
    """Print what has been measured so far and keep it in `out`: a later section that fails loses nothing."""
    text = "\n".join(lines + [""] + gates)
    print(text, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


# ---- C: the compiler's resource report ------------------------------------------------------------------------------------------------
def resource_report(root):
    """{kernel: (VGPRs, AGPRs, SGPRs, scratch bytes / lane, occupancy, LDS bytes, spilled VGPRs, spilled SGPRs)} of the two kernel files of the tree `root`."""
    csrc = os.path.join(root, "realsr-ncnn-vulkan_amd", "csrc")
    gen = os.path.join(csrc, "..", "lib", "obj", "gen")
    if not os.path.exists(os.path.join(gen, "conv_flow_hooks.inc")):
        os.makedirs(gen, exist_ok=True)
        subprocess.check_call([sys.executable, os.path.join(root, "tools", "gen_flow_hooks.py"), gen], stdout=subprocess.DEVNULL)
    got = {}
    for src in ("conv_flow.hip", "kernels.hip"):
        r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-I", gen,
                            "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull], cwd=csrc, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc %s in %s: %s" % (src, csrc, r.stderr[-1500:]))
        name, cur = None, {}
        for ln in r.stderr.splitlines():
            m = re.search(r"remark: (?:Function Name: (\S+)|\s*([A-Za-z ]+?)(?: \[[^\]]+\])?: (\d+))", ln)
            if not m:
                continue
            if m.group(1):
                name, cur = src + ":" + m.group(1), {}
                got[name] = cur
            elif name:
                cur[m.group(2).strip()] = int(m.group(3))
    keys = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "Occupancy", "LDS Size", "VGPRs Spill", "SGPRs Spill")
    return {k: tuple(v.get(f, -1) for f in keys) for k, v in got.items()}


def section_c():
    this = resource_report(HERE)
    lines.extend(["", "C  hipcc -Rpass-analysis=kernel-resource-usage, gfx950, conv_flow.hip + kernels.hip: %d kernels" % len(this),
                  "   most VGPRs %d, most AGPRs %d, kernels with scratch %d, kernels that spill VGPRs %d, lowest occupancy %d waves / SIMD" % (
                      max(v[0] for v in this.values()), max(v[1] for v in this.values()), sum(v[3] > 0 for v in this.values()), sum(v[6] > 0 for v in this.values()),
                      min(v[4] for v in this.values()))])
    assert all(min(v) >= 0 for v in this.values()), "a field of the compiler's report was not found"
    if not parent:
        lines.append("   against the parent commit: not compared (no parent=DIR)")
        return
    old = resource_report(parent)
    diff = sorted(k for k in set(this) | set(old) if this.get(k) != old.get(k))
    lines.append("   against the parent commit (%d kernels): %s" % (len(old), "every kernel has the same VGPRs, AGPRs, SGPRs, scratch, occupancy, LDS and spills" if not diff
                                                                   else "%d kernels DIFFER (VGPRs, AGPRs, SGPRs, scratch, occupancy, LDS, VGPR spills, SGPR spills):" % len(diff)))
    for k in diff:
        lines.append("     %s: parent %s, this %s" % (k, old.get(k), this.get(k)))
    same_src = all(open(os.path.join(r, "realsr-ncnn-vulkan_amd", "csrc", f), "rb").read() == open(os.path.join(HERE, "realsr-ncnn-vulkan_amd", "csrc", f), "rb").read()
                   for r in (parent,) for f in ("conv_flow.hip", "kernels.hip", "kernels.h"))
    lines.append("   conv_flow.hip, kernels.hip, kernels.h byte for byte the parent's: %s" % ("yes" if same_src else "NO"))
    gate("C no kernel changed registers, scratch, occupancy or LDS against the parent", not diff)


if resources == "only":
    lines.append("command: python tools/depth_perf.py " + " ".join(sys.argv[1:]))
    section_c()
    emit()
    sys.exit(0)

sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import realsr_ncnn_vulkan_amd as R  # noqa: E402
from realsr_ncnn_vulkan_amd import synth, torch_io  # noqa: E402

st = torch.cuda.Stream()
W_IN, H_IN, TILE = 1920, 1080, 200
lines.extend(["model depth: 6 blocks against 23.  %d repetitions x %d frames per depth, alternating, HIP events on one stream; B: %d runs per commit" % (reps, frames, rounds),
              "device: %s" % torch.cuda.get_device_name(0), "command: python tools/depth_perf.py " + " ".join(sys.argv[1:])])


def context(nb):
    d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K", 42, nb=nb)
    sr = R.RealSR(0)
    sr.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
    sr.tilesize = TILE
    assert sr.num_blocks == nb and sr.num_convs == 15 * nb + 6
    return sr


def row(name, t, extra=""):
    return "%-34s %9.2f %9.2f %9.2f %9.2f   %s%s" % (name, np.median(t), min(t), max(t), max(t) - min(t), " ".join("%.2f" % v for v in t), extra)


# ---- A: 6 blocks against 23 -------------------------------------------------------------------------------------------------------
srs = {nb: context(nb) for nb in (6, 23)}
x8 = torch.from_numpy(synth.make_image(1235, W_IN, H_IN)).cuda()
times = {nb: [] for nb in srs}
with torch.cuda.stream(st):
    for nb, sr in srs.items():  # warm-up: plans, workspace
        torch_io.upscale(sr, x8)
        torch_io.upscale(sr, x8)
    st.synchronize()
    for rep in range(reps):
        for nb, sr in srs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(frames):
                y = torch_io.upscale(sr, x8)
            e1.record(st)
            e1.synchronize()
            del y
            times[nb].append(e0.elapsed_time(e1) / frames)
    # one profiled frame per depth (events around every launch: a little slower than the frames above)
    prof = {}
    for nb, sr in srs.items():
        sr.set_profiling(True)
        torch_io.upscale(sr, x8)
        st.synchronize()
        sr.get_profile(reset=True)
        sr.get_conv_times(reset=True)
        torch_io.upscale(sr, x8)
        st.synchronize()
        prof[nb] = (sr.get_profile(reset=True), sr.get_conv_times(reset=True))
        sr.set_profiling(False)
for sr in srs.values():
    sr.close()
p23, t23 = prof[23]
p6, t6 = prof[6]
assert len(t23) == 351 and len(t6) == 96
trunk23, other23, prepost23 = float(t23[1:346].sum()), float(t23[0] + t23[346:].sum()), p23["pre_ms"] + p23["post_ms"]
predicted = trunk23 * 6 / 23 + other23 + prepost23
m6, m23 = float(np.median(times[6])), float(np.median(times[23]))
lines.extend(["", "A  C2 frame %d x %d -> %d x %d, tile %d, device-resident, u8 -> u8, synthetic models (seed 42)" % (W_IN, H_IN, 4 * W_IN, 4 * H_IN, TILE),
              "%-34s %9s %9s %9s %9s   %s" % ("depth", "median ms", "min ms", "max ms", "spread", "per repetition (ms per frame)"),
              row("6 blocks, 96 convolutions", times[6]), row("23 blocks, 351 convolutions", times[23]),
              "measured 6 / 23 = %.3f (6 / 23 of the blocks = %.3f); %.2f against %.2f Mpix/s of output" % (m6 / m23, 6 / 23, 16 * W_IN * H_IN / m6 / 1e3, 16 * W_IN * H_IN / m23 / 1e3),
              "one profiled 23-block frame: 345 trunk convolutions %.3f ms, the six others %.3f ms, pre + post %.3f ms (total %.3f ms between first and last launch)" % (
                  trunk23, other23, prepost23, p23["total_ms"]),
              "one profiled 6-block frame:   90 trunk convolutions %.3f ms, the six others %.3f ms, pre + post %.3f ms (total %.3f ms)" % (
                  float(t6[1:91].sum()), float(t6[0] + t6[91:].sum()), p6["pre_ms"] + p6["post_ms"], p6["total_ms"]),
              "6 blocks predicted from the 23-block profile: %.3f x 6 / 23 + %.3f + %.3f = %.2f ms; measured %.2f ms (%.1f %% of the prediction; no gate)" % (
                  trunk23, other23, prepost23, predicted, m6, 100 * m6 / predicted)])
del srs, x8
torch.cuda.empty_cache()
emit()


# ---- B: bench.py against the parent commit, child processes alternating ---------------------------------------------------------------
def child(root, cmd):
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("%s in %s failed (%d): %s" % (" ".join(cmd), root, r.returncode, r.stderr[-2000:]))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


if not parent:
    lines.extend(["", "B  bench.py against the parent commit: not measured (no parent=DIR)"])
else:
    trees = [("parent", parent), ("this", HERE)]
    bench = {k: [] for k, _ in trees}
    for rnd in range(rounds):
        for k, root in trees:
            bench[k].append(child(root, [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]))
    ms = {k: [r["ms_per_step"] for r in bench[k]] for k in bench}
    sums = {k: sorted(set(r["config"]["checksum"] for r in bench[k])) for k in bench}
    spread = max(ms["parent"]) - min(ms["parent"])
    lines.extend(["", "B  bench.py --gpus 1 --steps %d --warmup %d: %d runs per commit, alternating (the 23-block default model)" % (steps, warmup, rounds),
                  "%-34s %9s %9s %9s %9s   %s" % ("commit", "median ms", "min ms", "max ms", "spread", "ms_per_step per run")])
    for k in ("parent", "this"):
        lines.append(row(k, ms[k], "   checksum %s, value %s Mpix/s" % (sums[k], " ".join("%.2f" % r["value"] for r in bench[k]))))
    gate("B the same checksum (%s)" % sums["this"], sums["this"] == sums["parent"] and len(sums["this"]) == 1)
    gate("B ms_per_step median no further above the parent's than the parent's spread (%.3f <= %.3f + %.3f ms)" % (np.median(ms["this"]), np.median(ms["parent"]), spread),
         np.median(ms["this"]) <= np.median(ms["parent"]) + spread)
emit()

if resources == "1":
    section_c()
if args.get("append"):
    lines.extend([""] + open(args["append"]).read().rstrip("\n").splitlines())
emit()
