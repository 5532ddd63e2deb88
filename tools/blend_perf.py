"""Network interpolation (rsr_load_second / rsr_set_blend) at the default depth: what a change of strength costs, and that a blended
context runs as fast as one that loaded the blend.

Models: the synthetic models-DF2K (seed 42) and models-DF2K_JPEG (seed 43), 23 blocks, 33.5 MB packed each.  One board, everything alternating
inside every repetition, medians over the repetitions; a spread is max - min of one variant's repetitions.  Gates, each on its own line:
    (a) blend_blob against a device-to-device hipMemcpyAsync of one blob's bytes -- the copy is rsr_set_blend(1) itself: the same stream,
        the same two HIP events around the one launch / copy (stat "blend_us" under rsr_set_profiling).  The copy moves 2 bytes per blob
        byte, the blend 3:  blend <= 1.5 x the copy + the copy's own spread.
        Reported without a gate: the wall time of one rsr_set_blend call against rsr_load_packed of the host-blended blob.
    (b) the C2 frame (1920 x 1080 RGB, tile 200), u8 -> u8, device-resident, on a context after set_blend(0.4) against a context that loaded
        the exported blob: same kernels, same bytes.  |median blended - median loaded| <= the loaded context's spread.
    (c) with parent=<checkout of the parent commit, built>: bench.py, parent against this tree as alternating child processes x 3, same
        checksum; this median <= the parent's median + the parent's spread.
With resources=<parent report>,<this report> (the compiler's -Rpass-analysis=kernel-resource-usage output for kernels.hip, made without a
GPU; tools/kernel_resources.py says how): the kernels whose registers, scratch or occupancy changed, and the new instantiations.
    python tools/blend_perf.py [reps=7] [frames=4] [parent=DIR] [resources=A,B] [bench_steps=10] [out=profiles/blend.txt]
    python tools/blend_perf.py resources=A,B gpu=0     (the resource report alone)
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

reps, frames, out_path, parent, resources, bench_steps, use_gpu = 7, 4, None, None, None, 10, True
for kv in sys.argv[1:]:
    k, v = kv.split("=", 1)
    if k == "reps":
        reps = int(v)
    elif k == "frames":
        frames = int(v)
    elif k == "out":
        out_path = v
    elif k == "parent":
        parent = os.path.abspath(v)
    elif k == "resources":
        resources = v.split(",")
    elif k == "bench_steps":
        bench_steps = int(v)
    elif k == "gpu":
        use_gpu = v != "0"

W, H, T = 1920, 1080, 200
STRENGTH = 0.4


def spread(t):
    return max(t) - min(t)


lines = ["Network interpolation: rsr_load_second / rsr_set_blend (tools/blend_perf.py; python tools/blend_perf.py out=profiles/blend.txt)",
         "Every gate is printed on its own line; nothing was fixed in advance.", ""]

if use_gpu:
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import realsr_ncnn_vulkan_amd as R
    from realsr_ncnn_vulkan_amd import synth, torch_io

    root = os.environ.get("RSR_MODELS", "/tmp/rsr_models")
    da, db = synth.make_model_dir(root, "models-DF2K", 42), synth.make_model_dir(root, "models-DF2K_JPEG", 43)
    pa, pb = (os.path.join(da, "x4.param"), os.path.join(da, "x4.bin")), (os.path.join(db, "x4.param"), os.path.join(db, "x4.bin"))
    t_f32 = float(np.float32(STRENGTH))

    sr = R.RealSR(0)
    sr.load(*pa)
    sr.load_second(*pb)
    sr.tilesize = T
    blob_a, blob_b = R.model_pack(*pa), R.model_pack(*pb)
    t0 = time.perf_counter()
    host_blend = np.frombuffer(R.model_blend(blob_a, blob_b, t_f32), dtype=np.uint8)
    host_blend_ms = (time.perf_counter() - t0) * 1e3
    sr.blend = t_f32
    exported = np.frombuffer(sr.export_model(), dtype=np.uint8)
    assert np.array_equal(exported, host_blend), "the device blend differs from rsr_model_blend"
    plain = R.RealSR(0)
    plain.load_packed(exported)
    plain.tilesize = T

    # ---- (a) the blend against the copy ------------------------------------------------------------------------------------------------
    sr.set_profiling(True)
    us = {"blend": [], "copy": []}
    wall = {"set_blend": [], "load_packed": []}
    for t in (t_f32, 1.0, t_f32, 1.0):   # warm-up
        sr.blend = t
    for rep in range(reps):
        for name, t in (("blend", t_f32), ("copy", 1.0)):
            inner = []
            for _ in range(5):
                sr.blend = t
                inner.append(sr.get_stat("blend_us"))
            assert min(inner) > 0
            us[name].append(float(np.median(inner)))
    sr.set_profiling(False)
    for rep in range(reps):
        t0 = time.perf_counter()
        sr.blend = t_f32
        wall["set_blend"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        plain.load_packed(host_blend)
        wall["load_packed"].append((time.perf_counter() - t0) * 1e3)
    sr.blend = t_f32
    nbytes = exported.size
    mb, mc, sc = float(np.median(us["blend"])), float(np.median(us["copy"])), spread(us["copy"])
    ok_a = mb <= 1.5 * mc + sc
    lines += ["device: %s" % torch.cuda.get_device_name(0),
              "(a) one change of strength at 23 blocks: a blob of %d bytes (%.1f MB), %d repetitions, each the median of 5 calls, blend and copy alternating;" % (nbytes, nbytes / 1e6, reps),
              "    HIP events around the one launch / copy on the context's stream (stat \"blend_us\")",
              "%-34s %10s %9s %9s   %s" % ("variant", "median us", "min us", "max us", "per repetition"),
              "%-34s %10.1f %9.1f %9.1f   %s" % ("blend_blob (t = 0.4)", mb, min(us["blend"]), max(us["blend"]), " ".join("%.1f" % v for v in us["blend"])),
              "%-34s %10.1f %9.1f %9.1f   %s" % ("hipMemcpyAsync D2D (t = 1)", mc, min(us["copy"]), max(us["copy"]), " ".join("%.1f" % v for v in us["copy"])),
              "blend_blob moves 3 bytes per blob byte: %.2f TB/s; the copy 2: %.2f TB/s" % (3 * nbytes / mb / 1e6, 2 * nbytes / mc / 1e6),
              "gate (a): blend %.1f us <= 1.5 x copy %.1f + the copy's spread %.1f = %.1f us: %s (%.2f x the copy)" % (mb, mc, sc, 1.5 * mc + sc, "met" if ok_a else "NOT met", mb / mc),
              "reported, no gate: wall time of one rsr_set_blend call %.3f ms (median of %d; min %.3f, max %.3f) against rsr_load_packed of the host-blended blob %.2f ms (min %.2f, max %.2f)"
              % (float(np.median(wall["set_blend"])), reps, min(wall["set_blend"]), max(wall["set_blend"]), float(np.median(wall["load_packed"])), min(wall["load_packed"]), max(wall["load_packed"])),
              "reported, no gate: rsr_model_blend of the two blobs on the host, one call: %.0f ms" % host_blend_ms, ""]

    # ---- (b) the frame on the blended context against the context that loaded the blend -------------------------------------------------
    x = torch.from_numpy(synth.make_image(3, W, H)).cuda()
    st = torch.cuda.Stream()
    variants = [("blended (set_blend 0.4)", sr), ("loaded the exported blob", plain)]
    times = {n: [] for n, _ in variants}
    with torch.cuda.stream(st):
        outs = {}
        for n, s in variants:   # warm-up: plans, workspace, torch's allocator
            outs[n] = torch_io.upscale(s, x)
            torch_io.upscale(s, x)
        st.synchronize()
        assert torch.equal(outs[variants[0][0]], outs[variants[1][0]]), "the two contexts differ in their output"
        for rep in range(reps):
            for n, s in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(frames):
                    y = torch_io.upscale(s, x)
                e1.record(st)
                e1.synchronize()
                del y
                times[n].append(e0.elapsed_time(e1) / frames)
    st.synchronize()
    sr.close()
    plain.close()
    del sr, plain
    lines += ["(b) C2 frame 1920 x 1080 RGB, tile 200 (60 tiles), u8 -> u8, device-resident, %d repetitions x %d frames per variant, alternating, HIP events on one stream; same output bytes" % (reps, frames),
              "%-34s %10s %9s %9s   %s" % ("variant", "median ms", "min ms", "max ms", "per repetition")]
    for n, _ in variants:
        t = times[n]
        lines.append("%-34s %10.2f %9.2f %9.2f   %s" % (n, np.median(t), min(t), max(t), " ".join("%.2f" % v for v in t)))
    m_b, m_p, s_p = float(np.median(times[variants[0][0]])), float(np.median(times[variants[1][0]])), spread(times[variants[1][0]])
    ok_b = abs(m_b - m_p) <= s_p
    lines += ["gate (b): |blended %.2f - loaded %.2f| = %.2f ms <= the loaded context's spread %.2f ms: %s (%+.2f %%)" % (m_b, m_p, abs(m_b - m_p), s_p, "met" if ok_b else "NOT met", (m_b / m_p - 1) * 100), ""]

    # ---- (c) bench.py, parent against this tree ----------------------------------------------------------------------------------------
    if parent:
        bres = {"parent": [], "this": []}
        bsum = {"parent": set(), "this": set()}
        for _ in range(3):
            for name, tree in (("parent", parent), ("this", ROOT)):
                r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(bench_steps), "--warmup", "3"], capture_output=True, text=True, timeout=900, cwd=tree)
                if r.returncode != 0:
                    raise SystemExit("bench.py of %s failed: %s" % (name, r.stderr[-2000:]))
                j = json.loads([ln for ln in r.stdout.strip().split("\n") if ln.startswith("{")][-1])
                bres[name].append(float(j["ms_per_step"]))
                bsum[name].add(j["config"]["checksum"])
        bp, bt = float(np.median(bres["parent"])), float(np.median(bres["this"]))
        bok = bt <= bp + spread(bres["parent"])
        bsame = bsum["parent"] == bsum["this"] and len(bsum["this"]) == 1
        lines += ["(c) bench.py --gpus 1 --steps %d --warmup 3 (the C2 RGB frame), parent against this commit, alternating x 3, ms_per_step:" % bench_steps,
                  "parent  median %.3f ms (%s), spread %.3f" % (bp, " ".join("%.3f" % v for v in bres["parent"]), spread(bres["parent"])),
                  "this    median %.3f ms (%s)" % (bt, " ".join("%.3f" % v for v in bres["this"])),
                  "gate (c): this <= parent + the parent's spread: %s (%+.2f %%)" % ("met" if bok else "NOT met", (bt / bp - 1) * 100),
                  "gate (c): same checksum (%s): %s" % (" ".join(str(v) for v in sorted(bsum["this"])), "met" if bsame else "NOT met")]
    else:
        lines.append("(c) bench.py, parent against this commit: not measured in this run -- no parent= checkout was given")
    lines.append("")

if resources:
    from kernel_resources import FIELDS, parse
    a, b = parse(resources[0]), parse(resources[1])
    assert a and all(set(FIELDS) <= set(v) for v in list(a.values()) + list(b.values())), "not a resource report"
    changed = [n for n in a if n in b and any(a[n].get(k) != b[n].get(k) for k in FIELDS)]
    gone = [n for n in a if n not in b]
    new = [n for n in b if n not in a]
    lines += ["The compiler's resource report of kernels.hip (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; tools/kernel_resources.py), parent against this commit:",
              "kernels of the parent: %d; absent here: %d; with other VGPRs, AGPRs, scratch, occupancy or LDS here: %d" % (len(a), len(gone), len(changed))]
    lines += ["  absent: %s" % n for n in gone] + ["  changed: %s: %s -> %s" % (n, a[n], b[n]) for n in changed]
    lines.append("gate: every existing kernel of kernels.hip keeps its VGPRs, scratch and occupancy: %s" % ("met" if not gone and not changed else "NOT met"))
    lines.append("new instantiations: %d" % len(new))
    for n in new:
        r = b[n]
        lines.append("  %-44s VGPRs %3d  SGPRs %3d  scratch %d B/lane  occupancy %d waves/SIMD  LDS %d B" % (n, r["VGPRs"], r.get("SGPRs", -1), r["ScratchSize"], r["Occupancy"], r["LDS"]))
    lines.append("gate: no new instantiation uses scratch or LDS: %s" % ("met" if all(b[n]["ScratchSize"] == 0 and b[n]["LDS"] == 0 for n in new) else "NOT met"))
    lines.append("conv_flow.hip is the parent's file byte for byte (not compiled into this report).")

text = "\n".join(lines)
print(text)
if out_path:
    with open(out_path, "w") as fh:
        fh.write(text + "\n")
