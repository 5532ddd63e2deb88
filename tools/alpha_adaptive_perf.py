"""Option "alpha_adaptive" on the C2 frame (1920 x 1080 RGBA, tile 200: 60 tiles), u8 -> u8, device-resident: what skipping the alpha pass
on flat-alpha tiles saves, and what the scan and its host wait cost where nothing can be skipped.

Four alphas over one colour picture --
    opaque       255 everywhere: every tile flat
    noise        seeded noise everywhere: no tile flat
    sprite 6     255 with a block of noise inside 6 of the 60 tiles (inside: more than the prepadding from the tile's edges, so its
                 neighbours' source rectangles do not see it)
    sprite 30    the same inside 30 tiles
-- each at "alpha_net" 0, "alpha_net" 1 and "alpha_net" 1 + "alpha_adaptive" 1 where the line below needs it.  All variants alternate inside
every repetition, on ONE torch stream, each timed with HIP events around `frames` back-to-back frames.  Gates, each on its own line:
    (a) opaque:  adaptive <= alpha_net 0's median + alpha_net 0's own spread over the repetitions + the scan's time in a profiled frame
    (b) noise:   adaptive <= alpha_net 1's median + its spread + the scan
Reported without a gate: the two sprites, the scan alone, the host time spent in the wait.
With parent=<checkout of the parent commit, built>: bench.py, parent against this tree as alternating child processes x 3.
With resources=<parent report>,<this report> (the compiler's -Rpass-analysis=kernel-resource-usage output for kernels.hip, made without a
GPU; tools/kernel_resources.py says how): the kernels whose registers, scratch or occupancy changed, and the new instantiations.
    python tools/alpha_adaptive_perf.py [reps=5] [frames=4] [parent=DIR] [resources=A,B] [bench_steps=10] [out=profiles/alpha_adaptive.txt]
    python tools/alpha_adaptive_perf.py resources=A,B gpu=0     (the resource report alone)
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

reps, frames, out_path, parent, resources, bench_steps, use_gpu = 5, 4, None, None, None, 10, True
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

W, H, T, P = 1920, 1080, 200, 10


def spread(t):
    return max(t) - min(t)


def alphas():
    """name -> ((H, W) uint8 alpha, tiles that vary)."""
    import numpy as np
    rng = np.random.default_rng(4)
    noise = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    out = {"opaque": (np.full((H, W), 255, np.uint8), 0), "noise": (noise, 60)}
    nx = (W + T - 1) // T
    for n in (6, 30):
        a = np.full((H, W), 255, np.uint8)
        for t in range(0, 60, 60 // n):   # every 10th / every 2nd tile, row-major
            yi, xi = divmod(t, nx)
            y0, x0 = yi * T + 3 * P, xi * T + 3 * P
            y1, x1 = min(y0 + 100, H - 1), x0 + 100
            a[y0:y1, x0:x1] = noise[y0:y1, x0:x1]
        out["sprite %d" % n] = (a, n)
    return out


lines = ["Option \"alpha_adaptive\": skip the alpha pass on flat-alpha tiles (tools/alpha_adaptive_perf.py; python tools/alpha_adaptive_perf.py out=profiles/alpha_adaptive.txt)",
         "Every gate is printed on its own line; nothing was fixed in advance.", ""]

if use_gpu:
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import realsr_ncnn_vulkan_amd as R
    from realsr_ncnn_vulkan_amd import synth, torch_io

    d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K", 42)
    sr = R.RealSR(0)
    sr.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
    sr.tilesize = T
    rgb = synth.make_image(3, W, H)
    xs, want_tiles = {}, {}
    for name, (a, n) in alphas().items():
        xs[name] = torch.from_numpy(np.ascontiguousarray(np.concatenate([rgb, a[:, :, None]], axis=2))).cuda()
        want_tiles[name] = n
    st = torch.cuda.Stream()

    def at(alpha_net, adaptive, name):
        def g():
            sr.alpha_net, sr.alpha_adaptive = alpha_net, adaptive
            try:
                return torch_io.upscale(sr, xs[name])
            finally:
                sr.alpha_net, sr.alpha_adaptive = 0, 0
        return g

    variants = [("opaque, alpha_net 0", at(0, 0, "opaque")), ("opaque, adaptive", at(1, 1, "opaque")),
                ("noise, alpha_net 1", at(1, 0, "noise")), ("noise, adaptive", at(1, 1, "noise")),
                ("sprite 6, adaptive", at(1, 1, "sprite 6")), ("sprite 30, adaptive", at(1, 1, "sprite 30"))]
    times = {n: [] for n, _ in variants}
    wait_us = {n: 0.0 for n, _ in variants}
    ran = {}
    with torch.cuda.stream(st):
        outs = {}
        for n, f in variants:   # warm-up: plans, workspace, torch's allocator; and the tiles each variant sends through the alpha pass
            t0 = sr.get_stat("alpha_tiles")
            outs[n] = f()
            st.synchronize()
            ran[n] = int(sr.get_stat("alpha_tiles") - t0)
            f()
        st.synchronize()
        for rep in range(reps):
            for n, f in variants:
                w0 = sr.get_stat("alpha_wait_us")
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(frames):
                    y = f()
                e1.record(st)
                e1.synchronize()
                del y
                times[n].append(e0.elapsed_time(e1) / frames)
                wait_us[n] += sr.get_stat("alpha_wait_us") - w0
    st.synchronize()
    for name in ("sprite 6", "sprite 30"):
        assert ran[name + ", adaptive"] == want_tiles[name], (name, ran)
    assert ran["opaque, adaptive"] == 0 and ran["noise, adaptive"] == 60
    assert torch.equal(outs["opaque, adaptive"], outs["opaque, alpha_net 0"]) and torch.equal(outs["noise, adaptive"], outs["noise, alpha_net 1"])

    # the scan in a profiled frame: the preprocessing class of the adaptive frame minus that of the frame it is compared with
    sr.set_profiling(True)
    prof = {}
    with torch.cuda.stream(st):
        for n, f in variants[:4]:
            f()
            st.synchronize()
            for _ in range(3):
                sr.get_profile(reset=True)
                f()
                st.synchronize()
                p = sr.get_profile(reset=True)
                if n not in prof or p["pre_ms"] < prof[n]["pre_ms"]:
                    prof[n] = p
    sr.set_profiling(False)
    scan_a = prof["opaque, adaptive"]["pre_ms"] - prof["opaque, alpha_net 0"]["pre_ms"]
    scan_b = prof["noise, adaptive"]["pre_ms"] - prof["noise, alpha_net 1"]["pre_ms"]
    sr.close()
    del sr

    lines += ["C2 frame 1920 x 1080 RGBA, tile 200 (60 tiles), u8 -> u8, device-resident, %d repetitions x %d frames per variant, alternating, HIP events on one stream" % (reps, frames),
              "device: %s" % torch.cuda.get_device_name(0),
              "%-22s %6s %9s %9s %9s   %s" % ("variant", "tiles", "median ms", "min ms", "max ms", "per repetition")]
    for n, _ in variants:
        t = times[n]
        lines.append("%-22s %6d %9.2f %9.2f %9.2f   %s" % (n, ran[n], np.median(t), min(t), max(t), " ".join("%.2f" % v for v in t)))
    lines.append("(tiles: tiles of a frame that ran the alpha pass, stat \"alpha_tiles\")")
    met = []
    for tag, n, base, scan in (("(a) fully opaque alpha", "opaque, adaptive", "opaque, alpha_net 0", scan_a), ("(b) nothing flat", "noise, adaptive", "noise, alpha_net 1", scan_b)):
        m, mb, sp = float(np.median(times[n])), float(np.median(times[base])), spread(times[base])
        ok = m <= mb + sp + scan
        met.append(ok)
        lines.append("gate %s: adaptive %.2f ms <= %s %.2f + its spread %.2f + the scan %.3f ms: %s (%+.2f %%)" % (tag, m, base.split(", ")[1], mb, sp, scan, "met" if ok else "NOT met", (m / mb - 1) * 100))
    lines.append("gates met: %d of %d" % (sum(met), len(met)))
    a0, a1 = float(np.median(times["opaque, alpha_net 0"])), float(np.median(times["noise, alpha_net 1"]))
    for name in ("sprite 6", "sprite 30"):
        m = float(np.median(times[name + ", adaptive"]))
        lines.append("reported, no gate: %s of 60 tiles vary: %.2f ms = alpha_net 0 + %.2f ms = %.3f x alpha_net 0 = %.3f x alpha_net 1" % (name.split()[1], m, m - a0, m / a0, m / a1))
    lines.append("reported, no gate: the scan alone (memset, alpha_flat_tiles, the copy of 60 bytes; the preprocessing class of a profiled adaptive frame minus that of the frame beside it, least of three): %.1f us on the opaque frame, %.1f us on the noise frame" % (scan_a * 1000, scan_b * 1000))
    lines.append("reported, no gate: host time in the wait, per frame (stat \"alpha_wait_us\"; the frames are enqueued back to back, so the host waits for the frame in front): " +
                 "; ".join("%s %.2f ms" % (n, wait_us[n] / (reps * frames) / 1000) for n, _ in variants if n.endswith("adaptive")))
    lines.append("")

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
        lines += ["bench.py --gpus 1 --steps %d --warmup 3 (the C2 RGB frame), parent against this commit, alternating x 3, ms_per_step:" % bench_steps,
                  "parent  median %.3f ms (%s), spread %.3f" % (bp, " ".join("%.3f" % v for v in bres["parent"]), spread(bres["parent"])),
                  "this    median %.3f ms (%s)" % (bt, " ".join("%.3f" % v for v in bres["this"])),
                  "gate: this <= parent + the parent's spread: %s (%+.2f %%)" % ("met" if bok else "NOT met", (bt / bp - 1) * 100),
                  "gate: same checksum (%s): %s" % (" ".join(str(v) for v in sorted(bsum["this"])), "met" if bsame else "NOT met")]
    else:
        lines.append("bench.py, parent against this commit: not measured in this run -- no parent= checkout was given")
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
