"""Option "alpha_net" on the C2 frame (1920 x 1080 RGBA, tile 200), device-resident: the alpha through the network inside the library against
the detour a caller needed before the option existed --

    native       torch_io.upscale on the (H, W, 4) tensor with sr.alpha_net = 1: ONE call, two network passes
    detour       torch_io.upscale f32 -> f32 of the colour, torch_io.upscale f32 -> f32 of the gray image of the alpha, then in torch: the
                 mean of the three planes, quantise, stack, permute to HWC

-- for u8 -> u8 at out_scale 4 and 2 and for u16 -> u16 at 4.  All variants alternate inside every repetition, on ONE torch stream, each timed
with HIP events around `frames` back-to-back frames.  Gate, printed per line: native <= detour + the detour's own spread over the repetitions.
Reported without a gate: alpha_net 1 against alpha_net 0 on the RGBA frame and against the RGB frame; pre_ms / post_ms of a profiled frame.
With parent=<checkout of the parent commit, built>: the RGBA frame at alpha_net 0 (the parent knows no such option: its default) and
bench.py, parent against this tree as alternating child processes, with their output checksums.
With resources=<parent report>,<this report> (the compiler's -Rpass-analysis=kernel-resource-usage output for kernels.hip, made without a
GPU): the kernels whose registers, scratch or occupancy changed, and the new instantiations.
    python tools/alpha_net_perf.py [reps=5] [frames=4] [parent=DIR] [resources=A,B] [bench_steps=10] [out=profiles/alpha_net.txt]
    python tools/alpha_net_perf.py resources=A,B gpu=0     (the resource report alone)
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

reps, frames, out_path, parent, resources, bench_steps, use_gpu, child = 5, 4, None, None, None, 10, True, None
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
    elif k == "child":  # internal: the RGBA frame at the default options with the library of the tree `child`
        child = os.path.abspath(v)

W, H = 1920, 1080


def rgba_frame():
    """The C2 picture with an alpha of its own: a ramp, a hard-edged cut-out and noise."""
    import numpy as np
    from realsr_ncnn_vulkan_amd import synth
    img = synth.make_image(3, W, H)
    rng = np.random.default_rng(4)
    a = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    a[:H // 3] = (np.arange(W) * 255 // (W - 1)).astype(np.uint8)[None, :]
    a[H // 3:2 * H // 3, :W // 2] = 0
    a[H // 3:2 * H // 3, W // 2:] = 255
    return np.ascontiguousarray(np.concatenate([img, a[:, :, None]], axis=2))


def spread(t):
    return max(t) - min(t)


if child:
    # one child process: `reps` x `frames` RGBA frames with the library of the tree `child`, one JSON line
    sys.path.insert(0, child)
    import numpy as np
    import torch
    import realsr_ncnn_vulkan_amd as R
    from realsr_ncnn_vulkan_amd import synth, torch_io
    d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K", 42)
    sr = R.RealSR(0)
    sr.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
    sr.tilesize = 200
    x = torch.from_numpy(rgba_frame()).cuda()
    st = torch.cuda.Stream()
    ts = []
    with torch.cuda.stream(st):
        y = torch_io.upscale(sr, x)
        torch_io.upscale(sr, x)
        st.synchronize()
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(frames):
                y = torch_io.upscale(sr, x)
            e1.record(st)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) / frames)
    print(json.dumps({"ms": ts, "checksum": int(y[::97, ::89].to(torch.int64).sum().item())}), flush=True)
    sr.close()
    sys.exit(0)


def resource_lines(a_path, b_path):
    """The compiler's resource report of kernels.hip, parent against this tree (the parser of tools/kernel_resources.py)."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from kernel_resources import FIELDS, parse

    def demangle(names):
        try:
            r = subprocess.run(["c++filt"] + [n.replace("DF16_", "Dh") for n in names], capture_output=True, text=True)  # (_Float16 in the spelling binutils knows)
            got = r.stdout.split("\n")[:len(names)]
            return dict(zip(names, got)) if r.returncode == 0 and len(got) == len(names) else {n: n for n in names}
        except OSError:
            return {n: n for n in names}

    a, b = parse(a_path), parse(b_path)
    assert a and all(set(FIELDS) <= set(v) for v in list(a.values()) + list(b.values())), "not a resource report"
    changed = [n for n in a if n in b and any(a[n].get(k) != b[n].get(k) for k in FIELDS)]
    gone = [n for n in a if n not in b]
    new = [n for n in b if n not in a]
    dm = demangle(changed + gone + new)
    short = lambda n: dm[n].replace("rsr::", "").replace("(PostArgs)", "").replace("(PreArgs)", "").replace("void ", "")  # noqa: E731
    ls = ["The compiler's resource report of kernels.hip (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; tools/kernel_resources.py), parent against this commit:",
          "kernels of the parent: %d; absent here: %d; with other VGPRs, AGPRs, scratch, occupancy or LDS here: %d" % (len(a), len(gone), len(changed))]
    for n in gone:
        ls.append("  absent: %s" % short(n))
    for n in changed:
        ls.append("  changed: %s: %s -> %s" % (short(n), a[n], b[n]))
    ls.append("gate: every existing kernel of kernels.hip keeps its VGPRs, scratch and occupancy: %s" % ("met" if not gone and not changed else "NOT met"))
    ls.append("new instantiations: %d" % len(new))
    for n in new:
        r = b[n]
        ls.append("  %-52s VGPRs %3d  SGPRs %3d  scratch %d B/lane  occupancy %d waves/SIMD  LDS %d B" % (
            short(n), r["VGPRs"], r.get("SGPRs", -1), r["ScratchSize"], r["Occupancy"], r["LDS"]))
    ls.append("gate: no new instantiation uses scratch: %s" % ("met" if all(b[n]["ScratchSize"] == 0 for n in new) else "NOT met"))
    return ls


lines = ["Option \"alpha_net\": the alpha of an RGBA image through the network (tools/alpha_net_perf.py; python tools/alpha_net_perf.py out=profiles/alpha_net.txt)",
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
    sr.tilesize = 200
    img8 = rgba_frame()
    img16 = (img8.astype(np.uint16) * 257 + np.random.default_rng(5).integers(-128, 129, size=img8.shape)).clip(0, 65535).astype(np.uint16)
    x8 = torch.from_numpy(img8).cuda()
    x16 = torch.from_numpy(img16.view(np.int16)).cuda()
    x8rgb = x8[:, :, :3].contiguous()
    st = torch.cuda.Stream()

    def planar(x, top):
        """(H, W, 4) integer tensor -> the colour as (3, H, W) floats and the gray image of the alpha likewise."""
        f = ((x.to(torch.int32) & 0xFFFF).float() * (1.0 / top)).permute(2, 0, 1)
        return f[:3].contiguous(), f[3:4].expand(3, -1, -1).contiguous()

    def detour(x, top, dtype):
        """Two float calls and torch: what a caller did for the network's alpha before the option existed."""
        rgb, g = planar(x, top)
        y = torch_io.upscale(sr, rgb)
        a = torch_io.upscale(sr, g)
        m = (((a[0] + a[1]) + a[2]) * (1.0 / 3.0)).clamp_(max=1.0)
        q = (torch.cat([y, m[None]], dim=0) * float(top) + 0.5).floor_().to(torch.int32)
        return q.permute(1, 2, 0).contiguous().to(dtype)

    def at(scale, alpha_net, f):
        def g():
            sr.out_scale = scale
            sr.alpha_net = alpha_net
            try:
                return f()
            finally:
                sr.alpha_net = 0
        return g

    variants = []
    for name, scale, x, top, dtype in (("u8 x4", 4, x8, 255, torch.uint8), ("u8 x2", 2, x8, 255, torch.uint8), ("u16 x4", 4, x16, 65535, torch.int16)):
        variants.append(("native " + name, at(scale, 1, lambda x=x: torch_io.upscale(sr, x))))
        variants.append(("detour " + name, at(scale, 0, lambda x=x, top=top, dtype=dtype: detour(x, top, dtype))))
    variants.append(("rgba u8 x4, alpha_net 0", at(4, 0, lambda: torch_io.upscale(sr, x8))))
    variants.append(("rgb u8 x4", at(4, 0, lambda: torch_io.upscale(sr, x8rgb))))

    times = {n: [] for n, _ in variants}
    with torch.cuda.stream(st):
        outs = {n: f() for n, f in variants}   # warm-up: plans, workspace, torch's kernels and allocator
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
    checksum_here = int(outs["rgba u8 x4, alpha_net 0"][::97, ::89].to(torch.int64).sum().item())

    lines += ["C2 frame 1920 x 1080 RGBA, tile 200, device-resident, %d repetitions x %d frames per variant, alternating, HIP events on one stream" % (reps, frames),
              "device: %s" % torch.cuda.get_device_name(0),
              "%-26s %9s %9s %9s   %s" % ("variant", "median ms", "min ms", "max ms", "per repetition")]
    met = []
    for n, _ in variants:
        t = times[n]
        line = "%-26s %9.2f %9.2f %9.2f   %s" % (n, np.median(t), min(t), max(t), " ".join("%.2f" % v for v in t))
        if n.startswith("native"):
            dn = "detour" + n[len("native"):]
            dt = times[dn]
            ok = bool(np.median(t) <= np.median(dt) + spread(dt))
            met.append(ok)
            code = lambda a: a.to(torch.int32) & 0xFFFF  # noqa: E731
            da = int((code(outs[n])[:, :, 3] - code(outs[dn])[:, :, 3]).abs().max())
            dc = int((code(outs[n])[:, :, :3] - code(outs[dn])[:, :, :3]).abs().max())
            line += "   gate: <= detour %.2f + its spread %.2f ms: %s (%+.2f %%); max code difference to the detour: alpha %d, colour %d" % (
                np.median(dt), spread(dt), "met" if ok else "NOT met", (np.median(t) / np.median(dt) - 1) * 100, da, dc)
        lines.append(line)
    lines.append("gates met: %d of %d" % (sum(met), len(met)))
    n1, a0, rgb = (float(np.median(times[k])) for k in ("native u8 x4", "rgba u8 x4, alpha_net 0", "rgb u8 x4"))
    lines.append("reported, no gate: alpha_net 1 / alpha_net 0 on the RGBA frame = %.3f; alpha_net 1 / the RGB frame = %.3f; RGBA at alpha_net 0 / the RGB frame = %.3f" % (n1 / a0, n1 / rgb, a0 / rgb))

    # pre_ms / post_ms of a profiled frame: both passes' launches beside the one RGBA post launch of alpha_net 0
    lines.append("pre_ms / post_ms of a profiled frame (the least post_ms of three; no gate); at alpha_net 1 both classes hold two launches, the colour pass's and the alpha pass's:")
    sr.set_profiling(True)
    shapes = []
    for name, scale, x in (("u8 x4", 4, x8), ("u8 x2", 2, x8), ("u16 x4", 4, x16)):
        for an in (0, 1):
            shapes.append(("rgba %s, alpha_net %d" % (name, an), at(scale, an, lambda x=x: torch_io.upscale(sr, x))))
    prof = {}
    with torch.cuda.stream(st):
        for n, f in shapes:
            f()
            st.synchronize()
            for _ in range(3):
                sr.get_profile(reset=True)
                f()
                st.synchronize()
                p = sr.get_profile(reset=True)
                if n not in prof or p["post_ms"] < prof[n]["post_ms"]:
                    prof[n] = p
    sr.set_profiling(False)
    for n, _ in shapes:
        p = prof[n]
        lines.append("%-28s pre_ms %.3f post_ms %.3f conv_ms %.2f conv_launches %d" % (n, p["pre_ms"], p["post_ms"], p["conv_ms"], p["conv_launches"]))
    for name in ("u8 x4", "u8 x2", "u16 x4"):
        p0, p1 = prof["rgba %s, alpha_net 0" % name], prof["rgba %s, alpha_net 1" % name]
        lines.append("the new launches, %s: preproc_tiles<AlphaOf<..>> %.3f ms, postproc_tiles_alpha %.3f ms (the differences of the lines above)" % (
            name, p1["pre_ms"] - p0["pre_ms"], p1["post_ms"] - p0["post_ms"]))
    sr.out_scale = 4
    sr.close()
    del sr

    lines.append("")
    if parent:
        # RGBA at alpha_net 0 (the parent's only behaviour), parent against this tree: alternating child processes
        res = {"parent": [], "this": []}
        sums = {"parent": set(), "this": set()}
        for _ in range(3):
            for name, tree in (("parent", parent), ("this", ROOT)):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "child=" + tree, "reps=%d" % reps, "frames=%d" % frames], capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise SystemExit("child %s failed: %s" % (name, r.stderr[-2000:]))
                j = json.loads(r.stdout.strip().split("\n")[-1])
                res[name].append(float(np.median(j["ms"])))
                sums[name].add(j["checksum"])
        mp, mt = float(np.median(res["parent"])), float(np.median(res["this"]))
        ok = mt <= mp + spread(res["parent"])
        same = sums["parent"] == sums["this"] and len(sums["this"]) == 1
        lines += ["RGBA frame u8 -> u8 at alpha_net 0 (the parent has no such option), parent against this commit: 3 alternating pairs of child processes, each the median of %d x %d frames" % (reps, frames),
                  "parent  median %.2f ms (%s)" % (mp, " ".join("%.2f" % v for v in res["parent"])),
                  "this    median %.2f ms (%s)" % (mt, " ".join("%.2f" % v for v in res["this"])),
                  "gate: this <= parent + the parent's spread %.2f ms: %s (%+.2f %%)" % (spread(res["parent"]), "met" if ok else "NOT met", (mt / mp - 1) * 100),
                  "gate: identical output checksum (%s): %s" % (" ".join(str(v) for v in sorted(sums["this"])), "met" if same else "NOT met"),
                  "the same checksum in the alternating run above: %s" % (checksum_here in sums["this"])]
        # bench.py, parent against this tree, alternating x 3
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
        lines += ["", "bench.py --gpus 1 --steps %d --warmup 3 (the C2 RGB frame), parent against this commit, alternating x 3, ms_per_step:" % bench_steps,
                  "parent  median %.3f ms (%s), spread %.3f" % (bp, " ".join("%.3f" % v for v in bres["parent"]), spread(bres["parent"])),
                  "this    median %.3f ms (%s)" % (bt, " ".join("%.3f" % v for v in bres["this"])),
                  "gate: this <= parent + the parent's spread: %s (%+.2f %%)" % ("met" if bok else "NOT met", (bt / bp - 1) * 100),
                  "gate: same checksum (%s): %s" % (" ".join(str(v) for v in sorted(bsum["this"])), "met" if bsame else "NOT met")]
    else:
        lines.append("parent against this commit (RGBA at alpha_net 0, bench.py): not measured in this run -- no parent= checkout was given")
    lines.append("")

if resources:
    lines += resource_lines(resources[0], resources[1])

text = "\n".join(lines)
print(text)
if out_path:
    with open(out_path, "w") as fh:
        fh.write(text + "\n")
