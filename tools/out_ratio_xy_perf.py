"""A ratio per axis (rsr_set_out_ratio_xy, include/realsr_hip.h "a ratio per axis") measured on one board.

    A  native against the detour, in this process, alternating (HIP events on one torch stream, `frames` back-to-back frames per timing,
       medians over `reps` repetitions after a warm-up):
         720 x 480 NV12 -> 1920 x 1080 NV12 at (8/3, 9/4), tile 192      detour: the isotropic 9/4 call to F16_CHW (1620 x 1080), a torch
                                                                          area resize of the x axis to 1920, the NV12 encode as torch ops
         1440 x 1080 NV12 -> 1920 x 1080 NV12 at (4/3, 1), tile 198      detour: the x4 call to F16_CHW (5760 x 4320), a torch area resize
                                                                          to 1920 x 1080, the same encode
       gate: native median <= detour median + the detour's own spread (max - min).  The detour is a timing comparator: its rounding is
       torch's, not the library's.
    B  the isotropic path against the parent commit: the C2 frame (1920 x 1080) at 3/2 and tile 200, u8 -> u8 and nv12 -> nv12, frame
       median and post_ms (ten profiled frames per child, one figure each).  Parent and this commit run as child processes of this script, alternating, `rounds`
       times each; a child imports the package of the tree it is given.  gate: this commit's median <= the parent's median + the parent's
       own spread in this run (over all its repetitions), for the frame and for post_ms.
    C  the default path: bench.py --gpus 1, parent against this commit, alternating, `rounds` times each: the same checksum, and this
       commit's median ms_per_step within the parent's spread.

B and C need parent=DIR, a built checkout of the parent commit; without it they are reported as not measured.
    python tools/out_ratio_xy_perf.py [reps=5] [frames=4] [rounds=3] [steps=10] [warmup=3] [parent=DIR] [out=profiles/out_ratio_xy.txt]
"""
import json
import os
import subprocess
import sys
from fractions import Fraction

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = dict(kv.split("=", 1) for kv in sys.argv[1:])
ROOT = os.path.abspath(args.get("root", HERE))  # (a child of section B: the tree whose package it measures)
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import realsr_ncnn_vulkan_amd as R  # noqa: E402
from realsr_ncnn_vulkan_amd import synth, torch_io  # noqa: E402

reps, frames, rounds = int(args.get("reps", 5)), int(args.get("frames", 4)), int(args.get("rounds", 3))
steps, warmup = int(args.get("steps", 10)), int(args.get("warmup", 3))
parent, out_path = args.get("parent"), args.get("out")
KR, KB = 0.2126, 0.0722
KG = 1 - KR - KB
NV12 = R.RSR_FMT_NV12
d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K", 42)
st = torch.cuda.Stream()


def to_nv12(rgb):
    """float CHW RGB in [0, 1] -> the (3H/2, W) uint8 surface: BT.709 limited range, chroma = the quad's mean (tools/yuv_ratio_perf.py)."""
    rgb = rgb.float()
    y = KR * rgb[0] + KG * rgb[1] + KB * rgb[2]
    m = F.avg_pool2d(rgb[None], 2)[0]
    ym = KR * m[0] + KG * m[1] + KB * m[2]
    cb, cr = (m[2] - ym) / (2 * (1 - KB)), (m[0] - ym) / (2 * (1 - KR))
    yq = (y * 219 + 16.5).floor().clamp(0, 255)
    cq = (torch.stack([cb, cr], dim=-1) * 224 + 128.5).floor().clamp(0, 255)
    return torch.cat([yq, cq.reshape(cq.shape[0], -1)], dim=0).to(torch.uint8)


def context():
    sr = R.RealSR(0)
    sr.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
    return sr


def alternate(variants, reps_, frames_):
    """Every variant once per repetition, `frames_` back-to-back frames between two HIP events: ms per frame, per repetition; and what
    each variant returned in the warm-up pass."""
    times = {n: [] for n, _ in variants}
    with torch.cuda.stream(st):
        outs = {n: f() for n, f in variants}  # warm-up: plans, workspace, torch's kernels and allocator
        for n, f in variants:
            f()
        st.synchronize()
        for rep in range(reps_):
            for n, f in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(frames_):
                    y = f()
                e1.record(st)
                e1.synchronize()
                del y
                times[n].append(e0.elapsed_time(e1) / frames_)
    st.synchronize()
    return times, outs


def post_ms(sr, f, n=10):
    """post_ms of n profiled frames, one figure per frame (rsr_get_profile; profiling adds events around the launches)."""
    sr.set_profiling(True)
    try:
        with torch.cuda.stream(st):
            f()
            st.synchronize()
            got = []
            for _ in range(n):
                sr.get_profile(reset=True)
                f()
                st.synchronize()
                got.append(sr.get_profile(reset=True)["post_ms"])
            return got
    finally:
        sr.set_profiling(False)


def surface_of(w, h, seed):
    img = synth.make_image(seed, w, h)
    return to_nv12(torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).cuda().float() / 255)


# ---- a child of section B: the C2 frame at isotropic 3/2 on the tree `root`, one JSON line --------------------------------------------
if args.get("child") == "iso":
    sr = context()
    sr.tilesize = 200
    sr.out_ratio = Fraction(3, 2)
    img = synth.make_image(3, 1920, 1080)
    x8 = torch.from_numpy(img).cuda()
    surf = surface_of(1920, 1080, 3)
    variants = [("u8->u8 3/2", lambda: torch_io.upscale(sr, x8)), ("nv12->nv12 3/2", lambda: torch_io.upscale_yuv(sr, surf))]
    times, outs = alternate(variants, reps, frames)
    print(json.dumps({"times": times, "post_ms": {n: post_ms(sr, f) for n, f in variants},
                      "checksum": {n: int(o[::97, ::89].to(torch.int64).sum().item()) for n, o in outs.items()}}), flush=True)
    sr.close()
    sys.exit(0)


lines = ["rsr_set_out_ratio_xy: a ratio per axis.  %d repetitions x %d frames per variant, alternating, HIP events on one stream; B and C: %d rounds per commit"
         % (reps, frames, rounds), "device: %s" % torch.cuda.get_device_name(0), "command: python tools/out_ratio_xy_perf.py " + " ".join(sys.argv[1:])]
gates = []


def gate(text, ok):
    gates.append("gate: %-110s %s" % (text, "met" if ok else "MISSED"))


def emit():
    """Print what has been measured so far and keep it in `out`: a later section that fails loses nothing."""
    text = "\n".join(lines + [""] + gates)
    print(text, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


def row(name, t, extra=""):
    return "%-34s %9.2f %9.2f %9.2f   %s%s" % (name, np.median(t), min(t), max(t), " ".join("%.2f" % v for v in t), extra)


# ---- A: native against the detour -----------------------------------------------------------------------------------------------------
def section_a(sr, title, w, h, tile, pair, iso):
    sr.tilesize = tile
    surf = surface_of(w, h, 5)
    ow, oh = w * pair[0].numerator // pair[0].denominator, h * pair[1].numerator // pair[1].denominator

    def native():
        sr.out_ratio_xy = pair
        return torch_io.upscale_yuv(sr, surf)

    def detour():
        sr.out_ratio = iso
        iw, ih = sr.out_size(w, h)
        y = torch.empty((3, ih, iw), dtype=torch.float16, device="cuda")
        sr.process_device_fmt(surf.data_ptr(), NV12, w, h, 3, y.data_ptr(), R.RSR_FMT_F16_CHW, stream=torch.cuda.current_stream().cuda_stream)
        return to_nv12(F.interpolate(y[None], size=(oh, ow), mode="area")[0])

    variants = [("native", native), ("detour", detour)]
    times, outs = alternate(variants, reps, frames)
    pm = float(np.median(post_ms(sr, native)))
    assert tuple(outs["native"].shape) == tuple(outs["detour"].shape) == (oh * 3 // 2, ow)
    diff = (outs["native"].to(torch.int32) - outs["detour"].to(torch.int32)).abs()
    spread = max(times["detour"]) - min(times["detour"])
    lines.extend(["", "A  %s, tile %d: %d x %d -> %d x %d" % (title, tile, w, h, ow, oh),
                  "%-34s %9s %9s %9s   %s" % ("variant", "median ms", "min ms", "max ms", "per repetition (ms per frame)"),
                  row("native nv12->nv12 (%s, %s)" % pair, times["native"], "   post_ms %.3f" % pm),
                  row("detour: %s to F16 + area + encode" % iso, times["detour"], "   spread %.2f ms" % spread),
                  "code difference native - detour (another filter on the resized axis: no claim): mean %.2f, max %d" % (diff.float().mean().item(), int(diff.max()))])
    gate("A %s: native <= detour + its spread (%.2f <= %.2f + %.2f ms)" % (title, np.median(times["native"]), np.median(times["detour"]), spread),
         np.median(times["native"]) <= np.median(times["detour"]) + spread)


sr = context()
section_a(sr, "NTSC DVD", 720, 480, 192, (Fraction(8, 3), Fraction(9, 4)), Fraction(9, 4))
section_a(sr, "HDV", 1440, 1080, 198, (Fraction(4, 3), Fraction(1)), Fraction(4))
sr.close()
del sr
torch.cuda.empty_cache()
emit()


# ---- B, C: against the parent commit, child processes alternating ------------------------------------------------------------------------
def child(root, cmd):
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("%s in %s failed (%d): %s" % (" ".join(cmd), root, r.returncode, r.stderr[-2000:]))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


if not parent:
    lines.extend(["", "B  the isotropic path against the parent commit: not measured (no parent=DIR)", "C  bench.py against the parent commit: not measured (no parent=DIR)"])
else:
    parent = os.path.abspath(parent)
    trees = [("parent", parent), ("this", HERE)]
    runs = {k: [] for k, _ in trees}
    for rnd in range(rounds):
        for k, root in trees:
            runs[k].append(child(root, [sys.executable, os.path.abspath(__file__), "child=iso", "root=" + root, "reps=%d" % reps, "frames=%d" % frames]))
    lines.extend(["", "B  C2 frame 1920 x 1080 at isotropic 3/2, tile 200, device-resident: %d child processes per commit, alternating, %d repetitions x %d frames each" % (rounds, reps, frames),
                  "%-34s %9s %9s %9s   %s" % ("variant", "median ms", "min ms", "max ms", "per repetition (ms per frame), all rounds")])
    for n in ("u8->u8 3/2", "nv12->nv12 3/2"):
        t = {k: [v for r in runs[k] for v in r["times"][n]] for k in runs}
        p = {k: [v for r in runs[k] for v in r["post_ms"][n]] for k in runs}
        for k in ("parent", "this"):
            lines.append(row("%-7s %s" % (k, n), t[k], "   post_ms median %.3f min %.3f max %.3f (%d profiled frames)" % (np.median(p[k]), min(p[k]), max(p[k]), len(p[k]))))
        spread, pspread = max(t["parent"]) - min(t["parent"]), max(p["parent"]) - min(p["parent"])
        same = all(r["checksum"][n] == runs["parent"][0]["checksum"][n] for k in runs for r in runs[k])
        lines.append("%-34s checksum of the output %s" % ("", "identical in all runs" if same else "DIFFERS"))
        gate("B %s: frame median not above the parent's by more than its spread (%.2f <= %.2f + %.2f ms)" % (n, np.median(t["this"]), np.median(t["parent"]), spread),
             np.median(t["this"]) <= np.median(t["parent"]) + spread)
        gate("B %s: post_ms median not above the parent's by more than its spread (%.3f <= %.3f + %.3f ms)" % (n, np.median(p["this"]), np.median(p["parent"]), pspread),
             np.median(p["this"]) <= np.median(p["parent"]) + pspread)
        gate("B %s: the same output checksum as the parent" % n, same)
    emit()
    bench = {k: [] for k, _ in trees}
    for rnd in range(rounds):
        for k, root in trees:
            bench[k].append(child(root, [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]))
    ms = {k: [r["ms_per_step"] for r in bench[k]] for k in bench}
    sums = {k: sorted(set(r["config"]["checksum"] for r in bench[k])) for k in bench}
    spread = max(ms["parent"]) - min(ms["parent"])
    lines.extend(["", "C  bench.py --gpus 1 --steps %d --warmup %d: %d runs per commit, alternating" % (steps, warmup, rounds),
                  "%-34s %9s %9s %9s   %s" % ("commit", "median ms", "min ms", "max ms", "ms_per_step per run")])
    for k in ("parent", "this"):
        lines.append(row(k, ms[k], "   checksum %s, value %s Mpix/s" % (sums[k], " ".join("%.2f" % r["value"] for r in bench[k]))))
    gate("C the same checksum (%s)" % sums["this"], sums["this"] == sums["parent"] and len(sums["this"]) == 1)
    gate("C ms_per_step median within the parent's spread (%.3f <= %.3f + %.3f ms)" % (np.median(ms["this"]), np.median(ms["parent"]), spread),
         np.median(ms["this"]) <= np.median(ms["parent"]) + spread)

emit()
