"""NV12 / P010 OUTPUT at a rational output ratio (include/realsr_hip.h, "YUV output at a ratio") on the C2 frame (1920 x 1080),
device-resident, against the detour a caller had to take before: the same surface in, F16_CHW out at the same ratio, then RGB -> YUV, the
2 x 2 chroma mean, quantisation and the UV interleave as torch ops (BT.709 limited, centre siting -- a timing comparator: its rounding is
torch's, not the library's).

    A  tile 200   nv12->nv12 and p010->p010 at 3/2, 9/4 and 3/1, each against its detour; u8->u8 at the same ratio in the same run
    B  tile 201   the same at 4/3
    C  sitings    nv12->nv12 and p010->p010 at 3/2, tile 200: yuv_siting 1 and 2 against 0 in the same run
    D  post_ms    of the new launch (postproc_tiles_yuv_area) from one profiled frame per native variant of A, B and C
    E  C5 (TTA)   nv12->nv12 at 3/2 and its detour: recorded, no gate

All variants of a section alternate inside every repetition, on ONE torch stream, each timed with HIP events around `frames` back-to-back
frames; medians over the repetitions after a warm-up.  One gate per native line of A and B: its median is not above the detour's median
plus the detour's own spread (max - min) in that run.
    python tools/yuv_ratio_perf.py [reps=5] [frames=4] [out=profiles/yuv_ratio.txt] [tta=1]
"""
import os
import sys
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import realsr_ncnn_vulkan_amd as R  # noqa: E402
from realsr_ncnn_vulkan_amd import synth, torch_io  # noqa: E402

reps, frames, out_path, with_tta = 5, 4, None, 1
for kv in sys.argv[1:]:
    k, v = kv.split("=")
    if k == "reps":
        reps = int(v)
    elif k == "frames":
        frames = int(v)
    elif k == "out":
        out_path = v
    elif k == "tta":
        with_tta = int(v)

W, H = 1920, 1080
KR, KB = 0.2126, 0.0722
KG = 1 - KR - KB
FMT = {8: (R.RSR_FMT_NV12, "nv12"), 10: (R.RSR_FMT_P010, "p010")}
d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K", 42)
st = torch.cuda.Stream()
lines = ["YUV output at a ratio: C2 frame 1920 x 1080, device-resident, BT.709 limited, %d repetitions x %d frames per variant, alternating, HIP events on one stream"
         % (reps, frames), "device: %s" % torch.cuda.get_device_name(0), "command: python tools/yuv_ratio_perf.py " + " ".join(sys.argv[1:])]


def to_yuv(rgb, bits):
    """float CHW RGB in [0, 1] -> the (3H/2, W) surface (uint8, or int16 holding code << 6): BT.709 limited range, chroma = the quad's mean."""
    k = 1 << (bits - 8)
    rgb = rgb.float()
    y = KR * rgb[0] + KG * rgb[1] + KB * rgb[2]
    m = F.avg_pool2d(rgb[None], 2)[0]
    ym = KR * m[0] + KG * m[1] + KB * m[2]
    cb, cr = (m[2] - ym) / (2 * (1 - KB)), (m[0] - ym) / (2 * (1 - KR))
    yq = (y * (219 * k) + (16 * k + 0.5)).floor().clamp(0, (1 << bits) - 1)
    cq = (torch.stack([cb, cr], dim=-1) * (224 * k) + (128 * k + 0.5)).floor().clamp(0, (1 << bits) - 1)
    s = torch.cat([yq, cq.reshape(cq.shape[0], -1)], dim=0)
    return s.to(torch.uint8) if bits == 8 else (s.to(torch.int32) << 6).to(torch.int16)


img = synth.make_image(3, W, H)
x8 = torch.from_numpy(img).cuda()
rgb0 = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).cuda().float() / 255
surf = {8: to_yuv(rgb0, 8), 10: to_yuv(rgb0, 10)}


def context(tta):
    sr = R.RealSR(0, tta_mode=tta)
    sr.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
    return sr


def rname(r):
    return "%d/%d" % (r.numerator, r.denominator)


def native(sr, bits, ratio, siting=0):
    def f():
        sr.out_ratio, sr.yuv_siting = ratio, siting
        return torch_io.upscale_yuv(sr, surf[bits])
    return f


def detour(sr, bits, ratio):
    """The surface in, F16_CHW out at the same ratio (one call), then the encode as torch ops."""
    def f():
        sr.out_ratio, sr.yuv_siting = ratio, 0
        ow, oh = sr.out_size(W, H)
        y = torch.empty((3, oh, ow), dtype=torch.float16, device="cuda")
        sr.process_device_fmt(surf[bits].data_ptr(), FMT[bits][0], W, H, 3, y.data_ptr(), R.RSR_FMT_F16_CHW, stream=torch.cuda.current_stream().cuda_stream)
        return to_yuv(y, bits)
    return f


def u8(sr, ratio):
    def f():
        sr.out_ratio = ratio
        return torch_io.upscale(sr, x8)
    return f


def alternate(variants, reps_, frames_):
    """Every variant once per repetition, `frames_` back-to-back frames between two HIP events: ms per frame, per repetition; and what
    each variant returned in the first warm-up pass."""
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


def profiled(sr, variants):
    """One profiled frame per variant (rsr_get_profile; profiling adds events around the launches)."""
    post = {}
    sr.set_profiling(True)
    try:
        with torch.cuda.stream(st):
            for n, f in variants:
                f()
                st.synchronize()
                sr.get_profile(reset=True)
                f()
                st.synchronize()
                post[n] = sr.get_profile(reset=True)
    finally:
        sr.set_profiling(False)
    return post


def code(a):
    return a.to(torch.int32) if a.dtype == torch.uint8 else (a.to(torch.int32) & 0xFFFF) >> 6


def section(sr, title, tile, ratios, reps_, frames_, gated=True):
    sr.tilesize = tile
    variants = []
    for r in ratios:
        for bits in (8, 10):
            name = FMT[bits][1]
            variants.append(("%s->%s %s" % (name, name, rname(r)), native(sr, bits, r)))
            variants.append(("detour %s %s" % (name, rname(r)), detour(sr, bits, r)))
        variants.append(("u8->u8 %s" % rname(r), u8(sr, r)))
    times, outs = alternate(variants, reps_, frames_)
    post = profiled(sr, [(n, f) for n, f in variants if "->" in n])
    lines.extend(["", "%s, tile %d" % (title, tile), "%-18s %9s %9s %9s %8s   %s" % ("variant", "median ms", "min ms", "max ms", "post_ms", "per repetition")])
    for n, _ in variants:
        t = times[n]
        line = "%-18s %9.2f %9.2f %9.2f %8s   %s" % (n, np.median(t), min(t), max(t), "%.3f" % post[n]["post_ms"] if n in post else "", " ".join("%.2f" % v for v in t))
        if "->" in n and not n.startswith("u8"):
            dn = "detour %s %s" % (n.split("->")[0], n.split()[-1])
            dt = times[dn]
            spread = max(dt) - min(dt)
            diff = int((code(outs[n]) - code(outs[dn])).abs().max())
            if gated:
                ok = np.median(t) <= np.median(dt) + spread
                line += "   gate: <= detour %.2f + its spread %.2f ms: %s (%+.2f %%)" % (np.median(dt), spread, "met" if ok else "MISSED", (np.median(t) / np.median(dt) - 1) * 100)
            else:
                line += "   (no gate) detour %.2f, its spread %.2f ms (%+.2f %%)" % (np.median(dt), spread, (np.median(t) / np.median(dt) - 1) * 100)
            line += "; max code difference to the detour %d" % diff
        lines.append(line)


def sitings(sr, tile, ratio):
    sr.tilesize = tile
    variants = [("%s->%s %s siting %d" % (FMT[b][1], FMT[b][1], rname(ratio), k), native(sr, b, ratio, k)) for b in (8, 10) for k in (0, 1, 2)]
    times = alternate(variants, reps, frames)[0]
    post = profiled(sr, variants)
    lines.extend(["", "C  chroma sitings at %s, tile %d" % (rname(ratio), tile),
                  "%-28s %9s %9s %9s %8s   %s" % ("variant", "median ms", "min ms", "max ms", "post_ms", "per repetition")])
    for n, _ in variants:
        t = times[n]
        line = "%-28s %9.2f %9.2f %9.2f %8.3f   %s" % (n, np.median(t), min(t), max(t), post[n]["post_ms"], " ".join("%.2f" % v for v in t))
        if not n.endswith("siting 0"):
            t0 = times[n[:-1] + "0"]
            spread, over = max(t0) - min(t0), np.median(t) - np.median(t0)
            line += "   vs siting 0: %+.2f ms (%+.2f %%), its spread %.2f ms: %s" % (
                over, over / np.median(t0) * 100, spread, "within" if over <= spread else "OUTSIDE by %.2f ms" % (over - spread))
        lines.append(line)
    sr.yuv_siting = 0


sr = context(False)
section(sr, "A  C2 device-resident", 200, [Fraction(3, 2), Fraction(9, 4), Fraction(3, 1)], reps, frames)
section(sr, "B  C2 device-resident", 201, [Fraction(4, 3)], reps, frames)
sitings(sr, 200, Fraction(3, 2))
sr.close()
if with_tta:
    sr = context(True)
    section(sr, "E  C5 (TTA x8) device-resident, 2 repetitions x 2 frames, recorded with no gate", 200, [Fraction(3, 2)], 2, 2, gated=False)
    sr.close()

text = "\n".join(lines)
print(text)
if out_path:
    with open(out_path, "w") as fh:
        fh.write(text + "\n")
