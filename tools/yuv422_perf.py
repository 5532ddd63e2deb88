"""C2 frame (1920 x 1080, tile 200), device-resident, as a YUV 4:2:2 surface in and out (RSR_FMT_NV16 / RSR_FMT_P210) -- and the detour
through RGB a caller needed before these formats existed:

    nv16->nv16    RSR_FMT_NV16 in and out (torch_io.upscale_yuv(..., chroma=422)), at out_scale 4 and 2
    p210->p210    RSR_FMT_P210 likewise
    detour nv16   torch: horizontal chroma upsampling + YUV -> RGB (fp16 CHW)  ->  torch_io.upscale f16 -> f16  ->  torch: RGB -> YUV, the
    detour p210   pair mean of the chroma, quantisation, interleaving -- the same arithmetic (BT.709 limited, centre siting) as torch ops
    nv12->nv12    the 4:2:0 surface of the same picture, the same run
    u8->u8        uint8 HWC in and out, the same run (what the default path costs on this board)
    p210 1280x1080 -> 1920x1080 at (3/2, 1)    the DVCPRO-HD job of the README

All variants alternate inside every repetition, on ONE torch stream, each timed with HIP events around `frames` back-to-back frames.  The
gate is printed per line: the native path must not be slower than its detour by more than the detour's own spread over the repetitions.
Then post_ms / pre_ms of the new launches from one profiled frame each.
    python tools/yuv422_perf.py [reps=5] [frames=4] [out=profiles/yuv422.txt]
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

reps, frames, out_path = 5, 4, None
for kv in sys.argv[1:]:
    k, v = kv.split("=")
    if k == "reps":
        reps = int(v)
    elif k == "frames":
        frames = int(v)
    elif k == "out":
        out_path = v

d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K", 42)
sr = R.RealSR(0)
sr.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
sr.tilesize = 200
w, h = 1920, 1080
KR, KB = 0.2126, 0.0722
KG = 1 - KR - KB


def to_yuv(rgb, bits, chroma):
    """float CHW RGB in [0, 1] -> the surface (uint8, or int16 holding code << 6): BT.709 limited range; chroma = the mean of the pair
    (4:2:2: a (2H, W) surface) or of the quad (4:2:0: (3H/2, W))."""
    k = 1 << (bits - 8)
    rgb = rgb.float()
    y = KR * rgb[0] + KG * rgb[1] + KB * rgb[2]
    m = F.avg_pool2d(rgb[None], (1, 2) if chroma == 422 else 2)[0]
    ym = KR * m[0] + KG * m[1] + KB * m[2]
    cb, cr = (m[2] - ym) / (2 * (1 - KB)), (m[0] - ym) / (2 * (1 - KR))
    yq = (y * (219 * k) + (16 * k + 0.5)).floor().clamp(0, (1 << bits) - 1)
    cq = (torch.stack([cb, cr], dim=-1) * (224 * k) + (128 * k + 0.5)).floor().clamp(0, (1 << bits) - 1)
    s = torch.cat([yq, cq.reshape(cq.shape[0], -1)], dim=0)
    return s.to(torch.uint8) if bits == 8 else (s.to(torch.int32) << 6).to(torch.int16)


def to_rgb422(s, bits):
    """The (2H, W) surface -> fp16 CHW RGB in [0, 1]: chroma upsampled along x (centre siting: the 3/4 - 1/4 weights, edges clamped)."""
    k = 1 << (bits - 8)
    hh = s.shape[0] // 2
    c = s.float() if bits == 8 else ((s.to(torch.int32) & 0xFFFF) >> 6).float()
    yn = (c[:hh] - 16 * k) / (219 * k)
    uv = c[hh:].reshape(hh, -1, 2).permute(2, 0, 1)
    uv = (F.interpolate(uv[None], scale_factor=(1, 2), mode="bilinear", align_corners=False)[0] - 128 * k) / (224 * k)
    r = yn + 2 * (1 - KR) * uv[1]
    g = yn - 2 * KB * (1 - KB) / KG * uv[0] - 2 * KR * (1 - KR) / KG * uv[1]
    b = yn + 2 * (1 - KB) * uv[0]
    return torch.stack([r, g, b]).clamp_(0, 1).half()


img = synth.make_image(3, w, h)
x8 = torch.from_numpy(img).cuda()
rgb0 = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).cuda().float() / 255
surf = {8: to_yuv(rgb0, 8, 422), 10: to_yuv(rgb0, 10, 422)}
surf420 = to_yuv(rgb0, 8, 420)
dv = to_yuv(torch.from_numpy(np.ascontiguousarray(synth.make_image(4, 1280, 1080).transpose(2, 0, 1))).cuda().float() / 255, 10, 422)
st = torch.cuda.Stream()


def at(scale, f):
    def g():
        sr.out_scale = scale
        return f()
    return g


def dvcpro():
    sr.out_ratio_xy = (Fraction(3, 2), Fraction(1))
    return torch_io.upscale_yuv(sr, dv, chroma=422)


def alternate(variants):
    """Every variant once per repetition, `frames` back-to-back frames between two HIP events: ms per frame, per repetition; and what each
    variant returned in the first warm-up pass."""
    times = {n: [] for n, _ in variants}
    with torch.cuda.stream(st):
        outs = {n: f() for n, f in variants}  # warm-up: plans, workspace, torch's kernels and allocator
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
    return times, outs


variants = []
for s_ in (4, 2):
    for bits, name in ((8, "nv16"), (10, "p210")):
        variants.append(("%s->%s x%d" % (name, name, s_), at(s_, lambda b=bits: torch_io.upscale_yuv(sr, surf[b], chroma=422))))
        variants.append(("detour %s x%d" % (name, s_), at(s_, lambda b=bits: to_yuv(torch_io.upscale(sr, to_rgb422(surf[b], b)), b, 422))))
    variants.append(("nv12->nv12 x%d" % s_, at(s_, lambda: torch_io.upscale_yuv(sr, surf420))))
    variants.append(("u8->u8 x%d" % s_, at(s_, lambda: torch_io.upscale(sr, x8))))
variants.append(("p210 dvcpro 3/2x1", dvcpro))
times, outs = alternate(variants)
assert tuple(outs["p210 dvcpro 3/2x1"].shape) == (2 * 1080, 1920)

prof = {}
sr.set_profiling(True)
with torch.cuda.stream(st):
    for n, f in variants:  # one profiled frame each
        if n.startswith("detour") or n.startswith("u8"):
            continue
        sr.get_profile(reset=True)
        f()
        st.synchronize()
        prof[n] = sr.get_profile(reset=True)
sr.set_profiling(False)

lines = ["C2 frame 1920 x 1080, tile 200, device-resident, BT.709 limited, %d repetitions x %d frames per variant, alternating, HIP events on one stream"
         % (reps, frames),
         "device: %s" % torch.cuda.get_device_name(0),
         "%-18s %9s %9s %9s   %s" % ("variant", "median ms", "min ms", "max ms", "per repetition")]
for n, _ in variants:
    t = times[n]
    line = "%-18s %9.2f %9.2f %9.2f   %s" % (n, np.median(t), min(t), max(t), " ".join("%.2f" % v for v in t))
    if n in prof:
        line += "   pre_ms %.3f post_ms %.3f" % (prof[n]["pre_ms"], prof[n]["post_ms"])
    if n.startswith(("nv16", "p210 ->", "p210->")):
        fmt, scale = n.split("->")[0], n.split()[-1]
        dt = times["detour %s %s" % (fmt, scale)]
        spread = max(dt) - min(dt)
        ok = np.median(t) <= np.median(dt) + spread
        code = lambda a: a.to(torch.int32) if a.dtype == torch.uint8 else (a.to(torch.int32) & 0xFFFF) >> 6  # noqa: E731
        diff = int((code(outs[n]) - code(outs["detour %s %s" % (fmt, scale)])).abs().max())
        line += "   gate: <= detour %.2f + its spread %.2f ms: %s (%+.2f %%); max code difference to the detour %d" % (
            np.median(dt), spread, "PASS" if ok else "FAIL", (np.median(t) / np.median(dt) - 1) * 100, diff)
    lines.append(line)
text = "\n".join(lines)
print(text)
if out_path:
    with open(out_path, "w") as fh:
        fh.write(text + "\n")
sr.close()
