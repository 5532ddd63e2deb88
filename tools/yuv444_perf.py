"""C2 frame (1920 x 1080, tile 200), device-resident, as a planar YUV 4:4:4 image in and out (RSR_FMT_YUV444P / RSR_FMT_YUV444P10) -- and
the detour through RGB a caller needed before these formats existed:

    444p->444p      RSR_FMT_YUV444P in and out (torch_io.upscale_yuv(..., chroma=444)), at out_scale 4 and 2
    444p10->444p10  RSR_FMT_YUV444P10 likewise
    detour 444p     torch: YUV -> RGB (fp16 CHW)  ->  torch_io.upscale f16 -> f16  ->  torch: RGB -> YUV, quantisation -- the same
    detour 444p10   arithmetic (BT.709 limited) as torch ops
    nv16->nv16      the 4:2:2 surface of the same picture, the same run
    u8->u8          uint8 HWC in and out, the same run (what the default path costs on this board)

All variants alternate inside every repetition, on ONE torch stream, each timed with HIP events around `frames` back-to-back frames.  The
gate is printed per line: the native path must not be slower than its detour by more than the detour's own spread over the repetitions.
Then post_ms / pre_ms of the new launches from profiled frames (the least of three, one frame each), with the default thread shape of
postproc_tiles_yuv444 (two pixels per thread at out_scale 4, one at 2) and with one / two pixels forced (engine option "dbg" 32768 / 65536),
next to NV16's of the same run.  No gate on post_ms.
    python tools/yuv444_perf.py [reps=5] [frames=4] [out=profiles/yuv444.txt]
"""
import os
import sys

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


def to_yuv444(rgb, bits):
    """float CHW RGB in [0, 1] -> (3, H, W) codes (uint8, or int16 holding the code in its low bits): BT.709 limited range."""
    k = 1 << (bits - 8)
    rgb = rgb.float()
    y = KR * rgb[0] + KG * rgb[1] + KB * rgb[2]
    cb, cr = (rgb[2] - y) / (2 * (1 - KB)), (rgb[0] - y) / (2 * (1 - KR))
    yq = (y * (219 * k) + (16 * k + 0.5)).floor()
    cq = (torch.stack([cb, cr]) * (224 * k) + (128 * k + 0.5)).floor()
    s = torch.cat([yq[None], cq]).clamp(0, (1 << bits) - 1)
    return s.to(torch.uint8) if bits == 8 else s.to(torch.int16)


def to_rgb444(s, bits):
    """(3, H, W) codes -> fp16 CHW RGB in [0, 1]."""
    k = 1 << (bits - 8)
    c = s.float() if bits == 8 else (s.to(torch.int32) & 1023).float()
    yn = (c[0] - 16 * k) / (219 * k)
    cb, cr = (c[1] - 128 * k) / (224 * k), (c[2] - 128 * k) / (224 * k)
    r = yn + 2 * (1 - KR) * cr
    g = yn - 2 * KB * (1 - KB) / KG * cb - 2 * KR * (1 - KR) / KG * cr
    b = yn + 2 * (1 - KB) * cb
    return torch.stack([r, g, b]).clamp_(0, 1).half()


def to_nv16(rgb):
    rgb = rgb.float()
    y = KR * rgb[0] + KG * rgb[1] + KB * rgb[2]
    m = F.avg_pool2d(rgb[None], (1, 2))[0]
    ym = KR * m[0] + KG * m[1] + KB * m[2]
    cb, cr = (m[2] - ym) / (2 * (1 - KB)), (m[0] - ym) / (2 * (1 - KR))
    yq = (y * 219 + 16.5).floor().clamp(0, 255)
    cq = (torch.stack([cb, cr], dim=-1) * 224 + 128.5).floor().clamp(0, 255)
    return torch.cat([yq, cq.reshape(cq.shape[0], -1)], dim=0).to(torch.uint8)


img = synth.make_image(3, w, h)
x8 = torch.from_numpy(img).cuda()
rgb0 = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).cuda().float() / 255
img444 = {8: to_yuv444(rgb0, 8), 10: to_yuv444(rgb0, 10)}
surf422 = to_nv16(rgb0)
st = torch.cuda.Stream()


def at(scale, f, dbg=0):
    def g():
        sr.out_scale = scale
        sr.set_option("dbg", dbg)
        try:
            return f()
        finally:
            sr.set_option("dbg", 0)
    return g


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
    for bits, name in ((8, "444p"), (10, "444p10")):
        variants.append(("%s->%s x%d" % (name, name, s_), at(s_, lambda b=bits: torch_io.upscale_yuv(sr, img444[b], chroma=444))))
        variants.append(("detour %s x%d" % (name, s_), at(s_, lambda b=bits: to_yuv444(torch_io.upscale(sr, to_rgb444(img444[b], b)), b))))
    variants.append(("nv16->nv16 x%d" % s_, at(s_, lambda: torch_io.upscale_yuv(sr, surf422, chroma=422))))
    variants.append(("u8->u8 x%d" % s_, at(s_, lambda: torch_io.upscale(sr, x8))))
times, outs = alternate(variants)
assert tuple(outs["444p10->444p10 x2"].shape) == (3, 2 * h, 2 * w)

prof = {}
sr.set_profiling(True)
with torch.cuda.stream(st):
    shapes = [(n, f) for n, f in variants if not n.startswith(("detour", "u8"))]
    for s_ in (4, 2):  # either thread shape of the new post kernels forced: one pixel, two neighbouring pixels per thread
        for bits, name in ((8, "444p"), (10, "444p10")):
            for px, dbg in ((1, 32768), (2, 65536)):
                shapes.append(("%s->%s x%d, %d px/thread" % (name, name, s_, px), at(s_, lambda b=bits: torch_io.upscale_yuv(sr, img444[b], chroma=444), dbg)))
    for n, f in shapes:  # three profiled frames each (after a warm-up frame of the same shape): the one with the least post_ms
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

lines = ["C2 frame 1920 x 1080, tile 200, device-resident, BT.709 limited, %d repetitions x %d frames per variant, alternating, HIP events on one stream"
         % (reps, frames),
         "device: %s" % torch.cuda.get_device_name(0),
         "%-20s %9s %9s %9s   %s" % ("variant", "median ms", "min ms", "max ms", "per repetition")]
met = []
for n, _ in variants:
    t = times[n]
    line = "%-20s %9.2f %9.2f %9.2f   %s" % (n, np.median(t), min(t), max(t), " ".join("%.2f" % v for v in t))
    if n in prof:
        line += "   pre_ms %.3f post_ms %.3f" % (prof[n]["pre_ms"], prof[n]["post_ms"])
    if n.startswith("444p"):
        fmt, scale = n.split("->")[0], n.split()[-1]
        dt = times["detour %s %s" % (fmt, scale)]
        spread = max(dt) - min(dt)
        ok = bool(np.median(t) <= np.median(dt) + spread)
        met.append(ok)
        code = lambda a: a.to(torch.int32) & 0xFFFF  # noqa: E731
        diff = int((code(outs[n]) - code(outs["detour %s %s" % (fmt, scale)])).abs().max())
        line += "   gate: <= detour %.2f + its spread %.2f ms: %s (%+.2f %%); max code difference to the detour %d" % (
            np.median(dt), spread, "met" if ok else "NOT MET", (np.median(t) / np.median(dt) - 1) * 100, diff)
    lines.append(line)
lines.append("gates met: %d of %d" % (sum(met), len(met)))
lines.append("post_ms / pre_ms of a profiled frame (the least post_ms of three), postproc_tiles_yuv444 at its default and at either forced thread shape, next to NV16's postproc_tiles_yuv (no gate):")
for n, _ in shapes:
    lines.append("%-34s pre_ms %.3f post_ms %.3f" % (n, prof[n]["pre_ms"], prof[n]["post_ms"]))
text = "\n".join(lines)
print(text)
if out_path:
    with open(out_path, "w") as fh:
        fh.write(text + "\n")
sr.close()
