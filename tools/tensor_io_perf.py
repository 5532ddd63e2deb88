"""C2 frame (1920 x 1080, tile 200), device-resident, per pixel format of rsr_process_device_fmt -- and the detour through uint8 a torch user
needed before the planar float formats existed:

    u8->u8        uint8 HWC in, uint8 HWC out (rsr_process_device)
    f16->f16      planar fp16 in [0, 1] in and out
    f32->f32      planar fp32 likewise
    detour f16    fp16 CHW tensor -> quantise + permute (torch) -> rsr_process_device -> permute + convert to fp16 CHW (torch)
    detour f32    the same around an fp32 tensor

All variants alternate inside every repetition, on ONE torch stream, each timed with HIP events around `frames` back-to-back frames.
    python tools/tensor_io_perf.py [reps=5] [frames=4] [out=profiles/tensor_io.txt] [option=value ...]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import realsr_ncnn_vulkan_amd as R  # noqa: E402
from realsr_ncnn_vulkan_amd import synth, torch_io  # noqa: E402

reps, frames, out_path, opts = 5, 4, None, []
for kv in sys.argv[1:]:
    k, v = kv.split("=")
    if k == "reps":
        reps = int(v)
    elif k == "frames":
        frames = int(v)
    elif k == "out":
        out_path = v
    else:
        opts.append((k, int(v)))

d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K", 42)
sr = R.RealSR(0)
sr.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
sr.tilesize = 200
for k, v in opts:
    sr.set_option(k, v)
w, h = 1920, 1080
img = synth.make_image(3, w, h)
x8 = torch.from_numpy(img).cuda()
x32 = torch.from_numpy(np.ascontiguousarray((img.astype(np.float32) * np.float32(1 / 255.0)).transpose(2, 0, 1))).cuda()
x16 = x32.half()
st = torch.cuda.Stream()


def detour(x):
    """What a float CHW pipeline had to do around the uint8-only entry point: two extra passes over the input, two over the 16x output."""
    q = (x.float() * 255.0 + 0.5).clamp_(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()
    y = torch_io.upscale(sr, q)
    return (y.permute(2, 0, 1).to(x.dtype) * (1.0 / 255.0)).contiguous()


variants = [("u8->u8", lambda: torch_io.upscale(sr, x8)), ("f16->f16", lambda: torch_io.upscale(sr, x16)),
            ("f32->f32", lambda: torch_io.upscale(sr, x32)), ("detour f16", lambda: detour(x16)), ("detour f32", lambda: detour(x32))]
times = {n: [] for n, _ in variants}
with torch.cuda.stream(st):
    outs = {n: f() for n, f in variants}  # warm-up: plan, workspace, torch's kernels and allocator
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

# the float outputs against the uint8 one (default mode: exact), and what the detour loses
q = lambda t: (t.float() * 255.0 + 0.5).floor().clamp(0, 255).to(torch.uint8)  # noqa: E731
ref = outs["u8->u8"].permute(2, 0, 1)
same16, same32 = bool(torch.equal(q(outs["f16->f16"]), ref)), bool(torch.equal(q(outs["f32->f32"]), ref))
lost = float((outs["detour f32"] - outs["f32->f32"]).abs().max())
lines = ["C2 frame 1920 x 1080, tile 200, device-resident, %d repetitions x %d frames per variant, alternating, HIP events on one stream%s"
         % (reps, frames, "".join(" %s=%d" % kv for kv in opts)),
         "device: %s" % torch.cuda.get_device_name(0),
         "%-12s %9s %9s %9s   %s" % ("variant", "median ms", "min ms", "max ms", "per repetition")]
base = float(np.median(times["u8->u8"]))
for n, _ in variants:
    t = times[n]
    lines.append("%-12s %9.2f %9.2f %9.2f   %s   (%+.2f %% vs u8->u8)" % (n, np.median(t), min(t), max(t), " ".join("%.2f" % v for v in t),
                                                                         (np.median(t) / base - 1) * 100))
lines.append("spread of u8->u8 over the repetitions: %.2f %% (max - min over median)" % ((max(times["u8->u8"]) - min(times["u8->u8"])) / base * 100))
lines.append("quantised f16 output == uint8 output: %s; quantised f32 output == uint8 output: %s" % (same16, same32))
lines.append("max |detour f32 - direct f32| = %.3e (the output's uint8 hop: half a code = 1.96e-3)" % lost)
text = "\n".join(lines)
print(text)
if out_path:
    with open(out_path, "w") as fh:
        fh.write(text + "\n")
sr.close()
