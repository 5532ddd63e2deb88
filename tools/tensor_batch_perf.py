"""Tensor batches and strided views (rsr_process_device_batch, torch_io.upscale) against what a tensor pipeline had to do before:

    A  small frames   16 x 256 x 256 and 16 x 128 x 128, f16 -> f16, tile 128: torch_io.upscale of the (16, 3, H, W) tensor (ONE batch
                      call: merged tile batches) against a loop of 16 rsr_process_device_fmt calls
    B  large frames   2 x 1920 x 1080 at tile 200 (a frame fills the chip by itself: the batch call is two tile batches, like the loop)
    C  strided views  a 1920 x 1080 crop view of a (3, 1200, 2048) tensor written into a window of a canvas, in place, against
                      .contiguous() + a packed call + a copy into the canvas

All variants of a section alternate inside every repetition, on ONE torch stream, each timed with HIP events.
    python tools/tensor_batch_perf.py [reps=7] [out=profiles/tensor_batch.txt] [option=value ...]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import realsr_ncnn_vulkan_amd as R  # noqa: E402
from realsr_ncnn_vulkan_amd import synth, torch_io  # noqa: E402

reps, out_path, opts = 7, None, []
for kv in sys.argv[1:]:
    k, v = kv.split("=")
    if k == "reps":
        reps = int(v)
    elif k == "out":
        out_path = v
    else:
        opts.append((k, int(v)))

d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K", 42)
sr = R.RealSR(0)
sr.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
for k, v in opts:
    sr.set_option(k, v)
st = torch.cuda.Stream()
F16 = R.RSR_FMT_F16_CHW
lines = ["rsr_process_device_batch / torch_io.upscale, device-resident fp16, %d repetitions per variant, alternating, HIP events on one stream%s"
         % (reps, "".join(" %s=%d" % kv for kv in opts)), "device: %s" % torch.cuda.get_device_name(0)]


def planar(seed, w, h, n=None):
    imgs = [synth.make_image(seed + i, w, h) for i in range(n or 1)]
    x = np.stack([np.ascontiguousarray((im.astype(np.float32) * np.float32(1 / 255.0)).transpose(2, 0, 1)) for im in imgs])
    t = torch.from_numpy(x).cuda().half()
    return t if n else t[0]


def loop(x):
    """The parent's way for an (N, 3, H, W) tensor: N rsr_process_device_fmt calls on the current stream."""
    n, _, h, w = x.shape
    y = torch.empty((n, 3, 4 * h, 4 * w), dtype=x.dtype, device=x.device)
    cur = torch.cuda.current_stream().cuda_stream
    for xi, yi in zip(x, y):
        sr.process_device_fmt(xi.data_ptr(), F16, w, h, 3, yi.data_ptr(), F16, stream=cur)
    return y


def measure(title, variants, mpix, inner=1):
    """variants: [(name, f)]; the first is the baseline; mpix: OUTPUT megapixels of one run (the project's metric).  Returns the outputs
    of the warm-up."""
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
                for _ in range(inner):
                    y = f()
                e1.record(st)
                e1.synchronize()
                del y
                times[n].append(e0.elapsed_time(e1) / inner)
    st.synchronize()
    lines.append("")
    lines.append(title)
    lines.append("%-22s %9s %9s %9s %10s   %s" % ("variant", "median ms", "min ms", "max ms", "out Mpix/s", "per repetition"))
    base = times[variants[0][0]]
    bmed = float(np.median(base))
    for n, _ in variants:
        t = times[n]
        lines.append("%-22s %9.3f %9.3f %9.3f %10.1f   %s   (%+.2f %% vs %s)" % (n, np.median(t), min(t), max(t), mpix / np.median(t) * 1e3,
                                                                              " ".join("%.3f" % v for v in t), (np.median(t) / bmed - 1) * 100, variants[0][0]))
    lines.append("spread of %s over the repetitions: %.2f %% (max - min over median)" % (variants[0][0], (max(base) - min(base)) / bmed * 100))
    return outs


# ---- A: small frames ----
sr.tilesize = 128
for side in (256, 128):
    x = planar(100 + side, side, side, 16)
    g0 = sr.get_stat("batch_groups")
    outs = measure("A  16 x %d x %d f16 -> f16, tile 128" % (side, side),
                   [("loop of 16 calls", lambda: loop(x)), ("upscale (one batch)", lambda: torch_io.upscale(sr, x))], 16 * 16 * side * side / 1e6, inner=4)
    lines.append("tile batches per batch call: %d; outputs byte-identical to the loop's: %s"
                 % (round((sr.get_stat("batch_groups") - g0) / (4 * reps + 2)), bool(torch.equal(outs["loop of 16 calls"], outs["upscale (one batch)"]))))

# ---- B: large frames ----
sr.tilesize = 200
xb = planar(3, 1920, 1080, 2)
outs = measure("B  2 x 1920 x 1080 f16 -> f16, tile 200 (not merged: the same work)",
               [("loop of 2 calls", lambda: loop(xb)), ("upscale (one batch)", lambda: torch_io.upscale(sr, xb))], 16 * 2 * 1920 * 1080 / 1e6)
lines.append("outputs byte-identical: %s" % bool(torch.equal(outs["loop of 2 calls"], outs["upscale (one batch)"])))
del outs, xb

# ---- C: strided views ----
surface = torch.rand((3, 1200, 2048), device="cuda").half()
view = surface[:, 61:61 + 1080, 33:33 + 1920]
view.copy_(planar(3, 1920, 1080))
canvas = torch.zeros((3, 4 * 1200, 4 * 2048), dtype=torch.float16, device="cuda")
window = canvas[:, 4 * 61:4 * (61 + 1080), 4 * 33:4 * (33 + 1920)]
canvas2 = torch.zeros_like(canvas)
window2 = canvas2[:, 4 * 61:4 * (61 + 1080), 4 * 33:4 * (33 + 1920)]


def detour():
    window2.copy_(torch_io.upscale(sr, view.contiguous()))
    return window2


assert torch_io.describe(view) is not None and torch_io.describe(window) is not None
measure("C  1920 x 1080 crop view of a (3, 1200, 2048) tensor into a window of a (3, 4800, 8192) canvas, f16, tile 200",
        [("contiguous + copy", detour), ("strided, in place", lambda: torch_io.upscale(sr, view, out=window))], 16 * 1920 * 1080 / 1e6)
lines.append("canvases byte-identical: %s" % bool(torch.equal(canvas, canvas2)))

text = "\n".join(lines)
print(text)
if out_path:
    with open(out_path, "w") as fh:
        fh.write(text + "\n")
sr.close()
