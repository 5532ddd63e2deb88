"""C2 frame (1920 x 1080, tile 200), device-resident, as a decoder surface in and an encoder surface out -- and the detour through RGB a
caller needed before the NV12 / P010 formats existed:

    nv12->nv12    RSR_FMT_NV12 in and out (torch_io.upscale_yuv), at out_scale 4 and 2
    p010->p010    RSR_FMT_P010 likewise
    detour nv12   torch: chroma upsampling + YUV -> RGB (fp16 CHW)  ->  torch_io.upscale f16 -> f16  ->  torch: RGB -> YUV, avg_pool2d of the
    detour p010   chroma, quantisation, interleaving -- the same arithmetic (BT.709 limited, centre siting) as torch ops around the call
    u8->u8        uint8 HWC in and out, the same run (what the default path costs on this board)

All variants alternate inside every repetition, on ONE torch stream, each timed with HIP events around `frames` back-to-back frames.  The
gate is printed per line: the native path must not be slower than its detour by more than the detour's own spread over the repetitions.
    python tools/yuv_perf.py [reps=5] [frames=4] [out=profiles/yuv_io.txt] [option=value ...]

siting=1 measures the chroma sitings instead (option "yuv_siting"; profiles/yuv_siting.txt):
    nv12->nv12 / p010->p010 at out_scale 4 and 2, siting 1 (left) and 2 (top-left) against siting 0 (centre) in the same run, alternating;
    the expectation, printed per line: the frame time stays within siting 0's own spread over the repetitions.  post_ms of each from one
    profiled frame.  Then the size of the tile-edge effect (the sited chroma filters clamp at the first column / row of every tile's
    rectangle): the C2 golden frame's input as uint8, F32 out at x4 and x2, tests/yuv_siting_ref.encode with the tile grid against
    the same without it -- how many chroma samples differ and by how many codes, for NV12 and P010.  Reported, not gated.
    python tools/yuv_perf.py siting=1 [reps=5] [frames=4] [out=profiles/yuv_siting.txt]
The numpy restatement is the tests' (tests/yuv_siting_ref.py, on top of tests/yuv_ref.py): this mode puts tests/ on sys.path to import it.
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

reps, frames, out_path, opts, siting_mode = 5, 4, None, [], False
for kv in sys.argv[1:]:
    k, v = kv.split("=")
    if k == "reps":
        reps = int(v)
    elif k == "frames":
        frames = int(v)
    elif k == "out":
        out_path = v
    elif k == "siting":
        siting_mode = bool(int(v))
    else:
        opts.append((k, int(v)))

d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K", 42)
sr = R.RealSR(0)
sr.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
sr.tilesize = 200
for k, v in opts:
    sr.set_option(k, v)
w, h = 1920, 1080
KR, KB = 0.2126, 0.0722
KG = 1 - KR - KB


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


def to_rgb(s, bits):
    """The (3H/2, W) surface -> fp16 CHW RGB in [0, 1]: chroma upsampled bilinearly (centre siting: the 3/4 - 1/4 weights, edges clamped)."""
    k = 1 << (bits - 8)
    hh = s.shape[0] * 2 // 3
    c = s.float() if bits == 8 else ((s.to(torch.int32) & 0xFFFF) >> 6).float()
    yn = (c[:hh] - 16 * k) / (219 * k)
    uv = c[hh:].reshape(hh // 2, -1, 2).permute(2, 0, 1)
    uv = (F.interpolate(uv[None], scale_factor=2, mode="bilinear", align_corners=False)[0] - 128 * k) / (224 * k)
    r = yn + 2 * (1 - KR) * uv[1]
    g = yn - 2 * KB * (1 - KB) / KG * uv[0] - 2 * KR * (1 - KR) / KG * uv[1]
    b = yn + 2 * (1 - KB) * uv[0]
    return torch.stack([r, g, b]).clamp_(0, 1).half()


img = synth.make_image(3, w, h)
x8 = torch.from_numpy(img).cuda()
rgb0 = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).cuda().float() / 255
surf = {8: to_yuv(rgb0, 8), 10: to_yuv(rgb0, 10)}
st = torch.cuda.Stream()


def at(scale, f):
    def g():
        sr.out_scale = scale
        return f()
    return g


def finish(text):
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")
    sr.close()


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


def siting_report():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import yuv_siting_ref as ref  # noqa: E402

    def sited(scale, k, bits):
        def g():
            sr.out_scale, sr.yuv_siting = scale, k
            return torch_io.upscale_yuv(sr, surf[bits])
        return g

    cases = [(s_, bits, name) for s_ in (4, 2) for bits, name in ((8, "nv12"), (10, "p010"))]
    variants = [("%s->%s x%d siting %d" % (name, name, s_, k), sited(s_, k, bits)) for s_, bits, name in cases for k in (0, 1, 2)]
    times = alternate(variants)[0]
    post = {}
    sr.set_profiling(True)
    with torch.cuda.stream(st):
        for n, f in variants:  # one profiled frame each
            sr.get_profile(reset=True)
            f()
            st.synchronize()
            post[n] = sr.get_profile(reset=True)
    sr.set_profiling(False)
    lines = ["C2 frame 1920 x 1080, tile 200, device-resident, BT.709 limited, %d repetitions x %d frames per variant, alternating, HIP events on one stream"
             % (reps, frames), "device: %s" % torch.cuda.get_device_name(0),
             "%-26s %9s %9s %9s %8s %8s   %s" % ("variant", "median ms", "min ms", "max ms", "pre_ms", "post_ms", "per repetition")]
    for n, _ in variants:
        t = times[n]
        line = "%-26s %9.2f %9.2f %9.2f %8.3f %8.3f   %s" % (n, np.median(t), min(t), max(t), post[n]["pre_ms"], post[n]["post_ms"], " ".join("%.2f" % v for v in t))
        if not n.endswith("siting 0"):
            t0 = times[n[:-1] + "0"]
            spread, over = max(t0) - min(t0), np.median(t) - np.median(t0)
            line += "   vs siting 0: %+.2f ms (%+.2f %%), its spread %.2f ms: %s" % (
                over, over / np.median(t0) * 100, spread, "within" if over <= spread else "OUTSIDE by %.2f ms" % (over - spread))
        lines.append(line)
    # the tile-edge effect
    sr.yuv_siting = 0
    src = torch.from_numpy(synth.make_image(1235, w, h)).cuda()
    lines += ["", "Tile-edge effect: input of the C2 golden frame (uint8, 1920 x 1080, tile 200), F32 out; encode(d, siting, tilesize * out_scale) against",
              "encode(d, siting, 0) in numpy (tests/yuv_siting_ref.py): chroma samples that differ / all chroma samples, largest code difference"]
    for s_ in (4, 2):
        sr.out_scale = s_
        dst = torch.empty((3, h * s_, w * s_), dtype=torch.float32, device="cuda")
        sr.process_device_fmt(src.data_ptr(), R.RSR_FMT_U8_HWC, w, h, 3, dst.data_ptr(), R.RSR_FMT_F32_CHW)
        torch.cuda.synchronize()
        dd = dst.cpu().numpy()
        del dst
        for k in (1, 2):
            for bits, name in ((8, "nv12"), (10, "p010")):
                grid, free = ref.encode(dd, k, 200 * s_, 709, 0, bits)[1], ref.encode(dd, k, 0, 709, 0, bits)[1]
                diff = np.abs(grid - free)
                dm, step = diff.any(axis=2), 100 * s_
                first = np.zeros_like(dm)
                first[:, ::step] = True
                if k == 2:
                    first[::step, :] = True
                on_edges = not (dm & ~first).any()
                lines.append("x%d siting %d %s: %d of %d samples differ (%.4f %%), max %d codes, mean of the differing %.2f; all on tile-first chroma columns%s: %s" % (
                    s_, k, name, int((diff > 0).sum()), diff.size, 100.0 * (diff > 0).mean(), int(diff.max()),
                    float(diff[diff > 0].mean()) if (diff > 0).any() else 0.0, " / rows" if k == 2 else "", on_edges))
    finish("\n".join(lines))


if siting_mode:
    siting_report()
    sys.exit(0)

variants = []
for s_ in (4, 2):
    for bits, name in ((8, "nv12"), (10, "p010")):
        variants.append(("%s->%s x%d" % (name, name, s_), at(s_, lambda b=bits: torch_io.upscale_yuv(sr, surf[b]))))
        variants.append(("detour %s x%d" % (name, s_), at(s_, lambda b=bits: to_yuv(torch_io.upscale(sr, to_rgb(surf[b], b)), b))))
    variants.append(("u8->u8 x%d" % s_, at(s_, lambda: torch_io.upscale(sr, x8))))
times, outs = alternate(variants)

lines = ["C2 frame 1920 x 1080, tile 200, device-resident, BT.709 limited, %d repetitions x %d frames per variant, alternating, HIP events on one stream%s"
         % (reps, frames, "".join(" %s=%d" % kv for kv in opts)),
         "device: %s" % torch.cuda.get_device_name(0),
         "%-16s %9s %9s %9s   %s" % ("variant", "median ms", "min ms", "max ms", "per repetition")]
for n, _ in variants:
    t = times[n]
    line = "%-16s %9.2f %9.2f %9.2f   %s" % (n, np.median(t), min(t), max(t), " ".join("%.2f" % v for v in t))
    if "->" in n and not n.startswith("u8"):
        fmt, scale = n.split("->")[0], n.split()[-1]
        dt = times["detour %s %s" % (fmt, scale)]
        spread = max(dt) - min(dt)
        ok = np.median(t) <= np.median(dt) + spread
        code = lambda a: a.to(torch.int32) if a.dtype == torch.uint8 else (a.to(torch.int32) & 0xFFFF) >> 6  # noqa: E731
        diff = int((code(outs[n]) - code(outs["detour %s %s" % (fmt, scale)])).abs().max())
        line += "   gate: <= detour %.2f + its spread %.2f ms: %s (%+.2f %%); max code difference to the detour %d" % (
            np.median(dt), spread, "PASS" if ok else "FAIL", (np.median(t) / np.median(dt) - 1) * 100, diff)
    lines.append(line)
finish("\n".join(lines))
