"""post_ms (rsr_get_profile) and a SHA-256 of the output bytes for one configuration per post-processing kernel family, on a 1920 x 1080
synthetic frame at tile 200: the A/B instrument for changes to the post kernels of csrc/kernels.hip.  Run it once per build (RSR_LIB selects
the library, as in tools/ab_multi.sh), each run a process of its own; equal hashes = equal bytes, and the post_ms columns compare.
    [RSR_LIB=other/librealsr_hip.so] python tools/post_ms.py [frames=3] [tta_frames=3] [only=area]
only: run the lines whose name contains that text (a closer look at one family with more frames).
One line per configuration: name, post_ms of each profiled frame (after one warm-up frame; a TTA frame takes 0.7 s), their median, the hash."""
import hashlib
import os
import sys
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import realsr_ncnn_vulkan_amd as R  # noqa: E402
from realsr_ncnn_vulkan_amd import synth, torch_io  # noqa: E402

frames, tta_frames, only = 3, 3, ""
for kv in sys.argv[1:]:
    k, v = kv.split("=")
    if k == "frames":
        frames = int(v)
    elif k == "tta_frames":
        tta_frames = int(v)
    elif k == "only":
        only = v

W, H = 1920, 1080
d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K", 42)
rgba = synth.make_image(1239, W, H, 4)
x8 = torch.from_numpy(np.ascontiguousarray(rgba[..., :3])).cuda()
x8a = torch.from_numpy(rgba).cuda()
x16 = (x8.permute(2, 0, 1).float() * (1 / 255.0)).half().contiguous()
# any bytes are a surface: Y from one channel, the (U, V) pairs from two channels of a half-size image; P010 keeps the code in the high bits
uv = synth.make_image(7, W // 2, H // 2)[..., :2].reshape(H // 2, W)
nv12 = torch.from_numpy(np.concatenate([rgba[..., 1], uv], axis=0)).cuda()
p010 = (nv12.to(torch.int32) << 8).to(torch.int16)

R3_2, R9_4 = Fraction(3, 2), Fraction(9, 4)
# (name, TTA, input, function, output ratio, yuv_siting, options set for the line and reset to 0 behind it)
CASES = [
    ("postproc_tiles       rgba u8", False, x8a, torch_io.upscale, 4, 0, {}),
    ("postproc_tiles_lds   rgb u8 tta", True, x8, torch_io.upscale, 4, 0, {}),
    ("postproc_tiles       rgb u8 tta dbg 32768", True, x8, torch_io.upscale, 4, 0, {"dbg": 32768}),
    ("box   x2   rgb u8", False, x8, torch_io.upscale, 2, 0, {}),
    ("box   x1   rgb u8", False, x8, torch_io.upscale, 1, 0, {}),
    ("box   x2   rgb u8 tta", True, x8, torch_io.upscale, 2, 0, {}),
    ("box   x1   rgb u8 tta", True, x8, torch_io.upscale, 1, 0, {}),
    ("box   x1   rgba u8", False, x8a, torch_io.upscale, 1, 0, {}),
    ("area  3/2  rgb u8", False, x8, torch_io.upscale, R3_2, 0, {}),
    ("area  9/4  rgb u8", False, x8, torch_io.upscale, R9_4, 0, {}),
    ("area  3/2  rgb u8 tta", True, x8, torch_io.upscale, R3_2, 0, {}),
    ("area  9/4  rgb u8 tta", True, x8, torch_io.upscale, R9_4, 0, {}),
    ("area  3/2  rgba u8", False, x8a, torch_io.upscale, R3_2, 0, {}),
    ("area  3/2  f16 chw precise", False, x16, torch_io.upscale, R3_2, 0, {"precise": 1}),
] + [("yuv   x%d   nv12 siting %d" % (s, k), False, nv12, torch_io.upscale_yuv, s, k, {}) for s in (4, 2, 1) for k in (0, 2)] + [
    ("yuv   x4   p010", False, p010, torch_io.upscale_yuv, 4, 0, {}),
    ("yuv   x1   nv12 siting 1 precise", False, nv12, torch_io.upscale_yuv, 1, 1, {"precise": 1}),
    ("yuv   3/2  nv12 siting 0", False, nv12, torch_io.upscale_yuv, R3_2, 0, {}),
    ("yuv   3/2  nv12 siting 2", False, nv12, torch_io.upscale_yuv, R3_2, 2, {}),
    ("yuv   3/2  p010", False, p010, torch_io.upscale_yuv, R3_2, 0, {}),
    ("yuv   3/2  nv12 tta", True, nv12, torch_io.upscale_yuv, R3_2, 0, {}),
]
CASES = [c for c in CASES if only in c[0]]

print("post_ms: %d x %d, tile 200, %d profiled frames per line (TTA: %d); library %s; device %s" % (W, H, frames, tta_frames, R.LIB_PATH, torch.cuda.get_device_name(0)), flush=True)
for tta in sorted({c[1] for c in CASES}):
    sr = R.RealSR(0, tta_mode=tta)
    sr.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
    sr.tilesize = 200
    for name, _, x, f, ratio, siting, opts in (c for c in CASES if c[1] == tta):
        sr.out_ratio, sr.yuv_siting = ratio, siting
        for key, val in opts.items():
            sr.set_option(key, val)
        y = f(sr, x)  # warm-up: plans, workspace
        torch.cuda.synchronize()
        sr.set_profiling(True)
        sr.get_profile(reset=True)
        ms = []
        for _ in range(tta_frames if tta else frames):
            y = f(sr, x)
            torch.cuda.synchronize()
            ms.append(sr.get_profile(reset=True)["post_ms"])
        sr.set_profiling(False)
        for key in opts:
            sr.set_option(key, 0)
        digest = hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()
        print("%-42s post_ms %s  median %.4f  sha256 %s" % (name, " ".join("%.4f" % v for v in ms), float(np.median(ms)), digest[:32]), flush=True)
        del y
    sr.close()
