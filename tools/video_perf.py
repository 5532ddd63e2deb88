"""Three-plane frames and the host video session (rsr_pack_planes, rsr_unpack_planes, rsr_video_*) on 1920 x 1080 frames at tile 200.

    A  pack and unpack  the launches alone, HIP events around 10 calls: pack on a 1080p frame, unpack on its 7680 x 4320 result, NV12 and P010,
                        against the torch detour on the same bytes -- pack: torch.stack((u, v), -1) into the surface (P010: with the mask and
                        the shift); unpack: strided slices with .contiguous() (P010: with the shift).
                        gate: not slower than the detour by more than the detour's own spread.  GB/s: every byte read once and written once
                        (profiles/sequence.txt has propagate_rects' figure for the same kind of pass).
    B  the session, all tiles changing   NV12 -> NV12 at x4 and x2, window 8, pinned planes, host -> host, wall time per frame, against the sum,
                        measured in the same run, of the device-resident plain call, the pinned H2D and D2H copies of the same bytes and
                        the two launches of A.
                        gate: at most that sum plus its spread.  Pageable planes are reported, not gated; so is the share of the frame
                        the copies take: what overlapping one window's copies with the next window's compute could win back.
    C  the session, static content       1 and 6 changed tiles of 60 per frame: host -> host per frame beside torch_io.upscale_sequence
                        device-resident on the same frames, and the copies.  Reported.

All variants of a section alternate inside every repetition; medians over the repetitions after a warm-up; spread = max - min; every gate
on its own line.  (profiles/video.txt carries two more sections this tool does not write, each with its command: D, bench.py of the
parent commit against this one, and E, the compiler's resource report.)
                        The CLI end to end on 16-frame Y4M files (1 and 6 changed tiles per frame, and every tile): wall time of the
                        process, and per frame with the time of a 1-frame file (start-up, model load, the first full frame) taken off.
    python tools/video_perf.py [reps=5] [out=profiles/video.txt] [append=0] [only=cli]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import realsr_ncnn_vulkan_amd as R  # noqa: E402
from realsr_ncnn_vulkan_amd import synth, torch_io  # noqa: E402

reps, out_path, append, only = 5, None, 0, ""
for kv in sys.argv[1:]:
    k, v = kv.split("=")
    if k == "reps":
        reps = int(v)
    elif k == "out":
        out_path = v
    elif k == "append":
        append = int(v)
    elif k == "only":
        only = v  # only=cli: section C's CLI lines alone (appended to a profile the other sections are already in)

W, H, TILE, NF = 1920, 1080, 200, 8
NV12, P010 = R.RSR_FMT_NV12, R.RSR_FMT_P010
d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K", 42)
st = torch.cuda.Stream()
lines = ["rsr_pack_planes / rsr_unpack_planes / rsr_video_*: 1920 x 1080 frames at tile 200 (60 tiles), medians of %d repetitions, alternating, "
         "after a warm-up" % reps, "device: %s" % torch.cuda.get_device_name(0)]
sr = R.RealSR(0)
sr.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
sr.tilesize = TILE
rng = np.random.default_rng(5)


def stats(t):
    return float(np.median(t)), min(t), max(t)


def gate(text, met):
    lines.append("gate: %-110s %s" % (text, "met" if met else "NOT MET"))


_mm = torch.randn(8192, 8192, dtype=torch.float16, device="cuda")


def timed(variants, n_calls, blocker=True):
    """HIP events on the stream around n_calls calls; ms per call, per repetition; the first round is the warm-up.  blocker: a few ms of
    matrix products are enqueued in front of the first event, so that the host has queued all n_calls before the GPU reaches them:
    the bracket then holds GPU time, not the pace at which Python issues launches."""
    times = {n: [] for n, _ in variants}
    with torch.cuda.stream(st):
        for rep in range(reps + 1):
            for n, f in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if blocker:
                    for _ in range(6):
                        torch.mm(_mm, _mm)
                e0.record(st)
                for _ in range(n_calls):
                    f()
                e1.record(st)
                e1.synchronize()
                if rep:
                    times[n].append(e0.elapsed_time(e1) / n_calls)
    return times


def cli_section():
    import subprocess
    import tempfile
    cli = os.path.join(ROOT, "realsr-ncnn-vulkan_amd", "bin", "realsr-hip")
    out = ["", "C  the CLI end to end: realsr-hip -i in.y4m -o out.y4m -t 200 on 16-frame 1920 x 1080 C420mpeg2 files (x4, window 8), wall time of the process, median of %d" % reps,
           "%-34s %12s %12s %14s" % ("content", "16 frames s", "1 frame s", "ms per frame")]
    with tempfile.TemporaryDirectory() as tmp:
        def write(path, frames):
            with open(path, "wb") as fh:
                fh.write(b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420mpeg2\n" % (W, H))
                for f in frames:
                    fh.write(b"FRAME\n" + b"".join(p.tobytes() for p in f))

        def run(path):
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                subprocess.run([cli, "-i", path, "-o", os.path.join(tmp, "out.y4m"), "-m", d, "-t", str(TILE)], check=True, capture_output=True)
                ts.append(time.perf_counter() - t0)
            return float(np.median(ts))

        for label, k in (("1 changed tile of 60 per frame", 1), ("6 changed tiles of 60 per frame", 6), ("every tile changing", None)):
            frames = make_frames(k, 15)
            write(os.path.join(tmp, "v16.y4m"), frames)
            write(os.path.join(tmp, "v1.y4m"), frames[:1])
            t16, t1 = run(os.path.join(tmp, "v16.y4m")), run(os.path.join(tmp, "v1.y4m"))
            out.append("%-34s %12.3f %12.3f %14.3f" % (label, t16, t1, (t16 - t1) * 1e3 / 15))
    out.append("(ms per frame: (16 frames - 1 frame) / 15 -- the process start, the model load and the first, full frame taken off; file reads and writes are inside)")
    return out


# ---- A: the two launches against the torch detour ----
NCALLS = 100
lines += ["", "A  pack (1920 x 1080) and unpack (7680 x 4320, 3840 x 2160) alone against the torch detour: RealSR.pack_planes / unpack_planes with prebuilt",
          "   descriptors, %d calls per bracket.  'queued': behind a few ms of other work, so that all calls are queued when the GPU reaches them (GPU time;" % NCALLS,
          "   this is what the gate reads); 'paced': the same calls on an idle stream, where the host's launch rate is the bound (reported)",
          "%-28s %10s %9s %9s %9s %9s   %s" % ("variant", "median us", "min us", "max us", "spread", "GB/s", "per repetition (us per call)")]
launch_us = {}
for fmt, name, dt, bits in () if only == "cli" else ((NV12, "nv12", torch.uint8, 8), (P010, "p010", torch.int16, 10)):
    for what, w, h in (("pack", W, H), ("unpack", 4 * W, 4 * H), ("unpack", 2 * W, 2 * H)):
        with torch.cuda.stream(st):
            y = torch.randint(0, 1 << bits, (h, w), device="cuda").to(dt)
            u = torch.randint(0, 1 << bits, (h // 2, w // 2), device="cuda").to(dt)
            v = torch.randint(0, 1 << bits, (h // 2, w // 2), device="cuda").to(dt)
            surf = torch_io.pack_planes(sr, y, u, v)
            surf2, outs = torch.empty_like(surf), (torch.empty_like(y), torch.empty_like(u), torch.empty_like(v))

            def detour_pack():
                surf2[:h] = y if bits == 8 else (y & 1023) << 6
                uv = torch.stack((u, v), -1).view(h // 2, w)
                surf2[h:] = uv if bits == 8 else (uv & 1023) << 6

            es = y.element_size()
            d_planes = [(y.data_ptr(), u.data_ptr(), v.data_ptr(), w * es, w // 2 * es)]
            d_outs = [(outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), w * es, w // 2 * es)]
            d_surf, d_surf2 = [(surf.data_ptr(), w * es, h * w * es)], [(surf2.data_ptr(), w * es, h * w * es)]

            def ours_pack():
                sr.pack_planes(d_planes, d_surf2, fmt, w, h, stream=st.cuda_stream)

            def detour_unpack():
                uv = surf[h:].view(h // 2, w // 2, 2)
                if bits == 8:
                    return surf[:h].contiguous(), uv[..., 0].contiguous(), uv[..., 1].contiguous()
                return (surf[:h] >> 6) & 1023, (uv[..., 0] >> 6) & 1023, (uv[..., 1] >> 6) & 1023

            def ours_unpack():
                sr.unpack_planes(d_surf, d_outs, fmt, w, h, stream=st.cuda_stream)

            detour, ours = (detour_pack, ours_pack) if what == "pack" else (detour_unpack, ours_unpack)
            t = timed([("detour", detour), ("ours", ours)], NCALLS)
            tp = timed([("detour", detour), ("ours", ours)], NCALLS, blocker=False)
            if what == "pack":
                detour_pack()
                ref = surf2.clone()
                surf2.zero_()
                ours_pack()
                st.synchronize()
                same = torch.equal(ref, surf2) and torch.equal(ref, surf)
            else:
                ours_unpack()
                st.synchronize()
                same = all(torch.equal(a, b) for a, b in zip(detour_unpack(), outs)) and torch.equal(outs[0], y) and torch.equal(outs[2], v)
        nbytes = surf.numel() * surf.element_size()
        (dm, d0, d1), (om, o0, o1) = stats(t["detour"]), stats(t["ours"])
        size = "%dx%d" % (w, h)
        for label, key, (m, lo, hi) in (("torch detour", "detour", (dm, d0, d1)), ("rsr_%s_planes" % what, "ours", (om, o0, o1))):
            lines.append("%-5s %-6s %-9s %-17s queued %10.1f %9.1f %9.1f %9.1f %9.1f   %s" % (name, what, size, label, m * 1e3, lo * 1e3, hi * 1e3, (hi - lo) * 1e3, 2 * nbytes / (m * 1e-3) / 1e9,
                                                                               " ".join("%.1f" % (x * 1e3) for x in t[key])))
        lines.append("%-5s %-6s %-9s paced: torch detour %.1f us, rsr_%s_planes %.1f us per call" % (name, what, size, stats(tp["detour"])[0] * 1e3, what, stats(tp["ours"])[0] * 1e3))
        gate("%s %s " % (name, what) + size + ": ours - detour = %.1f us <= spread of the detour %.1f us (bytes equal: %s)" % ((om - dm) * 1e3, (d1 - d0) * 1e3, same), om - dm <= d1 - d0 and same)
        launch_us[(fmt, what, w)] = om * 1e3


# ---- B and C: the session ----
def pinned(a):
    m = R.PinnedArray((a.nbytes,))
    q = m.array.view(a.dtype).reshape(a.shape)
    q[...] = a
    return q, m


def make_frames(k, nf=NF):
    """nf + 1 frames of (y, u, v) uint8 planes; k = None: every frame all new; else frame j differs from j - 1 in the centre luma sample
    of k tiles (far from every halo: one tile each)."""
    base = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2))]
    frames = [base]
    nx = (W + TILE - 1) // TILE
    order = np.random.default_rng(7).permutation(60)
    for j in range(nf):
        if k is None:
            frames.append([rng.integers(0, 256, p.shape, dtype=np.uint8) for p in base])
            continue
        f = [p.copy() for p in frames[-1]]
        for t in order[:k]:
            yi, xi = divmod(int(t), nx)
            f[0][min(yi * TILE + TILE // 2, H - 21), min(xi * TILE + TILE // 2, W - 21)] += 1 + j
        frames.append(f)
    return frames


def wall(variants):
    times = {n: [] for n, _ in variants}
    for rep in range(reps + 1):
        for n, f in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if rep:
                times[n].append((time.perf_counter() - t0) * 1e3 / NF)
    return times


def session_runner(vs, frames, outs):
    def go():  # (the window before ended on frames[NF], which differs from frames[1] in the tiles frames[0] does: no reset, no extra frame)
        for f in frames[1:]:
            vs.send(*f)
        while vs.ready:
            vs.receive(outs)
    return go


keep = []
for scale in () if only == "cli" else (4, 2):
    sr.out_scale = scale
    ow, oh = W * scale, H * scale
    in_bytes, out_bytes = W * H * 3 // 2, ow * oh * 3 // 2
    for label, k in (("B  all tiles changing", None), ("C  1 changed tile of 60 per frame", 1), ("C  6 changed tiles of 60 per frame", 6)):
        if scale == 2 and k is not None:
            continue
        frames = make_frames(k)
        pf = []
        for f in frames:
            qs = [pinned(p) for p in f]
            keep.extend(m for _, m in qs)
            pf.append([q for q, _ in qs])
        outs_pin = [pinned(np.zeros(s, dtype=np.uint8)) for s in ((oh, ow), (oh // 2, ow // 2), (oh // 2, ow // 2))]
        keep.extend(m for _, m in outs_pin)
        outs_pin = [q for q, _ in outs_pin]
        outs_page = [np.zeros_like(q) for q in outs_pin]
        vs = R.Video(sr, NV12, W, H, window=NF)
        # the parts, measured in the same run: the plain device-resident call per frame, the pinned copies, (A's launches)
        surfs = [torch.from_numpy(np.concatenate([f[0], np.stack([f[1], f[2]], -1).reshape(H // 2, W)])).cuda() for f in frames]
        d_out = torch.empty((oh * 3 // 2, ow), dtype=torch.uint8, device="cuda")
        h_in, h_out = torch.empty(in_bytes, dtype=torch.uint8).pin_memory(), torch.empty(out_bytes, dtype=torch.uint8).pin_memory()
        d_in = torch.empty(in_bytes, dtype=torch.uint8, device="cuda")

        def plain():
            for s_ in surfs[1:]:
                sr.process_device_fmt(s_.data_ptr(), NV12, W, H, 3, d_out.data_ptr(), NV12)

        def copies():
            for _ in range(NF):
                d_in.copy_(h_in, non_blocking=True)
                h_out.copy_(d_out.view(-1), non_blocking=True)

        def sequence():
            with torch.cuda.stream(st):
                torch_io.upscale_sequence(sr, surfs[1:], prev_x=surfs[0], prev_y=y_prev)
                st.synchronize()

        with torch.cuda.stream(st):
            y_prev = torch_io.upscale_yuv(sr, surfs[0])
            st.synchronize()
        variants = [("session pinned", session_runner(vs, pf, outs_pin)), ("session pageable", session_runner(vs, frames, outs_page)), ("copies", copies)]
        variants += [("plain", plain), ("sequence", sequence)] if k is None else [("sequence", sequence)]
        t = wall(variants[1:])  # (warm: the first window of a session runs every tile)
        tab0, win0 = sr.get_stat("masked_table_us"), sr.get_stat("video_windows")
        t.update(wall(variants[:1]))
        table_ms = (sr.get_stat("masked_table_us") - tab0) / 1e3 / max(1.0, (sr.get_stat("video_windows") - win0) * NF)
        vs.close()
        lines += ["", "%s, NV12 -> NV12 at x%d, window %d: ms per frame, host -> host (wall)" % (label, scale, NF),
                  "%-34s %10s %9s %9s %9s   %s" % ("variant", "median ms", "min ms", "max ms", "spread", "per repetition")]
        names = {"session pinned": "session, pinned planes", "session pageable": "session, pageable planes", "copies": "pinned H2D + D2H of the same bytes",
                 "plain": "rsr_process_device_fmt, resident", "sequence": "upscale_sequence, resident"}
        for key, _ in variants:
            m, lo, hi = stats(t[key])
            lines.append("%-34s %10.3f %9.3f %9.3f %9.3f   %s" % (names[key], m, lo, hi, hi - lo, " ".join("%.3f" % x for x in t[key])))
        sm, s0, s1 = stats(t["session pinned"])
        cm = stats(t["copies"])[0]
        if k is None:
            launches = (launch_us[(NV12, "pack", W)] + launch_us[(NV12, "unpack", scale * W)]) * 1e-3
            parts = [p + c + launches for p, c in zip(t["plain"], t["copies"])]
            pm, p0, p1 = stats(parts)
            lines.append("sum of the parts: plain + copies + pack + unpack launches (%.3f ms) = median %.3f ms (%.3f .. %.3f); the copies are %.1f %% of the session's frame"
                         % (launches, pm, p0, p1, 100 * cm / sm))
            qm = stats(t["sequence"])[0]
            lines.append("where the rest goes: the same 8 frames as ONE device-resident upscale_sequence call cost %.3f ms per frame, %.3f more than the plain calls: "
                         "the session's remainder over sequence + copies + launches is %.3f ms per frame; building and uploading the tile tables of a window "
                         "(stat masked_table_us, host time during which the GPU waits) is %.3f ms per frame of it" % (qm, qm - stats(t["plain"])[0], sm - qm - cm - launches, table_ms))
            gate("x%d: session %.3f ms <= the sum %.3f ms + its spread %.3f ms" % (scale, sm, pm, p1 - p0), sm <= pm + (p1 - p0))
        else:
            qm = stats(t["sequence"])[0]
            lines.append("session - (sequence + copies) = %.3f ms per frame; the copies are %.1f %% of the session's frame" % (sm - qm - cm, 100 * cm / sm))
sr.out_scale = 4
sr.close()
for m in keep:
    m.free()
if only == "cli":
    lines = []
lines += cli_section()

text = "\n".join(lines)
print(text)
if out_path:
    with open(out_path, "a" if append else "w") as fh:
        fh.write(text + "\n")
