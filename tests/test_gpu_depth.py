"""RRDBNet x4 models of other depths than 23 on the GPU (run with -m gpu): 1, 2 and 6 blocks through the network, the tile loop and every
output path, held BIT FOR BIT to the two-term exact model of tests/exact_net.py driven at that depth (tests/depth_ref.py; its health at
these depths is tests/test_model_depth.py's business).  The kernels see one convolution at a time and do not know the depth; what is
tested here is the host side that walks them: the loop bound of run_network, the margins counted back from conv_last, the middle-RDB
event of merged batches, the arrays sized by the conv count, packed blobs whose header names the depth, and a context that changes
depth between loads.  One test ties a 6-block model with ordinary (synth) weights to the oracle at the project's +-1 uint8 bar."""
import os
import subprocess
import sys
import threading
from fractions import Fraction

import numpy as np
import pytest
import torch

import depth_ref as D
import exact_conv as X
import exact_net as N
import oracle
import realsr_ncnn_vulkan_amd as R
import yuv_ref
from area_reduce import area_reduce
from box_reduce import box_reduce
from realsr_ncnn_vulkan_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8, F16, F32, NV12 = R.RSR_FMT_U8_HWC, R.RSR_FMT_F16_CHW, R.RSR_FMT_F32_CHW, R.RSR_FMT_NV12
W, H, T = N.FRAME
DEPTHS = (1, 2, 6)
SENTINEL = 0xCD


# ---- models, contexts and references, each made once ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets(tmp_path_factory):
    """nb -> (the exact model of that depth, x4.param, x4.bin), everything made inside depth(nb)."""
    made = {}
    for nb in DEPTHS:
        d = str(tmp_path_factory.mktemp("depth_nb%d" % nb))
        with D.depth(nb):
            model = D.make_model(nb)
            pp, bp = os.path.join(d, "x4.param"), os.path.join(d, "x4.bin")
            synth.write_param(pp)
            synth.write_bin(bp, N.dense_weights(model), "fp16")
        made[nb] = (model, pp, bp)
    assert synth.NB == N.NB == 23
    return made


def reset(s):
    s.out_scale = 4
    s.tilesize, s.prepadding = T, 10
    for k, v in (("precise", 0), ("bgr", 0), ("max_workspace_mb", 65536), ("trim", 1), ("merge", 16), ("yuv_matrix", 709), ("yuv_range", 0)):
        s.set_option(k, v)
    s.set_profiling(0)


@pytest.fixture(scope="module")
def ctxs(nets):
    made = {}
    for nb in DEPTHS:
        made[nb] = R.RealSR(0)
        made[nb].load(*nets[nb][1:])
    yield made
    for s in made.values():
        s.close()


@pytest.fixture
def sr(ctxs):
    for s in ctxs.values():
        reset(s)
    yield ctxs
    for s in ctxs.values():
        reset(s)


_refs = {}


def ref_x4(nets, nb, key, x16, tile=T, **kw):
    """The mirror's x4 image (fp32, before clamp and conversion) of one input at depth nb, computed once per module and left unchanged."""
    if (nb, key) not in _refs:
        with D.depth(nb):
            _refs[nb, key] = N.image_x4(nets[nb][0], x16, tile, **kw)
        _refs[nb, key].setflags(write=False)
    return _refs[nb, key]


def frame_ref_u8(nets, nb):
    return hwc(N.to_u8(ref_x4(nets, nb, "u8", N.halfs_of_u8(N.frame_u8(W, H)))))


def hwc(planar):
    return np.ascontiguousarray(planar.transpose(1, 2, 0))


def same(got, want, what=""):
    """'' when the bit patterns are equal, else a message with the first mismatch."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = (np.ascontiguousarray(a).view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize]) for a in (got, want))
    bad = g != w
    if not bad.any():
        return ""
    i = tuple(np.argwhere(bad)[0])
    return "%s: %d of %d values differ, first at %s: got %r want %r" % (what, int(bad.sum()), g.size, i, got[i].item(), want[i].item())


NP = {U8: np.uint8, F16: np.float16, F32: np.float32, NV12: np.uint8}


def device_call(s, x, in_fmt, out_fmt, w, h):
    """One synchronous rsr_process_device_fmt call on the packed numpy image x at the context's output ratio; the destination is
    pre-filled with a sentinel."""
    ow, oh = s.out_size(w, h)
    d_in = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
    d_out = torch.full((R.image_bytes(out_fmt, ow, oh),), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s.process_device_fmt(d_in.data_ptr(), in_fmt, w, h, 3, d_out.data_ptr(), out_fmt)
    torch.cuda.synchronize()
    shape = (oh, ow, 3) if out_fmt == U8 else ((oh * 3 // 2, ow) if out_fmt == NV12 else (3, oh, ow))
    return d_out.cpu().numpy().view(NP[out_fmt]).reshape(shape)


# ---- the network, one tile per call -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", N.TILE_SHAPES)
@pytest.mark.parametrize("nb", DEPTHS)
def test_net_forward_tiles(sr, nets, nb, h, w):
    """rsr_net_forward in fp16 storage and rsr_net_forward_f32 (which exists in precise mode) on a folded tile, an odd one, exact blocks
    and one row / column over: the whole walk of 15 nb + 6 launches against forward() of the same depth."""
    s, x = sr[nb], N.tile_f16(h, w)
    with D.depth(nb):
        want = X.f16(N.forward(nets[nb][0], x))
        want_p = N.forward(nets[nb][0], x, precise=True)
    assert s.num_blocks == nb and s.num_convs == 15 * nb + 6
    msg = same(s.net_forward(x), want, "net_forward nb=%d %dx%d" % (nb, h, w))
    assert not msg, msg
    s.set_option("precise", 1)
    msg = same(s.net_forward_f32(x), want_p, "net_forward_f32 (precise) nb=%d %dx%d" % (nb, h, w))
    assert not msg, msg


# ---- the tile loop ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", DEPTHS)
def test_process_frame(sr, nets, nb):
    """50 x 40 at tile 24: 3 x 2 tiles, partial ones, the trimmed margins counted back from conv_last = convolution 15 nb + 5."""
    msg = same(sr[nb].process(N.frame_u8(W, H)), frame_ref_u8(nets, nb), "process nb=%d" % nb)
    assert not msg, msg


def test_two_blocks_precise_frame(sr, nets):
    s = sr[2]
    s.set_option("precise", 1)
    img = N.frame_u8(W, H)
    msg = same(s.process(img), hwc(N.to_u8(ref_x4(nets, 2, "u8 precise", N.halfs_of_u8(img), precise=True))), "process, precise")
    assert not msg, msg


def test_two_blocks_rgba_and_bgr(sr, nets):
    s = sr[2]
    img4 = N.frame_u8(W, H, 4)
    got = s.process(img4)
    assert got.shape == (4 * H, 4 * W, 4)
    msg = same(np.ascontiguousarray(got[:, :, :3]), hwc(N.to_u8(ref_x4(nets, 2, "rgba", N.halfs_of_u8(img4)))), "process RGBA")
    assert not msg, msg
    img = N.frame_u8(W, H)
    want = hwc(N.to_u8(ref_x4(nets, 2, "bgr", N.halfs_of_u8(img[:, :, ::-1]))))[:, :, ::-1]
    s.set_option("bgr", 1)
    msg = same(s.process(img), np.ascontiguousarray(want), "process bgr")
    assert not msg, msg


def test_two_blocks_tta(nets):
    """A TTA context on 30 x 26 at tile 16 (the two-block model reaches both clamps there with its own conv_last: tests/test_model_depth.py)."""
    s = R.RealSR(0, tta_mode=True)
    try:
        s.load(*nets[2][1:])
        s.tilesize = N.TTA_FRAME[2]
        img = N.tta_frame()
        want = hwc(N.to_u8(ref_x4(nets, 2, "tta", N.halfs_of_u8(img), tile=N.TTA_FRAME[2], tta=True)))
        msg = same(s.process(img), want, "process TTA")
        assert not msg, msg
    finally:
        s.close()


def test_two_blocks_float_formats(sr, nets):
    s = sr[2]
    x = N.frame_f16(W, H)
    want = N.to_unit(ref_x4(nets, 2, "f16", x))
    for name, got in (("F16 -> F32", device_call(s, x, F16, F32, W, H)),
                      ("F32 -> F16", device_call(s, x.astype(np.float32), F32, F16, W, H).astype(np.float32))):
        msg = same(got, want, name)
        assert not msg, msg


def test_two_blocks_reduced_outputs(sr, nets):
    """out_scale 2 (tests/box_reduce.py) and ratio 3/2 (tests/area_reduce.py: tile 24 -> 36 output pixels) of the mirror's x4 image."""
    s = sr[2]
    img = N.frame_u8(W, H)
    x4 = ref_x4(nets, 2, "u8", N.halfs_of_u8(img))
    s.out_scale = 2
    msg = same(device_call(s, img, U8, F32, W, H), box_reduce(x4, 2), "out_scale 2")
    assert not msg, msg
    s.out_ratio = Fraction(3, 2)
    msg = same(device_call(s, img, U8, F32, W, H), area_reduce(x4, 3, 2), "out_ratio 3/2")
    assert not msg, msg


def test_two_blocks_several_batches_and_untrimmed(sr, nets):
    """A workspace budget of about two tiles (several batches), and option "trim" 0 against 1: the same bytes."""
    s = sr[2]
    img, want = N.frame_u8(W, H), frame_ref_u8(nets, 2)
    s.set_option("max_workspace_mb", 30)
    got = s.process(img)
    assert s.get_stat("plan_batches") > 1
    msg = same(got, want, "process in %d batches" % s.get_stat("plan_batches"))
    assert not msg, msg
    s.set_option("max_workspace_mb", 65536)
    s.set_option("trim", 0)
    msg = same(s.process(img), want, "process, trim 0")
    assert not msg, msg


# ---- video ------------------------------------------------------------------------------------------------------------------------
def test_two_blocks_nv12_surface(sr):
    """NV12 -> NV12 on a 48 x 40 surface == yuv_ref.encode(F32 -> F32 of the same context on yuv_ref.decode(surface)): the definition
    tests/test_gpu_yuv.py uses (the F32 path itself is held to the mirror above)."""
    s = sr[2]
    w, h = 48, 40
    surf = np.random.default_rng(4840).integers(0, 256, size=(h * 3 // 2, w)).astype(np.uint8)
    y, uv = yuv_ref.split(surf, 8)
    d = device_call(s, yuv_ref.decode(y, uv, 709, 0, 8), F32, F32, w, h)
    assert np.isfinite(d).all() and len(np.unique(d)) > 100
    want = yuv_ref.join(*yuv_ref.encode(d, 709, 0, 8), 8)
    assert len(np.unique(want)) > 16
    msg = same(device_call(s, surf, NV12, NV12, w, h), want, "NV12 -> NV12")
    assert not msg, msg


# ---- masked calls and sequences -----------------------------------------------------------------------------------------------------
def tile_rects4(w, h, tile):
    """The x4 output rectangle (y0, y1, x0, x1) of every tile, row-major."""
    return [(4 * y0, 4 * (y0 + th), 4 * x0, 4 * (x0 + tw)) for x0, y0, tw, th in N.tile_grid(w, h, tile)]


def test_two_blocks_masked_call(sr, nets):
    """Two of the six tiles set: their rectangles carry the plain call's bytes, every other byte of the destination keeps the sentinel."""
    s = sr[2]
    img, plain = N.frame_u8(W, H), frame_ref_u8(nets, 2)
    mask = np.array([0, 1, 0, 0, 0, 1], dtype=np.uint8)
    d_in = torch.from_numpy(img).cuda()
    d_out = torch.full((4 * H, 4 * W, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s.process_device_masked(d_in.data_ptr(), U8, W, H, 3, d_out.data_ptr(), U8, mask)
    torch.cuda.synchronize()
    want = np.full((4 * H, 4 * W, 3), SENTINEL, dtype=np.uint8)
    for m, (y0, y1, x0, x1) in zip(mask, tile_rects4(W, H, T)):
        if m:
            want[y0:y1, x0:x1] = plain[y0:y1, x0:x1]
    msg = same(d_out.cpu().numpy(), want, "masked call")
    assert not msg, msg


def test_two_blocks_sequence(sr, nets):
    """Three frames in one call: frame 0 whole, then two tiles, then one.  Every output rectangle holds the plain call's bytes of the frame
    that computed it last (rsr_sequence_sources), and the bytes between the three output images keep the sentinel."""
    s = sr[2]
    frames = [N.frame_u8(W, H, seed=900 + k) for k in range(3)]
    plain = [s.process(f) for f in frames]
    msg = same(plain[0], hwc(N.to_u8(ref_x4(nets, 2, "seq0", N.halfs_of_u8(frames[0])))), "frame 0, plain")
    assert not msg, msg
    masks = np.array([[1, 1, 1, 1, 1, 1], [0, 1, 0, 0, 1, 0], [0, 0, 0, 0, 0, 1]], dtype=np.uint8)
    src = R.sequence_sources(masks, False)
    nbytes, gap = 4 * H * 4 * W * 3, 4096
    d_in = [torch.from_numpy(f).cuda() for f in frames]
    d_out = torch.full((3 * (nbytes + gap),), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s.process_device_sequence([t.data_ptr() for t in d_in], U8, W, H, 3, [d_out.data_ptr() + k * (nbytes + gap) for k in range(3)], U8, masks)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().reshape(3, nbytes + gap)
    assert (got[:, nbytes:] == SENTINEL).all()
    for k in range(3):
        want = np.empty_like(plain[0])
        for t, (y0, y1, x0, x1) in enumerate(tile_rects4(W, H, T)):
            want[y0:y1, x0:x1] = plain[src[k, t]][y0:y1, x0:x1]
        msg = same(got[k, :nbytes].reshape(plain[0].shape), want, "sequence frame %d" % k)
        assert not msg, msg


# ---- merged small images: the middle-RDB event of a network with three RDBs ----------------------------------------------------------
def test_one_block_merged_small_images(sr, nets):
    """Four threads, each three 40 x 40 images at tile 32, concurrently on the one-block context: the bytes of the lone calls, merged
    batches did form (their throttle event sits behind RDB 0 of 3 here), and one image equals the mirror."""
    s = sr[1]
    s.tilesize = 32
    imgs = [N.frame_u8(40, 40, seed=300 + i) for i in range(12)]
    s.set_option("merge", 1)
    b0 = s.get_stat("merged_batches")   # (the context is shared with the tests above: the counters are read as differences)
    lone = [s.process(im) for im in imgs]
    assert s.get_stat("merged_batches") == b0
    msg = same(lone[0], hwc(N.to_u8(ref_x4(nets, 1, "small0", N.halfs_of_u8(imgs[0]), tile=32))), "lone call")
    assert not msg, msg
    s.set_option("merge", 16)
    outs, errs, gate = [None] * 12, [], threading.Barrier(4)

    def work(t):
        try:
            gate.wait(30)
            for k in range(3):
                outs[t * 3 + k] = s.process(imgs[t * 3 + k], push_params=False)
        except Exception as e:  # noqa: BLE001
            errs.append((t, repr(e)))
    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    for i in range(12):
        assert np.array_equal(outs[i], lone[i]), i
    print("12 images in %d merged batches, widest so far %d" % (s.get_stat("merged_batches") - b0, s.get_stat("merged_widest")))
    assert s.get_stat("merged_batches") - b0 > 0


# ---- one context, several depths ----------------------------------------------------------------------------------------------------
def test_reload_23_2_23(sr, nets, model_dir):
    """One context loads 23 -> 2 -> 23 blocks and runs the frame after each load: the bytes of a fresh context of that depth.  The stats
    follow the model, and what the self-check said about the previous model is gone until it runs again."""
    p23 = (os.path.join(model_dir, "x4.param"), os.path.join(model_dir, "x4.bin"))
    img = N.frame_u8(W, H)
    fresh = R.RealSR(0)
    s = R.RealSR(0)
    try:
        fresh.load(*p23)
        fresh.tilesize = T
        want = {23: fresh.process(img), 2: frame_ref_u8(nets, 2)}
        assert fresh.num_blocks == 23 and fresh.num_convs == 351
        s.tilesize = T
        assert s.num_blocks == 0 and s.num_convs == 0
        for nb, paths in ((23, p23), (2, nets[2][1:]), (23, p23)):
            s.load(*paths)
            assert s.num_blocks == nb and s.get_stat("model_blocks") == nb and s.get_stat("model_convs") == 15 * nb + 6
            msg = same(s.process(img), want[nb], "after loading %d blocks" % nb)
            assert not msg, msg
            with pytest.raises(R.RealSRError) as e:   # the report of the model before this one is dropped
                s.selfcheck_ranges()
            assert e.value.code == R.RSR_E_STATE and s.get_stat("selfcheck_headroom") == -1
            s.set_profiling(1)
            s.process(img)
            s.set_profiling(0)
            times = s.conv_times()
            assert len(times) == 15 * nb + 6 and (times > 0).all()
            rep = s.selfcheck()
            peak, bad = s.selfcheck_ranges()
            assert len(peak) == len(bad) == 15 * nb + 6 and np.isfinite(peak).all() and (peak > 0).all() and rep["peak_conv"] < 15 * nb + 6
            msg = same(s.process(img), want[nb], "after the self-check at %d blocks" % nb)
            assert not msg, msg
    finally:
        s.close()
        fresh.close()


def test_two_blocks_selfcheck_and_conv_times(sr):
    s = sr[2]
    L, h = s._L, s._h
    import ctypes as C
    rep = s.selfcheck()
    assert rep["nonfinite"] == 0 and 0 <= rep["peak_conv"] < 36 and rep["peak_abs"] > 0
    fp, lp = C.POINTER(C.c_float), C.POINTER(C.c_longlong)
    p36, b36 = np.full(36, -1, np.float32), np.full(36, -1, np.int64)
    assert L.rsr_selfcheck_ranges(h, p36.ctypes.data_as(fp), b36.ctypes.data_as(lp), 36) == 0
    assert np.isfinite(p36).all() and (p36 > 0).all() and (b36 == 0).all() and p36.max() == np.float32(rep["peak_abs"])
    p351, b351 = np.full(351, -1, np.float32), np.full(351, -1, np.int64)
    assert L.rsr_selfcheck_ranges(h, p351.ctypes.data_as(fp), b351.ctypes.data_as(lp), 351) == 0
    assert np.array_equal(p351[:36], p36) and (p351[36:] == 0).all() and (b351 == 0).all()
    p967 = np.zeros(967, np.float32)
    assert L.rsr_selfcheck_ranges(h, p967.ctypes.data_as(fp), None, 967) == R.RSR_E_ARG
    assert L.rsr_selfcheck_ranges(h, p967.ctypes.data_as(fp), None, 966) == 0 and (p967[36:] == 0).all()
    s.set_profiling(1)
    s.get_conv_times(reset=True)
    s.process(N.frame_u8(W, H))
    s.set_profiling(0)
    ms = (C.c_double * 40)(*([-1.0] * 40))
    assert L.rsr_get_conv_times(h, ms, 36, 0) == 0
    assert all(v > 0 for v in ms[:36]) and all(v == -1.0 for v in ms[36:])
    assert L.rsr_get_conv_times(h, ms, 40, 1) == 0 and all(v > 0 for v in ms[:36]) and all(v == 0 for v in ms[36:])
    big = (C.c_double * 967)()
    assert L.rsr_get_conv_times(h, big, 967, 0) == R.RSR_E_ARG


# ---- packed blobs -------------------------------------------------------------------------------------------------------------------
def test_two_blocks_packed_host_and_device(sr, nets):
    want = frame_ref_u8(nets, 2)
    img = N.frame_u8(W, H)
    blob = R.model_pack(*nets[2][1:])
    for how in ("host", "device"):
        s = R.RealSR(0)
        try:
            if how == "host":
                s.load_packed(blob)
            else:
                d_blob = torch.from_numpy(blob).cuda()
                torch.cuda.synchronize()
                s.load_packed(blob.size, device_ptr=d_blob.data_ptr())
            assert s.num_blocks == 2 and s.num_convs == 36
            s.tilesize = T
            msg = same(s.process(img), want, "load_packed from a %s blob" % how)
            assert not msg, msg
        finally:
            s.close()


def test_two_blocks_group_through_rccl_in_a_child_process(nets, tmp_path):
    """rsr_create_group with RSR_GROUP_FORCE_RCCL=1: one rank, the blob of a 2-block model through the collective and load_blob_device."""
    out = str(tmp_path / "out.npy")
    code = (
        "import sys; sys.path[:0] = [%r, %r]\n"
        "import numpy as np\n"
        "import realsr_ncnn_vulkan_amd as R, exact_net as N\n"
        "srs, transport = R.create_group([0], %r, %r)\n"
        "assert transport == 'rccl', transport\n"
        "assert srs[0].num_blocks == 2 and srs[0].num_convs == 36\n"
        "srs[0].tilesize = %d\n"
        "np.save(%r, srs[0].process(N.frame_u8(%d, %d)))\n"
        "srs[0].close()\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), nets[2][1], nets[2][2], T, out, W, H)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env=dict(os.environ, RSR_GROUP_FORCE_RCCL="1"))
    assert r.returncode == 0, r.stderr[-1500:]
    msg = same(np.load(out), frame_ref_u8(nets, 2), "group member")
    assert not msg, msg


def test_group_members_of_different_depth_are_refused(sr, nets):
    img = N.frame_u8(W, H)
    with pytest.raises(R.RealSRError) as e:
        R.process_group([sr[2], sr[6]], img)
    assert e.value.code == R.RSR_E_ARG and "depth" in str(e.value)
    msg = same(R.process_group([sr[2], sr[2]], img), frame_ref_u8(nets, 2), "a group of one depth")
    assert not msg, msg


# ---- ordinary weights: the project's bar ---------------------------------------------------------------------------------------------
def test_six_blocks_oracle_parity():
    """synth weights at 6 blocks, 64 x 48 at tile 32: within +-1 uint8 of the CPU oracle, as every depth-23 parity test asks."""
    d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K", 42, nb=6)
    pp, bp = os.path.join(d, "x4.param"), os.path.join(d, "x4.bin")
    img = synth.make_image(7, 64, 48)
    s = R.RealSR(0)
    try:
        s.load(pp, bp)
        s.tilesize = 32
        got = s.process(img)
    finally:
        s.close()
    net = oracle.OracleNet(pp, bp)
    assert net.num_convs == 96
    ref = net.process(img, 32)
    diff = np.abs(got.astype(int) - ref.astype(int))
    print("6 blocks: max |diff| vs oracle = %d, %.2f %% bytes differ, %d distinct codes" % (diff.max(), 100 * (diff > 0).mean(), len(np.unique(got))))
    assert got.shape == (192, 256, 3) and len(np.unique(got)) > 100
    assert diff.max() <= 1


def test_cli_loads_a_six_block_directory_and_prints_the_depth(tmp_path):
    """realsr-hip -m <a 6-block directory> -v: "6 blocks, 96 convolutions" on stderr, and the image a context of that model writes."""
    from cli_support import CLI, read_png, write_png
    d = synth.make_model_dir(os.environ.get("RSR_MODELS", "/tmp/rsr_models"), "models-DF2K", 42, nb=6)
    img = synth.make_image(7, 50, 43)
    write_png(tmp_path / "in.png", img)
    env = {k: v for k, v in os.environ.items() if k not in ("RSR_PRECISE", "RSR_PRECISE_AUTO", "RSR_OUT_SCALE")}
    r = subprocess.run([CLI, "-i", str(tmp_path / "in.png"), "-o", str(tmp_path / "out.png"), "-m", d, "-t", "32", "-v"], capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0 and "6 blocks, 96 convolutions" in r.stderr, r.stderr[-2000:]
    s = R.RealSR(0)
    try:
        s.load(os.path.join(d, "x4.param"), os.path.join(d, "x4.bin"))
        s.tilesize = 32
        assert np.array_equal(read_png(tmp_path / "out.png"), s.process(img))
    finally:
        s.close()
