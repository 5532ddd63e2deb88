"""Frame sequences without a GPU: rsr_sequence_sources against tests/sequence_ref.py, its refusals, the header and the exported symbols,
a C host that links them, and torch_io.upscale_sequence against a context that records what it is handed.  The GPU side:
tests/test_gpu_sequence.py."""
import os
import subprocess

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

import sequence_ref
import tile_diff_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rsr_sequence_sources", "rsr_diff_tiles_sequence", "rsr_process_device_sequence")
U8, F16, F32, NV12, P010 = R.RSR_FMT_U8_HWC, R.RSR_FMT_F16_CHW, R.RSR_FMT_F32_CHW, R.RSR_FMT_NV12, R.RSR_FMT_P010


# ---- rsr_sequence_sources -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 16])
@pytest.mark.parametrize("ntiles", [1, 6, 60])
def test_sources_against_the_reference(n, ntiles):
    rng = np.random.default_rng(100 * n + ntiles)
    for density in (0.1, 0.5, 0.9):
        masks = (rng.random((n, ntiles)) < density).astype(np.uint8) * rng.integers(1, 256, size=(n, ntiles)).astype(np.uint8)
        masks[:, rng.integers(ntiles)] = 0  # a column nobody sets: -1 all the way down
        want = sequence_ref.sources(masks, True)
        assert (want == -1).any() and want.min() == -1 and want.max() <= n - 1
        assert np.array_equal(R.sequence_sources(masks, True), want)
        masks[0, :] = 1  # every tile of the first frame set: no previous output is needed
        want = sequence_ref.sources(masks, False)
        assert want.min() == 0
        assert np.array_equal(R.sequence_sources(masks, False), want)
        assert np.array_equal(R.sequence_sources(masks, True), want)


def test_sources_of_the_two_trivial_masks():
    assert R.sequence_sources(np.zeros((4, 6), np.uint8), True).tolist() == [[-1] * 6] * 4
    assert R.sequence_sources(np.ones((4, 6), np.uint8), False).tolist() == [[k] * 6 for k in range(4)]
    assert R.sequence_sources([[0, 1], [1, 0], [0, 0]], True).tolist() == [[-1, 0], [1, 0], [1, 0]]


def test_sources_refusals():
    assert R.RSR_SEQ_MAX == 16 and torch_io.SEQ_MAX == 16
    for masks, has_prev in ((np.ones((17, 6), np.uint8), True), (np.zeros((1, 6), np.uint8), False), (np.array([[1, 0], [1, 1]], np.uint8), False),
                            (np.ones((0, 6), np.uint8), True), (np.ones((3, 0), np.uint8), True)):
        with pytest.raises(R.RealSRError) as e:
            R.sequence_sources(masks, has_prev)
        assert e.value.code == R.RSR_E_ARG
    with pytest.raises(ValueError):
        sequence_ref.sources(np.array([[1, 0], [1, 1]]), False)
    L = R.lib()
    src = (R.C.c_int * 6)()
    m = np.ones(6, np.uint8)
    assert L.rsr_sequence_sources(1, 6, None, 1, src) == R.RSR_E_ARG
    assert L.rsr_sequence_sources(1, 6, m.ctypes.data_as(R.C.c_void_p), 1, None) == R.RSR_E_ARG
    assert L.rsr_sequence_sources(1, 6, m.ctypes.data_as(R.C.c_void_p), 0, src) == 0 and list(src) == [0] * 6


# ---- the header and the symbols ---------------------------------------------------------------------------------------------------------
def test_symbols():
    assert set(NEW_SYMBOLS) <= set(R.EXPORTS)
    for s in NEW_SYMBOLS:
        assert hasattr(R.lib(), s), s
    out = subprocess.run(["nm", "-D", "--defined-only", R.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for s in NEW_SYMBOLS:
        assert " T %s\n" % s in out, s


def test_header_carries_the_contract():
    text = open(os.path.join(R.INCLUDE_DIR, "realsr_hip.h")).read()
    for needle in ("#define RSR_SEQ_MAX 16", "int rsr_sequence_sources(", "int rsr_diff_tiles_sequence(", "int rsr_process_device_sequence(",
                   "the largest j < k with masks[j][t] != 0", "= -1, the previous output", "while has_prev == 0",
                   "rsr_diff_tiles(frames[k - 1], frames[k])", "with\n * prev == NULL it is all ones", "One memset and ONE kernel launch for all pairs",
                   "Every byte of every out[k] window is therefore written", "no byte outside a window is touched",
                   "prev_out may be out[0] itself", "a tile computed in frame 0 is never anybody's source -1",
                   "The copies are ONE launch behind", "no copy depends on another copy", "only the copy launch runs", "nothing is launched",
                   "nmask != n * nx * ny", "prev_out == NULL\n *            while row 0 has a zero byte",
                   '"seq_calls"', '"seq_frames"', '"seq_tiles_run"', '"seq_tiles_copied"', '"seq_batches"', 'The "masked_*" stats are not touched',
                   "Progress callback: one call per computed tile",
                   "Out of scope: host-pointer images, groups of GPUs, the CLI, merging with concurrent calls, frames of different geometry in one call",
                   # the masked section keeps its sentence
                   "Out of scope: n > 1, host-pointer images, groups of GPUs, the CLI, merging with concurrent calls"):
        assert needle in text, needle


def test_header_is_plain_c_and_a_c_host_links_the_three_symbols(tmp_path):
    src = tmp_path / "host.c"
    src.write_text(r'''
#include <stdio.h>
#include "realsr_hip.h"
int main(void)
{
    unsigned char masks[3 * 2] = {0, 1, 1, 0, 0, 0};
    int src[6], bad, rc, d, p;
    rsr_image im;
    im.data = NULL; im.row_pitch = 0; im.plane_pitch = 0;
    rc = rsr_sequence_sources(3, 2, masks, 1, src);
    bad = rsr_sequence_sources(3, 2, masks, 0, src);
    d = rsr_diff_tiles_sequence(NULL, 1, &im, NULL, RSR_FMT_U8_HWC, 8, 8, 3, NULL, NULL);
    p = rsr_process_device_sequence(NULL, 1, &im, RSR_FMT_U8_HWC, 8, 8, 3, &im, RSR_FMT_U8_HWC, NULL, masks, 6, NULL);
    printf("max %d rc %d src %d %d %d %d %d %d bad %d null %d %d\n", RSR_SEQ_MAX, rc, src[0], src[1], src[2], src[3], src[4], src[5], bad, d, p);
    return 0;
}
''')
    lib = os.path.join(ROOT, "realsr-ncnn-vulkan_amd", "lib")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(inc, "realsr_hip.h")])
    exe = str(tmp_path / "host")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", inc, "-o", exe, str(src), "-L", lib, "-lrealsr_hip", "-Wl,-rpath," + lib])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "max 16 rc 0 src -1 0 1 0 1 0 bad -1 null -1 -1" in r.stdout, r.stdout


# ---- torch_io.upscale_sequence against a recording context ------------------------------------------------------------------------------
class _Stream:
    cuda_stream = 5

    def __init__(self, log):
        self.log = log

    def synchronize(self):
        self.log.append(("sync",))


class _Ctx:
    """Records what torch_io hands the engine, at tile 32 and out_scale 4; the diff marks tile k % 6 of frame k of a window, and every
    tile of its first frame when there is no predecessor."""
    gpuid, scale, out_scale, tilesize, prepadding = 0, 4, 4, 32, 10

    def __init__(self):
        self.calls = []

    def out_size(self, w, h):
        return 4 * w, 4 * h

    def tile_count(self, w, h):
        return ref.tile_count(w, h, self.tilesize)

    def diff_tiles_sequence(self, frames, prev, fmt, w, h, c, d_masks, stream=None):
        self.calls.append(("diff", list(frames), prev, fmt, w, h, c, d_masks, stream))
        m = self.d_mask_tensor.view(len(frames), -1)
        assert d_masks == self.d_mask_tensor.data_ptr()
        m[:] = 0
        for k in range(len(frames)):
            m[k, k % m.shape[1]] = 1
        if prev is None:
            m[0, :] = 1

    def process_device_sequence(self, srcs, in_fmt, w, h, c, dsts, out_fmt, masks, prev_out=None, stream=None):
        self.calls.append(("seq", list(srcs), in_fmt, w, h, c, list(dsts), out_fmt, np.array(masks, dtype=np.uint8).copy(), prev_out, stream))


class _Cuda0(torch.Tensor):
    @property
    def device(self):
        return torch.device("cuda", 0)


def _on_cuda0(t):
    return t.as_subclass(_Cuda0)


@pytest.fixture
def fake(monkeypatch):
    """torch_io with a recording stream, pageable 'pinned' memory and a context whose device masks are the tensor torch_io allocates."""
    s = _Ctx()
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _Stream(s.calls))
    monkeypatch.setattr(torch_io, "_pinned_u8", lambda n: torch.empty(n, dtype=torch.uint8))
    real_new_empty = torch.Tensor.new_empty

    def new_empty(self, *a, **k):
        t = real_new_empty(self, *a, **k)
        if k.get("dtype") == torch.uint8 and t.dim() == 1:
            s.d_mask_tensor = t
        return t
    monkeypatch.setattr(_Cuda0, "new_empty", new_empty, raising=False)
    return s


def test_nineteen_frames_are_two_windows_and_the_second_takes_frame_15_as_prev(fake):
    s = fake
    frames = _on_cuda0(torch.zeros(19, 50, 70, 3, dtype=torch.uint8))
    ys, n = torch_io.upscale_sequence(s, frames)
    assert isinstance(ys, torch.Tensor) and tuple(ys.shape) == (19, 200, 280, 3) and ys.dtype == torch.uint8
    assert [c[0] for c in s.calls] == ["diff", "sync", "seq", "diff", "sync", "seq"]  # per window: one synchronisation, between the two
    d0, q0, d1, q1 = s.calls[0], s.calls[2], s.calls[3], s.calls[5]
    fd = [(frames[i].data_ptr(), 210, 0) for i in range(19)]
    yd = [(ys[i].data_ptr(), 840, 0) for i in range(19)]
    assert d0[1] == fd[:16] and d0[2] is None and d0[3:7] == (U8, 70, 50, 3) and d0[8] == 5
    assert q0[1] == fd[:16] and q0[2:6] == (U8, 70, 50, 3) and q0[6] == yd[:16] and q0[7] == U8 and q0[9] is None and q0[10] == 5
    assert q0[8].size == 16 * 6 and q0[8].reshape(16, 6)[0].tolist() == [1] * 6 and q0[8].reshape(16, 6)[7].tolist() == [0, 1, 0, 0, 0, 0]
    assert d1[1] == fd[16:] and d1[2] == fd[15]
    assert q1[1] == fd[16:] and q1[6] == yd[16:] and q1[9] == yd[15]
    assert q1[8].reshape(3, 6).tolist() == [[1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0]]
    assert n == (6 + 15) + 3


def test_a_list_with_prev_and_out_given(fake):
    s = fake
    xs = [_on_cuda0(torch.zeros(3, 50, 70, dtype=torch.float16)) for _ in range(3)]
    px, py = _on_cuda0(torch.zeros(3, 50, 70, dtype=torch.float16)), _on_cuda0(torch.zeros(3, 200, 280, dtype=torch.float16))
    canvas = torch.zeros(3, 3, 300, 400, dtype=torch.float16)
    outs = [_on_cuda0(canvas[i, :, 20:220, 40:320]) for i in range(3)]
    ys, n = torch_io.upscale_sequence(s, xs, px, py, out=outs)
    assert ys is outs and n == 3
    d, q = s.calls[0], s.calls[2]
    assert d[2] == (px.data_ptr(), 140, 50 * 140) and d[3] == F16
    assert q[9] == (py.data_ptr(), 560, 200 * 560)
    assert q[6] == [(canvas.data_ptr() + (i * 3 * 300 * 400 + 20 * 400 + 40) * 2, 800, 300 * 800) for i in range(3)]
    # without out: a list of new tensors
    ys, n = torch_io.upscale_sequence(s, xs, px, py)
    assert isinstance(ys, list) and [tuple(y.shape) for y in ys] == [(3, 200, 280)] * 3 and ys[0].dtype == torch.float16


def test_surfaces_and_pairs_come_as_lists(fake):
    s = fake
    xs = [_on_cuda0(torch.zeros(75, 70, dtype=torch.uint8)) for _ in range(2)]
    ys, n = torch_io.upscale_sequence(s, xs)
    assert [tuple(y.shape) for y in ys] == [(300, 280)] * 2 and n == 6 + 1
    q = s.calls[2]
    assert q[2:6] == (NV12, 70, 50, 3) and q[7] == NV12 and q[6] == [(y.data_ptr(), 280, 200 * 280) for y in ys]
    pairs = [(x[:50], x[50:]) for x in xs]
    ys, n = torch_io.upscale_sequence(s, pairs)
    assert all(isinstance(y, tuple) and tuple(y[0].shape) == (200, 280) and tuple(y[1].shape) == (100, 280) for y in ys)


def test_refusals_before_anything_is_launched(fake):
    s = fake
    frames = _on_cuda0(torch.zeros(3, 50, 70, 3, dtype=torch.uint8))
    x = _on_cuda0(torch.zeros(50, 70, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="mixed layouts"):
        torch_io.upscale_sequence(s, [x, _on_cuda0(torch.zeros(50, 66, 3, dtype=torch.uint8))])
    with pytest.raises(ValueError, match="mixed layouts"):
        torch_io.upscale_sequence(s, [x, _on_cuda0(torch.zeros(3, 50, 70, dtype=torch.float16))])
    with pytest.raises(ValueError, match="prev_y"):
        torch_io.upscale_sequence(s, frames, prev_x=x)
    with pytest.raises(ValueError, match="prev_x"):
        torch_io.upscale_sequence(s, frames, prev_x=_on_cuda0(torch.zeros(50, 70, 4, dtype=torch.uint8)), prev_y=_on_cuda0(torch.zeros(200, 280, 3, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="prev_y"):
        torch_io.upscale_sequence(s, frames, prev_x=x, prev_y=_on_cuda0(torch.zeros(200, 276, 3, dtype=torch.uint8)))
    for bad in (torch.zeros(3, 200, 276, 3, dtype=torch.uint8), torch.zeros(2, 200, 280, 3, dtype=torch.uint8), torch.zeros(3, 200, 280, 4, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="out"):
            torch_io.upscale_sequence(s, frames, out=_on_cuda0(bad))
    with pytest.raises(ValueError, match="out"):
        torch_io.upscale_sequence(s, frames, out=[_on_cuda0(torch.zeros(200, 280, 3, dtype=torch.uint8))] * 3)  # (a list for a stacked input)
    with pytest.raises(ValueError, match="stacked"):
        torch_io.upscale_sequence(s, _on_cuda0(torch.zeros(3, 75, 70, dtype=torch.uint8)))  # (surfaces come as a list)
    with pytest.raises(ValueError, match="non-empty"):
        torch_io.upscale_sequence(s, [])
    assert s.calls == []


def test_the_binding_hands_descriptors_and_masks_over():
    """RealSR.diff_tiles_sequence / process_device_sequence against a stand-in for the C library."""
    seen = {}

    class _Lib:
        def rsr_set_params(self, *a):
            return 0

        def rsr_diff_tiles_sequence(self, h, n, frames, prev, fmt, w, hh, c, d_masks, stream):
            seen["diff"] = (n, [(frames[i].data, frames[i].row_pitch) for i in range(n)], prev and prev[0].data, fmt, w, hh, c, d_masks.value, stream.value)
            return 0

        def rsr_process_device_sequence(self, h, n, src, in_fmt, w, hh, c, dst, out_fmt, prev, masks, nmask, stream):
            seen["seq"] = (n, [src[i].data for i in range(n)], in_fmt, w, hh, c, [(dst[i].data, dst[i].row_pitch) for i in range(n)], out_fmt,
                           prev and (prev[0].data, prev[0].row_pitch), bytes((R.C.c_uint8 * nmask).from_address(masks.value)), nmask, stream)
            return 0

        def rsr_last_error(self, h):
            return b"bad argument"

    sr = R.RealSR(0, _adopt=1)  # (adopts a handle: no device is opened)
    sr._L = _Lib()
    sr.tilesize, sr.prepadding = 32, 10
    sr.diff_tiles_sequence([4096, (8192, 256, 0)], None, NV12, 70, 50, 3, 12288, stream=5)
    assert seen["diff"] == (2, [(4096, 0), (8192, 256)], None, NV12, 70, 50, 3, 12288, 5)
    sr.diff_tiles_sequence([4096], 64, U8, 70, 50, 3, 12288, stream=5)
    assert seen["diff"][2] == 64
    sr.process_device_sequence([4096, 8192], U8, 70, 50, 3, [(16384, 900, 0), 32768], U8, [[0, 1, 0, 0, 7, 0], [1, 0, 0, 0, 0, 0]], prev_out=(16384, 900, 0))
    assert seen["seq"] == (2, [4096, 8192], U8, 70, 50, 3, [(16384, 900), (32768, 0)], U8, (16384, 900), bytes([0, 1, 0, 0, 7, 0, 1, 0, 0, 0, 0, 0]), 12, None)
    with pytest.raises(ValueError):
        sr.process_device_sequence([4096, 8192], U8, 70, 50, 3, [16384], U8, [1] * 12)
    sr._h = None
