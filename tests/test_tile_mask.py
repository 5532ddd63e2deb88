"""Masked tile processing and the frame diff without a GPU: the host-only tile geometry (rsr_tile_count, rsr_tile_source_rect) against
tests/tile_diff_ref.py, the argument that a tile reads nothing outside its source rectangle, the header's definitions, and
torch_io.upscale_delta against a context that records what it is handed.  The GPU side: tests/test_gpu_tile_mask.py."""
import os

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

import tile_diff_ref as ref

U8, F16, F32, NV12, P010 = R.RSR_FMT_U8_HWC, R.RSR_FMT_F16_CHW, R.RSR_FMT_F32_CHW, R.RSR_FMT_NV12, R.RSR_FMT_P010

# (w, h, T, P): w <= P, T > w, partial last tiles, exact multiples, one-pixel last tiles, no halo, the C2 frame
SWEEP = [(70, 50, 32, 10), (7, 5, 32, 10), (10, 10, 4, 10), (9, 33, 8, 10), (64, 64, 32, 10), (65, 33, 32, 10), (230, 36, 200, 10),
         (1920, 1080, 200, 10), (50, 70, 32, 0), (31, 31, 31, 3), (100, 3, 16, 18), (1, 1, 1, 0), (1, 1, 200, 10)]


@pytest.mark.parametrize("w,h,T,P", SWEEP)
def test_geometry_against_the_reference(w, h, T, P):
    nx, ny = R.tile_count(w, h, T)
    assert (nx, ny) == ref.tile_count(w, h, T)
    for t in range(nx * ny):
        r = R.tile_source_rect(w, h, T, P, t)
        assert r == ref.source_rect(w, h, T, P, t), t
        assert 0 <= r[0] < r[2] <= w and 0 <= r[1] < r[3] <= h


def test_tile_count_of_the_c2_frame_and_the_base_case():
    assert R.tile_count(1920, 1080, 200) == (10, 6)
    assert R.tile_count(70, 50, 32) == (3, 2)
    assert [R.tile_source_rect(70, 50, 32, 10, t)[::2] for t in range(3)] == [(0, 42), (22, 70), (54, 70)]


@pytest.mark.parametrize("w,h,T,P", [(70, 50, 32, 10), (7, 5, 32, 10), (10, 10, 4, 10), (9, 33, 8, 10), (230, 36, 200, 10), (100, 3, 16, 18)])
def test_a_padded_tile_samples_nothing_outside_its_rectangle(w, h, T, P):
    nx, ny = ref.tile_count(w, h, T)
    for t in range(nx * ny):
        xs, ys = ref.sampled(w, h, T, P, t)
        x0, y0, x1, y1 = R.tile_source_rect(w, h, T, P, t)
        assert min(xs) >= x0 and max(xs) < x1 and min(ys) >= y0 and max(ys) < y1, (t, sorted(xs), (x0, x1), sorted(ys), (y0, y1))


def test_error_codes():
    for args in ((0, 5, 32), (5, 0, 32), (5, 5, 0), (-1, 5, 32)):
        with pytest.raises(R.RealSRError) as e:
            R.tile_count(*args)
        assert e.value.code == R.RSR_E_ARG
    for args in ((70, 50, 32, 10, 6), (70, 50, 32, 10, -1), (70, 50, 32, -1, 0), (0, 50, 32, 10, 0), (70, 50, 0, 10, 0)):
        with pytest.raises(R.RealSRError) as e:
            R.tile_source_rect(*args)
        assert e.value.code == R.RSR_E_ARG
    L = R.lib()
    assert L.rsr_tile_count(70, 50, 32, None, None) == 0  # (any pointer may be NULL)
    assert L.rsr_tile_source_rect(70, 50, 32, 10, 5, None, None, None, None) == 0
    for name in ("rsr_tile_count", "rsr_tile_source_rect", "rsr_diff_tiles", "rsr_process_device_masked"):
        assert name in R.EXPORTS and hasattr(L, name)


def test_header_carries_the_definitions():
    text = open(os.path.join(R.INCLUDE_DIR, "realsr_hip.h")).read()
    for needle in ("int rsr_tile_count(", "int rsr_tile_source_rect(", "int rsr_diff_tiles(", "int rsr_process_device_masked(",
                   "sx0 = max(xi * T - P, 0)", "sx1 = min(min((xi + 1) * T, w) + P, w)", "reflect101(xi * T - P + gx)",
                   "bytes [sx0 * c, sx1 * c) of rows sy0 .. sy1 - 1", "Alpha is included", "-0.0 against 0.0",
                   "max((sx0 >> 1) - 1, 0) .. min(((sx1 - 1) >> 1) + 1, w / 2 - 1)", "whole 16-bit words", "Every mask byte is written",
                   "no other byte of `out` is touched", "No tile set", "Every tile set", "nmask != nx * ny", "all three rotating table buffers",
                   '"masked_calls"', '"masked_tiles_run"', '"masked_tiles_skipped"', '"masked_batches"',
                   "Out of scope: n > 1, host-pointer images, groups of GPUs, the CLI, merging with concurrent calls"):
        assert needle in text, needle


# ---- torch_io.upscale_delta against a recording context -----------------------------------------------------------------------------------
class _Stream:
    cuda_stream = 5

    def __init__(self, log):
        self.log = log

    def synchronize(self):
        self.log.append(("sync",))


class _Ctx:
    """Records what torch_io hands the engine, at tile 32 and out_scale 4; diff_tiles marks the tiles `changed`."""
    gpuid, scale, out_scale, tilesize, prepadding = 0, 4, 4, 32, 10

    def __init__(self, changed=()):
        self.calls, self.changed = [], changed

    def out_size(self, w, h):
        return 4 * w, 4 * h

    def tile_count(self, w, h):
        return ref.tile_count(w, h, self.tilesize)

    def diff_tiles(self, a, b, fmt, w, h, c, d_mask, stream=None):
        self.calls.append(("diff", a, b, fmt, w, h, c, d_mask, stream))
        self.d_mask_tensor[:] = 0
        for t in self.changed:
            self.d_mask_tensor[t] = 1

    def process_device_masked(self, src, in_fmt, w, h, c, dst, out_fmt, mask, stream=None):
        self.calls.append(("masked", src, in_fmt, w, h, c, dst, out_fmt, np.array(mask, dtype=np.uint8).copy(), stream))


class _Cuda0(torch.Tensor):
    @property
    def device(self):
        return torch.device("cuda", 0)


def _on_cuda0(t):
    return t.as_subclass(_Cuda0)


@pytest.fixture
def fake(monkeypatch):
    """torch_io with a recording stream, pageable 'pinned' memory and a context whose device mask is the tensor torch_io allocates."""
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


def test_upscale_delta_diffs_then_runs_the_masked_call(fake):
    s = fake
    s.changed = (1, 4)
    x, px = _on_cuda0(torch.zeros(50, 70, 3, dtype=torch.uint8)), _on_cuda0(torch.zeros(50, 70, 3, dtype=torch.uint8))
    y = _on_cuda0(torch.zeros(200, 280, 3, dtype=torch.uint8))
    out, n = torch_io.upscale_delta(s, x, px, y)
    assert out is y and n == 2
    kinds = [c[0] for c in s.calls]
    assert kinds == ["diff", "sync", "masked"]  # one synchronisation, between the two
    d, m = s.calls[0], s.calls[2]
    assert d[1] == (px.data_ptr(), 210, 0) and d[2] == (x.data_ptr(), 210, 0) and d[3:7] == (U8, 70, 50, 3) and d[8] == 5
    assert d[7] == s.d_mask_tensor.data_ptr() and s.d_mask_tensor.numel() == 6
    assert m[1] == (x.data_ptr(), 210, 0) and m[2:6] == (U8, 70, 50, 3) and m[6] == (y.data_ptr(), 840, 0) and m[7] == U8 and m[9] == 5
    assert m[8].tolist() == [0, 1, 0, 0, 1, 0]


def test_upscale_delta_without_a_previous_frame_runs_every_tile(fake):
    s = fake
    x = _on_cuda0(torch.zeros(3, 50, 70, dtype=torch.float16))
    y = _on_cuda0(torch.zeros(3, 200, 280, dtype=torch.float16))
    out, n = torch_io.upscale_delta(s, x, None, y)
    assert out is y and n == 6
    (m,) = s.calls  # no diff, no synchronisation
    assert m[0] == "masked" and m[8].tolist() == [1] * 6 and m[2] == F16 and m[6] == (y.data_ptr(), 560, 200 * 560)


def test_upscale_delta_passes_views_by_descriptor_and_copies_prev_y_into_out(fake):
    s = fake
    frame = torch.zeros(3, 80, 100, dtype=torch.float32)
    prev = torch.zeros(3, 80, 100, dtype=torch.float32)
    x, px = _on_cuda0(frame[:, 7:57, 11:81]), _on_cuda0(prev[:, 7:57, 11:81])
    y = _on_cuda0(torch.full((3, 200, 280), 0.25, dtype=torch.float32))
    canvas = torch.zeros(3, 300, 400, dtype=torch.float32)
    win = _on_cuda0(canvas[:, 20:220, 40:320])
    out, n = torch_io.upscale_delta(s, x, px, y, out=win)
    assert out is win and n == 0 and float(canvas[:, 20:220, 40:320].min()) == 0.25 and float(canvas.sum()) == 0.25 * 3 * 200 * 280
    d, m = s.calls[0], s.calls[2]
    off = (7 * 100 + 11) * 4
    assert d[1] == (prev.data_ptr() + off, 400, 80 * 400) and d[2] == (frame.data_ptr() + off, 400, 80 * 400)
    assert m[1] == d[2] and m[6] == (canvas.data_ptr() + (20 * 400 + 40) * 4, 1600, 300 * 1600)
    assert m[8].tolist() == [0] * 6


def test_upscale_delta_takes_surfaces(fake):
    s = fake
    s.changed = (0,)
    x, px = _on_cuda0(torch.zeros(75, 70, dtype=torch.uint8)), _on_cuda0(torch.zeros(75, 70, dtype=torch.uint8))
    y = _on_cuda0(torch.zeros(300, 280, dtype=torch.uint8))
    out, n = torch_io.upscale_delta(s, x, px, y)
    assert out is y and n == 1
    d, m = s.calls[0], s.calls[2]
    assert d[3:7] == (NV12, 70, 50, 3) and d[2] == (x.data_ptr(), 70, 50 * 70)
    assert m[6] == (y.data_ptr(), 280, 200 * 280) and m[7] == NV12


def test_upscale_delta_refuses_mismatches_before_anything_is_launched(fake):
    s = fake
    x, px = _on_cuda0(torch.zeros(50, 70, 3, dtype=torch.uint8)), _on_cuda0(torch.zeros(50, 70, 3, dtype=torch.uint8))
    y = _on_cuda0(torch.zeros(200, 280, 3, dtype=torch.uint8))
    for bad_y in (torch.zeros(200, 276, 3, dtype=torch.uint8), torch.zeros(100, 140, 3, dtype=torch.uint8), torch.zeros(200, 280, 4, dtype=torch.uint8),
                  torch.zeros(3, 200, 280, dtype=torch.float16)):
        with pytest.raises(ValueError, match="prev_y"):
            torch_io.upscale_delta(s, x, px, _on_cuda0(bad_y))
    with pytest.raises(ValueError, match="prev_x"):
        torch_io.upscale_delta(s, x, _on_cuda0(torch.zeros(50, 66, 3, dtype=torch.uint8)), y)
    with pytest.raises(ValueError, match="prev_x"):
        torch_io.upscale_delta(s, x, _on_cuda0(torch.zeros(3, 50, 70, dtype=torch.float16)), y)
    with pytest.raises(ValueError, match="out"):
        torch_io.upscale_delta(s, x, px, y, out=_on_cuda0(torch.zeros(200, 280, 4, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="batch"):
        torch_io.upscale_delta(s, _on_cuda0(torch.zeros(2, 3, 50, 70, dtype=torch.float16)), None, _on_cuda0(torch.zeros(2, 3, 200, 280, dtype=torch.float16)))
    assert s.calls == []


def test_the_binding_hands_the_mask_over_as_host_bytes():
    """RealSR.process_device_masked / diff_tiles / tile_count against a stand-in for the C library."""
    seen = {}

    class _Lib:
        def rsr_set_params(self, *a):
            return 0

        def rsr_process_device_masked(self, h, src, in_fmt, w, hh, c, dst, out_fmt, mask, nmask, stream):
            seen["masked"] = (src[0].data, src[0].row_pitch, in_fmt, w, hh, c, dst[0].data, out_fmt, bytes((R.C.c_uint8 * nmask).from_address(mask.value)), nmask, stream)
            return 0

        def rsr_diff_tiles(self, h, a, b, fmt, w, hh, c, d_mask, stream):
            seen["diff"] = (a[0].data, b[0].data, b[0].row_pitch, fmt, w, hh, c, d_mask.value, stream.value)
            return 0

        def rsr_tile_count(self, *a):
            return R.lib().rsr_tile_count(*a)  # (host-only: the real ones)

        def rsr_tile_source_rect(self, *a):
            return R.lib().rsr_tile_source_rect(*a)

        def rsr_last_error(self, h):
            return b"bad argument"

    sr = R.RealSR(0, _adopt=1)  # (adopts a handle: no device is opened)
    sr._L = _Lib()
    sr.tilesize, sr.prepadding = 32, 10
    assert sr.tile_count(70, 50) == (3, 2) and sr.tile_source_rect(70, 50, 4) == (22, 22, 70, 50)
    sr.process_device_masked(4096, U8, 70, 50, 3, (8192, 900, 0), U8, [0, 1, 0, 0, 7, 0])
    assert seen["masked"] == (4096, 0, U8, 70, 50, 3, 8192, U8, bytes([0, 1, 0, 0, 7, 0]), 6, None)
    sr.diff_tiles(4096, (8192, 256, 0), NV12, 70, 50, 3, 12288, stream=5)
    assert seen["diff"] == (4096, 8192, 256, NV12, 70, 50, 3, 12288, 5)
    sr._h = None
