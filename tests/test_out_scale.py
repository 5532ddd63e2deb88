"""Option "out_scale" (x2 / x1 output, box-reduced on the device): what can be said without a GPU -- the documented contract, how
torch_io.upscale sizes and checks `out`, the numpy reference the device tests compare against, and the share of uint8 results an fma
contraction could move.  The device side is tests/test_gpu_out_scale.py."""
import os
import subprocess

import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

from box_reduce import box_reduce, u8_expected

F16, F32 = R.RSR_FMT_F16_CHW, R.RSR_FMT_F32_CHW


def test_header_documents_out_scale():
    text = open(os.path.join(R.INCLUDE_DIR, "realsr_hip.h")).read()
    assert '"out_scale"' in text
    for needle in ("0.25f", "0.0625f", "(w * out_scale) x (h * out_scale)"):
        assert needle in text, needle


def test_binding_has_the_property():
    assert isinstance(R.RealSR.out_scale, property) and R.RealSR.out_scale.fset is not None


class _Engine:
    """Stands in for the C library behind a RealSR: holds the option as the engine does and records the size of every rsr_process."""

    def __init__(self):
        self.out_scale, self.calls = 4, []

    def rsr_set_option(self, h, key, value):
        if key == b"out_scale":
            if value not in (1, 2, 4):
                return R.RSR_E_ARG
            self.out_scale = value
        return 0

    def rsr_get_stat(self, h, key, ref):
        ref._obj.value = {b"out_scale": self.out_scale}[key]
        return 0

    def rsr_set_params(self, *a):
        return 0

    def rsr_process(self, h, src, w, h_, c, dst):
        self.calls.append((w, h_, c))
        return 0

    def rsr_last_error(self, h):
        return b"bad argument"

    def rsr_destroy(self, h):
        pass


def _binding_over(engine):
    sr = R.RealSR(0, _adopt=1)  # (adopts a handle: no device is opened)
    sr._L = engine
    return sr


def test_set_option_and_the_property_cannot_disagree(monkeypatch):
    """The binding keeps no copy of the option: whichever way it was set, out_scale reads what the engine will use, and outputs are
    sized with that -- a stale copy would hand the engine a x2 buffer for a x4 image."""
    e = _Engine()
    monkeypatch.setattr(R, "lib", lambda: e)
    sr = _binding_over(e)
    img = np.zeros((6, 10, 3), dtype=np.uint8)
    assert sr.out_scale == 4 and sr.process(img).shape == (24, 40, 3)
    sr.set_option("out_scale", 2)
    assert sr.out_scale == 2 and sr.process(img).shape == (12, 20, 3)
    sr.out_scale = 1
    assert e.out_scale == 1 and sr.process(img).shape == (6, 10, 3)
    sr.out_scale = 2
    sr.set_option("out_scale", 4)  # the order that overflowed with a copy in the binding
    assert sr.out_scale == 4 and sr.process(img).shape == (24, 40, 3)
    with pytest.raises(AssertionError):
        sr.process(img, out=np.zeros((12, 20, 3), dtype=np.uint8))
    with pytest.raises(R.RealSRError):
        sr.set_option("out_scale", 3)
    assert sr.out_scale == 4
    assert len(e.calls) == 4  # (the refused `out` never reached the engine)
    sr._h = None


class _Stream:
    cuda_stream = 5  # (not the null stream: upscale then enqueues on it directly)


class _Ctx:
    """A context that records what torch_io.upscale hands the engine instead of running it."""
    gpuid, scale = 0, 4

    def __init__(self):
        self.calls = []

    def process_device_fmt(self, *a, **k):
        self.calls.append(("fmt", a, k))

    def process_device_batch(self, *a, **k):
        self.calls.append(("batch", a, k))


class _Ctx2(_Ctx):
    out_scale = 2


class _Cuda0(torch.Tensor):
    """A CPU tensor that claims to live on cuda:0 (tests/test_tensor_batch.py)."""
    @property
    def device(self):
        return torch.device("cuda", 0)


def _on_cuda0(t):
    return t.as_subclass(_Cuda0)


@pytest.fixture
def fake_stream(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _Stream())


def test_upscale_rejects_a_4x_out_at_out_scale_2(fake_stream):
    s = _Ctx2()
    x = _on_cuda0(torch.zeros(3, 8, 12, dtype=torch.float16))
    with pytest.raises(ValueError, match="out"):
        torch_io.upscale(s, x, out=_on_cuda0(torch.zeros(3, 32, 48, dtype=torch.float16)))
    assert s.calls == []


def test_upscale_hands_the_engine_2x_descriptors(fake_stream):
    s = _Ctx2()
    x = _on_cuda0(torch.zeros(3, 8, 12, dtype=torch.float16))
    out = _on_cuda0(torch.zeros(3, 16, 24, dtype=torch.float16))
    y = torch_io.upscale(s, x, out=out)
    assert y is out
    (kind, a, k), = s.calls
    assert kind == "fmt" and a == (x.data_ptr(), F16, 12, 8, 3, out.data_ptr(), F16) and k == {"stream": 5}
    # a window of a canvas, a batch: the 2x windows' pointers and pitches (bytes)
    s = _Ctx2()
    xb = _on_cuda0(torch.zeros(2, 3, 8, 12, dtype=torch.float32))
    canvas = torch.zeros(2, 3, 40, 64, dtype=torch.float32)
    win = _on_cuda0(canvas[..., 6:22, 10:34])
    torch_io.upscale(s, xb, out=win)
    (kind, a, k), = s.calls
    assert kind == "batch"
    ins, fmt, w, h, c, outs, ofmt = a
    p0 = canvas.data_ptr() + (6 * 64 + 10) * 4
    assert (fmt, w, h, c, ofmt) == (F32, 12, 8, 3, F32)
    assert outs == [(p0, 256, 40 * 256), (p0 + 3 * 40 * 256, 256, 40 * 256)]
    assert ins == [(xb.data_ptr(), 48, 8 * 48), (xb.data_ptr() + 3 * 8 * 48, 48, 8 * 48)]


def test_upscale_without_the_attribute_behaves_as_before(fake_stream):
    s = _Ctx()
    x = _on_cuda0(torch.zeros(3, 8, 12, dtype=torch.float16))
    with pytest.raises(ValueError, match="out"):
        torch_io.upscale(s, x, out=_on_cuda0(torch.zeros(3, 16, 24, dtype=torch.float16)))
    assert s.calls == []
    out = _on_cuda0(torch.zeros(3, 32, 48, dtype=torch.float16))
    torch_io.upscale(s, x, out=out)
    (kind, a, k), = s.calls
    assert kind == "fmt" and a == (x.data_ptr(), F16, 12, 8, 3, out.data_ptr(), F16)


# ---- the numpy reference -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 4])
def test_box_reduce_is_the_clamped_average(k):
    v = np.random.default_rng(5).uniform(-0.2, 1.2, size=(3, 48, 64)).astype(np.float32)
    want = torch.nn.functional.avg_pool2d(torch.from_numpy(v).clamp(0, 1).double()[None], k)[0].numpy()
    got = box_reduce(v, k)
    assert got.dtype == np.float32 and got.shape == (3, 48 // k, 64 // k)
    assert np.abs(got.astype(np.float64) - want).max() <= 1e-6
    assert got.min() >= 0 and got.max() <= 1


@pytest.mark.parametrize("k", [2, 4])
def test_box_reduce_is_exact_where_every_sum_is(k):
    """Multiples of 2^-10 up to 1 are fp16 values; sums of sixteen of them are multiples of 2^-10 below 2^5: exact in float32, whatever
    the order.  The mean, another division by a power of two, is exact too: it must equal the float64 mean bit for bit."""
    m = np.random.default_rng(6).integers(0, 1025, size=(3, 40, 56))
    v = (m / 1024.0).astype(np.float16)
    assert np.array_equal(v.astype(np.float64) * 1024, m)
    want = m.reshape(3, 40 // k, k, 56 // k, k).sum(axis=(2, 4)) / (1024.0 * k * k)
    got = box_reduce(v.astype(np.float32), k)
    assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert np.array_equal(got.astype(np.float64), want)


def test_box_reduce_keeps_the_stated_order():
    """A box whose float32 sum depends on the order: 1 + 2^-24 + 2^-24 + ... only survives when the small terms meet first."""
    e = np.float32(2.0 ** -24)
    box = np.array([[0.5, 0.5], [e, e]], dtype=np.float32)  # (0.5 + 0.5) + (e + e) = 1 + 2^-23, representable; ((0.5 + 0.5) + e) + e = 1
    assert box_reduce(box, 2)[0, 0] == np.float32((1 + 2.0 ** -23) * 0.25)
    b4 = np.zeros((4, 4), dtype=np.float32)
    b4[0, :] = [0.5, 0.5, e, e]
    assert box_reduce(b4, 4)[0, 0] == np.float32((1 + 2.0 ** -23) * 0.0625)
    b4[:] = 0  # the same between rows: s0 = 1, s1 = 0, s2 = s3 = e: (s0 + s1) + (s2 + s3)
    b4[0, :] = 0.25
    b4[2, 0] = b4[3, 3] = e
    assert box_reduce(b4, 4)[0, 0] == np.float32((1 + 2.0 ** -23) * 0.0625)


def test_uint8_rule_leaves_out_few_elements(oracle_net):
    """Step 3 is checked against floor(float64(d) * 255 + 0.5) except where that lies within 2^-14 of an integer; the share left out is
    capped at 1e-3.  On the box means of a real network output -- the fp32 oracle on the whole 40 x 30 test image, one padded
    tile as at tile size 100: 57,600 means at k = 2 and 14,400 at k = 4, so the cap allows 57 and 14 elements -- it stays far below (a
    uniformly spread d gives 2 * 2^-14 = 1.2e-4)."""
    from oracle_pool import padded_tile
    img = np.random.default_rng(7000 + 10 * 40).integers(0, 256, size=(30, 40, 3), dtype=np.uint8)
    o = oracle_net.forward(np.ascontiguousarray(padded_tile(img, 0, 0, 40, 30)))[:, 40:-40, 40:-40].astype(np.float32)
    assert o.shape == (3, 120, 160)
    for k in (2, 4):
        d = box_reduce(o, k)
        q, near = u8_expected(d)
        assert near.mean() <= 1e-3, (k, near.mean())
        assert q.dtype == np.uint8 and len(np.unique(q)) > 16  # (the output is an image, not a constant)


def test_cli_refuses_a_bad_out_scale_before_anything_else(tmp_path):
    """RSR_OUT_SCALE is checked with the flags: no image is read (the input does not even exist), no GPU is touched."""
    cli = os.path.join(os.path.dirname(R.LIB_PATH), "..", "bin", "realsr-hip")
    for bad in ("3", "0", "8", "2x", ""):
        r = subprocess.run([cli, "-i", str(tmp_path / "missing.png"), "-o", str(tmp_path / "o.png")], capture_output=True, text=True,
                           env=dict(os.environ, RSR_OUT_SCALE=bad), timeout=60)
        assert r.returncode != 0 and "invalid RSR_OUT_SCALE" in r.stderr, (bad, r.stderr)
