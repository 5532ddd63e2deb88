"""torch_io.pack_planes / unpack_planes without a GPU: what they hand the context -- pointers, pitches in bytes, format, size, stream --
and that every refusal comes before anything is launched.  The context is a recorder; the tensors are CPU tensors that claim to live on
cuda:0 (the pattern of tests/test_yuv444.py)."""
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
from realsr_ncnn_vulkan_amd import torch_io

import pixfmt_ref as F


class _Stream:
    cuda_stream = 5  # (not the null stream: the call is enqueued on it directly)


class _Ctx:
    gpuid, scale, out_scale, tilesize = 0, 4, 4, 16

    def __init__(self):
        self.calls = []

    def pack_planes(self, *a, **k):
        self.calls.append(("pack", a, k))

    def unpack_planes(self, *a, **k):
        self.calls.append(("unpack", a, k))


class _Cuda0(torch.Tensor):
    @property
    def device(self):
        return torch.device("cuda", 0)


def _on_cuda0(t):
    return t.as_subclass(_Cuda0)


@pytest.fixture(autouse=True)
def fake_stream(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _Stream())


def z(*shape, dtype=torch.uint8):
    return _on_cuda0(torch.zeros(*shape, dtype=dtype))


def test_no_python_format_name_was_added():
    assert sorted(getattr(R, n) for n in dir(R) if n.startswith("RSR_FMT_")) == sorted(F.FORMATS)
    assert not [n for n in dir(torch_io) if n.startswith("RSR_FMT_") and not hasattr(R, n)]


@pytest.mark.parametrize("chroma,dtype,fmt,cshape,sshape", [
    (420, torch.uint8, F.NV12, (13, 18), (39, 36)), (420, torch.int16, F.P010, (13, 18), (39, 36)),
    (422, torch.uint8, F.NV16, (26, 18), (52, 36)), (422, torch.int16, F.P210, (26, 18), (52, 36)),
    (444, torch.uint8, F.YUV444P, (26, 36), (3, 26, 36)), (444, torch.int16, F.YUV444P10, (26, 36), (3, 26, 36))])
def test_pack_and_unpack_describe_packed_tensors(chroma, dtype, fmt, cshape, sshape):
    es = 1 if dtype == torch.uint8 else 2
    s = _Ctx()
    y, u, v = z(26, 36, dtype=dtype), z(*cshape, dtype=dtype), z(*cshape, dtype=dtype)
    surf = torch_io.pack_planes(s, y, u, v, chroma=chroma)
    assert tuple(surf.shape) == sshape and surf.dtype == dtype
    (kind, a, k), = s.calls
    plane = 26 * 36 * es
    assert kind == "pack" and k == {"stream": 5}
    assert a == ([(y.data_ptr(), u.data_ptr(), v.data_ptr(), 36 * es, cshape[1] * es)], [(surf.data_ptr(), 36 * es, plane)], fmt, 36, 26)
    s = _Ctx()
    got = torch_io.unpack_planes(s, _on_cuda0(surf), chroma=chroma)
    assert [tuple(p.shape) for p in got] == [(26, 36), cshape, cshape] and all(p.dtype == dtype for p in got)
    (kind, a, k), = s.calls
    assert kind == "unpack" and k == {"stream": 5}
    assert a == ([(surf.data_ptr(), 36 * es, plane)], [(got[0].data_ptr(), got[1].data_ptr(), got[2].data_ptr(), 36 * es, cshape[1] * es)], fmt, 36, 26)


def test_views_go_by_pointer_and_pitch_and_out_is_written_in_place():
    s = _Ctx()
    big = torch.zeros(40, 64, dtype=torch.int16)
    cpool = torch.zeros(2, 20, 32, dtype=torch.int16)
    y, u, v = _on_cuda0(big[3:29, 5:41]), _on_cuda0(cpool[0, 2:15, 1:19]), _on_cuda0(cpool[1, 2:15, 1:19])
    canvas = torch.zeros(60, 100, dtype=torch.int16)
    out = _on_cuda0(canvas[7:46, 10:46])
    assert torch_io.pack_planes(s, y, u, v, out=out) is out
    (_, a, _), = s.calls
    assert a[0] == [(big.data_ptr() + 2 * (3 * 64 + 5), cpool.data_ptr() + 2 * (2 * 32 + 1), cpool.data_ptr() + 2 * (20 * 32 + 2 * 32 + 1), 128, 64)]
    assert a[1] == [(canvas.data_ptr() + 2 * (7 * 100 + 10), 200, 26 * 200)] and a[2:] == (F.P010, 36, 26)
    # planes that fit no descriptor (a step along W; u and v with different row strides) are made contiguous first
    s = _Ctx()
    torch_io.pack_planes(s, _on_cuda0(torch.zeros(26, 72, dtype=torch.uint8)[:, ::2]), z(13, 18), z(13, 18))
    assert s.calls[0][1][0][0][3:] == (36, 18)
    s = _Ctx()
    torch_io.pack_planes(s, z(26, 36), _on_cuda0(torch.zeros(13, 20, dtype=torch.uint8)[:, :18]), _on_cuda0(torch.zeros(13, 24, dtype=torch.uint8)[:, :18]))
    assert s.calls[0][1][0][0][3:] == (36, 18)
    # unpack into given planes: a (y, uv) pair as upscale_yuv returns it, pitched chroma planes out
    s = _Ctx()
    padded = z(48, 36)
    ys, uvs = padded[:26], padded[32:45]
    oy, ou, ov = z(26, 36), _on_cuda0(cpool.view(torch.uint8)[0, :13, :18]), _on_cuda0(cpool.view(torch.uint8)[1, :13, :18])
    got = torch_io.unpack_planes(s, (ys, uvs), out=(oy, ou, ov))
    assert got[0] is oy and got[1] is ou and got[2] is ov
    (_, a, _), = s.calls
    assert a[0] == [(padded.data_ptr(), 36, 32 * 36)]
    assert a[1] == [(oy.data_ptr(), ou.data_ptr(), ov.data_ptr(), 36, 64)]


BAD_PACK = {
    "cpu": lambda: (torch.zeros(26, 36, dtype=torch.uint8), z(13, 18), z(13, 18), {}),
    "float": lambda: (z(26, 36, dtype=torch.float16), z(13, 18, dtype=torch.float16), z(13, 18, dtype=torch.float16), {}),
    "mixed-dtypes": lambda: (z(26, 36), z(13, 18, dtype=torch.int16), z(13, 18), {}),
    "3d": lambda: (z(1, 26, 36), z(13, 18), z(13, 18), {}),
    "odd-w-420": lambda: (z(26, 35), z(13, 17), z(13, 17), {}),
    "odd-h-420": lambda: (z(25, 36), z(12, 18), z(12, 18), {}),
    "odd-w-422": lambda: (z(26, 35), z(26, 17), z(26, 17), {"chroma": 422}),
    "chroma-size-420": lambda: (z(26, 36), z(26, 18), z(26, 18), {}),
    "chroma-size-422": lambda: (z(26, 36), z(13, 18), z(13, 18), {"chroma": 422}),
    "chroma-size-444": lambda: (z(26, 36), z(26, 18), z(26, 18), {"chroma": 444}),
    "u-v-differ": lambda: (z(26, 36), z(13, 18), z(13, 16), {}),
    "chroma-411": lambda: (z(26, 36), z(26, 9), z(26, 9), {"chroma": 411}),
    "out-size": lambda: (z(26, 36), z(13, 18), z(13, 18), {"out": z(39, 38)}),
    "out-dtype": lambda: (z(26, 36), z(13, 18), z(13, 18), {"out": z(39, 36, dtype=torch.int16)}),
    "out-chroma": lambda: (z(26, 36), z(13, 18), z(13, 18), {"out": z(52, 36)}),
    "out-stepped": lambda: (z(26, 36), z(13, 18), z(13, 18), {"out": _on_cuda0(torch.zeros(39, 72, dtype=torch.uint8)[:, ::2])}),
    "out-444-2d": lambda: (z(26, 36), z(26, 36), z(26, 36), {"chroma": 444, "out": z(78, 36)}),
}


@pytest.mark.parametrize("case", sorted(BAD_PACK))
def test_pack_planes_refuses_before_launching(case):
    y, u, v, kw = BAD_PACK[case]()
    s = _Ctx()
    with pytest.raises(ValueError) as e:
        torch_io.pack_planes(s, y, u, v, **kw)
    assert "pack_planes" in str(e.value) and s.calls == []


BAD_UNPACK = {
    "cpu": lambda: (torch.zeros(39, 36, dtype=torch.uint8), {}),
    "float": lambda: (z(39, 36, dtype=torch.float32), {}),
    "rows-420": lambda: (z(40, 36), {}),
    "odd-w": lambda: (z(39, 35), {}),
    "3d-for-420": lambda: (z(3, 26, 36), {}),
    "2d-for-444": lambda: (z(78, 36), {"chroma": 444}),
    "chroma": lambda: (z(39, 36), {"chroma": 400}),
    "stepped": lambda: (_on_cuda0(torch.zeros(39, 72, dtype=torch.uint8)[:, ::2]), {}),
    "out-not-three": lambda: (z(39, 36), {"out": (z(26, 36), z(13, 36))}),
    "out-tensor": lambda: (z(39, 36), {"out": z(39, 36)}),
    "out-size": lambda: (z(39, 36), {"out": (z(26, 36), z(13, 18), z(13, 16))}),
    "out-other-frame": lambda: (z(39, 36), {"out": (z(28, 36), z(14, 18), z(14, 18))}),
    "out-dtype": lambda: (z(39, 36), {"out": (z(26, 36, dtype=torch.int16), z(13, 18, dtype=torch.int16), z(13, 18, dtype=torch.int16))}),
    "out-stepped": lambda: (z(39, 36), {"out": (z(26, 36), _on_cuda0(torch.zeros(13, 36, dtype=torch.uint8)[:, ::2]), z(13, 18))}),
    "out-pitches-differ": lambda: (z(39, 36), {"out": (z(26, 36), _on_cuda0(torch.zeros(13, 20, dtype=torch.uint8)[:, :18]), _on_cuda0(torch.zeros(13, 24, dtype=torch.uint8)[:, :18]))}),
}


@pytest.mark.parametrize("case", sorted(BAD_UNPACK))
def test_unpack_planes_refuses_before_launching(case):
    surf, kw = BAD_UNPACK[case]()
    s = _Ctx()
    with pytest.raises(ValueError) as e:
        torch_io.unpack_planes(s, surf, **kw)
    assert "unpack_planes" in str(e.value) and s.calls == []
