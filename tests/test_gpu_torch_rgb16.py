"""torch_io with 16-bit RGB(A) tensors on the GPU (run with -m gpu): (H, W, 3 | 4) uint16 / int16 through upscale, upscale_delta and
upscale_sequence give the bytes of the C-level call on the same words."""
import numpy as np
import pytest
import torch

import realsr_ncnn_vulkan_amd as R
import rgb16_ref as Z
from gpu_support import context_fixtures, dev, paths  # noqa: F401
from pixfmt_ref import U8, image
from realsr_ncnn_vulkan_amd import torch_io

pytestmark = pytest.mark.gpu
U16 = R.RSR_FMT_U16_HWC
W, H, T, P = 36, 25, 16, 10
ctxs, ctx = context_fixtures(T, P)
DTYPES = [torch.uint16, torch.int16]


def c_call(s, x, in_fmt, out_fmt):
    h, w, c = x.shape
    ow, oh = s.out_size_fmt(out_fmt, w, h)
    d_in, d_out = dev(x), dev(Z.sentinel_bytes(out_fmt, (oh, ow, c)))
    s.process_device_fmt(d_in.data_ptr(), in_fmt, w, h, c, d_out.data_ptr(), out_fmt)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(Z.np_dtype(out_fmt)).reshape(oh, ow, c)


def as_t(a, dtype):
    """The numpy uint16 image as a device tensor of dtype (int16: the same words, codes >= 32768 read negative).  Everything but the
    calls under test is done on int16 views: torch implements few operators for uint16."""
    return torch.from_numpy(a.view(np.int16)).cuda().view(dtype)


def zeros(shape, dtype):
    return torch.zeros(shape, dtype=torch.int16, device="cuda").view(dtype)


def words(t):
    return t.view(torch.int16).contiguous().cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("c", [3, 4], ids=["rgb", "rgba"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["uint16", "int16"])
def test_upscale(ctx, dtype, c):
    s = ctx[False]
    img = Z.image16(300 + c, W, H, c)
    assert (img >= 32768).any()
    want = c_call(s, img, U16, U16)
    y = torch_io.upscale(s, as_t(img, dtype))
    torch.cuda.synchronize()
    assert y.dtype == dtype and tuple(y.shape) == (4 * H, 4 * W, c) and np.array_equal(words(y), want)
    s.out_scale = 2
    y = torch_io.upscale(s, as_t(img, dtype))
    torch.cuda.synchronize()
    assert tuple(y.shape) == (2 * H, 2 * W, c) and np.array_equal(words(y), c_call(s, img, U16, U16))


@pytest.mark.parametrize("dtype", DTYPES, ids=["uint16", "int16"])
def test_out_dtype_both_ways(ctx, dtype):
    s = ctx[False]
    img8, img16 = image(310, U8, W, H, 4), Z.image16(311, W, H, 4)
    y = torch_io.upscale(s, torch.from_numpy(img8).cuda(), out_dtype=dtype)   # 8 -> 16
    torch.cuda.synchronize()
    assert y.dtype == dtype and np.array_equal(words(y), c_call(s, img8, U8, U16))
    y = torch_io.upscale(s, as_t(img16, dtype), out_dtype=torch.uint8)        # 16 -> 8
    torch.cuda.synchronize()
    assert y.dtype == torch.uint8 and np.array_equal(y.cpu().numpy(), c_call(s, img16, U16, U8))
    y = torch_io.upscale(s, torch.from_numpy(img8).cuda(), out_dtype=torch.uint8)  # 8 -> 8, said aloud
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), c_call(s, img8, U8, U8))
    out = zeros((4 * H, 4 * W, 4), dtype)
    assert torch_io.upscale(s, torch.from_numpy(img8).cuda(), out=out, out_dtype=dtype) is out
    torch.cuda.synchronize()
    assert np.array_equal(words(out), c_call(s, img8, U8, U16))


@pytest.mark.parametrize("dtype", DTYPES, ids=["uint16", "int16"])
def test_crop_view_into_a_window(ctx, dtype):
    """A crop of a larger frame in, a window of a canvas out: no copies, no word outside the window changes."""
    s = ctx[False]
    img = Z.image16(320, W, H)
    want = c_call(s, img, U16, U16)
    big = zeros((H + 9, W + 12, 3), dtype)
    big.view(torch.int16)[4:4 + H, 3:3 + W] = as_t(img, torch.int16)
    crop = big[4:4 + H, 3:3 + W]
    d = torch_io.describe(crop)
    assert d is not None and d[1] == (W + 12) * 6 and d[2] == 0 and d[0] % 2 == 0 and (d[0] - big.data_ptr()) == (4 * (W + 12) + 3) * 6
    fill = 0x4D4D
    canvas = torch.full((4 * H + 8, 4 * W + 7, 3), fill, dtype=torch.int16, device="cuda").view(dtype)
    win = canvas[1:1 + 4 * H, 5:5 + 4 * W]
    got = torch_io.upscale(s, crop, out=win)
    torch.cuda.synchronize()
    assert got is win and np.array_equal(words(win), want)
    untouched = torch.ones(canvas.shape, dtype=torch.bool, device="cuda")
    untouched[1:1 + 4 * H, 5:5 + 4 * W] = False
    assert (canvas.view(torch.int16)[untouched] == fill).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["uint16", "int16"])
def test_delta_and_sequence(ctx, dtype):
    s = ctx[False]
    frames = [Z.image16(330, W, H)]
    for at in ((3, 5, 0), (20, 30, 2)):  # frame 1: the low byte of one sample of tile 0; frame 2: one of the last tile row
        f = frames[-1].copy()
        f[at] ^= 0x0001
        frames.append(f)
    want = [c_call(s, f, U16, U16) for f in frames]
    xs = [as_t(f, dtype) for f in frames]
    y0 = torch_io.upscale(s, xs[0])
    out, n = torch_io.upscale_delta(s, xs[1], xs[0], y0.view(torch.int16).clone().view(dtype))
    torch.cuda.synchronize()
    assert 0 < n < 6 and out.dtype == dtype and np.array_equal(words(out), want[1])
    ys, n = torch_io.upscale_sequence(s, xs)
    torch.cuda.synchronize()
    assert 6 < n < 18 and all(tuple(y.shape) == (4 * H, 4 * W, 3) and y.dtype == dtype for y in ys)
    for y, w_ in zip(ys, want):
        assert np.array_equal(words(y), w_)
    ys, n2 = torch_io.upscale_sequence(s, torch.stack([x.view(torch.int16) for x in xs]).view(dtype))  # a stacked (N, H, W, 3) tensor
    torch.cuda.synchronize()
    assert n2 == n and tuple(ys.shape) == (3, 4 * H, 4 * W, 3) and all(np.array_equal(words(ys[k]), want[k]) for k in range(3))


def test_value_errors(ctx):
    s = ctx[False]
    x = as_t(Z.image16(340, W, H), torch.int16)
    with pytest.raises(ValueError, match="out must be a torch.int16 tensor"):
        torch_io.upscale(s, x, out=torch.zeros(4 * H, 4 * W, 3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="out must be a torch.uint8 tensor"):
        torch_io.upscale(s, x, out=torch.zeros(4 * H, 4 * W, 3, dtype=torch.int16, device="cuda"), out_dtype=torch.uint8)
    with pytest.raises(ValueError, match="out_dtype"):
        torch_io.upscale(s, x, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="out_dtype"):
        torch_io.upscale(s, torch.zeros(3, H, W, dtype=torch.float16, device="cuda"), out_dtype=torch.int16)
    with pytest.raises(ValueError, match="16-bit tensor must be"):
        torch_io.upscale(s, torch.zeros(H, W, 2, dtype=torch.int16, device="cuda"))
    # an odd-strided view: every second column of a wider image fits no descriptor as an output ...
    wide = torch.zeros(4 * H, 8 * W, 3, dtype=torch.int16, device="cuda")
    assert torch_io.describe(wide[:, ::2]) is None
    with pytest.raises(ValueError, match="not addressable by row and plane pitch"):
        torch_io.upscale(s, x, out=wide[:, ::2])
    # ... and a view into the bytes at an odd address is no 16-bit image at all
    raw = torch.zeros(2 * H * W * 3 + 2, dtype=torch.uint8, device="cuda")
    with pytest.raises((ValueError, RuntimeError)):
        torch_io.upscale(s, raw[1:1 + 2 * H * W * 3].view(torch.int16).reshape(H, W, 3))
    # as an INPUT an odd-strided view is made contiguous first, like a uint8 one
    src = torch.zeros(H, 2 * W, 3, dtype=torch.int16, device="cuda")
    src[:, ::2] = x
    y = torch_io.upscale(s, src[:, ::2])
    torch.cuda.synchronize()
    assert np.array_equal(words(y), c_call(s, Z.image16(340, W, H), U16, U16))
