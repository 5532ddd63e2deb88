"""torch tensors in, torch tensors out: the supported way to call the engine from a PyTorch pipeline.

    from realsr_ncnn_vulkan_amd import RealSR, torch_io
    sr = RealSR(0); sr.load(param, bin)
    y = torch_io.upscale(sr, x)        # x: (3, H, W) or (N, 3, H, W) float16 / float32 in [0, 1] on cuda:0  ->  (.., 3, 4H, 4W)
    y16 = torch_io.upscale(sr, x16)    # x16: (H, W, 3 | 4) uint16 / int16, 16-bit RGB(A)  ->  (4H, 4W, c) of the same dtype
    y16 = torch_io.upscale(sr, x8, out_dtype=torch.int16)   # an 8-bit image in, the network's sub-code precision out as 16 bits
    torch_io.upscale(sr, frame[..., y0:y1, x0:x1], out=canvas[..., 4 * y0:4 * y1, 4 * x0:4 * x1])   # views in, a window out: no copies

    yuv444 = torch_io.upscale_yuv(sr, planes, chroma=444)   # a (3, H, W) uint8 / int16 yuv444p / yuv444p10le frame -> (3, H', W'), any H and W
    nv12 = torch_io.upscale_yuv(sr, surface)   # a decoder's (3H/2, W) uint8 NV12 or 16-bit P010 surface -> the same layout at out_scale
    sr.tilesize = 200; sr.out_ratio = Fraction(3, 2); nv12_1080 = torch_io.upscale_yuv(sr, nv12_720)   # ... or at a ratio: 720p -> 1080p
    sr.tilesize = 192; sr.out_ratio_xy = (Fraction(8, 3), Fraction(9, 4)); nv12_1080 = torch_io.upscale_yuv(sr, nv12_dvd)   # ... or one per axis: 720 x 480 -> 1920 x 1080

    nv12 = torch_io.pack_planes(sr, y, u, v)   # a software decoder's yuv420p / yuv420p10le planes -> the NV12 / P010 surface above, one launch ...
    y2, u2, v2 = torch_io.unpack_planes(sr, torch_io.upscale_yuv(sr, nv12))   # ... and the result as three planes again (chroma=422 / 444 alike)

    y, n = torch_io.upscale_delta(sr, frame, prev_frame, y)   # video: only the tiles whose source changed run again, y is updated in place

    ys, n = torch_io.upscale_sequence(sr, frames)   # video, N frames known in advance: one diff, one host wait and shared launches per 16

The float tensors go through rsr_process_device_fmt / rsr_process_device_batch as they are (planar fp16 / fp32, include/realsr_hip.h): no
quantisation to uint8 on either side, no permute, no extra pass over the frame.  An (N, 3, H, W) batch is ONE call: small images share
tile batches.  A view whose rows are contiguous (a crop, a slice of a batch, a frame inside a padded surface) is passed by pointer and
pitches (describe()); anything else is made contiguous first.  The work is enqueued on torch.cuda.current_stream() and nothing here
waits for the GPU: the result is ordered on that stream like the output of any torch op.
"""
import contextlib
import types

import numpy as np
import torch

from . import (RSR_FMT_F16_CHW, RSR_FMT_F32_CHW, RSR_FMT_NV12, RSR_FMT_NV16, RSR_FMT_P010, RSR_FMT_P210, RSR_FMT_U16_HWC, RSR_FMT_U8_HWC,
               RSR_FMT_YUV444P, RSR_FMT_YUV444P10)

_FMT = {torch.float16: RSR_FMT_F16_CHW, torch.float32: RSR_FMT_F32_CHW}
# integer HWC images: uint8, and 16-bit words as int16 too (the convention of _chroma below: torch's uint16 is a late and partial dtype);
# the engine reads the words unsigned whatever the tensor calls them
_HWC = {torch.uint8: RSR_FMT_U8_HWC, torch.int16: RSR_FMT_U16_HWC}
if hasattr(torch, "uint16"):
    _HWC[torch.uint16] = RSR_FMT_U16_HWC
_HWC_FMTS = (RSR_FMT_U8_HWC, RSR_FMT_U16_HWC)


def _check(sr, x):
    """Validate x against the context; returns (format, batched).  Raises ValueError: nothing has been launched then."""
    if not isinstance(x, torch.Tensor):
        raise ValueError("upscale: x must be a torch.Tensor, not %s" % type(x).__name__)
    if x.device.type != "cuda" or x.device.index != sr.gpuid:
        raise ValueError("upscale: x is on %s, the context runs on cuda:%d" % (x.device, sr.gpuid))
    if x.dtype == torch.uint8:
        if x.dim() != 3 or x.shape[2] not in (3, 4):
            raise ValueError("upscale: a uint8 tensor must be (H, W, 3) or (H, W, 4), not %s" % (tuple(x.shape),))
        if x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError("upscale: empty image %s" % (tuple(x.shape),))
        return RSR_FMT_U8_HWC, False
    if x.dtype in _HWC:
        if x.dim() != 3 or x.shape[2] not in (3, 4):
            raise ValueError("upscale: a 16-bit tensor must be (H, W, 3) or (H, W, 4), not %s" % (tuple(x.shape),))
        if x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError("upscale: empty image %s" % (tuple(x.shape),))
        return RSR_FMT_U16_HWC, False
    if x.dtype not in _FMT:
        raise ValueError("upscale: dtype %s is not supported (float16, float32 or uint8)" % x.dtype)
    if x.dim() not in (3, 4) or x.shape[-3] != 3:
        raise ValueError("upscale: a float tensor must be (3, H, W) or (N, 3, H, W), not %s" % (tuple(x.shape),))
    if x.shape[-1] < 1 or x.shape[-2] < 1:
        raise ValueError("upscale: empty image %s" % (tuple(x.shape),))
    return _FMT[x.dtype], x.dim() == 4


def describe(x):
    """The rsr_image descriptor of ONE image tensor -- float (3, H, W) or uint8 (H, W, c) -- as (data_ptr, row_pitch, plane_pitch) in bytes
    (plane_pitch 0 for uint8), or None when the view does not fit one and must be copied.  Pure: looks at shape and strides only.
      float:  stride(-1) == 1, stride(-2) >= W, stride(-3) > 0 (a crop, a slice along N, rows of a padded surface, planes stored apart)
      uint8:  stride(2) == 1, stride(1) == c, stride(0) >= W * c
      uint16 / int16 (H, W, c): the uint8 rule in elements -- element stride 1, pixel stride c, rows >= W * c elements apart -- and an even
              data pointer
    A dimension of size 1 has no stride to speak of.  Permuted views, stride 0 (expand) and steps along a row give None."""
    if x.dim() != 3:
        return None
    es = x.element_size()
    if x.dtype in _HWC:
        h, w, c = x.shape
        rs, ps, cs = x.stride()
        if (c > 1 and cs != 1) or (w > 1 and ps != c):
            return None
        row, plane = (rs if h > 1 else w * c), 0
        if row < w * c:
            return None
    else:
        _, h, w = x.shape
        plane, rs, cs = x.stride()
        if (w > 1 and cs != 1) or plane <= 0:
            return None
        row = rs if h > 1 else w
        if row < w:
            return None
    ptr = x.data_ptr()
    if ptr % es:
        return None
    return ptr, row * es, plane * es


def _packed(x, d):
    """Is the descriptor d of the image tensor x the tightly packed one?"""
    if x.dtype in _HWC:
        return d[1] == x.shape[1] * x.shape[2] * x.element_size()
    return d[1] == x.shape[2] * x.element_size() and d[2] == x.shape[1] * d[1]


def _out_size(sr, w, h):
    """(ow, oh) of the context's output for a w x h image: sr.out_size where the context has it (out_scale 4 / 2 / 1, a ratio such as
    3/2, or a ratio per axis, sr.out_ratio_xy, such as (8/3, 9/4): ValueError where w, h or the tile size does not take it), else w and h times its out_scale, else times its scale."""
    if hasattr(sr, "out_size"):
        return sr.out_size(w, h)
    s = getattr(sr, "out_scale", sr.scale)
    return w * s, h * s


def upscale(sr, x, out=None, out_dtype=None):
    """x4 -- or, with sr.out_scale 2 / 1, that result box-reduced on the device to x2 / x1, or with sr.out_ratio 3/2, 4/3, 3 ... area-averaged to that scale, or with sr.out_ratio_xy = (8/3, 9/4) ... to a scale per axis (720 x 480 -> 1920 x 1080) -- of x on the context `sr` (a loaded RealSR).  x lives on the context's GPU: float16 / float32 (3, H, W) or (N, 3, H, W)
    with values in [0, 1], or uint8 (H, W, 3 | 4).  Returns a tensor of the same dtype and layout at 4x (out_scale x), enqueued on
    torch.cuda.current_stream(); a batch is ONE rsr_process_device_batch call on that stream.  A view that fits a descriptor (describe)
    is read in place; any other non-contiguous input is made contiguous first.
    out: the tensor to write (and return) instead of a new one: the result's shape, dtype and device, and itself a view that fits a
    descriptor -- a window of a larger canvas, say.  ValueError otherwise, before anything is launched.  It must not overlap x.
    16-bit RGB(A): x may be a uint16 / int16 (H, W, 3 | 4) tensor (RSR_FMT_U16_HWC: full-range words, read unsigned whatever the dtype says);
    the result has the same dtype.  out_dtype (integer HWC inputs only): torch.uint8, torch.uint16 or torch.int16 -- the depth of the
    result, so that 8 -> 16 and 16 -> 8 bits are one call; with out= given, out.dtype must equal it.
    RGBA: the alpha of an (H, W, 4) input is the bicubic x4, or with sr.alpha_net = 1 the network's result for the gray image of the alpha
    (option "alpha_net": a second pass over the tiles, about twice the frame time); nothing here knows the option, the engine does.
    With sr.alpha_adaptive = 1 on top, tiles of constant alpha skip that pass; the engine then WAITS on the host once per tile batch, until
    the current stream has reached its scan of the alpha: the call is no longer purely asynchronous and must not run under stream capture.
    Dither: with sr.dither = 1 the colour samples of an integer result (uint8, uint16 / int16) are rounded against a threshold keyed to their
    place in the result (option "dither": gradients leave as fine static noise, not as bands; an out= window carries the pattern from its own
    origin); alpha and float results are not touched.  Nothing here knows the option, the engine does."""
    fmt, batched = _check(sr, x)
    ydtype = x.dtype
    if out_dtype is not None:
        if fmt not in _HWC_FMTS or out_dtype not in _HWC:
            raise ValueError("upscale: out_dtype is torch.uint8, torch.uint16 or torch.int16, for a uint8 / uint16 / int16 (H, W, 3 | 4) input only")
        ydtype = out_dtype
    out_fmt = _HWC[ydtype] if fmt in _HWC_FMTS else fmt
    # (the context's output size: x4 unless option "out_scale" says 2 or 1, or out_ratio another scale)
    if fmt in _HWC_FMTS:
        ow, oh = _out_size(sr, x.shape[1], x.shape[0])
        shape = (oh, ow, x.shape[2])
    else:
        ow, oh = _out_size(sr, x.shape[-1], x.shape[-2])
        shape = tuple(x.shape[:-3]) + (3, oh, ow)
    if out is not None:
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != ydtype or out.device != x.device:
            raise ValueError("upscale: out must be a %s tensor of shape %s on %s" % (ydtype, shape, x.device))
        if (batched and out.shape[0] > 1 and out.stride(0) == 0) or (out.numel() and describe(out[0] if batched else out) is None):
            raise ValueError("upscale: out (strides %s) is not addressable by row and plane pitch" % (tuple(out.stride()),))
    if x.numel() and describe(x[0] if batched else x) is None:
        x = x.contiguous()
    cur = torch.cuda.current_stream(x.device)
    if cur.cuda_stream == 0:
        # torch's default stream is the null stream, and a null stream means "the context's own stream, synchronously" to the C call.
        # The work goes onto a side stream ordered behind and in front of the default stream by events: still nothing waits on the host.
        side = _side_stream(x.device)
        side.wait_stream(cur)
        y = _enqueue(sr, x, fmt, batched, side.cuda_stream, out, shape, out_fmt, ydtype)
        cur.wait_stream(side)  # (x and y are next touched by work behind this wait: the allocator may reuse them safely)
        return y
    return _enqueue(sr, x, fmt, batched, cur.cuda_stream, out, shape, out_fmt, ydtype)


def _on_current_stream(device, enqueue):
    """enqueue(stream handle) on torch's current stream, with nothing waiting on the host (see upscale)."""
    cur = torch.cuda.current_stream(device)
    if cur.cuda_stream != 0:
        return enqueue(cur.cuda_stream)
    side = _side_stream(device)
    side.wait_stream(cur)
    y = enqueue(side.cuda_stream)
    cur.wait_stream(side)
    return y


# ---- YUV images, keyword chroma: what each subsampling is to this module -------------------------------------------------------------------
def _chroma(fmt8, fmt16, names, unit=0, yrows=1, tensor="", surface="", family=""):
    """One row of _CHROMA.  fmt: dtype -> format (16-bit words as int16 too: torch's uint16 is a late and partial dtype); names: the dtype
    refusal's list.  A surface (420, 422) is `unit` rows per `yrows` rows of Y -- (3h / 2, w) or (2h, w), uv (h / yrows, w), h a multiple of
    yrows --; unit 0: three full planes (3, h, w).  tensor, surface, family: the texts that differ."""
    fmt = {torch.uint8: fmt8, torch.int16: fmt16}
    if hasattr(torch, "uint16"):
        fmt[torch.uint16] = fmt16
    return types.SimpleNamespace(fmt=fmt, names=names, unit=unit, yrows=yrows, tensor=tensor, surface=surface, family=family)


_CHROMA = {
    # what a hardware decoder yields and an encoder takes; P010: the 10-bit code in the high bits
    420: _chroma(RSR_FMT_NV12, RSR_FMT_P010, "uint8 = NV12; uint16 / int16 = P010", 3, 2,
                 "a (3h / 2, w) tensor: h rows of Y, then h / 2 rows of interleaved UV", "a 4:2:0 surface (even h and w, uv (h / 2, w))"),
    # what broadcast and archive codecs hold: a UV row per Y row
    422: _chroma(RSR_FMT_NV16, RSR_FMT_P210, "uint8 = NV16; uint16 / int16 = P210", 2, 1,
                 "a (2h, w) tensor: h rows of Y, then h rows of interleaved UV (a YUV 4:2:2 surface)", "a YUV 4:2:2 surface (even w, uv (h, w))",
                 "YUV 4:2:2 surfaces"),
    # planar: three full planes (3, H, W); 16-bit words hold the 10-bit code in their LOW bits (yuv444p10le)
    444: _chroma(RSR_FMT_YUV444P, RSR_FMT_YUV444P10, "uint8 = yuv444p; uint16 / int16 = yuv444p10le", family="YUV 4:4:4 images"),
}
_CHROMA_OF = {f: c for c, k in _CHROMA.items() for f in k.fmt.values()}  # format -> chroma (an RGB format: in no row)


def _check_chroma(chroma, who):
    if chroma not in (420, 422, 444):
        raise ValueError("%s: chroma must be 420, 422 or 444 (YUV 4:2:0 / 4:2:2 surfaces, planar 4:4:4), not %r" % (who, chroma))


def _planes444(sr, s, what):
    """The three (H, W) plane views Y, U, V of a planar 4:4:4 image -- a (3, H, W) tensor, or a (y, u, v) triple of 2-D views -- validated;
    ValueError before anything is launched."""
    if isinstance(s, (tuple, list)):
        if len(s) != 3 or not all(isinstance(t, torch.Tensor) and t.dim() == 2 for t in s):
            raise ValueError("upscale_yuv: %s must be a (3, H, W) tensor or a (y, u, v) triple of (H, W) tensors (planar YUV 4:4:4)" % what)
        planes = list(s)
    else:
        if not isinstance(s, torch.Tensor) or s.dim() != 3 or s.shape[0] != 3:
            raise ValueError("upscale_yuv: %s must be a (3, H, W) tensor: the planes Y, U, V (planar YUV 4:4:4)" % what)
        planes = [s[0], s[1], s[2]]
    y = planes[0]
    if any(t.dtype != y.dtype or t.device != y.device or t.shape != y.shape for t in planes):
        raise ValueError("upscale_yuv: the planes of %s must have one shape and dtype, on one device" % what)
    if y.dtype not in _CHROMA[444].fmt:
        raise ValueError("upscale_yuv: dtype %s is not supported (%s)" % (y.dtype, _CHROMA[444].names))
    if y.device.type != "cuda" or y.device.index != sr.gpuid:
        raise ValueError("upscale_yuv: %s is on %s, the context runs on cuda:%d" % (what, y.device, sr.gpuid))
    if y.shape[0] < 1 or y.shape[1] < 1:
        raise ValueError("upscale_yuv: empty image %s" % (tuple(y.shape),))
    return planes


def _describe444(planes):
    """(data_ptr, row_pitch, plane_pitch) in bytes of the image behind three plane views, or None when no rsr_image describes it: a step
    along W, planes with different row strides, or planes that are not equally spaced upwards in memory."""
    y = planes[0]
    es, (h, w) = y.element_size(), y.shape
    if any((w > 1 and t.stride(1) != 1) or t.data_ptr() % es for t in planes):
        return None
    row = y.stride(0) if h > 1 else w
    if row < w or (h > 1 and any(t.stride(0) != row for t in planes)):
        return None
    plane = planes[1].data_ptr() - y.data_ptr()
    if plane <= 0 or planes[2].data_ptr() - planes[1].data_ptr() != plane:
        return None
    return y.data_ptr(), row * es, plane


def _desc444(sr, s, what):
    """(fmt, w, h, descriptor) of a planar 4:4:4 image; ValueError where it is none or no rsr_image describes it -- a 4:4:4 view is taken
    in place or not at all."""
    planes = _planes444(sr, s, what)
    d = _describe444(planes)
    if d is None:
        raise ValueError("upscale_yuv: %s is not addressable by one row pitch and one plane pitch (stride 1 along W, one row stride for all "
                         "three planes, the planes equally spaced)" % what)
    return _CHROMA[444].fmt[planes[0].dtype], planes[0].shape[1], planes[0].shape[0], d


def _new_yuv(like, ow, oh, chroma):
    """An uninitialised ow x oh YUV result of the kind of `like`: a surface tensor of the chroma's rows or a (3, oh, ow) tensor -- or, for
    a pair or triple, the plane views of one."""
    seq = isinstance(like, (tuple, list))
    first, k = like[0] if seq else like, _CHROMA[chroma]
    if not k.unit:
        o = first.new_empty((3, oh, ow))
        return (o[0], o[1], o[2]) if seq else o
    o = first.new_empty((oh * k.unit // k.yrows, ow))
    return (o[:oh], o[oh:]) if seq else o


def _upscale_yuv444(sr, surface, out):
    fmt, w, h, din = _desc444(sr, surface, "surface")
    ow, oh = _out_size_for(sr, fmt, w, h, "upscale_yuv")
    first = surface[0] if isinstance(surface, (tuple, list)) else surface
    if out is not None:
        if isinstance(out, (tuple, list)) != isinstance(surface, (tuple, list)):
            raise ValueError("upscale_yuv: out must be a %s like the input" % ("(y, u, v) triple" if isinstance(surface, (tuple, list)) else "(3, H, W) tensor"))
        ofmt, w2, h2, dout = _desc444(sr, out, "out")
        if (ofmt, w2, h2) != (fmt, ow, oh):
            raise ValueError("upscale_yuv: out must be a %s YUV 4:4:4 image of %d x %d on %s" % (first.dtype, ow, oh, first.device))
    else:
        out = _new_yuv(surface, ow, oh, 444)
        dout = _desc444(sr, out, "out")[3]
    _on_current_stream(first.device, lambda st: sr.process_device_batch([din], fmt, w, h, 3, [dout], fmt, stream=st))
    return out


def _planes(sr, s, what, chroma=420):
    """The (y, uv) views of a surface -- a (3h / 2, w) tensor (chroma=422: (2h, w)) or a pair of planes, uv (h / 2, w) ((h, w)) --
    validated; ValueError before anything is launched."""
    k = _CHROMA[chroma]
    if isinstance(s, (tuple, list)):
        if len(s) != 2 or not all(isinstance(t, torch.Tensor) for t in s):
            raise ValueError("upscale_yuv: %s must be a surface tensor or a (y, uv) pair of tensors" % what)
        y, uv = s
    else:
        if not isinstance(s, torch.Tensor) or s.dim() != 2 or s.shape[0] % k.unit or s.shape[0] < k.unit:
            raise ValueError("upscale_yuv: %s must be %s" % (what, k.tensor))
        h = s.shape[0] // k.unit * k.yrows
        y, uv = s[:h], s[h:]
    if y.dim() != 2 or uv.dim() != 2 or y.dtype != uv.dtype or y.device != uv.device:
        raise ValueError("upscale_yuv: y and uv of %s must be 2-D tensors of one dtype on one device" % what)
    if y.dtype not in k.fmt:
        raise ValueError("upscale_yuv: dtype %s is not supported (%s)" % (y.dtype, k.names))
    if y.device.type != "cuda" or y.device.index != sr.gpuid:
        raise ValueError("upscale_yuv: %s is on %s, the context runs on cuda:%d" % (what, y.device, sr.gpuid))
    h, w = y.shape
    if h < k.yrows or w < 2 or h % k.yrows or w % 2 or tuple(uv.shape) != (h // k.yrows, w):
        raise ValueError("upscale_yuv: y %s with uv %s is not %s" % (tuple(y.shape), tuple(uv.shape), k.surface))
    return y, uv


def _describe_yuv(y, uv):
    """(data_ptr, row_pitch, plane_pitch) in bytes of the surface behind the two views, or None when no rsr_image describes it: rows that
    are not contiguous, two different row pitches, or a UV plane that does not lie above Y(0,0) in memory."""
    es = y.element_size()
    if y.stride(1) != 1 or uv.stride(1) != 1 or y.stride(0) < y.shape[1] or y.data_ptr() % es or uv.data_ptr() % es:
        return None
    if uv.shape[0] > 1 and uv.stride(0) != y.stride(0):
        return None
    plane = uv.data_ptr() - y.data_ptr()
    return (y.data_ptr(), y.stride(0) * es, plane) if plane > 0 else None


def _ratio_text(sr):
    """The context's output ratio for an error text: its out_ratio, or, while that raises because the axes differ (out_ratio_xy), the pair
    as "rx x ry"; "in force" for a context that has neither."""
    try:
        return str(getattr(sr, "out_ratio", "in force"))
    except ValueError:
        pair = getattr(sr, "out_ratio_xy", None)
        return "%s x %s" % tuple(pair) if pair else "in force"


def _out_size_for(sr, fmt, w, h, who):
    """(ow, oh) of the context's output for a w x h image in fmt; ValueError where w, h or the tile size does not take it.  RGB: _out_size.
    A 4:2:0 surface: w and h times the context's out_scale 4 / 2 / 1, or, while another ratio is in force (sr.out_ratio, or a pair
    sr.out_ratio_xy: out_scale reads 0), sr.out_size_yuv -- ValueError for a context that has none.  4:2:2 and 4:4:4: sr.out_size_fmt at
    every out_scale, ratio or pair -- ValueError with "YUV" in it where the engine would refuse the call (4:2:2: an odd tile rectangle or
    image width; 4:4:4 has the rule of the RGB outputs, no parity anywhere), and for a context that has no out_size_fmt."""
    chroma = _CHROMA_OF.get(fmt)
    if chroma is None:
        return _out_size(sr, w, h)
    if chroma == 420:
        s = getattr(sr, "out_scale", sr.scale)
        if s:
            return w * s, h * s
        if not hasattr(sr, "out_size_yuv"):
            raise ValueError("%s: a YUV output takes out_scale 4, 2 or 1 only, not the output ratio %s" % (who, _ratio_text(sr)))
        return sr.out_size_yuv(w, h)
    if not hasattr(sr, "out_size_fmt"):
        raise ValueError("%s: this context writes no %s (no out_size_fmt)" % (who, _CHROMA[chroma].family))
    return sr.out_size_fmt(fmt, w, h)


def _yuv_ratio_note(sr):
    """What a size refusal adds while a YUV surface is written at a ratio other than 4 / 2 / 1 (else nothing)."""
    if getattr(sr, "out_scale", sr.scale):
        return ""
    return " (a YUV surface at the output ratio %s)" % (_ratio_text(sr),)


def upscale_yuv(sr, surface, out=None, chroma=420):
    """upscale() for a YUV 4:2:0 surface on the context's GPU: the YUV <-> RGB conversion and the chroma resampling happen inside the
    engine's pre- and post-processing kernels (RSR_FMT_NV12 / RSR_FMT_P010, include/realsr_hip.h; options "yuv_matrix", "yuv_range"), so no
    RGB frame is materialised.  Where the chroma samples sit is the context's option "yuv_siting" (sr.yuv_siting: 0 centre, 1 left -- what
    an H.264 / HEVC / AV1 decoder yields by default --, 2 top-left -- BT.2020 / UHD); it holds for the surface read and the one written.  surface: a (3H / 2, W) tensor as a decoder yields it -- uint8 (NV12), or uint16 / int16 (P010: the 10-bit
    code in the high bits) -- or a (y, uv) pair of views, y (H, W) and uv (H / 2, W).  A pair that no descriptor fits (a uv view that
    lies below y in memory, say) is packed into one allocation first.  Returns the same layout at sr.out_scale -- or at sr.out_ratio (3/2, 4/3,
    9/4, 3 ...) where sr.out_size_yuv admits the size --: a (3H' / 2, W') tensor,
    or for a pair the (y, uv) views of one.  out: the surface (or pair) to write and return instead.  Runs on torch.cuda.current_stream(),
    with no host synchronisation inside.
    chroma=422: a YUV 4:2:2 surface (RSR_FMT_NV16 / RSR_FMT_P210: chroma halved horizontally only, what DVCPRO-HD, ProRes 422, XDCAM HD422
    hold) -- a (2H, W) tensor, H rows of Y and H rows of interleaved UV, or a (y, uv) pair with uv (H, W); uint8 is NV16, uint16 / int16
    P210.  Any H >= 1 is taken.  The result has the same layout, sized by sr.out_size_fmt: ValueError with "YUV" in it where the engine would
    refuse (w or tilesize times the x ratio odd).
    chroma=444: planar YUV 4:4:4 (RSR_FMT_YUV444P / RSR_FMT_YUV444P10: what screen recordings, ProRes 4444 and software video frameworks
    hold) -- a (3, H, W) tensor of the planes Y, U, V, uint8 or uint16 / int16 with the 10-bit code in the LOW bits (yuv444p10le), or a
    (y, u, v) triple of (H, W) views.  Any H and W >= 1, odd ones included: no parity rule exists.  The view needs stride 1 along W, one row
    stride for all planes and equally spaced planes -- a crop, a window of a canvas -- and is then taken without a copy; ValueError
    otherwise.  The result is (3, H', W') of the same dtype (or a triple), sized by sr.out_size_fmt; out= takes a window.
    sr.dither = 1 (option "dither") holds here as in upscale: every Y, U and V code is rounded against the threshold of its own place in its
    own plane, the (U, V) pair of a chroma sample against one; at 10 bits sr.set_option("precise", 1) is its companion."""
    _check_chroma(chroma, "upscale_yuv")
    if chroma == 444:
        return _upscale_yuv444(sr, surface, out)
    pair = isinstance(surface, (tuple, list))
    y, uv = _planes(sr, surface, "surface", chroma)
    fmt, (h, w) = _CHROMA[chroma].fmt[y.dtype], y.shape
    ow, oh = _out_size_for(sr, fmt, w, h, "upscale_yuv")  # (out_scale 4 / 2 / 1, or a ratio such as 3/2: sr.out_ratio)
    if out is not None:
        if isinstance(out, (tuple, list)) != pair:
            raise ValueError("upscale_yuv: out must be a %s like the input" % ("(y, uv) pair" if pair else "surface tensor"))
        oy, ouv = _planes(sr, out, "out", chroma)
        if tuple(oy.shape) != (oh, ow) or oy.dtype != y.dtype or oy.device != y.device:
            raise ValueError("upscale_yuv: out must be a %s YUV surface of %d x %d on %s" % (y.dtype, ow, oh, y.device))
        dout = _describe_yuv(oy, ouv)
        if dout is None:
            raise ValueError("upscale_yuv: out is not addressable by one row pitch and a plane pitch")
    else:
        out = _new_yuv(surface, ow, oh, chroma)
        dout = _describe_yuv(*(out if pair else (out[:oh], out[oh:])))
    din = _describe_yuv(y, uv)
    if din is None:
        packed = torch.cat([y, uv], dim=0)  # (kept alive by the stream ordering below, like any temporary of a torch op)
        din = _describe_yuv(packed[:h], packed[h:])
    _on_current_stream(y.device, lambda st: sr.process_device_batch([din], fmt, w, h, 3, [dout], fmt, stream=st))
    return out


# ---- three-plane frames (yuv420p / yuv422p / yuv444p, 8 and 10 bits) to the surfaces upscale_yuv takes, and back ------------------------
def _plane_views(sr, planes, chroma, who, what):
    """(fmt, w, h, (y, u, v)) of a three-plane frame: 2-D tensors of one dtype on the context's GPU, u and v of the chroma's size;
    ValueError before anything is launched."""
    if len(planes) != 3 or not all(isinstance(t, torch.Tensor) and t.dim() == 2 for t in planes):
        raise ValueError("%s: %s must be three 2-D tensors, the planes Y, U and V" % (who, what))
    y, u, v = planes
    k = _CHROMA[chroma]
    if any(t.dtype != y.dtype or t.device != y.device for t in (u, v)):
        raise ValueError("%s: the planes of %s must have one dtype, on one device" % (who, what))
    if y.dtype not in k.fmt:
        raise ValueError("%s: dtype %s is not supported (uint8; uint16 / int16 with the 10-bit code in the LOW bits)" % (who, y.dtype))
    if y.device.type != "cuda" or y.device.index != sr.gpuid:
        raise ValueError("%s: %s is on %s, the context runs on cuda:%d" % (who, what, y.device, sr.gpuid))
    h, w = y.shape
    sx, sy = (1, 1) if chroma == 420 else (1, 0) if chroma == 422 else (0, 0)
    if h < 1 or w < 1 or w & sx or h & sy or tuple(u.shape) != (h >> sy, w >> sx) or u.shape != v.shape:
        raise ValueError("%s: y %s with u %s and v %s is no YUV 4:%s:%s frame" % (who, tuple(y.shape), tuple(u.shape), tuple(v.shape), str(chroma)[1], str(chroma)[2]))
    return k.fmt[y.dtype], w, h, (y, u, v)


def _rows_fit(t):
    """Is the 2-D view t addressable by a pointer and a row pitch (stride 1 along W, rows upwards in memory, aligned to its element)?"""
    return (t.shape[1] == 1 or t.stride(1) == 1) and (t.shape[0] == 1 or t.stride(0) >= t.shape[1]) and t.data_ptr() % t.element_size() == 0


def _planes_desc(y, u, v):
    """The rsr_planes entry (y, u, v, y_pitch, c_pitch), in bytes, of three views, or None when none describes them: rows that are not
    contiguous, or U and V rows that are not equally far apart."""
    if not all(_rows_fit(t) for t in (y, u, v)) or (u.shape[0] > 1 and u.stride(0) != v.stride(0)):
        return None
    es = y.element_size()
    return (y.data_ptr(), u.data_ptr(), v.data_ptr(), (y.stride(0) if y.shape[0] > 1 else y.shape[1]) * es,
            (u.stride(0) if u.shape[0] > 1 else u.shape[1]) * es)


def _surface_desc(sr, s, chroma, who, what, fmt, w, h):
    """The rsr_image descriptor of the w x h surface s of format fmt -- what upscale_yuv takes: a (3h / 2, w) / (2h, w) tensor or (y, uv)
    pair, or (3, h, w) / a (y, u, v) triple at 4:4:4 --; ValueError where it is none, of another size or dtype, or fits no descriptor."""
    try:
        if chroma == 444:
            sfmt, sw, sh, d = _desc444(sr, s, what)
        else:
            sy, suv = _planes(sr, s, what, chroma)
            sfmt, (sh, sw), d = _CHROMA[chroma].fmt[sy.dtype], sy.shape, _describe_yuv(sy, suv)
    except ValueError as e:
        raise ValueError(str(e).replace("upscale_yuv", who, 1)) from None
    if d is None:
        raise ValueError("%s: %s is not addressable by one row pitch and a plane pitch" % (who, what))
    if fmt is not None and (sfmt, sw, sh) != (fmt, w, h):
        raise ValueError("%s: %s must be a surface of %d x %d in the planes' dtype" % (who, what, w, h))
    return sfmt, sw, sh, d


def pack_planes(sr, y, u, v, chroma=420, out=None):
    """The three planes of a frame as a software decoder holds it -- yuv420p / yuv422p / yuv444p: uint8; their 10-bit little-endian forms:
    uint16 / int16 with the code in the LOW bits -- as the surface upscale_yuv takes: a (3h / 2, w) tensor (chroma=420: NV12 / P010),
    (2h, w) (422: NV16 / P210) or (3, h, w) (444).  One launch of rsr_pack_planes on torch.cuda.current_stream(): the chroma planes are
    interleaved on the device, and every 10-bit word of a 4:2:0 / 4:2:2 frame becomes (word & 1023) << 6 -- P010 / P210 hold the code
    high --; 4:4:4 words are copied as they are.  y (h, w); u and v (h / 2, w / 2), (h, w / 2) or (h, w).  Views with contiguous rows are
    read in place (a crop, a padded frame: u and v with one row stride); others are made contiguous first.  out: the surface (or, as
    upscale_yuv takes them, the pair or triple of views) to write and return instead of a new tensor.  ValueError before anything is
    launched."""
    _check_chroma(chroma, "pack_planes")
    fmt, w, h, (y, u, v) = _plane_views(sr, (y, u, v), chroma, "pack_planes", "the frame")
    if out is not None:
        dout = _surface_desc(sr, out, chroma, "pack_planes", "out", fmt, w, h)[3]
    else:
        out = _new_yuv(y, w, h, chroma)
        dout = _surface_desc(sr, out, chroma, "pack_planes", "out", fmt, w, h)[3]
    src = _planes_desc(y, u, v)
    if src is None:
        y, u, v = y.contiguous(), u.contiguous(), v.contiguous()  # (kept alive by the stream ordering, like any temporary of a torch op)
        src = _planes_desc(y, u, v)
    _on_current_stream(y.device, lambda st: sr.pack_planes([src], [dout], fmt, w, h, stream=st))
    return out


def unpack_planes(sr, surface, chroma=420, out=None):
    """The way back: the surface upscale_yuv returns -- a (3h / 2, w) / (2h, w) tensor or (y, uv) pair, (3, h, w) or a triple at
    chroma=444 -- as the three planes (y, u, v) of a yuv420p / yuv422p / yuv444p frame, 10-bit words with the code in the LOW bits
    (every P010 / P210 word >> 6).  One launch of rsr_unpack_planes on torch.cuda.current_stream().  out: the (y, u, v) tensors to write
    and return: the frame's shapes and dtype, rows contiguous, u and v with one row stride (ValueError otherwise: a result is written in
    place or not at all).  The surface is read in place and must fit a descriptor, as an out of upscale_yuv must."""
    _check_chroma(chroma, "unpack_planes")
    fmt, w, h, din = _surface_desc(sr, surface, chroma, "unpack_planes", "surface", None, 0, 0)
    first = surface[0] if isinstance(surface, (tuple, list)) else surface
    sx, sy = (1, 1) if chroma == 420 else (1, 0) if chroma == 422 else (0, 0)
    if out is None:
        out = (first.new_empty((h, w)), first.new_empty((h >> sy, w >> sx)), first.new_empty((h >> sy, w >> sx)))
    elif not isinstance(out, (tuple, list)):
        raise ValueError("unpack_planes: out must be the three tensors (y, u, v)")
    ofmt, ow, oh, planes = _plane_views(sr, tuple(out), chroma, "unpack_planes", "out")
    dst = _planes_desc(*planes)
    if (ofmt, ow, oh) != (fmt, w, h) or planes[0].device != first.device:
        raise ValueError("unpack_planes: out must be the planes of a %d x %d frame in the surface's dtype, on %s" % (w, h, first.device))
    if dst is None:
        raise ValueError("unpack_planes: out is not addressable by plane pointers, one luma and one chroma row pitch")
    _on_current_stream(first.device, lambda st: sr.unpack_planes([din], [dst], fmt, w, h, stream=st))
    return tuple(out)


# ---- video: run only the tiles that changed -----------------------------------------------------------------------------------------------
def _pinned_u8(n):
    """n bytes of pinned host memory as a uint8 tensor (the mask's landing place: a copy into it can be asynchronous)."""
    return torch.empty(n, dtype=torch.uint8, pin_memory=True)


def _image_desc(sr, t, what, chroma=420):
    """(fmt, w, h, c, descriptor or None) of ONE image as upscale (a single uint8 / float image) or upscale_yuv (a surface or a (y, uv)
    pair; chroma: its subsampling) takes it; ValueError before anything is launched.  chroma=444: every image is a planar 4:4:4 one."""
    if chroma == 444:
        fmt, w, h, d = _desc444(sr, t, what)
        return fmt, w, h, 3, d
    if isinstance(t, (tuple, list)) or (isinstance(t, torch.Tensor) and t.dim() == 2):
        y, uv = _planes(sr, t, what, chroma)
        return _CHROMA[chroma].fmt[y.dtype], y.shape[1], y.shape[0], 3, _describe_yuv(y, uv)
    fmt, batched = _check(sr, t)
    if batched:
        raise ValueError("upscale_delta: %s must be ONE image, not a batch %s" % (what, tuple(t.shape)))
    h, w, c = t.shape if fmt in _HWC_FMTS else (t.shape[1], t.shape[2], 3)
    return fmt, w, h, c, describe(t)


def _desc_or_packed(sr, t, what, chroma=420):
    """(descriptor, keep) of the image t: its own where one fits (_image_desc), else that of a packed copy `keep` (kept alive by the
    stream ordering, like any temporary of a torch op)."""
    d = _image_desc(sr, t, what, chroma)[4]
    if d is not None:
        return d, None
    if isinstance(t, torch.Tensor) and t.dim() == 3:
        keep = t.contiguous()
        return describe(keep), keep
    y, uv = _planes(sr, t, what, chroma)
    keep = torch.cat([y, uv], dim=0)
    return _describe_yuv(keep[:y.shape[0]], keep[y.shape[0]:]), keep


def _same_layout(a, b):
    """Do two images (tensors or (y, uv) pairs) agree in kind, shape, dtype and device?"""
    if isinstance(a, (tuple, list)) != isinstance(b, (tuple, list)):
        return False
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same_layout(p, q) for p, q in zip(a, b))
    return isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype and a.device == b.device


def upscale_delta(sr, x, prev_x, prev_y, out=None, chroma=420):
    """upscale() / upscale_yuv() of the video frame x, given the previous frame prev_x and its result prev_y: only the tiles whose SOURCE
    RECTANGLE differs between prev_x and x walk the network (rsr_diff_tiles + rsr_process_device_masked, include/realsr_hip.h); every
    other tile's output rectangle is a function of bytes that did not change, so what prev_y holds there is the answer, bit for bit.
    x and prev_x: one layout and dtype -- anything upscale takes for a SINGLE image (uint8 (H, W, 3 | 4), float (3, H, W)) or a surface
    as upscale_yuv takes it ((3H / 2, W) tensor or (y, uv) pair); views go through the same descriptors (describe).  prev_y: the result
    for prev_x, in the layout upscale / upscale_yuv returns, computed at the context's CURRENT options.
    out: None = prev_y is updated in place and returned; another tensor (or pair) of prev_y's layout first receives prev_y through copy_.
    Returns (out, tiles_run).  prev_x=None: every tile runs (the first frame, a scene cut) and prev_y only provides the memory.
    Steps, all on torch.cuda.current_stream(): the diff; a copy of the mask into pinned memory; ONE stream synchronisation -- the grid of
    every launch depends on the mask, so the host has to see it: this is the only host wait, and it is what the skipped tiles are paid
    with --; the masked call.
    chroma=422: surfaces and pairs are YUV 4:2:2 as upscale_yuv(..., chroma=422) takes them.  chroma=444: x, prev_x, prev_y and out are
    planar 4:4:4 images as upscale_yuv(..., chroma=444) takes them.
    sr.alpha_net = 1 holds here as in upscale: the marked tiles of an RGBA frame run both passes, and the diff compares the alpha bytes too.
    sr.alpha_adaptive = 1 likewise, with its host wait per tile batch (upscale)."""
    _check_chroma(chroma, "upscale_delta")
    fmt, w, h, c, _ = _image_desc(sr, x, "x", chroma)
    if prev_x is not None and not _same_layout(x, prev_x):
        raise ValueError("upscale_delta: prev_x must have x's layout, shape, dtype and device")
    ow, oh = _out_size_for(sr, fmt, w, h, "upscale_delta")
    note = _yuv_ratio_note(sr) if _CHROMA_OF.get(fmt) in (420, 422) else ""
    for t, what in ((prev_y, "prev_y"),) + (((out, "out"),) if out is not None else ()):
        if isinstance(t, (tuple, list)) != isinstance(x, (tuple, list)):
            raise ValueError("upscale_delta: %s must be a %s like x" % (what, "(y, uv) pair" if isinstance(x, (tuple, list)) else "tensor"))
        f2, w2, h2, c2, d2 = _image_desc(sr, t, what, chroma)
        if (f2, w2, h2, c2) != (fmt, ow, oh, c):
            raise ValueError("upscale_delta: %s must hold the %d x %d result for x (%d x %d) in x's format%s" % (what, ow, oh, w, h, note))
        if d2 is None:
            raise ValueError("upscale_delta: %s is not addressable by row and plane pitch" % what)
    if out is None:
        out = prev_y
    else:
        for dst, src in (zip(out, prev_y) if isinstance(out, (tuple, list)) else ((out, prev_y),)):
            dst.copy_(src)
    dout = _image_desc(sr, out, "out", chroma)[4]
    first = x[0] if isinstance(x, (tuple, list)) else x
    # A view no descriptor fits is packed first -- BOTH frames here, in front of the wait below: the packing runs on torch's current
    # stream, and the side stream (where the diff reads the copies) is ordered behind that stream only up to the wait.
    dx, keep_x = _desc_or_packed(sr, x, "x", chroma)
    dp, keep_p = _desc_or_packed(sr, prev_x, "prev_x", chroma) if prev_x is not None else (None, None)
    nx, ny = sr.tile_count(w, h)
    cur = torch.cuda.current_stream(first.device)
    st = cur if cur.cuda_stream != 0 else _side_stream(first.device)  # (the null stream means "synchronously" to the C calls: see upscale)
    if st is not cur:
        st.wait_stream(cur)
    if prev_x is None:
        mask = np.ones(nx * ny, dtype=np.uint8)
    else:
        d_mask = first.new_empty(nx * ny, dtype=torch.uint8)
        host = _pinned_u8(nx * ny)
        with (torch.cuda.stream(st) if st is not cur else contextlib.nullcontext()):  # (the copy below goes where torch's current stream is)
            sr.diff_tiles(dp, dx, fmt, w, h, c, d_mask.data_ptr(), stream=st.cuda_stream)
            host.copy_(d_mask, non_blocking=True)
        st.synchronize()  # the ONE host wait
        mask = host.numpy()
    sr.process_device_masked(dx, fmt, w, h, c, dout, fmt, mask, stream=st.cuda_stream)
    if st is not cur:
        cur.wait_stream(st)
    return out, int(np.count_nonzero(mask))


# ---- video: a window of frames shares one diff, one round trip and one walk through the network ------------------------------------------
SEQ_MAX = 16  # frames per rsr_process_device_sequence call (RSR_SEQ_MAX)


def _new_like_result(x, ow, oh, chroma=420):
    """An uninitialised result for the single image x (a tensor or a (y, uv) pair; chroma: a surface's subsampling) at ow x oh, of x's kind."""
    if chroma == 444 or isinstance(x, (tuple, list)) or x.dim() == 2:
        return _new_yuv(x, ow, oh, chroma)
    return x.new_empty((oh, ow, x.shape[2]) if x.dtype in _HWC else (3, oh, ow))


def upscale_sequence(sr, frames, prev_x=None, prev_y=None, out=None, chroma=420):
    """upscale() / upscale_yuv() of N consecutive video frames: returns (ys, tiles_run), ys[k] bit for bit what upscale(frames[k]) returns.
    Only the tiles whose source rectangle differs from the frame before walk the network, and the changed tiles of up to 16 frames share
    their launches (rsr_diff_tiles_sequence + rsr_process_device_sequence, include/realsr_hip.h); every other rectangle of ys[k] is copied
    from the frame that computed it last.
    frames: a stacked tensor -- (N, 3, H, W) float or (N, H, W, 3 | 4) uint8 -- or a list of single images of ONE layout, each anything
    upscale_delta takes for x (YUV surfaces and (y, uv) pairs come as a list only: a stacked 3-D uint8 tensor would be ambiguous).
    prev_x, prev_y: the frame in front of frames[0] and its result at the context's current options; without them every tile of
    frames[0] runs.  out: None = the results are allocated (torch.empty: every byte is written); else a stacked tensor or a list like
    the result, each image addressable by row and plane pitch.  The result has the kind the input had.
    Windows of at most 16 frames; window g + 1 takes the last frame and output of window g as its prev.  Per window, all on
    torch.cuda.current_stream() (the side stream for the null stream, as in upscale_delta): the diff of all pairs, ONE asynchronous copy
    of the masks into pinned memory, ONE stream synchronisation, the sequence call.
    chroma=422: surfaces and pairs are YUV 4:2:2 as upscale_yuv(..., chroma=422) takes them.  chroma=444: every frame is a planar 4:4:4
    image as upscale_yuv(..., chroma=444) takes it -- a list of them, or a stacked (N, 3, H, W) uint8 / int16 tensor.
    sr.alpha_net = 1 holds here as in upscale, for the tiles of RGBA frames that run; sr.alpha_adaptive = 1 likewise, with its host wait per
    tile batch."""
    _check_chroma(chroma, "upscale_sequence")
    stacked = isinstance(frames, torch.Tensor)
    if stacked:
        if frames.dim() != 4 or frames.shape[0] < 1:
            raise ValueError("upscale_sequence: a stacked tensor must be (N, 3, H, W) float or (N, H, W, 3 | 4) uint8, not %s" % (tuple(frames.shape),))
        xs = [frames[i] for i in range(frames.shape[0])]
    else:
        xs = list(frames) if isinstance(frames, (tuple, list)) else []
        if not xs:
            raise ValueError("upscale_sequence: frames must be a stacked tensor or a non-empty list of images")
    n = len(xs)
    fmt, w, h, c, _ = _image_desc(sr, xs[0], "frames[0]", chroma)
    for i, x in enumerate(xs[1:], 1):
        if not _same_layout(xs[0], x):
            raise ValueError("upscale_sequence: mixed layouts: frames[%d] differs from frames[0] in kind, shape, dtype or device" % i)
    if prev_x is not None and prev_y is None:
        raise ValueError("upscale_sequence: a prev_x needs its result prev_y")
    if prev_x is not None and not _same_layout(xs[0], prev_x):
        raise ValueError("upscale_sequence: prev_x must have the frames' layout, shape, dtype and device")
    if prev_x is None:
        prev_y = None  # (nothing of it would be used: every tile of frames[0] runs)
    pair = isinstance(xs[0], (tuple, list))
    ow, oh = _out_size_for(sr, fmt, w, h, "upscale_sequence")
    note = _yuv_ratio_note(sr) if _CHROMA_OF.get(fmt) == 420 else ""

    def result_desc(t, what):
        if isinstance(t, (tuple, list)) != pair:
            raise ValueError("upscale_sequence: %s must be a %s like the frames" % (what, "(y, uv) pair" if pair else "tensor"))
        f2, w2, h2, c2, d2 = _image_desc(sr, t, what, chroma)
        if (f2, w2, h2, c2) != (fmt, ow, oh, c):
            raise ValueError("upscale_sequence: %s must hold the %d x %d result of a %d x %d frame in the frames' format%s" % (what, ow, oh, w, h, note))
        if d2 is None:
            raise ValueError("upscale_sequence: %s is not addressable by row and plane pitch" % what)
        return d2

    dprev_y = result_desc(prev_y, "prev_y") if prev_y is not None else None
    first = xs[0][0] if pair else xs[0]
    if out is None:
        if stacked:
            out = first.new_empty((n, oh, ow, c) if fmt in _HWC_FMTS else (n, 3, oh, ow))
            ys = [out[i] for i in range(n)]
        else:
            out = ys = [_new_like_result(x, ow, oh, chroma) for x in xs]
    else:
        if stacked != isinstance(out, torch.Tensor) or (stacked and out.dim() != 4) or len(out) != n:
            raise ValueError("upscale_sequence: out must be a %s of %d results like the frames" % ("stacked tensor" if stacked else "list", n))
        ys = [out[i] for i in range(n)]
    douts = [result_desc(y, "out[%d]" % i) for i, y in enumerate(ys)]
    # Views no descriptor fits are packed first -- all of them here, in front of the wait below (see upscale_delta).
    packed = [_desc_or_packed(sr, x, "frames[%d]" % i, chroma) for i, x in enumerate(xs)]
    dxs = [p[0] for p in packed]
    dprev_x, keep_p = _desc_or_packed(sr, prev_x, "prev_x", chroma) if prev_x is not None else (None, None)
    nx, ny = sr.tile_count(w, h)
    nt = nx * ny
    cur = torch.cuda.current_stream(first.device)
    st = cur if cur.cuda_stream != 0 else _side_stream(first.device)  # (the null stream means "synchronously" to the C calls: see upscale)
    if st is not cur:
        st.wait_stream(cur)
    tiles_run = 0
    for g in range(0, n, SEQ_MAX):
        k = min(SEQ_MAX, n - g)
        px, py = (dprev_x, dprev_y) if g == 0 else (dxs[g - 1], douts[g - 1])
        d_masks = first.new_empty(k * nt, dtype=torch.uint8)
        host = _pinned_u8(k * nt)
        with (torch.cuda.stream(st) if st is not cur else contextlib.nullcontext()):  # (the copy below goes where torch's current stream is)
            sr.diff_tiles_sequence(dxs[g:g + k], px, fmt, w, h, c, d_masks.data_ptr(), stream=st.cuda_stream)
            host.copy_(d_masks, non_blocking=True)
        st.synchronize()  # the ONE host wait of the window
        masks = host.numpy()
        sr.process_device_sequence(dxs[g:g + k], fmt, w, h, c, douts[g:g + k], fmt, masks, prev_out=py, stream=st.cuda_stream)
        tiles_run += int(np.count_nonzero(masks))
    if st is not cur:
        cur.wait_stream(st)
    return out, tiles_run


_side = {}


def _side_stream(device):
    if device.index not in _side:
        _side[device.index] = torch.cuda.Stream(device)
    return _side[device.index]


def _enqueue(sr, x, fmt, batched, stream, out, shape, out_fmt=None, ydtype=None):
    out_fmt = fmt if out_fmt is None else out_fmt
    y = out if out is not None else torch.empty(shape, dtype=ydtype or x.dtype, device=x.device)
    if x.numel() == 0:
        return y
    if fmt in _HWC_FMTS:
        h, w, c = x.shape
    else:
        h, w, c = x.shape[-2], x.shape[-1], 3
    dx, dy = describe(x[0] if batched else x), describe(y[0] if batched else y)
    if batched:  # the batch stride only moves the per-image pointer
        n, es = x.shape[0], x.element_size()
        ins = [(dx[0] + i * x.stride(0) * es, dx[1], dx[2]) for i in range(n)]
        outs = [(dy[0] + i * y.stride(0) * es, dy[1], dy[2]) for i in range(n)]
        sr.process_device_batch(ins, fmt, w, h, c, outs, out_fmt, stream=stream)
    elif _packed(x, dx) and _packed(y, dy):
        sr.process_device_fmt(dx[0], fmt, w, h, c, dy[0], out_fmt, stream=stream)
    else:
        sr.process_device_batch([dx], fmt, w, h, c, [dy], out_fmt, stream=stream)
    return y
