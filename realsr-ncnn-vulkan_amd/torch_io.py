"""torch tensors in, torch tensors out: the supported way to call the engine from a PyTorch pipeline.

    from realsr_ncnn_vulkan_amd import RealSR, torch_io
    sr = RealSR(0); sr.load(param, bin)
    y = torch_io.upscale(sr, x)        # x: (3, H, W) or (N, 3, H, W) float16 / float32 in [0, 1] on cuda:0  ->  (.., 3, 4H, 4W)

The float tensors go through rsr_process_device_fmt as they are (planar fp16 / fp32, include/realsr_hip.h): no quantisation to
uint8 on either side, no permute, no extra pass over the frame.  The work is enqueued on torch.cuda.current_stream() and nothing
here waits for the GPU: the result is ordered on that stream like the output of any torch op.
"""
import torch

from . import RSR_FMT_F16_CHW, RSR_FMT_F32_CHW, RSR_FMT_U8_HWC

_FMT = {torch.float16: RSR_FMT_F16_CHW, torch.float32: RSR_FMT_F32_CHW}


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
    if x.dtype not in _FMT:
        raise ValueError("upscale: dtype %s is not supported (float16, float32 or uint8)" % x.dtype)
    if x.dim() not in (3, 4) or x.shape[-3] != 3:
        raise ValueError("upscale: a float tensor must be (3, H, W) or (N, 3, H, W), not %s" % (tuple(x.shape),))
    if x.shape[-1] < 1 or x.shape[-2] < 1:
        raise ValueError("upscale: empty image %s" % (tuple(x.shape),))
    return _FMT[x.dtype], x.dim() == 4


def upscale(sr, x):
    """x4 of x on the context `sr` (a loaded RealSR).  x lives on the context's GPU: float16 / float32 (3, H, W) or (N, 3, H, W)
    with values in [0, 1], or uint8 (H, W, 3 | 4).  Returns a new tensor of the same dtype and layout at 4x, enqueued on
    torch.cuda.current_stream(); a batch is N calls on that stream.  Non-contiguous input is made contiguous first."""
    fmt, batched = _check(sr, x)
    x = x.contiguous()
    cur = torch.cuda.current_stream(x.device)
    if cur.cuda_stream == 0:
        # torch's default stream is the null stream, and a null stream means "the context's own stream, synchronously" to the C call.
        # The work goes onto a side stream ordered behind and in front of the default stream by events: still nothing waits on the host.
        side = _side_stream(x.device)
        side.wait_stream(cur)
        y = _enqueue(sr, x, fmt, batched, side.cuda_stream)
        cur.wait_stream(side)  # (x and y are next touched by work behind this wait: the allocator may reuse them safely)
        return y
    return _enqueue(sr, x, fmt, batched, cur.cuda_stream)


_side = {}


def _side_stream(device):
    if device.index not in _side:
        _side[device.index] = torch.cuda.Stream(device)
    return _side[device.index]


def _enqueue(sr, x, fmt, batched, stream):
    s = sr.scale
    if fmt == RSR_FMT_U8_HWC:
        h, w, c = x.shape
        y = torch.empty((h * s, w * s, c), dtype=x.dtype, device=x.device)
        sr.process_device_fmt(x.data_ptr(), fmt, w, h, c, y.data_ptr(), fmt, stream=stream)
        return y
    h, w = x.shape[-2], x.shape[-1]
    y = torch.empty(tuple(x.shape[:-2]) + (h * s, w * s), dtype=x.dtype, device=x.device)
    for xi, yi in zip(x, y) if batched else ((x, y),):
        sr.process_device_fmt(xi.data_ptr(), fmt, w, h, 3, yi.data_ptr(), fmt, stream=stream)
    return y
