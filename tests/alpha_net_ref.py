"""Option "alpha_net" restated in numpy (include/realsr_hip.h "alpha through the network"): from the three planes A0, A1, A2 that
RSR_FMT_F32_CHW holds for the gray image of the alpha to the alpha samples of a U8 / U16 destination.  float32 operations, one at a time:
numpy rounds every one of them by itself, which is the rule.  numpy only."""
import numpy as np

F32 = np.float32
THIRD = F32(1.0 / 3.0)   # computed in double, rounded once


def gray(img):
    """G: the c == 3 image of img's sample type whose three samples are img's alpha sample (img: (H, W, 4) uint8 / uint16)."""
    img = np.asarray(img)
    assert img.ndim == 3 and img.shape[2] == 4 and img.dtype in (np.uint8, np.uint16)
    return np.ascontiguousarray(np.repeat(img[:, :, 3:4], 3, axis=2))


def mean3(a0, a1, a2):
    """Step 1: m = min(((A0 + A1) + A2) * fp32(1/3), 1)."""
    a0, a1, a2 = (np.asarray(a, F32) for a in (a0, a1, a2))
    s = (a0 + a1).astype(F32)
    s = (s + a2).astype(F32)
    m = (s * THIRD).astype(F32)
    return np.minimum(m, F32(1))


def store(m, bits):
    """Steps 2 / 3: floor(m * max + 0.5), the product and the sum each rounded by itself, clamped to 0 .. max; max = 255 (bits 8) or
    65535 (bits 16)."""
    assert bits in (8, 16)
    top = F32(255 if bits == 8 else 65535)
    p = (np.asarray(m, F32) * top).astype(F32)
    q = np.floor((p + F32(0.5)).astype(F32))
    return np.minimum(np.maximum(q, F32(0)), top).astype(np.uint8 if bits == 8 else np.uint16)


def alpha(planes, bits):
    """The alpha samples (H, W) of a `bits`-deep destination from planes = float32 [3][H][W], what RSR_FMT_F32_CHW holds for G."""
    planes = np.asarray(planes)
    assert planes.dtype == F32 and planes.ndim == 3 and planes.shape[0] == 3
    return store(mean3(planes[0], planes[1], planes[2]), bits)
