"""The numpy reference of the engine option "out_scale" (include/realsr_hip.h), shared by tests/test_out_scale.py and
tests/test_gpu_out_scale.py: steps 1 and 2 of the definition, in float32 and in the stated order of summation."""
import numpy as np

F32 = np.float32


def box_reduce(v, k):
    """v: float32 (..., H, W), H and W multiples of k in {1, 2, 4}.  Returns the float32 (..., H / k, W / k) array of
         c = min(max(v, 0), 1);  k = 2: ((c00 + c01) + (c10 + c11)) * 0.25f  (c[y][x]);
         k = 4: s_j = ((c_j0 + c_j1) + (c_j2 + c_j3)),  ((s0 + s1) + (s2 + s3)) * 0.0625f
    Every operand and every intermediate is a float32."""
    v = np.asarray(v)
    assert v.dtype == np.float32 and k in (1, 2, 4) and v.shape[-2] % k == 0 and v.shape[-1] % k == 0
    c = np.minimum(np.maximum(v, F32(0)), F32(1))
    if k == 1:
        return c
    h, w = c.shape[-2:]
    b = c.reshape(c.shape[:-2] + (h // k, k, w // k, k))

    def at(y, x):
        return b[..., :, y, :, x]

    if k == 2:
        d = ((at(0, 0) + at(0, 1)) + (at(1, 0) + at(1, 1))) * F32(0.25)
    else:
        s = [(at(j, 0) + at(j, 1)) + (at(j, 2) + at(j, 3)) for j in range(4)]
        d = ((s[0] + s[1]) + (s[2] + s[3])) * F32(0.0625)
    assert d.dtype == np.float32
    return d


def u8_expected(d):
    """The byte of step 3 for the float32 box mean d, evaluated exactly: (floor(E) clipped to 0..255, near) with E = float64(d) * 255 + 0.5;
    `near` marks the elements where E lies within 2^-14 of an integer -- there the engine's float32 (possibly fused) d * 255 + 0.5 may
    land on the other side (the rule of tests/test_gpu_tensor_io.py)."""
    E = d.astype(np.float64) * 255.0 + 0.5
    near = np.abs(E - np.rint(E)) < 2.0 ** -14
    return np.clip(np.floor(E), 0, 255).astype(np.uint8), near
