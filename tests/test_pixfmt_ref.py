"""The tests' one pixel format table against the library's host-only format functions: for every format, the packed numpy image of
tests/pixfmt_ref.py has the bytes rsr_image_bytes states, and as a pitched image it occupies exactly that many bytes, all of them inside
rsr_image_span.  No GPU is touched."""
import numpy as np
import pytest

import realsr_ncnn_vulkan_amd as R

import pixfmt_ref as F

NO_PARITY_RULE = (F.U8, F.F16, F.F32, F.YUV444P, F.YUV444P10)
CASES = [(fmt, w, h, c) for fmt in F.FORMATS for w, h in [(2, 2), (36, 26), (70, 50)] + ([(35, 25)] if fmt in NO_PARITY_RULE else [])
         for c in ((3, 4) if fmt == F.U8 else (3,))]
IDS = ["fmt%d-%dx%dx%d" % case for case in CASES]


def test_the_table_names_the_library_s_formats():
    assert {getattr(R, name) for name in dir(R) if name.startswith("RSR_FMT_")} == set(F.FORMATS)
    assert (R.RSR_FMT_U8_HWC, R.RSR_FMT_F16_CHW, R.RSR_FMT_F32_CHW, R.RSR_FMT_NV12, R.RSR_FMT_P010) == (F.U8, F.F16, F.F32, F.NV12, F.P010)
    assert (R.RSR_FMT_NV16, R.RSR_FMT_P210, R.RSR_FMT_YUV444P, R.RSR_FMT_YUV444P10) == (F.NV16, F.P210, F.YUV444P, F.YUV444P10)


@pytest.mark.parametrize("fmt,w,h,c", CASES, ids=IDS)
def test_a_packed_image_has_the_library_s_bytes(fmt, w, h, c):
    x = np.zeros(F.shape_of(fmt, w, h, c), F.NP[fmt])
    assert x.nbytes == R.image_bytes(fmt, w, h, c)
    assert F.dims_of(fmt, x) == (w, h) and sum(F.plane_rows(fmt, h)) * w * F.ES[fmt] * (c if fmt == F.U8 else 1) == x.nbytes
    assert F.image(1, fmt, w, h, c).shape == x.shape and F.image(1, fmt, w, h, c).dtype == x.dtype


@pytest.mark.parametrize("fmt,w,h,c", CASES, ids=IDS)
def test_a_pitched_image_lies_inside_the_library_s_span(fmt, w, h, c):
    img = F.image(7 + fmt, fmt, w, h, c)
    es = F.ES[fmt]
    rowbytes = w * es * (c if fmt == F.U8 else 1)
    off, pitch = 3 * es, rowbytes + 5 * es
    plane = 0 if fmt == F.U8 else (h + 2) * pitch + 6 * es
    span = R.image_span(fmt, w, h, c, pitch, plane)
    canvas = np.full(off + span + 16, 0x5A, dtype=np.uint8)
    inside = F.place(canvas, off, pitch, plane, img, fmt)
    assert F.same_bits(F.lift(canvas, off, pitch, plane, fmt, w, h, c), img)
    assert inside.sum() == img.nbytes == R.image_bytes(fmt, w, h, c)
    assert not inside[:off].any() and inside[off] and inside[off + span - 1] and not inside[off + span:].any()
    assert (canvas[~inside] == 0x5A).all()
