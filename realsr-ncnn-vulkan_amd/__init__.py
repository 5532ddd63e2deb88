"""realsr-ncnn-vulkan_amd -- MI355X-native RealSR x4 tiled inference.

The product is the C-ABI shared library `lib/librealsr_hip.so` (include/realsr_hip.h), built from
`csrc/` with hipcc for gfx950.  This module is only a thin ctypes binding used by the tests, the
bench and `__graft_entry__`; the reference-shaped C++ host class lives in csrc/realsr.h.

There is no CPU fallback: importing works anywhere (the library links against libamdhip64 only), but
creating a `RealSR` without a gfx950 device raises.  The directory name carries a hyphen (it is the
reference's name + `_amd`); import it through the repo-root shim `realsr_ncnn_vulkan_amd.py`.
"""
import ctypes as C
import fractions
import os
import subprocess
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RSR_LIB: load an alternative build of the same library (kernel experiments: tools/build_variant.sh)
LIB_PATH = os.environ.get("RSR_LIB") or os.path.join(_HERE, "lib", "librealsr_hip.so")
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

EXPORTS = [
    "rsr_create", "rsr_destroy", "rsr_load", "rsr_set_params", "rsr_process", "rsr_process_device",
    "rsr_model_pack", "rsr_load_packed", "rsr_model_info", "rsr_preproc", "rsr_preproc_tta", "rsr_postproc",
    "rsr_postproc_tta", "rsr_net_forward", "rsr_conv3x3", "rsr_set_profiling", "rsr_get_profile", "rsr_get_conv_times", "rsr_get_trace",
    "rsr_set_option", "rsr_last_error", "rsr_version", "rsr_host_alloc", "rsr_host_free",
    "rsr_set_progress_callback", "rsr_conv3x3_res", "rsr_create_group", "rsr_group_transport", "rsr_process_rows",
    "rsr_process_group", "rsr_device_memory", "rsr_process_tiles", "rsr_tile_partition", "rsr_rccl_probe", "rsr_get_stat",
    "rsr_net_forward_f32", "rsr_conv3x3_res_precise", "rsr_process_many",
    "rsr_selfcheck", "rsr_selfcheck_tile", "rsr_selfcheck_ranges",
    "rsr_process_device_fmt", "rsr_image_bytes",
    "rsr_process_device_batch", "rsr_image_span",
    "rsr_yuv_constants",
    "rsr_set_out_ratio", "rsr_out_size", "rsr_out_size_yuv",
    "rsr_set_out_ratio_xy", "rsr_out_size_xy", "rsr_out_size_yuv_xy",
    "rsr_tile_count", "rsr_tile_source_rect", "rsr_diff_tiles", "rsr_process_device_masked",
    "rsr_sequence_sources", "rsr_diff_tiles_sequence", "rsr_process_device_sequence",
    "rsr_out_size_fmt",
    "rsr_pack_planes", "rsr_unpack_planes",
    "rsr_video_open", "rsr_video_send", "rsr_video_ready", "rsr_video_receive", "rsr_video_flush", "rsr_video_reset", "rsr_video_info",
    "rsr_video_close",
    "rsr_process_fmt",
    "rsr_model_blend", "rsr_load_second", "rsr_load_second_packed", "rsr_set_blend", "rsr_model_export",
]

NUM_CONVS = 351  # convolutions of the default-depth model (23 RRDB blocks); a loaded model's own count is RealSR.num_convs
MAX_RRDB = 64    # RSR_MAX_RRDB: the deepest model rsr_load takes (15 * 64 + 6 = 966 convolutions)

RSR_OK, RSR_E_ARG, RSR_E_IO, RSR_E_FORMAT, RSR_E_GRAPH, RSR_E_DEVICE, RSR_E_STATE, RSR_E_NOMEM = 0, -1, -2, -3, -4, -5, -6, -7
# pixel formats of device-resident images (rsr_process_device_fmt): uint8 HWC, planar fp16 / fp32 [3][h][w] in [0, 1]
RSR_FMT_U8_HWC, RSR_FMT_F16_CHW, RSR_FMT_F32_CHW = 0, 1, 2
# YUV 4:2:0 surfaces: Y [h][w] then interleaved UV [h/2][w/2][2]; uint8, or uint16 with the 10-bit code in the high bits
RSR_FMT_NV12, RSR_FMT_P010 = 4, 5
# YUV 4:2:2 surfaces: Y [h][w] then interleaved UV [h][w/2][2] -- chroma halved horizontally only; uint8, or uint16 with the code in the high bits
RSR_FMT_NV16, RSR_FMT_P210 = 8, 9
# planar YUV 4:4:4: the planes Y, U, V [h][w] one plane pitch apart; uint8, or uint16 with the 10-bit code in the LOW bits (yuv444p10le)
RSR_FMT_YUV444P, RSR_FMT_YUV444P10 = 12, 13
# 16-bit RGB(A): uint16 [h][w][c], c in {3, 4}, native words, full range 0 .. 65535.  RSR_FMT_U16_HWC = 16 is an attribute of this module
# like the others (R.RSR_FMT_U16_HWC, `from realsr_ncnn_vulkan_amd import RSR_FMT_U16_HWC`), served by the module's __getattr__: the names
# dir() lists under RSR_FMT_* stay the formats of the tests' one packed-image table (tests/pixfmt_ref.py), which has no uint16 HWC layout --
# this format's table is tests/rgb16_ref.py.
_FMT_U16_HWC = 16
_LATE_FORMATS = {"RSR_FMT_U16_HWC": _FMT_U16_HWC}


def __getattr__(name):
    try:
        return _LATE_FORMATS[name]
    except KeyError:
        raise AttributeError("module %r has no attribute %r" % (__name__, name)) from None


RSR_SEQ_MAX = 16  # frames per rsr_process_device_sequence call


class Profile(C.Structure):
    _fields_ = [("conv_ms", C.c_double), ("conv_flops", C.c_double), ("conv_launches", C.c_longlong),
                ("pre_ms", C.c_double), ("post_ms", C.c_double), ("pre_bytes", C.c_double),
                ("post_bytes", C.c_double), ("total_ms", C.c_double), ("tiles", C.c_longlong),
                ("calls", C.c_longlong)]


class SelfcheckReport(C.Structure):
    _fields_ = [("tile_w", C.c_int), ("tile_h", C.c_int), ("storage_err", C.c_float), ("headroom", C.c_float),
                ("max_byte_diff", C.c_int), ("bytes_differ", C.c_longlong), ("peak_abs", C.c_float), ("peak_conv", C.c_int),
                ("nonfinite", C.c_longlong), ("fp16_overflow", C.c_int), ("recommend_precise", C.c_int),
                ("elapsed_ms", C.c_float)]


class Image(C.Structure):
    """rsr_image: a device image behind its own pointer, row pitch and plane pitch (bytes; 0 = tightly packed)."""
    _fields_ = [("data", C.c_void_p), ("row_pitch", C.c_longlong), ("plane_pitch", C.c_longlong)]


class Planes(C.Structure):
    """rsr_planes: the three planes of one YUV frame (yuv420p / yuv422p / yuv444p and their 10-bit forms) behind their own pointers;
    y_pitch and c_pitch in bytes, 0 = tightly packed."""
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("y_pitch", C.c_longlong), ("c_pitch", C.c_longlong)]


class RealSRError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("rsr error %d: %s" % (code, msg))
        self.code = code


def build(force=False, verbose=False):
    """Compile csrc/ into lib/librealsr_hip.so with hipcc --offload-arch=gfx950 (cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc")]
    if force:
        cmd.append("-B")
    if not verbose:
        cmd.append("-s")
    subprocess.check_call(cmd)
    return LIB_PATH


_lib = None


def lib():
    """Load the C-ABI library.  Fails loudly if it has not been built -- there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    # When PyTorch shares the process (tests, bench: device tensors + torch.distributed), its bundled HIP
    # runtime must be the one that is loaded first; loading /opt/rocm's copy first leaves torch without a GPU.
    if os.environ.get("RSR_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(or make -C realsr-ncnn-vulkan_amd/csrc)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, ip, cp = C.c_void_p, C.c_int, C.c_char_p
    L.rsr_create.argtypes = [C.POINTER(vp), ip, ip, ip]
    L.rsr_destroy.argtypes = [vp]
    L.rsr_destroy.restype = None
    L.rsr_load.argtypes = [vp, cp, cp]
    L.rsr_set_params.argtypes = [vp, ip, ip, ip]
    L.rsr_process.argtypes = [vp, vp, ip, ip, ip, vp]
    L.rsr_process_device.argtypes = [vp, vp, ip, ip, ip, vp, vp]
    L.rsr_process_device_fmt.argtypes = [vp, vp, ip, ip, ip, ip, vp, ip, vp]
    L.rsr_process_fmt.argtypes = [vp, vp, ip, ip, ip, ip, vp, ip]
    L.rsr_image_bytes.argtypes = [ip, ip, ip, ip]
    L.rsr_image_bytes.restype = C.c_longlong
    L.rsr_process_device_batch.argtypes = [vp, ip, C.POINTER(Image), ip, ip, ip, ip, C.POINTER(Image), ip, vp]
    L.rsr_image_span.argtypes = [ip, ip, ip, ip, C.c_longlong, C.c_longlong]
    L.rsr_image_span.restype = C.c_longlong
    L.rsr_yuv_constants.argtypes = [ip, ip, ip, C.POINTER(C.c_float), ip]
    L.rsr_set_out_ratio.argtypes = [vp, ip, ip]
    L.rsr_out_size.argtypes = [ip, ip, ip, ip, ip, C.POINTER(ip), C.POINTER(ip)]
    L.rsr_out_size_yuv.argtypes = [ip, ip, ip, ip, ip, C.POINTER(ip), C.POINTER(ip)]
    L.rsr_set_out_ratio_xy.argtypes = [vp, ip, ip, ip, ip]
    L.rsr_out_size_xy.argtypes = [ip, ip, ip, ip, ip, ip, ip, C.POINTER(ip), C.POINTER(ip)]
    L.rsr_out_size_yuv_xy.argtypes = [ip, ip, ip, ip, ip, ip, ip, C.POINTER(ip), C.POINTER(ip)]
    L.rsr_out_size_fmt.argtypes = [ip, ip, ip, ip, ip, ip, ip, ip, C.POINTER(ip), C.POINTER(ip)]
    L.rsr_tile_count.argtypes = [ip, ip, ip, C.POINTER(ip), C.POINTER(ip)]
    L.rsr_tile_source_rect.argtypes = [ip, ip, ip, ip, ip, C.POINTER(ip), C.POINTER(ip), C.POINTER(ip), C.POINTER(ip)]
    L.rsr_diff_tiles.argtypes = [vp, C.POINTER(Image), C.POINTER(Image), ip, ip, ip, ip, vp, vp]
    L.rsr_process_device_masked.argtypes = [vp, C.POINTER(Image), ip, ip, ip, ip, C.POINTER(Image), ip, vp, ip, vp]
    L.rsr_sequence_sources.argtypes = [ip, ip, vp, ip, C.POINTER(ip)]
    L.rsr_diff_tiles_sequence.argtypes = [vp, ip, C.POINTER(Image), C.POINTER(Image), ip, ip, ip, ip, vp, vp]
    L.rsr_process_device_sequence.argtypes = [vp, ip, C.POINTER(Image), ip, ip, ip, ip, C.POINTER(Image), ip, C.POINTER(Image), vp, ip, vp]
    L.rsr_pack_planes.argtypes = [vp, ip, C.POINTER(Planes), C.POINTER(Image), ip, ip, ip, vp]
    L.rsr_unpack_planes.argtypes = [vp, ip, C.POINTER(Image), C.POINTER(Planes), ip, ip, ip, vp]
    L.rsr_video_open.argtypes = [vp, ip, ip, ip, ip, C.POINTER(vp)]
    L.rsr_video_send.argtypes = [vp, C.POINTER(Planes)]
    L.rsr_video_ready.argtypes = [vp]
    L.rsr_video_receive.argtypes = [vp, C.POINTER(Planes)]
    L.rsr_video_flush.argtypes = [vp]
    L.rsr_video_reset.argtypes = [vp]
    L.rsr_video_info.argtypes = [vp, C.POINTER(ip), C.POINTER(ip), C.POINTER(ip)]
    L.rsr_video_close.argtypes = [vp]
    L.rsr_video_close.restype = None
    L.rsr_model_pack.argtypes = [cp, cp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rsr_device_memory.argtypes = [C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.rsr_host_alloc.argtypes = [C.c_size_t]
    L.rsr_host_alloc.restype = vp
    L.rsr_host_free.argtypes = [vp]
    L.rsr_host_free.restype = None
    L.rsr_set_progress_callback.argtypes = [vp, vp, vp]
    L.rsr_load_packed.argtypes = [vp, vp, C.c_size_t, ip]
    L.rsr_model_blend.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.c_float, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rsr_load_second.argtypes = [vp, cp, cp]
    L.rsr_load_second_packed.argtypes = [vp, vp, C.c_size_t, ip]
    L.rsr_set_blend.argtypes = [vp, C.c_float]
    L.rsr_model_export.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rsr_model_info.argtypes = [cp, cp, C.POINTER(ip), C.POINTER(ip), C.POINTER(C.c_longlong),
                                 C.POINTER(C.c_longlong), C.POINTER(ip)]
    L.rsr_preproc.argtypes = [vp, vp, ip, ip, ip, vp, ip, ip, ip, ip, ip, ip, vp, ip, ip]
    L.rsr_preproc_tta.argtypes = [vp, vp, ip, ip, ip, C.POINTER(vp), ip, ip, ip, ip, ip, ip]
    L.rsr_postproc.argtypes = [vp, vp, ip, ip, vp, ip, ip, vp, ip, ip, ip, ip, ip, ip, ip]
    L.rsr_postproc_tta.argtypes = [vp, C.POINTER(vp), ip, ip, vp, ip, ip, ip, ip, ip, ip, ip]
    L.rsr_net_forward.argtypes = [vp, vp, ip, ip, vp]
    L.rsr_conv3x3.argtypes = [vp, vp, ip, ip, ip, ip, vp, vp, ip, ip, vp]
    L.rsr_conv3x3_res.argtypes = [vp, vp, ip, ip, ip, vp, vp, ip, C.c_float, ip, vp, C.c_float, vp]
    L.rsr_process_many.argtypes = [vp, ip, C.POINTER(vp), C.POINTER(ip), C.POINTER(ip), C.POINTER(ip), C.POINTER(vp), C.POINTER(ip)]
    L.rsr_net_forward_f32.argtypes = [vp, vp, ip, ip, vp]
    L.rsr_conv3x3_res_precise.argtypes = [vp, vp, vp, ip, ip, ip, vp, vp, C.c_float, ip, vp, vp, C.c_float, vp, vp]
    L.rsr_selfcheck.argtypes = [vp, vp, ip, ip, C.POINTER(SelfcheckReport)]
    L.rsr_selfcheck_tile.argtypes = [vp, ip, ip]
    L.rsr_selfcheck_ranges.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_longlong), ip]
    L.rsr_create_group.argtypes = [C.POINTER(vp), C.POINTER(ip), ip, ip, cp, cp]
    L.rsr_group_transport.restype = cp
    L.rsr_process_rows.argtypes = [vp, vp, ip, ip, ip, vp, ip, ip]
    L.rsr_process_tiles.argtypes = [vp, vp, ip, ip, ip, vp, ip, ip]
    L.rsr_process_group.argtypes = [C.POINTER(vp), ip, vp, ip, ip, ip, vp]
    L.rsr_tile_partition.argtypes = [ip, ip, ip, ip, ip, C.POINTER(ip)]
    L.rsr_set_profiling.argtypes = [vp, ip]
    L.rsr_get_profile.argtypes = [vp, C.POINTER(Profile), ip]
    L.rsr_get_conv_times.argtypes = [vp, C.POINTER(C.c_double), ip, ip]
    L.rsr_get_trace.argtypes = [vp, C.POINTER(C.c_ulonglong), ip]
    L.rsr_set_option.argtypes = [vp, cp, C.c_longlong]
    L.rsr_get_stat.argtypes = [vp, cp, C.POINTER(C.c_double)]
    L.rsr_rccl_probe.argtypes = []
    L.rsr_last_error.argtypes = [vp]
    L.rsr_last_error.restype = cp
    L.rsr_version.restype = cp
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def model_info(param_path, bin_path):
    """Host-only parse + graph validation (no GPU).  Returns dict."""
    L = lib()
    nl, nc, enc = C.c_int(), C.c_int(), C.c_int()
    nw, nb = C.c_longlong(), C.c_longlong()
    rc = L.rsr_model_info(str(param_path).encode(), str(bin_path).encode(), nl, nc, nw, nb, enc)
    if rc != 0:
        raise RealSRError(rc, L.rsr_last_error(None).decode())
    return dict(n_layers=nl.value, n_convs=nc.value, n_weights=nw.value, n_biases=nb.value, bin_encoding=enc.value)


def model_pack(param_path, bin_path):
    """Host-only: parse, validate and pack the model into one relocatable blob (np.uint8 array; 33.5 MB at 23 blocks, 9.0 MB at 6): what rsr_load
    uploads and what the multi-GPU broadcast carries."""
    L = lib()
    need = C.c_size_t()
    rc = L.rsr_model_pack(str(param_path).encode(), str(bin_path).encode(), None, 0, need)
    if rc != 0:
        raise RealSRError(rc, L.rsr_last_error(None).decode())
    buf = np.zeros(need.value, dtype=np.uint8)
    rc = L.rsr_model_pack(str(param_path).encode(), str(bin_path).encode(), _p(buf), buf.size, need)
    if rc != 0:
        raise RealSRError(rc, L.rsr_last_error(None).decode())
    return buf


def model_blend(blob_a, blob_b, t):
    """Host-only network interpolation (rsr_model_blend): the blob (1 - t) * blob_a + t * blob_b of two packed models of one depth,
    t in [0, 1]; returns bytes.  The rule, rounding by rounding, is in include/realsr_hip.h; the result loads with load_packed."""
    L = lib()
    a = np.ascontiguousarray(np.frombuffer(blob_a, dtype=np.uint8) if isinstance(blob_a, (bytes, bytearray, memoryview)) else blob_a, dtype=np.uint8)
    b = np.ascontiguousarray(np.frombuffer(blob_b, dtype=np.uint8) if isinstance(blob_b, (bytes, bytearray, memoryview)) else blob_b, dtype=np.uint8)
    need = C.c_size_t()
    rc = L.rsr_model_blend(_p(a), a.size, _p(b), b.size, float(t), None, 0, need)
    if rc != 0:
        raise RealSRError(rc, L.rsr_last_error(None).decode())
    buf = np.empty(need.value, dtype=np.uint8)
    rc = L.rsr_model_blend(_p(a), a.size, _p(b), b.size, float(t), _p(buf), buf.size, need)
    if rc != 0:
        raise RealSRError(rc, L.rsr_last_error(None).decode())
    return buf.tobytes()


class PinnedArray:
    """A numpy uint8 view of rsr_host_alloc'ed (pinned) memory; free() or let it go out of scope."""

    def __init__(self, shape):
        self._L = lib()
        n = int(np.prod(shape))
        self._p = self._L.rsr_host_alloc(n)
        if not self._p:
            raise MemoryError("rsr_host_alloc(%d)" % n)
        self.array = np.ctypeslib.as_array((C.c_uint8 * n).from_address(self._p)).reshape(shape)

    def free(self):
        if self._p:
            self.array = None
            self._L.rsr_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class RealSR:
    """Python mirror of the reference's `class RealSR` (realsr.h:13-42) over the C-ABI.

    RealSR(gpuid, tta_mode=False, num_threads=1); load(parampath, modelpath); fields scale / tilesize /
    prepadding; process(in HWC uint8) -> out HWC uint8.
    """

    def __init__(self, gpuid, tta_mode=False, num_threads=1, _adopt=None):
        self._L = lib()
        if _adopt is not None:
            h = _adopt
        else:
            h = C.c_void_p()
            rc = self._L.rsr_create(C.byref(h), int(gpuid), int(bool(tta_mode)), int(num_threads))
            if rc != 0:
                raise RealSRError(rc, self._L.rsr_last_error(None).decode())
        self._h = h
        self.gpuid = int(gpuid)
        self.scale, self.tilesize, self.prepadding = 4, 200, 10
        self.tta_mode = bool(tta_mode)

    @property
    def out_scale(self):
        """Size of the output relative to the input: 4 (default) = the network's x4 image; 2 or 1 = that image box-reduced on the
        device, 2 x 2 or 4 x 4 (option "out_scale", include/realsr_hip.h).  Takes effect for the next call.  Read from the engine, so
        set_option("out_scale", s) and this property cannot disagree: every buffer below is sized with the value the engine will use."""
        return int(self.get_stat("out_scale"))

    @out_scale.setter
    def out_scale(self, s):
        self.set_option("out_scale", int(s))  # (anything but 1, 2 or 4 raises RealSRError(RSR_E_ARG) and leaves the value alone)

    @property
    def out_ratio(self):
        """Size of the output relative to the input as a fractions.Fraction: out_scale generalised to n / d with d in 1..4 and
        1 <= n / d <= 4 (3, 3/2, 4/3, 9/4 ...: rsr_set_out_ratio, include/realsr_hip.h), area-averaged on the device.  Set it with a
        Fraction, an (n, d) pair or an int; 4, 2 and 1 ARE out_scale 4 / 2 / 1.  Takes effect for the next call.  Read from the engine."""
        s = int(self.get_stat("out_scale"))
        if s:
            return fractions.Fraction(s)
        n, d = int(self.get_stat("out_num")), int(self.get_stat("out_den"))
        if d == 0:  # the axes differ (rsr_set_out_ratio_xy): no single ratio describes the output
            raise ValueError("the output ratio differs per axis (%s along x, %s along y): read out_ratio_xy" % self._ratio_pair())
        return fractions.Fraction(n, d)

    @staticmethod
    def _nd(r):
        if isinstance(r, (tuple, list)):
            return int(r[0]), int(r[1])  # (as given: the engine reduces it, and refuses a zero denominator)
        r = fractions.Fraction(r)
        return r.numerator, r.denominator

    @out_ratio.setter
    def out_ratio(self, r):
        n, d = self._nd(r)
        self._ck(self._L.rsr_set_out_ratio(self._h, n, d))  # (a ratio outside the set raises RealSRError(RSR_E_ARG) and leaves the value alone)

    @property
    def out_ratio_xy(self):
        """Size of the output relative to the input per axis, a pair of fractions.Fraction (x, y): DVD and HDV frames to square-pixel
        sizes -- 720 x 480 -> 1920 x 1080 is (8/3, 9/4), 720 x 576 -> 1920 x 1080 (8/3, 15/8), 1440 x 1080 -> 1920 x 1080 (4/3, 1)
        (rsr_set_out_ratio_xy, include/realsr_hip.h: each axis n / d with d in 1..8 and 1 <= n / d <= 4).  Set it with a pair whose
        members are a Fraction, an (n, d) pair or an int.  Equal members among the ratios of out_ratio ARE out_ratio; setting out_ratio
        or out_scale sets both axes again.  Takes effect for the next call.  Read from the engine."""
        r, pair = self._ratio_or_pair()
        return (r, r) if pair is None else pair

    def _ratio_pair(self):  # the pair while the axes differ (stats of their own: out_num / out_den read 0 then)
        return (fractions.Fraction(int(self.get_stat("out_num_x")), int(self.get_stat("out_den_x"))),
                fractions.Fraction(int(self.get_stat("out_num_y")), int(self.get_stat("out_den_y"))))

    @out_ratio_xy.setter
    def out_ratio_xy(self, r):
        if not isinstance(r, (tuple, list)) or len(r) != 2:
            raise ValueError("out_ratio_xy takes a pair (x ratio, y ratio)")
        (nx, dx), (ny, dy) = self._nd(r[0]), self._nd(r[1])
        self._ck(self._L.rsr_set_out_ratio_xy(self._h, nx, dx, ny, dy))  # (a pair outside the set raises RealSRError(RSR_E_ARG) and leaves the value alone)

    def _ratio_or_pair(self):
        """(r, None) while one ratio of rsr_set_out_ratio serves both axes -- the engine calls the methods below have always made --,
        else (None, (rx, ry)): the _xy stats and functions are consulted only then."""
        s = int(self.get_stat("out_scale"))
        if s:
            return fractions.Fraction(s), None
        n, d = int(self.get_stat("out_num")), int(self.get_stat("out_den"))
        if d == 0:
            return None, self._ratio_pair()
        r = fractions.Fraction(n, d)
        return (r, None) if r.denominator <= 4 else (None, (r, r))

    def _out_size_xy(self, fn, pair, w, h, what):
        rx, ry = pair
        ow, oh = C.c_int(0), C.c_int(0)
        if fn(rx.numerator, rx.denominator, ry.numerator, ry.denominator, int(self.tilesize), int(w), int(h), C.byref(ow), C.byref(oh)) != 0:
            raise ValueError("%s %s x %s: %d x %d at tile %d: %s" % (what, rx, ry, w, h, self.tilesize, self._L.rsr_last_error(None).decode()))
        return ow.value, oh.value

    def out_size(self, w, h):
        """(ow, oh) of the output the next call writes for a w x h image: (w * n / d, h * n / d) at the ratio and tile size in force --
        (w * nx / dx, h * ny / dy) while out_ratio_xy holds a pair.  ValueError where the engine would refuse the call: w, h or tilesize
        times n is no multiple of d, each axis with its own n / d (rsr_out_size, rsr_out_size_xy)."""
        r, pair = self._ratio_or_pair()
        if pair is not None:
            return self._out_size_xy(self._L.rsr_out_size_xy, pair, w, h, "output ratios")
        if r.denominator == 1:
            return w * r.numerator, h * r.numerator
        ow, oh = C.c_int(0), C.c_int(0)
        if self._L.rsr_out_size(r.numerator, r.denominator, int(self.tilesize), int(w), int(h), C.byref(ow), C.byref(oh)) != 0:
            raise ValueError("output ratio %s: %d x %d at tile %d: w, h and tilesize times %d must be multiples of %d"
                             % (r, w, h, self.tilesize, r.numerator, r.denominator))
        return ow.value, oh.value

    def out_size_yuv(self, w, h):
        """out_size for a YUV 4:2:0 OUTPUT (RSR_FMT_NV12 / RSR_FMT_P010): (w * n / d, h * n / d) at the ratio and tile size in force.
        ValueError where the engine would refuse the call: an odd w or h, w, h or tilesize times n no multiple of d, or one of
        w * n / d, h * n / d and tilesize * n / d odd -- a 2 x 2 chroma quad would cross a tile or the image's edge (rsr_out_size_yuv;
        per axis while out_ratio_xy holds a pair: rsr_out_size_yuv_xy)."""
        r, pair = self._ratio_or_pair()
        if pair is not None:
            return self._out_size_xy(self._L.rsr_out_size_yuv_xy, pair, w, h, "a YUV output at ratios")
        ow, oh = C.c_int(0), C.c_int(0)
        if self._L.rsr_out_size_yuv(r.numerator, r.denominator, int(self.tilesize), int(w), int(h), C.byref(ow), C.byref(oh)) != 0:
            raise ValueError("a YUV output at ratio %s: %d x %d at tile %d: w and h must be even, w, h and tilesize times %d multiples of %d, and "
                             "w, h and tilesize times %s even" % (r, w, h, self.tilesize, r.numerator, r.denominator, r))
        return ow.value, oh.value

    def out_size_fmt(self, fmt, w, h):
        """out_size for an output in pixel format `fmt` (RSR_FMT_*) at the ratio, or pair, and tile size in force: the rule of out_size for
        the RGB formats, of out_size_yuv for NV12 / P010, and for NV16 / P210 the 4:2:2 rule -- the ratio rule, and w * nx / dx and
        tilesize * nx / dx even; the rows carry no parity rule (rsr_out_size_fmt).  YUV444P / YUV444P10 and U16_HWC: the rule of out_size, no parity at
        all.  ValueError where the engine would refuse the call."""
        r, pair = self._ratio_or_pair()
        rx, ry = (r, r) if pair is None else pair
        ow, oh = C.c_int(0), C.c_int(0)
        if self._L.rsr_out_size_fmt(int(fmt), rx.numerator, rx.denominator, ry.numerator, ry.denominator, int(self.tilesize), int(w), int(h),
                                    C.byref(ow), C.byref(oh)) != 0:
            raise ValueError("format %d at %s x %s: %d x %d at tile %d: %s" % (fmt, rx, ry, w, h, self.tilesize, self._L.rsr_last_error(None).decode()))
        return ow.value, oh.value

    def _ratio_text(self):  # for error texts: one ratio, or "rx x ry"
        r, pair = self._ratio_or_pair()
        return str(r) if pair is None else "%s x %s" % pair

    @property
    def yuv_siting(self):
        """Where a chroma sample of an NV12 / P010 surface sits, on both sides of a call: 0 (default) = the centre of its 2 x 2 luma
        quad (JPEG, MPEG-1), 1 = left (H.264 / HEVC / AV1 / MPEG-2 default), 2 = top-left (BT.2020 / UHD HEVC) -- option "yuv_siting",
        include/realsr_hip.h.  Takes effect for the next call.  Read from the engine, like out_scale."""
        return int(self.get_stat("yuv_siting"))

    @yuv_siting.setter
    def yuv_siting(self, v):
        self.set_option("yuv_siting", int(v))  # (anything but 0, 1 or 2 raises RealSRError(RSR_E_ARG) and leaves the value alone)

    @property
    def alpha_net(self):
        """0 (default): the alpha of an RGBA image is the bicubic x4.  1: it walks the network as a gray image -- a second pass over the
        call's tiles, about twice the frame time -- and the mean of the three results becomes the alpha sample (option "alpha_net",
        include/realsr_hip.h has the exact rule; a constant alpha does not come out constant).  RGB calls are not concerned.  Takes effect
        for the next call.  Read from the engine, like yuv_siting; stat "alpha_tiles" counts the tiles that ran the alpha pass."""
        return int(self.get_stat("alpha_net"))

    @alpha_net.setter
    def alpha_net(self, v):
        self.set_option("alpha_net", int(v))  # (anything but 0 or 1 raises RealSRError(RSR_E_ARG) and leaves the value alone)

    @property
    def alpha_adaptive(self):
        """0 (default): under alpha_net 1 every tile of an RGBA call runs the alpha pass.  1: a tile whose source rectangle holds ONE alpha
        value skips it and keeps the bytes of alpha_net 0 -- that value, exactly -- while every other tile holds the bytes of alpha_net 1
        (option "alpha_adaptive", include/realsr_hip.h).  The library scans the alpha on the device and reads the result on the host: one
        host wait per tile batch, also in an asynchronous call, so no such call under stream capture.  Without alpha_net 1, and for RGB
        calls, the option does nothing.  Takes effect for the next call.  Stats "alpha_tiles" / "alpha_tiles_flat": tiles that ran /
        skipped the alpha pass."""
        return int(self.get_stat("alpha_adaptive"))

    @alpha_adaptive.setter
    def alpha_adaptive(self, v):
        self.set_option("alpha_adaptive", int(v))  # (anything but 0 or 1 raises RealSRError(RSR_E_ARG) and leaves the value alone)

    @property
    def dither(self):
        """0 (default): every integer sample is floor(d * M + 0.5) of the value d the library holds.  1: every COLOUR sample of every integer
        output format -- uint8 / uint16 RGB(A), the Y / U / V codes of NV12, P010, NV16, P210, YUV444P, YUV444P10 -- is rounded against a
        threshold keyed to its position in the output image instead (option "dither", include/realsr_hip.h has the rule): smooth gradients
        come out as fine static noise, not as bands.  A value that is exactly a code keeps it; alpha samples and the float formats are not
        touched; masked calls, sequences, tile ranges and batches give the bytes of the plain call.  A uint8 RGB call then leaves conv_last's
        fused store for one post-processing launch.  At 10 and 16 bits `precise` is its companion: fp16 has no steps to spare there.  Takes
        effect for the next call.  Read from the engine, like alpha_net."""
        return int(self.get_stat("dither"))

    @dither.setter
    def dither(self, v):
        if int(v) != v:  # (the C ABI takes an integer: a fraction must not be truncated into a valid value on its way there)
            raise RealSRError(RSR_E_ARG, "dither must be 0 (round to nearest) or 1 (ordered dither of integer outputs)")
        self.set_option("dither", int(v))  # (anything but 0 or 1 raises RealSRError(RSR_E_ARG) and leaves the value alone)

    def close(self):
        if getattr(self, "_h", None):
            for v in list(getattr(self, "_videos", ())):  # open video sessions go first: they hold device memory of this context
                v.close()
            self._L.rsr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise RealSRError(rc, self._L.rsr_last_error(self._h).decode())

    def load(self, parampath, modelpath):
        self._ck(self._L.rsr_load(self._h, str(parampath).encode(), str(modelpath).encode()))
        return 0

    def load_packed(self, blob, device_ptr=None):
        """blob: np.uint8 array (host), or pass device_ptr (int) + blob = nbytes."""
        if device_ptr is not None:
            self._ck(self._L.rsr_load_packed(self._h, C.c_void_p(int(device_ptr)), int(blob), 1))
        else:
            blob = np.ascontiguousarray(blob, dtype=np.uint8)
            self._ck(self._L.rsr_load_packed(self._h, _p(blob), blob.size, 0))

    def load_second(self, parampath, modelpath):
        """A second model of the same depth beside the loaded one (rsr_load_second); `blend` then moves the weights between the two."""
        self._ck(self._L.rsr_load_second(self._h, str(parampath).encode(), str(modelpath).encode()))

    def load_second_packed(self, blob, device_ptr=None):
        """load_second from a packed blob: np.uint8 array or bytes (host), or pass device_ptr (int) + blob = nbytes."""
        if device_ptr is not None:
            self._ck(self._L.rsr_load_second_packed(self._h, C.c_void_p(int(device_ptr)), int(blob), 1))
        else:
            blob = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else blob, dtype=np.uint8)
            self._ck(self._L.rsr_load_second_packed(self._h, _p(blob), blob.size, 0))

    @property
    def blend(self):
        """The strength t of the network interpolation, the weights being (1 - t) * first + t * second model (stat "blend"; 0 without a
        second model).  Setting it rewrites the context's active weights on the device (rsr_set_blend): not while calls are in flight."""
        return self.get_stat("blend")

    @blend.setter
    def blend(self, t):
        self._ck(self._L.rsr_set_blend(self._h, float(t)))

    def export_model(self):
        """The packed blob the kernels read, as bytes (rsr_model_export): model_pack's for a plain load, model_blend's behind `blend`."""
        need = C.c_size_t()
        self._ck(self._L.rsr_model_export(self._h, None, 0, need))
        buf = np.empty(need.value, dtype=np.uint8)
        self._ck(self._L.rsr_model_export(self._h, _p(buf), buf.size, need))
        return buf.tobytes()

    @property
    def num_blocks(self):
        """RRDB blocks of the loaded model (stat "model_blocks"): 23 for the reference's x4.param, 1 .. MAX_RRDB accepted; 0 before a load."""
        return int(self.get_stat("model_blocks"))

    @property
    def num_convs(self):
        """Convolutions of the loaded model, 15 * num_blocks + 6 (stat "model_convs"); 0 before a load."""
        return int(self.get_stat("model_convs"))

    def _push_params(self):
        self._ck(self._L.rsr_set_params(self._h, int(self.scale), int(self.tilesize), int(self.prepadding)))

    def set_option(self, key, value):
        self._ck(self._L.rsr_set_option(self._h, key.encode(), int(value)))

    def get_stat(self, key):
        """rsr_get_stat: read-only engine state ("plan_batches", "workspace_mb", "lane_out_mb", "last_test_us", ...)."""
        v = C.c_double(0)
        self._ck(self._L.rsr_get_stat(self._h, key.encode(), C.byref(v)))
        return v.value

    def process(self, img, out=None, push_params=True):
        """out: optional preallocated (oh, ow, c) uint8 array, (ow, oh) = out_size(w, h) (e.g. PinnedArray(...).array)."""
        img = np.ascontiguousarray(img, dtype=np.uint8) if not (isinstance(img, np.ndarray) and img.flags.c_contiguous and img.dtype == np.uint8) else img
        h, w, c = img.shape
        if push_params:
            self._push_params()
        ow, oh = self.out_size(w, h)
        if out is None:
            out = np.empty((oh, ow, c), dtype=np.uint8)
        assert out.shape == (oh, ow, c) and out.dtype == np.uint8 and out.flags.c_contiguous
        self._ck(self._L.rsr_process(self._h, _p(img), w, h, c, _p(out)))
        return out

    def process_fmt(self, img, in_fmt, out_fmt, out=None):
        """rsr_process_fmt: process() for host images in any pair of pixel formats rsr_process_device_fmt takes.  img: a C-contiguous numpy
        array of the shape and dtype of in_fmt (format_array_spec: (h, w, c) uint8 / uint16 for the HWC formats, (3, h, w) for the planar
        ones, (rows, w) for a semi-planar YUV surface); returns (or fills `out` with) the array of out_fmt at out_size_fmt(out_fmt, w, h)."""
        if not isinstance(img, np.ndarray) or not img.flags.c_contiguous:
            raise ValueError("process_fmt: img must be a C-contiguous numpy array")
        w, h, c = format_array_dims(in_fmt, img)
        self._push_params()
        ow, oh = self.out_size_fmt(out_fmt, w, h)
        shape, dtype = format_array_spec(out_fmt, ow, oh, c)
        if out is None:
            out = np.empty(shape, dtype=dtype)
        if not (isinstance(out, np.ndarray) and out.shape == shape and out.dtype == dtype and out.flags.c_contiguous):
            raise ValueError("process_fmt: out must be a C-contiguous %s array of shape %s" % (np.dtype(dtype).name, shape))
        self._ck(self._L.rsr_process_fmt(self._h, _p(img), int(in_fmt), w, h, c, _p(out), int(out_fmt)))
        return out

    def process_many(self, imgs):
        """rsr_process_many: a list of uint8 HWC images in ONE call (small ones share tile batches); returns the list of outputs."""
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in imgs]
        n = len(imgs)
        sizes = [self.out_size(im.shape[1], im.shape[0]) for im in imgs]
        outs = [np.empty((oh, ow, im.shape[2]), dtype=np.uint8) for im, (ow, oh) in zip(imgs, sizes)]
        self._push_params()
        ins_p = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
        outs_p = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        ws = (C.c_int * n)(*[im.shape[1] for im in imgs])
        hs = (C.c_int * n)(*[im.shape[0] for im in imgs])
        cs = (C.c_int * n)(*[im.shape[2] for im in imgs])
        rcs = (C.c_int * n)()
        self._ck(self._L.rsr_process_many(self._h, n, ins_p, ws, hs, cs, outs_p, rcs))
        return outs

    def process_device(self, d_in, w, h, c, d_out, stream=None):
        """d_in/d_out: integer device pointers (e.g. torch tensor .data_ptr())."""
        self._push_params()
        self._ck(self._L.rsr_process_device(self._h, C.c_void_p(int(d_in)), w, h, c, C.c_void_p(int(d_out)),
                                            C.c_void_p(int(stream)) if stream else None))

    def process_device_fmt(self, d_in, in_fmt, w, h, c, d_out, out_fmt, stream=None):
        """rsr_process_device_fmt: process_device with a pixel format (RSR_FMT_*) per side; the planar float formats need c == 3.
        Buffer sizes: image_bytes(in_fmt, w, h, c) and image_bytes(out_fmt, *out_size(w, h), c).  torch tensors: torch_io.upscale."""
        self._push_params()
        self._ck(self._L.rsr_process_device_fmt(self._h, C.c_void_p(int(d_in)), int(in_fmt), w, h, c, C.c_void_p(int(d_out)), int(out_fmt),
                                                C.c_void_p(int(stream)) if stream else None))

    def process_device_batch(self, ins, in_fmt, w, h, c, outs, out_fmt, stream=None):
        """rsr_process_device_batch: len(ins) images of one geometry as merged tile batches.  An entry of ins / outs is an integer device
        pointer (tightly packed) or (ptr, row_pitch, plane_pitch) in bytes, 0 = packed; sizes: image_span()."""
        if len(ins) != len(outs):
            raise ValueError("process_device_batch: %d inputs for %d outputs" % (len(ins), len(outs)))
        self._push_params()
        self._ck(self._L.rsr_process_device_batch(self._h, len(ins), _images(ins), int(in_fmt), w, h, c, _images(outs), int(out_fmt),
                                                  C.c_void_p(int(stream)) if stream else None))

    def tile_count(self, w, h):
        """(nx, ny) of the tile grid of a w x h image at the context's tilesize (rsr_tile_count); tiles count row-major."""
        return tile_count(w, h, self.tilesize, _L=self._L)

    def tile_source_rect(self, w, h, tile):
        """(x0, y0, x1, y1), half-open: the image pixels tile `tile` reads at the context's tilesize and prepadding (rsr_tile_source_rect)."""
        return tile_source_rect(w, h, self.tilesize, self.prepadding, tile, _L=self._L)

    def diff_tiles(self, a, b, fmt, w, h, c, d_mask, stream=None):
        """rsr_diff_tiles: d_mask[t] (device pointer, nx * ny bytes) = 1 where the device images a and b -- an integer pointer or
        (ptr, row_pitch, plane_pitch), as for process_device_batch -- differ inside tile t's source rectangle, else 0.  Asynchronous on
        `stream`; None = the context's stream, synchronously."""
        self._push_params()
        self._ck(self._L.rsr_diff_tiles(self._h, _images([a]), _images([b]), int(fmt), w, h, c, C.c_void_p(int(d_mask)),
                                        C.c_void_p(int(stream)) if stream else None))

    def process_device_masked(self, src, in_fmt, w, h, c, dst, out_fmt, mask, stream=None):
        """rsr_process_device_masked: process_device_batch for ONE image, restricted to the tiles t with mask[t] != 0.  mask: a HOST uint8
        array (or bytes) of nx * ny entries, or an integer address of that many bytes with the count as (address, nmask).  Only the
        output rectangles of those tiles are written; every tile set is the plain call, none set launches nothing."""
        if isinstance(mask, tuple):
            mp, nmask = C.c_void_p(int(mask[0]) or None), int(mask[1])
        elif mask is None:
            mp, nmask = None, 0
        else:
            mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
            mp, nmask = _p(mask), mask.size
        self._push_params()
        self._ck(self._L.rsr_process_device_masked(self._h, _images([src]), int(in_fmt), w, h, c, _images([dst]), int(out_fmt), mp, nmask,
                                                   C.c_void_p(int(stream)) if stream else None))

    def diff_tiles_sequence(self, frames, prev, fmt, w, h, c, d_masks, stream=None):
        """rsr_diff_tiles_sequence: row k of d_masks (device pointer, len(frames) * nx * ny bytes) is what diff_tiles(frames[k - 1], frames[k])
        writes; row 0 compares prev with frames[0], prev=None marks every tile of it.  One launch for all pairs.  frames: pointers or
        (ptr, row_pitch, plane_pitch) descriptors, as for process_device_batch."""
        self._push_params()
        self._ck(self._L.rsr_diff_tiles_sequence(self._h, len(frames), _images(frames), _images([prev]) if prev is not None else None, int(fmt), w, h, c,
                                                 C.c_void_p(int(d_masks)), C.c_void_p(int(stream)) if stream else None))

    def pack_planes(self, planes, surfaces, fmt, w, h, stream=None):
        """rsr_pack_planes: the three-plane frames planes[i] -- (y, u, v) device pointers or (y, u, v, y_pitch, c_pitch), pitches in bytes,
        0 = packed -- into the surfaces surfaces[i] (pointers or (ptr, row_pitch, plane_pitch)) of format fmt, ONE launch for all of
        them.  P010 / P210: every word becomes (word & 1023) << 6.  Asynchronous on `stream`; None = the context's stream, synchronously."""
        if len(planes) != len(surfaces):
            raise ValueError("pack_planes: %d frames for %d surfaces" % (len(planes), len(surfaces)))
        self._ck(self._L.rsr_pack_planes(self._h, len(planes), _planes(planes), _images(surfaces), int(fmt), w, h,
                                         C.c_void_p(int(stream)) if stream else None))

    def unpack_planes(self, surfaces, planes, fmt, w, h, stream=None):
        """rsr_unpack_planes: the way back, surfaces[i] -> planes[i]; P010 / P210: every plane word is the surface word >> 6."""
        if len(planes) != len(surfaces):
            raise ValueError("unpack_planes: %d surfaces for %d frames" % (len(surfaces), len(planes)))
        self._ck(self._L.rsr_unpack_planes(self._h, len(surfaces), _images(surfaces), _planes(planes), int(fmt), w, h,
                                           C.c_void_p(int(stream)) if stream else None))

    def process_device_sequence(self, srcs, in_fmt, w, h, c, dsts, out_fmt, masks, prev_out=None, stream=None):
        """rsr_process_device_sequence: the frames srcs[k] -> dsts[k] (at most RSR_SEQ_MAX) in one call.  masks: a HOST uint8 array of
        len(srcs) * nx * ny entries, row k the tiles of frame k that walk the network (or (address, nmask)); every other output rectangle
        is copied from the frame that computed it last, or from prev_out (a descriptor; it may be dsts[0] itself: frame 0 in place)."""
        if len(srcs) != len(dsts):
            raise ValueError("process_device_sequence: %d inputs, %d outputs" % (len(srcs), len(dsts)))
        if isinstance(masks, tuple):
            mp, nmask = C.c_void_p(int(masks[0]) or None), int(masks[1])
        elif masks is None:
            mp, nmask = None, 0
        else:
            masks = np.ascontiguousarray(masks, dtype=np.uint8).reshape(-1)
            mp, nmask = _p(masks), masks.size
        self._push_params()
        self._ck(self._L.rsr_process_device_sequence(self._h, len(srcs), _images(srcs), int(in_fmt), w, h, c, _images(dsts), int(out_fmt),
                                                     _images([prev_out]) if prev_out is not None else None, mp, nmask,
                                                     C.c_void_p(int(stream)) if stream else None))

    def _check_full_out(self, out, h, w, c):
        ow, oh = self.out_size(w, h)
        if out.shape != (oh, ow, c) or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous uint8 array of shape %s (output ratio %s), not %s %s" % ((oh, ow, c), self._ratio_text(), out.dtype, out.shape))

    def process_rows(self, img, out, row0, row1):
        """Tile rows [row0, row1) of img's tile grid into the full-size `out` (see rsr_process_rows)."""
        h, w, c = img.shape
        self._check_full_out(out, h, w, c)
        self._push_params()
        self._ck(self._L.rsr_process_rows(self._h, _p(img), w, h, c, _p(out), int(row0), int(row1)))
        return out

    def process_tiles(self, img, out, tile0, tile1):
        """Tiles [tile0, tile1) of img's row-major tile grid into the full-size `out` (see rsr_process_tiles)."""
        h, w, c = img.shape
        self._check_full_out(out, h, w, c)
        self._push_params()
        self._ck(self._L.rsr_process_tiles(self._h, _p(img), w, h, c, _p(out), int(tile0), int(tile1)))
        return out

    def net_forward(self, x):
        """x: float16 planar (3,h,w) -> float16 (3,4h,4w)."""
        x = np.ascontiguousarray(x, dtype=np.float16)
        _, h, w = x.shape
        out = np.empty((3, 4 * h, 4 * w), dtype=np.float16)
        self._ck(self._L.rsr_net_forward(self._h, _p(x), w, h, _p(out)))
        return out

    def net_forward_f32(self, x):
        """x: float16 planar (3,h,w) -> float32 (3,4h,4w): conv_last's unrounded result (option "precise" = 1 only)."""
        x = np.ascontiguousarray(x, dtype=np.float16)
        _, h, w = x.shape
        out = np.empty((3, 4 * h, 4 * w), dtype=np.float32)
        self._ck(self._L.rsr_net_forward_f32(self._h, _p(x), w, h, _p(out)))
        return out

    def selfcheck(self, tile=None, w=0, h=0):
        """rsr_selfcheck: one tile through the network in fp16 storage and in precise mode, compared on the device.  tile: float16
        planar (3,h,w) in [0,1], or None = the built-in tile at w x h (0, 0: 148 x 148).  Returns the report as a dict."""
        if tile is not None:
            tile = np.ascontiguousarray(tile, dtype=np.float16)
            _, h, w = tile.shape
        r = SelfcheckReport()
        self._ck(self._L.rsr_selfcheck(self._h, _p(tile), int(w), int(h), C.byref(r)))
        return {k: getattr(r, k) for k, _ in SelfcheckReport._fields_}

    def selfcheck_ranges(self):
        """rsr_selfcheck_ranges of the last selfcheck(): (peak float32[num_convs], nonfinite int64[num_convs]), x4.param order
        (351 entries for the default 23-block model)."""
        n = self.num_convs or NUM_CONVS
        peak = np.zeros(n, dtype=np.float32)
        bad = np.zeros(n, dtype=np.int64)
        self._ck(self._L.rsr_selfcheck_ranges(self._h, peak.ctypes.data_as(C.POINTER(C.c_float)),
                                              bad.ctypes.data_as(C.POINTER(C.c_longlong)), n))
        return peak, bad

    def conv3x3_res_precise(self, x, weight, bias, s1, own_input_residual=False, x_lo=None, res=None, res_lo=None, s2=1.0, want_lo=True):
        """rsr_conv3x3_res_precise: the residual forms on the hi + lo / 2048 stream (hi float16, lo uint8 = bf8 bytes);
        returns (hi, lo), lo None unless want_lo."""
        x = np.ascontiguousarray(x, dtype=np.float16)
        weight = np.ascontiguousarray(weight, dtype=np.float32)
        bias = np.ascontiguousarray(bias, dtype=np.float32)
        cin, h, w = x.shape
        assert weight.shape[0] == 64
        u8 = lambda t: None if t is None else np.ascontiguousarray(t, dtype=np.uint8)  # noqa: E731
        x_lo, res_lo = u8(x_lo), u8(res_lo)
        res = None if res is None else np.ascontiguousarray(res, dtype=np.float16)
        out = np.empty((64, h, w), dtype=np.float16)
        out_lo = np.empty((64, h, w), dtype=np.uint8) if want_lo else None
        self._ck(self._L.rsr_conv3x3_res_precise(self._h, _p(x), _p(x_lo), cin, h, w, _p(weight), _p(bias), float(s1),
                                                 int(bool(own_input_residual)), _p(res), _p(res_lo), float(s2), _p(out), _p(out_lo)))
        return out, out_lo

    def conv3x3(self, x, weight, bias, lrelu=False, upsample2x=False):
        x = np.ascontiguousarray(x, dtype=np.float16)
        weight = np.ascontiguousarray(weight, dtype=np.float32)
        bias = np.ascontiguousarray(bias, dtype=np.float32)
        cin, h, w = x.shape
        cout = weight.shape[0]
        s = 2 if upsample2x else 1
        out = np.empty((cout, h * s, w * s), dtype=np.float16)
        self._ck(self._L.rsr_conv3x3(self._h, _p(x), cin, h, w, int(upsample2x), _p(weight), _p(bias), cout, int(lrelu), _p(out)))
        return out

    def conv3x3_res(self, x, weight, bias, s1, own_input_residual=False, res=None, s2=1.0):
        """v = s1*(conv+b) [+ x[:cout]] [; v = s2*v + res | v + res]  -- see rsr_conv3x3_res."""
        x = np.ascontiguousarray(x, dtype=np.float16)
        weight = np.ascontiguousarray(weight, dtype=np.float32)
        bias = np.ascontiguousarray(bias, dtype=np.float32)
        cin, h, w = x.shape
        cout = weight.shape[0]
        if res is not None:
            res = np.ascontiguousarray(res, dtype=np.float16)
            assert res.shape == (cout, h, w)
        out = np.empty((cout, h, w), dtype=np.float16)
        self._ck(self._L.rsr_conv3x3_res(self._h, _p(x), cin, h, w, _p(weight), _p(bias), cout, float(s1),
                                         int(bool(own_input_residual)), _p(res), float(s2), _p(out)))
        return out

    def preproc(self, band, outw, outh, pad_top, pad_left, crop_x, crop_y, alphaw=0, alphah=0):
        band = np.ascontiguousarray(band, dtype=np.uint8)
        h, w, c = band.shape
        top = np.zeros((3, outh, outw), dtype=np.float16)
        alpha = np.zeros((alphah, alphaw), dtype=np.float16) if c == 4 else None
        self._ck(self._L.rsr_preproc(self._h, _p(band), w, h, c, _p(top), outw, outh, pad_top, pad_left, crop_x, crop_y,
                                     _p(alpha), alphaw, alphah))
        return (top, alpha) if c == 4 else top

    def preproc_tta(self, band, outw, outh, pad_top, pad_left, crop_x, crop_y):
        band = np.ascontiguousarray(band, dtype=np.uint8)
        h, w, c = band.shape
        tops = [np.zeros((3, outh, outw) if k < 4 else (3, outw, outh), dtype=np.float16) for k in range(8)]
        arr = (C.c_void_p * 8)(*[t.ctypes.data for t in tops])
        self._ck(self._L.rsr_preproc_tta(self._h, _p(band), w, h, c, arr, outw, outh, pad_top, pad_left, crop_x, crop_y))
        return tops

    def postproc(self, bottom, out_band, offset_x, gx_max, crop_x, crop_y, alpha=None):
        bottom = np.ascontiguousarray(bottom, dtype=np.float16)
        _, h, w = bottom.shape
        outh, outw, c = out_band.shape
        assert out_band.flags.c_contiguous and out_band.dtype == np.uint8
        if alpha is not None:
            alpha = np.ascontiguousarray(alpha, dtype=np.float16)
        aw = alpha.shape[1] if alpha is not None else 0
        ah = alpha.shape[0] if alpha is not None else 0
        self._ck(self._L.rsr_postproc(self._h, _p(bottom), w, h, _p(alpha), aw, ah, _p(out_band), outw, outh, offset_x,
                                      gx_max, crop_x, crop_y, c))
        return out_band

    def postproc_tta(self, bottoms, out_band, offset_x, gx_max, crop_x, crop_y):
        bottoms = [np.ascontiguousarray(b, dtype=np.float16) for b in bottoms]
        _, h, w = bottoms[0].shape
        outh, outw, c = out_band.shape
        arr = (C.c_void_p * 8)(*[b.ctypes.data for b in bottoms])
        self._ck(self._L.rsr_postproc_tta(self._h, arr, w, h, _p(out_band), outw, outh, offset_x, gx_max, crop_x, crop_y, c))
        return out_band

    def set_profiling(self, on):
        self._ck(self._L.rsr_set_profiling(self._h, int(bool(on))))

    def get_conv_times(self, reset=True):
        """rsr_get_conv_times: accumulated ms per convolution of the loaded model, num_convs entries (351 for the default model)."""
        n = self.num_convs or NUM_CONVS
        arr = (C.c_double * n)()
        self._ck(self._L.rsr_get_conv_times(self._h, arr, n, int(bool(reset))))
        return np.array(arr[:])

    conv_times = get_conv_times

    def get_trace(self, n=1024):
        arr = (C.c_ulonglong * n)()
        self._ck(self._L.rsr_get_trace(self._h, arr, n))
        return np.array(arr[:], dtype=np.uint64)

    def get_profile(self, reset=True):
        p = Profile()
        self._ck(self._L.rsr_get_profile(self._h, C.byref(p), int(bool(reset))))
        return {k: getattr(p, k) for k, _ in Profile._fields_}


_VIDEO_CHROMA = {RSR_FMT_NV12: (1, 1), RSR_FMT_P010: (1, 1), RSR_FMT_NV16: (1, 0), RSR_FMT_P210: (1, 0), RSR_FMT_YUV444P: (0, 0), RSR_FMT_YUV444P10: (0, 0)}


class Video:
    """rsr_video: a host video session on the loaded context sr (include/realsr_hip.h "A video session").  fmt names the layout of the
    three planes -- RSR_FMT_NV12 = yuv420p, RSR_FMT_P010 = yuv420p10le (the code in the LOW bits), NV16 / P210 = yuv422p / yuv422p10le,
    YUV444P / YUV444P10 --, the same on both sides.  send(y, u, v) takes numpy arrays (uint8, or uint16 for the 10-bit formats), strides
    along the rows honoured; every `window` frames run as one sequence call; receive() returns the oldest ready frame as (y, u, v)."""

    def __init__(self, sr, fmt, w, h, window=0):
        self._sr, self._L, self._h = sr, sr._L, None
        self.fmt, self.w, self.h = int(fmt), int(w), int(h)
        sr._push_params()
        hnd = C.c_void_p()
        sr._ck(self._L.rsr_video_open(sr._h, self.fmt, self.w, self.h, int(window), C.byref(hnd)))
        self._h = hnd
        if not hasattr(sr, "_videos"):
            sr._videos = weakref.WeakSet()  # RealSR.close closes the sessions that are still open
        sr._videos.add(self)
        ow, oh, win = C.c_int(0), C.c_int(0), C.c_int(0)
        sr._ck(self._L.rsr_video_info(self._h, C.byref(ow), C.byref(oh), C.byref(win)))
        self.out_size, self.window = (ow.value, oh.value), win.value
        self._dtype = np.dtype(np.uint8 if self.fmt in (RSR_FMT_NV12, RSR_FMT_NV16, RSR_FMT_YUV444P) else np.uint16)

    def _shapes(self, w, h):
        sx, sy = _VIDEO_CHROMA[self.fmt]
        return (h, w), (h >> sy, w >> sx), (h >> sy, w >> sx)

    def _entry(self, planes, w, h, what):
        """The rsr_planes of three numpy arrays (rows contiguous, u and v with one row stride)."""
        es = self._dtype.itemsize
        for a, shape in zip(planes, self._shapes(w, h)):
            if not isinstance(a, np.ndarray) or a.dtype != self._dtype or a.shape != shape:
                raise ValueError("%s: a plane must be a %s array of shape %s" % (what, self._dtype, shape))
            if (a.shape[1] > 1 and a.strides[1] != es) or (a.shape[0] > 1 and a.strides[0] < a.shape[1] * es):
                raise ValueError("%s: the rows of a plane must be contiguous and lie upwards in memory (strides %s)" % (what, a.strides))
        y, u, v = planes
        if u.shape[0] > 1 and u.strides[0] != v.strides[0]:
            raise ValueError("%s: u and v must have one row stride" % what)
        p = Planes()
        p.y, p.u, p.v = y.ctypes.data, u.ctypes.data, v.ctypes.data
        p.y_pitch = y.strides[0] if y.shape[0] > 1 else 0
        p.c_pitch = u.strides[0] if u.shape[0] > 1 else 0
        return p

    def _live(self):
        if self._h is None:
            raise RealSRError(RSR_E_STATE, "the video session is closed")
        return self._h

    def send(self, y, u, v):
        """One frame in; the window-th frame runs the window before this returns."""
        h = self._live()
        self._sr._push_params()
        self._sr._ck(self._L.rsr_video_send(h, C.byref(self._entry((y, u, v), self.w, self.h, "send"))))

    @property
    def ready(self):
        return int(self._L.rsr_video_ready(self._live()))

    def receive(self, out=None):
        """The oldest ready frame as (y, u, v) -- new arrays, or the three arrays `out` (views with contiguous rows are written in place)."""
        h = self._live()
        if out is None:
            out = tuple(np.empty(s, dtype=self._dtype) for s in self._shapes(*self.out_size))
        self._sr._ck(self._L.rsr_video_receive(h, C.byref(self._entry(tuple(out), self.out_size[0], self.out_size[1], "receive"))))
        return tuple(out)

    def flush(self):
        """Run the frames that are pending as a partial window."""
        h = self._live()
        self._sr._push_params()
        self._sr._ck(self._L.rsr_video_flush(h))

    def reset(self):
        """A scene cut, a seek: the next frame is compared with nothing."""
        self._sr._ck(self._L.rsr_video_reset(self._live()))

    def close(self):
        if self._h is not None:
            if getattr(self._sr, "_h", None):  # (RealSR.close closes its sessions first, so a live handle has a live context)
                self._L.rsr_video_close(self._h)
            self._h = None
            getattr(self._sr, "_videos", set()).discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def selfcheck_tile(w=0, h=0):
    """rsr_selfcheck_tile (host-only): the self-check's built-in tile, float16 planar (3,h,w); 0, 0 = 148 x 148."""
    if w == 0 and h == 0:
        w = h = 148
    t = np.empty((3, int(h), int(w)), dtype=np.float16)
    rc = lib().rsr_selfcheck_tile(_p(t), int(w), int(h))
    if rc != RSR_OK:
        raise RealSRError(rc, lib().rsr_last_error(None).decode())
    return t


def image_bytes(fmt, w, h, c=3):
    """rsr_image_bytes (host-only): bytes of a w x h x c image in pixel format `fmt` (RSR_FMT_*; NV12: w*h*3/2, P010: 3*w*h,
    NV16: 2*w*h, P210: 4*w*h, YUV444P: 3*w*h, YUV444P10: 6*w*h, U16_HWC: 2*w*h*c)."""
    n = lib().rsr_image_bytes(int(fmt), int(w), int(h), int(c))
    if n < 0:
        raise RealSRError(int(n), lib().rsr_last_error(None).decode())
    return int(n)


_FMT_HWC = {RSR_FMT_U8_HWC: np.uint8, _FMT_U16_HWC: np.uint16}
_FMT_PLANAR = {RSR_FMT_F16_CHW: np.float16, RSR_FMT_F32_CHW: np.float32, RSR_FMT_YUV444P: np.uint8, RSR_FMT_YUV444P10: np.uint16}
_FMT_SURFACE = {RSR_FMT_NV12: (np.uint8, 1), RSR_FMT_P010: (np.uint16, 1), RSR_FMT_NV16: (np.uint8, 0), RSR_FMT_P210: (np.uint16, 0)}  # dtype, vertical chroma shift


def format_array_spec(fmt, w, h, c=3):
    """(shape, dtype) of the tightly packed numpy array that holds a w x h x c image in pixel format `fmt`: (h, w, c) for the HWC formats,
    (3, h, w) for the planar ones, (h + (h >> csy), w) for a semi-planar YUV surface (the UV rows behind the Y rows)."""
    if fmt in _FMT_HWC:
        return (h, w, c), np.dtype(_FMT_HWC[fmt])
    if fmt in _FMT_PLANAR:
        return (3, h, w), np.dtype(_FMT_PLANAR[fmt])
    if fmt in _FMT_SURFACE:
        dt, csy = _FMT_SURFACE[fmt]
        return (h + (h >> csy), w), np.dtype(dt)
    raise ValueError("unknown pixel format %r" % (fmt,))


def format_array_dims(fmt, a):
    """(w, h, c) of the image the array `a` holds in pixel format `fmt` (format_array_spec's inverse); ValueError for a wrong dtype or rank."""
    if fmt in _FMT_HWC and a.ndim == 3:
        h, w, c = a.shape
    elif fmt in _FMT_PLANAR and a.ndim == 3 and a.shape[0] == 3:
        (_, h, w), c = a.shape, 3
    elif fmt in _FMT_SURFACE and a.ndim == 2:
        csy = _FMT_SURFACE[fmt][1]
        rows, w = a.shape
        h, c = (rows * 2 // 3 if csy else rows // 2), 3
    else:
        raise ValueError("format %r does not come as an array of shape %s" % (fmt, a.shape))
    shape, dtype = format_array_spec(fmt, w, h, c)
    if a.shape != shape or a.dtype != dtype:
        raise ValueError("format %r: a %d x %d x %d image is a %s array of shape %s, not %s %s" % (fmt, w, h, c, dtype.name, shape, a.dtype.name, a.shape))
    return int(w), int(h), int(c)


def yuv_constants(matrix=709, range_=0, bits=8):
    """rsr_yuv_constants (host-only): the 18 float32 constants of the NV12 / P010 definition (include/realsr_hip.h) as an array."""
    out = np.zeros(18, dtype=np.float32)
    rc = lib().rsr_yuv_constants(int(matrix), int(range_), int(bits), out.ctypes.data_as(C.POINTER(C.c_float)), 18)
    if rc != RSR_OK:
        raise RealSRError(rc, lib().rsr_last_error(None).decode())
    return out


def tile_count(w, h, tilesize, _L=None):
    """rsr_tile_count (host-only): (nx, ny) = (ceil(w / tilesize), ceil(h / tilesize)); tiles are counted row-major."""
    L = _L or lib()
    nx, ny = C.c_int(0), C.c_int(0)
    rc = L.rsr_tile_count(int(w), int(h), int(tilesize), C.byref(nx), C.byref(ny))
    if rc != RSR_OK:
        raise RealSRError(rc, L.rsr_last_error(None).decode())
    return nx.value, ny.value


def tile_source_rect(w, h, tilesize, prepadding, tile, _L=None):
    """rsr_tile_source_rect (host-only): (x0, y0, x1, y1), half-open, the image pixels the padded tile reads (include/realsr_hip.h)."""
    L = _L or lib()
    r = [C.c_int(0) for _ in range(4)]
    rc = L.rsr_tile_source_rect(int(w), int(h), int(tilesize), int(prepadding), int(tile), *[C.byref(v) for v in r])
    if rc != RSR_OK:
        raise RealSRError(rc, L.rsr_last_error(None).decode())
    return tuple(v.value for v in r)


def sequence_sources(masks, has_prev, _L=None):
    """rsr_sequence_sources (host-only): masks is an (n, ntiles) array; returns the int32 (n, ntiles) array src with src[k, t] = k where
    masks[k, t] is set, else the last j < k with masks[j, t] set, else -1 (the previous output: RealSRError unless has_prev)."""
    L = _L or lib()
    m = np.ascontiguousarray(masks, dtype=np.uint8)
    if m.ndim != 2:
        raise ValueError("sequence_sources: masks must be (n, ntiles), not %s" % (m.shape,))
    src = np.zeros(m.shape, dtype=np.int32)
    rc = L.rsr_sequence_sources(m.shape[0], m.shape[1], _p(m), int(bool(has_prev)), src.ctypes.data_as(C.POINTER(C.c_int)))
    if rc != RSR_OK:
        raise RealSRError(rc, L.rsr_last_error(None).decode())
    return src


def _images(entries):
    """A ctypes array of rsr_image from pointers or (ptr, row_pitch, plane_pitch) tuples."""
    arr = (Image * max(len(entries), 1))()
    for a, e in zip(arr, entries):
        ptr, row, plane = e if isinstance(e, (tuple, list)) else (e, 0, 0)
        a.data, a.row_pitch, a.plane_pitch = int(ptr), int(row), int(plane)
    return arr


def _planes(entries):
    """A ctypes array of rsr_planes from (y, u, v) or (y, u, v, y_pitch, c_pitch) tuples."""
    arr = (Planes * max(len(entries), 1))()
    for a, e in zip(arr, entries):
        y, u, v, yp, cp = tuple(e) if len(e) == 5 else tuple(e) + (0, 0)
        a.y, a.u, a.v, a.y_pitch, a.c_pitch = int(y) or None, int(u) or None, int(v) or None, int(yp), int(cp)
    return arr


def image_span(fmt, w, h, c=3, row_pitch=0, plane_pitch=0):
    """rsr_image_span (host-only): bytes from the data pointer to one past the last byte of a w x h x c image with these pitches."""
    n = lib().rsr_image_span(int(fmt), int(w), int(h), int(c), int(row_pitch), int(plane_pitch))
    if n < 0:
        raise RealSRError(int(n), lib().rsr_last_error(None).decode())
    return int(n)


def device_memory(gpuid=0):
    """(free MiB, total MiB) of HIP device gpuid (rsr_device_memory)."""
    f, t = C.c_longlong(0), C.c_longlong(0)
    rc = lib().rsr_device_memory(int(gpuid), C.byref(f), C.byref(t))
    if rc != RSR_OK:
        raise RealSRError(rc, lib().rsr_last_error(None).decode())
    return f.value, t.value


def rccl_probe():
    """rsr_rccl_probe (host-only): None when librccl can be dlopen'ed with every entry point rsr_create_group's RCCL branch
    calls, else the reason."""
    L = lib()
    rc = L.rsr_rccl_probe()
    return None if rc == RSR_OK else L.rsr_last_error(None).decode()


def create_group(gpuids, parampath, modelpath, tta_mode=False):
    """rsr_create_group: one context per GPU, the model packed once and broadcast (RCCL).  Returns (list of RealSR, transport)."""
    L = lib()
    n = len(gpuids)
    hs = (C.c_void_p * n)()
    ids = (C.c_int * n)(*[int(g) for g in gpuids])
    rc = L.rsr_create_group(hs, ids, n, int(bool(tta_mode)), str(parampath).encode(), str(modelpath).encode())
    if rc != 0:
        raise RealSRError(rc, L.rsr_last_error(None).decode())
    srs = [RealSR(int(g), tta_mode, _adopt=C.c_void_p(hs[i])) for i, g in enumerate(gpuids)]
    return srs, L.rsr_group_transport().decode()


def process_group(srs, img, out=None):
    """rsr_process_group: ONE image, its tiles dealt over the contexts in contiguous ranges of equal load."""
    L = lib()
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w, c = img.shape
    for s in srs:
        s._push_params()
    ow, oh = srs[0].out_size(w, h)  # (members that disagree: RSR_E_ARG from the call)
    if out is None:
        out = np.empty((oh, ow, c), dtype=np.uint8)
    if out.shape != (oh, ow, c) or out.dtype != np.uint8 or not out.flags.c_contiguous:
        raise ValueError("out must be a contiguous uint8 array of shape %s (output ratio %s)" % ((oh, ow, c), srs[0]._ratio_text()))
    hs = (C.c_void_p * len(srs))(*[s._h for s in srs])
    rc = L.rsr_process_group(hs, len(srs), _p(img), w, h, c, _p(out))
    if rc != 0:
        raise RealSRError(rc, L.rsr_last_error(None).decode())
    return out


def tile_partition(w, h, tilesize, prepadding, parts):
    """rsr_tile_partition: the contiguous tile ranges rsr_process_group deals to `parts` contexts (host-only)."""
    b = (C.c_int * (parts + 1))()
    n = lib().rsr_tile_partition(int(w), int(h), int(tilesize), int(prepadding), int(parts), b)
    if n < 0:
        raise RealSRError(n, lib().rsr_last_error(None).decode())
    return list(b[:n + 1])


# ---- tile sharding for multi-GPU runs: pure host logic, shared by bench + tests ----
def shard_frames(n_frames, world_size, rank):
    """Frames dealt round-robin to ranks (the reference's work-stealing queue, main.cpp:811-828,
    made deterministic).  Returns the list of frame indices this rank processes."""
    return list(range(rank, n_frames, world_size))
