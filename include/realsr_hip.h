/*
 * realsr_hip.h -- C-ABI of the MI355X-native RealSR x4 tiled-inference engine (librealsr_hip.so).
 *
 * This is the drop-in boundary for the reference's `class RealSR`
 * (/root/reference/src/realsr.h:13-42), the only seam between the CLI/orchestration
 * (/root/reference/src/main.cpp) and the compute path.  Plain pointers and sizes only; no C++,
 * ncnn or torch types.  Every entry point cites the reference interface it replaces.
 *
 * Conventions
 *   - return 0 = ok, negative = error (RSR_E_*); rsr_last_error() gives a message.  (The reference
 *     returns 0 unconditionally and its callers ignore the value -- main.cpp:786,325 -- so this is a
 *     strict superset.)
 *   - images are HWC uint8, tightly packed, c in {3,4}, RGB(A) order (main.cpp:275-276); the output is
 *     caller-allocated (w*scale) x (h*scale) x c.  The engine never retains either pointer.
 *   - one context per GPU (main.cpp:778-791); rsr_process* are thread-safe on a shared context
 *     (the reference calls process() concurrently from jobs_proc threads, main.cpp:811-828): every
 *     call owns private device image buffers, pinned staging and a copy stream ("lane", up to
 *     max_lanes in flight, further callers wait); the network kernels of all calls are queued on one
 *     compute stream, so upload(k+1) | kernels(k) | download(k-1) overlap; SMALL images of concurrent
 *     calls are merged into one tile batch (option "merge"; the reference's "-j 4:4:4 for many small
 *     images", README.md:61) -- same bytes, shared launches.
 *   - rsr_last_error() reports the CALLING THREAD's most recent failure.
 *   - there is NO CPU fallback: gpuid must name a HIP device; the reference's "-g -1" CPU path
 *     (RealSR::process_cpu) lives only in oracle/ as the parity checker.
 */
#ifndef REALSR_HIP_H
#define REALSR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSR_OK 0
#define RSR_E_ARG (-1)      /* bad argument */
#define RSR_E_IO (-2)       /* cannot open / truncated file */
#define RSR_E_FORMAT (-3)   /* .param/.bin not parseable */
#define RSR_E_GRAPH (-4)    /* parsed graph is not the RRDBNet(3,3,64,nb,32) x4.param describes, for any nb in 1..RSR_MAX_RRDB */
#define RSR_E_DEVICE (-5)   /* HIP error / no such device */
#define RSR_E_STATE (-6)    /* call order (e.g. process before load) */
#define RSR_E_NOMEM (-7)

/* The deepest RRDBNet a context loads: RRDB blocks of the x4 graph (x4.param of the reference's model directories has 23; the anime
 * networks 6, "lite" trainings 16).  A model of nb blocks has 15 nb + 6 convolutions, 966 at this bound -- which is what bounds the
 * conv table a packed blob's header may announce and the `n` of rsr_selfcheck_ranges / rsr_get_conv_times. */
#define RSR_MAX_RRDB 64

typedef struct rsr_ctx rsr_ctx;

/* ---- lifecycle -------------------------------------------------------------------------- */

/* RealSR::RealSR(int gpuid, bool tta_mode, int num_threads)   realsr.h:16, realsr.cpp:13-23.
 * gpuid: HIP device ordinal (>= 0).  num_threads is accepted for signature parity and ignored
 * (it only sizes ncnn's CPU thread pool in the reference, realsr.cpp:17). */
int rsr_create(rsr_ctx** out, int gpuid, int tta_mode, int num_threads);

/* RealSR::~RealSR   realsr.cpp:25-35 */
void rsr_destroy(rsr_ctx* ctx);

/* RealSR::load(parampath, modelpath)   realsr.h:19-23, realsr.cpp:37-143.
 * Parses the ncnn text graph and tagged weight stream (fp16-tagged or raw fp32), checks that the
 * DAG is exactly the x4.param RRDBNet, packs the weights for the MFMA kernels and uploads them.
 * Depth: the graph may have any number nb of RRDB blocks in 1..RSR_MAX_RRDB (23 in the reference's files); the depth is derived from
 * the node count and everything else -- operator types and parameters (never names), nf 64, gc 32, three RDBs per RRDB, the 0.2 / 1
 * Eltwise residuals, two nearest x2 Interp stages -- must equal the canonical graph of that depth, else RSR_E_GRAPH with a message that
 * names the depth found or the first node that differs.  Stats "model_blocks" / "model_convs" read what was loaded.  A context that
 * already ran may load a model of another depth: plans and workspace stay, the self-check report, what option "precise_auto" made of
 * it, and the per-convolution times of the old model are dropped.
 * Out of scope: another nf / gc, x2 / x1 / x8 networks, pixel-unshuffle inputs, SRVGG-style compact networks (they need other
 * epilogues and a second reference), and other operator spellings of the same network (a residual written as two BinaryOps ...). */
int rsr_load(rsr_ctx* ctx, const char* parampath, const char* modelpath);

/* The public mutable fields `scale`, `tilesize`, `prepadding` assigned after load()
 * (realsr.h:31-33, main.cpp:788-790).  scale must be 4 (main.cpp:533-537); tilesize >= 32
 * (main.cpp:539-552; smaller values are accepted for tests, >= 1); prepadding >= 0 (10 for
 * models-DF2K*, main.cpp:663-667). */
int rsr_set_params(rsr_ctx* ctx, int scale, int tilesize, int prepadding);

/* ---- the hot path ----------------------------------------------------------------------- */

/* RealSR::process(const ncnn::Mat& in, ncnn::Mat& out) const   realsr.h:25, realsr.cpp:145-523.
 * `in`/`out` are HOST pointers (what ncnn::Mat::data is at main.cpp:275-276).  H2D, all tiles,
 * D2H; returns when `out` is complete.  `out` is (w * out_scale) x (h * out_scale) x c (option "out_scale", default 4). */
int rsr_process(rsr_ctx* ctx, const uint8_t* in, int w, int h, int c, uint8_t* out);

/* n images in one call (no reference counterpart: main.cpp's proc threads call process() once per image, :311-331).  Every image is
 * what rsr_process would make of it; up to max_lanes of them are in flight at once on helper threads of the call, so that SMALL
 * images share tile batches (option "merge") without the host having to be multi-threaded.  rcs (may be NULL) receives the code of
 * every image; the return value is the first failure (0 = all ok).  out[i]: (w[i] * out_scale) x (h[i] * out_scale) x c[i]. */
int rsr_process_many(rsr_ctx* ctx, int n, const uint8_t* const* in, const int* w, const int* h, const int* c, uint8_t* const* out, int* rcs);

/* Same computation with both images already resident in this context's device memory
 * (what the reference keeps in VkMat in_gpu/out_gpu, realsr.cpp:211-233, minus the PCIe hops).
 * `stream` is a hipStream_t (NULL = the context's own stream).  Asynchronous when a stream is
 * given: the caller synchronises.  When nothing else is in flight on the context the kernels are
 * enqueued on `stream` itself; otherwise they run on the context's compute stream, ordered behind
 * the work already on `stream` and in front of what the caller enqueues on it next.
 * d_out: "4w x 4h" reads "(w * out_scale) x (h * out_scale)" (option "out_scale", default 4). */
int rsr_process_device(rsr_ctx* ctx, const void* d_in, int w, int h, int c, void* d_out, void* stream);

/* Pixel formats of device-resident images (no reference counterpart: the reference's images are uint8 HWC only). */
#define RSR_FMT_U8_HWC 0  /* what rsr_process_device takes: uint8 [h][w][c], c in {3,4} */
#define RSR_FMT_F16_CHW 1 /* planar fp16 [3][h][w], values in [0,1]; c must be 3 (tightly packed unless described by an rsr_image) */
#define RSR_FMT_F32_CHW 2 /* planar fp32 [3][h][w], likewise */
/* YUV 4:2:0 surfaces: what a hardware video decoder hands over and an encoder takes (ids 3 and 7 stay unknown) */
#define RSR_FMT_NV12 4  /* uint8  Y [h][w], then interleaved UV [h/2][w/2][2]; c must be 3 */
#define RSR_FMT_P010 5  /* uint16 little-endian, the code in the HIGH 10 bits (code << 6), same layout */
/* YUV 4:2:2 surfaces: what broadcast and archive codecs hold -- chroma halved horizontally only ("YUV 4:2:2" below; id 6 stays unknown too) */
#define RSR_FMT_NV16 8  /* uint8  Y [h][w], then interleaved UV [h][w/2][2]; c must be 3 */
#define RSR_FMT_P210 9  /* uint16 little-endian, the code in the HIGH 10 bits (code << 6), same layout */
/* Planar YUV 4:4:4: what screen recordings, mezzanine masters and software video frameworks hold ("YUV 4:4:4" below; ids 10 and 11 stay unknown) */
#define RSR_FMT_YUV444P   12  /* uint8  planes Y, U, V, each [h][w]; c must be 3 */
#define RSR_FMT_YUV444P10 13  /* uint16 little-endian, the code in the LOW 10 bits (yuv444p10le), same layout */
/* 16-bit RGB(A): what scans, raw developments and renders hold ("16-bit RGB(A)" below; ids 14 and 15 stay unknown, as do -1, 3, 6, 7, 10, 11) */
#define RSR_FMT_U16_HWC 16    /* uint16 little-endian [h][w][c], c in {3,4}, full range 0 .. 65535 */
/* (Mind the contrast: P010 / P210 hold code << 6, as hardware decoders write it; YUV444P10 holds the code itself, as every producer of planar 4:4:4 does.) */

/* rsr_process_device with a pixel format per side: what a tensor pipeline holds (float CHW in [0,1]) goes in and comes out without a
 * uint8 hop.  The two formats are independent; rsr_process_device(...) is exactly rsr_process_device_fmt(..., U8, ..., U8, ...).
 * Same stream / ordering contract.  A planar format with c != 3 or an unknown format: RSR_E_ARG.  A call with a planar format on
 * either side is never merged with concurrent calls (option "merge"); it is still safe next to them.
 *   Input.   F16: the half IS the network input (the uint8 path feeds fp16(float(k) * (1/255.f)) for byte k: a caller who passes
 *            exactly those halfs gets exactly the uint8 path's result).  F32: rounded to fp16, to nearest even.  Values are not
 *            clamped.  The halo of a tile is filled by the same reflect-101 indexing as for uint8 images.
 *   Output.  Let r be the fp32 value the uint8 conversion sees for a pixel in the context's current mode: the fp16-rounded conv_last
 *            result (default), the fp32 mean of the eight fp16 values (TTA), conv_last's fp32 result or the fp32 mean of those
 *            (option "precise").  F32 receives min(max(r, 0), 1); F16 that value rounded once to fp16 (lossless in the default
 *            non-TTA mode).  Quantising it with floor(v * 255 + 0.5) reproduces the uint8 path's byte.
 *   Option "bgr" swaps planes 0 and 2 the way it swaps bytes 0 and 2 of a uint8 pixel.
 *   Option "out_scale" 2 / 1: d_out is (w * out_scale) x (h * out_scale) and receives the box means of those values (rsr_set_option).
 * This is rsr_process_device_batch (below) with n = 1 and tightly packed images.
 * Out of scope: RGBA in planar form.  (Host pointers: rsr_process_fmt below; rsr_process stays uint8 HWC.) */
int rsr_process_device_fmt(rsr_ctx* ctx, const void* d_in, int in_fmt, int w, int h, int c, void* d_out, int out_fmt, void* stream);

/* RSR_FMT_NV12 / RSR_FMT_P010 on either side of rsr_process_device_fmt / rsr_process_device_batch, independently of the other side (NV12 ->
 * NV12, P010 -> P010, NV12 -> F16_CHW, U8_HWC -> NV12 ...): the YUV <-> RGB conversion and the chroma resampling happen inside the pre- and
 * post-processing kernels, so no RGB frame exists outside the library -- a 1080p frame at x4 would be 199 MB of fp16 RGB for 50 MB of
 * NV12 -- and a 10-bit source never passes through 8 bits.  Everything said of the planar float formats holds: the stream contract, no
 * merging with concurrent calls, batches grouped alike, windows whose outside stays untouched, TTA, "precise", "out_scale" 4 / 2 / 1.
 * Option "bgr" concerns RGB sides only.
 *   Layout.  A surface is a plane of Y [h][w] and a plane of interleaved (U, V) pairs [h/2][w/2][2]: `data` is Y(0,0); the row pitch serves
 *            both planes (a UV row has as many bytes as a Y row); the UV plane starts at data + plane_pitch, 0 = h * row pitch (tightly
 *            packed: rsr_image_bytes = w*h*3/2 for NV12, 3*w*h for P010).  rsr_process_device_fmt takes packed surfaces.
 *   Errors.  RSR_E_ARG before anything is launched: c != 3; an odd w or h of a YUV input; a YUV output whose w * out_scale, h * out_scale or
 *            tilesize * out_scale is odd (out_scale 1 only: no 2 x 2 chroma quad may cross a tile); P010 with an odd data pointer or pitch.
 *   Options. "yuv_matrix" 709 [default] / 601 / 2020 and "yuv_range" 0 = limited [default] / 1 = full (rsr_set_option).  "yuv_siting" says
 *            where a chroma sample sits: 0 [default] = at the CENTRE of its 2 x 2 luma quad in both directions (MPEG-1 / JPEG siting), which
 *            the definition below describes; 1 = left, 2 = top-left: "Chroma siting" behind it.
 *   The definition, exact.  All arithmetic is fp32; every multiplication and every addition is rounded by itself, in the order written (no
 *   contraction).  Constants are computed in double from Kr and Kb -- 0.2126 / 0.0722 (709), 0.299 / 0.114 (601), 0.2627 / 0.0593 (2020),
 *   Kg = 1 - Kr - Kb -- and rounded once to fp32, written fp32(.) below; rsr_yuv_constants returns them.  b = 8 (NV12) or 10 (P010) bits,
 *   k = 2^(b-8).  Limited range: yoff = 16k, ys = 1/(219k), cs = 1/(224k), yscale = 219k, cscale = 224k; full range: yoff = 0,
 *   ys = cs = 1/(2^b - 1), yscale = cscale = 2^b - 1.  coff = 2^(b-1) always.
 *   Decode, image pixel (x, y) (a halo pixel: the reflect-101 index is taken first, exactly as for uint8 images):
 *            Y is the code at (x, y) (P010: word >> 6).  U and V come from the four nearest chroma samples with weights 3/4 and 1/4 per
 *            axis, indices clamped at the image edge: horizontally first, (3 * c_near + c_far) * 0.25f, then vertically the same way
 *            (exact for codes).  yn = (Y - yoff) * ys, cb = (U - coff) * cs, cr = (V - coff) * cs;
 *            R = yn + fp32(2(1-Kr)) * cr;  G = (yn - fp32(2Kb(1-Kb)/Kg) * cb) - fp32(2Kr(1-Kr)/Kg) * cr;  B = yn + fp32(2(1-Kb)) * cb.
 *            Each of R, G, B is clamped to [0, 1] and rounded to fp16, to nearest even: the network input.
 *   Encode.  d(x, y, q) = what RSR_FMT_F32_CHW holds at the context's out_scale (clamped, TTA-merged, box-reduced as defined there).
 *            Y' = (Kr * R + Kg * G) + Kb * B; Y code = floor(Y' * yscale + (yoff + 0.5f)) clamped to [0, 2^b - 1].  Chroma of a 2 x 2 quad:
 *            per channel m = ((d00 + d01) + (d10 + d11)) * 0.25f, Ym from m as Y' from d, Cb = (Bm - Ym) * fp32(1/(2(1-Kb))),
 *            Cr = (Rm - Ym) * fp32(1/(2(1-Kr))), code = floor(C * cscale + (coff + 0.5f)) clamped alike.  P010 stores code << 6.
 *   Chroma siting, exact ("yuv_siting" 1 / 2; it holds for both sides of a call).  1 = LEFT, the default of H.264, HEVC, AV1 and MPEG-2
 *   (chroma_sample_loc_type 0): chroma is co-sited with the even luma columns and lies between the two luma rows.  2 = TOP-LEFT, BT.2020 /
 *   UHD HEVC (chroma_sample_loc_type 2): chroma is co-sited with luma (2X, 2Y).  Call an axis on which chroma is co-sited with the even luma
 *   index "cos": siting 1 is cos horizontally and centre vertically, siting 2 is cos on both axes.  Everything not said here is the
 *   definition above: constants, luma, the RGB matrix, clamps, code rounding, reflect-101 first, every operation rounded by itself.
 *   Decode.  Luma index i of an axis with N/2 chroma samples, n = i >> 1.  A centre axis: (3 * c_near + c_far) * 0.25f as above.  A cos axis:
 *            c[n] for an even i, (c[n] + c[min(n + 1, N/2 - 1)]) * 0.5f for an odd one.  Horizontally first, then vertically (both rules are
 *            exact in fp32 for 8- and 10-bit codes, so the order cannot show; it is fixed all the same).
 *   Encode.  Luma is unchanged: the Y plane does not depend on the siting.  Chroma of quad (X, Y), per channel, d as above:
 *            Hs(y) = (d(xl, y) + d(2X+1, y)) + (d(2X, y) + d(2X, y)) -- the [1 2 1] filter about the co-sited column, unnormalised -- with
 *            xl = 2X - 1, but xl = 2X where column 2X is the first column of its TILE's output rectangle (the image's first column included).
 *            Siting 1: m = (Hs(2Y) + Hs(2Y+1)) * 0.125f.  Siting 2: m = ((Hs(yu) + Hs(2Y+1)) + (Hs(2Y) + Hs(2Y))) * 0.0625f, yu = 2Y - 1, but
 *            yu = 2Y on the first row of the tile's rectangle.  Ym, Cb, Cr and the codes follow from m as above.  A tile's rectangle starts
 *            at multiples of tilesize * out_scale output pixels (even: see Errors).
 *            Why the filter clamps at a tile's edge and does not take the neighbouring tile's column: that column is part of another tile's
 *            network output, which may belong to another batch of the call; the tile's own halo there is not computed (the last convolutions
 *            skip the margin nothing reads), and computing it would widen the hot convolution launches.  The price: one chroma column (row)
 *            per tile edge -- every tilesize * out_scale output pixels, 800 at the defaults -- is filtered [0 3 1] / 4 instead of [1 2 1] / 4.
 * On the output side conv_last leaves its planar blob and one more small launch (postproc_tiles_yuv) writes the surface: the route RGBA, TTA
 * and "out_scale" below 4 take anyway.  Out of scope: host pointers of rsr_process* and the CLI, which stay uint8 RGB(A) (YUV frames in host memory: "A video session" below). */

/* Host-only: the fp32 constants of the definition above for yuv_matrix `matrix`, yuv_range `range` and `bits` = 8 / 10, the first n of
 * { yoff, ys, coff, cs, 2(1-Kr), 2Kb(1-Kb)/Kg, 2Kr(1-Kr)/Kg, 2(1-Kb), Kr, Kg, Kb, yscale, yoff + 0.5, cscale, coff + 0.5, 1/(2(1-Kb)),
 * 1/(2(1-Kr)), 2^b - 1 } (18 values).  RSR_E_ARG for any other matrix, range or depth. */
int rsr_yuv_constants(int matrix, int range, int bits, float* out, int n);

/* ---- YUV 4:2:2: RSR_FMT_NV16 / RSR_FMT_P210 in and out (no reference counterpart) -------------------------------------------------------
 * DVCPRO-HD, Digital Betacam, ProRes 422, DNxHD, XDCAM HD422, MPEG-2 4:2:2 profile and uncompressed broadcast captures hold chroma halved
 * HORIZONTALLY only.  Such a surface goes in and comes out as it is -- no chroma row is thrown away to make NV12 of it, and no RGB frame
 * exists outside the library.  Either side of a call, independently of the other (NV16 -> NV16, P210 -> P210, NV16 -> NV12, P210 -> F16_CHW,
 * U8_HWC -> NV16 ...), through every entry point that takes NV12 / P010: rsr_process_device_fmt, _batch (windows, pitched surfaces), _masked,
 * _sequence, rsr_diff_tiles, rsr_diff_tiles_sequence; in every mode: TTA, "precise", every "yuv_matrix" / "yuv_range", "out_scale" 4 / 2 / 1,
 * rsr_set_out_ratio, rsr_set_out_ratio_xy.
 *   Layout.  The rsr_image conventions of NV12 / P010: `data` is Y(0,0); one row pitch serves both planes (a UV row [w/2][2] has as many
 *            bytes as a Y row); the UV plane starts at data + plane_pitch, 0 = h * row pitch, and has h rows.  Tightly packed:
 *            rsr_image_bytes = 2*w*h for NV16, 4*w*h for P210; rsr_image_span follows, the UV plane's last row at plane + (h - 1) * row.
 *   Admission.  Every check is RSR_E_ARG before anything is launched; c must be 3; P210 refuses an odd data pointer or pitch, as P010 does.
 *            A 4:2:2 INPUT needs an even w; any h >= 1 is taken, odd heights included.  A 4:2:2 OUTPUT needs the ratio rule (w * nx and
 *            tilesize * nx divisible by dx, h * ny and tilesize * ny divisible by dy) and w * nx / dx and tilesize * nx / dx EVEN, so that no
 *            2 x 1 chroma pair crosses a tile or the image's edge, with "YUV" in rsr_last_error where only this parity refuses; the two row
 *            quotients carry no parity rule.  1280 x 1080 at (3/2, 1) and tile 200 is taken (1920 x 1080, tile rectangle 300 x 200); 36 x 26
 *            at 3/2 and tile 16 gives 54 x 39, taken here and refused for NV12; tile 30 at 3/2 (45 columns) and "out_scale" 1 at an odd tile
 *            size stay refused.  rsr_out_size_fmt states the rule of any output format.
 *   The definition, exact.  Everything not said here is the NV12 / P010 definition above: the constants of rsr_yuv_constants (b = 8 for NV16,
 *   10 for P210), luma, the matrix, clamps, code rounding, reflect-101 first, fp32 throughout, every operation rounded by itself (no contraction).
 *   Decode, image pixel (x, y).  The chroma row is y itself: there is no vertical filter.  Horizontally, with w/2 chroma columns:
 *            "yuv_siting" 0 (centre): (3 * c_near + c_far) * 0.25f, c_near = c[x >> 1], the far index +-1 by the parity of x, clamped to
 *            [0, w/2 - 1].  "yuv_siting" 1 (left): the co-sited rule, c[n] for x = 2n, (c[n] + c[min(n + 1, w/2 - 1)]) * 0.5f for x = 2n + 1.
 *            "yuv_siting" 2 (top-left) has no vertical meaning at 4:2:2 and IS siting 1: the same kernels, the same bytes.
 *   Encode, output row y, chroma pair X, per channel; d = what RSR_FMT_F32_CHW holds at the context's scale or ratio.
 *            Siting 0: m = (d(2X, y) + d(2X+1, y)) * 0.5f.  Siting 1 / 2: m = Hs(y) * 0.25f, Hs(y) = (d(xl, y) + d(2X+1, y)) + (d(2X, y) +
 *            d(2X, y)), xl = 2X - 1, but xl = 2X where column 2X is the first column of its TILE's output rectangle: the tile-first clamp of
 *            the 4:2:0 sitings, for the reason given there.  Ym, Cb, Cr and the codes follow from m as for 4:2:0; the (U, V) pair lands at
 *            UV row y, pair X.  Luma is per pixel and independent of the siting.  P210 stores code << 6.
 *   Diff.    rsr_diff_tiles / rsr_diff_tiles_sequence compare the Y samples of the tile's source rectangle and the (U, V) pairs of chroma
 *            columns max((sx0 >> 1) - 1, 0) .. min(((sx1 - 1) >> 1) + 1, w/2 - 1) on rows sy0 .. sy1 - 1; P210 compares whole words.
 *   Sequences.  The propagated UV rectangle of a tile has the tile's own rows.
 * One more small launch behind conv_last writes the surface, as for NV12 / P010: postproc_tiles_yuv / postproc_tiles_yuv_area with two stacked
 * 2 x 1 pairs per thread.  rsr_out_size_yuv and rsr_out_size_yuv_xy keep their exact 4:2:0 behaviour.
 * Out of scope: three-plane SUBSAMPLED layouts as a format of their own (yuv422p: rsr_pack_planes interleaves the two chroma planes into an
 * NV16 / P210 surface and rsr_unpack_planes takes one apart, "Three-plane YUV frames" below; "YUV 4:4:4" below says why rsr_image cannot
 * describe them -- planar 4:4:4 itself is RSR_FMT_YUV444P / YUV444P10), 4:1:1, a siting per side, host pointers
 * of rsr_process*, groups of GPUs and the CLI, which stay uint8 RGB(A) (YUV frames in host memory: "A video session" below). */

/* Host-only (no GPU): the admission rule and the size of an output in `out_fmt` at the pair of ratios and the tile size given -- *ow = w *
 * nx / dx, *oh = h * ny / dy (either pointer may be NULL).  RSR_FMT_U8_HWC / F16_CHW / F32_CHW: exactly rsr_out_size_xy.  RSR_FMT_NV12 /
 * P010: exactly rsr_out_size_yuv_xy.  RSR_FMT_NV16 / P210: the 4:2:2 rule above.  RSR_FMT_YUV444P / YUV444P10: exactly rsr_out_size_xy (a
 * 4:4:4 surface has no parity rule).  RSR_FMT_U16_HWC: exactly rsr_out_size_xy.  RSR_E_ARG for an unknown format. */
int rsr_out_size_fmt(int out_fmt, int num_x, int den_x, int num_y, int den_y, int tilesize, int w, int h, int* ow, int* oh);

/* ---- 16-bit RGB(A): RSR_FMT_U16_HWC in and out (no reference counterpart) -----------------------------------------------------------------
 * The still-image sibling of the 10-bit video formats: a 16-bit scan, raw development or render goes in without losing its low byte, and the
 * network's sub-code precision -- what keeps an upscaled gradient from banding -- leaves in integer form, also for an 8-bit source.  Either side
 * of a call, independently of the other (U16 -> U16, U8 -> U16, U16 -> U8, U16 <-> F16_CHW / F32_CHW, any YUV format <-> U16), through
 * rsr_process_device_fmt, _batch (windows, pitches), _masked, _sequence, rsr_diff_tiles, rsr_diff_tiles_sequence and the host call
 * rsr_process_fmt; in every mode: TTA, "precise", "bgr", "out_scale" 4 / 2 / 1, rsr_set_out_ratio, rsr_set_out_ratio_xy.  A call with U16 on a
 * side is never merged with concurrent calls, like the planar formats.
 *   Layout.  uint16 [h][w][c], c in {3, 4}, native little-endian words, full range, RGB(A) order; option "bgr" swaps samples 0 and 2 as it
 *            swaps bytes.  rsr_image: `data` and row_pitch must be multiples of 2 (RSR_E_ARG otherwise); plane_pitch is ignored.  A row is
 *            2*w*c bytes; rsr_image_bytes = 2*w*h*c; rsr_image_span and rsr_out_size_fmt follow U8_HWC (rsr_out_size_fmt is exactly
 *            rsr_out_size_xy).  There is no parity rule.
 *   Input.   The network input of sample k is fp16(float(k) * fp32(1/65535)): ONE multiplication, k UNSIGNED (an int16 view of the words holds
 *            the codes >= 32768 as negatives; the library reads uint16).  The alpha sample is skipped, as for U8_HWC.  For every byte b the
 *            sample 257 * b gives exactly the half the uint8 path makes of b: an 8-bit image widened by x257 is the same network input.
 *   Precision, honestly.  The network reads fp16, so the 65,536 codes land on 7,169 distinct inputs; the round trip code -> input -> code is
 *            off by at most 16 codes (near white), against 128 codes for a hop through 8 bits.
 *   Output.  Let d be what RSR_FMT_F32_CHW holds for the output pixel in the context's current mode, scale, ratio or pair (in [0, 1]).  The
 *            sample is (uint16) floor(d * 65535.f + 0.5f), the product and the sum each rounded by itself (nothing is contracted).  In the
 *            default mode d is an fp16-rounded value, spaced up to 2^-11 apart: about 32 codes near white.  Under option "precise" it is
 *            conv_last's fp32 result: "precise" (the CLI: RSR_PRECISE=1) is the recommended companion of 16-bit output.
 *   Alpha (c == 4).  Both sides must then be HWC -- U8 or U16, in any combination.  The bicubic x4 alpha is computed from the source's alpha
 *            samples in SOURCE units, with the arithmetic of the uint8 path: four rows of four taps, row = ((p0 c0 + p1 c1) + p2 c2) +
 *            p3 c3, then the four rows likewise.  A U16 source rounds every one of these products and sums by itself (fp32, nothing is
 *            contracted); a U8 source keeps the uint8 path's own code.  Where the two depths differ ONE multiplication follows the
 *            bicubic sum: by 257.f (U8 -> U16) or by fp32(1/257) (U16 -> U8).  Then, as ever: the clamp to [0, max] (max = 65535 for a U16
 *            output), the box / area mean, floor(mean + 0.5).  U8 -> U8 is bit for bit what it was.
 *   Diff.    rsr_diff_tiles / _sequence compare bytes [x0*2c, x1*2c) of the rows of the tile's source rectangle, alpha included.
 *   Sequences.  The propagated rectangle is the tile's output rectangle, 2c bytes per pixel.
 * conv_last leaves its planar blob and ONE more launch (postproc_tiles and its box / area siblings) writes the image: the route RGBA, TTA and
 * YUV outputs take.  At out_scale 4 without TTA a thread makes two neighbouring pixels -- 12 bytes as three dword stores, an RGBA pair as
 * two 8-byte stores, where the address allows, else as samples --, elsewhere one.  Option "dbg" 32768 / 65536 force one / two pixels per
 * thread at out_scale 4 and change no byte: the LDS-staged kernels they force for uint8 images are uint8-only. */

/* Host pointers for every format pair: rsr_process with a pixel format per side.  `in` and `out` are tightly packed HOST images (`out` of the
 * size rsr_out_size_fmt / rsr_image_bytes state for the context's ratio); the call is synchronous and returns when `out` is complete.  Any
 * pair rsr_process_device_fmt takes goes: H2D on a copy stream (pinned memory of rsr_host_alloc travels directly, pageable memory through
 * pinned staging), the device path, D2H, one wait.  The progress callback fires as for a synchronous rsr_process_device call.  Safe next to
 * every other call from several threads.  Never merged with concurrent calls; no tile ranges, no groups.  Every argument is checked before
 * anything is enqueued (RSR_E_ARG; RSR_E_STATE before rsr_load).  rsr_process_fmt(U8 -> U8) writes the bytes rsr_process writes. */
int rsr_process_fmt(rsr_ctx* ctx, const void* in, int in_fmt, int w, int h, int c, void* out, int out_fmt);

/* ---- alpha through the network: option "alpha_net" (no reference counterpart) ------------------------------------------------------------
 * Game textures, sprites, UI atlases, scans with cut-outs and logos are RGBA.  By default the colour of such an image walks the network and
 * comes out sharp while its alpha takes ncnn's bicubic x4 and comes out soft: the two disagree along every edge, which shows as a halo.
 * With option "alpha_net" 1 a call whose images have c == 4 (RSR_FMT_U8_HWC / RSR_FMT_U16_HWC on both sides, in any combination) sends the
 * alpha through the same network, as a gray image, instead.  0 [default]: everything is byte for byte and launch for launch what it was.  A
 * c == 3 call is not concerned at either value: same launches, same bytes.
 *   The definition, exact.  Let G be the gray image of the source: c == 3, the source's sample type (uint8 or uint16), the same w x h, all
 *            three samples of pixel (x, y) equal to the source's alpha sample there.  G enters the network as any U8 / U16 RGB image does
 *            (fp16(b / 255); fp16(float(k) * fp32(1/65535)) for U16), with the same tiles, halo and reflect-101 as the colour.  For an
 *            output pixel let A0, A1, A2 be what RSR_FMT_F32_CHW planes 0, 1, 2 would hold for a call on G with option "bgr" 0 in the
 *            context's current mode, scale, ratio or pair: under TTA the eight variants merged first; under "precise" conv_last's fp32
 *            result; below x4 the box or area mean per channel; each value in [0, 1].  Then, in this order:
 *              1. m = min(((A0 + A1) + A2) * fp32(1/3), 1): fp32 throughout, every operation rounded by itself, the constant computed in
 *                 double and rounded once;
 *              2. a U8 destination stores floor(m * 255.f + 0.5f) clamped to 0 .. 255, the product and the sum each rounded by itself --
 *                 unlike the fp16-valued colour, m * 255 is not exact in fp32, so the rule does not leave a contraction (fma) to the compiler;
 *              3. a U16 destination stores (uint16) floor(m * 65535.f + 0.5f), likewise (the colour's own store, "16-bit RGB(A)" above).
 *            No x257 or 1/257 step exists on this route: the depth of the source decides how G is read, the depth of the destination how m
 *            is stored.  "bgr" does not change the alpha.  The colour samples of the call are exactly those of the same call with
 *            "alpha_net" 0.  Nothing outside the destination window is written, as ever.
 *   A constant alpha does not come out constant.  The network is no identity on flat images: f(255) need not be 255, and a fully opaque
 *            image may leave with alpha 254 here and there.  By default the library does not look for constant tiles: that changes bytes
 *            and needs a host round trip on the device paths, so it is an option of its own, "alpha_adaptive" below.  Without it, a caller
 *            who knows an image to be opaque sets "alpha_net" to 0 for it, as the CLI does under RSR_ALPHA=net.
 *   Cost.    The tiles of an RGBA batch walk the network TWICE, over the same tables, plan and workspace (no workspace byte is added): expect
 *            about twice the frame time of "alpha_net" 0 (profiles/alpha_net.txt).  The colour pass runs as ever; the alpha pass is one
 *            more preprocessing launch, the network, and one post-processing launch that stores sample 3 alone.
 *   Where.   Every route: rsr_process, _many, _tiles, _rows, merged concurrent calls, rsr_process_fmt, rsr_process_device, _fmt, _batch
 *            (windows, pitches), _masked and _sequence (a tile's alpha depends on its padded source rectangle alone, and the diffs compare
 *            the alpha bytes: masks stay valid; the rectangles are propagated behind the last batch as ever).  rsr_process_group: the
 *            members must agree on "alpha_net" (RSR_E_ARG otherwise, like differing ratios).  The option is read when a tile batch is
 *            enqueued.  The progress callback stays one call per tile.  Under profiling the per-class times, launch counts and
 *            FLOPs of rsr_profile include both passes; its tile count does not.
 *   Stats.   "alpha_net": the value in force.  "alpha_tiles": tiles run through the alpha pass since creation -- a masked call adds its
 *            marked tiles only, a c == 3 call none.
 * Out of scope: luma-weighted or single-channel alpha, premultiplied alpha, alpha for planar or YUV formats, one network pass shared by
 * colour and alpha.
 *
 * ---- "alpha_adaptive": skip the alpha pass on tiles of constant alpha ------------------------------------------------------------------
 * In sprites, atlases, logos and cut-outs the alpha is constant over most of the area and interesting along silhouettes only.  Option
 * "alpha_adaptive" 1 (0 [default]; anything else RSR_E_ARG, the value in force stays) concerns calls with c == 4 under "alpha_net" 1 and
 * nothing else: with "alpha_net" 0, and for a c == 3 call, it is ignored -- same launches, same bytes, same stats.
 *   The rule, exact.  A tile is FLAT when all alpha samples of its source rectangle (rsr_tile_source_rect: the padded tile clipped to the
 *            image) are equal, compared at the source's depth: 8 bits for U8, 16 for U16 -- two U16 values that share a high byte differ.
 *            The output rectangle of a flat tile holds, in all four samples, the bytes "alpha_net" 0 writes: its alpha is the bicubic
 *            value, which for a constant k is k converted to the destination's depth.  Every other tile's rectangle holds the bytes
 *            "alpha_net" 1 writes.  The colour samples are those of "alpha_net" 0 everywhere, as before.  The decision is a function of the
 *            source rectangle alone, so masks, diffs and sequences stay valid.
 *   THE HOST WAITS.  The library scans the alpha on the device in front of the colour pass (one launch per tile batch; under TTA once per
 *            tile), copies one byte per tile to the host and reads them there while the colour pass runs.  So with the option on, an RGBA
 *            call under "alpha_net" 1 performs ONE HOST WAIT PER TILE BATCH, also where the call is asynchronous (a stream argument, the
 *            device entry points): the calling thread blocks until the caller's stream has reached the scan -- everything enqueued on it
 *            before the call has finished by then -- and the context is held meanwhile.  Such a call must not be made under stream
 *            capture.  The GPU has the colour pass queued behind the scan, so it does not run dry.  With the option off no call gains a
 *            wait.
 *   Cost.    profiles/alpha_adaptive.txt.  No tile varies: no alpha pass, no launch beyond the scan.  All vary: the alpha pass of
 *            "alpha_net" 1 on the batch's own tables.  Otherwise the varying tiles run as a tile batch of their own, built on the fly, in a
 *            subset of the batch's slots: no workspace byte is added.
 *   Where.   Every route "alpha_net" takes.  rsr_process_group: the members must agree on the option (RSR_E_ARG otherwise).  Read when a
 *            tile batch is enqueued.  The progress callback stays one call per tile.  Under profiling the scan counts in the
 *            preprocessing class.
 *   Stats.   "alpha_adaptive": the value in force.  "alpha_tiles_flat": tiles whose alpha pass was skipped since creation.  "alpha_tiles"
 *            keeps its meaning, tiles run through the alpha pass: now the varying ones only.  "alpha_wait_us": host time spent in the waits.
 * Out of scope: a device-side decision without a host wait, a tolerance ("nearly flat"), flat-colour tiles, a public scan entry point. */

/* ---- "dither": position-keyed ordered dither for integer outputs (no reference counterpart) ------------------------------------------------
 * Every integer the library writes is floor(d * M + 0.5) of a value d it holds far more finely than one code.  An upscaler makes large smooth
 * gradients -- sky, vignettes, anime backgrounds, out-of-focus areas -- and rounding each pixel to the nearest code turns them into steps
 * several pixels wide: the banding "16-bit RGB(A)" above exists to avoid.  Most callers cannot take 16 bits (an 8-bit encoder wants NV12, a
 * 10-bit one P010, a PNG for the web is 8 bits); the library is the one place that still has the unquantised value at the moment of the store.
 * Option "dither" 1 (0 [default]; anything else RSR_E_ARG, the value in force stays): every COLOUR sample of every INTEGER output format is
 * rounded against a position-dependent threshold instead of 0.5.  With 0 every launch, byte and stat is what it was.
 *   The rule, exact.  For the sample at column x, row y of its own plane, in the coordinates of the output image -- (0, 0) is the sample
 *            rsr_image::data points at (the window's own origin for a window of a canvas):
 *              h     = (x * 0xC13FA9A9u + y * 0x91E10DA5u) mod 2^32      (uint32 wrap-around)
 *              k     = h >> 25                                            0 .. 127
 *              theta = (2k + 1) * 2^-8                                    1/256 .. 255/256, exact in fp32
 *            the R2 low-discrepancy lattice in integer form: no table, blue-noise-like on gradients, the 128 values equally frequent.  For
 *            a sample of a subsampled plane (UV of NV12 / P010 / NV16 / P210) x and y are the chroma sample's own indices (X, Y).  The three
 *            colour samples of an interleaved HWC pixel share the pixel's theta, U and V of one chroma sample share theirs: no chroma noise.
 *   RGB codes (U8_HWC: M = 255; U16_HWC: M = 65535).  The code is floor(add_rn(mul_rn(d, M), theta)), every operation rounded by itself, d
 *            what RSR_FMT_F32_CHW holds for that pixel in the same context: clamped to [0, 1], TTA merged, the box or area mean taken,
 *            fp16-rounded in the default mode and fp32 under "precise".
 *   YUV codes.  floor(v * scale + (offset + 0.5f)) clamped to [0, maxcode] becomes floor(add_rn(mul_rn(v, scale), add_rn(offset, theta))) with
 *            the same clamp.  P010 / P210 still store code << 6, YUV444P10 the code low.  The value v that is quantised is the one of
 *            "dither" 0: the quad mean, the sited filters and their tile-first clamp are untouched.
 *   Not touched.  Alpha samples are those of "dither" 0, the bicubic alpha and the "alpha_net" alpha alike.  RSR_FMT_F16_CHW / F32_CHW outputs
 *            are not concerned (same launches, same bytes).  "bgr" swaps samples, not thresholds.
 *   What follows.  theta is a multiple of 2^-8 below 1, so n + theta is exact for every integer n < 2^16: a d that is exactly a code keeps
 *            its code -- black stays 0, white stays M, an 8-bit-exact image passes unchanged -- and no clamp can be hit for d in [0, 1].
 *            The pattern is static and keyed to image coordinates, so a tile's output rectangle is still a function of its padded source
 *            rectangle alone: masked calls, sequences, propagated rectangles, the video session's reuse of prev_out, tile ranges
 *            (rsr_process_tiles, _rows), batches, merged concurrent calls and group sharding all give the bytes of the plain call.  An
 *            `out` window of a canvas carries the pattern from the window's own origin.
 *   Depths, honestly.  At 8 bits the default mode has about eight fp16 steps per code near white: the dither has something to work with.
 *            At 10 bits fp16 has two steps per code near white, at 16 bits none to spare: for P010 / P210 / YUV444P10 / U16_HWC the option
 *            is accepted and follows the same rule, and "precise" is its recommended companion.
 *   Route.   The rounding lives in the post-processing launch.  A U8_HWC RGB call without TTA at out_scale 4, whose bytes conv_last writes
 *            itself by default, takes the planar blob and ONE postproc_tiles launch while the option is on -- the route U16, RGBA, TTA and
 *            YUV calls take anyway -- and the host calls' early download of the first half of the image (the split tail, which hangs on the
 *            fused store) is off, as for U16.  profiles/dither.txt has the cost.
 *   Where.   Every route.  rsr_process_group: the members must agree on the option (RSR_E_ARG otherwise).  Read when a tile batch is
 *            enqueued.  The CLI: RSR_DITHER=1.
 *   Stats.   "dither": the value in force.
 * Out of scope: error diffusion, a temporally varying pattern (it would break the masked / sequence invariant and is hostile to encoders),
 * a table-based blue-noise mask, dithered alpha, a strength, a per-side or per-format switch, a dithering epilogue fused into conv_last,
 * dither of the fp16 float output. */

/* ---- YUV 4:4:4: RSR_FMT_YUV444P / RSR_FMT_YUV444P10 in and out (no reference counterpart) -------------------------------------------------
 * Screen recordings (H.264 Hi444PP, HEVC RExt, AV1 4:4:4, lossless x264 / FFV1: subsampled chroma smears coloured text), ProRes 4444 and
 * DNxHR 444 masters, and whatever was ever RGB inside libavfilter, VapourSynth or an encoder's input hold three FULL planes of integer codes:
 * yuv444p / yuv444p10le.  Such a surface goes in and comes out as it is -- no chroma is halved to make NV16 of it, a 10-bit source never
 * passes through 8 bits, and no RGB frame exists outside the library.  Either side of a call, independently of the other (YUV444P -> YUV444P,
 * YUV444P10 -> NV12, P010 -> YUV444P10, U8_HWC -> YUV444P, YUV444P -> F16_CHW ...), through every entry point that takes NV16 / P210:
 * rsr_process_device_fmt, _batch (windows, pitched surfaces), _masked, _sequence, rsr_diff_tiles, rsr_diff_tiles_sequence; in every mode: TTA,
 * "precise", every "yuv_matrix" / "yuv_range", "out_scale" 4 / 2 / 1, rsr_set_out_ratio, rsr_set_out_ratio_xy.
 *   Layout.  The rsr_image conventions of the planar float formats: `data` is Y(0,0); one row pitch serves all three planes, 0 = tightly packed;
 *            plane q (0 = Y, 1 = U, 2 = V) starts at data + q * plane_pitch, 0 = h * row pitch.  Tightly packed: rsr_image_bytes = 3*w*h for
 *            YUV444P, 6*w*h for YUV444P10; rsr_image_span follows.  YUV444P takes any byte pointer and any byte pitches; YUV444P10 refuses an
 *            odd data pointer, row pitch or plane pitch, as the planar float formats refuse non-multiples of their element size.
 *            The 10-bit code sits in the LOW bits of its word (P010 / P210: code << 6).  On input the bits above bit 9 are ignored (word &
 *            1023); on output they are written 0.
 *   Admission.  Every check is RSR_E_ARG before anything is launched; c must be 3; w, h >= 1.  There is NO PARITY RULE on either side: a 4:4:4
 *            surface has no chroma pairs and no quads, so nothing can cross a tile or the image's edge.  Any w, any h, any tile size and any
 *            admitted ratio is taken, exactly as for the RGB outputs: a 4:4:4 output needs the ratio rule and nothing else, and
 *            rsr_out_size_fmt(RSR_FMT_YUV444P*, ...) is exactly rsr_out_size_xy.  35 x 25 at tile 16 is taken at x4, x2, x1 and 3/2 alike.
 *   Options.  "yuv_matrix" and "yuv_range" apply.  "yuv_siting" has no meaning -- every chroma sample sits on its luma sample -- and 0, 1 and 2
 *            give the same kernels and the same bytes.  "bgr" concerns RGB sides only.
 *   The definition, exact.  Everything not said here is the NV12 / P010 definition above: the constants of rsr_yuv_constants (b = 8 for
 *   YUV444P, 10 for YUV444P10), the matrix, clamps, code rounding, reflect-101 first, fp32 throughout, every operation rounded by itself.
 *   Decode, image pixel (x, y).  Y, U, V are the codes at (x, y) of planes 0, 1, 2 (YUV444P10: word & 1023).  There is no chroma filter.
 *            yn = (Y - yoff) * ys, cb = (U - coff) * cs, cr = (V - coff) * cs; then the matrix, the clamp to [0, 1] and the rounding to fp16
 *            word for word as for NV12.
 *   Encode, output pixel (x, y); d = what RSR_FMT_F32_CHW holds there at the context's scale, ratio or pair.  Y' = (Kr * R + Kg * G) + Kb * B;
 *            Y code = floor(Y' * yscale + (yoff + 0.5f)) clamped to [0, 2^b - 1]; Cb = (B - Y') * fp32(1/(2(1-Kb))), Cr = (R - Y') *
 *            fp32(1/(2(1-Kr))), codes floor(C * cscale + (coff + 0.5f)) clamped alike -- the 4:2:0 rule with m = d.  Nothing is filtered, so
 *            no tile-first clamp exists.  Codes are stored as they are; the high six bits of a YUV444P10 word are 0.
 *   Diff.    rsr_diff_tiles / rsr_diff_tiles_sequence compare the three planes over the tile's source rectangle and nothing beyond it;
 *            YUV444P10 compares whole words.
 *   Sequences.  The propagated rectangle is the tile's output rectangle in each of the three planes.
 * One more small launch behind conv_last writes the surface, as for every YUV output: postproc_tiles_yuv444 / postproc_tiles_yuv444_area, one
 * output pixel per thread and three plane stores.
 * Out of scope: the three-plane SUBSAMPLED layouts (yuv420p, yuv422p and their 10-bit forms) as a pixel format -- rsr_image cannot express
 * them: its one plane_pitch is the distance Y -> U AND U -> V.  Their chroma planes are smaller than the luma plane, so the two distances
 * differ, and a window of such a canvas needs a U -> V distance (and a chroma row pitch) of its own, for which the descriptor has no field --
 * rsr_pack_planes ("Three-plane YUV frames" below) interleaves the chroma planes to NV12 / NV16 on the device, shift of the 10-bit words
 * included, and rsr_unpack_planes is the way back; semi-planar or packed 4:4:4 (NV24, P410, Y410, AYUV); 12- and 16-bit codes (rsr_yuv_constants keeps refusing them);
 * 4:1:1; planar RGB (GBRP); a siting per side; host pointers of rsr_process*, groups of GPUs and the CLI, which stay uint8 RGB(A) (YUV
 * frames in host memory: "A video session" below). */

/* ---- rational output scales: x3, x3/2, x4/3, x9/4 ... area-averaged on the device (no reference counterpart) --------------------------
 * Option "out_scale" (rsr_set_option) takes the x4 image down to x2 or x1 inside the library.  rsr_set_out_ratio generalises it to the
 * scales real resize jobs ask for -- 720p -> 1080p is 3/2, 1080p -> 1440p 4/3, 480p -> 1080p 9/4, 720p -> 2160p 3/1 -- so that the x4
 * frame (199 MB of fp16 for a 1080p source) never leaves the library to be resampled outside.
 *   num / den is reduced by its gcd; after that den must be 1, 2, 3 or 4 and 1 <= num / den <= 4:
 *            d = 1: 1, 2, 3, 4;  d = 2: 3/2, 5/2, 7/2;  d = 3: 4/3, 5/3, 7/3, 8/3, 10/3, 11/3;  d = 4: 5/4, 7/4, 9/4, 11/4, 13/4, 15/4.
 *            Anything else: RSR_E_ARG, the ratio in force stays.  A new ratio takes effect for the next call, like "out_scale".
 *   4/1, 2/1 and 1/1 ARE option "out_scale" 4 / 2 / 1: the same kernels, launches and bytes.  rsr_set_option("out_scale", v) keeps its
 *            exact behaviour (v = 3 is still RSR_E_ARG: x3 is rsr_set_out_ratio(ctx, 3, 1)) and leaves a fractional ratio again.
 *   Stats    "out_num" / "out_den": the ratio in force, in lowest terms; "out_scale" reads 4 / 2 / 1 as ever and 0 while any other ratio
 *            is in force.
 *   Sizes.   The output is (w * n / d) x (h * n / d) (rsr_out_size).  Every rsr_process* entry point honours the ratio -- host, device,
 *            _fmt, _batch with windows, _tiles / _rows, _many, _group (whose members must agree on it), merged concurrent calls -- and
 *            wherever a comment says "(w * out_scale) x (h * out_scale)" read "(w * n / d) x (h * n / d)".  Row pitches and windows are
 *            checked against that size.
 *   Errors.  RSR_E_ARG at call time, before anything is launched: w * n, h * n or tilesize * n not divisible by d (reduced terms).  The
 *            tile condition is what keeps an averaging footprint inside its tile: every tile's output rectangle then starts on a whole
 *            output pixel (tile 200 serves d = 2 and 4; tile 198 or 201 serves d = 3), and the reduction stays one small per-tile launch
 *            behind conv_last (postproc_tiles_area) -- no whole-frame pass, no materialised x4 image.
 *   Formats. Outputs RSR_FMT_U8_HWC (c 3 and 4), RSR_FMT_F16_CHW, RSR_FMT_F32_CHW.  The input side is independent: a YUV input works at
 *            any ratio.
 *            (RSR_FMT_NV12 / RSR_FMT_P010 outputs: "YUV output at a ratio" below.)
 *   The definition, exact.  Scale n / d in lowest terms, L = 4 d.  Along one axis, on the integer grid where x4 pixel i covers
 *   [i n, (i + 1) n), output pixel X covers [X L, (X + 1) L): its taps are i = floor(X L / n) .. floor(((X + 1) L - 1) / n), with the
 *   integer weights g_i = min((X + 1) L, (i + 1) n) - max(X L, i n), each in 1 .. n, summing to L; at most 4 taps per axis for the
 *   permitted ratios.  Coordinates are the image's (they equal the tile's own: tiles start on whole output pixels).
 *            1. c(x, y) = min(max(r(x, y), 0), 1), r the fp32 value the uint8 conversion sees at x4 pixel (x, y) in the context's current
 *               mode, as for "out_scale" (what RSR_FMT_F32_CHW holds at out_scale 4; under TTA the eight variants are merged first, in
 *               the existing order)
 *            2. horizontally first: for every source row, H = g_i0 * c_i0, then H = H + g_i * c_i in ascending i.  The weights are
 *               converted to fp32; every multiplication and every addition is rounded by itself (no contraction)
 *            3. then vertically the same way over the H of the tap rows: V = g_j0 * H_j0, then V = V + g_j * H_j in ascending j
 *            4. m = min(V * fp32(1 / (16 d^2)), 1), the constant computed in double and rounded once
 *            5. RSR_FMT_F32_CHW stores m, RSR_FMT_F16_CHW m rounded once to fp16, RSR_FMT_U8_HWC floor(m * 255 + 0.5) clamped to 0 .. 255
 *            6. alpha (uint8, c == 4): the bicubic x4 alpha value of the x4 path, clamped to [0, 255], under the same weights, order and
 *               constant, stored as floor(mean + 0.5)
 *            7. "bgr" swaps channels 0 and 2 on store as ever; "precise" changes only what r is.
 *   (For 2/1 the definition gives the bits of "out_scale" 2 -- weights 2, 2 and 1/16 against plain adds and 1/4 -- but 2/1 takes the box
 *   kernel all the same.)
 * Out of scope: a YUV OUTPUT (RSR_FMT_NV12 / RSR_FMT_P010) whose w * n / d, h * n / d or tilesize * n / d is odd: RSR_E_ARG ("YUV output at
 * a ratio" below says what is admitted).
 *
 * YUV output at a ratio.  RSR_FMT_NV12 / RSR_FMT_P010 on the OUTPUT side at any permitted n / d -- 720p NV12 -> 1080p NV12 is one call at
 * 3/2 -- through every device entry point that honours ratios and YUV formats: rsr_process_device_fmt, _batch (windows and pitched
 * surfaces included), _masked and _sequence (whose propagated rectangles are the reduced ones).  A YUV input stays independent of it.
 *   Admission.  The ratio rule above (w * n, h * n and tilesize * n divisible by d), and w * n / d, h * n / d and tilesize * n / d EVEN, so
 *            that no 2 x 2 chroma quad crosses a tile or the image's edge: 1280 x 720 at 3/2 and tile 200 (tile rectangle 300), 1920 x 1080
 *            at 4/3 and tile 198 (264) or 201 (268), 720 x 480 at 9/4 and tile 200 (450), any even size at 3/1 and tile 200 (600); not tile
 *            30 at 3/2 (45, odd).  Anything else: RSR_E_ARG before anything is launched, with "YUV" in rsr_last_error (rsr_out_size_yuv).
 *   The definition, exact.  d(X, Y, q) = what RSR_FMT_F32_CHW holds for output pixel (X, Y) at the context's ratio n / d: steps 1 to 4
 *            above, unchanged.  The surface is "Encode" of the YUV section applied to those d: luma per pixel, chroma from the quad mean
 *            at "yuv_siting" 0 and from the [1 2 1] filters of "Chroma siting" at 1 and 2, with the same clamp at the first column / row of
 *            every TILE's output rectangle -- which now starts at multiples of tilesize * n / d output pixels.  TTA and "precise" change
 *            only what r is, as ever.
 *   One more small launch behind conv_last writes the surface (postproc_tiles_yuv_area: one thread per 2 x 2 quad, every output pixel
 *   gathered tap by tap as postproc_tiles_area gathers it); 4/1, 2/1 and 1/1 keep postproc_tiles_yuv, the same launches and bytes.
 *   Host pointers, groups of GPUs and the CLI stay uint8 RGB(A), as before. */
int rsr_set_out_ratio(rsr_ctx* ctx, int num, int den);
/* Host-only (no GPU): *ow = w * n / d, *oh = h * n / d for n / d = num / den reduced (either pointer may be NULL), or RSR_E_ARG for a ratio
 * outside the set above, or when w * n, h * n or tilesize * n is not divisible by d: what a call at that ratio and tile size refuses. */
int rsr_out_size(int num, int den, int tilesize, int w, int h, int* ow, int* oh);
/* Host-only (no GPU): rsr_out_size for a YUV 4:2:0 OUTPUT (RSR_FMT_NV12 / RSR_FMT_P010) -- the same results and conventions, and RSR_E_ARG
 * also for an odd w or h, or when w * n / d, h * n / d or tilesize * n / d is odd: what a call with a YUV output at that ratio and tile size
 * refuses.  For 4/1, 2/1 and 1/1 that is the rule of the YUV section ("Errors": tilesize * out_scale even). */
int rsr_out_size_yuv(int num, int den, int tilesize, int w, int h, int* ow, int* oh);

/* ---- a ratio per axis: DVD and HDV frames to square-pixel sizes (no reference counterpart) -------------------------------------------
 * Frames whose pixels are not square need a different ratio along x and along y: NTSC DVD 720 x 480 -> 1920 x 1080 is 8/3 along x and 9/4
 * along y, PAL DVD 720 x 576 -> 1920 x 1080 is 8/3 and 15/8, HDV / XDCAM 1440 x 1080 -> 1920 x 1080 is 4/3 and 1 (-> 3840 x 2160: 8/3 and
 * 2), DVCPRO-HD 1280 x 1080 -> 1920 x 1080 is 3/2 and 1.  rsr_set_out_ratio_xy sets the pair; the area average is separable, so nothing
 * but the two axes' taps and weights differ from rsr_set_out_ratio.
 *   Each axis is reduced by its gcd; after that it needs 1 <= den <= 8 and 1 <= num / den <= 4: 67 ratios per axis (the 19 above; d = 5:
 *            6/5 .. 19/5; d = 6: 7/6 .. 23/6; d = 7: 8/7 .. 27/7; d = 8: 9/8 .. 31/8 -- the eighths are what PAL needs).  A footprint then
 *            has at most 5 taps per axis; the 19 ratios of rsr_set_out_ratio keep at most 4.  Anything else: RSR_E_ARG, the ratio in force
 *            stays.  rsr_set_out_ratio, rsr_out_size, rsr_out_size_yuv and option "out_scale" keep their exact behaviour, every refusal
 *            included (d <= 4 there; a lone 3 is no out_scale).
 *   Equal axes.  rsr_set_out_ratio_xy(ctx, n, d, n, d) with n / d one of the 19 IS rsr_set_out_ratio(ctx, n, d): the same kernels,
 *            launches, bytes and stats -- so 4/1, 2/1 and 1/1 on both axes are option "out_scale".  Any other pair is area-averaged, 4/1 x
 *            2/1 and 15/8 x 15/8 included.  rsr_set_out_ratio and option "out_scale" afterwards set both axes again.
 *   Stats    "out_num_x" / "out_den_x" / "out_num_y" / "out_den_y": the pair in force, always valid.  "out_num" / "out_den" read the common
 *            reduced ratio while the axes agree and 0 / 0 while they differ; "out_scale" is as ever (4 / 2 / 1, else 0).
 *   Sizes.   The output is (w * nx / dx) x (h * ny / dy) (rsr_out_size_xy).  Every entry point that honours a ratio honours the pair:
 *            rsr_process, _many, _tiles, _rows, _group (whose members must agree on both axes), merged concurrent calls, _device, _fmt,
 *            _batch with windows and pitches, _masked and _sequence (whose output rectangles and propagated rectangles are the per-axis
 *            reduced ones).
 *   Errors.  RSR_E_ARG at call time, before anything is launched, unless w * nx and tilesize * nx are multiples of dx, and h * ny and
 *            tilesize * ny are multiples of dy.  No footprint then crosses a tile, and the reduction stays one per-tile launch.  A YUV
 *            output (RSR_FMT_NV12 / RSR_FMT_P010) additionally needs w * nx / dx, tilesize * nx / dx, h * ny / dy and tilesize * ny / dy
 *            EVEN, with "YUV" in rsr_last_error (rsr_out_size_yuv_xy).
 *            720 x 480 at (8/3, 9/4) and tile 192: tile rectangle 512 x 432, output 1920 x 1080.  720 x 576 at (8/3, 15/8) and tile 192:
 *            512 x 360.  1440 x 1080 at (4/3, 1) and tile 198: 264 x 198.  720 x 480 at (8/3, 9/4) and tile 200 is refused (200 * 8 is no
 *            multiple of 3).
 *   The definition, exact.  Steps 1 to 7 of rsr_set_out_ratio, with n, d, L per axis: the horizontal taps and weights (step 2) come from
 *            (nx, Lx = 4 dx), the vertical ones (step 3) from (ny, Ly = 4 dy).  Step 4 reads m = min(V * fp32(1 / (16 dx dy)), 1), the
 *            constant computed in double and rounded once; for dx = dy it is the constant above.  Alpha (step 6) uses the same per-axis
 *            weights.  A YUV output is "Encode" applied to those pixels; the sited chroma filters clamp at the first column of every tile
 *            rectangle (multiples of tilesize * nx / dx) and at its first row (multiples of tilesize * ny / dy). */
int rsr_set_out_ratio_xy(rsr_ctx* ctx, int num_x, int den_x, int num_y, int den_y);
/* Host-only (no GPU): *ow = w * nx / dx, *oh = h * ny / dy for the pair reduced per axis (either pointer may be NULL), or RSR_E_ARG for a
 * pair outside the set above, or when the call-time rule above refuses w, h or tilesize. */
int rsr_out_size_xy(int num_x, int den_x, int num_y, int den_y, int tilesize, int w, int h, int* ow, int* oh);
/* Host-only (no GPU): rsr_out_size_xy for a YUV 4:2:0 OUTPUT: RSR_E_ARG also for an odd w or h, or when one of the four quotients above is
 * odd. */
int rsr_out_size_yuv_xy(int num_x, int den_x, int num_y, int den_y, int tilesize, int w, int h, int* ow, int* oh);

/* A device image behind its own pointer and pitches: a whole tensor, a crop of a larger frame, a frame inside a padded decoder surface, a
 * window of a canvas.  Pitches are in BYTES.  A uint8 row pitch need not be a multiple of the pixel size; for the planar formats both
 * pitches and `data` must be multiples of the element size (2 / 4).  No further alignment is asked of `data`. */
typedef struct rsr_image
{
    void* data;            /* device pointer to element (0,0) [of plane 0; NV12 / P010: Y(0,0)] */
    long long row_pitch;   /* bytes from one row to the next; 0 = tightly packed */
    long long plane_pitch; /* planar formats: bytes from one plane to the next (NV12 / P010: from `data` to the UV plane); 0 = h * row pitch.  Ignored for uint8 HWC */
} rsr_image;

/* n images of ONE geometry (w x h x c, in_fmt -> out_fmt), each with its own pointer and pitches: what a tensor pipeline holds as an
 * (N, 3, H, W) batch, or as views into larger tensors.  Image i receives exactly the bytes rsr_process_device_fmt(in[i] -> out[i]) writes
 * for the same pixels in the context's current mode (default, TTA, "precise", "bgr"; uint8 with c 3 or 4, planar with c == 3); out[i]
 * describes the 4w x 4h result -- (w * out_scale) x (h * out_scale) with option "out_scale" -- and no byte outside that window is touched.
 *   Batching.  The images are cut into groups of as many as one merged tile batch of this geometry takes (option "merge": up to 16 small
 *            images; 1 for a frame that fills the chip by itself, for "merge" = 1 and while profiling is on); every group walks the
 *            network as ONE tile batch, on the plan and workspace the merged host calls of that geometry use -- 16 images of 256 x 256
 *            share 352 launches instead of paying for them 16 times.  n has no upper bound.  n == 1 with packed descriptors enqueues what
 *            rsr_process_device_fmt enqueues.  Stats "batch_calls", "batch_images", "batch_groups".
 *   Stream.  The contract of rsr_process_device: NULL = synchronous on the context's stream; otherwise asynchronous, on `stream` itself
 *            when the context is idle (stat "device_direct"), else on the compute stream ordered around `stream` by events.  No host
 *            waits inside an asynchronous call.  The call forms its own batches: it is never merged with concurrent calls and is safe
 *            next to calls of every kind.
 *   Errors.  All arguments are checked before anything is launched (RSR_E_ARG): n < 1, a null array or data pointer, an unknown format, a
 *            planar format with c != 3, a negative pitch, a row pitch below the bytes of a row (or beyond 2^31 - 1), for planar formats a
 *            pitch or data pointer that is not a multiple of the element size.  When a later group fails (RSR_E_NOMEM, say) the call
 *            returns that error; the groups already enqueued complete.
 *   Overlap between outputs, or between an output and an input, is the caller's responsibility: nothing here looks for it.
 *   Progress callback: one call per tile, tiles_total = the tiles of all n images.
 * Out of scope: images of different sizes in one call, RGBA in planar form, host pointers (rsr_process_many). */
int rsr_process_device_batch(rsr_ctx* ctx, int n, const rsr_image* in, int in_fmt, int w, int h, int c,
                             const rsr_image* out, int out_fmt, void* stream);

/* ---- masked tiles and a device frame diff: run only what changed (no reference counterpart) ----------------------------------------------
 * Decoded video repeats itself: skip blocks, letterbox bars, static backgrounds, screen recordings, held frames are bit-identical to the
 * previous frame over large areas.  Tiles are independent (realsr.cpp:377-380,458-459,490): a tile's output rectangle is a function of its
 * padded source rectangle and of nothing else, so where that rectangle is unchanged the bytes already in the previous output ARE the answer.
 * rsr_diff_tiles finds the tiles whose source changed, on the device; rsr_process_device_masked runs exactly those.
 *
 * Host-only geometry (no GPU).  The tile grid of a w x h image is nx x ny = ceil(w / tilesize) x ceil(h / tilesize); tiles are counted
 * row-major, tile = yi * nx + xi, as rsr_process_tiles counts them.  Either pointer may be NULL.  RSR_E_ARG for w, h or tilesize < 1 or
 * above 2^24. */
int rsr_tile_count(int w, int h, int tilesize, int* nx, int* ny);
/* The SOURCE RECTANGLE of tile (yi, xi), half-open [x0, x1) x [y0, y1):
 *            sx0 = max(xi * T - P, 0),  sx1 = min(min((xi + 1) * T, w) + P, w), and likewise in y  (T = tilesize, P = prepadding).
 * It is the clipped image of what the preprocessing reads: padded pixel gx samples reflect101(xi * T - P + gx), and a reflected index always
 * lands inside the clipped rectangle (an index d <= P outside an edge reflects to d inside it, within the P pixels of halo on that side or,
 * where the tile is narrower than that, onto the clamped last pixel).  Any pointer may be NULL.  RSR_E_ARG for bad sizes (as above), a
 * prepadding that is negative or above 2^24, or a tile outside the grid. */
int rsr_tile_source_rect(int w, int h, int tilesize, int prepadding, int tile, int* x0, int* y0, int* x1, int* y1);

/* Which tiles changed.  a and b are two device images of ONE format and geometry (fmt, w x h x c), each behind its own pointer and pitches as in
 * rsr_process_device_batch; the grid and the rectangles are those of the context's current tilesize and prepadding.  d_mask: DEVICE memory, nx * ny
 * bytes.  mask[t] = 1 if any COMPARED BYTE of tile t's source rectangle differs between a and b, else 0.  Every mask byte is written, 0 as
 * well as 1: the caller does not clear the buffer.  The compared bytes, exactly:
 *   RSR_FMT_U8_HWC                     bytes [sx0 * c, sx1 * c) of rows sy0 .. sy1 - 1.  Alpha is included.
 *   RSR_FMT_F16_CHW / RSR_FMT_F32_CHW  the rectangle's elements in each of the three planes.  Bytes are compared, not values: -0.0 against 0.0
 *                                      counts as changed, a NaN equals itself.  That is conservative.
 *   RSR_FMT_NV12 / RSR_FMT_P010        the Y samples of the rectangle, and the (U, V) pairs of chroma columns
 *                                      max((sx0 >> 1) - 1, 0) .. min(((sx1 - 1) >> 1) + 1, w / 2 - 1) inclusive, rows likewise with sy and h: the
 *                                      decode of every siting reads one chroma sample beyond its own.  P010 compares whole 16-bit words, the low
 *                                      6 bits included.
 *   RSR_FMT_NV16 / RSR_FMT_P210        the Y samples of the rectangle, and the (U, V) pairs of the same chroma columns on rows sy0 .. sy1 - 1
 *                                      ("YUV 4:2:2": a chroma row per luma row).  P210 compares whole words.
 *   RSR_FMT_YUV444P / RSR_FMT_YUV444P10  the samples of the rectangle in each of the three planes, nothing beyond it ("YUV 4:4:4").  YUV444P10
 *                                      compares whole words, the bits above bit 9 included.
 * A tile whose mask byte is 0 would get, from rsr_process_device* on b, the bytes it got from a -- in every mode and at every option that is the
 * same for both calls.
 *   Stream.  Asynchronous on `stream` with the contract of rsr_process_device (NULL = the context's stream, and the call waits).  One memset and
 *            one kernel launch; no host wait inside; the kernel uses none of the context's workspace and is safe next to calls of every kind.
 *   Errors.  RSR_E_ARG before anything is launched, as rsr_process_device_batch checks one image: unknown format, format with c, pitches,
 *            alignment of the planar formats and P010 to their elements, an odd w or h of a YUV surface, a null pointer. */
int rsr_diff_tiles(rsr_ctx* ctx, const rsr_image* a, const rsr_image* b, int fmt, int w, int h, int c, uint8_t* d_mask, void* stream);

/* rsr_process_device_batch with n = 1, restricted to the tiles t with mask[t] != 0.  mask is a HOST array of nmask = nx * ny bytes: the grid
 * size of every launch depends on it, so it is the caller who makes the one round trip (rsr_diff_tiles, a copy, one synchronisation), explicitly.
 * The marked tiles walk the network and exactly their output rectangles are written: no other byte of `out` is touched.  For every written
 * rectangle the bytes are those rsr_process_device_batch writes with n = 1 for the same image in the context's current mode -- every format
 * pair, c 3 and 4, TTA, "precise", "bgr", "out_scale" 4 / 2 / 1 and every output ratio (with their admission checks), the YUV matrices, ranges
 * and sitings, pitched images and windows.
 *   No tile set:    RSR_OK, nothing is launched.
 *   Every tile set: the call IS rsr_process_device_batch with n = 1: the same path, launches and bytes.
 *   Batches.  The tables of the selected tiles are built per call (no plan is cached for a mask) and cut into as many tile batches as the
 *            workspace budget requires ("max_workspace_mb", free device memory).  The slots have the capacity of the FRAME's largest tile,
 *            whatever is selected, so plain and masked calls on one geometry share one workspace layout.  A workspace that cannot be allocated
 *            halves the batches of this call and leaves no bound behind for later calls.
 *   Stream.  The contract of rsr_process_device_batch: on `stream` itself when the context is idle (stat "device_direct"), else on the compute
 *            stream ordered around `stream` by events.  The call forms its own batches and is never merged with concurrent calls.  A host wait
 *            occurs only when all three rotating table buffers still belong to earlier masked calls in flight: the tables travel from pinned
 *            memory with one asynchronous copy on the stream the launches go to, so no other stream is involved, blocking or not.
 *   Progress callback: one call per selected tile.  rsr_profile.tiles counts the slots actually run.
 *   Errors.  RSR_E_ARG before anything is launched: nmask != nx * ny, a null mask, and everything rsr_process_device_batch refuses.
 *   Stats    "masked_calls", "masked_tiles_run", "masked_tiles_skipped" (counted once a call is enqueued, or returns with no tile set: a call that
 *            fails counts nothing), "masked_batches" (the tile batches built for partial masks; a call
 *            with every tile set runs the plain plan and adds none), "masked_table_us" (host time spent building and uploading those
 *            tables, accumulated).  A masked call that launches counts in "batch_calls" too.
 * Out of scope: n > 1, host-pointer images, groups of GPUs, the CLI, merging with concurrent calls. */
int rsr_process_device_masked(rsr_ctx* ctx, const rsr_image* in, int in_fmt, int w, int h, int c, const rsr_image* out, int out_fmt,
                              const uint8_t* mask /* HOST, nmask bytes */, int nmask, void* stream);

/* ---- frame sequences: N video frames share one diff and one tile batch (no reference counterpart) -----------------------------------------
 * A masked call pays its fixed cost -- 352 launches, one host round trip -- per frame, however few tiles changed.  A caller who knows the next
 * N decoded frames (an offline transcode, a player's look-ahead) pays it once per window: one launch diffs every consecutive pair, one round
 * trip brings N masks to the host, the changed tiles of all N frames walk the network as shared tile batches, and one memory-bound launch
 * fills every output rectangle that was not computed from the frame that computed it last.
 *
 * Definitions.  All frames of a call have ONE format and geometry; the tile grid (nx x ny, ntiles = nx * ny, row-major) and a tile's source
 * and output rectangles are those of the masked section above, at the context's current tilesize, prepadding and output ratio.  masks is a
 * row-major [n][ntiles] byte array; any non-zero byte is "set".  The SOURCE of output tile t of frame k is
 *            src[k * ntiles + t] = k                                      where masks[k][t] != 0,
 *                                = the largest j < k with masks[j][t] != 0  otherwise,
 *                                = -1, the previous output,                 where there is no such j.
 * rsr_sequence_sources computes exactly this (host-only, no GPU): the one definition of where every output rectangle comes from.
 * RSR_E_ARG for n < 1, n > RSR_SEQ_MAX, ntiles < 1, a null pointer, or a -1 that would be needed while has_prev == 0. */
#define RSR_SEQ_MAX 16 /* frames per call: the images one tile batch can address */
int rsr_sequence_sources(int n, int ntiles, const uint8_t* masks, int has_prev, int* src /* n * ntiles */);

/* The masks of n consecutive frames.  Row k of d_masks (DEVICE memory, n * nx * ny bytes, every byte written) is what
 * rsr_diff_tiles(frames[k - 1], frames[k]) writes: the same compared bytes, the same tile grid.  Row 0 compares prev with frames[0]; with
 * prev == NULL it is all ones (a first frame, a scene cut).
 *   Stream.  The contract of rsr_diff_tiles.  One memset and ONE kernel launch for all pairs; no host wait inside.
 *   Errors.  RSR_E_ARG before anything is launched: n outside 1 .. RSR_SEQ_MAX, a null pointer (frames, d_masks, any data), and for every
 *            descriptor what rsr_diff_tiles refuses. */
int rsr_diff_tiles_sequence(rsr_ctx* ctx, int n, const rsr_image* frames, const rsr_image* prev /* may be NULL */, int fmt, int w, int h, int c,
                            uint8_t* d_masks /* DEVICE, n * nx * ny */, void* stream);

/* n frames in[k] -> out[k] in one call.  masks (HOST, nmask = n * nx * ny bytes) alone define it -- any bytes, not necessarily a diff; as in
 * the masked call it is the caller who makes the one round trip (rsr_diff_tiles_sequence, a copy, one synchronisation), because the grid of
 * every launch depends on the masks.  With src = rsr_sequence_sources(n, ntiles, masks, prev_out != NULL):
 *   src == k:   tile t of in[k] walks the network; its output rectangle in out[k] receives the bytes rsr_process_device_batch with n = 1 writes
 *               there, in the context's current mode.
 *   otherwise:  the rectangle in out[k] receives the bytes of the same rectangle of out[src], or of prev_out for src == -1.
 * Every byte of every out[k] window is therefore written, and no byte outside a window is touched.
 *   Supported.  Everything the masked call supports: every format pair, NV12 and P010 on either side included; c 3 and 4; TTA, "precise",
 *            "bgr"; "out_scale" 4 / 2 / 1 and every output ratio, with their admission checks; the YUV matrices, ranges and sitings; pitched
 *            images and windows.  The copies move bytes at any alignment: prev_out and the out[k] may sit at different offsets modulo 16, a
 *            uint8 pitch need not be a multiple of 3.
 *   Aliasing.  prev_out may be out[0] itself (the same data and pitches): frame 0 is then updated in place and its source -1 rectangles are
 *            skipped.  That is safe: a tile computed in frame 0 is never anybody's source -1.  Any other overlap between prev_out, the in[k]
 *            and the out[k] is the caller's responsibility.
 *   Ordering.  The changed tiles of all frames, in frame-major order, are cut into tile batches as in the masked call (slots of the frame's
 *            largest tile; a refused workspace halves the batches of this call and leaves no bound behind).  The copies are ONE launch behind
 *            the last tile batch: every source is a computed rectangle or prev_out, so no copy depends on another copy.  With no tile set
 *            anywhere only the copy launch runs; with n == 1 and prev_out == out[0] in addition, nothing is launched.
 *   Stream.  The contract of rsr_process_device_masked, the copy launch included; the tables of the tiles and of the copies travel in the
 *            rotating buffers of the masked calls with the same single asynchronous copy.
 *   Errors.  RSR_E_ARG before anything is launched: n outside 1 .. RSR_SEQ_MAX, nmask != n * nx * ny, a null pointer, prev_out == NULL
 *            while row 0 has a zero byte, a prev_out that fails the checks of an output image, and everything rsr_process_device_batch refuses.
 *   Progress callback: one call per computed tile.
 *   Stats    "seq_calls", "seq_frames", "seq_tiles_run" (computed), "seq_tiles_copied" (tiles whose rectangles the copy launch moved: the
 *            ones skipped in place are not counted), "seq_batches"; counted once the call is enqueued, like the masked stats.  A call that
 *            launches counts in "batch_calls" too.  The "masked_*" stats are not touched.
 * Out of scope: host-pointer images, groups of GPUs, the CLI, merging with concurrent calls, frames of different geometry in one call. */
int rsr_process_device_sequence(rsr_ctx* ctx, int n, const rsr_image* in, int in_fmt, int w, int h, int c, const rsr_image* out, int out_fmt,
                                const rsr_image* prev_out /* may be NULL */, const uint8_t* masks /* HOST, nmask bytes */, int nmask, void* stream);

/* ---- Three-plane YUV frames: yuv420p / yuv422p / yuv444p and their 10-bit forms to surfaces and back (no reference counterpart) ------------
 * Every software decoder -- ffmpeg's default pix_fmt, VapourSynth, libavfilter, YUV4MPEG2 -- emits three planes Y, U, V, each with rows of
 * its own; the chroma planes of the subsampled layouts are smaller than the luma plane, which no rsr_image describes ("YUV 4:4:4" above).
 * No new pixel format is made of them: rsr_pack_planes writes the SURFACE of format `fmt` the engine takes from the three planes of a frame,
 * rsr_unpack_planes the three planes from a surface; two memory-bound launches around the calls that exist.  `fmt` fixes the chroma plane's
 * size and the sample width:
 *            RSR_FMT_NV12 / P010            chroma (w/2) x (h/2), samples of 8 / 16 bits   (yuv420p / yuv420p10le)
 *            RSR_FMT_NV16 / P210            chroma (w/2) x h                               (yuv422p / yuv422p10le)
 *            RSR_FMT_YUV444P / YUV444P10    chroma w x h                                   (yuv444p / yuv444p10le)
 *   The definition, exact.  Y row r of the surface is Y row r of the planes; a subsampled surface has UV[r][2X] = U[r][X], UV[r][2X+1] =
 *            V[r][X]; a 4:4:4 surface has plane 1 = U and plane 2 = V.  8-bit: bytes move unchanged.  P010 / P210, pack: every surface
 *            word is (plane word & 1023) << 6, Y included -- planar 10-bit holds the code in the LOW bits, the surfaces hold code << 6, the
 *            trap of doing this by hand.  P010 / P210, unpack: every plane word is surface word >> 6.  YUV444P10: words are copied verbatim
 *            both ways (both layouts hold the code low).  unpack(pack(p)) == p wherever the planar words are codes (below 1024).
 *   Planes.  y, u, v point at sample (0,0) of each plane, in DEVICE memory here; y_pitch and c_pitch are the bytes from one row to the
 *            next of the Y plane and of the U and the V plane, 0 = tightly packed (w, or the chroma width, samples).
 *   Launch.  The n frames of one geometry go in ONE launch per call, n in 1 .. RSR_SEQ_MAX (the frames one argument block carries); frame i
 *            is src[i] -> dst[i].  Rows go to waves, lanes run along the row; 16-byte accesses where the addresses of a row allow them (a UV
 *            piece of 16 bytes against 8 of U and 8 of V), then 4, then single samples, chosen per row; interleave and shift in registers.
 *   Stream.  The contract of rsr_diff_tiles: asynchronous on `stream` (NULL = the context's stream, and the call waits); no host wait inside;
 *            none of the context's workspace is used, so the call is safe next to calls of every kind.
 *   Errors.  RSR_E_ARG before anything is launched: n outside 1 .. RSR_SEQ_MAX; a null pointer (ctx aside: src, dst, any plane, any data); an
 *            unknown or RGB format; the parity rule of the format (rsr_image_bytes: an odd w of a 4:2:x surface, an odd h at 4:2:0); a plane
 *            pitch below the bytes of a row; a negative pitch; for the 16-bit formats an odd plane pointer or pitch; and everything
 *            rsr_process_device_batch refuses of the rsr_image.
 *   Write discipline.  No byte outside the rows of the destination is written, no byte outside the rows of the source is read: pitched planes
 *            inside a larger canvas and surfaces inside a padded allocation keep their surroundings.
 * Out of scope: 4:1:1 and mono, 12- and 16-bit codes, NV24 / P410 / Y410 / AYUV, planes in host memory. */
typedef struct rsr_planes
{
    void* y; void* u; void* v; /* the three planes of one YUV frame */
    long long y_pitch;         /* bytes from one Y row to the next; 0 = tightly packed */
    long long c_pitch;         /* bytes from one U (and V) row to the next; 0 = tightly packed */
} rsr_planes;
int rsr_pack_planes(rsr_ctx* ctx, int n, const rsr_planes* src, const rsr_image* dst, int fmt, int w, int h, void* stream);
int rsr_unpack_planes(rsr_ctx* ctx, int n, const rsr_image* src, const rsr_planes* dst, int fmt, int w, int h, void* stream);

/* ---- A video session: three-plane frames in HOST memory in, upscaled frames out (no reference counterpart) -----------------------------------
 * What an ffmpeg filter, a VapourSynth plugin or a Y4M pipe holds are frames in host memory; rsr_process* stays uint8 RGB(A).  A session
 * carries such frames through the diff / masked / sequence path above: rsr_video_send takes one frame, every `window` frames run as ONE
 * sequence call, rsr_video_receive hands the results out in order.  fmt is one of the six YUV formats and names the planes' layout as in
 * "Three-plane YUV frames" (NV12 = yuv420p, P010 = yuv420p10le -- the code in the LOW bits --, NV16 / P210 = yuv422p / yuv422p10le, YUV444P /
 * YUV444P10); input and output have the same format; the rsr_planes point into HOST memory.
 *   Open.    RSR_E_ARG for an RGB or unknown format, for a window outside 0 .. RSR_SEQ_MAX, for the parity rule of the input, and for what
 *            rsr_out_size_fmt refuses at the context's output ratio and tile size -- the same message, with "YUV" in it where the parity rule
 *            of the output bites.  window 0 means 8.  The session lowers the window, never below 1, until its device buffers -- window + 1
 *            input and window + 1 output surfaces (the predecessor of a window stays resident) and the planar staging of one window on each
 *            side -- fit half of the device memory that is free at open; RSR_E_NOMEM if a window of 1 does not fit.  rsr_video_info tells
 *            the output size and the window in force (any pointer may be NULL).
 *   States.  send stages a frame (it is copied before send returns); the window-th frame runs the window before send returns, and all its
 *            frames are then ready.  rsr_video_ready: how many receive can hand out now.  send while ready frames remain: RSR_E_STATE;
 *            receive with none ready: RSR_E_STATE.  flush runs what is pending (nothing pending: RSR_OK; ready frames remain:
 *            RSR_E_STATE).  reset (a scene cut, a seek): the next frame is compared with nothing and all its tiles run; RSR_E_STATE while
 *            frames are pending (flush first), frames that are ready stay ready.  close drops pending and ready frames; a session is closed BEFORE its context.  One thread at a
 *            time per session; other calls on the context stay legal between the session's calls.  A change of the context's output
 *            ratio or tile size while a session is open makes the next send (and flush) fail with RSR_E_STATE; every other option
 *            (TTA aside: it is fixed at creation) takes effect for the next window.  Where "precise", "yuv_matrix", "yuv_range",
 *            "yuv_siting" or the prepadding differ from the window before, the window's first frame is compared with nothing and all its
 *            tiles run: no rectangle computed in the old mode is carried over.  After loading another model: rsr_video_reset.  A window
 *            that fails is dropped whole (its copies are waited for), and the next frame is compared with nothing.
 *   A window run.  The uploads (below); one rsr_pack_planes launch; rsr_diff_tiles_sequence against the last input surface of the window
 *            before (all ones after open and reset); the one copy of the masks and the one synchronisation; rsr_process_device_sequence
 *            with prev_out = the last output surface of the window before; one rsr_unpack_planes launch.  The download is receive's.
 *   Host memory.  Pinned planes (rsr_host_alloc, registered memory: all three) are copied to and from the device directly, as rsr_process
 *            copies pinned images; pageable planes go through the session's pinned staging.  Pitches as in rsr_planes, 0 = packed; what
 *            rsr_pack_planes refuses of device planes (null, negative or short pitch, 16-bit: odd pointer or pitch) is RSR_E_ARG here.  No
 *            byte outside the rows of a destination plane is written.
 *   Exactness.  Output frame k is unpack(rsr_process_device_fmt(pack(frame k))) in the context's mode at the time its window runs, byte for
 *            byte: it depends neither on the window size nor on the frames before it.
 *   Stats    "video_frames", "video_windows", "video_tiles_run", "video_tiles_skipped" (counted once a window is enqueued); the sequence
 *            calls count in "seq_*" as ever.
 * Out of scope: RGB or float frames, different formats on the two sides, groups of GPUs, overlap of one window's copies with the next
 * window's compute, interlaced material.  (The CLI runs YUV4MPEG2 streams through one such session: realsr-hip -i in.y4m -o out.y4m.) */
typedef struct rsr_video rsr_video;
int rsr_video_open(rsr_ctx* ctx, int fmt, int w, int h, int window, rsr_video** out);
int rsr_video_send(rsr_video* v, const rsr_planes* host_frame);    /* one frame in */
int rsr_video_ready(rsr_video* v);                                 /* frames receive can hand out now (negative: RSR_E_ARG) */
int rsr_video_receive(rsr_video* v, const rsr_planes* host_frame); /* oldest ready frame out */
int rsr_video_flush(rsr_video* v);                                 /* run the partial window */
int rsr_video_reset(rsr_video* v);                                 /* scene cut / seek: the next frame is compared with nothing */
int rsr_video_info(rsr_video* v, int* ow, int* oh, int* window);
void rsr_video_close(rsr_video* v);

/* Host-only: bytes from `data` to one past the last byte a w x h x c image in `fmt` with these pitches touches (0 = packed, as above: then
 * rsr_image_bytes), or RSR_E_ARG for a combination rsr_process_device_batch refuses. */
long long rsr_image_span(int fmt, int w, int h, int c, long long row_pitch, long long plane_pitch);

/* Host-only: bytes of a w x h x c image in `fmt` (a negative RSR_E_ARG for a bad combination: unknown format, planar or YUV with c != 3,
 * uint8 with c not in {3,4}, w or h < 1, YUV with an odd w or h).  NV12: w*h*3/2, P010: 3*w*h. */
long long rsr_image_bytes(int fmt, int w, int h, int c);

/* Pinned host memory for images.  rsr_process copies pinned buffers (these, hipHostMalloc'd or hipHostRegister'ed
 * memory) to / from the GPU directly; pageable memory goes through the call's pinned staging (the download in chunks,
 * the CPU copy of one chunk under the PCIe transfer of the next).  The reference gets the same from ncnn's Vulkan
 * staging allocator (realsr.cpp:161-167, 208-220). */
void* rsr_host_alloc(size_t bytes);
void rsr_host_free(void* p);

/* Free / total device memory of HIP device `gpuid` in MiB: what ncnn's VulkanDevice::get_heap_budget() is to the
 * reference's automatic tile-size policy (main.cpp:761-774). */
int rsr_device_memory(int gpuid, long long* free_mb, long long* total_mb);

/* The reference prints one line per tile to stderr (realsr.cpp:481).  Here all tiles of a batch run together: `cb` is
 * called once per TILE (tiles_done = 1 .. tiles_total, from the calling thread) when the tile's batch has been enqueued --
 * kernels not necessarily finished; the calls of one batch arrive back to back. */
int rsr_set_progress_callback(rsr_ctx* ctx, void (*cb)(int tiles_done, int tiles_total, void* user), void* user);

/* ---- weights as one relocatable blob (multi-GPU load path) -------------------------------- */
/* The reference re-reads x4.bin once per GPU (main.cpp:784-786).  Here rank 0 parses and packs once,
 * the blob travels by a single RCCL broadcast over xGMI (done by the caller, e.g.
 * torch.distributed.broadcast with backend nccl), and every rank loads it with rsr_load_packed. */

/* Host-only: parse + validate + pack into `dst` (capacity `cap` bytes).  *need receives the blob
 * size (33.5 MB for the 23-block x4.param; 1.44 MB per RRDB block + 0.38 MB for the six other convolutions: 9.0 MB at 6 blocks); call with dst=NULL to query.  The header's
 * conv count, 15 nb + 6, carries the depth; the layout is the same at every depth.  No GPU required. */
int rsr_model_pack(const char* parampath, const char* modelpath, void* dst, size_t cap, size_t* need);

/* Load a blob produced by rsr_model_pack.  `blob` may be a host pointer (is_device=0) or a device
 * pointer on this context's GPU (is_device=1). */
int rsr_load_packed(rsr_ctx* ctx, const void* blob, size_t bytes, int is_device);

/* ---- network interpolation: a strength between two loaded models (no reference counterpart) ---------------------------------------------
 * The reference ships two x4 networks of one architecture, models-DF2K (sharp, keeps compression artefacts) and models-DF2K_JPEG (removes
 * them, softer), and its user picks one with -m.  ESRGAN's own answer to "too sharp / too smooth" is network interpolation,
 * w = (1 - t) w_A + t w_B over the weights of two networks with one graph (Real-ESRGAN's -dn, the denoise strength).  Every model the
 * loader accepts is the one canonical graph, so any two models of one depth can be blended.
 *
 * THE RULE.  A and B are packed blobs (rsr_model_pack) whose header and conv table are BYTE-IDENTICAL -- the conv count and, per
 * convolution, cin / cout / act / nplanes / nt / slope and the three offsets; anything else is RSR_E_GRAPH, rsr_last_error() naming the
 * first convolution and field that differ (or the two depths).  t is an fp32 in [0, 1], u = fp32(1) - t.  The blend C holds
 *   - A's header, A's table and every byte of A outside the segments below (the padding behind a segment);
 *   - for every convolution, every half c of its fp16 weight image, and of the aux image where it has one:
 *         c = fp16_rne((u * float(a)) + (t * float(b)));
 *   - for every fp32 bias:  c = (u * a) + (t * b);
 *   - every operation rounded by itself in fp32, round to nearest even, NO fused multiply-add;
 *   - t == 0 is A's bytes verbatim and t == 1 B's: copies, not arithmetic;
 *   - zero padding stays zero by the arithmetic itself; inf and NaN among the weights get no special treatment (IEEE decides).
 * The blend is of the PACKED halves: a raw-fp32 .bin has been rounded to fp16 by the packing, as for every other use, and the blend
 * rounds once more -- against blending the fp32 sources that is a second rounding, at most one fp16 ulp.
 *
 * rsr_model_blend is the rule in host code (no GPU): check of both blobs (RSR_E_FORMAT), comparison of the tables (RSR_E_GRAPH), then
 * dst = the blend.  *need (may be NULL) receives its size, a_bytes; dst == NULL only reports it; cap < *need, a NULL blob, NaN or a t
 * outside [0, 1] are RSR_E_ARG.  dst must not overlap a or b.  The result loads with rsr_load_packed and serves rsr_create_group users
 * through a model of their own making. */
int rsr_model_blend(const void* a, size_t a_bytes, const void* b, size_t b_bytes, float t, void* dst, size_t cap, size_t* need);

/* On the device: a context takes a SECOND model beside the one it has loaded and then holds three blobs -- A, B and the active one the
 * kernels read, which starts as a device-to-device copy of A (strength 0).  A context without a second model holds one blob, as ever.
 * rsr_load_second / rsr_load_second_packed: RSR_E_STATE before a first model is loaded; everything is validated (and every allocation
 * made: RSR_E_NOMEM) before the context changes, so a failed call leaves it as it was.  Loading another second model keeps the strength
 * and blends again; rsr_load / rsr_load_packed of a new FIRST model drop the second and set the strength to 0.
 * rsr_set_blend: RSR_E_STATE without a second model, RSR_E_ARG for NaN or a t outside [0, 1].  The contract of rsr_load: it waits for
 * the context's stream, must not run concurrently with processing calls on this context nor under stream capture, and returns when the
 * active blob is complete (one kernel launch over all segments; a copy at 0 and 1).  The model has then changed hands as behind a
 * load: the self-check's report and ranges, a `precise` that option "precise_auto" switched on and the per-convolution times are
 * dropped (under "precise_auto" the self-check runs again on the blended model); plans and workspace stay.
 * Stats "blend" (the fp32 strength) and "second_loaded".  rsr_process_group: the members must agree on both (the strength by its bits),
 * RSR_E_ARG before any launch otherwise; rsr_create_group takes no pair -- load the second model per member, or make the group's model
 * with rsr_model_blend / rsr_model_export. */
int rsr_load_second(rsr_ctx* ctx, const char* parampath, const char* modelpath);
int rsr_load_second_packed(rsr_ctx* ctx, const void* blob, size_t bytes, int is_device);
int rsr_set_blend(rsr_ctx* ctx, float t);

/* The active blob -> host memory: for a plainly loaded context the bytes of rsr_model_pack, behind rsr_set_blend the bytes of
 * rsr_model_blend.  Keeps a chosen blend for a later rsr_load_packed.  *need (may be NULL) receives the size; dst == NULL only reports
 * it.  RSR_E_STATE before a load, RSR_E_ARG when cap is too small.  Waits for the context's stream. */
int rsr_model_export(rsr_ctx* ctx, void* dst, size_t cap, size_t* need);

/* ---- several GPUs of one node ------------------------------------------------ */
/* What main.cpp:778-791 does per GPU (construct, load), for n GPUs at once: the model is parsed and packed once, uploaded to
 * gpuids[0] and broadcast to the other devices with ONE RCCL collective over xGMI (librccl is dlopen'ed; when it is not
 * available the blob is uploaded to every device from the host instead -- rsr_group_transport() tells which).  out[0..n-1]
 * receive the contexts (all NULL on failure).  Images are then dealt to the contexts by the caller's work queue
 * (main.cpp:811-828), or ONE large image is split with rsr_process_group. */
int rsr_create_group(rsr_ctx** out, const int* gpuids, int n, int tta_mode, const char* parampath, const char* modelpath);
const char* rsr_group_transport(void); /* "rccl" | "host ..." for the calling thread's last rsr_create_group */
/* With RSR_GROUP_FORCE_RCCL=1 in the environment rsr_create_group takes the RCCL branch also for n == 1 (a communicator of one
 * rank, an in-place broadcast, the model loaded from the device copy): the whole collective path can be exercised on a
 * single-GPU machine.  rsr_rccl_probe is host-only (no GPU, no communicator): 0 when librccl can be dlopen'ed and exports every
 * entry point that branch calls (ncclCommInitAll, ncclCommDestroy, ncclGroupStart, ncclGroupEnd, ncclBroadcast,
 * ncclGetErrorString), RSR_E_DEVICE + rsr_last_error() otherwise.  Reference semantics: one RealSR + one load per GPU id,
 * /root/reference/src/main.cpp:778-791. */
int rsr_rccl_probe(void);

/* RealSR::process restricted to the tiles [tile_begin, tile_end) of the image's tile grid, counted row-major (tile (yi, xi) =
 * yi * ceil(w / tilesize) + xi; tiles are independent: realsr.cpp:377-380,458-459,490).  `in` is the whole image, `out` the
 * whole (4w x 4h x c) output -- (w * out_scale) x (h * out_scale) x c with option "out_scale" --; only the output rectangles
 * of those tiles are written.  Disjoint ranges may run concurrently on different contexts into the same `out`.  rsr_process_rows: the same for whole tile rows [tile_row_begin, tile_row_end). */
int rsr_process_tiles(rsr_ctx* ctx, const uint8_t* in, int w, int h, int c, uint8_t* out, int tile_begin, int tile_end);
int rsr_process_rows(rsr_ctx* ctx, const uint8_t* in, int w, int h, int c, uint8_t* out, int tile_row_begin, int tile_row_end);

/* One image over n contexts (normally one per GPU): the TILES are dealt in contiguous row-major ranges of equal padded-pixel
 * load (within one tile; a 1080p frame at tile 200 = 60 tiles = 7-8 per GPU on 8 GPUs), every context runs its range on its
 * own thread and fetches the rectangles of its tiles into `out`; the call returns when `out` is complete.  All contexts must
 * carry the same tilesize / prepadding / scale / out_scale / tta (checked: RSR_E_ARG otherwise); `out` is
 * (w * out_scale) x (h * out_scale) x c. */
int rsr_process_group(rsr_ctx* const* ctx, int n, const uint8_t* in, int w, int h, int c, uint8_t* out);
/* (rsr_process_group keeps its worker threads between calls: a process that has called it must not dlclose() the library.) */

/* Host-only (no GPU): the tile ranges rsr_process_group deals to `parts` shares of a w x h image: share i runs the tiles
 * [bounds[i], bounds[i+1]) of the row-major grid; bounds has parts + 1 entries.  Balanced by padded tile area to within one
 * tile.  Returns the number of shares used (min(parts, number of tiles)) or a negative RSR_E_*. */
int rsr_tile_partition(int w, int h, int tilesize, int prepadding, int parts, int* bounds);

/* Host-only model introspection (no GPU): conv count, weight/bias counts and the .bin encoding
 * (1 = fp16-tagged, 0 = raw fp32, 2 = mixed/table).  Any pointer may be NULL. */
int rsr_model_info(const char* parampath, const char* modelpath, int* n_layers, int* n_convs,
                   long long* n_weights, long long* n_biases, int* bin_encoding);

/* ---- the four shader-equivalent kernels, callable alone (bit-exact parity tests) ----------- */
/* Arguments mirror the shaders' push constants; all pointers are HOST pointers, the call copies
 * in, runs the HIP kernel, copies out, synchronises.
 *
 * rsr_preproc:  realsr_preproc.comp:47-95 / dispatch realsr.cpp:372-415
 *   band  u8 HWC (w x h x channels) -> top: planar fp16 [3][outh][outw] (cstep = outw*outh),
 *   alpha: fp16 [alphah][alphaw] un-normalised (only when channels == 4, may be NULL otherwise).
 * rsr_preproc_tta: realsr_preproc_tta.comp:54-113; top[0..3] are outw x outh, top[4..7] outh x outw. */
int rsr_preproc(rsr_ctx* ctx, const uint8_t* band, int w, int h, int channels, uint16_t* top, int outw,
                int outh, int pad_top, int pad_left, int crop_x, int crop_y, uint16_t* alpha, int alphaw,
                int alphah);
int rsr_preproc_tta(rsr_ctx* ctx, const uint8_t* band, int w, int h, int channels, uint16_t* const top[8],
                    int outw, int outh, int pad_top, int pad_left, int crop_x, int crop_y);

/* rsr_postproc: realsr_postproc.comp:47-89 / dispatch realsr.cpp:444-472
 *   bottom planar fp16 [3][h][w] -> top u8 HWC band (outw x outh x channels), written in place
 *   for gx < gx_max at column offset offset_x (the band is copied in first, so untouched pixels
 *   keep their value).  alpha (channels==4): fp16 [alphah][alphaw], 0..255 units.
 * rsr_postproc_tta: realsr_postproc_tta.comp:54-110. */
int rsr_postproc(rsr_ctx* ctx, const uint16_t* bottom, int w, int h, const uint16_t* alpha, int alphaw,
                 int alphah, uint8_t* top, int outw, int outh, int offset_x, int gx_max, int crop_x, int crop_y,
                 int channels);
int rsr_postproc_tta(rsr_ctx* ctx, const uint16_t* const bottom[8], int w, int h, uint8_t* top, int outw,
                     int outh, int offset_x, int gx_max, int crop_x, int crop_y, int channels);

/* ---- network on one tile (layer-level parity; replaces ncnn::Extractor input/extract,
 *      realsr.cpp:420-428) -------------------------------------------------------------------- */
/* in: planar fp16 [3][h][w] in [0,1]; out: planar fp16 [3][4h][4w].  Host pointers. */
int rsr_net_forward(rsr_ctx* ctx, const uint16_t* in, int w, int h, uint16_t* out);

/* The same with the network's result in fp32 (planar [3][4h][4w]), as conv_last leaves it in precise mode (option "precise" = 1;
 * RSR_E_STATE otherwise): what the uint8 conversion sees there.  rsr_net_forward in precise mode returns this blob rounded to fp16. */
int rsr_net_forward_f32(rsr_ctx* ctx, const uint16_t* in, int w, int h, float* out);

/* One 3x3/s1/p1 convolution through the MFMA kernel with caller-supplied weights (layer-level parity;
 * the arithmetic ncnn::Convolution [+ Interp nearest x2 in front when upsample2x] performs for each
 * Convolution line of x4.param).  in: planar fp16 [cin][h][w]; weight: fp32 OIHW [cout][cin][3][3]
 * (rounded to fp16 by the packer); bias fp32 [cout]; cout <= 64; out: planar fp16 [cout][H][W],
 * H,W = h,w (or 2h,2w).  Host pointers. */
int rsr_conv3x3(rsr_ctx* ctx, const uint16_t* in, int cin, int h, int w, int upsample2x, const float* weight,
                const float* bias, int cout, int lrelu, uint16_t* out);

/* The residual epilogues of the graph on one convolution (what Eltwise / BinaryOp do behind a Convolution in x4.param):
 *   v = s1*(conv + b)  [+ in[0:cout] when own_input_residual: RDB conv5, x4.param:17-18]
 *   [v = s2*v + res when own_input_residual and res: every third RDB, x4.param:47]
 *   [v = v + res when !own_input_residual and res: trunk_conv + global skip, x4.param:994-995]
 * res: planar fp16 [cout][h][w] or NULL; cout 32 or 64; no upsampling, no activation.  Host pointers. */
int rsr_conv3x3_res(rsr_ctx* ctx, const uint16_t* in, int cin, int h, int w, const float* weight, const float* bias, int cout,
                    float s1, int own_input_residual, const uint16_t* res, float s2, uint16_t* out);

/* The same residual forms as the engine runs them in precise mode (option "precise"; 64 output channels): every tensor of the
 * residual stream is hi + lo / 2048 -- hi = fp16(v) as ever, lo = the rounding residue (v - hi) * 2048 as ONE byte (bf8 / e5m2: the
 * upper byte of an IEEE fp16); the adds are done in fp32 and rounded once.  in_lo: lo of in[0:64] (own_input_residual only),
 * res_lo: lo of res, out_lo: receives the lo of the result; any of the three may be NULL (= zero / not wanted).  Planar [64][h][w],
 * hi blobs fp16, lo blobs bytes. */
int rsr_conv3x3_res_precise(rsr_ctx* ctx, const uint16_t* in, const uint8_t* in_lo, int cin, int h, int w, const float* weight,
                            const float* bias, float s1, int own_input_residual, const uint16_t* res, const uint8_t* res_lo, float s2,
                            uint16_t* out, uint8_t* out_lo);

/* ---- model self-check (no reference counterpart) ----------------------------------------------------------------------- */
/* Every feature map is stored as fp16, like the reference's GPU path (realsr.cpp:44-46); the bar is the reference's fp32 CPU path
 * (realsr.cpp:525-838), +-1 per uint8.  Whether fp16 storage holds it depends on the weights.  rsr_selfcheck answers, on the
 * device and in a few milliseconds: do the activations of the loaded model fit fp16, and how far does fp16 storage put the output
 * from the fp32 result?  One tile walks the network in fp16 storage (a reduction behind every convolution reads what it stored) and
 * again in precise mode (option "precise"); the two outputs are compared on the device.  storage_err = max |default - precise|
 * estimates the default mode's true error e16 against fp32: e16 - eP <= storage_err <= e16 + eP with eP, precise mode's own error,
 * about a third of e16 (profiles/selfcheck.txt has the estimate measured against the fp32 oracle). */
typedef struct rsr_selfcheck_report
{
    int tile_w, tile_h;     /* the tile the check ran on */
    float storage_err;      /* max |default - precise| of the network output before quantisation, [0,1] units */
    float headroom;         /* (1/255) / storage_err  (FLT_MAX when storage_err == 0) */
    int max_byte_diff;      /* max |q(default) - q(precise)|, q = the engine's uint8 conversion */
    long long bytes_differ; /* output elements where q differs; of 3 * 16 * tile_w * tile_h */
    float peak_abs;         /* largest finite |value| any convolution stored, default mode */
    int peak_conv;          /* its index in x4.param order (0..350) */
    long long nonfinite;    /* stored values that are inf / NaN, all convolutions, default mode */
    int fp16_overflow;      /* nonfinite > 0 || peak_abs >= 65504 */
    int recommend_precise;  /* headroom < 1.5 */
    float elapsed_ms;       /* wall time of the check */
} rsr_selfcheck_report;

/* tile: planar fp16 [3][h][w] in [0,1] (host), or NULL = the built-in tile at w x h (w = h = 0: 148 x 148, the padded tile of a
 * 256 x 256 image at tile 128).  RSR_E_STATE before load.  Works in either mode and leaves the context in the mode, with the plans
 * and the output bytes it had; waits for the calls in flight on the context.  fp16_overflow is reported, not an error. */
int rsr_selfcheck(rsr_ctx* ctx, const uint16_t* tile, int w, int h, rsr_selfcheck_report* out);
/* Host-only (no GPU): the built-in tile, planar fp16 [3][h][w]: flat areas, ramps, hard edges and fine texture over 0 .. 1, every
 * value k / 255 as the preprocessing produces it.  Integer arithmetic only: the same bytes everywhere. */
int rsr_selfcheck_tile(uint16_t* dst, int w, int h);
/* Per convolution (x4.param order) of the context's last rsr_selfcheck: the largest finite |value| it stored and the number of
 * inf / NaN it stored; either pointer may be NULL.  n: entries of the caller's arrays, 0 .. 15 RSR_MAX_RRDB + 6 = 966 (else RSR_E_ARG);
 * entries [0, min(n, model_convs)) are written and the rest of the n are zeroed (351 convolutions at 23 blocks: stat "model_convs").
 * RSR_E_STATE when no self-check has run since the model was loaded. */
int rsr_selfcheck_ranges(rsr_ctx* ctx, float* peak, long long* nonfinite, int n);

/* ---- measurement ------------------------------------------------------------------------- */
typedef struct rsr_profile
{
    double conv_ms;        /* summed HIP-event time of the conv3x3 MFMA kernel launches */
    double conv_flops;     /* algorithmic FLOPs of those launches: 2*9*Cin*Cout*H*W per tile (true Cin/Cout) */
    long long conv_launches;
    double pre_ms, post_ms; /* preproc / postproc kernels */
    double pre_bytes, post_bytes;
    double total_ms;       /* first launch -> last launch of the profiled rsr_process* calls */
    long long tiles;       /* network tile evaluations (x8 under TTA) */
    long long calls;
} rsr_profile;

/* enable=1: every kernel launch is bracketed by hipEvents on the launch stream; accumulate until
 * rsr_get_profile(reset=1).  The events add ~1 us per launch. */
int rsr_set_profiling(rsr_ctx* ctx, int enable);
int rsr_get_profile(rsr_ctx* ctx, rsr_profile* out, int reset);

/* Accumulated HIP-event time per convolution of x4.param (index = order in the file; stat "model_convs" entries, 351 at 23 blocks),
 * over the profiled calls since the last reset or load.  n as in rsr_selfcheck_ranges: 0 .. 966, entries beyond the model's zeroed. */
int rsr_get_conv_times(rsr_ctx* ctx, double* ms, int n, int reset);

/* Profiling aid: after rsr_set_option("trace_conv", i) the launch of convolution i records, for workgroup 0 /
 * MFMA wave 0, the s_memtime stamps (arrival at, release from) every stage barrier in out[0..1023]; builds with
 * -DRSR_EXP_OVLTRACE add per-stage epilogue stamps at out[1024 + 8*stage ..]; n <= 8192 values. */
int rsr_get_trace(rsr_ctx* ctx, unsigned long long* out, int n);

/* Engine knobs (optional).  key/value:
 *   "max_workspace_mb"  tile-batch memory budget (default 65536).  The effective budget is additionally bounded by 90 % of the
 *                       device memory that is actually free when a plan is built, and a batch whose workspace cannot be
 *                       allocated is halved and re-planned (down to one tile) before RSR_E_NOMEM is reported
 *   "flow_flags"        bit 0 = 64-output-channel convs with 4 MFMA waves x 64 channels instead of 8 x 32,
 *                       bit 1 = no deferred epilogue for the 32-output-channel convs, bit 2 = weights re-streamed from L2 for every
 *                       block even where a conv's weight images fit in LDS for the whole launch (default: resident where they fit),
 *                       bit 3 = conv_last (64 -> 3) through the generic 32-output-channel path instead of the variant that puts
 *                       (dy, cout) into the MFMA's M dimension (half the matrix work; same arithmetic, other summation order)
 *   "trim"              1 [default]: blocks / rows of the convs behind the trunk whose output only feeds cropped (halo) pixels of
 *                       the tile are not computed (dead-output elimination, engine.cpp: tail_margin; output bytes unchanged);
 *                       0: every padded-tile pixel is computed at every layer
 *   "tail_group"        slots (tiles; x8 under TTA) per launch group of the 2x / 4x convs (default 0 = the whole batch at once).  Small
 *                       groups keep the 4x intermediates in the Infinity Cache between upconv2 -> HRconv -> conv_last; measured
 *                       worth <= 1.5 % of those launches on MI355X and a loss at the 2x level, hence off
 *   "precise"           1: the 64-channel residual stream of the network is kept as THREE bytes per element (the fp16 the convs read +
 *                       one byte of its rounding residue) and conv_last's fp32 result is converted to uint8 without an fp16 blob in
 *                       between: half the distance to the reference's fp32 CPU path (realsr.cpp:525-838) that fp16 storage -- the
 *                       reference's own GPU path, realsr.cpp:44-46, and this engine's default (0) -- has; costs ~6 % more workspace
 *                       and the extra traffic of the residue planes in 71 of the 351 convolutions
 *   "out_scale"         4 [default]: the output is the network's x4 image.  2 / 1: that image box-reduced on the device, 2 x 2 / 4 x 4, to
 *                       (2w) x (2h) / w x h -- 1080p -> 2160p, or a restoration model (models-DF2K_JPEG) at the image's own size -- without
 *                       the x4 image ever leaving the library.  Any other value: RSR_E_ARG, the value in force stays (stat "out_scale").
 *                       Takes effect for the next call, like "precise"; every rsr_process* entry point honours it, and wherever a
 *                       comment below says "4w x 4h" read "(w * out_scale) x (h * out_scale)".  rsr_set_params is not concerned: its
 *                       `scale` stays the network's 4.  rsr_image_bytes / rsr_image_span take the image's own w and h.  Definition,
 *                       bit for bit, for output pixel (X, Y), channel q, k = 4 / out_scale:
 *                         1. c(x, y) = min(max(r(x, y), 0), 1), r the fp32 value the uint8 conversion sees at x4 pixel (x, y) in the
 *                            context's current mode (rsr_process_device_fmt, "Output": what RSR_FMT_F32_CHW holds at out_scale 4;
 *                            under TTA the eight variants are merged first, (v0 + ... + v7) * 0.125f)
 *                         2. d = the fp32 mean of c over x in [kX, kX + k), y in [kY, kY + k), in this order (c_yx):
 *                            k = 2: ((c00 + c01) + (c10 + c11)) * 0.25f;  k = 4: s_j = ((c_j0 + c_j1) + (c_j2 + c_j3)), then
 *                            ((s0 + s1) + (s2 + s3)) * 0.0625f.  Plain fp32 adds, one multiplication by a power of two
 *                         3. RSR_FMT_F32_CHW stores d, RSR_FMT_F16_CHW d rounded once to fp16, RSR_FMT_U8_HWC floor(d * 255 + 0.5)
 *                            clamped to 0 .. 255 (the conversion of the x4 path)
 *                         4. alpha (uint8, c == 4): the bicubic x4 alpha value of the x4 path, clamped to [0, 255], averaged over the
 *                            box in the same order and stored as floor(mean + 0.5)
 *                         5. "bgr" swaps channels 0 and 2 on store as ever; "precise" changes only what r is.
 *                       The clamp comes BEFORE the mean (the mean of the x4 image one would have got, not of the raw network output);
 *                       a box never crosses a tile.  Below 4, conv_last leaves its planar blob and one more small launch
 *                       (postproc_tiles_box) writes the image: the route RGBA and TTA take anyway.  Other scales (3, 3/2, 4/3 ...):
                       rsr_set_out_ratio; setting "out_scale" leaves such a ratio again
 *   "yuv_matrix"        709 [default], 601 or 2020: Kr / Kb of the RSR_FMT_NV12 / RSR_FMT_P010 conversion; "yuv_range": 0 [default] = limited (16..235 /
 *                       16..240 at 8 bits), 1 = full.  Any other value: RSR_E_ARG, the value in force stays (stats "yuv_matrix", "yuv_range").
 *                       Both take effect for the next call, like "out_scale" (rsr_process_device_fmt has the definition)
 *   "yuv_siting"        0 [default] = centre, 1 = left, 2 = top-left: where a chroma sample of an RSR_FMT_NV12 / RSR_FMT_P010 surface sits, on the
 *                       input and the output side alike ("Chroma siting" above); takes effect for the next call.  Any other value: RSR_E_ARG,
 *                       the value in force stays (stat "yuv_siting").  RGB formats, host pointers and the CLI are not concerned.
 *   "alpha_net"         0 [default]: the alpha of an RGBA image is ncnn's bicubic x4.  1: it walks the network as a gray image, a second
 *                       pass over the call's tiles at about twice the frame time ("alpha through the network" above has the exact rule);
 *                       c == 3 calls are not concerned.  Takes effect for the next call.  Any other value: RSR_E_ARG, the value in force
 *                       stays (stat "alpha_net"; stat "alpha_tiles": tiles run through the alpha pass since creation)
 *   "alpha_adaptive"    0 [default]: under "alpha_net" 1 every tile of an RGBA call runs the alpha pass.  1: a tile whose source rectangle
 *                       holds one alpha value skips it and keeps the bytes of "alpha_net" 0 ("alpha_adaptive" above has the exact rule) --
 *                       at the price of ONE HOST WAIT PER TILE BATCH, also in asynchronous calls; no such call under stream capture.
 *                       Ignored with "alpha_net" 0 and for c == 3.  Takes effect for the next call.  Any other value: RSR_E_ARG, the value
 *                       in force stays (stats "alpha_adaptive", "alpha_tiles_flat", "alpha_wait_us")
 *   "dither"            0 [default]: every integer sample is rounded to the nearest code.  1: every colour sample of every integer output
 *                       format (U8 / U16 RGB(A), the Y / U / V codes of the YUV formats) is rounded against a threshold keyed to its place in
 *                       the output image ("dither" above has the exact rule); alpha and the float formats are not touched.  A U8 RGB call
 *                       then leaves conv_last's fused store for one post launch.  Takes effect for the next call.  Any other value:
 *                       RSR_E_ARG, the value in force stays (stat "dither")
 *   "precise_auto"      1: "precise" is set by the model: on a loaded context rsr_selfcheck runs at once on the built-in tile and "precise"
 *                       becomes its recommend_precise; on a context not yet loaded the same happens at the end of the next successful
 *                       rsr_load / rsr_load_packed (which then returns the self-check's error, if it has one; the model stays loaded).
 *                       0 [default]: off, "precise" stays where it is.  A later explicit "precise" still wins
 *   "merge"             small images of concurrent rsr_process / synchronous rsr_process_device calls walk the network as ONE tile batch, up
 *                       to this many per batch (default 16 = the most; 1 = off: the calls queue up on the compute stream).  An image is
 *                       small when its tiles are fewer than a quarter of "merge_target_items" (default 4096) 16 x 32 blocks -- 256 x 256
 *                       at tile 128 is 200; a 1080p frame, 5,900, fills the chip by itself.  The images of a batch may differ in
 *                       size ("merge_mixed" 0: only images of one size share a batch).  Output bytes unchanged
 *   "bgr"               1: the caller's images are BGR(A) (the reference's Windows build: WIC decodes to BGR, realsr.cpp:188-206,
 *                       497-515, realsr_preproc.comp:17-21); the network always sees RGB.  Default 0 = RGB(A)
 *   "max_lanes"         rsr_process calls in flight per context (default 16: small images of concurrent calls are merged, the more in
 *                       flight the fuller the launches); "chunk_mb": download chunk for pageable
 *                       destinations (default 16); "copy_threads": CPU threads per staging copy of a pageable image
 *                       (default 4; 1 = the calling thread alone)
 *   "num_cu"            persistent grid size (profiling aid)
 *   "test_repeat"       rsr_conv3x3 / rsr_conv3x3_res: the work items N times in ONE launch (an L2-resident workload; stat "last_test_us")
 *   "ws_clamp_mb"       test hook: plant the workspace bound a failed allocation leaves behind (< 0 clears it; see rsr_get_stat)
 *   "ws_fail_above_mb"  test hook: workspaces above this size fail to allocate, every time (a persistently fragmented device; < 0 off);
 *                       stat "ws_failures" counts the refusals, "clamp_backoff" the calls between two attempts at the full size
 *   "ws_poison"         test hook: 0 [default] = off; 0x10000 + p = every workspace set-up of a call first fills EVERY byte of every workspace
 *                       buffer with the 16-bit pattern p, then zeroes exactly what a change of slot capacity inside an existing
 *                       allocation zeroes (the 64-byte plane guards of the new layout over the whole allocation, and the input
 *                       buffer IN) and nothing more: the worst history a workspace can have in production.  No output may depend
 *                       on it (tests/test_gpu_ws_hygiene.py: 0xFFFF = NaN in every storage type, 0x7BFF = 65504).  Off: the calls
 *                       made are exactly those without the hook
 *   "test_redzone"      test hook: bytes (a multiple of 256; 0 [default] = off).  rsr_conv3x3 / rsr_conv3x3_res / rsr_conv3x3_res_precise place
 *                       their input, residual and output buffers between two red zones of that size, filled -- like the whole output
 *                       buffer, in place of zeros -- with the "ws_poison" pattern (0xFFFF without one); stat "test_redzone_dirty" is the
 *                       number of red-zone bytes the last such launch changed (-1: it had none)
 *   "trace_conv"        conv index whose launch records s_memtime stamps (rsr_get_trace; -DRSR_EXPERIMENT -DRSR_FLOW_TRACE builds), -1 off
 *   "alternate_order"   1 [default]: every second conv walks its work items backwards (starts on the tiles the previous conv
 *                       touched last -> Infinity Cache hits); 0: always forwards
 *   "xcd_order"         1 [default]: the backward tables of "alternate_order" are reversed inside each XCD's share of the list, so an XCD
 *                       starts on the blocks IT wrote last (its own 4 MB L2); 0: the list is reversed as a whole
 *   "fold"              1 [default]: a tile's last block column, when it is only 1..14 pixels wide, is computed by FOLDED work items
 *                       (two block rows of that narrow column per 16 x 32 block: C3's 420-wide tiles 13.5 instead of 14 block
 *                       columns); 0: one plain block column more.  Output bytes unchanged (kernels.h: kFoldBit)
 *   "dbg"               A-B bits of ConvArgs::dbg, profiling only (bits 1 / 4 / 64 / 128 act only in -DRSR_EXPERIMENT builds of conv_flow.hip):
 *                         1 skip LDS-DMA (64: weights only, 128: patches only), 4 skip epilogue stores, 32 MFMA waves do not skip rows
 *                         outside the tile / inside the unread frame, 8192 conv_last never writes the uint8 image itself, 16384 no split tail for early download,
 *                         32768 / 65536 force the one-thread-per-pixel / the LDS-staged pre and post kernels (default: chosen per launch) */
int rsr_set_option(rsr_ctx* ctx, const char* key, long long value);

/* Engine state, read-only (tests and measurement scripts; no reference counterpart).  key:
 *   "plan_batches" / "plan_slots_per_batch"  tile batches / slots per batch of the most recently used plan (a 4K frame at tile 400
 *                       fits ONE batch of 60 slots under the default 64 GiB budget; max_workspace_mb splits it), "plans" cached plans
 *   "plan_items_lr" / "plan_items_2x" / "plan_items_4x"  work items (16 x 32 pixel blocks) of that plan per resolution level and image: what the
 *                       conv launches of a frame actually walk (blocks that only feed cropped pixels are left out, narrow last columns folded)
 *   "merged_batches" / "merged_images" / "merged_widest" / "merged_mixed"  tile batches that merged small images of concurrent calls, the
 *                       images they carried, the widest one, those whose images differed in size; "device_direct": rsr_process_device[_fmt | _batch] calls that ran on the caller's own stream
 *   "batch_calls" / "batch_images" / "batch_groups"  rsr_process_device_batch calls, the images they enqueued and the tile batches those went in (the merged_* stats count the cross-call combiner alone)
 *   "workspace_mb"      device memory the workspace holds, "ws_clamp_mb" the bound a failed allocation left behind (-1 = none)
 *   "ws_guard_dirty"    test hook: waits for the context's streams and counts, on the host, the non-zero bytes among (a) the 64-byte guard in
 *                       front of every plane of the current workspace layout, over the whole allocation of every guarded buffer, and
 *                       (b) channels 3 .. 31 of the input buffer IN.  Both are invariants every convolution's zero padding rests on --
 *                       no kernel ever writes either -- and the count is 0 after every call (tests/test_gpu_ws_hygiene.py).  -1 while the
 *                       workspace has no layout (before the first call, after rsr_selfcheck)
 *   "lanes", "lane_in_mb", "lane_out_mb"   rsr_process lanes created so far and the device image buffers they hold (a member of
 *                       rsr_process_group allocates only the output rows of its tile range)
 *   "last_test_us"      HIP-event time of the last rsr_conv3x3 / rsr_conv3x3_res launch (with option "test_repeat" = N the
 *                       work items are repeated N times in that one launch: an L2-resident workload)
 *   "precise_active"    0 / 1: the storage mode the next call runs in (option "precise", whoever set it); "out_scale": the output scale in force (0: a ratio other than 4 / 2 / 1, "out_num" / "out_den": rsr_set_out_ratio; 0 / 0 while the axes differ, "out_num_x" / "out_den_x" / "out_num_y" / "out_den_y": rsr_set_out_ratio_xy); "yuv_matrix" / "yuv_range" / "yuv_siting": likewise
 *   "selfcheck_runs"    self-checks run on the context; of the last one: "selfcheck_headroom", "selfcheck_peak_abs", "selfcheck_ms",
 *                       "selfcheck_overflow" (-1 before the first run)
 *   "model_blocks" / "model_convs"  RRDB blocks and convolutions (15 blocks + 6) of the loaded model; 0 before a load
 *   "second_loaded" / "blend"       0 / 1: a second model is loaded (rsr_load_second); the strength of rsr_set_blend, the fp32 value exactly;
 *                       "blend_us": HIP-event time of the last rsr_set_blend's one launch (or copy), taken while rsr_set_profiling is on, else -1 */
int rsr_get_stat(rsr_ctx* ctx, const char* key, double* value);

const char* rsr_last_error(const rsr_ctx* ctx); /* ctx may be NULL: last global (create/pack) error */
const char* rsr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* REALSR_HIP_H */
