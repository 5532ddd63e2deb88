// kernels.h -- launch interface of the gfx950 kernels (kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rsr {

// ---- activation storage ("planes") -----------------------------------------------------------
// Every feature tensor lives in HBM as a set of 16-channel planes: plane = [guard 64 B | [H][W][16] fp16]
// (32 B per pixel, pixels row-major, no border).  A 64-channel tensor = 4 planes, the 192-channel
// dense-block working set = 12 planes.  Tiles of one batch occupy "slots" at a fixed stride.
//
// Work decomposition of the conv kernel: one workgroup computes a 16-row x 32-column block of output
// pixels for all output channels; work items (slot, y0, x0) come from a device table.

constexpr int kBlkH = 16, kBlkW = 32;          // output block of one workgroup
constexpr int kPatchH = kBlkH + 2, kPatchW = kBlkW + 2;
constexpr int kPatchPx = kPatchH * kPatchW;     // 612
constexpr int kGuard = 64;                      // zero bytes in front of every conv-input plane (LDS-DMA source for padding)
constexpr int kPlaneCh = 16;                    // channels per plane

// FOLDED blocks.  A tile whose width leaves a remainder of 1..kFoldMaxW columns behind its last full 32-column block would spend a
// whole block (32-pixel MFMA rows) on those few columns: C3's 420-wide tiles 14 block columns for 13.1, +6.7 % executed matrix
// work.  Such a last column is covered by folded work items instead: ONE block = that column over TWO block rows (rows y0..y0+15
// in lanes / patch columns 0..15, rows y0+16..y0+31 in 16..31).  The matrix loop is unchanged -- lanes never look across pixels --
// only the loaders' gather and the epilogue's scatter know (conv_flow.hip).  WorkItem::x0 carries the flag in bit 30.
constexpr int kFoldBit = 1 << 30;
constexpr int kFoldMaxW = 14; // strip = left halo + <= 14 pixels + right halo = 16 patch columns

// MERGED batches: the tiles of up to kMaxMerge small images of one geometry, handed in by concurrent rsr_process calls, walk the
// network as ONE batch (engine.cpp: Combiner) -- a 256 x 256 image is 200 blocks for 256 CUs and costs as much per launch as four of
// them.  Every image keeps its own device buffers: the kernels that touch images get the pointers by value and the tile's image index.
constexpr int kMaxMerge = 16;

// Pixel formats of the caller's images (the RSR_FMT_* values of include/realsr_hip.h).  The planar formats are RGB only, [3][h][w],
// values in [0, 1]; they ride in the same pointer arrays as the uint8 images (PreArgs::imgs, PostArgs::outs, ConvArgs::out_u8s).
constexpr int kFmtU8 = 0, kFmtF16 = 1, kFmtF32 = 2;
// YUV 4:2:0 surfaces, as a video decoder yields and an encoder takes them (RSR_FMT_NV12 / RSR_FMT_P010): a plane of Y [h][w], then --
// `plane pitch` bytes behind Y(0,0) -- a plane of interleaved UV [h/2][w/2][2] whose rows are as many bytes apart as the Y rows.  uint8
// codes, or uint16 words that hold a 10-bit code in their HIGH bits (code << 6).  w and h are even.
constexpr int kFmtNV12 = 4, kFmtP010 = 5;
// YUV 4:2:2 surfaces, what broadcast and archive codecs hold (RSR_FMT_NV16 / RSR_FMT_P210): the same two planes, but chroma is halved
// horizontally only -- the UV plane is [h][w/2][2], one UV row per Y row.  w is even; h is any.
constexpr int kFmtNV16 = 8, kFmtP210 = 9;
// Planar YUV 4:4:4, what screen recordings, mezzanine masters and software video frameworks hold (RSR_FMT_YUV444P / RSR_FMT_YUV444P10,
// yuv444p / yuv444p10le): three full planes Y, U, V [h][w] one plane pitch apart -- the LAYOUT of the planar float formats with a YUV
// colour model.  uint8 codes, or uint16 words that hold a 10-bit code in their LOW bits.  No pairs, no quads: w and h are any.
constexpr int kFmtYUV444P = 12, kFmtYUV444P10 = 13;
// 16-bit RGB(A), what scans, raw developments and renders hold (RSR_FMT_U16_HWC): the LAYOUT of the uint8 image with uint16 samples, native
// little-endian words, full range 0 .. 65535, c = 3 or 4.  `data` and the row pitch are multiples of 2.
constexpr int kFmtU16 = 16;

// What a pixel format IS, said once: sizes, parity rules, admission rules and byte rectangles on the host, the rectangle selection of the
// diff kernel on the device, all read these fields.  A new format is one more case of pix_fmt.
struct PixFmt
{
    int es;             // bytes of one element of a row: c (2 c) for uint8 (uint16) HWC, elsewhere of one sample / half / float; 0 = no such format
    int planes;         // planes addressed through the plane pitch: 1 (uint8 / uint16 HWC), 2 (Y, then UV) or 3
    bool pairs;         // plane 1 holds interleaved (U, V) pairs (the semi-planar surfaces: the geometry behind the pair / quad units) ...
    int csx, csy;       // ... the chroma shift of that plane along x and y: 1, 1 at 4:2:0; 1, 0 at 4:2:2; 0, 0 everywhere else
    int bits;           // of a Y'CbCr code (the colour model: YuvCoef, the decode in front of the network, the encode behind conv_last); 0 = RGB
    bool high;          // a 10-bit code sits in the HIGH bits of its 16-bit word (code << 6), not in the low ones
    int cmax;           // channel counts admitted: 3 .. cmax
    const char* family; // as the messages name it: "YUV 4:2:0", "YUV 4:2:2", else ""
    int sample = 1;     // bytes of one sample of an interleaved one-plane image (es = c * sample): 1 uint8 HWC, 2 uint16 HWC
    constexpr bool known() const { return es != 0; }
    constexpr bool takes(int c) const { return c >= 3 && c <= cmax; }
    constexpr int align() const { return planes == 1 ? sample : es; }                           // what `data` and the pitches of a descriptor must be multiples of
    constexpr long long rows(long long h) const { return h + (planes - 1) * (h >> csy); } // rows of all planes of an image h rows high, each w * es bytes
    constexpr bool odd(long long w, long long h) const { return ((w & csx) | (h & csy)) != 0; } // w or h breaks the parity rule of a subsampled axis
};
constexpr __host__ __device__ PixFmt pix_fmt(int fmt, int c = 3)
{
    switch (fmt)
    {
    case kFmtU8: return {c, 1, false, 0, 0, 0, false, 4, ""};
    case kFmtF16: return {2, 3, false, 0, 0, 0, false, 3, ""};
    case kFmtF32: return {4, 3, false, 0, 0, 0, false, 3, ""};
    case kFmtNV12: return {1, 2, true, 1, 1, 8, false, 3, "YUV 4:2:0"};
    case kFmtP010: return {2, 2, true, 1, 1, 10, true, 3, "YUV 4:2:0"};
    case kFmtNV16: return {1, 2, true, 1, 0, 8, false, 3, "YUV 4:2:2"};
    case kFmtP210: return {2, 2, true, 1, 0, 10, true, 3, "YUV 4:2:2"};
    case kFmtYUV444P: return {1, 3, false, 0, 0, 8, false, 3, ""};
    case kFmtYUV444P10: return {2, 3, false, 0, 0, 10, false, 3, ""};
    case kFmtU16: return {2 * c, 1, false, 0, 0, 0, false, 4, "", 2};
    default: return {0, 0, false, 0, 0, 0, false, 0, ""};
    }
}
// readers of it, where a name reads better than a field (the template dispatch of launch_preproc_tiles / launch_postproc_tiles)
constexpr bool fmt_is_422(int fmt) { return pix_fmt(fmt).csx && !pix_fmt(fmt).csy; }
constexpr bool fmt_is_444(int fmt) { return pix_fmt(fmt).bits && !pix_fmt(fmt).pairs; }
constexpr bool fmt_is_yuv(int fmt) { return pix_fmt(fmt).bits != 0; }
constexpr int fmt_yuv_bits(int fmt) { return pix_fmt(fmt).bits; }
// Every image is addressed through its own ROW PITCH and (planar formats) PLANE PITCH, both in BYTES (rsr_image of the C ABI): a crop of
// a larger frame, a window of a canvas.  A uint8 pitch need not be a multiple of the pixel size and a base pointer is aligned to the
// element only, so the image accesses are element-sized (the LDS-staged pre / post kernels, which move dwords, align by themselves or
// are not chosen: launch_*_tiles).  Planar pitches are multiples of the element size.  Row pitches fit an int (the engine checks).

struct WorkItem // 32 bytes: one aligned 2 x 16-byte fetch gives a workgroup everything about its block
{
    int slot, y0, x0; // tile slot and block origin at this table's resolution level (x0 | kFoldBit: a folded block)
    int H, W;         // dims of the slot's tile at this level (output dims of the conv)
    // 4x-level items of a non-TTA batch (conv_last writes the image itself): image coordinates of tile pixel (0,0) (= out_x - crop,
    // out_y - crop; may be negative) and pad2 = item_pad2(out_w, out_h, image): the size of the tile's un-padded output rectangle
    // (13 bits each) and the index of the tile's image in a merged batch (6 bits)
    int pad0, pad1, pad2;
};
__host__ __device__ inline int item_pad2(int out_w, int out_h, int img) { return out_w | ((img & 7) << 13) | (out_h << 16) | int((unsigned)(img >> 3) << 29); }
__host__ __device__ inline int pad2_w(int p) { return p & 0x1fff; }
__host__ __device__ inline int pad2_h(int p) { return (p >> 16) & 0x1fff; }
__host__ __device__ inline int pad2_img(int p) { return ((p >> 13) & 7) | int(((unsigned)p >> 29) << 3); }

struct TileDim
{
    int h, w; // LR dims of the (padded) tile living in this slot
};

struct PlaneSrc
{
    const void* base;     // plane 0 of slot 0
    long long slot_stride;  // bytes between slots
    long long plane_stride; // bytes between planes
};

struct ConvArgs
{
    // input planes: the first n0 from src0, then n1 from src1 (dense-block x planes + x1..x4 planes)
    PlaneSrc src0, src1;
    int n0, n1;
    int lvl_in;  // input resolution = LR << lvl_in
    int lvl_out; // output resolution = LR << lvl_out (lvl_out == lvl_in + 1 for the nearest-x2 fused convs)
    // weights: packed LDS images [plane of 16 cin][9 taps][NT*32 cout][16 cin]; bias fp32 [NT*32]
    const void* wpk16;
    const void* waux; // conv_last only: [plane of 16 cin][dx 0..2][row = dy*8 + cout][16 cin] (PackedConv::aux_off), or null
    int wpieces;      // 1-KiB pieces per plane of the resident image (set by choose_conv_flow)
    const float* bias;
    int lrelu; // LeakyReLU(0.2) on (acc + bias)
    // Output pixels closer than `margin` to the tile border (at this conv's output level) are never read by anything that
    // reaches the cropped output rectangle (engine.cpp: tail_margins): MFMA waves whose four rows lie wholly inside that frame
    // skip their block like rows below the tile.  0 = every pixel is needed.
    int margin;
    int pr; // patch ring depth of a resident-weight launch (set by choose_conv_flow)
    // residual stages: v = v*s + r  (r = fp16 planes)
    PlaneSrc res1, res2;
    int res1_kind, res2_kind; // 0 none, 1 fp16 planes
    float s1, s2;
    int res1_in_acc;  // res1 == the first planes of this conv's own input: added as an identity tap on the matrix pipe, coefficient
    float res1_coef;  // 1/s1 (must be exact in fp16)
    // outputs (any may be null)
    PlaneSrc out16;  // fp16 planes (2*NT planes)
    // conv_last: planar fp16 [3][H][W] per slot
    void* out_planar3;
    long long planar3_slot_stride; // bytes
    // conv_last fused with realsr_postproc.comp (non-TTA RGB, conv3x3_flow): uint8 HWC image, out_u8_w pixels wide (row pitch:
    // out_pitch below); the work items of the launch carry the tile's placement (WorkItem::pad0..2, see engine.cpp make_items)
    uint8_t* out_u8;
    int out_u8_w, out_u8_crop, out_u8_bgr; // crop = prepadding * scale; bgr: channel 0 <-> 2 on store
    // work
    const WorkItem* items;
    int nitems;
    const TileDim* dims;
    const void* zeros; // >= 16 zero bytes in device memory (LDS-DMA source for out-of-image pixels)
    unsigned long long* trace; // optional: block 0 / wave 0 writes per-stage s_memtime stamps (profiling aid), 2 x u64 per stage
    int dbg;           // ablation switches for profiling: 1 skip DMA, 2 skip MFMA, 4 skip epilogue stores, ...  (realsr_hip.h)
    // PRECISE residual stream (engine option "precise"; EPI 4 / 5 of conv3x3_flow).  The reference's Vulkan path rounds the 64-channel
    // trunk to fp16 after every RDB / RRDB (fp16 storage, realsr.cpp:44-46); the bar is its fp32 CPU path (realsr.cpp:525-838).  Here
    // a trunk value v lives as hi = fp16(v) -- the plane every conv reads, unchanged -- and lo = bf8((v - hi) * 2048): the rounding
    // residue as ONE byte (e5m2, i.e. the upper byte of an fp16; scaled so that it never becomes subnormal), 5 more bits of v than
    // hi alone -- as good as an fp16 residue for this network (profiles/r06_storage_emulation.txt).  The residual adds of the
    // epilogue use hi + lo / 2048.  The lo bytes of a tensor sit in the same allocation as its hi planes, a fixed number of bytes behind
    // plane 0 (same slot stride): only that distance travels; 0 = the tensor has no lo planes.  Layout: the two planes of an n-tile (32
    // channels) share one "pair plane" of the hi geometry (32 B per pixel: [half of the 16 channels][plane][8 channels]), so that a lane
    // of the epilogue reads / writes its 16 lo bytes of a row with ONE 1-KiB-per-wave access at the very offsets of its hi stores
    // (conv_flow.hip lo_row).  A 64-channel tensor: two pair planes = the room of two hi planes.
    int precise;          // 1: residual forms run the precise epilogue (out16 single-rounded from the fp32 value)
    long long lo1_off;    // lo planes of res1 = res1 + lo1_off bytes
    long long lo2_off;    // lo planes of res2
    long long out_lo_off; // lo planes of the output = out16 + out_lo_off (0: not kept)
    // fused conv_last: the uint8 image of every image of a (merged) batch and its row pitch in BYTES (the images of a merged batch may
    // differ in size); out_u8 == out_u8s[0] doubles as the mode flag
    uint8_t* out_u8s[kMaxMerge];
    int out_pitch[kMaxMerge];
    // ... or, out_fmt != kFmtU8, planar fp16 / fp32 images behind the same pointers, their planes out_plane[i] BYTES apart: min(max(r, 0), 1)
    // of the value r the uint8 conversion sees (fp16: that rounded once), plane = 2 - ch under out_u8_bgr
    int out_fmt;
    long long out_plane[kMaxMerge];
};

// ---- conv3x3_flow (conv_flow.hip: half-stage ring on 16-channel planes) -------------------------------------------------------------
// The bits of the engine option "flow_flags" (include/realsr_hip.h has the user's wording; the values are public) ...
constexpr int kFlowNtw2 = 1;        // two n-tiles per MFMA wave for the 64-output-channel convs: 4 MFMA waves x 64 channels, not 8 x 32
constexpr int kFlowInlineEpi = 2;   // no deferred epilogue for the 32-output-channel convs
constexpr int kFlowStreamW = 4;     // weights re-streamed per block even where they would fit in LDS for the whole launch
constexpr int kFlowLastGeneric = 8; // conv_last through the generic 32-output-channel path instead of (dy, cout) in M
// ... and those of the engine option "dbg" that exist in the product build (the ablation bits 1 / 4 / 64 / 128 of ConvArgs::dbg act in
// -DRSR_EXPERIMENT builds only: conv_flow.hip RSR_ABL)
constexpr int kDbgAllRows = 32;          // MFMA waves compute the rows they would skip (a test hook: results unchanged)
constexpr int kDbgNoFusedLast = 8192;    // conv_last never writes the caller's image itself
constexpr int kDbgNoSplitTail = 16384;   // no split tail for the early download
constexpr int kDbgPrePostVar1 = 32768, kDbgPrePostVar2 = 65536; // force variant 1 / 2 of the pre and post kernels (PreArgs::variant)

// The EPILOGUES of conv3x3_flow: the values of its template parameter EPI.  EPI stays an int (the numbers are part of the kernels'
// symbol names, which profiles/, tools/ and bench.py's report quote; DESIGN.md, README.md and the tests speak of "EPI 4 / 5"), but
// nothing outside this definition writes a number for one.
//   kEpiPlain (1)            v = act(acc) -> fp16 planes
//   kEpiRes (2)              v = s1*acc (the conv's own input rides in the accumulator as an identity tap) [, v = s2*v + r2] -> fp16 planes
//   kEpiPrec / kEpiPrec2 (4 / 5)  the PRECISE forms of kEpiRes without / with the second residual (engine option "precise"; 64 output
//        channels): the residual stream is kept as hi + lo / 2048, hi an fp16 plane as ever and lo ONE BYTE per element (bf8 = e5m2: the
//        upper byte of an fp16; ConvArgs::precise) -- v = s1*acc + lo1/2048 [, v = s2*v + r2 + lo2/2048] in fp32, then ONE rounding:
//        hi = fp16(v) -> out16 (what the next convs read), lo = bf8((v - hi) * 2048) -> the output's lo planes (16 B per pixel).  The
//        reference's GPU path rounds the trunk 92 times on its way through the 23 RRDBs (fp16 storage, realsr.cpp:44-46); this halves the
//        engine's distance to the fp32 CPU path (realsr.cpp:525-838; profiles/r06_storage_emulation.txt).  Absent lo planes are read
//        through a null buffer resource (zeros, no memory access) and written into one: the epilogue is branch-free.
//   kEpiLast* (0, 3, 6 .. 11)  conv_last, eight of them = 2 layouts x fp32 kept or not x 2 kinds of output:
//        layout: "3" = (dy, cout) in the MFMA's M dimension (3 / 6 / 8 / 9), "G" = the generic 32-output-channel path (0 / 7 / 10 / 11);
//        F32 (6 / 7 / 9 / 11; precise mode): conv_last's fp32 result goes to the uint8 conversion (or a planar fp32 blob) without the fp16
//        rounding of the reference's `output` blob in between;
//        Img (8 .. 11): the fused image is the caller's PLANAR FLOAT one (ConvArgs::out_fmt: fp16 or fp32, chosen at run time), not the
//        uint8 one / the planar blob -- instantiations of their own, so that the uint8 kernels keep their registers.
enum FlowEpi : int
{
    kEpiLastG = 0, kEpiPlain = 1, kEpiRes = 2, kEpiLast3 = 3, kEpiPrec = 4, kEpiPrec2 = 5, kEpiLast3F32 = 6, kEpiLastGF32 = 7,
    kEpiLast3Img = 8, kEpiLast3ImgF32 = 9, kEpiLastGImg = 10, kEpiLastGImgF32 = 11, kEpiCount = 12
};
enum FlowEpiForm : int { kFormPlain, kFormRes, kFormPrec, kFormPrec2, kFormLast };
struct EpiDesc
{
    int form;    // FlowEpiForm
    bool dycout; // conv_last's layout: (dy, cout) in M; false: generic
    bool out32;  // conv_last: the fp32 result is kept (converted / stored without an fp16 rounding in between)
    bool fimg;   // conv_last: the output is a planar float image
    constexpr bool last3() const { return form == kFormLast && dycout; }
    constexpr bool lastg() const { return form == kFormLast && !dycout; }
    constexpr bool resid() const { return form == kFormRes || form == kFormPrec || form == kFormPrec2; } // residual forms
    constexpr bool prec() const { return form == kFormPrec || form == kFormPrec2; }                       // ... with the hi + lo residual stream
    constexpr bool operator==(const EpiDesc& o) const { return form == o.form && dycout == o.dycout && out32 == o.out32 && fimg == o.fimg; }
};
constexpr __host__ __device__ EpiDesc epi_desc(int epi)
{
    switch (epi)
    {
    case kEpiPlain: return {kFormPlain, false, false, false};
    case kEpiRes: return {kFormRes, false, false, false};
    case kEpiPrec: return {kFormPrec, false, false, false};
    case kEpiPrec2: return {kFormPrec2, false, false, false};
    case kEpiLast3: return {kFormLast, true, false, false};
    case kEpiLast3F32: return {kFormLast, true, true, false};
    case kEpiLast3Img: return {kFormLast, true, false, true};
    case kEpiLast3ImgF32: return {kFormLast, true, true, true};
    case kEpiLastG: return {kFormLast, false, false, false};
    case kEpiLastGF32: return {kFormLast, false, true, false};
    case kEpiLastGImg: return {kFormLast, false, false, true};
    default: return {kFormLast, false, true, true}; // kEpiLastGImgF32
    }
}
// the epilogue that IS this description
constexpr int epi_of(const EpiDesc& d)
{
    for (int e = 0; e < kEpiCount; e++)
        if (epi_desc(e) == d) return e;
    return -1;
}

// What launch_conv_flow launches for a ConvArgs: the kernel (a row of conv_flow.hip's variant list), its launch geometry and its
// argument.  Pure host arithmetic -- choose_conv_flow makes no HIP call (tools/host_check runs it without a GPU).
struct FlowPlan
{
    int nt, ntw;      // conv3x3_flow<nt, ntw, ups, epi, defer, wres>
    bool ups;
    int epi;          // FlowEpi
    bool defer, wres;
    int pr;           // patch ring depth of a resident-weight launch (= args.pr), 0 when the weights are streamed
    int lds;          // dynamic LDS bytes
    int grid, block;
    // the ConvArgs as the kernel gets them: a first residual that is not the conv's own input moved into the second residual's slot
    // (trunk_conv), res1 = out16 for the precise conv_first, wpk16 = waux with wpieces = 3 for the (dy, cout) conv_last, pr
    ConvArgs args;
};
enum FlowChoice : int { kFlowNothing, kFlowLaunch, kFlowNotCovered }; // kFlowNothing: no work items, nothing to launch (a success)
// flags: kFlow* above.  nt: n-tiles (32 output channels) of the conv, ncu: the persistent grid's size
FlowChoice choose_conv_flow(const ConvArgs& a, int nt, int ncu, int flags, FlowPlan& plan);
bool flow_variant_exists(int nt, int ntw, bool ups, int epi, bool defer, bool wres); // a row of the variant list with this WRES
// false = this combination of outputs / residuals is not covered (the engine then reports an error)
bool launch_conv_flow(const ConvArgs& a, int nt, int ncu, int flags, hipStream_t st);
// Opt-in to > 64 KiB of dynamic LDS for every kernel instantiation, on the CURRENT device (call once per device).
hipError_t kernels_init_device();
hipError_t flow_init_device();

// ---- pre / post ------------------------------------------------------------------------------
// The fp32 constants of the YUV <-> RGB definition of include/realsr_hip.h ("yuv_matrix"), each computed in double and rounded once
// (engine.cpp yuv_coef): a function of the matrix, the range and the bit depth of the surface.  The kernels use them with one rounding per
// operation, in the order the header writes (kernels.hip mul_rn / add_rn: nothing is contracted).
struct YuvCoef
{
    // decode: yn = (Y - yoff) * ys, cb = (U - coff) * cs, cr = (V - coff) * cs; R = yn + rv * cr, G = (yn - gu * cb) - gv * cr, B = yn + bu * cb
    float yoff, ys, coff, cs, rv, gu, gv, bu;
    // encode: Y' = (kr * R + kg * G) + kb * B, code floor(Y' * yscale + yadd); Cb = (B - Y') * icb, Cr = (R - Y') * icr, code floor(C * cscale + cadd)
    float kr, kg, kb, yscale, yadd, cscale, cadd, icb, icr, maxcode;
};
constexpr int kYuvCoefFloats = 18;

struct BaseTile
{
    int x_org, y_org; // image coords of padded-tile pixel (0,0)  (= xi*T - P, yi*T - P)
    int tw, th;       // padded tile size
    int slot0;        // first slot (TTA: 8 consecutive slots)
    int out_x, out_y; // top-left of this tile's output rectangle in the x4 image
    int out_w, out_h; // size of that rectangle (tile_w_nopad*4, tile_h_nopad*4)
    int img;          // image of a merged batch this tile belongs to (index into PreArgs::imgs / PostArgs::outs; 0 otherwise)
};

struct PreArgs
{
    const uint8_t* imgs[kMaxMerge]; // HWC u8, one per image of the batch (ws[i] x hs[i] x c); BaseTile::img selects
    int fmt;                        // kFmtU8, or kFmtF16 / kFmtF32: the images are planar [3][hs[i]][ws[i]] of that type (c == 3),
                                    // or a YUV surface (PixFmt::bits): Y at imgs[i], UV plane[i] bytes behind it (planar 4:4:4: U, then V another
                                    // plane[i] behind), decoded with `yuv`; bgr does not apply
    int ws[kMaxMerge], hs[kMaxMerge];
    int pitch[kMaxMerge];           // bytes from one row of image i to the next (>= ws[i] * pixel size) ...
    long long plane[kMaxMerge];     // ... and, planar formats, from one plane to the next
    int nimgs;
    int c;
    const BaseTile* tiles;
    int ntiles;
    int tta;
    void* in_plane; // fp16 plane [th][tw][plane_ch] per slot, channels 0..2 = RGB/255, rest 0
    long long slot_stride;
    int bgr;
    int plane_ch;   // 16
    int variant;    // 0 default (launch_preproc_tiles picks), 1 one thread per pixel (engine dbg kDbgPrePostVar1), 2 LDS-staged (kDbgPrePostVar2; uint8 sources only)
    YuvCoef yuv;    // YUV formats only
    int siting;     // ... likewise: where a chroma sample sits in its luma quad (engine option "yuv_siting"): 0 centre, 1 left, 2 top-left
                    // (a 4:2:2 surface has no vertical siting: 2 is 1 there)
    int alpha_src;  // 1 (c == 4, uint8 / uint16 HWC): the alpha pass of engine option "alpha_net" -- sample 3 of the pixel goes into channels 0..2,
                    // converted like a colour sample (the gray image G of include/realsr_hip.h); bgr does not apply.  Kernels of their own.
};
void launch_preproc_tiles(const PreArgs& a, int max_tw, int max_th, hipStream_t st);

struct PostArgs
{
    const void* planar3; // fp16 (f32: fp32) [3][4th][4tw] per slot
    int f32;             // 1: precise mode, conv_last left its fp32 result (ConvArgs::precise)
    long long slot_stride;
    const BaseTile* tiles;
    int ntiles;
    int tta;
    int crop;   // prepadding*scale
    uint8_t* outs[kMaxMerge]; // HWC u8 (4w x 4h x c), one per image of the batch
    int out_fmt;              // kFmtU8, or kFmtF16 / kFmtF32: the outs are planar [3][4h][4w] of that type (c == 3; see ConvArgs::out_fmt),
                              // or a YUV surface (PixFmt::bits): Y at outs[i], UV out_plane[i] bytes behind it (postproc_tiles_yuv; box 0 / 1, 2 and 4 alike;
                              // planar 4:4:4: the planes Y, U, V out_plane[i] apart, postproc_tiles_yuv444)
    long long out_plane[kMaxMerge]; // planar formats: bytes from one plane of `outs[i]` to the next
    int out_pitch[kMaxMerge]; // row pitches of the outs in bytes
    int in_pitch[kMaxMerge];  // ... and those of the source images
    int nimgs;
    int c;
    int out_row0; // the outs point at output row out_row0 of the x4 image (a tile range's device buffer holds only its rows)
    const uint8_t* in_imgs[kMaxMerge]; // for alpha (c==4): the source images (w x h x 4)
    int tilesize;
    int bgr;
    int variant; // 0 default (LDS-staged under TTA, else one thread per pixel), 1 per-pixel (engine dbg kDbgPrePostVar1), 2 LDS-staged (kDbgPrePostVar2)
                 // (a uint16 HWC image at out_scale 4: 1 one pixel per thread, 2 two neighbouring pixels, 0 two without TTA and one with)
                 // (a planar 4:4:4 surface: 1 one pixel per thread, 2 two neighbouring pixels, 0 two at out_scale 4 and one elsewhere --
                 // with_pixels_per_thread)
    // Box-reduced output (engine option "out_scale"): 0 / 1 = the x4 image as above; 2 / 4 = every K x K box of x4 pixels, each clamped
    // to [0, 1] first, leaves as ONE pixel, its fp32 mean (postproc_tiles_box): the outs are (4 / K)w x (4 / K)h.  Everything above stays in
    // x4 units (BaseTile::out_*, out_row0, crop: all multiples of 4); the kernel divides by K.
    int box;
    // Area-averaged output at a rational scale num / den in lowest terms (rsr_set_out_ratio; den in 1..4, 1 <= num / den <= 4) that is not
    // 4, 2 or 1 -- those are `box` above, and num = 0 / 4 with box <= 1 is the x4 image --: postproc_tiles_area, the outs are
    // (w * num / den) x (h * num / den).  Everything above stays in x4 units; the kernel converts with * num / (4 * den), exact because the
    // engine refuses a call whose image or tile size times num is not a multiple of den.
    // num / den is the ratio along x; num_y / den_y the one along y (rsr_set_out_ratio_xy; den up to 8 there, so a footprint has up to 5
    // taps per axis) -- equal to num / den wherever one ratio serves both axes.  The outs are (w * num / den) x (h * num_y / den_y), columns
    // convert with * num / (4 * den), rows with * num_y / (4 * den_y); a pair that differs is never `box`, whatever its two ratios.
    // area_norm = fp32(1 / (16 * den * den_y)).
    int num, den;
    int num_y, den_y;
    float area_norm;
    YuvCoef yuv; // YUV out_fmt only
    // ... likewise: the chroma siting (engine option "yuv_siting": 0 centre, 1 left, 2 top-left).  The sited chroma filters clamp at the
    // first column / row of a TILE's rectangle; that is quad column / row 0 of the tile's own grid (BaseTile::out_*), so nothing else travels.
    int siting;
    int in_fmt; // c == 4: what in_imgs are made of, kFmtU8 or kFmtU16 (alpha_bicubic reads their samples)
    // 1 (c == 4, uint8 / uint16 HWC outs): the alpha pass of engine option "alpha_net" -- the blob holds the network's result for the gray
    // image of the alpha; ONLY sample 3 of every pixel is stored, the mean of the three channel values RSR_FMT_F32_CHW would hold
    // (postproc_tiles_alpha: x4, box and area alike).  in_imgs, in_fmt, bgr and variant are not looked at.
    int alpha_dst;
    // 1 (engine option "dither"; an integer out_fmt: uint8 / uint16 HWC, every YUV surface): every colour sample is rounded against the
    // threshold theta(x, y) of include/realsr_hip.h ("dither") instead of 0.5 -- x, y the sample's own indices in its plane of the output
    // image, made from BaseTile::out_x / out_y (NOT relative to out_row0: a tile range carries the image's pattern).  Kernels of their own:
    // the instantiations of 0 are untouched.  Alpha samples (the bicubic, and the whole alpha_dst launch) and the float formats ignore it.
    int dither;
};
void launch_postproc_tiles(const PostArgs& a, int max_ow, int max_oh, hipStream_t st);

// ---- frame diff per tile, frame sequences (rsr_diff_tiles, rsr_diff_tiles_sequence, rsr_process_device_sequence) --------------------
// The SOURCE RECTANGLE of tile (yi, xi) of a w x h image at tile size T and prepadding P: the image pixels its padded tile reads, i.e. the
// padded rectangle clipped to the image (reflect-101 never leaves it: the reflection of an index less than P outside an edge lies less
// than P + 1 inside it).  Half-open, r = {x0, y0, x1, y1}.
__host__ __device__ inline void tile_source_rect(int w, int h, int T, int P, int xi, int yi, int r[4])
{
    const int ex = (xi + 1) * T < w ? (xi + 1) * T : w, ey = (yi + 1) * T < h ? (yi + 1) * T : h;
    r[0] = xi * T - P > 0 ? xi * T - P : 0;
    r[1] = yi * T - P > 0 ? yi * T - P : 0;
    r[2] = ex + P < w ? ex + P : w;
    r[3] = ey + P < h ? ey + P : h;
}
// n pairs of images of ONE format and geometry in one launch.  mask[k][t] = 1 when any compared byte of tile t's source rectangle differs
// between the images a and b of pair k (their own pitches), else 0; include/realsr_hip.h rsr_diff_tiles says which bytes are compared.  The
// pair index travels in the grid; every pair brings its own two descriptors, by value.  A pair without an `a` (the first frame of a stream
// that has no predecessor) marks every tile.  One kernel body for two sizes of its argument block: room for kMaxMerge pairs, and for ONE
// (rsr_diff_tiles) -- a 10 us call pays measurably for 720 bytes of arguments it does not use (profiles/format_table.txt).
struct DiffPair
{
    const uint8_t* a; // null: every tile of this pair is marked
    const uint8_t* b;
    long long pitch_a, plane_a, pitch_b, plane_b; // bytes, resolved (plane: from one plane to the next; a surface: Y(0,0) to the UV plane)
};
template <int N> struct DiffArgs // N: 1 or kMaxMerge
{
    DiffPair pair[N];
    int n;            // <= N
    int fmt, w, h, c;
    int T, P, nx, ny; // tile size, prepadding, tile grid
    uint8_t* mask;    // [n][ny * nx]
};
template <int N> hipError_t launch_diff_tiles(const DiffArgs<N>& a, hipStream_t st); // the error of the memset or of the launch

// ---- flat-alpha scan (engine option "alpha_adaptive") ------------------------------------------------------------------------------
// flags[t] = 1 when the alpha samples of tile t's source rectangle are not all equal, else 0: tile t of a batch's DEVICE tile table, whose
// rectangle is [max(x_org, 0), min(x_org + tw, w)) x [max(y_org, 0), min(y_org + th, h)) of image BaseTile::img -- what tile_source_rect
// returns for the tile.  The images are RGBA, uint8 or uint16 HWC (u16), and travel by value as PreArgs carries them; samples are compared
// at their own depth.  No byte outside the rectangle's rows and pixels is read.  Under TTA a tile is scanned once: the grid runs over
// tiles, not slots.
struct FlatArgs
{
    const uint8_t* imgs[kMaxMerge];
    int ws[kMaxMerge], hs[kMaxMerge];
    long long pitch[kMaxMerge]; // bytes from one row of image i to the next
    const BaseTile* tiles;
    int ntiles;
    int u16;        // 1: uint16 samples (kFmtU16), 0: uint8
    uint8_t* flags; // device, [ntiles]
};
// max_th: the tallest padded tile of the table (sizes the grid).  The error of the memset or of the launch.
hipError_t launch_alpha_flat_tiles(const FlatArgs& a, int max_th, hipStream_t st);

// One rectangle of bytes to move: `rows` rows of `width` bytes, from src to dst, each with its own pitch, at any alignment.  The rectangles
// of one launch never overlap one another's destinations, and no source is another rectangle's destination.
struct PropRect
{
    uint8_t* dst;
    const uint8_t* src;
    long long dst_pitch, src_pitch;
    int width, rows;
};
// d_rects: DEVICE table of nrects entries; max_rows: the tallest of them (sizes the grid)
hipError_t launch_propagate_rects(const PropRect* d_rects, int nrects, int max_rows, hipStream_t st);

// ---- three-plane YUV frames <-> surfaces (rsr_pack_planes, rsr_unpack_planes) -----------------------------------------------------------
// A frame as a software decoder holds it (yuv420p, yuv422p, yuv444p and their 10-bit little-endian forms: three planes, each with rows
// of its own) beside the surface of format `fmt` the engine takes.  Pitches in bytes, resolved; the chroma planes are (w >> csx) x
// (h >> csy) samples.  Up to kMaxMerge frames of one geometry by value, as DiffArgs carries its pairs: ONE launch moves them all.
struct PlaneFrame
{
    uint8_t *y, *u, *v; // the three planes
    uint8_t* surf;      // Y(0,0) of the surface
    long long y_pitch, c_pitch; // of the Y plane, of the U and V planes
    long long row, plane;       // of the surface (ImageRef)
};
struct PlanesArgs
{
    PlaneFrame f[kMaxMerge];
    int n; // <= kMaxMerge
    int fmt, w, h;
};
// pack: planes -> surface, every P010 / P210 word (plane word & 1023) << 6; unpack: surface -> planes, every such word >> 6.  Bytes of the
// 8-bit formats and words of YUV444P10 move unchanged.  Nothing outside the rows of the destination is written, nothing outside the rows
// of the source read.
hipError_t launch_move_planes(const PlanesArgs& a, bool pack, hipStream_t st);

// ---- network interpolation: the active blob from two resident ones (rsr_set_blend) --------------------------------------------------------
// One piece of a blend segment (model.h BlendSeg): `units` 16-byte units from byte `off` of the blobs on, at most kBlendChunkUnits of
// them, never across the end of its segment.  A workgroup takes whole chunks, so which segment a unit belongs to is never searched for.
constexpr int kBlendChunkUnits = 1024; // 16 KiB: four units per thread of a 256-thread workgroup, all loads of both blobs in flight in front of the stores
struct BlendChunk
{
    uint64_t off;   // from the start of the blob; a multiple of 16 (segments start 256-byte aligned, chunks are multiples of 16 bytes)
    uint32_t units; // 1 .. kBlendChunkUnits
    uint32_t f32;   // fp32 elements (biases), else fp16
};
// c = (u * a) + (t * b) over every chunk of the DEVICE table, u = 1 - t: fp16 elements converted to fp32, blended and rounded to nearest
// even; every operation rounded by itself (no fused multiply-add).  a, b, c: three blobs of one table, 16-byte aligned, c neither a nor
// b.  Nothing outside the chunks is read or written.  One launch.
hipError_t launch_blend_blob(const BlendChunk* d_chunks, int nchunks, const void* a, const void* b, void* c, float t, int num_cu, hipStream_t st);

// shader-shaped standalone kernels (parity tests): device pointers
void launch_preproc_shader(const uint8_t* bottom, int w, int h, int channels, uint16_t* const top[8], int ntop, int outw,
                           int outh, int outcstep, int pad_top, int pad_left, int crop_x, int crop_y, uint16_t* alpha,
                           int alphaw, int alphah, int bgr, hipStream_t st);
void launch_postproc_shader(const uint16_t* const bottom[8], int nbottom, int w, int h, int cstep, const uint16_t* alpha,
                            int alphaw, int alphah, uint8_t* top, int outw, int outh, int offset_x, int gx_max, int crop_x,
                            int crop_y, int channels, int bgr, hipStream_t st);

// planar fp16 [3][h][w]  ->  plane [h][w][plane_ch] (net_forward test hook)
void launch_planar3_to_plane(const uint16_t* planar, int w, int h, void* plane, int plane_ch, hipStream_t st);
// zero the 64-byte guards of `count` planes, `stride` bytes apart
void launch_zero_guards(void* first_guard, long long stride, long long count, hipStream_t st);

// ---- model self-check (Engine::selfcheck): two reductions, results independent of scheduling ----
// Range probe: what ONE convolution stored for ONE tile whose slot holds exactly the tile's pixels (capacity = h * w): `nplanes`
// runs of `halfs_per_plane` fp16 values (a multiple of 8; 16-byte aligned), `plane_stride` bytes apart -- the [H][W][16] planes of
// ConvArgs::out16 without their guards, or conv_last's planar blob as one run.  *peak_bits = max(*peak_bits, bits of the largest
// finite |v| as a float) (atomicMax: the bit pattern of a non-negative float orders like the value), *nonfinite += inf / NaN count.
void launch_range_probe(const void* base, long long plane_stride, int nplanes, long long halfs_per_plane, unsigned* peak_bits,
                        unsigned long long* nonfinite, hipStream_t st);
// Output compare: the network's result of fp16 storage (a) against precise mode's fp32 blob (b), n elements each (a multiple of 8).
// res[0] = bits of max |a - b| (atomicMax as above), res[1] = max |q(a) - q(b)|, q = the uint8 conversion of postproc_tiles
// (post_store(v * 255)); *ndiff = elements with q(a) != q(b).  The caller zeroes res[0..1] and *ndiff.
void launch_output_compare(const uint16_t* a, const float* b, long long n, unsigned* res, unsigned long long* ndiff, hipStream_t st);

} // namespace rsr
