// kernels.hip -- gfx950 (CDNA4 / MI355X) pre/post kernels of the RealSR x4 hot path.
//
//   preproc_tiles[_lds]    realsr_preproc{,_tta}.comp equivalent, writes the network input planes (from uint8 HWC or planar fp16 / fp32 images)
//   postproc_tiles[_lds]   realsr_postproc{,_tta}.comp equivalent, writes the uint8 HWC image (or a planar fp16 / fp32 one)
//                          (_lds: rows staged in LDS, dword loads / 1-KiB stores, transposed TTA variants through an LDS tile;
//                          chosen per launch by measurement: launch_*_tiles)
//   preproc_tiles<uint16_t> / postproc_tiles<., uint16_t> / postproc_tiles_u16x2   a 16-bit RGB(A) image (kFmtU16) as the source / destination;
//                          the box and area kernels take uint16_t as their TO alike
//   postproc_tiles_box     the image box-reduced to x2 / x1 (out_scale)
//   postproc_tiles_area    the image area-averaged to any other ratio, or to a ratio per axis (rsr_set_out_ratio, rsr_set_out_ratio_xy)
//   preproc_tiles<., true> an NV12 / P010 (4:2:0) or NV16 / P210 (4:2:2) surface as the source (YUV -> RGB inside the kernel)
//   postproc_tiles_yuv[_area]   such a surface as the destination, at out_scale 4 / 2 / 1 [at any other ratio]
//   preproc_tiles<., true, 0, kVs444> / postproc_tiles_yuv444[_area]   a planar 4:4:4 surface (kFmtYUV444P / kFmtYUV444P10) as the source / destination
//   *_shader               the same arithmetic in the shaders' own memory layout (parity tests; independent of everything below)
//
// Every rule the header (include/realsr_hip.h) fixes bit for bit is written ONCE, as a __device__ __forceinline__ function the kernels share:
//   tta_dest               where pixel (gx, gy) of a tile goes in TTA variant k                    preproc_tiles, preproc_tiles_lds
//   tta_gather / merged_block   the eight TTA variants of a K x K block merged in the shader's order [and clamped]
//                                                                                                    every post kernel but postproc_tiles_lds
//   alpha_bicubic          the bicubic x4 alpha value                                               every post kernel that writes RGBA
//   area_sum / area_pixel  the area-average loop nest over a tap source                            postproc_tiles_area, postproc_tiles_yuv_area
//   yuv_quad               a luma quad and its (U, V) pair(s) from a source of pixels d              postproc_tiles_yuv, postproc_tiles_yuv_area
//   yuv_pixels             one or two pixels' Y, U and V codes from the same sources (4:4:4)        postproc_tiles_yuv444, postproc_tiles_yuv444_area
//   yuv_sample             the code of one sample of a surface: word >> 6, or word & 1023 (4:4:4)  yuv_decode
//
// The 351 convolutions live in conv_flow.hip (conv3x3_flow).  Written for gfx950 only.
#include "kernels.h"
#include <type_traits>

namespace rsr {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// > 64 KiB of dynamic LDS needs an opt-in per kernel AND per device (a process-wide "done" flag would leave the
// second GPU of a multi-device process without it): the engine calls this once per context, on its own device.
hipError_t kernels_init_device() { return flow_init_device(); }

// =============================================================================================
// pre / post processing
// =============================================================================================

// reflect-101 exactly as realsr_preproc.comp:59-62.  The shader's single reflection leaves the image
// when the halo exceeds the image (n <= prepadding): the reference then reads out of bounds; here
// the index is clamped (as the oracle does) so tiny images stay memory-safe and deterministic.
__device__ __forceinline__ int reflect101(int v, int n)
{
    v = abs(v);
    v = (n - 1) - abs(v - (n - 1));
    return min(max(v, 0), n - 1);
}

// ---- YUV 4:2:0 and 4:2:2 sources (PreArgs::fmt kFmtNV12 / kFmtP010, kFmtNV16 / kFmtP210) ----------------------------------------
// ONE fp32 operation, rounded by itself.  HIP's __fmul_rn / __fadd_rn are the plain operators, which the compiler contracts with their
// neighbours into an fma once they are inlined; an operation compiled with contraction off takes no part in that.
__device__ __forceinline__ float mul_rn(float a, float b)
{
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b)
{
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float sub_rn(float a, float b)
{
#pragma clang fp contract(off)
    return a - b;
}

// The vertical-chroma-shift argument VS of the YUV templates below: 1 = 4:2:0, 0 = 4:2:2, kVs444 = a planar 4:4:4 surface, which has no
// chroma shift on either axis and a plane of its own per component.
constexpr int kVs444 = -1;

// The code of the sample at p as a float: a byte; or a 16-bit word that holds its 10-bit code in the HIGH bits (P010 / P210: word >> 6) or,
// LOW = true, in the low ones (yuv444p10le: word & 1023 -- whatever a producer left above bit 9 is not part of the sample).
template <typename SRC, bool LOW>
__device__ __forceinline__ float yuv_sample(const uint8_t* p)
{
    if constexpr (sizeof(SRC) == 1) return (float)*p;
    else if constexpr (LOW) return (float)(*reinterpret_cast<const unsigned short*>(p) & 1023u);
    else return (float)(*reinterpret_cast<const unsigned short*>(p) >> 6);
}

// The (U, V) pair of chroma sample cx of a UV row: ONE 2-byte (NV12) or 4-byte (P010) load where the address allows it -- an NV12 surface
// may start on any byte, a P010 surface on any even one.
template <typename SRC>
__device__ __forceinline__ void load_uv(const uint8_t* row, int cx, float& u, float& v)
{
    const uint8_t* p = row + (long long)cx * (2 * (int)sizeof(SRC));
    if constexpr (sizeof(SRC) == 1)
    {
        unsigned w;
        if (!(reinterpret_cast<uintptr_t>(p) & 1)) w = *reinterpret_cast<const unsigned short*>(p);
        else w = (unsigned)p[0] | ((unsigned)p[1] << 8);
        u = (float)(w & 0xffu);
        v = (float)(w >> 8);
    }
    else
    {
        unsigned w;
        if (!(reinterpret_cast<uintptr_t>(p) & 3)) w = *reinterpret_cast<const unsigned*>(p);
        else w = (unsigned)reinterpret_cast<const unsigned short*>(p)[0] | ((unsigned)reinterpret_cast<const unsigned short*>(p)[1] << 16);
        u = (float)((w & 0xffffu) >> 6);
        v = (float)(w >> 22);
    }
}

// RGB in [0, 1] of pixel (x, y) of a w x h surface (Y at img, rows `pitch` bytes apart; UV `plane` bytes behind Y(0,0), same pitch).
// Chroma is sited at the centre of its 2 x 2 luma quad: a luma pixel takes 3/4 of the chroma sample of its own quad and 1/4 of the next
// one on its side, per axis, indices clamped at the image edge -- horizontally first, (3 * near + far) * 0.25f, then vertically the same
// way: exact for codes.  Lanes run along x: the Y loads of a wave are contiguous, a pair of neighbouring lanes shares its near chroma
// column, and U and V always travel in one load.  Every product and sum below is rounded by itself (no contraction).
//
// SITE (option "yuv_siting"; include/realsr_hip.h "Chroma siting"): 0 = the centre siting above, on both axes.  1 (left) / 2 (top-left):
// chroma is CO-SITED with the even luma index horizontally / on both axes (yuv_decode_cos); a left-sited surface keeps the centre rule
// vertically.  A co-sited axis takes c[n] for an even index i = 2n and (c[n] + c[min(n + 1, N/2 - 1)]) * 0.5f for an odd one: one chroma
// column (row) for even pixels, two for odd ones, so the lanes of a pair still share their loads.  Exact for codes, like the centre rule.
// The centre rule along one axis: 3/4 of the near chroma sample, 1/4 of the far one (yuv_decode, yuv_decode_cos).
__device__ __forceinline__ float chroma_mix(float near, float far) { return mul_rn(add_rn(mul_rn(3.f, near), far), 0.25f); }

// VS (the surface's vertical chroma shift): 1 = 4:2:0, everything above.  0 = 4:2:2 (kFmtNV16 / kFmtP210; include/realsr_hip.h "YUV 4:2:2"): the
// chroma row of pixel (x, y) is row y itself, so only the horizontal half of either rule applies -- two load_uv per pixel instead of four --
// and SITE is 0 or 1 (top-left has no vertical meaning there: launch_preproc_tiles runs it as 1).
template <typename SRC, int SITE, int VS = 1>
__device__ __forceinline__ void yuv_decode_cos(const uint8_t* img, int pitch, long long plane, int x, int y, int w, int h, float& U, float& V)
{
    const int cx0 = x >> 1, cx1 = min(cx0 + (x & 1), (w >> 1) - 1); // an even x reads its column twice: (c + c) * 0.5f == c
    if constexpr (VS == 0)
    {
        const uint8_t* r = img + plane + (long long)y * pitch;
        float u0, v0, u1, v1;
        load_uv<SRC>(r, cx0, u0, v0);
        load_uv<SRC>(r, cx1, u1, v1);
        U = mul_rn(add_rn(u0, u1), 0.5f), V = mul_rn(add_rn(v0, v1), 0.5f);
        return;
    }
    int cy0 = y >> 1, cy1;
    if constexpr (SITE == 2) cy1 = min(cy0 + (y & 1), (h >> 1) - 1);
    else cy1 = min(max(cy0 + ((y & 1) ? 1 : -1), 0), (h >> 1) - 1); // centre rule: cy0 near, cy1 far
    const uint8_t* r0 = img + plane + (long long)cy0 * pitch;
    const uint8_t* r1 = img + plane + (long long)cy1 * pitch;
    float u00, v00, u01, v01, u10, v10, u11, v11; // (row, column)
    load_uv<SRC>(r0, cx0, u00, v00);
    load_uv<SRC>(r0, cx1, u01, v01);
    load_uv<SRC>(r1, cx0, u10, v10);
    load_uv<SRC>(r1, cx1, u11, v11);
    auto cos = [](float a, float b) { return mul_rn(add_rn(a, b), 0.5f); };
    const float ua = cos(u00, u01), ub = cos(u10, u11), va = cos(v00, v01), vb = cos(v10, v11); // horizontally first
    if constexpr (SITE == 2) { U = cos(ua, ub); V = cos(va, vb); }
    else { U = chroma_mix(ua, ub); V = chroma_mix(va, vb); }
}

template <typename SRC, int SITE = 0, int VS = 1>
__device__ __forceinline__ void yuv_decode(const uint8_t* img, int pitch, long long plane, int x, int y, int w, int h, const YuvCoef& k, float (&rgb)[3])
{
    const uint8_t* yp = img + (long long)y * pitch + (long long)x * (int)sizeof(SRC);
    const float Y = yuv_sample<SRC, VS == kVs444>(yp);
    float U, V;
    if constexpr (VS == kVs444)
    { // planar 4:4:4 (include/realsr_hip.h "YUV 4:4:4"): the pixel's own sample of planes 1 and 2 -- no chroma filter, no siting
        U = yuv_sample<SRC, true>(yp + plane), V = yuv_sample<SRC, true>(yp + 2 * plane);
    }
    else if constexpr (SITE != 0) yuv_decode_cos<SRC, SITE, VS>(img, pitch, plane, x, y, w, h, U, V);
    else if constexpr (VS == 0)
    { // 4:2:2, centre: the horizontal rule on the pixel's own chroma row
        const int cxn = x >> 1, cxf = min(max(cxn + ((x & 1) ? 1 : -1), 0), (w >> 1) - 1);
        const uint8_t* r = img + plane + (long long)y * pitch;
        float un, vn, uf, vf;
        load_uv<SRC>(r, cxn, un, vn);
        load_uv<SRC>(r, cxf, uf, vf);
        U = chroma_mix(un, uf), V = chroma_mix(vn, vf);
    }
    else
    {
        const int cxn = x >> 1, cxf = min(max(cxn + ((x & 1) ? 1 : -1), 0), (w >> 1) - 1);
        const int cyn = y >> 1, cyf = min(max(cyn + ((y & 1) ? 1 : -1), 0), (h >> 1) - 1);
        const uint8_t* rn = img + plane + (long long)cyn * pitch;
        const uint8_t* rf = img + plane + (long long)cyf * pitch;
        float unn, vnn, unf, vnf, ufn, vfn, uff, vff; // (row, column): near / far
        load_uv<SRC>(rn, cxn, unn, vnn);
        load_uv<SRC>(rn, cxf, unf, vnf);
        load_uv<SRC>(rf, cxn, ufn, vfn);
        load_uv<SRC>(rf, cxf, uff, vff);
        U = chroma_mix(chroma_mix(unn, unf), chroma_mix(ufn, uff)), V = chroma_mix(chroma_mix(vnn, vnf), chroma_mix(vfn, vff));
    }
    const float yn = mul_rn(sub_rn(Y, k.yoff), k.ys);
    const float cb = mul_rn(sub_rn(U, k.coff), k.cs), cr = mul_rn(sub_rn(V, k.coff), k.cs);
    const float r = add_rn(yn, mul_rn(k.rv, cr));
    const float g = sub_rn(sub_rn(yn, mul_rn(k.gu, cb)), mul_rn(k.gv, cr));
    const float b = add_rn(yn, mul_rn(k.bu, cb));
    rgb[0] = fminf(fmaxf(r, 0.f), 1.f);
    rgb[1] = fminf(fmaxf(g, 0.f), 1.f);
    rgb[2] = fminf(fmaxf(b, 0.f), 1.f);
}

// realsr_preproc_tta.comp:104-111: pixel (gx, gy) of a tw x th tile lands at (ox, oy) of TTA variant k, whose rows are ow long
// (preproc_tiles, preproc_tiles_lds).
__device__ __forceinline__ void tta_dest(int k, int gx, int gy, int tw, int th, int& oy, int& ox, int& ow)
{
    switch (k)
    {
    default: oy = gy; ox = gx; ow = tw; break;
    case 1: oy = gy; ox = tw - 1 - gx; ow = tw; break;
    case 2: oy = th - 1 - gy; ox = tw - 1 - gx; ow = tw; break;
    case 3: oy = th - 1 - gy; ox = gx; ow = tw; break;
    case 4: oy = gx; ox = gy; ow = th; break;
    case 5: oy = gx; ox = th - 1 - gy; ow = th; break;
    case 6: oy = tw - 1 - gx; ox = th - 1 - gy; ow = th; break;
    case 7: oy = tw - 1 - gx; ox = gy; ow = th; break;
    }
}

// realsr_preproc.comp:47-95 and realsr_preproc_tta.comp:54-113, for a batch of tiles.
// One thread per padded-tile pixel; writes the 32-channel fp16 input plane(s) (channels 3..31 = 0).
// The band-relative coordinates of the shader (crop_x/crop_y/pad) are folded into x_org/y_org:
// reflecting against the band equals reflecting against the image (engine.cpp explains why).
// SRC: what the caller's image is made of -- uint8_t (HWC), uint16_t (HWC, YUV = false), or _Float16 / float: planar [3][ih][iw] in [0, 1].  A half IS the network
// input (the uint8 path makes fp16(float(k) * (1/255.f)) of byte k: those halfs give that path's input exactly); a float is rounded to
// fp16, to nearest even.  Lanes run along x: the three plane reads of a wave are contiguous.  Rows are PreArgs::pitch bytes apart, planes
// PreArgs::plane: the reflected (x, y) is an index into the image, never into the surface around it.
// YUV = true: the image is a 4:2:0 surface, SRC its sample type -- uint8_t (NV12) or uint16_t (P010, the code in the high 10 bits).  Pixel
// (x, y) -- reflected first, like every other source -- is decoded as include/realsr_hip.h ("yuv_matrix") defines, bit for bit: yuv_decode;
// SITE is the chroma siting (PreArgs::siting: a kernel per siting, the centre-sited one is what it was before the others existed).
// VS = 0: a 4:2:2 surface (kFmtNV16 / kFmtP210), SRC its sample type likewise; the chroma row of a pixel is its own (yuv_decode).
// VS = kVs444: a planar 4:4:4 surface (kFmtYUV444P / kFmtYUV444P10; a uint16_t holds its code in the LOW 10 bits): three plane reads at
// the pixel's own (x, y), each contiguous over the lanes of a wave like those of the planar float sources; SITE is 0.
// SRC = AlphaOf<uint8_t> / AlphaOf<uint16_t> (PreArgs::alpha_src, engine option "alpha_net"): the RGBA image's ALPHA sample, converted
// like a colour sample of its type, goes into channels 0 .. 2 -- the gray image G of include/realsr_hip.h.  Instantiations of their own.
template <typename S> struct AlphaOf { typedef S sample; };
template <typename T> struct alpha_of { typedef void sample; };
template <typename S> struct alpha_of<AlphaOf<S>> { typedef S sample; };

template <typename SRC, bool YUV = false, int SITE = 0, int VS = 1>
__global__ __launch_bounds__(256) void preproc_tiles(const PreArgs a)
{
    const BaseTile t = a.tiles[blockIdx.z];
    const int gx = blockIdx.x * 32 + (threadIdx.x & 31);
    const int gy = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (gx >= t.tw || gy >= t.th) return;
    const int im = __builtin_amdgcn_readfirstlane(t.img), iw = a.ws[im], ih = a.hs[im];
    const int x = reflect101(gx + t.x_org, iw);
    const int y = reflect101(gy + t.y_org, ih);
    [[maybe_unused]] const int i0 = a.bgr ? 2 : 0, i2 = a.bgr ? 0 : 2; // (a YUV source has no channel order to swap)
    half8 v0;
#pragma unroll
    for (int e = 0; e < 8; e++) v0[e] = (_Float16)0.f;
    if constexpr (YUV)
    {
        float rgb[3];
        yuv_decode<SRC, SITE, VS>(a.imgs[im], a.pitch[im], a.plane[im], x, y, iw, ih, a.yuv, rgb);
        v0[0] = (_Float16)rgb[0];
        v0[1] = (_Float16)rgb[1];
        v0[2] = (_Float16)rgb[2];
    }
    else if constexpr (!std::is_void<typename alpha_of<SRC>::sample>::value)
    { // the alpha pass: sample 3 of RGBA pixel (x, y), as the branches below convert a colour sample of its type
        typedef typename alpha_of<SRC>::sample S;
        const S k = reinterpret_cast<const S*>(a.imgs[im] + (long long)y * a.pitch[im])[x * 4 + 3];
        const float norm_val = sizeof(S) == 1 ? 1 / 255.f : 1 / 65535.f;
        v0[0] = v0[1] = v0[2] = (_Float16)((float)k * norm_val);
    }
    else if constexpr (sizeof(SRC) == 1)
    {
        const uint8_t* p = a.imgs[im] + (long long)y * a.pitch[im] + x * a.c;
        const float norm_val = 1 / 255.f;
        v0[0] = (_Float16)((float)p[i0] * norm_val);
        v0[1] = (_Float16)((float)p[1] * norm_val);
        v0[2] = (_Float16)((float)p[i2] * norm_val);
    }
    else if constexpr (std::is_same<SRC, uint16_t>::value)
    { // uint16 HWC (kFmtU16): fp16(float(k) * (1 / 65535.f)) of the unsigned word k -- for k = 257 b exactly the half the uint8 path makes of byte b
        const uint16_t* p = reinterpret_cast<const uint16_t*>(a.imgs[im] + (long long)y * a.pitch[im]) + x * a.c;
        const float norm_val = 1 / 65535.f;
        v0[0] = (_Float16)((float)p[i0] * norm_val);
        v0[1] = (_Float16)((float)p[1] * norm_val);
        v0[2] = (_Float16)((float)p[i2] * norm_val);
    }
    else
    {
        const long long cstep = a.plane[im]; // bytes, like the row pitch
        const uint8_t* p = a.imgs[im] + (long long)y * a.pitch[im] + (long long)x * (int)sizeof(SRC);
        v0[0] = (_Float16) * reinterpret_cast<const SRC*>(p + i0 * cstep);
        v0[1] = (_Float16) * reinterpret_cast<const SRC*>(p + cstep);
        v0[2] = (_Float16) * reinterpret_cast<const SRC*>(p + i2 * cstep);
    }
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    const int nv = a.tta ? 8 : 1;
    for (int k = 0; k < nv; k++)
    {
        int oy, ox, ow;
        tta_dest(k, gx, gy, t.tw, t.th, oy, ox, ow);
        char* dst = static_cast<char*>(a.in_plane) + (long long)(t.slot0 + k) * a.slot_stride + ((long long)oy * ow + ox) * (a.plane_ch * 2);
        *reinterpret_cast<half8*>(dst) = v0;
        *reinterpret_cast<uint4*>(dst + 16) = z;
        if (a.plane_ch == 32)
        {
            *reinterpret_cast<uint4*>(dst + 32) = z;
            *reinterpret_cast<uint4*>(dst + 48) = z;
        }
    }
}

// The same arithmetic with the memory traffic of realsr_preproc{,_tta}.comp reorganised for HBM (round 4; byte-identical to the
// one-thread-per-pixel kernel above, which stays the default -- see launch_preproc_tiles):
//   * one workgroup = a 32 x 32 block of padded-tile pixels.  Its source rows are staged in LDS with aligned DWORD loads, one
//     wave per row (reflection folds the 32 columns of a block onto at most 32 source columns, i.e. <= 132 contiguous bytes);
//   * the pixels are converted once (uint8 -> fp16 / 255) into an LDS tile [32][33] of (r, g, b) halfs;
//   * every TTA variant is then written row by row of ITS OWN orientation: a wave stores 32 pixels x 32 B = 1 KiB of whole
//     cache lines per instruction (lane = (pixel, 16-byte half)) -- also for the four transposed variants, whose rows run down
//     the tile's columns (column reads of the LDS tile are conflict-free through the 33-pixel pitch).
__global__ __launch_bounds__(256) void preproc_tiles_lds(const PreArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned char raw[32][144];
    __shared__ uint2 px[32][33];
    const BaseTile t = a.tiles[blockIdx.z];
    const int gx0 = blockIdx.x * 32, gy0 = blockIdx.y * 32;
    if (gx0 >= t.tw || gy0 >= t.th) return;
    const int im = __builtin_amdgcn_readfirstlane(t.img), iw = a.ws[im], ih = a.hs[im];
    const uint8_t* const img = a.imgs[im];
    const int nx = min(32, t.tw - gx0), ny = min(32, t.th - gy0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // source column span [lo, hi] of the block's columns (every wave computes it for itself)
    int xs = reflect101(gx0 + min(lane & 31, nx - 1) + t.x_org, iw);
    int lo = xs, hi = xs;
#pragma unroll
    for (int d = 1; d < 32; d <<= 1)
    {
        lo = min(lo, __shfl_xor(lo, d));
        hi = max(hi, __shfl_xor(hi, d));
    }
    const int pitch = a.pitch[im];
    const long long total = (long long)(ih - 1) * pitch + (long long)iw * a.c; // one past the image's last byte
    for (int r = wave; r < ny; r += 4)
    {
        const int y = reflect101(gy0 + r + t.y_org, ih);
        const long long b0 = (long long)y * pitch + lo * a.c, b1 = (long long)y * pitch + (hi + 1) * a.c;
        const long long a0 = b0 & ~3ll;
        const int nd = int((b1 - a0 + 3) >> 2); // <= 33 dwords
        if (lane < nd)
        {
            const long long ad = a0 + 4 * lane;
            uint32_t v;
            if (ad + 4 <= total) v = *reinterpret_cast<const uint32_t*>(img + ad);
            else
            { // the last bytes of the image: never read past its end (inside it, a dword may take in bytes of the row pitch's slack)
                v = 0;
                for (int e = 0; e < 4; e++)
                    if (ad + e < total) v |= (uint32_t)img[ad + e] << (8 * e);
            }
            *reinterpret_cast<uint32_t*>(&raw[r][4 * lane]) = v;
        }
    }
    __syncthreads();
    const float norm_val = 1 / 255.f;
    const int i0 = a.bgr ? 2 : 0, i2 = a.bgr ? 0 : 2;
#pragma unroll
    for (int m = 0; m < 4; m++)
    {
        const int r = (tid >> 5) + 8 * m, cx = tid & 31;
        if (r < ny && cx < nx)
        {
            const int x = reflect101(gx0 + cx + t.x_org, iw);
            const int y = reflect101(gy0 + r + t.y_org, ih);
            const int shift = int(((long long)y * pitch + lo * a.c) & 3);
            const unsigned char* p = &raw[r][shift + (x - lo) * a.c];
            const _Float16 hr = (_Float16)((float)p[i0] * norm_val), hg = (_Float16)((float)p[1] * norm_val), hb = (_Float16)((float)p[i2] * norm_val);
            uint2 v;
            v.x = (uint32_t)__builtin_bit_cast(unsigned short, hr) | ((uint32_t)__builtin_bit_cast(unsigned short, hg) << 16);
            v.y = (uint32_t)__builtin_bit_cast(unsigned short, hb);
            px[r][cx] = v;
        }
    }
    __syncthreads();
    const int nv = a.tta ? 8 : 1;
    const int pi = lane >> 1, half = lane & 1; // lane = (pixel of the output row, 16-byte half of its 32 B)
    for (int k = 0; k < nv; k++)
    {
        const bool tr = k >= 4;                 // transposed variants: an output row runs down a tile column
        const int nrow = tr ? nx : ny, ncol = tr ? ny : nx;
        char* const base = static_cast<char*>(a.in_plane) + (long long)(t.slot0 + k) * a.slot_stride;
        for (int ro = wave; ro < nrow; ro += 4)
        {
            if (pi >= ncol) continue;
            const int r = tr ? pi : ro, cx = tr ? ro : pi;
            const int gx = gx0 + cx, gy = gy0 + r;
            int oy, ox, ow;
            tta_dest(k, gx, gy, t.tw, t.th, oy, ox, ow);
            const uint2 v = px[r][cx];
            const uint4 o = half ? make_uint4(0u, 0u, 0u, 0u) : make_uint4(v.x, v.y, 0u, 0u);
            *reinterpret_cast<uint4*>(base + ((long long)oy * ow + ox) * 32 + half * 16) = o;
        }
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------
// f(T{}) with T = the blob's element type (PostArgs::f32), a surface's sample type, an image's element type; f(integral_constant) with
// the chroma siting: how the launchers below pick these template arguments.  (launch_postproc_box and launch_postproc_area keep a ladder
// of their own: their ALPHA argument exists for the uint8 image only.)
template <typename F>
static void with_blob_type(const PostArgs& a, F f)
{
    if (a.f32) f(float{});
    else f(_Float16{});
}
template <typename F>
static void with_sample_type(int fmt, F f)
{
    if (fmt_yuv_bits(fmt) == 8) f(uint8_t{});
    else f(uint16_t{});
}
template <typename F>
static void with_image_type(int fmt, F f)
{
    if (fmt == kFmtF16) f(_Float16{});
    else if (fmt == kFmtF32) f(float{});
    else if (fmt == kFmtU16) f(uint16_t{});
    else f(uint8_t{});
}
// f(T{}) with T = the sample type of the RGBA source image the alpha of a c == 4 launch is read from (PostArgs::in_fmt)
template <typename F>
static void with_alpha_type(const PostArgs& a, F f)
{
    if (a.c == 4 && a.in_fmt == kFmtU16) f(uint16_t{});
    else f(uint8_t{});
}
template <typename F>
static void with_siting(int siting, F f)
{
    if (siting == 1) f(std::integral_constant<int, 1>{});
    else if (siting == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 0>{});
}
// f(bool_constant DI): the dithering instantiation of a post kernel (PostArgs::dither) or the plain one
template <typename F>
static void with_dither(const PostArgs& a, F f)
{
    if (a.dither) f(std::true_type{});
    else f(std::false_type{});
}
// f(siting, vertical chroma shift VS) of a YUV surface: VS 1 = 4:2:0 with its three sitings; VS 0 = 4:2:2, left or centre -- top-left has no
// vertical meaning there and IS left (the same kernels, the same bytes).  (Semi-planar surfaces: a planar 4:4:4 one has nothing to site.)
template <typename F>
static void with_chroma(int fmt, int siting, F f)
{
    if (!fmt_is_422(fmt)) with_siting(siting, [&](auto site) { f(site, std::integral_constant<int, 1>{}); });
    else if (siting != 0) f(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{});
    else f(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
}

void launch_preproc_tiles(const PreArgs& a, int max_tw, int max_th, hipStream_t st)
{
    if (a.ntiles <= 0) return;
    // Measured (tools/prepost_perf.py, profiles/r04_prepost.txt): 0.042 ms LDS-staged vs 0.032 ms per-pixel on a 1080p frame, 0.145 vs
    // 0.150 ms with the 8 TTA scatters -- the byte loads of the plain kernel are served by the caches, its 32-byte stores are whole
    // sectors: staging buys nothing here.  Default = the plain kernel; variant 2 forces the staged one (tests, A/B).
    bool aligned = true; // (the staged kernel reads the images in dwords, aligned down from any byte offset: only the base matters, not the pitch)
    for (int i = 0; i < a.nimgs; i++) aligned = aligned && !(reinterpret_cast<uintptr_t>(a.imgs[i]) & 3);
    if (a.variant != 2 || a.plane_ch != 16 || !aligned || a.fmt != kFmtU8 || a.alpha_src) // (the staged kernel knows uint8 colour sources only)
    {
        const dim3 grid((max_tw + 31) / 32, (max_th + 7) / 8, a.ntiles), block(256);
        if (a.alpha_src) // (the engine sends c == 4 uint8 / uint16 HWC images only)
        {
            if (a.fmt == kFmtU16) hipLaunchKernelGGL(preproc_tiles<AlphaOf<uint16_t>>, grid, block, 0, st, a);
            else hipLaunchKernelGGL(preproc_tiles<AlphaOf<uint8_t>>, grid, block, 0, st, a);
        }
        else if (fmt_is_444(a.fmt)) // nothing is sited: one kernel per sample type whatever "yuv_siting" says
            with_sample_type(a.fmt, [&](auto src) { hipLaunchKernelGGL((preproc_tiles<decltype(src), true, 0, kVs444>), grid, block, 0, st, a); });
        else if (fmt_is_yuv(a.fmt))
            with_sample_type(a.fmt, [&](auto src) {
                with_chroma(a.fmt, a.siting, [&](auto site, auto vs) {
                    hipLaunchKernelGGL((preproc_tiles<decltype(src), true, decltype(site)::value, decltype(vs)::value>), grid, block, 0, st, a);
                });
            });
        else if (a.fmt == kFmtF16) hipLaunchKernelGGL(preproc_tiles<_Float16>, grid, block, 0, st, a);
        else if (a.fmt == kFmtF32) hipLaunchKernelGGL(preproc_tiles<float>, grid, block, 0, st, a);
        else if (a.fmt == kFmtU16) hipLaunchKernelGGL(preproc_tiles<uint16_t>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(preproc_tiles<uint8_t>, grid, block, 0, st, a);
        return;
    }
    const dim3 grid((max_tw + 31) / 32, (max_th + 31) / 32, a.ntiles), block(256);
    hipLaunchKernelGGL(preproc_tiles_lds, grid, block, 0, st, a);
}

// store conversion of realsr_postproc.comp:71-78 (v + 0.5, floor, clamp 0..255); negative values
// saturate to 0 as on the reference CPU path (GLSL uint(floor(v)) is undefined there).
__device__ __forceinline__ uint8_t post_store(float v)
{
    v = floorf(v + 0.5f);
    v = fminf(fmaxf(v, 0.f), 255.f);
    return (uint8_t)v;
}

// An image of interleaved integer samples (uint8 / uint16 HWC), as opposed to a planar float one: the TO of the post kernels.
template <typename T> constexpr bool is_hwc = std::is_integral<T>::value;

// The uint16 sample (kFmtU16) of d, what RSR_FMT_F32_CHW holds for the pixel, already in [0, 1]: floor(d * 65535 + 0.5), the product and the
// sum rounded by themselves.
__device__ __forceinline__ uint16_t post_store16(float d) { return (uint16_t)floorf(add_rn(mul_rn(d, 65535.f), 0.5f)); }

// ---- ordered dither (engine option "dither": PostArgs::dither) -------------------------------------------------------------------------
// The threshold theta of include/realsr_hip.h ("dither") for the sample at column x, row y of its plane of the OUTPUT IMAGE: the R2 lattice
// in integers, h = x * 0xC13FA9A9 + y * 0x91E10DA5 mod 2^32, k = h >> 25, theta = (2k + 1) / 256 -- two 32-bit multiplications and an add
// per pixel, shared by the pixel's samples; no table, no LDS.  Every post kernel has the template argument DI: false = the kernel as it
// always was (theta_at folds to the 0.5f nobody reads), true = an instantiation of its own that makes theta from the output coordinates
// the thread already holds and hands it to the sample helpers below.
__device__ __forceinline__ float dither_theta(int x, int y)
{
    const unsigned h = (unsigned)x * 0xC13FA9A9u + (unsigned)y * 0x91E10DA5u;
    return (float)(2u * (h >> 25) + 1u) * (1.f / 256.f); // (an integer below 256 times 2^-8: exact)
}
template <bool DI>
__device__ __forceinline__ float theta_at(int x, int y)
{
    if constexpr (DI) return dither_theta(x, y);
    else return 0.5f;
}
// The dithered colour sample of d in [0, 1]: floor(d * M + theta), the product and the sum rounded by themselves.  n + theta is exact for
// every integer n <= M, so a d that is a code keeps it, and d <= 1 gives at most M + 255/256: no clamp is needed.
template <typename TO>
__device__ __forceinline__ TO hwc_dither(float d, float theta)
{
    return (TO)floorf(add_rn(mul_rn(d, sizeof(TO) == 1 ? 255.f : 65535.f), theta));
}
// The colour sample of an HWC image from the value v the uint8 conversion sees (not clamped) ...
template <typename TO, bool DI = false>
__device__ __forceinline__ TO hwc_sample(float v, [[maybe_unused]] float theta = 0.5f)
{
    if constexpr (DI) return hwc_dither<TO>(fminf(fmaxf(v, 0.f), 1.f), theta);
    else if constexpr (sizeof(TO) == 1) return post_store(v * 255.f);
    else return post_store16(fminf(fmaxf(v, 0.f), 1.f));
}
// ... and from a value d in [0, 1] (the box mean, the area average)
template <typename TO, bool DI = false>
__device__ __forceinline__ TO hwc_sample01(float d, [[maybe_unused]] float theta = 0.5f)
{
    if constexpr (DI) return hwc_dither<TO>(d, theta);
    else if constexpr (sizeof(TO) == 1) return post_store(d * 255.f);
    else return post_store16(d);
}
// Alpha: the bicubic value v in the units of the SOURCE's samples (TA) becomes one in the units of the destination's (TO) -- where the
// depths differ, ONE multiplication by 257.f or by fp32(1 / 257) -- then the clamp to [0, max] (alpha_max) and floor(mean + 0.5) (alpha_store).
template <typename TO, typename TA>
__device__ __forceinline__ float alpha_units(float v)
{
    if constexpr (sizeof(TO) > sizeof(TA)) return mul_rn(v, 257.f);
    else if constexpr (sizeof(TO) < sizeof(TA)) return mul_rn(v, 1 / 257.f);
    else return v;
}
template <typename TO> constexpr float alpha_max = sizeof(TO) == 1 ? 255.f : 65535.f;
template <typename TO>
__device__ __forceinline__ TO alpha_store(float v)
{
    if constexpr (sizeof(TO) == 1) return post_store(v);
    else return (uint16_t)fminf(fmaxf(floorf(v + 0.5f), 0.f), 65535.f);
}

// The planar float destinations (PostArgs::out_fmt): the value the uint8 conversion sees, clamped to [0, 1] -- so that
// floor(v * 255 + 0.5) of it is post_store's byte -- as fp32, or rounded once to fp16.  o = element (y, x) of plane 0, the planes
// `plane` bytes apart.
template <typename TO>
__device__ __forceinline__ void post_store_planar(uint8_t* o, long long plane, int bgr, const float (&v)[3])
{
    *reinterpret_cast<TO*>(o + (bgr ? 2 * plane : 0)) = (TO)fminf(fmaxf(v[0], 0.f), 1.f);
    *reinterpret_cast<TO*>(o + plane) = (TO)fminf(fmaxf(v[1], 0.f), 1.f);
    *reinterpret_cast<TO*>(o + (bgr ? 0 : 2 * plane)) = (TO)fminf(fmaxf(v[2], 0.f), 1.f);
}

// ncnn Interp bicubic coefficients (alpha channel only; realsr.cpp:128-140)
__device__ __forceinline__ void cubic_coeffs(int w, int outw, int dx, int& sx, float c[4])
{
    const float scale = (float)w / (float)outw;
    float fx = ((float)dx + 0.5f) * scale - 0.5f;
    sx = (int)floorf(fx);
    fx -= (float)sx;
    const float A = -0.75f;
    const float fx0 = fx + 1.f, fx1 = fx, fx2 = 1.f - fx;
    c[0] = A * fx0 * fx0 * fx0 - 5.f * A * fx0 * fx0 + 8.f * A * fx0 - 4.f * A;
    c[1] = (A + 2.f) * fx1 * fx1 * fx1 - (A + 3.f) * fx1 * fx1 + 1.f;
    c[2] = (A + 2.f) * fx2 * fx2 * fx2 - (A + 3.f) * fx2 * fx2 + 1.f;
    c[3] = 1.f - c[0] - c[1] - c[2];
    if (sx <= -1) { sx = 1; c[0] = 1.f - c[3]; c[1] = c[3]; c[2] = 0.f; c[3] = 0.f; }
    if (sx == 0) { sx = 1; c[0] = c[0] + c[1]; c[1] = c[2]; c[2] = c[3]; c[3] = 0.f; }
    if (sx == w - 2) { sx = w - 3; c[3] = c[2] + c[3]; c[2] = c[1]; c[1] = c[0]; c[0] = 0.f; }
    if (sx >= w - 1) { sx = w - 3; c[3] = 1.f - c[0]; c[2] = c[0]; c[1] = 0.f; c[0] = 0.f; }
}

__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// The bicubic x4 alpha value (in the units of the source's samples TA: 0..255, or 0..65535 of a uint16 image; not clamped) of a tile's kept
// rectangle -- realsr.cpp:431-442, realsr_preproc.comp:79-88 (crop), realsr_postproc.comp:58-61 -- from the coefficient sets cubic_coeffs made
// for its column (bx, cx) and row (by, cy): four rows of four taps of the RGBA source image, indices clamped to the rectangle.
// postproc_tiles, postproc_tiles_lds, postproc_tiles_box and postproc_tiles_area; a kernel that needs one row's coefficients for several
// pixels makes them once, at its call site.
// A uint8 source keeps the expression it always had (the compiler contracts it as it likes: a sum of four 20-bit products barely rounds).
// A uint16 source has 16 more bits to lose, so its sums are pinned: ((p0 c0 + p1 c1) + p2 c2) + p3 c3, every product and sum rounded by
// itself (dot4_rn) -- the definition of include/realsr_hip.h, which tests/rgb16_ref.py restates.
__device__ __forceinline__ float dot4_rn(float p0, float p1, float p2, float p3, const float (&c)[4])
{
    return add_rn(add_rn(add_rn(mul_rn(p0, c[0]), mul_rn(p1, c[1])), mul_rn(p2, c[2])), mul_rn(p3, c[3]));
}
template <typename TA = uint8_t>
__device__ __forceinline__ float alpha_bicubic(const PostArgs& a, const BaseTile& t, int im, int bx, const float (&cx)[4], int by, const float (&cy)[4])
{
    const int aw = t.out_w / 4, ah = t.out_h / 4;
    const int ax0 = t.out_x / 4, ay0 = t.out_y / 4;
    float rows[4];
#pragma unroll
    for (int j = 0; j < 4; j++)
    {
        const int yy = ay0 + clampi(by - 1 + j, ah);
        const TA* rp = reinterpret_cast<const TA*>(a.in_imgs[im] + (long long)yy * a.in_pitch[im]) + ax0 * 4 + 3;
        if constexpr (sizeof(TA) != 1)
            rows[j] = dot4_rn((float)rp[clampi(bx - 1, aw) * 4], (float)rp[clampi(bx, aw) * 4], (float)rp[clampi(bx + 1, aw) * 4], (float)rp[clampi(bx + 2, aw) * 4], cx);
        else
            rows[j] = (float)rp[clampi(bx - 1, aw) * 4] * cx[0] + (float)rp[clampi(bx, aw) * 4] * cx[1] +
                      (float)rp[clampi(bx + 1, aw) * 4] * cx[2] + (float)rp[clampi(bx + 2, aw) * 4] * cx[3];
    }
    if constexpr (sizeof(TA) != 1) return dot4_rn(rows[0], rows[1], rows[2], rows[3], cy);
    else return rows[0] * cy[0] + rows[1] * cy[1] + rows[2] * cy[2] + rows[3] * cy[3];
}

// K contiguous blob elements, K-element aligned: ONE 4- / 8-byte (fp16) or 8- / 16-byte (fp32) load.
template <typename TP, int K>
__device__ __forceinline__ void load_run(const TP* p, float (&o)[K])
{
    typedef TP vec __attribute__((ext_vector_type(K)));
    const vec v = *reinterpret_cast<const vec*>(p);
#pragma unroll
    for (int i = 0; i < K; i++) o[i] = (float)v[i];
}

// The K x K block of x4 pixels at (sx, sy) of one channel's blob b (w x h, the TTA variants ss elements apart): under TTA the eight
// variants merged as realsr_postproc_tta.comp:76-85 does, (v0 + v1 + ... + v7) * 0.125f in this order.  The only place that knows the
// eight source addresses.  sx and the row length are multiples of K: every run of K elements is ONE load (load_run) -- also in the
// mirrored variants (the run is read backwards) and in the TRANSPOSED ones, where a run lies along y.  postproc_tiles (K = 1), and
// through merged_block every box, area and YUV kernel; postproc_tiles_lds stages the transposed variants in LDS instead.
template <typename TP, int K>
__device__ __forceinline__ void tta_gather(const TP* b, long long ss, int w, int h, int sx, int sy, int tta, float (&c)[K][K])
{
    float r[K];
#pragma unroll
    for (int j = 0; j < K; j++)
    {
        load_run<TP, K>(b + (long long)(sy + j) * w + sx, r);
#pragma unroll
        for (int i = 0; i < K; i++) c[j][i] = r[i];
    }
    if (!tta) return;
#pragma unroll
    for (int j = 0; j < K; j++)
    {
        load_run<TP, K>(b + ss + (long long)(sy + j) * w + (w - K - sx), r);
#pragma unroll
        for (int i = 0; i < K; i++) c[j][i] += r[K - 1 - i];
    }
#pragma unroll
    for (int j = 0; j < K; j++)
    {
        load_run<TP, K>(b + 2 * ss + (long long)(h - 1 - sy - j) * w + (w - K - sx), r);
#pragma unroll
        for (int i = 0; i < K; i++) c[j][i] += r[K - 1 - i];
    }
#pragma unroll
    for (int j = 0; j < K; j++)
    {
        load_run<TP, K>(b + 3 * ss + (long long)(h - 1 - sy - j) * w + sx, r);
#pragma unroll
        for (int i = 0; i < K; i++) c[j][i] += r[i];
    }
#pragma unroll
    for (int i = 0; i < K; i++)
    {
        load_run<TP, K>(b + 4 * ss + (long long)(sx + i) * h + sy, r);
#pragma unroll
        for (int j = 0; j < K; j++) c[j][i] += r[j];
    }
#pragma unroll
    for (int i = 0; i < K; i++)
    {
        load_run<TP, K>(b + 5 * ss + (long long)(sx + i) * h + (h - K - sy), r);
#pragma unroll
        for (int j = 0; j < K; j++) c[j][i] += r[K - 1 - j];
    }
#pragma unroll
    for (int i = 0; i < K; i++)
    {
        load_run<TP, K>(b + 6 * ss + (long long)(w - 1 - sx - i) * h + (h - K - sy), r);
#pragma unroll
        for (int j = 0; j < K; j++) c[j][i] += r[K - 1 - j];
    }
#pragma unroll
    for (int i = 0; i < K; i++)
    {
        load_run<TP, K>(b + 7 * ss + (long long)(w - 1 - sx - i) * h + sy, r);
#pragma unroll
        for (int j = 0; j < K; j++) c[j][i] += r[j];
    }
#pragma unroll
    for (int j = 0; j < K; j++)
#pragma unroll
        for (int i = 0; i < K; i++) c[j][i] *= 0.125f;
}

// tta_gather's block clamped to [0, 1]: the x4 pixels every reduced output is made of (postproc_tiles_box, postproc_tiles_area through
// area_pixel, and the two YUV kernels).
template <typename TP, int K>
__device__ __forceinline__ void merged_block(const TP* b, long long ss, int w, int h, int sx, int sy, int tta, float (&c)[K][K])
{
    tta_gather<TP, K>(b, ss, w, h, sx, sy, tta, c);
#pragma unroll
    for (int j = 0; j < K; j++)
#pragma unroll
        for (int i = 0; i < K; i++) c[j][i] = fminf(fmaxf(c[j][i], 0.f), 1.f);
}

// realsr_postproc.comp:47-89 and realsr_postproc_tta.comp:54-110 for a batch of tiles.
// One thread per output pixel of the tile's un-padded x4 rectangle.
// TP: element type of the planar blob: _Float16 (the reference's `output` blob) or float (precise mode)
// TO: element type of the image: uint8_t / uint16_t (HWC), or _Float16 / float (planar [3][out_hs][out_ws], RGB only: post_store_planar)
// TA: sample type of the RGBA source image the alpha is read from (c == 4; uint8_t or uint16_t, whatever TO is)
// DI: the colour samples of an HWC image are dithered (theta_at; the pixel's three share one threshold, the alpha has none)
template <typename TP, typename TO, typename TA = uint8_t, bool DI = false>
__global__ __launch_bounds__(256) void postproc_tiles(const PostArgs a)
{
    const BaseTile t = a.tiles[blockIdx.z];
    const int im = __builtin_amdgcn_readfirstlane(t.img);
    const int gx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int gy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (gx >= t.out_w || gy >= t.out_h) return;
    const int w = t.tw * 4, h = t.th * 4;
    const long long cstep = (long long)w * h;
    const TP* b0 = reinterpret_cast<const TP*>(static_cast<const char*>(a.planar3) + (long long)t.slot0 * a.slot_stride);
    const long long ss = a.slot_stride / (long long)sizeof(TP);
    const int sx = gx + a.crop, sy = gy + a.crop;
    float v[3];
    if (!a.tta)
    { // (a branch of its own: the three loads leave together, with no test of a.tta between them)
#pragma unroll
        for (int q = 0; q < 3; q++) v[q] = (float)b0[q * cstep + (long long)sy * w + sx];
    }
    else
    {
#pragma unroll
        for (int q = 0; q < 3; q++)
        {
            float c[1][1];
            tta_gather<TP, 1>(b0 + q * cstep, ss, w, h, sx, sy, 1, c);
            v[q] = c[0][0];
        }
    }
    if constexpr (!is_hwc<TO>)
    {
        uint8_t* o = a.outs[im] + (long long)(t.out_y - a.out_row0 + gy) * a.out_pitch[im] + (long long)(t.out_x + gx) * (int)sizeof(TO);
        post_store_planar<TO>(o, a.out_plane[im], a.bgr, v);
        return;
    }
    else
    {
        TO* o = reinterpret_cast<TO*>(a.outs[im] + (long long)(t.out_y - a.out_row0 + gy) * a.out_pitch[im]) + (t.out_x + gx) * a.c;
        const float th = theta_at<DI>(t.out_x + gx, t.out_y + gy);
        const TO r = hwc_sample<TO, DI>(v[0], th), g = hwc_sample<TO, DI>(v[1], th), bl = hwc_sample<TO, DI>(v[2], th);
        o[a.bgr ? 2 : 0] = r;
        o[1] = g;
        o[a.bgr ? 0 : 2] = bl;
        if (a.c == 4)
        {
            int bx, by;
            float cx[4], cy[4];
            cubic_coeffs(t.out_w / 4, t.out_w, gx, bx, cx);
            cubic_coeffs(t.out_h / 4, t.out_h, gy, by, cy);
            o[3] = alpha_store<TO>(alpha_units<TO, TA>(alpha_bicubic<TA>(a, t, im, bx, cx, by, cy)));
        }
    }
}

// realsr_postproc{,_tta}.comp with coalesced traffic (round 4; byte-identical to the kernel above; the default under TTA):
// one workgroup = a 32 x 32 block of the tile's kept output rectangle, 4 pixels per thread.  The four plain TTA variants are
// read along their rows (lanes along x, forwards or backwards: contiguous either way).  The four TRANSPOSED variants store pixel
// (sx, sy) at [sx][sy]: read naively, a wave touches 64 different cache lines for 128 useful bytes -- here each (variant,
// channel) block is read along ITS rows into an LDS tile and picked up transposed (34-half pitch: conflict-free).  The merge keeps
// the shader's summation order (v0 + v1 + ... + v7) * 0.125.  The uint8 pixels are collected in LDS and leave as aligned dwords
// (a 32-pixel row segment of the HWC image = 96 or 128 contiguous bytes).
// TO != uint8_t (planar float image): lanes run along x, so the values leave straight from the registers, 32 contiguous elements per
// channel row, and the uint8 staging at the end is not needed.
// DI (uint8 image): the colour bytes are dithered on their way into the staging rows.
template <typename TP, typename TO, bool DI = false>
__global__ __launch_bounds__(256) void postproc_tiles_lds(const PostArgs a)
{
    __shared__ TP T[32][sizeof(TP) == 2 ? 34 : 33]; // pitch: conflict-free column reads for 2- and 4-byte elements
    __shared__ __attribute__((aligned(16))) unsigned char ob[32][128];
    const BaseTile t = a.tiles[blockIdx.z];
    const int im = __builtin_amdgcn_readfirstlane(t.img);
    const int gx0 = blockIdx.x * 32, gy0 = blockIdx.y * 32;
    if (gx0 >= t.out_w || gy0 >= t.out_h) return;
    const int nx = min(32, t.out_w - gx0), ny = min(32, t.out_h - gy0);
    const int tid = threadIdx.x, lx = tid & 31, ly = tid >> 5;
    const int w = t.tw * 4, h = t.th * 4;
    const long long cstep = (long long)w * h;
    const TP* b0 = reinterpret_cast<const TP*>(static_cast<const char*>(a.planar3) + (long long)t.slot0 * a.slot_stride);
    const long long ss = a.slot_stride / (long long)sizeof(TP);
    float acc[4][3];
    const int sx = gx0 + lx + a.crop;
#pragma unroll
    for (int m = 0; m < 4; m++)
    {
        const int gyl = ly + 8 * m, sy = gy0 + gyl + a.crop;
        const bool ok = lx < nx && gyl < ny;
#pragma unroll
        for (int q = 0; q < 3; q++)
        {
            float v = 0.f;
            if (ok)
            {
                const TP* b = b0 + q * cstep;
                v = (float)b[(long long)sy * w + sx];
                if (a.tta)
                { // realsr_postproc_tta.comp:76-79
                    v += (float)b[ss + (long long)sy * w + (w - 1 - sx)];
                    v += (float)b[2 * ss + (long long)(h - 1 - sy) * w + (w - 1 - sx)];
                    v += (float)b[3 * ss + (long long)(h - 1 - sy) * w + sx];
                }
            }
            acc[m][q] = v;
        }
    }
    if (a.tta)
    {
        for (int k = 4; k < 8; k++)
            for (int q = 0; q < 3; q++)
            {
                __syncthreads(); // the previous tile has been consumed
                const TP* b = b0 + k * ss + q * cstep;
#pragma unroll
                for (int m = 0; m < 4; m++)
                {
                    const int ai = ly + 8 * m, bi = lx; // local (sx, sy) of the element this thread fetches: lanes along sy = along the row
                    if (ai < nx && bi < ny)
                    {
                        const int ex = gx0 + ai + a.crop, ey = gy0 + bi + a.crop;
                        long long off; // realsr_postproc_tta.comp:80-83
                        if (k == 4) off = (long long)ex * h + ey;
                        else if (k == 5) off = (long long)ex * h + (h - 1 - ey);
                        else if (k == 6) off = (long long)(w - 1 - ex) * h + (h - 1 - ey);
                        else off = (long long)(w - 1 - ex) * h + ey;
                        T[ai][bi] = b[off];
                    }
                }
                __syncthreads();
#pragma unroll
                for (int m = 0; m < 4; m++)
                {
                    const int gyl = ly + 8 * m;
                    if (lx < nx && gyl < ny) acc[m][q] += (float)T[lx][gyl];
                }
            }
    }
#pragma unroll
    for (int m = 0; m < 4; m++)
    {
        const int gyl = ly + 8 * m;
        if (!(lx < nx && gyl < ny)) continue;
        float v[3];
#pragma unroll
        for (int q = 0; q < 3; q++) v[q] = a.tta ? acc[m][q] * 0.125f : acc[m][q];
        if constexpr (sizeof(TO) != 1)
        {
            uint8_t* o = a.outs[im] + (long long)(t.out_y - a.out_row0 + gy0 + gyl) * a.out_pitch[im] + (long long)(t.out_x + gx0 + lx) * (int)sizeof(TO);
            post_store_planar<TO>(o, a.out_plane[im], a.bgr, v);
            continue;
        }
        unsigned char* o = &ob[gyl][lx * a.c];
        if constexpr (DI)
        {
            const float th = dither_theta(t.out_x + gx0 + lx, t.out_y + gy0 + gyl);
            o[a.bgr ? 2 : 0] = hwc_sample<uint8_t, true>(v[0], th);
            o[1] = hwc_sample<uint8_t, true>(v[1], th);
            o[a.bgr ? 0 : 2] = hwc_sample<uint8_t, true>(v[2], th);
        }
        else
        {
            o[a.bgr ? 2 : 0] = post_store(v[0] * 255.f);
            o[1] = post_store(v[1] * 255.f);
            o[a.bgr ? 0 : 2] = post_store(v[2] * 255.f);
        }
        if (a.c == 4)
        {
            int bx, by;
            float cx[4], cy[4];
            cubic_coeffs(t.out_w / 4, t.out_w, gx0 + lx, bx, cx);
            cubic_coeffs(t.out_h / 4, t.out_h, gy0 + gyl, by, cy);
            o[3] = post_store(alpha_bicubic(a, t, im, bx, cx, by, cy));
        }
    }
    if constexpr (sizeof(TO) != 1) return;
    __syncthreads();
    const int nd = nx * a.c / 4; // out_w, gx0 are multiples of 4: a row segment is whole dwords, 4-byte aligned in the image (base and pitch: launch_postproc_tiles)
    for (int i = tid; i < ny * nd; i += 256)
    {
        const int r = i / nd, d = i - r * nd;
        uint8_t* o = a.outs[im] + (long long)(t.out_y - a.out_row0 + gy0 + r) * a.out_pitch[im] + (t.out_x + gx0) * a.c;
        reinterpret_cast<uint32_t*>(o)[d] = reinterpret_cast<const uint32_t*>(&ob[r][0])[d];
    }
}

// postproc_tiles for a uint16 image with TWO neighbouring pixels per thread (the default without TTA; PostArgs::variant 1 / 2 force one / two
// pixels; bytes equal to postproc_tiles<., uint16_t>): the pair's 12 bytes (C = 3) leave as three dword stores, its 16 bytes (C = 4) as two 8-byte stores, where
// the address allows -- a tile's rectangle starts on a multiple of 4 pixels, so only the image's own base and row pitch decide --, else
// as samples.  The blob's two elements are ONE load (the kept rectangle and the crop are multiples of 4: the run is 2-aligned).
// DI: each of the two pixels has its own threshold.
template <typename TP, int C, typename TA = uint8_t, bool DI = false>
__global__ __launch_bounds__(256) void postproc_tiles_u16x2(const PostArgs a)
{
    const BaseTile t = a.tiles[blockIdx.z];
    const int im = __builtin_amdgcn_readfirstlane(t.img);
    const int gx = (blockIdx.x * 64 + (threadIdx.x & 63)) * 2;
    const int gy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (gx >= t.out_w || gy >= t.out_h) return;
    const int w = t.tw * 4, h = t.th * 4;
    const long long cstep = (long long)w * h;
    const TP* b0 = reinterpret_cast<const TP*>(static_cast<const char*>(a.planar3) + (long long)t.slot0 * a.slot_stride);
    const long long ss = a.slot_stride / (long long)sizeof(TP);
    const int sx = gx + a.crop, sy = gy + a.crop;
    unsigned s[3][2]; // [channel of the blob][pixel]
    const float th0 = theta_at<DI>(t.out_x + gx, t.out_y + gy), th1 = theta_at<DI>(t.out_x + gx + 1, t.out_y + gy);
#pragma unroll
    for (int q = 0; q < 3; q++)
    {
        float v[2];
        if (!a.tta) load_run<TP, 2>(b0 + q * cstep + (long long)sy * w + sx, v);
        else
        {
#pragma unroll
            for (int i = 0; i < 2; i++)
            {
                float c[1][1];
                tta_gather<TP, 1>(b0 + q * cstep, ss, w, h, sx + i, sy, 1, c);
                v[i] = c[0][0];
            }
        }
        s[q][0] = hwc_sample<uint16_t, DI>(v[0], th0), s[q][1] = hwc_sample<uint16_t, DI>(v[1], th1);
    }
    const unsigned f0 = a.bgr ? s[2][0] : s[0][0], l0 = a.bgr ? s[0][0] : s[2][0], f1 = a.bgr ? s[2][1] : s[0][1], l1 = a.bgr ? s[0][1] : s[2][1];
    uint8_t* o = a.outs[im] + (long long)(t.out_y - a.out_row0 + gy) * a.out_pitch[im] + (long long)(t.out_x + gx) * (2 * C);
    if constexpr (C == 3)
    {
        if (!(reinterpret_cast<uintptr_t>(o) & 3))
        {
            unsigned* d = reinterpret_cast<unsigned*>(o);
            d[0] = f0 | (s[1][0] << 16), d[1] = l0 | (f1 << 16), d[2] = s[1][1] | (l1 << 16);
        }
        else
        {
            unsigned short* d = reinterpret_cast<unsigned short*>(o);
            d[0] = f0, d[1] = s[1][0], d[2] = l0, d[3] = f1, d[4] = s[1][1], d[5] = l1;
        }
    }
    else
    {
        int by;
        float cy[4];
        cubic_coeffs(t.out_h / 4, t.out_h, gy, by, cy);
        unsigned al[2];
#pragma unroll
        for (int i = 0; i < 2; i++)
        {
            int bx;
            float cx[4];
            cubic_coeffs(t.out_w / 4, t.out_w, gx + i, bx, cx);
            al[i] = alpha_store<uint16_t>(alpha_units<uint16_t, TA>(alpha_bicubic<TA>(a, t, im, bx, cx, by, cy)));
        }
        if (!(reinterpret_cast<uintptr_t>(o) & 7))
        {
            uint2* d = reinterpret_cast<uint2*>(o);
            d[0] = make_uint2(f0 | (s[1][0] << 16), l0 | (al[0] << 16)), d[1] = make_uint2(f1 | (s[1][1] << 16), l1 | (al[1] << 16));
        }
        else
        {
            unsigned short* d = reinterpret_cast<unsigned short*>(o);
            d[0] = f0, d[1] = s[1][0], d[2] = l0, d[3] = al[0], d[4] = f1, d[5] = s[1][1], d[6] = l1, d[7] = al[1];
        }
    }
}

// ---- box-reduced output (engine option "out_scale" 2 / 1: PostArgs::box = K = 2 / 4) ----------------------------------------
// The fp32 mean of a K x K box c[y][x] in the fixed order of include/realsr_hip.h ("out_scale"): pairs along x, then pairs of rows.
// Plain adds and one multiplication by a power of two behind them: nothing a contraction could change.
template <int K>
__device__ __forceinline__ float box_mean(const float (&c)[K][K])
{
    if constexpr (K == 2) return ((c[0][0] + c[0][1]) + (c[1][0] + c[1][1])) * 0.25f;
    else
    {
        float s[4];
#pragma unroll
        for (int j = 0; j < 4; j++) s[j] = (c[j][0] + c[j][1]) + (c[j][2] + c[j][3]);
        return ((s[0] + s[1]) + (s[2] + s[3])) * 0.0625f;
    }
}

// The box-reducing sibling of postproc_tiles: one thread makes ONE pixel of the (4 / K)x image -- the mean of the K x K box of x4
// pixels min(max(r, 0), 1), r what postproc_tiles converts (TTA: the eight variants merged first, in the shader's order).  A tile's
// kept x4 rectangle starts and ends on multiples of 4 (BaseTile::out_*), so no box crosses a tile; BaseTile stays in x4 units and is
// divided by K here.  Lanes run along x.  The K elements a thread needs of a blob row are contiguous and K-aligned (crop, the row
// length 4 * tw and the plane size are multiples of 4): merged_block fetches each run with one load.
// ALPHA: the uint8 / uint16 image is RGBA (PostArgs::c == 4; a kernel of its own: the bicubic's registers stay out of the RGB path); TA the
// sample type of the RGBA source.  DI: the colour samples are dithered at the pixel's place (t.out_x / K + gx, t.out_y / K + gy) of the reduced image.
template <typename TP, typename TO, int K, bool ALPHA, typename TA = uint8_t, bool DI = false>
__global__ __launch_bounds__(256) void postproc_tiles_box(const PostArgs a)
{
    const BaseTile t = a.tiles[blockIdx.z];
    const int im = __builtin_amdgcn_readfirstlane(t.img);
    const int gx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int gy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (gx >= t.out_w / K || gy >= t.out_h / K) return;
    const int w = t.tw * 4, h = t.th * 4;
    const long long cstep = (long long)w * h;
    const int sx = gx * K + a.crop, sy = gy * K + a.crop; // first x4 pixel of the box, in the blob
    const TP* b0 = reinterpret_cast<const TP*>(static_cast<const char*>(a.planar3) + (long long)t.slot0 * a.slot_stride);
    const long long ss = a.slot_stride / (long long)sizeof(TP);
    constexpr int es = (int)sizeof(TO);
    uint8_t* const o = a.outs[im] + ((t.out_y - a.out_row0) / K + gy) * (long long)a.out_pitch[im] + (long long)(t.out_x / K + gx) * (is_hwc<TO> ? a.c * es : es);
    [[maybe_unused]] const float th = theta_at<DI>(t.out_x / K + gx, t.out_y / K + gy);
#pragma unroll 1 // (one channel at a time: unrolled, the loads of all three are hoisted to the top and cost three times the registers)
    for (int q = 0; q < 3; q++)
    {
        float c[K][K];
        merged_block<TP, K>(b0 + q * cstep, ss, w, h, sx, sy, a.tta, c);
        const float d = box_mean<K>(c); // in [0, 1] like its sixteen / four terms
        const int qo = a.bgr ? 2 - q : q;
        if constexpr (!is_hwc<TO>) *reinterpret_cast<TO*>(o + qo * a.out_plane[im]) = (TO)d;
        else reinterpret_cast<TO*>(o)[qo] = hwc_sample01<TO, DI>(d, th);
    }
    if constexpr (ALPHA)
    { // alpha: the box mean of postproc_tiles' bicubic x4 value, each clamped to [0, 255] first; two box rows per turn: (s0 + s1) [+ (s2 + s3)]
        float tot = 0.f;
#pragma unroll 1
        for (int p = 0; p < K / 2; p++)
        {
            float s2[2];
#pragma unroll
            for (int jj2 = 0; jj2 < 2; jj2++)
            {
                float al[K];
                int by;
                float cy[4];
                cubic_coeffs(t.out_h / 4, t.out_h, gy * K + 2 * p + jj2, by, cy); // (of the row alone: once per box row, not per pixel)
#pragma unroll
                for (int i = 0; i < K; i++)
                {
                    int bx;
                    float cx[4];
                    cubic_coeffs(t.out_w / 4, t.out_w, gx * K + i, bx, cx);
                    const float av = alpha_units<TO, TA>(alpha_bicubic<TA>(a, t, im, bx, cx, by, cy));
                    al[i] = fminf(fmaxf(av, 0.f), alpha_max<TO>);
                }
                if constexpr (K == 2) s2[jj2] = al[0] + al[1];
                else s2[jj2] = (al[0] + al[1]) + (al[2] + al[3]);
            }
            const float tp = s2[0] + s2[1];
            tot = p == 0 ? tp : tot + tp;
        }
        reinterpret_cast<TO*>(o)[3] = alpha_store<TO>(tot * (K == 2 ? 0.25f : 0.0625f));
    }
}

template <typename TP, int K>
static void launch_postproc_box(const PostArgs& a, int max_ow, int max_oh, hipStream_t st)
{
    const dim3 grid((max_ow / K + 63) / 64, (max_oh / K + 3) / 4, a.ntiles), block(256);
    if (a.out_fmt == kFmtF16) hipLaunchKernelGGL((postproc_tiles_box<TP, _Float16, K, false>), grid, block, 0, st, a);
    else if (a.out_fmt == kFmtF32) hipLaunchKernelGGL((postproc_tiles_box<TP, float, K, false>), grid, block, 0, st, a);
    else
        with_dither(a, [&](auto di) {
            constexpr bool DI = decltype(di)::value;
            if (a.out_fmt == kFmtU16 && a.c == 4)
                with_alpha_type(a, [&](auto ta) { hipLaunchKernelGGL((postproc_tiles_box<TP, uint16_t, K, true, decltype(ta), DI>), grid, block, 0, st, a); });
            else if (a.out_fmt == kFmtU16) hipLaunchKernelGGL((postproc_tiles_box<TP, uint16_t, K, false, uint8_t, DI>), grid, block, 0, st, a);
            else if (a.c == 4 && a.in_fmt == kFmtU16) hipLaunchKernelGGL((postproc_tiles_box<TP, uint8_t, K, true, uint16_t, DI>), grid, block, 0, st, a);
            else if (a.c == 4) hipLaunchKernelGGL((postproc_tiles_box<TP, uint8_t, K, true, uint8_t, DI>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((postproc_tiles_box<TP, uint8_t, K, false, uint8_t, DI>), grid, block, 0, st, a);
        });
}

// ---- area-averaged output at a rational scale (rsr_set_out_ratio: PostArgs::num / den, e.g. 3/2, 4/3, 9/4, 3/1) -------------------------
// The area-average loop nest of output pixel (X, Y) of a tile's rectangle at the scale n / d, L = 4 d -- per axis: (nx, Lx) along x,
// (ny, Ly) along y (rsr_set_out_ratio_xy; one ratio on both axes passes it twice).  On the integer grid where x4
// pixel i covers [i n, (i + 1) n) and output pixel X covers [X L, (X + 1) L), its taps along an axis are i = floor(X L / n) ..
// floor(((X + 1) L - 1) / n) -- at most 4 (d <= 4) or 5 (d <= 8) -- with the integer weights g_i = the overlap, which sum to L.  include/realsr_hip.h
// (rsr_set_out_ratio) fixes the arithmetic: horizontally H = g c, H = H + g c in ascending i, then vertically the same over the rows' H,
// every product and sum rounded by itself.  row(j), called once per tap row, returns that row's tap function: tap(i) is the value c of
// x4 pixel (i, j) of the tile's kept rectangle.  The caller multiplies the sum V it gets by fp32(1 / (16 dx dy)).
// The ratio is a runtime argument: the tap loops have no arrays to index, so nothing is gained by unrolling them per ratio.
// Used by area_pixel (colour) and by postproc_tiles_area's alpha.
template <typename ROW>
__device__ __forceinline__ float area_sum(int nx, int Lx, int ny, int Ly, int X, int Y, ROW row)
{
    const int x0 = X * Lx, x1 = x0 + Lx, y0 = Y * Ly, y1 = y0 + Ly;                   // the pixel's footprint on the two grids
    const int ix0 = x0 / nx, ix1 = (x1 - 1) / nx, iy0 = y0 / ny, iy1 = (y1 - 1) / ny; // its taps
    float V = 0.f;
#pragma unroll 1
    for (int j = iy0; j <= iy1; j++)
    {
        const auto tap = row(j);
        float H = 0.f;
#pragma unroll 1
        for (int i = ix0; i <= ix1; i++)
        {
            const float p = mul_rn((float)(min(x1, (i + 1) * nx) - max(x0, i * nx)), tap(i));
            H = i == ix0 ? p : add_rn(H, p);
        }
        const float p = mul_rn((float)(min(y1, (j + 1) * ny) - max(y0, j * ny)), H);
        V = j == iy0 ? p : add_rn(V, p);
    }
    return V;
}

// ONE pixel d(X, Y) of a tile's output rectangle at the scales nx / dx, ny / dy of one channel's blob -- what RSR_FMT_F32_CHW holds for it: every tap
// clamped to [0, 1] (TTA: the eight variants merged first), fetched one at a time through merged_block<TP, 1>, and m = min(V * norm, 1).
// (X, Y) are the tile's own coordinates, which are the image's.  postproc_tiles_area and postproc_tiles_yuv_area.
template <typename TP>
__device__ __forceinline__ float area_pixel(const TP* b, long long ss, int w, int h, int crop, int tta, int nx, int Lx, int ny, int Ly, float norm, int X, int Y)
{
    const float V = area_sum(nx, Lx, ny, Ly, X, Y, [&](int j) {
        return [&, j](int i) {
            float c[1][1];
            merged_block<TP, 1>(b, ss, w, h, i + crop, j + crop, tta, c);
            return c[0][0];
        };
    });
    return fminf(mul_rn(V, norm), 1.f);
}

// The sibling of postproc_tiles_box for the scales n / d that are not 4, 2 or 1: one thread makes ONE output pixel (X, Y) of the tile's
// rectangle, area_pixel per channel.  A tile's kept x4 rectangle starts on a multiple of L grid units (the engine refuses the call
// otherwise: tilesize * n is a multiple of d, on each axis with its own n / d), so the tile's own coordinates are the image's and no footprint crosses a tile.  Lanes run
// along x, so a wave's loads of one tap row fall into a few cache lines.  One channel at a time, as in the box kernel.
// ALPHA: PostArgs::c == 4, the bicubic x4 alpha, clamped to [0, 255] ([0, 65535] of a uint16 image), under the same weights, order and
// constant; TA the sample type of the RGBA source.  DI: the colour samples are dithered at the pixel's place in the output image.
template <typename TP, typename TO, bool ALPHA, typename TA = uint8_t, bool DI = false>
__global__ __launch_bounds__(256) void postproc_tiles_area(const PostArgs a)
{
    const BaseTile t = a.tiles[blockIdx.z];
    const int im = __builtin_amdgcn_readfirstlane(t.img);
    const int nx = a.num, Lx = 4 * a.den, ny = a.num_y, Ly = 4 * a.den_y;
    const int gx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int gy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (gx >= t.out_w * nx / Lx || gy >= t.out_h * ny / Ly) return;
    const int w = t.tw * 4, h = t.th * 4;
    const long long cstep = (long long)w * h;
    const TP* b0 = reinterpret_cast<const TP*>(static_cast<const char*>(a.planar3) + (long long)t.slot0 * a.slot_stride);
    const long long ss = a.slot_stride / (long long)sizeof(TP);
    constexpr int es = (int)sizeof(TO);
    uint8_t* const o = a.outs[im] + ((long long)(t.out_y - a.out_row0) * ny / Ly + gy) * (long long)a.out_pitch[im] +
                       ((long long)t.out_x * nx / Lx + gx) * (is_hwc<TO> ? a.c * es : es);
    [[maybe_unused]] const float th = theta_at<DI>(int((long long)t.out_x * nx / Lx) + gx, int((long long)t.out_y * ny / Ly) + gy);
#pragma unroll 1
    for (int q = 0; q < 3; q++)
    {
        const float m = area_pixel<TP>(b0 + q * cstep, ss, w, h, a.crop, a.tta, nx, Lx, ny, Ly, a.area_norm, gx, gy);
        const int qo = a.bgr ? 2 - q : q;
        if constexpr (!is_hwc<TO>) *reinterpret_cast<TO*>(o + qo * a.out_plane[im]) = (TO)m;
        else reinterpret_cast<TO*>(o)[qo] = hwc_sample01<TO, DI>(m, th);
    }
    if constexpr (ALPHA)
    {
        const float V = area_sum(nx, Lx, ny, Ly, gx, gy, [&](int j) {
            int by;
            float cy[4];
            cubic_coeffs(t.out_h / 4, t.out_h, j, by, cy);
            return [&, by, cy](int i) {
                int bx;
                float cx[4];
                cubic_coeffs(t.out_w / 4, t.out_w, i, bx, cx);
                return fminf(fmaxf(alpha_units<TO, TA>(alpha_bicubic<TA>(a, t, im, bx, cx, by, cy)), 0.f), alpha_max<TO>);
            };
        });
        reinterpret_cast<TO*>(o)[3] = alpha_store<TO>(mul_rn(V, a.area_norm));
    }
}

template <typename TP>
static void launch_postproc_area(const PostArgs& a, int max_ow, int max_oh, hipStream_t st)
{
    const int Lx = 4 * a.den, Ly = 4 * a.den_y;
    const dim3 grid((max_ow * a.num / Lx + 63) / 64, (max_oh * a.num_y / Ly + 3) / 4, a.ntiles), block(256);
    if (a.out_fmt == kFmtF16) hipLaunchKernelGGL((postproc_tiles_area<TP, _Float16, false>), grid, block, 0, st, a);
    else if (a.out_fmt == kFmtF32) hipLaunchKernelGGL((postproc_tiles_area<TP, float, false>), grid, block, 0, st, a);
    else
        with_dither(a, [&](auto di) {
            constexpr bool DI = decltype(di)::value;
            if (a.out_fmt == kFmtU16 && a.c == 4)
                with_alpha_type(a, [&](auto ta) { hipLaunchKernelGGL((postproc_tiles_area<TP, uint16_t, true, decltype(ta), DI>), grid, block, 0, st, a); });
            else if (a.out_fmt == kFmtU16) hipLaunchKernelGGL((postproc_tiles_area<TP, uint16_t, false, uint8_t, DI>), grid, block, 0, st, a);
            else if (a.c == 4 && a.in_fmt == kFmtU16) hipLaunchKernelGGL((postproc_tiles_area<TP, uint8_t, true, uint16_t, DI>), grid, block, 0, st, a);
            else if (a.c == 4) hipLaunchKernelGGL((postproc_tiles_area<TP, uint8_t, true, uint8_t, DI>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((postproc_tiles_area<TP, uint8_t, false, uint8_t, DI>), grid, block, 0, st, a);
        });
}

// A rational scale other than 4 / 2 / 1 on both axes (rsr_set_out_ratio, rsr_set_out_ratio_xy)?
static bool generic_ratio(const PostArgs& a)
{
    const bool same = a.num_y == a.num && a.den_y == a.den;
    return a.num > 0 && !(same && a.den == 1 && (a.num == 4 || a.num == 2 || a.num == 1));
}

// ---- alpha through the network (engine option "alpha_net": PostArgs::alpha_dst) --------------------------------------------------------
// The alpha sample of include/realsr_hip.h ("alpha_net") from A0, A1, A2, what RSR_FMT_F32_CHW would hold for the pixel of the gray image:
// m = min(((A0 + A1) + A2) * fp32(1 / 3), 1), every operation rounded by itself ...
__device__ __forceinline__ float alpha_net_mean(float a0, float a1, float a2)
{
    return fminf(mul_rn(add_rn(add_rn(a0, a1), a2), (float)(1.0 / 3.0)), 1.f);
}
// ... and its store: floor(m * 255 + 0.5) clamped to 0 .. 255, the product and the sum rounded by themselves (m * 255 is not exact in fp32,
// unlike the fp16-valued colour, so the definition does not leave the contraction to the compiler), or post_store16(m).
template <typename TO>
__device__ __forceinline__ TO alpha_net_store(float m)
{
    if constexpr (sizeof(TO) == 1) return (uint8_t)fminf(fmaxf(floorf(add_rn(mul_rn(m, 255.f), 0.5f)), 0.f), 255.f);
    else return post_store16(m);
}

// The post launch of the alpha pass: one thread makes ONE output pixel of the tile's rectangle and stores ONLY its sample 3 (TO: uint8_t /
// uint16_t, RGBA).  The three channel values come from the helpers the colour kernels use, so they ARE what RSR_FMT_F32_CHW holds:
//   K = 1  the x4 image: merged_block<TP, 1> (postproc_tiles' value, clamped to [0, 1]);
//   K = 2 / 4  out_scale 2 / 1: box_mean of merged_block<TP, K> (postproc_tiles_box);
//   K = 0  a ratio or pair: area_pixel (postproc_tiles_area).
// One channel at a time, as in the box kernel.  Lanes run along x.
template <typename TP, typename TO, int K>
__global__ __launch_bounds__(256) void postproc_tiles_alpha(const PostArgs a)
{
    const BaseTile t = a.tiles[blockIdx.z];
    const int im = __builtin_amdgcn_readfirstlane(t.img);
    const int nx = K ? 1 : a.num, Lx = K ? K : 4 * a.den, ny = K ? 1 : a.num_y, Ly = K ? K : 4 * a.den_y; // output pixels per x4 pixel: n / L
    const int gx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int gy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (gx >= t.out_w * nx / Lx || gy >= t.out_h * ny / Ly) return;
    const int w = t.tw * 4, h = t.th * 4;
    const long long cstep = (long long)w * h;
    const TP* b0 = reinterpret_cast<const TP*>(static_cast<const char*>(a.planar3) + (long long)t.slot0 * a.slot_stride);
    const long long ss = a.slot_stride / (long long)sizeof(TP);
    float v0 = 0.f, v1 = 0.f, v2 = 0.f; // (no array: the loop is not unrolled, and an indexed one would live in scratch)
#pragma unroll 1
    for (int q = 0; q < 3; q++)
    {
        float d;
        if constexpr (K == 0) d = area_pixel<TP>(b0 + q * cstep, ss, w, h, a.crop, a.tta, nx, Lx, ny, Ly, a.area_norm, gx, gy);
        else
        {
            float c[K][K];
            merged_block<TP, K>(b0 + q * cstep, ss, w, h, gx * K + a.crop, gy * K + a.crop, a.tta, c);
            if constexpr (K == 1) d = c[0][0];
            else d = box_mean<K>(c);
        }
        v0 = q == 0 ? d : v0, v1 = q == 1 ? d : v1, v2 = q == 2 ? d : v2;
    }
    TO* const o = reinterpret_cast<TO*>(a.outs[im] + ((long long)(t.out_y - a.out_row0) * ny / Ly + gy) * (long long)a.out_pitch[im]) +
                  ((long long)t.out_x * nx / Lx + gx) * 4;
    o[3] = alpha_net_store<TO>(alpha_net_mean(v0, v1, v2));
}

template <typename TP>
static void launch_postproc_alpha(const PostArgs& a, int max_ow, int max_oh, hipStream_t st)
{
    auto go = [&](auto k, int ow, int oh) {
        constexpr int K = decltype(k)::value;
        const dim3 grid((ow + 63) / 64, (oh + 3) / 4, a.ntiles), block(256);
        if (a.out_fmt == kFmtU16) hipLaunchKernelGGL((postproc_tiles_alpha<TP, uint16_t, K>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((postproc_tiles_alpha<TP, uint8_t, K>), grid, block, 0, st, a);
    };
    if (generic_ratio(a)) go(std::integral_constant<int, 0>{}, max_ow * a.num / (4 * a.den), max_oh * a.num_y / (4 * a.den_y));
    else if (a.box == 2) go(std::integral_constant<int, 2>{}, max_ow / 2, max_oh / 2);
    else if (a.box > 1) go(std::integral_constant<int, 4>{}, max_ow / 4, max_oh / 4);
    else go(std::integral_constant<int, 1>{}, max_ow, max_oh);
}

// ---- YUV 4:2:0 and 4:2:2 output (PostArgs::out_fmt kFmtNV12 / kFmtP010, kFmtNV16 / kFmtP210) ------------------------------------
// code = floor(v * scale + add) clamped to [0, maxcode] (add = offset + 0.5f), as the sample type stores it: P010 / P210 keep it in the
// high bits; LOW = true (planar 4:4:4) stores the code itself, the six bits above it 0
// DI (option "dither"): code = floor(v * scale + (offset + theta)), the same clamp -- `add` is then the offset ALONE (YuvAdd), the sum in
// the brackets rounded by itself like the other two operations (exact: an integer offset below 2^16 plus a multiple of 2^-8)
template <typename TO, bool LOW = false, bool DI = false>
__device__ __forceinline__ unsigned yuv_code(float v, float scale, float add, float maxcode, [[maybe_unused]] float theta = 0.5f)
{
    if constexpr (DI) add = add_rn(add, theta);
    const float q = fminf(fmaxf(floorf(add_rn(mul_rn(v, scale), add)), 0.f), maxcode);
    return sizeof(TO) == 1 || LOW ? (unsigned)q : (unsigned)q << 6;
}
// The `add` of yuv_code for the luma (y) and the chroma (c) codes: offset + 0.5f as YuvCoef carries it, or under DI the offset itself (the
// decode's yoff / coff are the very numbers yadd / cadd were made from: engine.cpp yuv_coef)
template <bool DI>
struct YuvAdd
{
    float y, c;
    __device__ __forceinline__ YuvAdd(const YuvCoef& k) : y(DI ? k.yoff : k.yadd), c(DI ? k.coff : k.cadd) {}
};

// Two neighbouring samples of a surface row (lo in front) as ONE store of twice the sample size where the address allows it.
template <typename TO>
__device__ __forceinline__ void store_pair(uint8_t* o, unsigned lo, unsigned hi)
{
    if constexpr (sizeof(TO) == 1)
    {
        if (!(reinterpret_cast<uintptr_t>(o) & 1)) *reinterpret_cast<unsigned short*>(o) = (unsigned short)(lo | (hi << 8));
        else { o[0] = (uint8_t)lo; o[1] = (uint8_t)hi; }
    }
    else
    {
        if (!(reinterpret_cast<uintptr_t>(o) & 3)) *reinterpret_cast<unsigned*>(o) = lo | (hi << 16);
        else { reinterpret_cast<unsigned short*>(o)[0] = (unsigned short)lo; reinterpret_cast<unsigned short*>(o)[1] = (unsigned short)hi; }
    }
}

// ONE pixel d of the context's out_scale image (K = 4 / out_scale x4 pixels per axis; (px, py) its first x4 pixel in the blob, K-aligned):
// the K x K block gathered by merged_block and box-reduced in the order of include/realsr_hip.h ("out_scale") -- what RSR_FMT_F32_CHW
// holds for it.  QuadBox::at.
template <typename TP, int K>
__device__ __forceinline__ float out_pixel(const TP* b, long long ss, int w, int h, int px, int py, int tta)
{
    float c[K][K];
    merged_block<TP, K>(b, ss, w, h, px, py, tta, c);
    if constexpr (K == 1) return c[0][0];
    else if constexpr (K == 2) return mul_rn(add_rn(add_rn(c[0][0], c[0][1]), add_rn(c[1][0], c[1][1])), 0.25f);
    else return box_mean<4>(c);
}

// Where yuv_quad takes the RGB value d of an output pixel from, b the channel's blob -- what RSR_FMT_F32_CHW holds for that pixel: quad(b, d)
// = the four d of the thread's 2 x 2 quad, at(b, ox, oy) = ONE d, ox / oy output pixels beside the quad's first; out_x(v) / out_y(v) = a
// length v of the x4 image in output columns / rows.
// QuadBox: out_scale OS = 4, 2 or 1 (K = 4 / OS x4 pixels per output pixel and axis; (sx, sy) the quad's first x4 pixel in the blob).
// The quad is the 2K x 2K block in one or four merged_block fetches; a neighbour is out_pixel at (sx + K ox, sy + K oy), K-aligned like
// sx and sy.
// whole_quads: both rows of every quad exist whatever the surface (a tile's rectangle has an even number of rows) -- what a 4:2:2 surface,
// whose rectangles may end on an odd row, needs to know (yuv_quad).
template <typename TP, int OS>
struct QuadBox
{
    static constexpr int K = 4 / OS;
    static constexpr bool whole_quads = OS != 1; // (4 th rows of x4 pixels: even at out_scale 4 and 2, th of them at out_scale 1)
    long long ss;
    int w, h, sx, sy, tta;
    __device__ __forceinline__ void quad(const TP* b, float (&d)[2][2]) const
    {
        if constexpr (OS == 4)
            merged_block<TP, 2>(b, ss, w, h, sx, sy, tta, d);
        else if constexpr (OS == 2)
        {
            float c[4][4];
            merged_block<TP, 4>(b, ss, w, h, sx, sy, tta, c);
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int i = 0; i < 2; i++)
                    d[j][i] = mul_rn(add_rn(add_rn(c[2 * j][2 * i], c[2 * j][2 * i + 1]), add_rn(c[2 * j + 1][2 * i], c[2 * j + 1][2 * i + 1])), 0.25f);
        }
        else
        {
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int i = 0; i < 2; i++)
                {
                    float c[4][4];
                    merged_block<TP, 4>(b, ss, w, h, sx + 4 * i, sy + 4 * j, tta, c);
                    d[j][i] = box_mean<4>(c);
                }
        }
    }
    __device__ __forceinline__ float at(const TP* b, int ox, int oy) const { return out_pixel<TP, K>(b, ss, w, h, sx + K * ox, sy + K * oy, tta); }
    __device__ __forceinline__ int out_x(int v) const { return v / K; }
    __device__ __forceinline__ int out_y(int v) const { return v / K; }
};

// QuadArea: any other ratio n / d or pair of ratios (rsr_set_out_ratio, rsr_set_out_ratio_xy); (px, py) the quad's first output pixel in
// the tile's rectangle.  Every d is area_pixel.  Every tap index stays inside the tile's kept rectangle as in postproc_tiles_area:
// X < out_w nx / Lx gives ((X + 1) Lx - 1) / nx <= out_w - 1, and the rows likewise.  out_x(v) / out_y(v) = a length v of the x4 image in
// output columns / rows.
template <typename TP>
struct QuadArea
{
    static constexpr bool whole_quads = false;
    long long ss;
    int w, h, crop, tta, nx, Lx, ny, Ly;
    float norm;
    int px, py;
    __device__ __forceinline__ void quad(const TP* b, float (&d)[2][2]) const
    {
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int i = 0; i < 2; i++) d[j][i] = at(b, i, j);
    }
    __device__ __forceinline__ float at(const TP* b, int ox, int oy) const { return area_pixel<TP>(b, ss, w, h, crop, tta, nx, Lx, ny, Ly, norm, px + ox, py + oy); }
    __device__ __forceinline__ int out_x(int v) const { return v * nx / Lx; }
    __device__ __forceinline__ int out_y(int v) const { return v * ny / Ly; }
};

// ONE 2 x 2 quad of luma samples and the (U, V) pair they share, quad (gx, gy) of tile t's rectangle: what a thread of
// postproc_tiles_yuv and postproc_tiles_yuv_area does behind its source `src` of RGB values d (QuadBox / QuadArea; b0 the blob of
// channel 0, the channels cstep elements apart).  include/realsr_hip.h ("yuv_matrix") defines it: Y' = (kr R + kg G) + kb B per pixel;
// chroma from the mean m of the quad, ((d00 + d01) + (d10 + d11)) * 0.25f per channel.  One channel at a time (the loads of three would
// cost three times the registers): Y' is accumulated across the channel loop, 0 + kr R being kr R exactly (d >= 0).
//
// SITE (PostArgs::siting, option "yuv_siting"): 0 = chroma at the centre of the quad, as above.  1 (left) / 2 (top-left): chroma co-sited
// with the quad's first column / first pixel -- include/realsr_hip.h "Chroma siting": per channel Hs(y) = (d(xl, y) + d(2X+1, y)) +
// (d(2X, y) + d(2X, y)), the unnormalised [1 2 1] filter about column 2X, and m = (Hs(2Y) + Hs(2Y+1)) * 0.125f (left) or ((Hs(yu) +
// Hs(2Y+1)) + (Hs(2Y) + Hs(2Y))) * 0.0625f (top-left), xl = 2X - 1 and yu = 2Y - 1 -- or 2X / 2Y in the first quad column / row of the
// TILE's rectangle (gx == 0 / gy == 0): the pixel beyond belongs to another tile's blob.  Luma does not change.  The neighbours
// d(2X-1, .) and d(., 2Y-1) are pixels of this tile's own kept rectangle, gathered like every other d by the thread itself: redundant with
// the lane beside it / the wave above it, served by the caches, and free of any cross-lane dependence on threads that have returned.  At
// a tile-first column / row the offset is 0, the pixel's own: the same loads, the same arithmetic, hence bitwise d(2X, .) / d(., 2Y) with
// no divergent branch.
//
// VS (the surface's vertical chroma shift): 1 = 4:2:0, the above.  0 = 4:2:2 (kFmtNV16 / kFmtP210; include/realsr_hip.h "YUV 4:2:2"): the unit
// is a 2 x 1 luma pair and its (U, V), and the thread makes the two stacked pairs of its quad -- one gather of the same 2 x 2 block, two UV
// stores.  Per row j and channel, m_j = (d(2X, j) + d(2X+1, j)) * 0.5f (SITE 0) or Hs(j) * 0.25f (SITE 1; top-left is left here); nothing
// is filtered vertically, so no row clamp exists.  rows = the luma rows of this quad that exist: 2, or 1 where the tile's rectangle ends on
// an odd row (no parity rule holds for a 4:2:2 surface's rows) -- then nothing of row 1 is gathered (unless SRC::whole_quads says it cannot
// happen) or stored.
//
// DI (option "dither"): every code is rounded against theta of its own place in its own plane of the output image -- a luma sample at
// (X + i, Yi + j), Yi the quad's first row in the IMAGE (not in the buffer of a tile range), the (U, V) pair, which shares one threshold,
// at its chroma indices (X / 2, Yi / 2) or, 4:2:2, (X / 2, Yi + n).  The values that are quantised are untouched.
template <typename TO, int SITE, int VS, bool DI, typename SRC, typename TP>
__device__ __forceinline__ void yuv_quad(const PostArgs& a, const BaseTile& t, int im, int gx, int gy, const SRC& src, const TP* b0, long long cstep, int rows = 2)
{
    constexpr int NC = VS ? 1 : 2; // chroma rows of the quad
    const YuvCoef& k = a.yuv;
    float yq[2][2] = {{0.f, 0.f}, {0.f, 0.f}}, ym[NC], rm[NC], bm[NC];
#pragma unroll
    for (int n = 0; n < NC; n++) ym[n] = rm[n] = bm[n] = 0.f;
    [[maybe_unused]] const int xl = gx ? -1 : 0, yu = gy ? -1 : 0; // output column xl / row yu, relative to the quad's first pixel
#pragma unroll 1
    for (int q = 0; q < 3; q++)
    {
        const TP* b = b0 + q * cstep;
        float d[2][2];
        if (VS || SRC::whole_quads || rows == 2) src.quad(b, d);
        else
        {
            d[0][0] = src.at(b, 0, 0), d[0][1] = src.at(b, 1, 0);
            d[1][0] = d[0][0], d[1][1] = d[0][1]; // (carried along, never stored)
        }
        const float kq = q == 0 ? k.kr : (q == 1 ? k.kg : k.kb);
        float m[NC];
        if constexpr (VS == 0)
        {
#pragma unroll
            for (int j = 0; j < 2; j++)
                if constexpr (SITE == 0) m[j] = mul_rn(add_rn(d[j][0], d[j][1]), 0.5f);
                else m[j] = mul_rn(add_rn(add_rn(src.at(b, xl, min(j, rows - 1)), d[j][1]), add_rn(d[j][0], d[j][0])), 0.25f);
        }
        else if constexpr (SITE == 0) m[0] = mul_rn(add_rn(add_rn(d[0][0], d[0][1]), add_rn(d[1][0], d[1][1])), 0.25f);
        else
        {
            float hs[2];
#pragma unroll
            for (int j = 0; j < 2; j++) hs[j] = add_rn(add_rn(src.at(b, xl, j), d[j][1]), add_rn(d[j][0], d[j][0]));
            if constexpr (SITE == 1) m[0] = mul_rn(add_rn(hs[0], hs[1]), 0.125f);
            else
            {
                const float u0 = src.at(b, 0, yu);
                const float hu = add_rn(add_rn(src.at(b, xl, yu), src.at(b, 1, yu)), add_rn(u0, u0));
                m[0] = mul_rn(add_rn(add_rn(hu, hs[1]), add_rn(hs[0], hs[0])), 0.0625f);
            }
        }
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int i = 0; i < 2; i++) yq[j][i] = add_rn(yq[j][i], mul_rn(kq, d[j][i]));
#pragma unroll
        for (int n = 0; n < NC; n++)
        {
            ym[n] = add_rn(ym[n], mul_rn(kq, m[n]));
            if (q == 0) rm[n] = m[n];
            if (q == 2) bm[n] = m[n];
        }
    }
    const long long pitch = a.out_pitch[im];
    const int X = src.out_x(t.out_x) + 2 * gx, Y = src.out_y(t.out_y - a.out_row0) + 2 * gy; // the quad's first luma sample
    uint8_t* const oy = a.outs[im] + Y * pitch + (long long)X * (int)sizeof(TO);
    const YuvAdd<DI> add(k);
    [[maybe_unused]] const int Yi = src.out_y(t.out_y) + 2 * gy; // the quad's first luma row in the image
#pragma unroll
    for (int j = 0; j < 2; j++)
        if (VS || j < rows)
            store_pair<TO>(oy + j * pitch, yuv_code<TO, false, DI>(yq[j][0], k.yscale, add.y, k.maxcode, theta_at<DI>(X, Yi + j)),
                           yuv_code<TO, false, DI>(yq[j][1], k.yscale, add.y, k.maxcode, theta_at<DI>(X + 1, Yi + j)));
    // the (U, V) pairs: a UV row is as long as a Y row, a pair as wide as two luma samples; 4:2:0 has one for the quad, on UV row Y / 2
    uint8_t* const ouv = a.outs[im] + a.out_plane[im] + (VS ? Y >> 1 : Y) * pitch + (long long)X * (int)sizeof(TO);
#pragma unroll
    for (int n = 0; n < NC; n++)
    {
        const float cb = mul_rn(sub_rn(bm[n], ym[n]), k.icb), cr = mul_rn(sub_rn(rm[n], ym[n]), k.icr);
        const float th = theta_at<DI>(X >> 1, VS ? Yi >> 1 : Yi + n);
        if (VS || n < rows)
            store_pair<TO>(ouv + n * pitch, yuv_code<TO, false, DI>(cb, k.cscale, add.c, k.maxcode, th), yuv_code<TO, false, DI>(cr, k.cscale, add.c, k.maxcode, th));
    }
}

// The YUV 4:2:0 sibling of postproc_tiles_box: one thread makes ONE quad (yuv_quad over QuadBox) at the context's out_scale OS (4, 2 or
// 1).  A tile's rectangle starts and ends on even output pixels (the engine refuses an out_scale 1 call where it would not), so no quad
// crosses a tile.  Lanes run along x.
// TP: element type of the blob (_Float16, or float in precise mode); TO: sample type of the surface, uint8_t (NV12) or uint16_t (P010).
// VS = 0: a 4:2:2 surface (TO: uint8_t NV16, uint16_t P210), two stacked luma pairs per thread.  Its rectangles start and end on even
// COLUMNS only; where one has an odd number of rows (out_scale 1) the threads of its last quad row make one pair (yuv_quad, rows).
template <typename TP, typename TO, int OS, int SITE = 0, int VS = 1, bool DI = false>
__global__ __launch_bounds__(256) void postproc_tiles_yuv(const PostArgs a)
{
    constexpr int K = 4 / OS, Q = 2 * K; // x4 pixels per output pixel / per quad, along an axis
    const BaseTile t = a.tiles[blockIdx.z];
    const int im = __builtin_amdgcn_readfirstlane(t.img);
    const int gx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int gy = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int oh = t.out_h / K; // output rows of the rectangle (4:2:0: even)
    if (gx >= t.out_w / Q || 2 * gy >= oh) return;
    const int w = t.tw * 4, h = t.th * 4;
    const TP* b0 = reinterpret_cast<const TP*>(static_cast<const char*>(a.planar3) + (long long)t.slot0 * a.slot_stride);
    const QuadBox<TP, OS> src{a.slot_stride / (long long)sizeof(TP), w, h, gx * Q + a.crop, gy * Q + a.crop, a.tta};
    yuv_quad<TO, SITE, VS, DI>(a, t, im, gx, gy, src, b0, (long long)w * h, min(2, oh - 2 * gy));
}

// The sibling of postproc_tiles_yuv for the scales n / d that are not 4, 2 or 1: yuv_quad over QuadArea.  A tile's rectangle is
// tilesize * n / d output pixels and starts at its multiples (per axis: tilesize * nx / dx columns, tilesize * ny / dy rows); the engine
// admits the call only where those, w * nx / dx and h * ny / dy are even (out_admit), so no quad crosses a tile or the image's edge.
// Lanes run along x.
// VS = 0: a 4:2:2 surface -- w * nx / dx and tilesize * nx / dx are even, the two row counts are any (yuv_quad, rows).
template <typename TP, typename TO, int SITE, int VS = 1, bool DI = false>
__global__ __launch_bounds__(256) void postproc_tiles_yuv_area(const PostArgs a)
{
    const BaseTile t = a.tiles[blockIdx.z];
    const int im = __builtin_amdgcn_readfirstlane(t.img);
    const int nx = a.num, Lx = 4 * a.den, ny = a.num_y, Ly = 4 * a.den_y;
    const int gx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int gy = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int oh = t.out_h * ny / Ly; // output rows of the rectangle (4:2:0: even)
    if (gx >= t.out_w * nx / Lx / 2 || 2 * gy >= oh) return;
    const int w = t.tw * 4, h = t.th * 4;
    const TP* b0 = reinterpret_cast<const TP*>(static_cast<const char*>(a.planar3) + (long long)t.slot0 * a.slot_stride);
    const QuadArea<TP> src{a.slot_stride / (long long)sizeof(TP), w, h, a.crop, a.tta, nx, Lx, ny, Ly, a.area_norm, 2 * gx, 2 * gy};
    yuv_quad<TO, SITE, VS, DI>(a, t, im, gx, gy, src, b0, (long long)w * h, min(2, oh - 2 * gy));
}

template <typename TP, typename TO>
static void launch_postproc_yuv_area(const PostArgs& a, int max_ow, int max_oh, hipStream_t st)
{
    const int Lx = 4 * a.den, Ly = 4 * a.den_y; // (ow_tile / 2) x (oh_tile / 2) quads per tile (4:2:2: the last quad row may be half a quad)
    const dim3 grid((max_ow * a.num / Lx / 2 + 63) / 64, ((max_oh * a.num_y / Ly + 1) / 2 + 3) / 4, a.ntiles), block(256);
    with_chroma(a.out_fmt, a.siting, [&](auto site, auto vs) {
        with_dither(a, [&](auto di) {
            hipLaunchKernelGGL((postproc_tiles_yuv_area<TP, TO, decltype(site)::value, decltype(vs)::value, decltype(di)::value>), grid, block, 0, st, a);
        });
    });
}

template <typename TP, typename TO>
static void launch_postproc_yuv(const PostArgs& a, int max_ow, int max_oh, hipStream_t st)
{
    const int q = a.box > 1 ? 2 * a.box : 2; // x4 pixels per quad and axis
    const dim3 grid((max_ow / q + 63) / 64, ((max_oh / (q / 2) + 1) / 2 + 3) / 4, a.ntiles), block(256); // (4:2:2: the last quad row may be half a quad)
    with_chroma(a.out_fmt, a.siting, [&](auto site, auto vs) {
        constexpr int SITE = decltype(site)::value, VS = decltype(vs)::value;
        with_dither(a, [&](auto di) {
            constexpr bool DI = decltype(di)::value;
            if (a.box == 4) hipLaunchKernelGGL((postproc_tiles_yuv<TP, TO, 1, SITE, VS, DI>), grid, block, 0, st, a);
            else if (a.box == 2) hipLaunchKernelGGL((postproc_tiles_yuv<TP, TO, 2, SITE, VS, DI>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((postproc_tiles_yuv<TP, TO, 4, SITE, VS, DI>), grid, block, 0, st, a);
        });
    });
}

// ---- planar YUV 4:4:4 output (PostArgs::out_fmt kFmtYUV444P / kFmtYUV444P10; include/realsr_hip.h "YUV 4:4:4") -----------------------------
// NP (1 or 2) neighbouring pixels of ONE output row, the first at column gx * NP of tile t's rectangle, row gy: the per-pixel sibling of
// yuv_quad, behind the same sources of RGB values d (QuadBox / QuadArea, whose origin is the first of these pixels: d = src.at(b, i, 0)).
// This is the 4:2:0 rule with m = d: Y' = (kr R + kg G) + kb B, accumulated across the channel loop as in yuv_quad (one channel's gather
// at a time: the three never hold registers together), Cb = (B - Y') * icb, Cr = (R - Y') * icr; nothing is filtered, so no siting and no
// tile-first clamp exist.  Three plane stores finish it, the planes out_plane apart; a 10-bit code is stored as it is (the high six bits
// 0).  n = how many of the NP pixels exist: a rectangle may have an odd width, and nothing of a pixel beyond it is gathered or stored.
// DI (option "dither"): the three codes of a pixel sit at the same (x, y) of their planes and share theta(x, y).
template <typename TO, int NP, bool DI, typename SRC, typename TP>
__device__ __forceinline__ void yuv_pixels(const PostArgs& a, const BaseTile& t, int im, int gx, int gy, const SRC& src, const TP* b0, long long cstep, int n)
{
    const YuvCoef& k = a.yuv;
    float y[NP], r[NP], bl[NP];
#pragma unroll
    for (int i = 0; i < NP; i++) y[i] = r[i] = bl[i] = 0.f;
#pragma unroll 1
    for (int q = 0; q < 3; q++)
    {
        const TP* b = b0 + q * cstep;
        const float kq = q == 0 ? k.kr : (q == 1 ? k.kg : k.kb);
#pragma unroll
        for (int i = 0; i < NP; i++)
        {
            const float d = src.at(b, i < n ? i : 0, 0); // (a pixel beyond the rectangle: the first one again, carried along, never stored)
            y[i] = add_rn(y[i], mul_rn(kq, d));
            if (q == 0) r[i] = d;
            if (q == 2) bl[i] = d;
        }
    }
    unsigned cy[NP], cu[NP], cv[NP];
    const int X = src.out_x(t.out_x) + NP * gx, Y = src.out_y(t.out_y - a.out_row0) + gy;
    const YuvAdd<DI> add(k);
    [[maybe_unused]] const int Yi = src.out_y(t.out_y) + gy; // the row in the image (Y: in the buffer of a tile range)
#pragma unroll
    for (int i = 0; i < NP; i++)
    {
        const float th = theta_at<DI>(X + i, Yi);
        cy[i] = yuv_code<TO, true, DI>(y[i], k.yscale, add.y, k.maxcode, th);
        cu[i] = yuv_code<TO, true, DI>(mul_rn(sub_rn(bl[i], y[i]), k.icb), k.cscale, add.c, k.maxcode, th);
        cv[i] = yuv_code<TO, true, DI>(mul_rn(sub_rn(r[i], y[i]), k.icr), k.cscale, add.c, k.maxcode, th);
    }
    uint8_t* const o = a.outs[im] + Y * (long long)a.out_pitch[im] + (long long)X * (int)sizeof(TO);
    const long long plane = a.out_plane[im];
    if constexpr (NP == 2)
    {
        if (n == 2)
        { // (store_pair falls back to two sample stores where the address is odd: a window starts at any byte)
            store_pair<TO>(o, cy[0], cy[1]);
            store_pair<TO>(o + plane, cu[0], cu[1]);
            store_pair<TO>(o + 2 * plane, cv[0], cv[1]);
            return;
        }
    }
    *reinterpret_cast<TO*>(o) = (TO)cy[0];
    *reinterpret_cast<TO*>(o + plane) = (TO)cu[0];
    *reinterpret_cast<TO*>(o + 2 * plane) = (TO)cv[0];
}

// The 4:4:4 sibling of postproc_tiles_yuv: one thread makes NP pixels of one row (yuv_pixels over QuadBox) at the context's out_scale OS (4,
// 2 or 1).  The rectangle of a tile is out_w / K x out_h / K output pixels, of any parity.  Lanes run along x: every plane store of a wave
// is one contiguous run.  TP: element type of the blob; TO: uint8_t (YUV444P) or uint16_t (YUV444P10).
template <typename TP, typename TO, int OS, int NP, bool DI = false>
__global__ __launch_bounds__(256) void postproc_tiles_yuv444(const PostArgs a)
{
    constexpr int K = 4 / OS; // x4 pixels per output pixel, along an axis
    const BaseTile t = a.tiles[blockIdx.z];
    const int im = __builtin_amdgcn_readfirstlane(t.img);
    const int gx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int gy = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int ow = t.out_w / K, oh = t.out_h / K;
    if (NP * gx >= ow || gy >= oh) return;
    const int w = t.tw * 4, h = t.th * 4;
    const TP* b0 = reinterpret_cast<const TP*>(static_cast<const char*>(a.planar3) + (long long)t.slot0 * a.slot_stride);
    const QuadBox<TP, OS> src{a.slot_stride / (long long)sizeof(TP), w, h, NP * gx * K + a.crop, gy * K + a.crop, a.tta};
    yuv_pixels<TO, NP, DI>(a, t, im, gx, gy, src, b0, (long long)w * h, min(NP, ow - NP * gx));
}

// ... and of postproc_tiles_yuv_area, for every other ratio or pair: yuv_pixels over QuadArea.  The engine admits the call where the ratio
// rule holds (w, h and tilesize times the ratios whole); the quotients may be odd.
template <typename TP, typename TO, int NP, bool DI = false>
__global__ __launch_bounds__(256) void postproc_tiles_yuv444_area(const PostArgs a)
{
    const BaseTile t = a.tiles[blockIdx.z];
    const int im = __builtin_amdgcn_readfirstlane(t.img);
    const int nx = a.num, Lx = 4 * a.den, ny = a.num_y, Ly = 4 * a.den_y;
    const int gx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int gy = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int ow = t.out_w * nx / Lx, oh = t.out_h * ny / Ly;
    if (NP * gx >= ow || gy >= oh) return;
    const int w = t.tw * 4, h = t.th * 4;
    const TP* b0 = reinterpret_cast<const TP*>(static_cast<const char*>(a.planar3) + (long long)t.slot0 * a.slot_stride);
    const QuadArea<TP> src{a.slot_stride / (long long)sizeof(TP), w, h, a.crop, a.tta, nx, Lx, ny, Ly, a.area_norm, NP * gx, gy};
    yuv_pixels<TO, NP, DI>(a, t, im, gx, gy, src, b0, (long long)w * h, min(NP, ow - NP * gx));
}

// f(integral_constant NP): pixels per thread of the 4:4:4 kernels.  Chosen by the compiler's resource report and by measurement (DESIGN.md
// 4.8, profiles/yuv444.txt): two at out_scale 4 -- 50 VGPRs against 42 at the same occupancy 8, stores twice as wide, post_ms 0.19 - 0.21
// against 0.22 - 0.23 ms on a 1080p frame -- and one everywhere else: a second pixel costs out_scale 2 a third of its occupancy (116
// VGPRs against 80; 0.13 against 0.08 ms), takes out_scale 1 to 256 VGPRs and occupancy 1 (140 and 3) and the area kernel from
// occupancy 8 to 6.  PostArgs::variant forces a shape (tests, A/B): 1 = one pixel, 2 = two.
template <typename F>
static void with_pixels_per_thread(const PostArgs& a, bool x4, F f)
{
    if (a.variant == 2 || (a.variant == 0 && x4)) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 1>{});
}

template <typename TP, typename TO>
static void launch_postproc_yuv444_area(const PostArgs& a, int max_ow, int max_oh, hipStream_t st)
{
    const int ow = max_ow * a.num / (4 * a.den), oh = max_oh * a.num_y / (4 * a.den_y); // output pixels of the largest tile rectangle
    with_pixels_per_thread(a, false, [&](auto np) {
        constexpr int NP = decltype(np)::value;
        const dim3 grid(((ow + NP - 1) / NP + 63) / 64, (oh + 3) / 4, a.ntiles), block(256);
        with_dither(a, [&](auto di) { hipLaunchKernelGGL((postproc_tiles_yuv444_area<TP, TO, NP, decltype(di)::value>), grid, block, 0, st, a); });
    });
}

template <typename TP, typename TO>
static void launch_postproc_yuv444(const PostArgs& a, int max_ow, int max_oh, hipStream_t st)
{
    const int K = a.box > 1 ? a.box : 1, ow = max_ow / K, oh = max_oh / K;
    with_pixels_per_thread(a, K == 1, [&](auto np) {
        constexpr int NP = decltype(np)::value;
        const dim3 grid(((ow + NP - 1) / NP + 63) / 64, (oh + 3) / 4, a.ntiles), block(256);
        with_dither(a, [&](auto di) {
            constexpr bool DI = decltype(di)::value;
            if (a.box == 4) hipLaunchKernelGGL((postproc_tiles_yuv444<TP, TO, 1, NP, DI>), grid, block, 0, st, a);
            else if (a.box == 2) hipLaunchKernelGGL((postproc_tiles_yuv444<TP, TO, 2, NP, DI>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((postproc_tiles_yuv444<TP, TO, 4, NP, DI>), grid, block, 0, st, a);
        });
    });
}

void launch_postproc_tiles(const PostArgs& a, int max_ow, int max_oh, hipStream_t st)
{
    if (a.ntiles <= 0) return;
    with_blob_type(a, [&](auto tp) {
        using TP = decltype(tp);
        if (a.alpha_dst) return launch_postproc_alpha<TP>(a, max_ow, max_oh, st); // (the engine sends c == 4 uint8 / uint16 HWC images only)
        if (fmt_is_444(a.out_fmt))
        { // a planar 4:4:4 surface: one thread per pixel (or two), at every out_scale or ratio, with and without TTA
            with_sample_type(a.out_fmt, [&](auto to) {
                using TO = decltype(to);
                if (generic_ratio(a)) launch_postproc_yuv444_area<TP, TO>(a, max_ow, max_oh, st);
                else launch_postproc_yuv444<TP, TO>(a, max_ow, max_oh, st);
            });
            return;
        }
        if (fmt_is_yuv(a.out_fmt))
        { // a 4:2:0 or 4:2:2 surface: one thread per luma quad, at every out_scale or ratio, with and without TTA
            with_sample_type(a.out_fmt, [&](auto to) {
                using TO = decltype(to);
                if (generic_ratio(a)) launch_postproc_yuv_area<TP, TO>(a, max_ow, max_oh, st);
                else launch_postproc_yuv<TP, TO>(a, max_ow, max_oh, st);
            });
            return;
        }
        // one thread per output pixel, with and without TTA: the area-averaging kernel, or at out_scale 2 / 1 the box-reducing one
        if (generic_ratio(a)) return launch_postproc_area<TP>(a, max_ow, max_oh, st);
        if (a.box == 2) return launch_postproc_box<TP, 2>(a, max_ow, max_oh, st);
        if (a.box > 1) return launch_postproc_box<TP, 4>(a, max_ow, max_oh, st);
        // Measured on the C5 frame: the TTA gather 0.92 ms staged vs 1.72 ms per-pixel (profiles/post_dedupe.txt; 2.42 ms before the per-pixel
        // kernel took its value through tta_gather, profiles/r04_prepost.txt: the transposed variants), but 0.19 vs 0.12 ms for the plain
        // single-variant conversion.  Default: staged under TTA, plain otherwise.
        // A uint16 image on either side (the destination, or the RGBA source the alpha is read from) has the per-pixel kernel only: the
        // staged one collects uint8 pixels and reads uint8 alpha.
        const bool sixteen = a.out_fmt == kFmtU16 || (a.c == 4 && a.in_fmt == kFmtU16);
        const bool staged = !sixteen && (a.variant == 2 || (a.variant == 0 && a.tta));
        bool aligned = true; // (the staged kernel stores the uint8 image in dwords: base and row pitch must be multiples of 4)
        for (int i = 0; i < a.nimgs; i++) aligned = aligned && (a.out_fmt != kFmtU8 || !((reinterpret_cast<uintptr_t>(a.outs[i]) | (uintptr_t)a.out_pitch[i]) & 3));
        with_image_type(a.out_fmt, [&](auto to) {
            using TO = decltype(to);
            const dim3 grid((max_ow + 63) / 64, (max_oh + 3) / 4, a.ntiles);
            with_dither(a, [&](auto di) {
                constexpr bool DI = decltype(di)::value && is_hwc<TO>; // (a planar float image is never dithered: no instantiation for it)
                if constexpr (std::is_same<TO, uint16_t>::value)
                    with_alpha_type(a, [&](auto ta) {
                        const dim3 grid2((max_ow / 2 + 63) / 64, (max_oh + 3) / 4, a.ntiles);
                        // Measured on the C2 frame (profiles/rgb16.txt): two pixels per thread 0.128 ms against 0.136 for one (RGBA 0.390 against
                        // 0.453); under TTA the gather dominates and the pair's doubled registers cost more than its stores save (RGB 1.816
                        // against 1.661).  Default: two without TTA, one with; variant 1 / 2 force one / two (the bytes are the same).
                        const bool two = a.variant == 2 || (a.variant == 0 && !a.tta);
                        if (two && a.c == 4) hipLaunchKernelGGL((postproc_tiles_u16x2<TP, 4, decltype(ta), DI>), grid2, dim3(256), 0, st, a);
                        else if (two) hipLaunchKernelGGL((postproc_tiles_u16x2<TP, 3, uint8_t, DI>), grid2, dim3(256), 0, st, a);
                        else hipLaunchKernelGGL((postproc_tiles<TP, TO, decltype(ta), DI>), grid, dim3(256), 0, st, a);
                    });
                else if (sixteen) // (a uint8 image with a uint16 RGBA source)
                {
                    if constexpr (std::is_same<TO, uint8_t>::value) hipLaunchKernelGGL((postproc_tiles<TP, TO, uint16_t, DI>), grid, dim3(256), 0, st, a);
                }
                else if (staged && aligned)
                    hipLaunchKernelGGL((postproc_tiles_lds<TP, TO, DI>), dim3((max_ow + 31) / 32, (max_oh + 31) / 32, a.ntiles), dim3(256), 0, st, a);
                else hipLaunchKernelGGL((postproc_tiles<TP, TO, uint8_t, DI>), grid, dim3(256), 0, st, a);
            });
        });
    });
}

// ---- shader-shaped kernels: same arithmetic, the shaders' own buffer layouts -----------------
struct Ptr8
{
    uint16_t* p[8];
};
struct CPtr8
{
    const uint16_t* p[8];
};

__global__ __launch_bounds__(256) void preproc_shader(const uint8_t* bottom, int w, int h, int channels, Ptr8 top, int ntop,
                                                      int outw, int outh, int outcstep, int pad_top, int pad_left,
                                                      int crop_x, int crop_y, uint16_t* alpha, int alphaw, int alphah, int bgr)
{
    int gx = blockIdx.x * 32 + (threadIdx.x & 31);
    int gy = blockIdx.y * 8 + (threadIdx.x >> 5);
    const int gz = blockIdx.z;
    if (gx >= outw || gy >= outh || gz >= channels) return;
    int x = gx + crop_x - pad_left;
    int y = gy + crop_y - pad_top;
    x = reflect101(x, w);
    y = reflect101(y, h);
    const int v_offset = y * w + x;
    float v;
    if (bgr == 1 && gz != 3) v = (float)bottom[v_offset * channels + 2 - gz];
    else v = (float)bottom[v_offset * channels + gz];
    if (gz == 3)
    {
        gx -= pad_left;
        gy -= pad_top;
        if (alpha && gx >= 0 && gx < alphaw && gy >= 0 && gy < alphah)
            reinterpret_cast<_Float16*>(alpha)[gy * alphaw + gx] = (_Float16)v;
        return;
    }
    const float norm_val = 1 / 255.f;
    const _Float16 hv = (_Float16)(v * norm_val);
    const int gzi = gz * outcstep;
    _Float16* const* T = reinterpret_cast<_Float16* const*>(top.p);
    T[0][gzi + gy * outw + gx] = hv;
    if (ntop == 8)
    {
        T[1][gzi + gy * outw + (outw - 1 - gx)] = hv;
        T[2][gzi + (outh - 1 - gy) * outw + (outw - 1 - gx)] = hv;
        T[3][gzi + (outh - 1 - gy) * outw + gx] = hv;
        T[4][gzi + gx * outh + gy] = hv;
        T[5][gzi + gx * outh + (outh - 1 - gy)] = hv;
        T[6][gzi + (outw - 1 - gx) * outh + (outh - 1 - gy)] = hv;
        T[7][gzi + (outw - 1 - gx) * outh + gy] = hv;
    }
}

void launch_preproc_shader(const uint8_t* bottom, int w, int h, int channels, uint16_t* const top[8], int ntop, int outw,
                           int outh, int outcstep, int pad_top, int pad_left, int crop_x, int crop_y, uint16_t* alpha,
                           int alphaw, int alphah, int bgr, hipStream_t st)
{
    Ptr8 t;
    for (int i = 0; i < 8; i++) t.p[i] = i < ntop ? top[i] : nullptr;
    const dim3 grid((outw + 31) / 32, (outh + 7) / 8, channels), block(256);
    hipLaunchKernelGGL(preproc_shader, grid, block, 0, st, bottom, w, h, channels, t, ntop, outw, outh, outcstep, pad_top,
                       pad_left, crop_x, crop_y, alpha, alphaw, alphah, bgr);
}

__global__ __launch_bounds__(256) void postproc_shader(CPtr8 bottom, int nbottom, int w, int h, int cstep, const uint16_t* alpha,
                                                       int alphaw, int alphah, uint8_t* top, int outw, int outh, int offset_x,
                                                       int gx_max, int crop_x, int crop_y, int channels, int bgr)
{
    const int gx = blockIdx.x * 32 + (threadIdx.x & 31);
    const int gy = blockIdx.y * 8 + (threadIdx.x >> 5);
    const int gz = blockIdx.z;
    if (gx >= gx_max || gy >= outh || gz >= channels) return;
    const _Float16* const* B = reinterpret_cast<const _Float16* const*>(bottom.p);
    float v;
    if (gz == 3) v = (float)reinterpret_cast<const _Float16*>(alpha)[gy * alphaw + gx];
    else
    {
        const int gzi = gz * cstep;
        const int sy = gy + crop_y, sx = gx + crop_x;
        if (nbottom == 1) v = (float)B[0][gzi + sy * w + sx];
        else
        {
            const float v0 = (float)B[0][gzi + sy * w + sx];
            const float v1 = (float)B[1][gzi + sy * w + (w - 1 - sx)];
            const float v2 = (float)B[2][gzi + (h - 1 - sy) * w + (w - 1 - sx)];
            const float v3 = (float)B[3][gzi + (h - 1 - sy) * w + sx];
            const float v4 = (float)B[4][gzi + sx * h + sy];
            const float v5 = (float)B[5][gzi + sx * h + (h - 1 - sy)];
            const float v6 = (float)B[6][gzi + (w - 1 - sx) * h + (h - 1 - sy)];
            const float v7 = (float)B[7][gzi + (w - 1 - sx) * h + sy];
            v = (v0 + v1 + v2 + v3 + v4 + v5 + v6 + v7) * 0.125f;
        }
        v = v * 255.f;
    }
    const int v_offset = gy * outw + gx + offset_x;
    const uint8_t u = post_store(v);
    if (bgr == 1 && gz != 3) top[v_offset * channels + 2 - gz] = u;
    else top[v_offset * channels + gz] = u;
}

void launch_postproc_shader(const uint16_t* const bottom[8], int nbottom, int w, int h, int cstep, const uint16_t* alpha,
                            int alphaw, int alphah, uint8_t* top, int outw, int outh, int offset_x, int gx_max, int crop_x,
                            int crop_y, int channels, int bgr, hipStream_t st)
{
    CPtr8 b;
    for (int i = 0; i < 8; i++) b.p[i] = i < nbottom ? bottom[i] : nullptr;
    const dim3 grid((gx_max + 31) / 32, (outh + 7) / 8, channels), block(256);
    hipLaunchKernelGGL(postproc_shader, grid, block, 0, st, b, nbottom, w, h, cstep, alpha, alphaw, alphah, top, outw, outh,
                       offset_x, gx_max, crop_x, crop_y, channels, bgr);
}

__global__ __launch_bounds__(256) void planar3_to_plane(const uint16_t* planar, int w, int h, void* plane, int plane_ch)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)w * h) return;
    const long long hw = (long long)w * h;
    uint4 v0 = make_uint4(0u, 0u, 0u, 0u);
    v0.x = (uint32_t)planar[i] | ((uint32_t)planar[hw + i] << 16);
    v0.y = (uint32_t)planar[2 * hw + i];
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    uint4* d = reinterpret_cast<uint4*>(static_cast<char*>(plane) + i * (plane_ch * 2));
    d[0] = v0;
    d[1] = z;
    if (plane_ch == 32)
    {
        d[2] = z;
        d[3] = z;
    }
}

void launch_planar3_to_plane(const uint16_t* planar, int w, int h, void* plane, int plane_ch, hipStream_t st)
{
    const long long n = (long long)w * h;
    hipLaunchKernelGGL(planar3_to_plane, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, planar, w, h, plane, plane_ch);
}

// Zero the 64-byte guard in front of `count` planes spaced `stride` bytes apart (see Engine::ensure_workspace).
__global__ __launch_bounds__(256) void zero_guards(char* first_guard, long long stride, long long count)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x; // one 16-byte piece per thread
    if (i >= count * 4) return;
    *reinterpret_cast<uint4*>(first_guard + (i >> 2) * stride + (i & 3) * 16) = make_uint4(0u, 0u, 0u, 0u);
}

void launch_zero_guards(void* first_guard, long long stride, long long count, hipStream_t st)
{
    if (count <= 0) return;
    hipLaunchKernelGGL(zero_guards, dim3((unsigned)((count * 4 + 255) / 256)), dim3(256), 0, st, static_cast<char*>(first_guard), stride, count);
}

// =============================================================================================
// frame diff per tile (rsr_diff_tiles, rsr_diff_tiles_sequence): which tiles' source rectangles differ between two frames
// =============================================================================================
constexpr int kDiffRows = 16; // rows of a rectangle per workgroup and step: 4 per wave, so that a 220-row tile spreads over 14 workgroups

__device__ __forceinline__ bool differ(uint4 x, uint4 y) { return ((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w)) != 0; }
__device__ __forceinline__ bool differ(uint32_t x, uint32_t y) { return x != y; }
__device__ __forceinline__ bool differ(uint8_t x, uint8_t y) { return x != y; }

// Do the n bytes behind pa and pb differ?  One wave, lanes along the row.  TV is the widest access both rows allow: their addresses agree
// modulo sizeof(TV), so one head of 0 .. 15 bytes brings both to that boundary.  Head and tail are compared byte by byte (lanes 0 .. 15 and
// 16 .. 31), the body in aligned pieces, 64 per step (a 220-pixel row of fp32 is 55 pieces of 16 bytes; a wider one loops).  No byte
// outside [pa, pa + n) and [pb, pb + n) is read: a crop's neighbours may belong to someone else.
template <typename TV>
__device__ __forceinline__ bool row_differs(const uint8_t* pa, const uint8_t* pb, int n, int lane)
{
    constexpr int V = int(sizeof(TV));
    const int head = min(n, int((0 - reinterpret_cast<uintptr_t>(pa)) & uintptr_t(V - 1)));
    const int nvec = (n - head) / V, tail = n - head - nvec * V;
    bool d = false;
    if (V > 1)
    {
        int e = -1;
        if (lane < 16) e = lane < head ? lane : -1;
        else if (lane < 32) e = lane - 16 < tail ? n - tail + lane - 16 : -1;
        if (e >= 0) d = pa[e] != pb[e];
    }
    const TV* const va = reinterpret_cast<const TV*>(pa + head);
    const TV* const vb = reinterpret_cast<const TV*>(pb + head);
#pragma clang loop unroll(disable) vectorize(disable)
    for (int i = lane; i < nvec; i += 64) d |= differ(va[i], vb[i]);
    return d;
}

// A wave's rows of a rectangle: y = ys, ys + 4, ... inside every chunk of kDiffRows rows, the chunks `step` rows apart.
template <typename TV>
__device__ __forceinline__ bool rows_differ(const uint8_t* pa, long long pitch_a, const uint8_t* pb, long long pitch_b, int n, int ys, int y1, int step, int lane)
{
    bool d = false;
#pragma unroll 1
    for (; ys < y1; ys += step)
#pragma unroll 1
        for (int y = ys; y < min(ys + kDiffRows, y1); y += 4) d |= row_differs<TV>(pa + (long long)y * pitch_a, pb + (long long)y * pitch_b, n, lane);
    return d;
}

// n pairs of images at once (DiffArgs<1>: the one of rsr_diff_tiles), grid (tile, row chunk, pair * planes + plane): the compared bytes of a tile are one byte
// rectangle per plane of the format (PixFmt::planes: uint8 HWC one, a surface Y and UV, a planar image three), the same columns and rows
// in every plane but the UV plane of a surface.  A workgroup that finds a difference stores the 1 into row `pair` of the mask; the launch
// function zeroes the mask in front of the kernel.
template <int N> __global__ __launch_bounds__(256) void diff_tiles(const DiffArgs<N> a)
{
    const PixFmt f = pix_fmt(a.fmt, a.c);
    const int pair = N == 1 ? 0 : blockIdx.z / f.planes, rect = blockIdx.z - pair * f.planes; // (one pair: no division per workgroup)
    const int tile = blockIdx.x, yi = tile / a.nx, xi = tile - yi * a.nx;
    const DiffPair& p = a.pair[pair];
    uint8_t* const mask = a.mask + (long long)pair * a.nx * a.ny;
    if (!p.a)
    { // no predecessor: every tile of this frame is marked
        if (rect == 0 && blockIdx.y == 0 && threadIdx.x == 0) mask[tile] = 1;
        return;
    }
    int r[4];
    tile_source_rect(a.w, a.h, a.T, a.P, xi, yi, r);
    int bx0 = r[0] * f.es, bx1 = r[2] * f.es, y0 = r[1], y1 = r[3];
    if (f.pairs && rect == 1)
    { // the (U, V) pairs the decode of this rectangle reads: one chroma sample beyond its own, at every siting
        const int cx0 = max((r[0] >> 1) - 1, 0), cx1 = min(((r[2] - 1) >> 1) + 1, a.w / 2 - 1);
        bx0 = cx0 * 2 * f.es, bx1 = (cx1 + 1) * 2 * f.es;
        if (f.csy) y0 = max((r[1] >> 1) - 1, 0), y1 = min(((r[3] - 1) >> 1) + 1, a.h / 2 - 1) + 1; // (4:2:2: the rectangle's own rows)
    }
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint8_t* const pa = p.a + rect * p.plane_a + bx0;
    const uint8_t* const pb = p.b + rect * p.plane_b + bx0;
    // the widest access EVERY row of the rectangle allows: both images' rows then reach its boundary after the same head
    const unsigned mis = unsigned(reinterpret_cast<uintptr_t>(pa) ^ reinterpret_cast<uintptr_t>(pb)) | unsigned(p.pitch_a ^ p.pitch_b);
    const int n = bx1 - bx0, ys = y0 + blockIdx.y * kDiffRows + wave, step = gridDim.y * kDiffRows;
    bool d;
    if (!(mis & 15)) d = rows_differ<uint4>(pa, p.pitch_a, pb, p.pitch_b, n, ys, y1, step, lane);
    else if (!(mis & 3)) d = rows_differ<uint32_t>(pa, p.pitch_a, pb, p.pitch_b, n, ys, y1, step, lane);
    else d = rows_differ<uint8_t>(pa, p.pitch_a, pb, p.pitch_b, n, ys, y1, step, lane);
    if (__any(d) && lane == 0) mask[tile] = 1;
}

template <int N> hipError_t launch_diff_tiles(const DiffArgs<N>& a, hipStream_t st)
{
    const int ntiles = a.nx * a.ny;
    if (ntiles <= 0 || a.n <= 0) return hipSuccess;
    const hipError_t e = hipMemsetAsync(a.mask, 0, size_t(ntiles) * size_t(a.n), st); // every byte is written: the kernel only ever stores ones
    if (e != hipSuccess) return e;
    const long long padded = (long long)a.T + 2 * a.P; // rows of the tallest rectangle
    const int rows = padded < a.h ? int(padded) : a.h, chunks = (rows + kDiffRows - 1) / kDiffRows;
    const dim3 grid(ntiles, chunks < 1024 ? chunks : 1024, a.n * pix_fmt(a.fmt).planes), block(256); // (taller rectangles: the kernel strides over the chunks)
    hipLaunchKernelGGL(diff_tiles<N>, grid, block, 0, st, a);
    return hipGetLastError();
}
template hipError_t launch_diff_tiles<1>(const DiffArgs<1>&, hipStream_t);
template hipError_t launch_diff_tiles<kMaxMerge>(const DiffArgs<kMaxMerge>&, hipStream_t);

// =============================================================================================
// flat-alpha scan (engine option "alpha_adaptive"): which tiles' source rectangles hold more than one alpha value
// =============================================================================================
// Do the alpha samples of the n RGBA pixels behind p differ from ref?  One wave, lanes along the row.  T is the sample type; a pixel is PB =
// 4 * sizeof(T) bytes and its alpha sits in the high bits of the pixel's last dword (mask M: the top byte of a uint8 pixel's one dword, the
// top half of a uint16 pixel's second), so ref is the alpha shifted up there and low bits zero.  A row that starts on a pixel boundary is read in
// 16-byte pieces (4 / 2 pixels), 64 per step, behind a head of up to 3 / 1 pixels that brings it to that boundary and in front of a tail;
// head and tail are read one pixel's alpha dword per lane (lanes 0 .. 15 and 16 .. 31).  Any other row (a uint8 pitch or base that is no
// multiple of 4) is read one alpha sample per lane.  No byte outside [p, p + n * PB) is read.
template <typename T>
__device__ __forceinline__ bool row_alpha_varies(const uint8_t* p, int n, uint32_t ref, int lane)
{
    constexpr int PB = 4 * int(sizeof(T)), PPV = 16 / PB, SH = 32 - 8 * int(sizeof(T));
    constexpr uint32_t M = ~uint32_t(0) << SH;
    bool d = false;
    if (reinterpret_cast<uintptr_t>(p) & uintptr_t(PB - 1))
    {
        const T* const s = reinterpret_cast<const T*>(p) + 3;
#pragma clang loop unroll(disable) vectorize(disable)
        for (int i = lane; i < n; i += 64) d |= (uint32_t(s[4 * i]) << SH) != ref;
        return d;
    }
    const int head = min(n, int(((0 - reinterpret_cast<uintptr_t>(p)) & uintptr_t(15)) / PB));
    const int nvec = (n - head) / PPV, tail = n - head - nvec * PPV;
    int e = -1;
    if (lane < 16) e = lane < head ? lane : -1;
    else if (lane < 32) e = lane - 16 < tail ? n - tail + lane - 16 : -1;
    if (e >= 0) d = ((reinterpret_cast<const uint32_t*>(p + (long long)e * PB)[PB / 4 - 1] ^ ref) & M) != 0;
    const uint4* const v = reinterpret_cast<const uint4*>(p + head * PB);
#pragma clang loop unroll(disable) vectorize(disable)
    for (int i = lane; i < nvec; i += 64)
    {
        const uint4 x = v[i];
        const uint32_t m = sizeof(T) == 1 ? (x.x ^ ref) | (x.y ^ ref) | (x.z ^ ref) | (x.w ^ ref) : (x.y ^ ref) | (x.w ^ ref);
        d |= (m & M) != 0;
    }
    return d;
}

// Grid (tile, row chunk), the rows spread as diff_tiles spreads them: kDiffRows per workgroup and step, 4 per wave.  Every sample is compared
// with the alpha of the rectangle's first pixel; a wave that finds another value stores the 1, behind the launch function's memset.
template <typename T> __global__ __launch_bounds__(256) void alpha_flat_tiles(const FlatArgs a)
{
    constexpr int PB = 4 * int(sizeof(T)), SH = 32 - 8 * int(sizeof(T));
    const BaseTile t = a.tiles[blockIdx.x];
    const int w = a.ws[t.img], h = a.hs[t.img];
    const long long pitch = a.pitch[t.img];
    const int x0 = max(t.x_org, 0), x1 = min(t.x_org + t.tw, w), y0 = max(t.y_org, 0), y1 = min(t.y_org + t.th, h);
    const uint8_t* const base = a.imgs[t.img] + (long long)x0 * PB; // every offset from the image's base in 64 bits
    const uint32_t ref = uint32_t(reinterpret_cast<const T*>(base + (long long)y0 * pitch)[3]) << SH;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int step = gridDim.y * kDiffRows;
    bool d = false;
#pragma unroll 1
    for (int ys = y0 + blockIdx.y * kDiffRows + wave; ys < y1; ys += step)
#pragma unroll 1
        for (int y = ys; y < min(ys + kDiffRows, y1); y += 4) d |= row_alpha_varies<T>(base + (long long)y * pitch, x1 - x0, ref, lane);
    if (__any(d) && lane == 0) a.flags[blockIdx.x] = 1;
}

hipError_t launch_alpha_flat_tiles(const FlatArgs& a, int max_th, hipStream_t st)
{
    if (a.ntiles <= 0) return hipSuccess;
    const hipError_t e = hipMemsetAsync(a.flags, 0, size_t(a.ntiles), st); // every byte is written: the kernel only ever stores ones
    if (e != hipSuccess) return e;
    const int chunks = (max_th + kDiffRows - 1) / kDiffRows;
    const dim3 grid(a.ntiles, chunks < 1 ? 1 : (chunks < 1024 ? chunks : 1024)), block(256); // (taller rectangles: the kernel strides over the chunks)
    if (a.u16) hipLaunchKernelGGL(alpha_flat_tiles<uint16_t>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(alpha_flat_tiles<uint8_t>, grid, block, 0, st, a);
    return hipGetLastError();
}

// =============================================================================================
// frame sequences: the copy of the rectangles nobody computed
// =============================================================================================
// Rows of a rectangle per workgroup and step: 4 per wave.  An 800-row rectangle spreads over 50 workgroups, the 60 of a 1080p frame at x4
// over 3000: a dozen per CU, enough in flight for a pass that only waits for memory.
constexpr int kPropRows = 16;

// n bytes from ps to pd, one wave, lanes along the row; TV is the widest access the two addresses allow (they agree modulo sizeof(TV)).
// The head up to pd's boundary and the tail behind the last whole piece go byte by byte (lanes 0 .. 15 and 16 .. 31), the body in aligned
// pieces, 64 per step.  No byte outside [ps, ps + n) is read and none outside [pd, pd + n) written: the neighbours belong to someone else.
template <typename TV>
__device__ __forceinline__ void copy_row(uint8_t* pd, const uint8_t* ps, int n, int lane)
{
    constexpr int V = int(sizeof(TV));
    const int head = min(n, int((0 - reinterpret_cast<uintptr_t>(pd)) & uintptr_t(V - 1)));
    const int nvec = (n - head) / V, tail = n - head - nvec * V;
    if (V > 1)
    {
        int e = -1;
        if (lane < 16) e = lane < head ? lane : -1;
        else if (lane < 32) e = lane - 16 < tail ? n - tail + lane - 16 : -1;
        if (e >= 0) pd[e] = ps[e];
    }
    TV* const vd = reinterpret_cast<TV*>(pd + head);
    const TV* const vs = reinterpret_cast<const TV*>(ps + head);
    // four pieces per lane and step, all loads in front of the stores: a 2400-byte row (an 800-pixel uint8 rectangle) is in flight at once
#pragma clang loop unroll(disable) vectorize(disable)
    for (int i = lane; i < nvec; i += 256)
    {
        const bool b1 = i + 64 < nvec, b2 = i + 128 < nvec, b3 = i + 192 < nvec;
        const TV v0 = vs[i];
        TV v1 = v0, v2 = v0, v3 = v0;
        if (b1) v1 = vs[i + 64];
        if (b2) v2 = vs[i + 128];
        if (b3) v3 = vs[i + 192];
        vd[i] = v0;
        if (b1) vd[i + 64] = v1;
        if (b2) vd[i + 128] = v2;
        if (b3) vd[i + 192] = v3;
    }
}

// grid (rectangle, row chunk): wave w of a workgroup moves rows w, w + 4, ... of its chunks.  The access width is chosen per row, uniformly
// for the wave: 16 bytes where source and destination of the row are co-aligned (a window at the same offset in equally pitched surfaces;
// every row of it when the pitches agree modulo 16), 4 where they agree modulo 4, single bytes otherwise.
__global__ __launch_bounds__(256) void propagate_rects(const PropRect* __restrict__ rects)
{
    const PropRect r = rects[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int step = gridDim.y * kPropRows;
#pragma unroll 1
    for (int ys = blockIdx.y * kPropRows + wave; ys < r.rows; ys += step)
#pragma unroll 1
        for (int y = ys; y < min(ys - wave + kPropRows, r.rows); y += 4)
        {
            uint8_t* const pd = r.dst + (long long)y * r.dst_pitch;
            const uint8_t* const ps = r.src + (long long)y * r.src_pitch;
            const unsigned mis = __builtin_amdgcn_readfirstlane(unsigned(reinterpret_cast<uintptr_t>(pd) ^ reinterpret_cast<uintptr_t>(ps)));
            if (!(mis & 15)) copy_row<uint4>(pd, ps, r.width, lane);
            else if (!(mis & 3)) copy_row<uint32_t>(pd, ps, r.width, lane);
            else copy_row<uint8_t>(pd, ps, r.width, lane);
        }
}

hipError_t launch_propagate_rects(const PropRect* d_rects, int nrects, int max_rows, hipStream_t st)
{
    if (nrects <= 0 || max_rows <= 0) return hipSuccess;
    const int chunks = (max_rows + kPropRows - 1) / kPropRows;
    // (a table of many rectangles: the workgroups stride over the chunks rather than the grid growing beyond what the device keeps in flight)
    const int cap = nrects >= 8192 ? 1 : 8192 / nrects;
    const dim3 grid(nrects, chunks < cap ? chunks : cap), block(256);
    hipLaunchKernelGGL(propagate_rects, grid, block, 0, st, d_rects);
    return hipGetLastError();
}

// =============================================================================================
// three-plane YUV frames <-> surfaces (rsr_pack_planes, rsr_unpack_planes)
// =============================================================================================
// The idiom of propagate_rects: rows go to waves, lanes run along the row, the access is the widest the addresses of the row allow, and
// the samples in front of the first and behind the last whole piece go one by one.  What is new is done in registers: the shift of the
// P010 / P210 words and the interleave of a U and a V row into a UV row (and back).
constexpr int kPlaneRows = 4; // rows per workgroup and step, one per wave: a 4320-row plane spreads over 1024 workgroups (propagate_rects has many rectangles for that; a frame has two or three planes)

enum { kKeep = 0, kToHigh = 1, kToLow = 2 }; // a sample as it is | (word & 1023) << 6: planar -> P010 / P210 | word >> 6: the way back

template <int OP> __device__ __forceinline__ uint32_t conv2(uint32_t x) // two 16-bit words at once
{
    if (OP == kToHigh) return (x & 0x03ff03ffu) << 6;
    if (OP == kToLow) return (x >> 6) & 0x03ff03ffu;
    return x;
}
template <int OP, typename E> __device__ __forceinline__ E conv1(E x) // one sample (OP != kKeep: a uint16_t)
{
    if (OP == kToHigh) return E((x & 1023u) << 6);
    if (OP == kToLow) return E(x >> 6);
    return x;
}
template <int OP> __device__ __forceinline__ uint4 conv(uint4 v) { return make_uint4(conv2<OP>(v.x), conv2<OP>(v.y), conv2<OP>(v.z), conv2<OP>(v.w)); }
template <int OP> __device__ __forceinline__ uint32_t conv(uint32_t v) { return conv2<OP>(v); }
template <int OP> __device__ __forceinline__ uint16_t conv(uint16_t v) { return conv1<OP>(v); }

// copy_row for n bytes of 16-bit words that change on the way (OP != kKeep); pd, ps and n are even, so head and tail are whole words:
// lanes 0 .. 7 and 8 .. 15 move them.
template <typename TV, int OP>
__device__ __forceinline__ void convert_row(uint8_t* pd, const uint8_t* ps, int n, int lane)
{
    constexpr int V = int(sizeof(TV));
    const int head = min(n, int((0 - reinterpret_cast<uintptr_t>(pd)) & uintptr_t(V - 1)));
    const int nvec = (n - head) / V, tail = n - head - nvec * V;
    if (V > 2)
    {
        int e = -1;
        if (lane < 8) e = 2 * lane < head ? 2 * lane : -1;
        else if (lane < 16) e = 2 * (lane - 8) < tail ? n - tail + 2 * (lane - 8) : -1;
        if (e >= 0) *reinterpret_cast<uint16_t*>(pd + e) = conv1<OP>(*reinterpret_cast<const uint16_t*>(ps + e));
    }
    TV* const vd = reinterpret_cast<TV*>(pd + head);
    const TV* const vs = reinterpret_cast<const TV*>(ps + head);
#pragma clang loop unroll(disable) vectorize(disable)
    for (int i = lane; i < nvec; i += 256)
    {
        const bool b1 = i + 64 < nvec, b2 = i + 128 < nvec, b3 = i + 192 < nvec;
        const TV v0 = vs[i];
        TV v1 = v0, v2 = v0, v3 = v0;
        if (b1) v1 = vs[i + 64];
        if (b2) v2 = vs[i + 128];
        if (b3) v3 = vs[i + 192];
        vd[i] = conv<OP>(v0);
        if (b1) vd[i + 64] = conv<OP>(v1);
        if (b2) vd[i + 128] = conv<OP>(v2);
        if (b3) vd[i + 192] = conv<OP>(v3);
    }
}

// One row of a plane that keeps its layout (Y; every plane of a 4:4:4 frame): n bytes of ES-byte samples.  The width is chosen per row,
// uniformly for the wave, as propagate_rects chooses it; 16-bit rows fall back to words, not bytes.
template <int ES, int OP>
__device__ __forceinline__ void move_row(uint8_t* pd, const uint8_t* ps, int n, int lane)
{
    const unsigned mis = __builtin_amdgcn_readfirstlane(unsigned(reinterpret_cast<uintptr_t>(pd) ^ reinterpret_cast<uintptr_t>(ps)));
    if (OP == kKeep)
    {
        if (!(mis & 15)) copy_row<uint4>(pd, ps, n, lane);
        else if (!(mis & 3)) copy_row<uint32_t>(pd, ps, n, lane);
        else if (ES == 2) copy_row<uint16_t>(pd, ps, n, lane);
        else copy_row<uint8_t>(pd, ps, n, lane);
    }
    else
    {
        if (!(mis & 15)) convert_row<uint4, OP>(pd, ps, n, lane);
        else if (!(mis & 3)) convert_row<uint32_t, OP>(pd, ps, n, lane);
        else convert_row<uint16_t, OP>(pd, ps, n, lane);
    }
}

// Two source bytes of U and two of V (the low halves of u and v) as the four bytes of UV they make: two pairs of bytes, one pair of words.
template <int ES> __device__ __forceinline__ uint32_t weave2(uint32_t u, uint32_t v)
{
    if (ES == 1) return (u & 0xffu) | ((v & 0xffu) << 8) | ((u & 0xff00u) << 8) | ((v & 0xff00u) << 16);
    return (u & 0xffffu) | (v << 16);
}
template <int ES> __device__ __forceinline__ void unweave2(uint32_t d, uint32_t& u, uint32_t& v) // ... and back, into the low halves
{
    if (ES == 1) u = (d & 0xffu) | ((d >> 8) & 0xff00u), v = ((d >> 8) & 0xffu) | ((d >> 16) & 0xff00u);
    else u = d & 0xffffu, v = d >> 16;
}
template <int ES, int OP> __device__ __forceinline__ uint4 weave(uint2 u, uint2 v)
{
    return make_uint4(conv2<OP>(weave2<ES>(u.x, v.x)), conv2<OP>(weave2<ES>(u.x >> 16, v.x >> 16)), conv2<OP>(weave2<ES>(u.y, v.y)),
                      conv2<OP>(weave2<ES>(u.y >> 16, v.y >> 16)));
}
template <int ES, int OP> __device__ __forceinline__ uint32_t weave(uint16_t u, uint16_t v) { return conv2<OP>(weave2<ES>(u, v)); }
template <int ES, int OP> __device__ __forceinline__ void unweave(uint4 d, uint2& u, uint2& v)
{
    uint32_t u0, v0, u1, v1, u2, v2, u3, v3;
    unweave2<ES>(conv2<OP>(d.x), u0, v0), unweave2<ES>(conv2<OP>(d.y), u1, v1), unweave2<ES>(conv2<OP>(d.z), u2, v2), unweave2<ES>(conv2<OP>(d.w), u3, v3);
    u = make_uint2(u0 | (u1 << 16), u2 | (u3 << 16)), v = make_uint2(v0 | (v1 << 16), v2 | (v3 << 16));
}
template <int ES, int OP> __device__ __forceinline__ void unweave(uint32_t d, uint16_t& u, uint16_t& v)
{
    uint32_t u0, v0;
    unweave2<ES>(conv2<OP>(d), u0, v0);
    u = uint16_t(u0), v = uint16_t(v0);
}

// np (U, V) pairs of ES-byte samples between a UV row and a U and a V row, one wave.  PACK: UV[2X] = U[X], UV[2X + 1] = V[X]; else the way
// back.  A piece is one SV of U, one of V and one DV (twice as wide) of UV; the caller has seen that the three addresses reach the
// boundaries of their pieces after the same number of pairs.  Those head pairs and the tail behind the last whole piece go sample by
// sample (lanes 0 .. 7 and 8 .. 15: a piece has at most 8 pairs).
template <bool PACK, int ES, int OP, typename SV, typename DV>
__device__ __forceinline__ void pair_row(uint8_t* puv, uint8_t* pu, uint8_t* pv, int np, int lane)
{
    using E = std::conditional_t<ES == 1, uint8_t, uint16_t>;
    constexpr int K = int(sizeof(SV)) / ES; // pairs per piece
    static_assert(sizeof(DV) == 2 * sizeof(SV) && K >= 1 && K <= 8, "a UV piece is one piece of U and one of V");
    const int head = min(np, int((0 - reinterpret_cast<uintptr_t>(pu)) & uintptr_t(sizeof(SV) - 1)) / ES);
    const int nvec = (np - head) / K, tail = np - head - nvec * K;
    E* const euv = reinterpret_cast<E*>(puv);
    E* const eu = reinterpret_cast<E*>(pu);
    E* const ev = reinterpret_cast<E*>(pv);
    if (K > 1)
    {
        int e = -1;
        if (lane < 8) e = lane < head ? lane : -1;
        else if (lane < 16) e = lane - 8 < tail ? np - tail + lane - 8 : -1;
        if (e >= 0)
        {
            if (PACK) euv[2 * e] = conv1<OP>(eu[e]), euv[2 * e + 1] = conv1<OP>(ev[e]);
            else eu[e] = conv1<OP>(euv[2 * e]), ev[e] = conv1<OP>(euv[2 * e + 1]);
        }
    }
    DV* const vuv = reinterpret_cast<DV*>(puv + head * 2 * ES);
    SV* const vu = reinterpret_cast<SV*>(pu + head * ES);
    SV* const vv = reinterpret_cast<SV*>(pv + head * ES);
#pragma clang loop unroll(disable) vectorize(disable)
    for (int i = lane; i < nvec; i += 64)
    {
        if (PACK) vuv[i] = weave<ES, OP>(vu[i], vv[i]);
        else
        {
            SV su, sv;
            unweave<ES, OP>(vuv[i], su, sv);
            vu[i] = su, vv[i] = sv;
        }
    }
}

// The same at any addresses: a lane moves one pair, sample by sample.
template <bool PACK, int ES, int OP>
__device__ __forceinline__ void pair_row_samples(uint8_t* puv, uint8_t* pu, uint8_t* pv, int np, int lane)
{
    using E = std::conditional_t<ES == 1, uint8_t, uint16_t>;
    E* const euv = reinterpret_cast<E*>(puv);
    E* const eu = reinterpret_cast<E*>(pu);
    E* const ev = reinterpret_cast<E*>(pv);
#pragma clang loop unroll(disable) vectorize(disable)
    for (int i = lane; i < np; i += 64)
        if (PACK) euv[2 * i] = conv1<OP>(eu[i]), euv[2 * i + 1] = conv1<OP>(ev[i]);
        else eu[i] = conv1<OP>(euv[2 * i]), ev[i] = conv1<OP>(euv[2 * i + 1]);
}

// grid (row chunk, plane, frame): plane 0 is Y, plane 1 the UV plane of a surface -- made of, or taken apart into, the planes U and V --
// or, 4:4:4, U, and plane 2 V.  PACK: planes -> surface.  The UV piece is 16 bytes (8 of U, 8 of V) where the UV row starts on a whole
// pair and half its address agrees with the U and the V address modulo 8, 4 bytes where they agree modulo 2, single samples otherwise.
template <bool PACK, int ES, int OP>
__global__ __launch_bounds__(256) void move_planes(const PlanesArgs a)
{
    const PixFmt f = pix_fmt(a.fmt);
    const PlaneFrame& fr = a.f[blockIdx.z];
    const int part = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int step = gridDim.x * kPlaneRows;
    const bool pairs = f.pairs && part == 1;
    const int rows = part ? a.h >> f.csy : a.h, n = a.w * ES;
    uint8_t* const plane = part == 0 ? fr.y : part == 1 ? fr.u : fr.v;
    const long long ppitch = part ? fr.c_pitch : fr.y_pitch;
    uint8_t* const surf = fr.surf + part * fr.plane;
#pragma unroll 1
    for (int ys = blockIdx.x * kPlaneRows + wave; ys < rows; ys += step)
#pragma unroll 1
        for (int y = ys; y < min(ys - wave + kPlaneRows, rows); y += 4)
        {
            uint8_t* const ps = surf + (long long)y * fr.row;
            uint8_t* const pp = plane + (long long)y * ppitch;
            if (!pairs)
            {
                if (PACK) move_row<ES, OP>(ps, pp, n, lane);
                else move_row<ES, OP>(pp, ps, n, lane);
                continue;
            }
            uint8_t* const pv = fr.v + (long long)y * ppitch;
            const uintptr_t auv = reinterpret_cast<uintptr_t>(ps), half = auv >> 1;
            const unsigned mis = __builtin_amdgcn_readfirstlane(unsigned((half ^ reinterpret_cast<uintptr_t>(pp)) | (half ^ reinterpret_cast<uintptr_t>(pv))) |
                                                                (unsigned(auv) & unsigned(2 * ES - 1) ? 15u : 0u));
            if (!(mis & 7)) pair_row<PACK, ES, OP, uint2, uint4>(ps, pp, pv, a.w >> 1, lane);
            else if (!(mis & 1)) pair_row<PACK, ES, OP, uint16_t, uint32_t>(ps, pp, pv, a.w >> 1, lane);
            else pair_row_samples<PACK, ES, OP>(ps, pp, pv, a.w >> 1, lane);
        }
}

hipError_t launch_move_planes(const PlanesArgs& a, bool pack, hipStream_t st)
{
    const PixFmt f = pix_fmt(a.fmt);
    if (a.n <= 0 || a.h <= 0 || !f.bits) return hipSuccess;
    const int chunks = (a.h + kPlaneRows - 1) / kPlaneRows;
    const dim3 grid(chunks < 4096 ? chunks : 4096, f.planes, a.n), block(256); // (a taller frame: the workgroups stride over the chunks)
    void (*k)(const PlanesArgs);
    if (f.es == 1) k = pack ? move_planes<true, 1, kKeep> : move_planes<false, 1, kKeep>;
    else if (!f.high) k = pack ? move_planes<true, 2, kKeep> : move_planes<false, 2, kKeep>;
    else k = pack ? move_planes<true, 2, kToHigh> : move_planes<false, 2, kToLow>;
    hipLaunchKernelGGL(k, grid, block, 0, st, a);
    return hipGetLastError();
}

// =============================================================================================
// model self-check: range probe and output compare (Engine::selfcheck)
// =============================================================================================
constexpr int kCheckBlocks = 512; // grid-stride: at most this many workgroups of 256

__device__ __forceinline__ unsigned wave_max_u32(unsigned v)
{
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v)
{
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}

// |fp16| as its 15-bit pattern orders like the value: the maximum is taken on the patterns, the one conversion to float at the end.
__global__ __launch_bounds__(256) void range_probe(const char* base, long long plane_stride, int nplanes, long long vec_per_plane,
                                                   unsigned* peak_bits, unsigned long long* nonfinite)
{
    unsigned peak = 0, bad = 0;
    const long long total = vec_per_plane * nplanes, step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += step)
    {
        const long long p = i / vec_per_plane, v = i - p * vec_per_plane;
        const uint4 q = *reinterpret_cast<const uint4*>(base + p * plane_stride + v * 16);
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            const unsigned lo = w[k] & 0x7fffu, hi = (w[k] >> 16) & 0x7fffu;
            if (lo >= 0x7c00u) bad++; else peak = max(peak, lo);
            if (hi >= 0x7c00u) bad++; else peak = max(peak, hi);
        }
    }
    peak = wave_max_u32(peak);
    bad = wave_sum_u32(bad);
    if ((threadIdx.x & 63) == 0)
    {
        const unsigned short hb = (unsigned short)peak;
        _Float16 hv;
        __builtin_memcpy(&hv, &hb, 2);
        if (peak) atomicMax(peak_bits, __float_as_uint((float)hv));
        if (bad) atomicAdd(nonfinite, (unsigned long long)bad);
    }
}

void launch_range_probe(const void* base, long long plane_stride, int nplanes, long long halfs_per_plane, unsigned* peak_bits,
                        unsigned long long* nonfinite, hipStream_t st)
{
    const long long vpp = halfs_per_plane / 8, total = vpp * nplanes;
    if (total <= 0) return;
    const unsigned grid = (unsigned)((total + 1023) / 1024 < kCheckBlocks ? (total + 1023) / 1024 : kCheckBlocks);
    hipLaunchKernelGGL(range_probe, dim3(grid), dim3(256), 0, st, static_cast<const char*>(base), plane_stride, nplanes, vpp, peak_bits,
                       nonfinite);
}

__global__ __launch_bounds__(256) void output_compare(const uint16_t* a, const float* b, long long nvec, unsigned* res, unsigned long long* ndiff)
{
    unsigned err = 0, qmax = 0, cnt = 0; // err: bits of a non-negative float
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += step)
    {
        const half8 ha = *reinterpret_cast<const half8*>(a + i * 8);
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(b + i * 8), b1 = *reinterpret_cast<const f32x4*>(b + i * 8 + 4);
#pragma unroll
        for (int k = 0; k < 8; k++)
        {
            const float va = (float)ha[k], vb = k < 4 ? b0[k] : b1[k - 4];
            const float d = fabsf(va - vb);
            if (d == d) err = max(err, __float_as_uint(d)); // (+inf orders above every finite value; NaN is left out)
            else err = max(err, 0x7f800000u);
            const int qa = post_store(va * 255.f), qb = post_store(vb * 255.f);
            const unsigned qd = (unsigned)(qa > qb ? qa - qb : qb - qa);
            qmax = max(qmax, qd);
            cnt += qd != 0;
        }
    }
    err = wave_max_u32(err);
    qmax = wave_max_u32(qmax);
    cnt = wave_sum_u32(cnt);
    if ((threadIdx.x & 63) == 0)
    {
        if (err) atomicMax(&res[0], err);
        if (qmax) atomicMax(&res[1], qmax);
        if (cnt) atomicAdd(ndiff, (unsigned long long)cnt);
    }
}

void launch_output_compare(const uint16_t* a, const float* b, long long n, unsigned* res, unsigned long long* ndiff, hipStream_t st)
{
    const long long nvec = n / 8;
    if (nvec <= 0) return;
    const unsigned grid = (unsigned)((nvec + 1023) / 1024 < kCheckBlocks ? (nvec + 1023) / 1024 : kCheckBlocks);
    hipLaunchKernelGGL(output_compare, dim3(grid), dim3(256), 0, st, a, b, nvec, res, ndiff);
}

// =============================================================================================
// network interpolation: the active blob from two resident ones (rsr_set_blend)
// =============================================================================================
// (u * a) + (t * b), three roundings.  hipcc contracts a product and a sum into one fused multiply-add by default -- also through
// __fmul_rn / __fadd_rn, which are a plain * and + in this toolchain's headers -- so the two operators stand under the pragma that
// forbids it: the rule of include/realsr_hip.h is the unfused one, what numpy and the host function compute.
__device__ __forceinline__ float blend1(float u, float a, float t, float b)
{
#pragma clang fp contract(off)
    const float p = u * a;
    const float q = t * b;
    return p + q;
}

// One 16-byte unit: four fp32 biases, or eight fp16 weights through fp32 and back (round to nearest even: the conversion's default).
__device__ __forceinline__ uint4 blend_unit(uint4 qa, uint4 qb, float t, float u, bool f32)
{
    uint4 r;
    if (f32)
    {
        f32x4 a, b, c;
        __builtin_memcpy(&a, &qa, 16);
        __builtin_memcpy(&b, &qb, 16);
#pragma unroll
        for (int k = 0; k < 4; k++) c[k] = blend1(u, a[k], t, b[k]);
        __builtin_memcpy(&r, &c, 16);
    }
    else
    {
        half8 a, b, c;
        __builtin_memcpy(&a, &qa, 16);
        __builtin_memcpy(&b, &qb, 16);
#pragma unroll
        for (int k = 0; k < 8; k++) c[k] = (_Float16)blend1(u, (float)a[k], t, (float)b[k]);
        __builtin_memcpy(&r, &c, 16);
    }
    return r;
}

// A workgroup takes whole chunks, grid-stride: thread i of it the units i, i + 256, i + 512, i + 768 of the chunk -- a wave-instruction
// moves 1 KiB contiguously.  The eight loads of a thread (four per blob) are issued in front of the arithmetic and the stores; a unit
// beyond the chunk's end is neither loaded nor stored.  The chunk's three words are the same for the whole workgroup (scalar loads).
__global__ __launch_bounds__(256) void blend_blob(const BlendChunk* __restrict__ chunks, int nchunks, const char* __restrict__ a, const char* __restrict__ b,
                                                  char* __restrict__ c, float t, float u)
{
#pragma unroll 1
    for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x)
    {
        const BlendChunk k = chunks[ch];
        const int units = int(k.units), i = threadIdx.x;
        const bool f32 = k.f32 != 0;
        const uint4* const va = reinterpret_cast<const uint4*>(a + k.off);
        const uint4* const vb = reinterpret_cast<const uint4*>(b + k.off);
        uint4* const vc = reinterpret_cast<uint4*>(c + k.off);
        const bool b0 = i < units, b1 = i + 256 < units, b2 = i + 512 < units, b3 = i + 768 < units;
        uint4 a0 = {}, a1 = {}, a2 = {}, a3 = {}, c0 = {}, c1 = {}, c2 = {}, c3 = {};
        if (b0) a0 = va[i], c0 = vb[i];
        if (b1) a1 = va[i + 256], c1 = vb[i + 256];
        if (b2) a2 = va[i + 512], c2 = vb[i + 512];
        if (b3) a3 = va[i + 768], c3 = vb[i + 768];
        if (b0) vc[i] = blend_unit(a0, c0, t, u, f32);
        if (b1) vc[i + 256] = blend_unit(a1, c1, t, u, f32);
        if (b2) vc[i + 512] = blend_unit(a2, c2, t, u, f32);
        if (b3) vc[i + 768] = blend_unit(a3, c3, t, u, f32);
    }
}
static_assert(kBlendChunkUnits == 4 * 256, "blend_blob: four units per thread of a 256-thread workgroup");

hipError_t launch_blend_blob(const BlendChunk* d_chunks, int nchunks, const void* a, const void* b, void* c, float t, int num_cu, hipStream_t st)
{
    if (nchunks <= 0) return hipSuccess;
    // a pass that only waits for memory: eight workgroups per CU (eight waves per SIMD) cover the device, the chunks beyond are strided over
    const int cap = (num_cu > 0 ? num_cu : 256) * 8;
    const unsigned grid = unsigned(nchunks < cap ? nchunks : cap);
    hipLaunchKernelGGL(blend_blob, dim3(grid), dim3(256), 0, st, d_chunks, nchunks, static_cast<const char*>(a), static_cast<const char*>(b),
                       static_cast<char*>(c), t, 1.f - t);
    return hipGetLastError();
}

} // namespace rsr
