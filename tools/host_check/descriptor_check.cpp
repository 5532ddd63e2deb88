// descriptor_check.cpp -- the pure host code of the device entry points under AddressSanitizer + UBSan: no GPU, no Python.
//
// Includes engine.cpp itself (so the file-static table builder is in reach) and links the kernel objects of the library build; nothing
// here initialises HIP.  `make -C realsr-ncnn-vulkan_amd/csrc host_check` builds and runs it.
//   1. image_refs: the refusal table of tests/test_gpu_device_refusals.py (every row RSR_E_ARG, no ImageRef written past its slot) and
//      valid layouts: packed, strided, n = 16 -- one format of every family (uint8 HWC, planar float, YUV 4:2:0, 4:2:2, 4:4:4).
//   1b. out_admit: the engine's wording of every kind of refusal, and the sizes each family takes.
//   2. fill_batch: batches of 1, 7 and 60 tiles with and without TTA; every table entry is read back and range-checked.
//   3. choose_conv_flow: which conv3x3_flow kernel, patch ring, LDS size and grid every convolution of the network and of rsr_conv3x3 gets
//      under flow_flags 1 / 2 / 4 / 8 and in precise mode, against rows written out by hand; every plan names a row of the variant list.
//   4. WsLayout (workspace.h): buffer sizes and the 6,048 / 6,400 B per pixel against the formulas written out by hand, no two planes or
//      slots overlap, every plane (lo pair planes included) starts a whole number of planes behind its buffer's start in either mode; and
//      PlanKey: keys that differ in any one field compare unequal.
//   5. fetch_plan / fetch_chunks (the download of a host call): for five tile grids, RGB and RGBA, x4, x2 and x3/2, EVERY tile range and every
//      early half, the spans cover the union of the range's output rectangles byte for byte, each byte once, inside the rows the device
//      buffer holds; and the staging chunks of every span tile it in order, slot by slot, a rectangle narrower than a row being refused.
#include "../../realsr-ncnn-vulkan_amd/csrc/engine.cpp"

#include <cinttypes>

using namespace rsr;

static int failures = 0;
#define CHECK(cond)                                                              \
    do                                                                           \
    {                                                                            \
        if (!(cond))                                                             \
        {                                                                        \
            std::fprintf(stderr, "%s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, last_error()); \
            failures++;                                                          \
        }                                                                        \
    } while (0)

static void descriptors()
{
    const int W = 40, H = 36;
    alignas(16) static unsigned char mem[64];
    void* p = mem;
    const OutRatio x4;
    struct Row
    {
        const char* name;
        int fmt, w, c;
        rsr_image im;
    };
    const Row bad[] = {
        {"null data", RSR_FMT_U8_HWC, W, 3, {nullptr, 0, 0}},
        {"row pitch one below packed", RSR_FMT_U8_HWC, W, 3, {p, 3 * W - 1, 0}},
        {"negative plane pitch", RSR_FMT_F32_CHW, W, 3, {p, 0, -1}},
        {"f16 at an odd address", RSR_FMT_F16_CHW, W, 3, {mem + 1, 0, 0}},
        {"pitch no element multiple", RSR_FMT_F16_CHW, W, 3, {p, 2 * W + 1, 0}},
        {"odd w with NV12", RSR_FMT_NV12, W + 1, 3, {p, 0, 0}},
        {"odd w with P210", RSR_FMT_P210, W + 1, 3, {p, 0, 0}},
        {"NV16 row pitch below packed", RSR_FMT_NV16, W, 3, {p, W - 1, 0}},
        {"YUV444P10 at an odd address", RSR_FMT_YUV444P10, W, 3, {mem + 1, 0, 0}},
        {"YUV444P10 plane pitch no element multiple", RSR_FMT_YUV444P10, W, 3, {p, 0, 2ll * W * H + 1}},
        {"YUV444P with c == 4", RSR_FMT_YUV444P, W, 4, {p, 0, 0}},
        {"w beyond 2^24", RSR_FMT_U8_HWC, (1 << 24) + 1, 3, {p, 0, 0}},
        {"unknown format", 7, W, 3, {p, 0, 0}},
        {"planar with c == 4", RSR_FMT_F16_CHW, W, 4, {p, 0, 0}},
    };
    for (const Row& r : bad)
        for (const OutRatio* os : {static_cast<const OutRatio*>(nullptr), &x4})
            for (int at : {0, 2})
            { // the bad descriptor first and last of three; the slots behind it must stay untouched
                rsr_image im[3] = {{p, 0, 0}, {p, 0, 0}, {p, 0, 0}};
                if (os && r.w != W && (r.fmt == RSR_FMT_NV12 || r.fmt == RSR_FMT_P210)) continue; // (x4 of an odd width is even: it is the input descriptor that refuses this call)
                im[at] = r.im;
                std::vector<ImageRef> out(3); // exactly three: a write past the array is ASan's to report
                const int rc = image_refs(3, im, r.fmt, r.w, H, r.c, os, "image", 0, out.data());
                CHECK(rc == RSR_E_ARG);
                CHECK(std::strstr(last_error(), at == 0 || r.w != W || r.fmt == 7 || r.c == 4 ? "image 0: " : "image 2: ") == last_error());
                if (rc != RSR_E_ARG) std::fprintf(stderr, "  (%s, bad descriptor %d)\n", r.name, at);
            }
    // valid layouts
    {
        ImageRef out;
        const rsr_image packed = {p, 0, 0};
        CHECK(image_refs(1, &packed, RSR_FMT_U8_HWC, W, H, 3, nullptr, "image", 0, &out) == RSR_OK && out.data == p && out.row == 3 * W && out.plane == 0);
        CHECK(image_refs(1, &packed, RSR_FMT_U8_HWC, W, H, 3, &x4, "image", 0, &out) == RSR_OK && out.row == 12 * W);
        CHECK(image_refs(1, &packed, RSR_FMT_F32_CHW, W, H, 3, nullptr, "image", 0, &out) == RSR_OK && out.row == 4 * W && out.plane == 4ll * W * H);
        CHECK(image_refs(1, &packed, RSR_FMT_NV12, W, H, 3, nullptr, "image", 0, &out) == RSR_OK && out.row == W && out.plane == (long long)W * H);
        const rsr_image strided = {mem + 4, 4 * W + 20, (4 * W + 20) * (H + 3ll)};
        CHECK(image_refs(1, &strided, RSR_FMT_F32_CHW, W, H, 3, nullptr, "previous output", -1, &out) == RSR_OK && out.data == mem + 4 && out.row == 4 * W + 20 &&
              out.plane == (4 * W + 20) * (H + 3ll));
        const rsr_image odd_u8 = {mem + 1, 3 * W + 1, 0};
        CHECK(image_refs(1, &odd_u8, RSR_FMT_U8_HWC, W, H, 3, nullptr, "image", 0, &out) == RSR_OK && out.row == 3 * W + 1);
        const rsr_image far_row = {p, 0x7fffffffll, 0};
        CHECK(image_refs(1, &far_row, RSR_FMT_U8_HWC, W, 3, 3, nullptr, "image", 0, &out) == RSR_OK && out.row == 0x7fffffffll);
        CHECK(image_refs(1, &packed, RSR_FMT_P010, W, H, 3, nullptr, "image", 0, &out) == RSR_OK && out.row == 2 * W && out.plane == 2ll * W * H);
        CHECK(image_refs(1, &packed, RSR_FMT_NV16, W, H + 1, 3, nullptr, "image", 0, &out) == RSR_OK && out.row == W && out.plane == W * (H + 1ll)); // (4:2:2: any h)
        CHECK(image_refs(1, &packed, RSR_FMT_P210, W, H, 3, &x4, "image", 0, &out) == RSR_OK && out.row == 8 * W && out.plane == 32ll * W * H);
        CHECK(image_refs(1, &packed, RSR_FMT_YUV444P, W + 1, H + 1, 3, nullptr, "image", 0, &out) == RSR_OK && out.row == W + 1 && out.plane == (W + 1ll) * (H + 1)); // (4:4:4: any w and h)
        const rsr_image strided444 = {mem + 2, 2 * W + 6, (2 * W + 6) * (H + 1ll)};
        CHECK(image_refs(1, &strided444, RSR_FMT_YUV444P10, W, H, 3, nullptr, "image", 0, &out) == RSR_OK && out.data == mem + 2 && out.row == 2 * W + 6 && out.plane == (2 * W + 6) * (H + 1ll));
        long long row = 0, plane = 0;
        CHECK(image_layout(RSR_FMT_NV16, W, H, 3, W + 4, 0, &row, &plane) == RSR_OK && row == W + 4 && plane == (W + 4ll) * H);
        CHECK(image_layout(RSR_FMT_NV12, W, H + 1, 3, 0, 0, &row, &plane) == RSR_E_ARG && !std::strcmp(last_error(), "a YUV 4:2:0 surface needs an even width and height"));
        CHECK(image_layout(RSR_FMT_NV16, W + 1, H, 3, 0, 0, &row, &plane) == RSR_E_ARG && !std::strcmp(last_error(), "a YUV 4:2:2 surface needs an even width"));
        std::vector<rsr_image> many(16, packed);
        std::vector<ImageRef> outs(16);
        CHECK(image_refs(16, many.data(), RSR_FMT_F16_CHW, W, H, 3, nullptr, "image", 0, outs.data()) == RSR_OK && outs[15].row == 2 * W && outs[15].plane == 2ll * W * H);
    }
}

// out_admit as the engine asks it: what each family takes, and the engine's wording of every kind of refusal
static void admission()
{
    struct Row
    {
        int fmt, w, h, T;
        OutRatio r;
        const char* text; // null: admitted
    };
    const Row rows[] = {
        {RSR_FMT_U8_HWC, 35, 25, 16, OutRatio(1, 1), nullptr},
        {RSR_FMT_F16_CHW, 35, 25, 16, OutRatio(3, 2), "output ratio 3/2: w, h and tilesize times 3 must be multiples of 2 (35 x 25 at tile 16)"},
        {RSR_FMT_F32_CHW, 36, 26, 16, OutRatio(3, 2), nullptr},
        {RSR_FMT_YUV444P, 35, 25, 16, OutRatio(1, 1), nullptr},
        {RSR_FMT_YUV444P10, 35, 25, 16, OutRatio(3, 2, 1, 1), "output ratios 3/2 x 1/1: w and tilesize times 3 must be multiples of 2, h and tilesize times 1 multiples of 1 (35 x 25 at tile 16)"},
        {RSR_FMT_NV12, 36, 26, 16, OutRatio(1, 1), nullptr},
        {RSR_FMT_NV12, 35, 26, 16, OutRatio(1, 1), "a YUV 4:2:0 output needs w * out_scale, h * out_scale and tilesize * out_scale even"},
        {RSR_FMT_P010, 35, 25, 3, OutRatio(2, 1), nullptr},
        {RSR_FMT_NV12, 35, 26, 16, OutRatio(3, 2), "YUV 4:2:0 output at output ratio 3/2: w, h and tilesize times 3 must be multiples of 2 (35 x 26 at tile 16)"},
        {RSR_FMT_P010, 36, 26, 6, OutRatio(3, 2), "a YUV 4:2:0 output at ratio 3/2 needs w, h and tilesize times 3/2 even (36 x 26 at tile 6)"},
        {RSR_FMT_NV12, 36, 26, 16, OutRatio(3, 2, 1, 1), nullptr},
        {RSR_FMT_NV12, 36, 25, 16, OutRatio(3, 2, 1, 1), "a YUV 4:2:0 output at ratios 3/2 x 1/1 needs w and tilesize times 3/2 and h and tilesize times 1/1 even (36 x 25 at tile 16)"},
        {RSR_FMT_NV16, 36, 25, 16, OutRatio(1, 1), nullptr},
        {RSR_FMT_NV16, 35, 25, 16, OutRatio(1, 1), "a YUV 4:2:2 output needs w * out_scale and tilesize * out_scale even"},
        {RSR_FMT_P210, 36, 26, 6, OutRatio(3, 2), "a YUV 4:2:2 output at ratios 3/2 needs w and tilesize times 3/2 even (36 x 26 at tile 6)"},
        {RSR_FMT_P210, 36, 25, 16, OutRatio(3, 2, 1, 1), nullptr},
        {RSR_FMT_NV16, 35, 25, 16, OutRatio(8, 3, 9, 4),
         "YUV 4:2:2 output at output ratios 8/3 x 9/4: w and tilesize times 8 must be multiples of 3, h and tilesize times 9 multiples of 4 (35 x 25 at tile 16)"},
    };
    for (const Row& r : rows)
    {
        const int rc = out_admit(pix_fmt(r.fmt), r.w, r.h, r.T, r.r, kWhoEngine);
        CHECK(rc == (r.text ? RSR_E_ARG : RSR_OK));
        if (r.text) CHECK(!std::strcmp(last_error(), r.text));
    }
    CHECK(pix_fmt(7).known() == false && fmt_check(pix_fmt(7), 3) == RSR_E_ARG && fmt_check(pix_fmt(RSR_FMT_U8_HWC, 4), 4) == RSR_OK && fmt_check(pix_fmt(RSR_FMT_NV16), 4) == RSR_E_ARG);
}

static void batches()
{
    const int T = 200, P = 10, scale = 4;
    std::vector<BaseTile> all;
    long long cap = 0;
    int mtw = 0, mth = 0;
    image_tiles(1920, 1080, T, P, scale, 0, 60, 0, all, cap, mtw, mth);
    CHECK(all.size() == 60 && mtw == T + 2 * P && cap == (long long)(T + 2 * P) * (T + 2 * P));
    for (const bool tta : {false, true})
        for (const int count : {1, 7, 60})
            for (const bool fold : {false, true})
            {
                Plan::Batch b;
                const int per = tta ? 8 : 1;
                const size_t bytes = fill_batch(b, 3, count, [&](int i) { BaseTile t = all[size_t((i * 7) % 60)]; t.img = i % 3; return t; }, tta, P * scale, true, fold, 0);
                CHECK(b.tile0 == 3 && b.ntiles == count && b.nslots == count * per && int(b.tiles.size()) == count && int(b.dims.size()) == count * per);
                CHECK(b.trim4 == P * scale && bytes == batch_table_bytes(b) && bytes % 256 == 0);
                for (int i = 0; i < count; i++) CHECK(b.tiles[size_t(i)].slot0 == i * per && b.tiles[size_t(i)].img == i % 3);
                for (int lvl = 0; lvl < 3; lvl++)
                {
                    CHECK(int(b.item_start[lvl].size()) == b.nslots + 1 && b.item_start[lvl].back() == int(b.items[lvl].size()));
                    for (const WorkItem& it : b.items[lvl])
                    {
                        CHECK(it.slot >= 0 && it.slot < b.nslots);
                        const TileDim& d = b.dims[size_t(it.slot)];
                        CHECK(it.H == d.h << lvl && it.W == d.w << lvl && it.y0 >= 0 && it.y0 < it.H && (it.x0 & ~kFoldBit) >= 0 && (it.x0 & ~kFoldBit) < it.W);
                    }
                }
            }
}

// choose_conv_flow: ConvArgs as Engine::run_network and Engine::conv_test fill them, against rows written out by hand
static unsigned char flow_mem[64];
static ConvArgs flow_conv(int n0, int n1, int lrelu = 0, int precise = 0)
{
    ConvArgs a{};
    a.n0 = n0;
    a.n1 = n1;
    a.wpk16 = flow_mem;
    a.out16.base = flow_mem + 1;
    a.lrelu = lrelu;
    a.precise = precise;
    a.nitems = 1000;
    a.pr = -7; // (a streamed launch leaves it alone)
    return a;
}
static ConvArgs flow_residual(int n1, bool own_input, bool second, int precise)
{
    ConvArgs a = flow_conv(4, n1, 0, precise);
    a.res1_kind = 1;
    a.res1_in_acc = own_input;
    a.res1.base = flow_mem + 2;
    a.s1 = 0.2f;
    a.lo1_off = precise ? 4096 : 0;
    a.out_lo_off = precise ? 8192 : 0;
    if (second)
    {
        a.res2_kind = 1;
        a.res2.base = flow_mem + 3;
        a.s2 = 0.2f;
    }
    return a;
}
static ConvArgs flow_last(int n0, int kind, int precise) // kind 0: the planar blob, 1: the uint8 image, 2: a planar float image
{
    ConvArgs a = flow_conv(n0, 0, 0, precise);
    a.out16.base = nullptr;
    a.waux = flow_mem + 4;
    if (kind == 0) a.out_planar3 = flow_mem + 5;
    else a.out_u8 = flow_mem + 6;
    a.out_fmt = kind == 2 ? kFmtF32 : kFmtU8;
    return a;
}
// the plan of (a, nt, flags) is conv3x3_flow<nt, ntw, ups, epi, defer, wres> with this ring, LDS and block size
static FlowPlan flow_expect(int line, const ConvArgs& a, int nt, int flags, int ntw, bool ups, int epi, bool defer, bool wres, int pr, int lds, int block)
{
    FlowPlan p{};
    const FlowChoice c = choose_conv_flow(a, nt, 256, flags, p);
    const bool ok = c == kFlowLaunch && p.nt == nt && p.ntw == ntw && p.ups == ups && p.epi == epi && p.defer == defer && p.wres == wres && p.pr == pr &&
                    p.lds == lds && p.block == block && p.grid == 256 && p.args.pr == (wres ? pr : -7) && flow_variant_exists(p.nt, p.ntw, p.ups, p.epi, p.defer, p.wres);
    if (!ok)
    {
        std::fprintf(stderr, "%s:%d: plan <%d,%d,%d,%d,%d,%d> ring %d lds %d block %d grid %d (choice %d)\n", __FILE__, line, p.nt, p.ntw, p.ups, p.epi, p.defer, p.wres, p.pr,
                     p.lds, p.block, p.grid, int(c));
        failures++;
    }
    return p;
}
#define FLOW(...) flow_expect(__LINE__, __VA_ARGS__)
static void flow_choice()
{
    FlowPlan p;
    // LDS bytes, written out: resident = ring * 20480 + planes * bytes per plane + nt * 128; streamed = FlowCfg<NT>::TOTAL
    const int kTotal1 = 150656, kTotal2 = 137472, kLast3 = 6 * 20480 + 4 * 3072 + 128;
    for (const int precise : {0, 1})
    {
        // conv_first: 3 channels in two planes; in precise mode its lo planes are kept and it starts the stream
        ConvArgs first = flow_conv(2, 0, 0, precise);
        first.out_lo_off = precise ? 8192 : 0;
        p = FLOW(first, 2, 0, 1, false, precise ? kEpiPrec : kEpiPlain, false, true, 6, 160000, 768);
        CHECK(p.args.res1.base == (precise ? first.out16.base : nullptr) && p.args.res1_kind == 0);
        FLOW(first, 2, kFlowNtw2, precise ? 1 : 2, false, precise ? kEpiPrec : kEpiPlain, false, true, 6, 160000, precise ? 768 : 512);
        FLOW(first, 2, kFlowStreamW, 1, false, precise ? kEpiPrec : kEpiPlain, false, false, 0, kTotal2, 768);
        // the dense convs of an RDB: x + k grown planes
        const int ring[4] = {6, 5, 4, 3}, lds[4] = {159872, 157824, 155776, 153728};
        for (int k = 0; k < 4; k++)
        {
            const ConvArgs dense = flow_conv(4, 2 * k, 1, precise);
            FLOW(dense, 1, 0, 1, false, kEpiPlain, true, true, ring[k], lds[k], 512);
            FLOW(dense, 1, kFlowNtw2, 1, false, kEpiPlain, true, true, ring[k], lds[k], 512);
            FLOW(dense, 1, kFlowInlineEpi, 1, false, kEpiPlain, false, true, ring[k], lds[k], 512);
            FLOW(dense, 1, kFlowStreamW, 1, false, kEpiPlain, true, false, 0, kTotal1, 512);
            FLOW(dense, 1, kFlowNtw2 | kFlowInlineEpi, 1, false, kEpiPlain, false, true, ring[k], lds[k], 512);
        }
        // conv5: 12 planes of 18 KiB do not fit, streamed whatever the flags say
        for (const bool second : {false, true})
        {
            const ConvArgs conv5 = flow_residual(8, true, second, precise);
            const int epi = precise ? (second ? kEpiPrec2 : kEpiPrec) : kEpiRes;
            p = FLOW(conv5, 2, 0, 1, false, epi, false, false, 0, kTotal2, 768);
            CHECK(p.args.res1.base == conv5.res1.base && p.args.res2_kind == (second ? 1 : 0) && p.args.lo1_off == conv5.lo1_off);
            FLOW(conv5, 2, kFlowNtw2, precise ? 1 : 2, false, epi, false, false, 0, kTotal2, precise ? 768 : 512);
            FLOW(conv5, 2, kFlowStreamW, 1, false, epi, false, false, 0, kTotal2, 768);
        }
        // trunk_conv: fea is not its own input and moves into the second residual's slot
        const ConvArgs trunk = flow_residual(0, false, false, precise);
        p = FLOW(trunk, 2, 0, 1, false, precise ? kEpiPrec2 : kEpiRes, false, true, 4, 155904, 768);
        CHECK(p.args.res2.base == trunk.res1.base && p.args.res2_kind == 1 && p.args.s2 == 1.f && p.args.lo2_off == trunk.lo1_off && p.args.lo1_off == 0 && p.args.res1_kind == 1);
        FLOW(trunk, 2, kFlowNtw2, precise ? 1 : 2, false, precise ? kEpiPrec2 : kEpiRes, false, true, 4, 155904, precise ? 768 : 512);
        FLOW(trunk, 2, kFlowStreamW, 1, false, precise ? kEpiPrec2 : kEpiRes, false, false, 0, kTotal2, 768);
        // upconv1 / upconv2 (nearest x2 in front) and HRconv: plain in either mode
        ConvArgs up = flow_conv(4, 0, 1, precise);
        up.lvl_out = 1;
        FLOW(up, 2, 0, 1, true, kEpiPlain, false, true, 4, 155904, 768);
        FLOW(up, 2, kFlowNtw2, 2, true, kEpiPlain, false, true, 4, 155904, 512);
        FLOW(up, 2, kFlowStreamW | kFlowInlineEpi, 1, true, kEpiPlain, false, false, 0, kTotal2, 768);
        ConvArgs hr = flow_conv(4, 0, 1, precise);
        hr.lvl_in = hr.lvl_out = 2;
        FLOW(hr, 2, 0, 1, false, kEpiPlain, false, true, 4, 155904, 768);
        FLOW(hr, 2, kFlowNtw2, 2, false, kEpiPlain, false, true, 4, 155904, 512);
        FLOW(hr, 2, kFlowStreamW, 1, false, kEpiPlain, false, false, 0, kTotal2, 768);
        // conv_last: the planar blob and the uint8 image run one kernel, a planar float image another
        const int last3[3] = {precise ? kEpiLast3F32 : kEpiLast3, precise ? kEpiLast3F32 : kEpiLast3, precise ? kEpiLast3ImgF32 : kEpiLast3Img};
        const int lastg[3] = {precise ? kEpiLastGF32 : kEpiLastG, precise ? kEpiLastGF32 : kEpiLastG, precise ? kEpiLastGImgF32 : kEpiLastGImg};
        for (int kind = 0; kind < 3; kind++)
        {
            ConvArgs last = flow_last(4, kind, precise);
            last.lvl_in = last.lvl_out = 2;
            for (const int flags : {0, int(kFlowStreamW), kFlowNtw2 | kFlowInlineEpi})
            {
                p = FLOW(last, 1, flags, 1, false, last3[kind], false, true, 6, kLast3, 512);
                CHECK(p.args.wpk16 == last.waux && p.args.wpieces == 3);
            }
            p = FLOW(last, 1, kFlowLastGeneric, 1, false, lastg[kind], false, true, 6, 159872, 512);
            CHECK(p.args.wpk16 == last.wpk16);
            FLOW(last, 1, kFlowLastGeneric | kFlowStreamW, 1, false, lastg[kind], false, false, 0, kTotal1, 512);
            last.waux = nullptr; // a model without the aux image
            FLOW(last, 1, 0, 1, false, lastg[kind], false, true, 6, 159872, 512);
            CHECK(choose_conv_flow(last, 2, 256, 0, p) == kFlowNotCovered); // 64 output channels and conv_last's epilogue
            CHECK(choose_conv_flow(flow_last(34, kind, precise), 1, 256, 0, p) == kFlowNotCovered); // (dy, cout): 34 planes leave 2 ring slots
            FLOW(flow_last(32, kind, precise), 1, 0, 1, false, last3[kind], false, true, 3, 3 * 20480 + 32 * 3072 + 128, 512);
        }
    }
    // rsr_conv3x3 / rsr_conv3x3_res (Engine::conv_test): 32 output channels with upsampling, with a residual, with few input planes
    ConvArgs t = flow_conv(4, 0, 1);
    t.lvl_out = 1;
    FLOW(t, 1, 0, 1, true, kEpiPlain, false, true, 6, 159872, 512);
    FLOW(flow_residual(0, true, false, 0), 1, 0, 1, false, kEpiRes, false, true, 6, 159872, 512);
    FLOW(flow_residual(0, true, true, 0), 1, kFlowNtw2, 1, false, kEpiRes, false, true, 6, 159872, 512);
    FLOW(flow_conv(2, 0, 1), 1, 0, 1, false, kEpiPlain, false, true, 6, 6 * 20480 + 2 * 9216 + 128, 512); // fewer than 4 planes never defer
    // the grid: whole groups of 8 workgroups, no more than the work items need
    t = flow_conv(4, 0, 1);
    t.nitems = 9;
    CHECK(choose_conv_flow(t, 1, 256, 0, p) == kFlowLaunch && p.grid == 16);
    CHECK(choose_conv_flow(t, 1, 13, 0, p) == kFlowLaunch && p.grid == 8);
    // nothing to launch
    t.nitems = 0;
    CHECK(choose_conv_flow(t, 1, 256, 0, p) == kFlowNothing);
    // not covered
    CHECK(choose_conv_flow(flow_conv(3, 0, 1), 1, 256, 0, p) == kFlowNotCovered);                     // an odd plane count
    CHECK(choose_conv_flow(flow_residual(0, false, true, 0), 2, 256, 0, p) == kFlowNotCovered);      // a fetched first residual and a second one
    CHECK(choose_conv_flow(flow_residual(0, true, false, 1), 1, 256, 0, p) == kFlowNotCovered);      // the precise forms have 64 output channels
    t = flow_residual(0, true, false, 0);
    t.lvl_out = 1;
    CHECK(choose_conv_flow(t, 2, 256, 0, p) == kFlowNotCovered);                                     // a residual behind the upsampling
    t = flow_conv(4, 0);
    t.wpk16 = nullptr;
    CHECK(choose_conv_flow(t, 1, 256, 0, p) == kFlowNotCovered);
    CHECK(choose_conv_flow(flow_conv(4, 0), 3, 256, 0, p) == kFlowNotCovered);
    // the description of the epilogues names each of them once
    for (int e = 0; e < kEpiCount; e++) CHECK(epi_of(epi_desc(e)) == e);
}

// WsLayout (workspace.h) against the sizes written out by hand; no overlap; the guard positions; PlanKey
static void workspace_layout()
{
    const int hi[6] = {2, 4, 12, 4, 4, 4}, lo[6] = {0, 2, 2, 0, 0, 0}, level[6] = {1, 1, 1, 4, 16, 16}; // in, fea, rdb, up1, up2, hr
    const int kind[kWsCount] = {0, 1, 2, 2, 2, 3, 4, 5, -1};                                               // of every buffer; -1: the planar output
    for (const long long cap : {1ll, 2080ll, 2704ll, 48400ll})
        for (const bool precise : {false, true})
        {
            const WsLayout L{cap, precise}, other{cap, !precise};
            for (const long long n : {1ll, 3ll, 16ll})
            {
                long long sum = 0, guards = 0;
                for (int b = 0; b < kWsCount; b++)
                {
                    const int k = kind[b], planes = k < 0 ? 0 : hi[k] + (precise ? lo[k] : 0);
                    const long long want = k < 0 ? n * cap * (precise ? 192 : 96) : n * planes * (cap * level[k] * 32 + 64);
                    CHECK(L.bytes(b, n) == want);
                    sum += L.bytes(b, n), guards += n * planes * 64;
                }
                CHECK(sum - guards == n * cap * (precise ? 6400 : 6048));
                CHECK(n * cap * WsLayout::bytes_per_px(precise) == sum - guards);
            }
            for (int b = 0; b < kWsCount; b++)
            {
                if (!WsLayout::guarded(b))
                {
                    CHECK(L.lo_off(b) == 0 && L.slot_stride(b) == cap * (precise ? 192 : 96));
                    continue;
                }
                const int k = kind[b];
                const long long pb = L.plane_bytes(b), px = cap * level[k] * 32;
                CHECK(pb == other.plane_bytes(b) && pb == px + kGuard); // the plane, hence the guards' spacing, does not depend on the mode
                CHECK((L.lo_off(b) != 0) == (precise && lo[k] != 0));
                // the pixel ranges [start, start + px) of every plane of three slots, as the kernels address them: hi plane p at plane_off(p),
                // lo pair plane q at plane_off(0) + lo_off + q * plane stride (conv_flow.hip lo_row), slot s at s * slot_stride
                std::vector<long long> starts;
                for (long long s = 0; s < 3; s++)
                {
                    for (int p = 0; p < hi[k]; p++) starts.push_back(s * L.slot_stride(b) + L.plane_off(b, p));
                    for (int q = 0; q < (precise ? lo[k] : 0); q++) starts.push_back(s * L.slot_stride(b) + L.plane_off(b, 0) + L.lo_off(b) + q * pb);
                }
                CHECK((long long)starts.size() == 3 * L.planes_per_slot(b));
                for (size_t i = 0; i < starts.size(); i++)
                {
                    // every plane starts a whole number of planes behind the buffer's start: its guard is one of those launch_zero_guards clears
                    CHECK((starts[i] - kGuard) % pb == 0 && starts[i] >= kGuard && starts[i] + px <= L.bytes(b, 3));
                    for (size_t j = 0; j < i; j++) CHECK(starts[i] - starts[j] >= pb || starts[j] - starts[i] >= pb); // a guard apart at least: no overlap
                }
            }
        }
    // PlanKey: equal to itself, unequal when any single field differs
    const PlanKey k0{70, 20, 3, 32, 10, 0, 1, false, OutRatio(), false, 0, 3, 65536, true, true, true, -1};
    PlanKey v[17];
    for (PlanKey& k : v) k = k0;
    v[0].w++, v[1].h++, v[2].c++, v[3].T++, v[4].P++, v[5].tta++, v[6].nimg++, v[7].precise = true, v[8].ratio = OutRatio(2, 1), v[9].ntw2 = true, v[10].tile0++, v[11].tile1++,
        v[12].budget_mb++, v[13].trim = false, v[14].xcd_order = false, v[15].fold = false, v[16].clamp = 0;
    CHECK(k0 == PlanKey(k0));
    for (const PlanKey& k : v) CHECK(!(k == k0) && !(k0 == k));
}

// fetch_chunks / fetch_chunk: the chunks tile the span exactly and in order, none larger than a staging slot, a rectangle's are whole rows
static void span_chunks(const FetchSpan& s, size_t rowbytes)
{
    const bool flat = s.width == rowbytes;
    size_t n = 0;
    for (const size_t slot : {s.width, s.width + 1, size_t(4096), size_t(1) << 20})
    {
        if (!flat && s.width > slot) continue; // (refused: below)
        CHECK(fetch_chunks(s, rowbytes, slot, n) == RSR_OK && n >= 1);
        size_t next = s.off;
        for (size_t i = 0; i < n; i++)
        {
            const FetchSpan ch = fetch_chunk(s, rowbytes, slot, i);
            CHECK(ch.off == next && ch.early == s.early && ch.width >= 1 && ch.rows >= 1 && ch.width * ch.rows <= slot);
            CHECK(flat ? ch.rows == 1 : ch.width == s.width);
            next += flat ? ch.width : ch.rows * rowbytes;
        }
        CHECK(next == s.off + (flat ? s.width * s.rows : s.rows * rowbytes));
    }
    if (!flat)
        for (const size_t slot : {s.width - 1, size_t(1)})
            CHECK(fetch_chunks(s, rowbytes, slot, n) == RSR_E_ARG && !std::strcmp(last_error(), "chunk_mb smaller than one output row"));
}

// fetch_plan: the spans of every tile range against the union of the range's output rectangles, written out from min(t * T, extent) and
// OutRatio::of_x / of_y alone; every byte exactly once, none outside (the maps have the exact size of the output: an overrun is ASan's)
static void fetch_plans()
{
    const int geo[][3] = {{70, 150, 32}, {45, 100, 32}, {33, 32, 32}, {32, 32, 32}, {96, 33, 32}};
    for (const auto& g : geo)
        for (const int c : {3, 4})
            for (const OutRatio os : {OutRatio(), OutRatio(2, 1), OutRatio(3, 2)})
            {
                const int w = g[0], h = g[1], T = g[2];
                if (out_admit(pix_fmt(RSR_FMT_U8_HWC), w, h, T, os, kWhoEngine) != RSR_OK) continue;
                const int xt = (w + T - 1) / T, yt = (h + T - 1) / T;
                const size_t rowbytes = size_t(os.of_x(w)) * c, orows = size_t(os.of_y(h));
                auto edge_x = [&](int t) { return size_t(os.of_x(std::min(t * T, w))) * c; };
                auto edge_y = [&](int t) { return size_t(os.of_y(std::min(t * T, h))); };
                for (int tile0 = 0; tile0 < xt * yt; tile0++)
                    for (int tile1 = tile0 + 1; tile1 <= xt * yt; tile1++)
                    {
                        std::vector<uint8_t> want(rowbytes * orows, 0);
                        for (int t = tile0; t < tile1; t++)
                            for (size_t y = edge_y(t / xt); y < edge_y(t / xt + 1); y++)
                                for (size_t x = edge_x(t % xt); x < edge_x(t % xt + 1); x++) want[y * rowbytes + x] = 1;
                        const int r0 = tile0 / xt, r1 = (tile1 - 1) / xt;
                        const bool whole = tile0 % xt == 0 && tile1 % xt == 0;
                        const size_t first_row = edge_y(r0), nrows = edge_y(r1 + 1) - first_row;
                        std::vector<size_t> halves = {0, nrows + 1}; // (rows of the range: what enqueue_images reports)
                        for (int tr = r0 + 1; tr <= r1; tr++) halves.push_back(edge_y(tr) - first_row);
                        for (const size_t half : halves)
                        {
                            const FetchPlan p = fetch_plan(w, h, c, T, os, tile0, tile1, half);
                            CHECK(p.n >= 1 && p.n <= (whole ? 2 : 3) && p.row0 == first_row && p.rows == nrows);
                            std::vector<uint8_t> got(rowbytes * orows, 0);
                            size_t bytes = 0;
                            for (int k = 0; k < p.n; k++)
                            {
                                const FetchSpan& s = p.span[k];
                                CHECK(s.width >= 1 && s.width <= rowbytes && s.rows >= 1 && s.off % rowbytes + s.width <= rowbytes);
                                CHECK(s.off >= p.row0 * rowbytes && s.off + (s.rows - 1) * rowbytes + s.width <= (p.row0 + p.rows) * rowbytes);
                                if (s.early) CHECK(whole && k == 0 && s.width == rowbytes && s.off == first_row * rowbytes && s.rows <= half);
                                for (size_t y = 0; y < s.rows; y++)
                                    for (size_t x = 0; x < s.width; x++) got[s.off + y * rowbytes + x]++;
                                bytes += s.width * s.rows;
                                span_chunks(s, rowbytes);
                            }
                            CHECK(got == want && bytes == p.bytes());
                            if (whole && half) CHECK(p.span[0].early && p.span[0].rows == std::min(half, nrows));
                        }
                    }
            }
}

int main()
{
    descriptors();
    admission();
    batches();
    flow_choice();
    workspace_layout();
    fetch_plans();
    if (failures) return std::fprintf(stderr, "%d check(s) failed\n", failures), 1;
    std::puts("descriptor_check ok");
    return 0;
}
