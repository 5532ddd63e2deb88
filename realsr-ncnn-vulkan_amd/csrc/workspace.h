// workspace.h -- THE description of the engine's device workspace (host only): which buffers a tile slot has, how many guarded 16-channel
// planes each holds at which resolution, and where the residue planes of precise mode sit.  Sizes, strides, the memory budget's bytes per
// pixel and the tile-size bound are read from the one table below; tools/host_check checks it against the formulas written out by hand.
#pragma once
#include "kernels.h"

namespace rsr {

// The buffers, in allocation order.  A slot of a guarded buffer is a run of planes [guard kGuard B | pixels x 32 B] (kernels.h "activation
// storage"); the three RDB buffers rotate through the dense blocks (Engine::run_network).
enum WsBuf { kWsIn, kWsFea, kWsRdb0, kWsRdb1, kWsRdb2, kWsUp1, kWsUp2, kWsHr, kWsOut3, kWsCount };
struct WsRow
{
    int level;     // pixels per padded LR pixel of the slot: 1, 4 (2x) or 16 (4x)
    int planes;    // guarded hi planes per slot; 0 = an unguarded flat buffer of `flat` bytes per pixel of its level
    int lo_planes; // precise mode: pair planes of one-byte rounding residue behind them (kernels.h ConvArgs::lo1_off), each with the geometry of a hi plane
    bool zero_all; // a change of layout zeroes the whole buffer, not only its guards
    int flat[2];   // planes == 0: bytes per pixel in fp16 storage / in precise mode
};
constexpr WsRow kWsRdbRow = {1, 12, 2, false, {}}; // x (4 planes) + the dense x1..x4 (4 x 2); the lo pair planes of x
constexpr WsRow kWsTable[kWsCount] = {
    {1, 2, 0, true, {}},        // IN: the 3-channel input padded to 32 channels; channels 3.. are never written and must stay zero (stat "ws_guard_dirty")
    {1, 4, 2, false, {}},       // FEA: conv_first's result, the global skip; the residual stream of precise mode starts here
    kWsRdbRow, kWsRdbRow, kWsRdbRow,
    {4, 4, 0, false, {}},       // UP1 @2x
    {16, 4, 0, false, {}},      // UP2 @4x
    {16, 4, 0, false, {}},      // HR @4x
    {16, 0, 0, false, {6, 12}}, // OUT3: conv_last's planar [3][4H][4W] blob, fp16 or -- precise -- fp32 (where it does not write the image itself)
};

// The layout of the workspace for slots of cap_px padded LR pixels.  All sizes in bytes.
struct WsLayout
{
    long long cap_px = 0;
    bool precise = false;
    static constexpr long long kPxBytes = kPlaneCh * 2; // of one pixel of one plane
    static constexpr bool guarded(int buf) { return kWsTable[buf].planes != 0; }
    static constexpr long long guarded_plane(long long px) { return px * kPxBytes + kGuard; } // guard + px pixels
    static constexpr long long lo_behind(int hi_planes, long long plane_stride) { return hi_planes * plane_stride; } // a tensor's lo pair planes follow its hi planes at their stride
    // One plane of a guarded buffer.  It depends on the slot capacity alone, and every plane of the buffer -- lo pair planes included --
    // starts a whole number of them behind the buffer's start: no guard moves when `precise` changes.
    constexpr long long plane_bytes(int buf) const { return guarded_plane(cap_px * kWsTable[buf].level); }
    constexpr int planes_per_slot(int buf) const { return kWsTable[buf].planes + (precise ? kWsTable[buf].lo_planes : 0); }
    constexpr long long slot_stride(int buf) const { return guarded(buf) ? planes_per_slot(buf) * plane_bytes(buf) : cap_px * kWsTable[buf].level * kWsTable[buf].flat[precise]; }
    constexpr long long bytes(int buf, long long nslots) const { return nslots * slot_stride(buf); }
    constexpr long long plane_off(int buf, int plane) const { return plane * plane_bytes(buf) + kGuard; } // pixel 0 of hi plane `plane` of slot 0, from the buffer's start
    // the lo pair planes of the buffer's tensor, from pixel 0 of its plane 0 (ConvArgs::lo1_off / out_lo_off); 0 = there are none
    constexpr long long lo_off(int buf) const { return precise && kWsTable[buf].lo_planes ? lo_behind(kWsTable[buf].planes, plane_bytes(buf)) : 0; }
    static constexpr long long bytes_per_px(bool precise) // workspace bytes per padded LR pixel of a slot, guards aside: what the memory budget counts
    {
        long long n = 0;
        for (int b = 0; b < kWsCount; b++) n += WsLayout{1, precise}.slot_stride(b) - (guarded(b) ? WsLayout{1, precise}.planes_per_slot(b) * kGuard : 0);
        return n;
    }
    static constexpr long long max_plane_px_bytes() // pixel bytes of the largest plane per padded LR pixel (Engine::check_tile_px)
    {
        long long n = 0;
        for (const WsRow& r : kWsTable) n = r.planes && r.level * kPxBytes > n ? r.level * kPxBytes : n;
        return n;
    }
};
static_assert(WsLayout::bytes_per_px(false) == 6048 && WsLayout::bytes_per_px(true) == 6400, "DESIGN.md 2, tests/test_gpu_exact_geometry.py BYTES_PER_PX and the budgets of several tests state these figures");
static_assert(WsLayout::max_plane_px_bytes() == 16 * 32, "Engine::check_tile_px bounds a 4x plane of 32 B per pixel");

} // namespace rsr
