// engine.h -- the tiled super-resolution engine behind the C-ABI (include/realsr_hip.h).
//
// Replaces RealSR::process (/root/reference/src/realsr.cpp:145-523): instead of a row-band loop with
// one Vulkan submit_and_wait per tile and >= 722 dispatches per tile, ALL tiles of an image (x8 under
// TTA) are laid out as "slots" of one batch and walk the model's convolutions (351 at 23 RRDB blocks) together: one kernel launch
// per network layer per batch, no host synchronisation inside a call (the one exception is opt-in: option "alpha_adaptive" waits once
// per tile batch for the bytes of its scan).
//
// Concurrency (the reference calls RealSR::process from several proc threads on one object, main.cpp:811-828,
// with per-call allocators, realsr.cpp:161-167):
//   * every rsr_process call owns a LANE for its duration: private device image buffers, private pinned staging,
//     a private copy stream and events -- nothing of a call's data path is shared with another call;
//   * the network itself runs on ONE compute stream over ONE workspace; calls enqueue their kernels under `mu`
//     (a few hundred microseconds of host time) and the GPU executes them in that order.  A lane's upload runs
//     ahead of, and its download behind, the other lanes' kernels: H2D(k+1) | kernels(k) | D2H(k-1) overlap;
//   * SMALL images of concurrent calls are MERGED: a 256 x 256 image is 200 blocks for 256 CUs -- every one of the 352
//     launches costs its fixed ~14 us whatever it carries -- so calls whose image is small (any small size; same channel
//     count) are combined into ONE tile batch (up to kMaxMerge images, Engine::submit_merged): the caller that finds no leader
//     becomes one, waits until the previous merged batch is half way through the network (while it waits, further calls
//     queue up; its own launches are then enqueued underneath the second half), takes the queued calls of its
//     geometry and enqueues them as one batch; the others sleep until
//     their batch is enqueued and then fetch their own output.  The reference runs such calls side by side on the
//     device ("-j 4:4:4 for many small images", README.md:61, main.cpp:811-828); here they share the launches.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <list>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/realsr_hip.h"
#include "kernels.h"
#include "model.h"
#include "workspace.h"

namespace rsr {

// The size of the output relative to the input, per axis: nx / dx along x and ny / dy along y, each in lowest terms
// (include/realsr_hip.h rsr_set_out_ratio, rsr_set_out_ratio_xy).  4 / 1, 2 / 1 and 1 / 1 on BOTH axes are option "out_scale" 4 / 2 / 1
// and take its kernels; every other permitted pair is area-averaged by postproc_tiles_area.
struct OutRatio
{
    int nx = 4, dx = 1, ny = 4, dy = 1;
    OutRatio() = default;
    OutRatio(int n, int d) : nx(n), dx(d), ny(n), dy(d) {} // one ratio on both axes
    OutRatio(int nx0, int dx0, int ny0, int dy0) : nx(nx0), dx(dx0), ny(ny0), dy(dy0) {}
    bool operator==(const OutRatio& o) const { return nx == o.nx && dx == o.dx && ny == o.ny && dy == o.dy; }
    bool operator!=(const OutRatio& o) const { return !(*this == o); }
    bool same() const { return nx == ny && dx == dy; }                      // one ratio on both axes (what stats "out_num" / "out_den" can read)
    bool is_box() const { return same() && dx == 1 && (nx == 4 || nx == 2 || nx == 1); }
    int out_scale() const { return is_box() ? nx : 0; }                     // what stat "out_scale" reads
    long long of_x(long long x) const { return x * nx / dx; }               // an input length in output pixels (exact where the call was admitted)
    long long of_y(long long y) const { return y * ny / dy; }
    bool divides_x(long long x) const { return x * nx % dx == 0; }
    bool divides_y(long long y) const { return y * ny % dy == 0; }
    std::string str() const { return same() ? std::to_string(nx) + "/" + std::to_string(dx) : std::to_string(nx) + "/" + std::to_string(dx) + " x " + std::to_string(ny) + "/" + std::to_string(dy); }
};
// Host-only: num / den reduced to lowest terms on both axes when it is one of the permitted ratios of rsr_set_out_ratio (d in 1..4,
// 1 <= n / d <= 4), else false.
bool out_ratio_reduce(int num, int den, OutRatio* out);
// Host-only: the pair reduced per axis when each axis is one of the permitted ratios of rsr_set_out_ratio_xy (d in 1..8, 1 <= n / d <= 4).
bool out_ratio_reduce_xy(int num_x, int den_x, int num_y, int den_y, OutRatio* out);
// Host-only, the rules of a pixel format (kernels.h PixFmt), each RSR_OK or RSR_E_ARG through Engine::fail.
// fmt_check: is it a format at all ("unknown pixel format"), and does it come with c channels (c_text)?
int fmt_check(const PixFmt& f, int c, const char* c_text = "no such pixel format / channel count");
// parity_check: w (h) of a surface is even on every axis its chroma is subsampled on; `noun`: what the message calls the image.
int parity_check(const PixFmt& f, int w, int h, const char* noun);
// out_admit, THE output admission rule: may a w x h image at tile size T leave in format f at ratio r?  The ratio rule: w and T times
// nx / dx, h and T times ny / dy are whole -- an output pixel is a whole number of them only where the image's sides times n are multiples
// of d, and only where the tile size times n is one too does every tile's rectangle start on a whole output pixel, so that no averaging
// footprint crosses a tile (postproc_tiles_area is a per-tile launch); always true at 4, 2 and 1.  On every axis the format's chroma is
// subsampled on, the parity rule on top: those quotients are even -- a YUV output is written one 2 x 2 luma quad (4:2:0) or one 2 x 1 pair
// (4:2:2: the columns alone answer to it) per thread, tile by tile, so the image and every tile's rectangle start and end on even output
// pixels; at out_scale 4 / 2 / 1 that reads w * os, h * os and T * os even.  `who` words the refusal as its caller always has.
enum OutWho { kWhoOutSize, kWhoOutSizeXY, kWhoEngine }; // rsr_out_size / _yuv; the _xy and _fmt size functions; the engine (adds "(w x h at tile T)")
int out_admit(const PixFmt& f, int w, int h, int T, OutRatio r, OutWho who);

struct DevBuf
{
    void* p = nullptr;
    size_t bytes = 0;
};

// A device buffer that lives as long as its scope (the scratch tables and tiles of the test hooks); filled by Engine::ensure.
struct ScratchBuf : DevBuf
{
    ScratchBuf() = default;
    ScratchBuf(const ScratchBuf&) = delete;
    ScratchBuf& operator=(const ScratchBuf&) = delete;
    ~ScratchBuf()
    {
        if (p) (void)hipFree(p);
    }
};

// What a cached plan was built for: the call's arguments and the engine state its tables and batch sizes depend on (Engine::get_plan)
struct PlanKey
{
    int w = 0, h = 0, c = 0, T = 0, P = 0, tta = 0;
    int nimg = 1;         // images of this geometry merged into one tile batch (kernels.h kMaxMerge); their tiles follow each other image by image
    bool precise = false; // Engine::precise (the slots are larger)
    OutRatio ratio;       // Engine::out_ratio (though no field of a Plan depends on it today: the placement tables are built alike and below 4 merely go unused)
    bool ntw2 = false;    // flow_flags has kFlowNtw2 (an MFMA wave then reaches 4 planes from one base: the tile-size bound halves)
    int tile0 = 0, tile1 = 0; // tiles [tile0, tile1) of the image's tile grid, row-major (multi-GPU tile sharding)
    long long budget_mb = 0;
    bool trim = true, xcd_order = true, fold = true;
    long long clamp = -1; // Engine::ws_clamp_bytes
    bool operator==(const PlanKey& o) const
    {
        return w == o.w && h == o.h && c == o.c && T == o.T && P == o.P && tta == o.tta && nimg == o.nimg && precise == o.precise && ratio == o.ratio && ntw2 == o.ntw2 &&
               tile0 == o.tile0 && tile1 == o.tile1 && budget_mb == o.budget_mb && trim == o.trim && xcd_order == o.xcd_order && fold == o.fold && clamp == o.clamp;
    }
};

// geometry of one rsr_process call; cached per PlanKey
struct Plan
{
    PlanKey key;
    int out_row0 = 0; // output rows are addressed relative to this one: the first row of the tile range (the device buffer of a range holds only its rows)
    long long cap_px = 0; // slot capacity in LR pixels
    int max_tw = 0, max_th = 0;
    struct Batch
    {
        int tile0 = 0, ntiles = 0, nslots = 0;
        std::vector<BaseTile> tiles; // slot0 relative to the batch
        std::vector<TileDim> dims;   // per slot
        std::vector<WorkItem> items[3];
        std::vector<int> item_start[3]; // first item of every slot (+ end): items are sorted by slot
        double px[3] = {0, 0, 0}; // sum over slots of H*W at each level (for FLOP accounting)
        int trim4 = 0;            // prepadding * scale when the tables were trimmed to the kept rectangle (make_items), else 0
        // device copies
        BaseTile* d_tiles = nullptr;
        TileDim* d_dims = nullptr;
        WorkItem* d_items[3] = {nullptr, nullptr, nullptr};
        WorkItem* d_items_rev[3] = {nullptr, nullptr, nullptr}; // the same blocks in reverse order (see run_network)
    };
    std::vector<Batch> batches;
    int slots_per_batch = 0;
    void* d_tables = nullptr; // one allocation backing all device tables
};

// Device tables of the range probe (Engine::selfcheck): entry i receives what convolution i of x4.param stored.
struct RangeProbe
{
    unsigned* peak_bits = nullptr;           // bits of the largest finite |value| as a float [Engine::nconv]
    unsigned long long* nonfinite = nullptr; // stored inf / NaN [Engine::nconv]
};

// Helper threads for the staging copies of pageable images (pinned chunk <-> the caller's malloc'ed buffer): one core
// moves ~10 GB/s, a 100 MB output would cost as much as a tenth of the network.  Started on first use.
struct CopyPool
{
    struct Job
    {
        char* dst;
        const char* src;
        size_t n;
        int* pending; // under m
    };
    std::mutex m;
    std::condition_variable cv, done;
    std::deque<Job> q;
    std::vector<std::thread> workers;
    bool stop = false;
    ~CopyPool();
    void copy(void* dst, const void* src, size_t n, int threads); // returns when all of [dst, dst+n) is written
};

// one image waiting to be merged into a tile batch (Engine::submit_merged); lives on its caller's stack
struct MergeReq
{
    const void* d_in = nullptr;
    void* d_out = nullptr;
    int w = 0, h = 0, c = 0, T = 0;
    OutRatio os;                  // Engine::out_ratio when the call came in: d_out is os.of_x(w) x os.of_y(h)
    long long items = 0;          // LR-level work items of the image (Engine::image_items)
    int width = 1;                // Engine::merge_width of its geometry when the call came in
    hipEvent_t ev_in = nullptr;   // the input is complete behind this event (null: it already is)
    hipEvent_t ev_done = nullptr; // recorded on the compute stream behind the batch (null: the leader takes one from the pool -> ev_done_pool)
    bool pool_event = false;      // ev_done came from Engine::take_event: the caller gives it back
    int rc = RSR_OK;
    std::string err;
    bool done = false, lead = false; // under Engine::cq_mu
};

// One device image as a call addresses it: its base and the bytes from one row / one plane to the next, resolved (0 = "tightly packed"
// has been replaced by the packed value; plane stays 0 for uint8 HWC behind a descriptor, which has no planes).
struct ImageRef
{
    const void* data = nullptr;
    long long row = 0, plane = 0;
};

// Three rotating device buffers for tile tables that are built per call (Engine::enqueue_mixed, Engine::enqueue_sequence), each guarded by
// an event recorded behind the last launch that reads it: the host waits only when the call three turns back is still in flight.  With
// want_stage a slot has a pinned host image of the same size, from which the tables travel in one asynchronous copy.  Engine::mu held.
struct TableRing
{
    DevBuf tab[3];
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    void* stage[3] = {nullptr, nullptr, nullptr};
    size_t stage_bytes[3] = {0, 0, 0};
    unsigned long long seq = 0;
    int k = 0;                                   // the slot in use
    int acquire(size_t bytes, bool want_stage);  // the next slot: waits for its event, grows its buffer(s) to `bytes`; RSR_*
    char* dev() const { return static_cast<char*>(tab[k].p); }
    char* host() const { return static_cast<char*>(stage[k]); }
    void release(hipStream_t st);                // records the slot's event behind what `st` holds (no event to be had: waits for `st`)
    void free();
};

// What one tile batch is told about its caller (Engine::launch_batch, Engine::run_network): the images its tiles come from and go
// to, and the events the caller wants recorded on the way.
struct BatchIO
{
    int nimg = 0, c = 0;        // images of the batch (<= kMaxMerge; BaseTile::img selects) and their channel count
    const void* in[kMaxMerge];  // per image: the device image, in_fmt, w[i] x h[i] ...
    void* out[kMaxMerge];       // ... and its os.of_x(w[i]) x os.of_y(h[i]) result, out_fmt
    OutRatio os;                // Engine::out_ratio of the call: 4, or 2 / 1 = the x4 result box-reduced (kernels.h PostArgs::box = 4 / os), or another ratio or pair = area-averaged (PostArgs::num / den per axis)
    int w[kMaxMerge], h[kMaxMerge];
    // Bytes from one row / one plane (planar formats) of an image to the next, resolved (never 0; rsr_image of the C ABI, image_layout).
    // set() takes them from two ImageRefs (what image_refs made of the caller's descriptors), or packs them tightly itself.
    long long in_pitch[kMaxMerge], in_plane[kMaxMerge], out_pitch[kMaxMerge], out_plane[kMaxMerge];
    int in_fmt = RSR_FMT_U8_HWC, out_fmt = RSR_FMT_U8_HWC; // RSR_FMT_* (the planar float and the YUV formats come with whole images of c == 3 only;
                                                           // YUV: the plane pitch is the distance from Y(0,0) to the UV plane)
    int out_row0 = 0;           // `out` points at output row os.of_y(out_row0) / 4 of the image; out_row0 counts x4 rows (a tile range's device buffer holds only its rows)
    int split_slot = 0;         // > 0: the 4x tail is split in front of this slot and ...
    hipEvent_t ev_half = nullptr; // ... this event recorded behind the first part (the caller starts downloading its output rows)
    hipEvent_t ev_mid = nullptr;  // recorded behind the middle RDB (a merged batch's throttle event, Engine::submit_merged)
    BatchIO(const void* d_in, void* d_out, int w0, int h0, int c0, int in_fmt0, int out_fmt0, OutRatio os0) : nimg(1), c(c0), os(os0), in_fmt(in_fmt0), out_fmt(out_fmt0)
    {
        set(0, d_in, d_out, w0, h0);
    }
    BatchIO(MergeReq* const* g, int n) : nimg(n), c(g[0]->c), os(g[0]->os) // the uint8 images of merged calls (one out_scale: Engine::run_group)
    {
        for (int i = 0; i < n; i++) set(i, g[i]->d_in, g[i]->d_out, g[i]->w, g[i]->h);
    }
    BatchIO(int n, int c0, int in_fmt0, int out_fmt0, OutRatio os0) : nimg(n), c(c0), os(os0), in_fmt(in_fmt0), out_fmt(out_fmt0) {} // the caller calls set() n times
    static double image_px_bytes(int fmt, int c) // bytes of one PIXEL of a whole image: c for uint8 HWC, 3 halfs / floats, 1.5 samples of a 4:2:0 surface, 2 of a 4:2:2, 3 of a 4:4:4 one
    {
        const PixFmt f = pix_fmt(fmt, c);
        return double(f.rows(2) * f.es) / 2; // (two rows: the smallest height every format takes)
    }
    static ImageRef packed(const void* data, int fmt, long long wi, long long hi, int c) // a tightly packed wi x hi image
    {
        const long long row = wi * pix_fmt(fmt, c).es; // (a UV row has as many bytes as a Y row)
        return ImageRef{data, row, hi * row};
    }
    void set(int i, const ImageRef& src, const ImageRef& dst, int wi, int hi) // image i: wi x hi behind src, its x os result behind dst
    {
        in[i] = src.data, out[i] = const_cast<void*>(dst.data), w[i] = wi, h[i] = hi;
        in_pitch[i] = src.row, in_plane[i] = src.plane, out_pitch[i] = dst.row, out_plane[i] = dst.plane;
    }
    void set(int i, const void* d_in, void* d_out, int wi, int hi) // ... both tightly packed
    {
        set(i, packed(d_in, in_fmt, wi, hi, c), packed(d_out, out_fmt, os.of_x(wi), os.of_y(hi), c), wi, hi);
    }
};

// one in-flight rsr_process call (host API)
struct Lane
{
    hipStream_t copy = nullptr;
    hipEvent_t ev_in = nullptr, ev_done = nullptr, ev_half = nullptr, ev_chunk[2] = {nullptr, nullptr};
    std::array<hipEvent_t*, 5> events() { return {&ev_in, &ev_done, &ev_half, &ev_chunk[0], &ev_chunk[1]}; } // THE list: open() creates them, ~Engine destroys them
    int open(); // the copy stream and the events, on the lane's first use
    DevBuf d_in, d_out;
    std::atomic<size_t> in_bytes{0}, out_bytes{0}; // sizes of d_in / d_out for readers that do not own the lane (device_avail, rsr_get_stat)
    void* h_in = nullptr;
    size_t h_in_bytes = 0;
    void* h_out = nullptr; // two download chunks
    size_t h_out_bytes = 0;
    bool busy = false;
};
struct LaneHold; // engine.cpp: a lane for the duration of one host call

// What a host call downloads (engine.cpp fetch_plan; Engine::lane_fetch): spans of the full-size, tightly packed output image.  A span is
// `rows` pieces of `width` bytes, one per output row from byte `off` on; width == the bytes of a row: ONE contiguous byte range.
struct FetchSpan
{
    size_t off, width, rows;
    bool early; // complete at the lane's ev_half already (the first part of a split 4x tail); else at ev_done
};
struct FetchPlan
{
    size_t row0, rows; // the output rows the spans lie in: what the lane's d_out holds (a member of a group allocates the rows of its range, not the frame)
    int n;
    FetchSpan span[3];
    size_t bytes() const
    {
        size_t b = 0;
        for (int i = 0; i < n; i++) b += span[i].width * span[i].rows;
        return b;
    }
};

struct Engine
{
    int device = -1;
    int tta = 0;
    int scale = 4, tilesize = 200, prepadding = 10;
    bool loaded = false;
    bool bgr = false; // pixel order of the caller's images: BGR(A) like the reference's Windows/WIC path (realsr.cpp:188-206,497-515)
    // Precise residual stream (option "precise"; kernels.h ConvArgs::precise): the 64-channel trunk is kept as an fp16 plane + a byte of rounding residue and
    // conv_last's fp32 result goes to the uint8 conversion unrounded.  Default off = the storage of the reference's Vulkan path
    // (fp16 everywhere, realsr.cpp:44-46); on = half the distance to its fp32 CPU path (realsr.cpp:525-838), the bar of the parity tests.
    bool precise = false;
    // Output scale (option "out_scale"; include/realsr_hip.h): 4 = the network's x4 image; 2 / 1 = every 2 x 2 / 4 x 4 box of it, clamped to
    // [0, 1] first, leaves as its fp32 mean.  A box never crosses a tile (a tile's x4 rectangle starts and ends on multiples of 4), so the
    // reduction is the per-tile post-processing launch (kernels.hip postproc_tiles_box); conv_last then leaves the planar blob.
    // out_ratio generalises it (rsr_set_out_ratio): n / d with d in 1..4 and 1 <= n / d <= 4.  For a scale that is not 4, 2 or 1 the footprint of
    // an output pixel is up to 4 x 4 x4 pixels with integer weights; whenever tilesize * n is a multiple of d a tile's rectangle starts on a
    // whole output pixel, no footprint crosses a tile, and the reduction is still ONE per-tile launch (postproc_tiles_area).
    // rsr_set_out_ratio_xy gives each axis a ratio of its own (d in 1..8: up to 5 taps per axis); the rule above then holds per axis.
    OutRatio out_ratio;
    // YUV <-> RGB of the NV12 / P010 device formats (options "yuv_matrix", "yuv_range"; include/realsr_hip.h): Kr / Kb of BT.709, 601 or
    // 2020, limited (0) or full (1) range.  Read when a call is enqueued: the constants travel with the launch (kernels.h YuvCoef).
    int yuv_matrix = 709, yuv_range = 0;
    // Chroma siting of those surfaces (option "yuv_siting"; include/realsr_hip.h "Chroma siting"), on both sides of a call: 0 = centre of the
    // 2 x 2 luma quad (JPEG, MPEG-1), 1 = left (H.264 / HEVC / AV1 / MPEG-2 default), 2 = top-left (BT.2020 / UHD HEVC).  Read when a call is
    // enqueued, like the matrix; 1 and 2 launch kernels of their own (kernels.h PreArgs::siting / PostArgs::siting).
    int yuv_siting = 0;
    // Alpha through the network (option "alpha_net"; include/realsr_hip.h "alpha_net"): an RGBA batch (c == 4) walks the network twice, once
    // for the colour as ever and once for the gray image of its alpha samples, whose channel mean becomes sample 3 (launch_batch).  Read
    // when a batch is enqueued, like bgr.  Both passes share the tables, the plan and the workspace: the stream orders them.
    bool alpha_net = false;
    long long alpha_tiles = 0; // stat: tiles that ran the alpha pass since creation, under mu
    // Option "alpha_adaptive" (include/realsr_hip.h "alpha_adaptive"): under alpha_net, the alpha pass runs only on the tiles whose source
    // rectangle holds more than one alpha value.  A scan in front of the colour pass (kernels.h FlatArgs) leaves one byte per tile, the host
    // reads them while the colour pass runs -- ONE host wait per tile batch -- and launch_batch picks the alpha pass: none, the batch's own
    // tables, or a sub-batch of the varying tiles built on the fly.  Read when a batch is enqueued, like alpha_net.
    bool alpha_adaptive = false;
    long long alpha_tiles_flat = 0; // stat: tiles whose alpha pass was skipped since creation, under mu
    double alpha_wait_us = 0;       // stat: host time spent waiting for the scans' bytes
    TableRing flat_ring;            // the scan's bytes: device and pinned, rotating like the tables
    TableRing alpha_ring;           // the tables of the sub-batches (pinned image, one asynchronous copy on the call's stream)
    // The scan of the first ntiles tiles of b on st, its bytes on their way to flat_ring.host(), the ring's event recorded behind them
    int enqueue_flat_scan(const Plan::Batch& b, int max_th, int ntiles, hipStream_t st, const BatchIO& io);
    // Option "dither" (include/realsr_hip.h "dither"): the colour samples of every integer output format are rounded against a threshold
    // keyed to the sample's position in the output image instead of 0.5 (kernels.h PostArgs::dither).  Read when a batch is enqueued, like
    // alpha_adaptive.  The rounding lives in the post launch alone, so while it is on conv_last never writes the image itself
    // (conv_last_writes_image): a uint8 RGB call without TTA takes the planar blob and one postproc_tiles launch, the route uint16, RGBA, TTA
    // and YUV calls take anyway, and the split tail of the host calls' early download, which hangs on the fused store, is off as for uint16.
    // No table of a plan depends on the route (the placement fields of the 4x work items are made for every non-TTA plan and merely go
    // unread), so one cached plan serves a context that alternates between the two settings.
    bool dither = false;
    // Model self-check (include/realsr_hip.h rsr_selfcheck): one tile through the network in both storages, compared on the device.
    bool precise_auto = false;    // option "precise_auto": `precise` follows the self-check's recommendation (now when loaded, else at the next load)
    long long selfcheck_runs = 0;
    rsr_selfcheck_report sc_last{}; // of the last run
    bool sc_have = false;           // sc_last / sc_peak / sc_nonfinite describe the loaded model (a load drops them)
    bool precise_by_auto = false;   // `precise` is on because a self-check of the loaded model recommended it (a load drops that too)
    std::vector<float> sc_peak;     // [nconv], resized and zeroed on every load (adopt_model)
    std::vector<long long> sc_nonfinite;
    int selfcheck(const uint16_t* tile, int w, int h, rsr_selfcheck_report* out); // mu held
    int apply_precise_auto();                                                      // mu held, loaded: self-check on the built-in tile -> precise
    long long bytes_per_px() const { return WsLayout::bytes_per_px(precise); } // workspace bytes per padded LR pixel of a slot
    int flow_flags = 0; // kFlow* bits of kernels.h
    int num_cu = 256;
    int dbg = 0; // ConvArgs::dbg ablation bits (profiling only)
    bool trim_tail = true; // leave out the blocks / rows behind the trunk that only feed cropped output pixels (engine.cpp: tail_margin)
    bool xcd_order = true; // backward work-item tables reversed per XCD share (each XCD re-reads what IT wrote last: L2 hits), else as a whole
    bool fold_cols = true; // a tile's last column of <= 14 pixels as folded work items (kernels.h: kFoldBit); off = one plain block column more
    bool alternate_order = true; // odd convs walk the work items backwards: they start on the data the previous conv touched last
    int test_repeat = 1;        // conv_test: work items repeated N times in one launch (measurement aid)
    double last_test_us = 0.0;  // HIP-event time of the last conv_test launch
    int trace_conv = -1; // conv index whose launch records s_memtime stamps into trace_buf (profiling only)
    DevBuf trace_buf;
    long long max_workspace_mb = 65536;
    long long ws_clamp_bytes = -1; // set after a workspace allocation failed: the next plans stay below it (-1 = none); dropped
                                   // again when the device can give twice that much (get_plan)
    long long clamp_fail_avail = -1; // device_avail() at the moment of the last failed workspace allocation (-1: the clamp was planted by the test hook)
    long long clamp_saved = -1;      // the clamp an un-clamp attempt set aside (restored when the attempt fails)
    int clamp_backoff = 4;           // calls between two un-clamp attempts while the device does not report clearly more room; doubles per failed attempt
    int clamp_calls_left = 0;
    long long ws_fail_above_bytes = -1; // test hook: workspaces above this size fail with RSR_E_NOMEM (a persistently fragmented device)
    long long ws_failures = 0;          // ... how often it fired (stat "ws_failures")
    // Test hooks of the workspace's contents (include/realsr_hip.h "ws_poison"; tests/test_gpu_ws_hygiene.py).  ws_poison: 0 = off, else bit 16 +
    // a 16-bit pattern that every ensure_workspace writes over every byte of every buffer before it zeroes what a change of slot capacity zeroes.
    int ws_poison = 0;
    long long ws_guard_dirty(); // stat: non-zero bytes in the guards of the current layout and in IN's channels 3 .. 31; -1 without a layout.  mu held
    // conv_test inside red zones of this many bytes (option "test_redzone", 0 = off) ...
    long long test_redzone = 0;
    long long test_redzone_dirty = -1; // ... and how many of their bytes the last launch changed (stat; -1: the last conv_test had none)
    int tail_group_slots = 0; // slots per launch group of the 2x / 4x convs (0 = the whole batch at once), see run_network
    int max_lanes = 16; // (small images are merged across calls: the more callers in flight, the fuller the launches)
    size_t chunk_bytes = size_t(16) << 20; // download chunk for pageable destinations
    int copy_threads = 4;                  // CPU threads per staging copy (1 = the calling thread alone)
    CopyPool pool;
    hipStream_t stream = nullptr;          // the compute stream

    // model: depth of the loaded RRDBNet (0 before a load) -- nb RRDB blocks, nrdb = 3 nb dense blocks, nconv = 15 nb + 6 convolutions
    int nb = 0, nrdb = 0, nconv = 0;
    std::vector<PackedConv> convs;
    DevBuf blob; // packed weights on device: THE blob the kernels read (run_network)
    DevBuf zeros;
    std::vector<unsigned char> model_head; // header + table of `blob` as it was validated (adopt_model): what a second model's table is compared with
    // Network interpolation (include/realsr_hip.h "network interpolation"; rsr_load_second, rsr_set_blend).  Without a second model the
    // context holds `blob` alone, as ever.  With one it holds three blobs of one table: blob_a (the first model: the allocation that was
    // `blob`), blob_b (the second) and `blob`, the ACTIVE one, = (1 - blend_t) * A + blend_t * B as launch_blend_blob wrote it over the
    // chunks of blend_tab (a copy of A at 0, of B at 1).  A load of a new first model drops all of it (drop_second).
    bool second = false;
    float blend_t = 0.f;
    DevBuf blob_a, blob_b, blend_tab; // blend_tab: BlendChunk[blend_chunks], built once per second model's first load (the table is A's)
    int blend_chunks = 0;
    double last_blend_us = -1.0; // stat "blend_us": HIP-event time of the last blend launch or copy, taken under rsr_set_profiling only (-1: not taken)
    int load_second_files(const char* param, const char* bin);
    int load_second_blob(const void* data, size_t bytes, bool is_device);
    int set_blend(float t);                                  // mu held; returns when the active blob is complete
    int apply_blend();                                       // active <- blend_t of A and B on the compute stream, waited for; then drop_model_state
    int export_model(void* dst, size_t cap, size_t* need);   // the active blob -> host
    void drop_second();                                      // back to one blob (the active one stays `blob`); blend_t = 0
    void drop_model_state();                                 // what described the model whose weights just changed: see adopt_model

    // workspace (workspace.h: one allocation per buffer), laid out for slots of ws_cap_px pixels (0: no layout)
    long long ws_cap_px = 0;
    DevBuf ws[kWsCount];

    // plans, most recently used first
    std::list<Plan> plans;

    // lanes
    std::mutex lane_mu;
    std::condition_variable lane_cv;
    std::vector<std::unique_ptr<Lane>> lanes;

    // merging small images across calls (see the top of this file)
    std::atomic<int> merge_max{kMaxMerge};      // option "merge": images per merged batch at most (1 = off)
    std::atomic<int> merge_target_items{4096};  // LR-level work items a merged batch aims at (16 per CU); an image with more than a quarter of it is not merged
    std::mutex cq_mu;
    std::condition_variable cq_cv;
    std::deque<MergeReq*> cq;        // FIFO of waiting calls, under cq_mu
    bool cq_leader = false;          // some caller is forming / enqueuing a batch
    hipEvent_t merge_mid = nullptr;  // recorded half way through the network of the last merged batch (the throttle of the next leader)
    bool merge_mid_used = false;
    hipEvent_t merge_done = nullptr; // ... and behind it
    int merge_last_n = 0;            // images in that batch
    std::atomic<long long> merged_batches{0}, merged_images{0}, merged_widest{0}; // stats
    std::atomic<int> merge_inbound{0}; // calls with a small image that are on their way to submit_merged (uploading): a leader waits a moment for them
    long long device_direct = 0; // rsr_process_device calls that ran on the caller's own stream (the engine was idle), under mu
    long long batch_calls = 0, batch_images = 0, batch_groups = 0; // rsr_process_device_batch: calls, their images, the tile batches they enqueued; under mu
    std::atomic<bool> merge_mixed{true}; // option "merge_mixed": a merged batch may hold images of different sizes (0: of one geometry only)
    TableRing mix_ring;              // the device tables of such batches (uploaded table by table: no pinned images)
    std::atomic<long long> merged_mixed{0}; // stat: merged batches whose images differed in size
    // masked calls (rsr_process_device_masked): the tables of the selected tiles, built per call, in a ring of their own; they are laid out
    // in the slot's pinned image and go to the device with ONE asynchronous copy on the call's stream
    TableRing mask_ring;
    long long masked_calls = 0, masked_tiles_run = 0, masked_tiles_skipped = 0, masked_batches = 0; // stats, under mu
    double masked_table_us = 0; // stat: host time spent building and uploading those tables
    // frame sequences (rsr_process_device_sequence); their tables travel in the rotating buffers of the masked calls
    long long seq_calls = 0, seq_frames = 0, seq_tiles_run = 0, seq_tiles_copied = 0, seq_batches = 0; // stats, under mu
    long long video_frames = 0, video_windows = 0, video_tiles_run = 0, video_tiles_skipped = 0; // of the video sessions (video.cpp), under mu
    long long image_items(int w, int h, long long limit) const;
    int merge_width(int w, int h, int c) const; // images of this geometry one batch may take (1: not a small image / merging off)
    int submit_merged(MergeReq& r);             // returns when r's batch has been ENQUEUED (r.ev_done recorded) or failed
    int run_group(MergeReq* const* g, int n);   // mu inside

    std::mutex mu; // compute section: plan cache, workspace, kernel enqueue, profiling state
    std::vector<hipEvent_t> sync_events; // free list, under mu

    // profiling
    bool profiling = false;
    std::vector<hipEvent_t> ev_pool;
    struct Seg
    {
        int cls; // 0 pre, 1 conv, 2 post
        double flops, bytes;
        int conv_index;
    };
    std::vector<double> conv_ms_by_index; // [nconv], resized and zeroed on every load
    std::vector<Seg> segs;
    size_t ev_used = 0;
    rsr_profile prof{};
    void (*progress)(int done, int total, void* user) = nullptr; // per tile batch (the reference prints per tile, realsr.cpp:481)
    void* progress_user = nullptr;

    ~Engine();
    int init(int gpuid, int tta_mode);
    int load_files(const char* param, const char* bin);
    int load_blob_host(const void* blob, size_t bytes);
    int load_blob_device(const void* blob, size_t bytes);
    // d_in/d_out on this device.  user_stream == nullptr: returns when the output is complete (sync) or enqueued (!sync);
    // otherwise ordered after / before the work of user_stream, asynchronous.
    // in_fmt / out_fmt: RSR_FMT_* of the two images (the planar float formats need c == 3; such a call is never merged with others)
    int process_device(const void* d_in, int w, int h, int c, void* d_out, hipStream_t user_stream, bool sync, int in_fmt = RSR_FMT_U8_HWC,
                       int out_fmt = RSR_FMT_U8_HWC);
    // n images of one geometry, each behind its own descriptor (pointer, row pitch, plane pitch), in groups of merge_width(w, h, c) images:
    // every group ONE tile batch on the cached merged plan (include/realsr_hip.h rsr_process_device_batch).  Stream contract: on_stream.
    // mask (n == 1 only; include/realsr_hip.h rsr_process_device_masked): nmask bytes, one per tile of the row-major grid; only the tiles with
    // a non-zero byte run (enqueue_masked).  No tile set: nothing is launched; every tile set: the call without a mask.
    int process_device_batch(int n, const rsr_image* in, int in_fmt, int w, int h, int c, const rsr_image* out, int out_fmt, hipStream_t user_stream, bool sync,
                             const uint8_t* mask = nullptr, int nmask = 0);
    // mask[t] = do the images a and b differ inside tile t's source rectangle (include/realsr_hip.h rsr_diff_tiles); d_mask: device, one byte per tile
    int diff_tiles(const rsr_image* a, const rsr_image* b, int fmt, int w, int h, int c, uint8_t* d_mask, hipStream_t user_stream);
    int diff_pairs(int n, const ImageRef* r, int fmt, int w, int h, int c, uint8_t* d_masks, hipStream_t user_stream); // what the two diffs share: the launch for checked images r[0 .. n]
    // Frame sequences (include/realsr_hip.h "frame sequences").  diff_tiles_sequence: row k of d_masks = diff_tiles(frames[k - 1], frames[k]), row 0
    // against prev (null: all ones); one memset, one launch.  process_device_sequence: the tiles of in[k] whose mask byte is set walk the
    // network as shared tile batches (enqueue_sequence); every other output rectangle is copied from the frame that computed it last, or
    // from prev_out, by one launch behind the last batch.
    int diff_tiles_sequence(int n, const rsr_image* frames, const rsr_image* prev, int fmt, int w, int h, int c, uint8_t* d_masks, hipStream_t user_stream);
    // Three-plane YUV frames <-> surfaces (include/realsr_hip.h rsr_pack_planes / rsr_unpack_planes): n frames of one geometry, one launch on the
    // caller's stream with the contract of diff_tiles; pack: planes -> surface.  Everything is checked before the launch.
    int move_planes(bool pack, int n, const rsr_planes* planes, const rsr_image* surf, int fmt, int w, int h, hipStream_t user_stream);
    int process_device_sequence(int n, const rsr_image* in, int in_fmt, int w, int h, int c, const rsr_image* out, int out_fmt, const rsr_image* prev_out,
                                const uint8_t* masks, int nmask, hipStream_t user_stream, bool sync);
    // tile0/tile1: tiles [tile0, tile1) of the row-major tile grid only (tile1 < 0: all); `out` is always the full (w * out_scale x h * out_scale x c) image,
    // only the output rectangles of
    // those tiles are written
    int process_host(const uint8_t* in, int w, int h, int c, uint8_t* out, int tile0 = 0, int tile1 = -1);
    // host images of any format pair process_device takes, tightly packed (include/realsr_hip.h rsr_process_fmt); never merged, whole images only
    int process_host_fmt(const void* in, int in_fmt, int w, int h, int c, void* out, int out_fmt);
    // The steps of a host entry point behind its checks, each on the lane the call holds:
    // d_out of dev_bytes; out_pinned: `out` is pinned memory and receives the copies directly, else the two staging slots of a download of fetch_bytes are made
    int lane_reserve_out(Lane& L, const void* out, size_t dev_bytes, size_t fetch_bytes, bool& out_pinned);
    int lane_upload(Lane& L, const void* in, size_t nin);                                 // d_in <- in on the copy stream (pageable memory through h_in), ev_in behind it
    // the tiles [tile0, tile1) of io on the compute stream behind ev_in, ev_done behind them; refuses when the context is no longer what the call's checks saw (T, io.os)
    int lane_run(LaneHold& hold, const BatchIO& io, int tile0, int tile1, int T, size_t* half_rows);
    int lane_fetch(Lane& L, char* out, bool out_pinned, size_t rowbytes, const FetchPlan& fp); // the spans of fp: d_out -> out, each behind its event; returns when they have arrived
    int net_forward(const uint16_t* in, int w, int h, uint16_t* out, float* out32 = nullptr); // out32: the fp32 result (precise mode only)
    // out = act(conv + b); with s1 != 0: v = s1*(conv + b) [+ in[0:cout] when own_res] [, v = s2*v + res when res]
    // precise form (in_lo / res_lo / out_lo, any may be null): the hi + lo / 2048 residual stream of ConvArgs::precise
    int conv_test(const uint16_t* in, int cin, int h, int w, int ups, const float* weight, const float* bias, int cout, int lrelu,
                  uint16_t* out, float s1 = 0.f, int own_res = 0, const uint16_t* res = nullptr, float s2 = 1.f, bool prec = false,
                  const uint8_t* in_lo = nullptr, const uint8_t* res_lo = nullptr, uint8_t* out_lo = nullptr);

    // ---- internals (call with `mu` held unless noted) ----
    static constexpr int plane_ch() { return kPlaneCh; }
    // The call skeleton of the device entry points (DESIGN.md "The call skeleton of a device entry point"): image_refs, admit, on_stream.
    // admit: may a w x h image leave in out_fmt at output ratio os -- out_admit (a w or h below 1 is left to the
    // descriptor check) --; with `enter`, the call is about to enqueue: before those, is a model loaded, the scale 4, and os still the
    // ratio in force (the descriptors were checked against os in front of the lock).
    int admit(int out_fmt, int w, int h, OutRatio os, bool enter) const;
    // In FRONT of the lock (mu is taken inside, for a moment): *os = the ratio in force and admit(.., false) -- a ratio the images do not
    // take is refused before any descriptor is looked at --, then image_refs of in[i] and of out[i], image by image.
    int check_pairs(int n, const rsr_image* in, int in_fmt, int w, int h, int c, const rsr_image* out, int out_fmt, OutRatio* os, ImageRef* src, ImageRef* dst);
    // The stream protocol.  lk holds mu.  An idle engine (nothing pending on the compute stream) with a caller's stream runs body on that
    // stream -- no event hop -- and makes the compute stream wait behind it; a call that ends so with RSR_OK counts in device_direct.
    // Otherwise body runs on the compute stream, behind what the caller's stream holds, and the caller's stream is ordered behind it (or,
    // without one, a sync call waits for it, lk released meanwhile).  body(st, enqueued) enqueues on st and returns RSR_*; it sets
    // `enqueued` when it put anything on st: then the ordering behind it happens also where body failed later on.
    template <class Body> int on_stream(std::unique_lock<std::mutex>& lk, hipStream_t user_stream, bool sync, Body body);
    int tile_count(int w, int h, int* nx = nullptr) const { const int x = (w + tilesize - 1) / tilesize; if (nx) *nx = x; return x * ((h + tilesize - 1) / tilesize); } // tiles of the grid (realsr.cpp:170-171)
    static int ensure(DevBuf& b, size_t bytes);
    int ensure_planes(DevBuf& b, size_t bytes, long long plane_bytes, bool layout_changed, bool zero_all, hipStream_t st);
    int get_plan(int w, int h, int c, int tile0, int tile1, int nimg, Plan*& out);
    // Every merged batch -- of one geometry (get_plan, nimg > 1) or of several (enqueue_mixed) -- gives its slots the capacity of a full tile: the
    // workspace layout, hence its guards, then stays put from batch to batch whatever small images come
    long long merged_cap_px() const { return (long long)(tilesize + 2 * prepadding) * (tilesize + 2 * prepadding); }
    long long budget_slots(long long cap_px, int w, int h, int c); // slots of cap_px LR pixels one tile batch may have: the memory policy of get_plan and enqueue_masked
    long long device_avail(int w, int h, int c);
    void free_workspace(hipStream_t st);
    int ensure_workspace(int nslots, long long cap_px, hipStream_t st);
    WsLayout layout() const { return WsLayout{ws_cap_px, precise}; } // of the workspace as ensure_workspace left it
    PlaneSrc ws_planes(int buf, int plane = 0) const // plane `plane` of slot 0 of a workspace buffer, with the buffer's strides
    {
        return PlaneSrc{static_cast<const char*>(ws[buf].p) + layout().plane_off(buf, plane), layout().slot_stride(buf), layout().plane_bytes(buf)};
    }
    // no TTA merge / alpha channel / box reduction / YUV surface / uint16 image needs the planar blob (kDbgNoFusedLast: off); nor does a
    // dithered uint8 image (the planar float formats are not dithered and keep the fused store)
    bool conv_last_writes_image(int c, int out_fmt) const
    {
        return !tta && c == 3 && out_ratio == OutRatio() && !fmt_is_yuv(out_fmt) && out_fmt != kFmtU16 && !(dbg & kDbgNoFusedLast) &&
               !(dither && out_fmt == kFmtU8);
    }
    int check_tile_px(long long cap_px) const; // RSR_E_ARG when the 32-bit plane offsets of the kernels cannot address a slot of cap_px LR pixels
    // The first nslots_used slots of the batch through the network (a merged batch narrower than its plan: fewer than b.nslots).
    // io: null = conv_last leaves the planar OUT3 blob (the hooks below; with an io, a TTA or RGBA batch gets it too).
    // probe: non-null = every convolution is followed by a range-probe launch on what it stored (the self-check's one-tile batch in
    // fp16 storage only; null everywhere else: the launch sequence is then exactly the one without it)
    int run_network(const Plan::Batch& b, hipStream_t st, int nslots_used, const BatchIO* io, const RangeProbe* probe);
    int launch_batch(const Plan::Batch& b, int max_tw, int max_th, int ntiles, hipStream_t st, const BatchIO& io);
    int enqueue_mixed(MergeReq* const* g, int n, hipStream_t st, hipEvent_t ev_mid); // a merged batch of images of different sizes: tables built on the fly
    int enqueue_masked(BatchIO io, const std::vector<int>& sel, hipStream_t st);     // the tiles `sel` (ascending) of the ONE image of io: tables built on the fly
    // The (image, tile) pairs `sel` (frame-major, tile = image * tiles_per_image + tile of the grid) of the io.nimg images of ONE geometry:
    // tables built on the fly, then the copies `rects` in one launch behind the last batch (either may be empty).  enqueue_masked is this with
    // one image and no copies.  batches_stat / table_us (may be null): the stats of the caller's kind of call
    int enqueue_sequence(BatchIO io, const std::vector<int>& sel, const std::vector<PropRect>& rects, hipStream_t st, long long& batches_stat, double* table_us);
    int launch(const ConvArgs& a, int ci, const Plan::Batch& b, hipStream_t st);
    // The images of io -- all of io.w[0] x io.h[0] -- as ONE tile batch per workspace-full: tiles [tile0, tile1) of the tile grid
    // (tile1 < 0: all; whole images only when io.nimg > 1).  io.ev_half with half_rows: the engine may split the 4x tail and reports
    // the output rows that are complete at ev_half.
    // plan_nimg: 0 = the call of one caller; else a merged batch whose plan is the one of plan_nimg >= io.nimg images, of which only the
    // first io.nimg are launched (every width of a merged batch shares ONE plan: slots, tiles and work items of an image are
    // contiguous, so a narrower batch is a prefix of the tables)
    int enqueue_images(BatchIO io, int tile0, int tile1, int plan_nimg, size_t* half_rows, hipStream_t st);
    // The one-tile batch of net_forward and selfcheck: its tables and the caller's planar fp16 [3][h][w] tile in device scratch
    struct OneTile
    {
        Plan::Batch b;
        ScratchBuf tab, tile;
        int w = 0, h = 0;
    };
    int one_tile_upload(OneTile& t, const uint16_t* tile, int w, int h);
    int one_tile_walk(const OneTile& t, const RangeProbe* probe); // workspace of the current storage mode, tile -> IN, the network (never profiled)
    void mark_begin(hipStream_t st);
    void mark(int cls, double flops, double bytes, hipStream_t st, int conv_index = -1);
    void collect_profile(hipStream_t st);
    void free_plans();
    hipEvent_t take_event();
    hipEvent_t take_event_timed(); // caller destroys
    void give_event(hipEvent_t e);
    Lane* acquire_lane(); // lane_mu inside
    void release_lane(Lane* l);
    int adopt_table(const unsigned char* head, size_t head_bytes, size_t bytes); // check_packed of a header + table that came from anywhere
    void adopt_model(const unsigned char* head);             // a validated header + table -> convs, nb / nrdb / nconv; drops what belonged to the old model
    static int fail(int code, const std::string& msg);
};

// Host-only: the resolved row and plane pitch (bytes) of a w x h x c image in `fmt` described with row_pitch / plane_pitch (0 = tightly
// packed), or RSR_E_ARG (through Engine::fail) for a combination rsr_process_device_batch refuses.  plane = 0 for uint8 HWC.
int image_layout(int fmt, int w, int h, int c, long long row_pitch, long long plane_pitch, long long* row, long long* plane);
// Host-only: THE descriptor check of the device entry points.  im[0 .. n) describe images of one format and geometry: w x h x c, or with
// os the os->of(w) x os->of(h) results of such images.  Per descriptor, in this order: a null `data`, image_layout, w or h beyond 2^24 (of
// the input geometry: what the kernels' tile coordinates hold), `data` no multiple of PixFmt::align.  out[i] receives the resolved
// image; a refusal is RSR_E_ARG (through Engine::fail), its message led by `what` (+ " <index0 + i>" where index0 >= 0).
int image_refs(int n, const rsr_image* im, int fmt, int w, int h, int c, const OutRatio* os, const char* what, int index0, ImageRef* out);
// Host-only (include/realsr_hip.h rsr_sequence_sources): src[k * ntiles + t] = the frame whose computed rectangle output tile t of frame k
// shows -- k itself where masks[k][t] != 0, else the last j < k with masks[j][t] != 0, else -1 = the previous output.  RSR_E_ARG (through
// Engine::fail) for n outside 1 .. kMaxMerge, ntiles < 1, a null pointer, or a -1 while has_prev == 0.
int sequence_sources(int n, int ntiles, const uint8_t* masks, int has_prev, int* src);
// Host-only: the constants of the YUV definition for a matrix (709 / 601 / 2020), a range (0 limited, 1 full) and a bit depth (8 / 10);
// false for any other combination.
bool yuv_coef(int matrix, int range, int bits, YuvCoef* out);
void selfcheck_tile(uint16_t* dst, int w, int h); // host-only: the built-in tile of the self-check, planar fp16 [3][h][w]
const char* last_error(); // message of the calling thread's last failure
long long share_pool_stat(int what); // group.cpp: 0 = worker threads of rsr_process_group's pool, 1 = shares run inline because no worker could be started

} // namespace rsr

// The opaque context of the C-ABI (include/realsr_hip.h): ONE definition for every translation unit.
struct rsr_ctx
{
    rsr::Engine e;
};
