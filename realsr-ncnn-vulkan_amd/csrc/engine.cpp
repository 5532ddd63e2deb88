// engine.cpp -- host side of the tiled engine (compiled by hipcc as HIP host code).  See engine.h.
#include "engine.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

namespace rsr {

static thread_local std::string tl_err;
const char* last_error() { return tl_err.c_str(); }

#define HIP_TRY(expr)                                                                              \
    do                                                                                             \
    {                                                                                              \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return Engine::fail(RSR_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

int Engine::fail(int code, const std::string& msg)
{
    tl_err = msg;
    return code;
}

CopyPool::~CopyPool()
{
    {
        std::lock_guard<std::mutex> lk(m);
        stop = true;
    }
    cv.notify_all();
    for (std::thread& t : workers) t.join();
}

void CopyPool::copy(void* dst, const void* src, size_t n, int threads)
{
    const size_t kMin = size_t(1) << 20; // pieces below 1 MiB are not worth a hand-off
    int parts = int(std::min<size_t>(size_t(std::max(threads, 1)), n / kMin));
    if (parts <= 1)
    {
        std::memcpy(dst, src, n);
        return;
    }
    const size_t piece = ((n + parts - 1) / parts + 4095) & ~size_t(4095);
    int pending = 0;
    {
        std::lock_guard<std::mutex> lk(m);
        while (int(workers.size()) < threads - 1)
            workers.emplace_back([this]() {
                std::unique_lock<std::mutex> lk(m);
                for (;;)
                {
                    cv.wait(lk, [this]() { return stop || !q.empty(); });
                    if (q.empty()) return; // stop
                    const Job j = q.front();
                    q.pop_front();
                    lk.unlock();
                    std::memcpy(j.dst, j.src, j.n);
                    lk.lock();
                    if (--*j.pending == 0) done.notify_all();
                }
            });
        for (size_t off = piece; off < n; off += piece)
        {
            q.push_back(Job{static_cast<char*>(dst) + off, static_cast<const char*>(src) + off, std::min(piece, n - off), &pending});
            pending++;
        }
    }
    cv.notify_all();
    std::memcpy(dst, src, std::min(piece, n));
    std::unique_lock<std::mutex> lk(m);
    done.wait(lk, [&]() { return pending == 0; });
}

Engine::~Engine()
{
    if (device >= 0) (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    for (auto& l : lanes)
    {
        if (l->copy) (void)hipStreamSynchronize(l->copy);
        if (l->d_in.p) (void)hipFree(l->d_in.p);
        if (l->d_out.p) (void)hipFree(l->d_out.p);
        if (l->h_in) (void)hipHostFree(l->h_in);
        if (l->h_out) (void)hipHostFree(l->h_out);
        for (hipEvent_t* e : l->events())
            if (*e) (void)hipEventDestroy(*e);
        if (l->copy) (void)hipStreamDestroy(l->copy);
    }
    free_plans();
    for (DevBuf* b : {&blob, &blob_a, &blob_b, &blend_tab, &zeros, &trace_buf})
        if (b->p) (void)hipFree(b->p);
    for (DevBuf& b : ws)
        if (b.p) (void)hipFree(b.p);
    for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : sync_events) (void)hipEventDestroy(e);
    if (merge_mid) (void)hipEventDestroy(merge_mid);
    if (merge_done) (void)hipEventDestroy(merge_done);
    mix_ring.free();
    mask_ring.free();
    flat_ring.free();
    alpha_ring.free();
    if (stream) (void)hipStreamDestroy(stream);
}

int TableRing::acquire(size_t bytes, bool want_stage)
{
    k = int(seq++ % 3);
    if (ev[k]) HIP_TRY(hipEventSynchronize(ev[k])); // the call that read this slot last has finished (its copy from the pinned image too)
    if (const int rc = Engine::ensure(tab[k], bytes)) return rc;
    if (!want_stage || stage_bytes[k] >= bytes) return RSR_OK;
    if (stage[k]) (void)hipHostFree(stage[k]);
    stage[k] = nullptr, stage_bytes[k] = 0;
    if (hipHostMalloc(&stage[k], bytes, hipHostMallocDefault) != hipSuccess)
    {
        (void)hipGetLastError();
        stage[k] = nullptr;
        return Engine::fail(RSR_E_NOMEM, "hipHostMalloc(" + std::to_string(bytes) + ") for the tile tables failed");
    }
    stage_bytes[k] = bytes;
    return RSR_OK;
}

void TableRing::release(hipStream_t st)
{
    if (!ev[k] && hipEventCreateWithFlags(&ev[k], hipEventDisableTiming) != hipSuccess) ev[k] = nullptr;
    if (!ev[k] || hipEventRecord(ev[k], st) != hipSuccess) (void)hipStreamSynchronize(st);
}

void TableRing::free()
{
    for (int i = 0; i < 3; i++)
    {
        if (ev[i]) (void)hipEventDestroy(ev[i]);
        if (tab[i].p) (void)hipFree(tab[i].p);
        if (stage[i]) (void)hipHostFree(stage[i]);
        ev[i] = nullptr, tab[i] = DevBuf(), stage[i] = nullptr, stage_bytes[i] = 0;
    }
}

int Engine::init(int gpuid, int tta_mode)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(RSR_E_DEVICE, "no HIP device available (this engine has no CPU fallback)");
    if (gpuid < 0 || gpuid >= n) return fail(RSR_E_DEVICE, "invalid gpu device " + std::to_string(gpuid));
    device = gpuid;
    tta = tta_mode ? 1 : 0;
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(RSR_E_DEVICE, std::string("kernels are built for gfx950 only, device is ") + prop.gcnArchName);
    num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    HIP_TRY(kernels_init_device()); // per-device opt-in to > 64 KiB dynamic LDS for every kernel instantiation
    HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIP_TRY(hipMalloc(&zeros.p, 256));
    zeros.bytes = 256;
    HIP_TRY(hipMemsetAsync(zeros.p, 0, 256, stream)); // on OUR stream: it is non-blocking, the null stream does not order with it
    HIP_TRY(hipStreamSynchronize(stream));
    return RSR_OK;
}

// Grow-only device buffer.  Growing frees the old allocation: the caller guarantees nothing in flight uses it
// (workspace: the compute stream is drained first; lane buffers: the lane is owned by the caller).
int Engine::ensure(DevBuf& b, size_t bytes)
{
    if (b.bytes >= bytes && b.p) return RSR_OK;
    if (b.p)
    {
        (void)hipFree(b.p);
        b.p = nullptr;
        b.bytes = 0;
    }
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess)
    {
        b.p = nullptr;
        (void)hipGetLastError();
        return fail(RSR_E_NOMEM, "hipMalloc(" + std::to_string(bytes) + ") failed: " + hipGetErrorString(e));
    }
    b.bytes = bytes;
    return RSR_OK;
}

hipEvent_t Engine::take_event()
{
    if (!sync_events.empty())
    {
        hipEvent_t e = sync_events.back();
        sync_events.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    return e;
}

hipEvent_t Engine::take_event_timed()
{
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

void Engine::give_event(hipEvent_t e)
{
    if (e) sync_events.push_back(e);
}

// ---- model --------------------------------------------------------------------------------
int Engine::adopt_table(const unsigned char* head, size_t head_bytes, size_t bytes)
{
    std::string e;
    const int rc = check_packed(head, head_bytes, bytes, e);
    if (rc != RSR_OK) return fail(rc, e);
    return RSR_OK;
}

// The model changes hands.  Plans and workspace do not depend on the depth (tile tables, slot layout and the margins of tail_margin are
// those of the convs behind the trunk, which every depth has), so they stay.  What described the OLD model goes: the self-check's
// report and ranges, a `precise` that its recommendation switched on, and the per-convolution times.
void Engine::adopt_model(const unsigned char* head)
{
    PackedHeader H;
    std::memcpy(&H, head, sizeof H);
    const PackedConv* T = reinterpret_cast<const PackedConv*>(head + sizeof(PackedHeader));
    convs.assign(T, T + H.nconv);
    nconv = int(H.nconv);
    nb = depth_of_convs(H.nconv);
    nrdb = 3 * nb;
    model_head.assign(head, head + packed_table_bytes(H.nconv));
    drop_model_state();
    loaded = true;
}

void Engine::drop_model_state()
{
    sc_peak.assign(size_t(nconv), 0.f);
    sc_nonfinite.assign(size_t(nconv), 0);
    conv_ms_by_index.assign(size_t(nconv), 0.0);
    std::memset(&sc_last, 0, sizeof sc_last);
    sc_have = false;
    if (precise_by_auto) precise = false;
    precise_by_auto = false;
}

int Engine::load_blob_host(const void* data, size_t bytes)
{
    if (!data || bytes < sizeof(PackedHeader)) return fail(RSR_E_FORMAT, "packed blob too small");
    // validate BEFORE touching engine state: a failed load leaves a previously loaded model intact
    int rc = adopt_table(static_cast<const unsigned char*>(data), bytes, bytes);
    if (rc != RSR_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamSynchronize(stream));
    DevBuf fresh;
    if ((rc = ensure(fresh, bytes)) != RSR_OK) return rc;
    hipError_t he = hipMemcpy(fresh.p, data, bytes, hipMemcpyHostToDevice);
    if (he != hipSuccess)
    {
        (void)hipFree(fresh.p);
        return fail(RSR_E_DEVICE, std::string("blob upload: ") + hipGetErrorString(he));
    }
    if (blob.p) (void)hipFree(blob.p);
    blob = fresh;
    drop_second(); // a new first model: the pair is gone, the strength back at 0
    adopt_model(static_cast<const unsigned char*>(data));
    return RSR_OK;
}

int Engine::load_blob_device(const void* data, size_t bytes)
{
    // header + table are small: fetch them to the host for validation, keep the payload on device.  The header first: it says how
    // long the table is (nconv, bounded by kMaxConvs before it sizes anything); never more than `bytes` is copied.
    if (!data || bytes < sizeof(PackedHeader)) return fail(RSR_E_FORMAT, "packed blob too small");
    HIP_TRY(hipSetDevice(device));
    PackedHeader H;
    HIP_TRY(hipMemcpy(&H, data, sizeof H, hipMemcpyDeviceToHost));
    if (depth_of_convs(H.nconv) == 0 || packed_table_bytes(H.nconv) > bytes) return fail(RSR_E_FORMAT, "packed blob header mismatch (conv count / size)");
    std::vector<unsigned char> head(packed_table_bytes(H.nconv));
    HIP_TRY(hipMemcpy(head.data(), data, head.size(), hipMemcpyDeviceToHost));
    int rc = adopt_table(head.data(), head.size(), bytes);
    if (rc != RSR_OK) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    DevBuf fresh;
    if ((rc = ensure(fresh, bytes)) != RSR_OK) return rc;
    hipError_t he = hipMemcpy(fresh.p, data, bytes, hipMemcpyDeviceToDevice);
    if (he != hipSuccess)
    {
        (void)hipFree(fresh.p);
        return fail(RSR_E_DEVICE, std::string("blob copy: ") + hipGetErrorString(he));
    }
    if (blob.p) (void)hipFree(blob.p);
    blob = fresh;
    drop_second(); // a new first model: the pair is gone, the strength back at 0
    adopt_model(head.data());
    return RSR_OK;
}

int Engine::load_files(const char* param, const char* bin)
{
    if (!param || !bin) return fail(RSR_E_ARG, "null path");
    Model m;
    std::string e;
    int rc = load_model(param, bin, m, e);
    if (rc != RSR_OK) return fail(rc, e);
    std::vector<unsigned char> buf(packed_size(m));
    rc = pack_model(m, buf.data(), buf.size(), e);
    if (rc != RSR_OK) return fail(rc, e);
    return load_blob_host(buf.data(), buf.size());
}

// ---- network interpolation ----------------------------------------------------------------
void Engine::drop_second()
{
    for (DevBuf* b : {&blob_a, &blob_b, &blend_tab})
    {
        if (b->p) (void)hipFree(b->p);
        *b = DevBuf();
    }
    blend_chunks = 0;
    second = false;
    blend_t = 0.f;
}

int Engine::load_second_files(const char* param, const char* bin)
{
    if (!param || !bin) return fail(RSR_E_ARG, "null path");
    if (!loaded) return fail(RSR_E_STATE, "rsr_load_second: no first model is loaded");
    Model m;
    std::string e;
    int rc = load_model(param, bin, m, e);
    if (rc != RSR_OK) return fail(rc, e);
    std::vector<unsigned char> buf(packed_size(m));
    rc = pack_model(m, buf.data(), buf.size(), e);
    if (rc != RSR_OK) return fail(rc, e);
    return load_second_blob(buf.data(), buf.size(), false);
}

// Everything that can fail happens on fresh allocations; the context changes hands only in the last lines, which cannot fail.
int Engine::load_second_blob(const void* data, size_t bytes, bool is_device)
{
    if (!loaded) return fail(RSR_E_STATE, "rsr_load_second: no first model is loaded");
    if (!data || bytes < sizeof(PackedHeader)) return fail(RSR_E_FORMAT, "packed blob too small");
    HIP_TRY(hipSetDevice(device));
    std::vector<unsigned char> fetched; // header + table of a device blob (load_blob_device)
    const unsigned char* head = static_cast<const unsigned char*>(data);
    size_t head_bytes = bytes;
    if (is_device)
    {
        PackedHeader H;
        HIP_TRY(hipMemcpy(&H, data, sizeof H, hipMemcpyDeviceToHost));
        if (depth_of_convs(H.nconv) == 0 || packed_table_bytes(H.nconv) > bytes) return fail(RSR_E_FORMAT, "packed blob header mismatch (conv count / size)");
        fetched.resize(packed_table_bytes(H.nconv));
        HIP_TRY(hipMemcpy(fetched.data(), data, fetched.size(), hipMemcpyDeviceToHost));
        head = fetched.data(), head_bytes = fetched.size();
    }
    int rc = adopt_table(head, head_bytes, bytes);
    if (rc != RSR_OK) return rc;
    std::string e;
    if ((rc = compare_tables(model_head.data(), head, e)) != RSR_OK) return fail(rc, "second model: " + e);
    HIP_TRY(hipStreamSynchronize(stream));

    // the chunks of the segments: the table is the first model's, so a pair that is already loaded keeps its own
    std::vector<BlendChunk> chunks;
    if (!second)
    {
        std::vector<BlendSeg> segs;
        blend_segments(convs.data(), uint32_t(nconv), segs);
        for (const BlendSeg& s : segs)
            for (uint64_t o = 0; o < s.bytes; o += uint64_t(kBlendChunkUnits) * 16)
                chunks.push_back(BlendChunk{s.off + o, uint32_t(std::min<uint64_t>(s.bytes - o, uint64_t(kBlendChunkUnits) * 16) / 16), s.f32 ? 1u : 0u});
    }
    DevBuf fresh_b, fresh_active, fresh_tab;
    auto give_up = [&](int code) {
        for (DevBuf* b : {&fresh_b, &fresh_active, &fresh_tab})
            if (b->p) (void)hipFree(b->p);
        return code;
    };
    if ((rc = ensure(fresh_b, bytes)) != RSR_OK) return give_up(rc);
    if (!second && ((rc = ensure(fresh_active, bytes)) != RSR_OK || (rc = ensure(fresh_tab, chunks.size() * sizeof(BlendChunk))) != RSR_OK)) return give_up(rc);
    hipError_t he = hipMemcpy(fresh_b.p, data, bytes, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    if (he == hipSuccess && !second)
    { // the active blob starts as ONE device-to-device copy of A -- under the test hook "ws_poison" over a buffer full of its pattern
        if (ws_poison) he = hipMemsetD16(fresh_active.p, (unsigned short)(ws_poison & 0xffff), bytes / 2);
        if (he == hipSuccess) he = hipMemcpy(fresh_active.p, blob.p, bytes, hipMemcpyDeviceToDevice);
        if (he == hipSuccess) he = hipMemcpy(fresh_tab.p, chunks.data(), chunks.size() * sizeof(BlendChunk), hipMemcpyHostToDevice);
    }
    if (he != hipSuccess) return give_up(fail(RSR_E_DEVICE, std::string("second model upload: ") + hipGetErrorString(he)));

    if (second)
        (void)hipFree(blob_b.p);
    else
    {
        blob_a = blob;
        blob = fresh_active;
        blend_tab = fresh_tab;
        blend_chunks = int(chunks.size());
    }
    blob_b = fresh_b;
    second = true;
    // a new second model under a strength that was already chosen: the active blob follows (at 0 it is A's copy and stays)
    return blend_t != 0.f ? apply_blend() : RSR_OK;
}

int Engine::apply_blend()
{
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamSynchronize(stream));
    // under rsr_set_profiling the one launch (or copy) is bracketed with HIP events: stat "blend_us" (tools/blend_perf.py)
    hipEvent_t e0 = profiling ? take_event_timed() : nullptr, e1 = profiling ? take_event_timed() : nullptr;
    if (e0 && e1) (void)hipEventRecord(e0, stream);
    hipError_t he;
    if (blend_t == 0.f || blend_t == 1.f) // copies, not arithmetic
        he = hipMemcpyAsync(blob.p, blend_t == 0.f ? blob_a.p : blob_b.p, blob_a.bytes, hipMemcpyDeviceToDevice, stream);
    else
        he = launch_blend_blob(static_cast<const BlendChunk*>(blend_tab.p), blend_chunks, blob_a.p, blob_b.p, blob.p, blend_t, num_cu, stream);
    if (e0 && e1 && he == hipSuccess) (void)hipEventRecord(e1, stream);
    if (he == hipSuccess) he = hipStreamSynchronize(stream);
    float ms = 0.f;
    last_blend_us = (e0 && e1 && he == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ? double(ms) * 1e3 : -1.0;
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (he != hipSuccess) return fail(RSR_E_DEVICE, std::string("blend: ") + hipGetErrorString(he));
    drop_model_state(); // the weights changed hands: what a self-check said about the old ones, and the times of their convolutions, go
    return RSR_OK;
}

int Engine::set_blend(float t)
{
    if (!second) return fail(RSR_E_STATE, "rsr_set_blend: no second model is loaded (rsr_load_second)");
    if (!(t >= 0.f && t <= 1.f)) return fail(RSR_E_ARG, "rsr_set_blend: the strength must be a number in [0, 1]");
    const float before = blend_t;
    blend_t = t == 0.f ? 0.f : t; // (-0 is 0: the members of a group compare their strengths by the bits)
    const int rc = apply_blend();
    if (rc != RSR_OK) blend_t = before; // (a device error: the active blob may hold either)
    return rc;
}

int Engine::export_model(void* dst, size_t cap, size_t* need)
{
    if (!loaded) return fail(RSR_E_STATE, "rsr_model_export: no model is loaded");
    if (need) *need = blob.bytes;
    if (!dst) return RSR_OK;
    if (cap < blob.bytes) return fail(RSR_E_ARG, "rsr_model_export: buffer too small");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy(dst, blob.p, blob.bytes, hipMemcpyDeviceToHost));
    return RSR_OK;
}

// ---- plan ---------------------------------------------------------------------------------
void Engine::free_plans()
{
    if (plans.empty()) return;
    if (stream) (void)hipStreamSynchronize(stream); // kernels in flight read the tables
    for (Plan& p : plans)
        if (p.d_tables) (void)hipFree(p.d_tables);
    plans.clear();
}

// Dead-output elimination behind the trunk.  The caller keeps only the un-padded rectangle of a tile's output: pixels closer
// than crop4 = prepadding * scale to the tile border are cropped (realsr_postproc.comp:62-69, realsr.cpp:460-461).  Walking
// back from there, every 3x3 conv needs one more ring of its input: conv_last's output is read from margin crop4 inwards,
// HRconv's from crop4 - 1, upconv2's from crop4 - 2; upconv2 reads the nearest-x2 of upconv1's output (2x level) from
// (crop4 - 3) >> 1 = crop4 / 2 - 2, and so on through the last LR convs.  Output pixels outside those regions influence
// nothing that is kept, so their blocks are left out of the work-item tables (block granularity, here) and their 4-row groups
// are skipped by the MFMA waves (ConvArgs::margin).  The bytes of the kept rectangle are unchanged -- this is what a
// compiler calls dead-code elimination; the algorithmic FLOP count still counts the halo densely.
static int tail_margin(int crop4, int which) // which: 0 conv_last, 1 HRconv, 2 upconv2 (4x level), 3 upconv1 (2x level), 4.. LR convs backwards
{
    if (crop4 <= 0) return 0;
    int m;
    if (which <= 2) m = crop4 - which;
    else
    {
        m = crop4 / 2 - 2; // upconv1: (crop4 - 3) >> 1 below, the same above for the even crops prepadding * 4 gives
        if (which >= 4)
        {
            m = (m - 1) >> 1;  // trunk_conv: read by upconv1 through the nearest-x2 gather
            m -= (which - 4);  // the last RDB's conv5, conv4, ... each one ring further out
        }
    }
    return m > 0 ? m : 0;
}

// The work items of one H x W tile plane: 16 x 32 blocks row-major; blocks wholly inside the margin `m` (dead-output elimination)
// are left out.  With `fold` a last column of 1..kFoldMaxW pixels is covered by FOLDED items (kernels.h), one per pair of block rows,
// placed behind the second row of the pair: C3's 420-wide tiles 13 columns + 14 folded items instead of 14 x 27 blocks (-3.4 %),
// the 140-wide edge tiles of C2 4 columns + 7 folded items instead of 5 x 14 (-10 %).  Tile geometry: realsr.cpp:170-181,246-249.
// The kernel decides "these four rows need no matrix work" (wave_is_dead) from a folded block's FIRST strip alone; that is exact for
// rows below the tile and for the bottom margin, and it would be wrong where the first strip lies in the TOP margin and the second
// does not -- so block rows that start above `mtop` (the largest margin any conv of this level is launched with) stay plain blocks and
// the pairing begins below them.
void append_block_items(std::vector<WorkItem>& out, int slot, int H, int W, int m, int mtop, int p0, int p1, int p2, bool fold)
{
    const int rem = W % kBlkW;
    const bool fold_last = fold && rem >= 1 && rem <= kFoldMaxW;
    const int wfull = fold_last ? W - rem : W; // columns covered by plain blocks in every row
    auto row_skipped = [&](int y0) { return y0 + kBlkH <= m || y0 >= H - m; };
    auto plain_row = [&](int y0, int x_from, int x_to) {
        for (int x0 = x_from; x0 < x_to; x0 += kBlkW)
        {
            if (row_skipped(y0) || x0 + kBlkW <= m || x0 >= W - m) continue; // nothing kept depends on it
            out.push_back(WorkItem{slot, y0, x0, H, W, p0, p1, p2});
        }
    };
    // block rows above the first one that starts at or below `mtop` stay plain; pairs are counted from there
    const int first_pair = fold_last ? std::min(H, (mtop + kBlkH - 1) / kBlkH * kBlkH) : H;
    for (int y0 = 0; y0 < first_pair; y0 += kBlkH) plain_row(y0, 0, W);
    for (int y0 = first_pair; y0 < H; y0 += 2 * kBlkH) // pairs of block rows
    {
        const bool has2 = y0 + kBlkH < H;
        plain_row(y0, 0, wfull);
        if (has2) plain_row(y0 + kBlkH, 0, wfull);
        const bool dead = (row_skipped(y0) && (!has2 || row_skipped(y0 + kBlkH))) || wfull >= W - m;
        if (!dead) out.push_back(WorkItem{slot, y0, wfull | kFoldBit, H, W, p0, p1, p2});
    }
}

// place4 = prepadding * scale when the slots ARE the tiles (non-TTA: conv_last may write the image itself), < 0 otherwise
// (TTA: 8 slots per tile, net_forward); trim4 = prepadding * scale when only the cropped rectangle is kept, 0 = keep all
static void make_items(Plan::Batch& b, bool fold, int place4 = -1, int trim4 = 0, int out_row0 = 0)
{
    const int margin[3] = {0, tail_margin(trim4, 3), tail_margin(trim4, 2)}; // per level: the smallest margin of its convs
    const int mtop[3] = {tail_margin(trim4, 4), tail_margin(trim4, 3), tail_margin(trim4, 0)}; // ... and the largest (append_block_items)
    for (int lvl = 0; lvl < 3; lvl++)
    {
        b.items[lvl].clear();
        b.item_start[lvl].assign(size_t(b.nslots) + 1, 0);
        b.px[lvl] = 0;
        const int m = margin[lvl];
        for (int s = 0; s < b.nslots; s++)
        {
            b.item_start[lvl][size_t(s)] = int(b.items[lvl].size());
            const int H = b.dims[size_t(s)].h << lvl, W = b.dims[size_t(s)].w << lvl;
            b.px[lvl] += double(H) * W;
            // 4x-level items carry the tile's placement in the output image: conv_last can write the uint8 image itself
            int p0 = 0, p1 = 0, p2 = 0;
            if (lvl == 2 && place4 >= 0 && size_t(s) < b.tiles.size())
            {
                const BaseTile& t = b.tiles[size_t(s)];
                p0 = t.out_x - place4;
                p1 = t.out_y - out_row0 - place4; // rows relative to the first output row the caller's device buffer holds
                p2 = item_pad2(t.out_w, t.out_h, t.img);
            }
            append_block_items(b.items[lvl], s, H, W, m, mtop[lvl], p0, p1, p2, fold);
        }
        b.item_start[lvl][size_t(b.nslots)] = int(b.items[lvl].size());
    }
}

static size_t al256(size_t v) { return (v + 255) & ~size_t(255); }

static size_t batch_table_bytes(const Plan::Batch& b)
{
    size_t n = al256(b.tiles.size() * sizeof(BaseTile)) + al256(b.dims.size() * sizeof(TileDim));
    for (int l = 0; l < 3; l++) n += 2 * al256(b.items[l].size() * sizeof(WorkItem));
    return n;
}

// Makes b the tile batch of the `count` tiles tile_at(0 .. count) (each with the index of its image in BaseTile::img), the tile0-th of its
// call onwards: every tile gets its slots (eight orientations under TTA, realsr.cpp:251-258; else one), then the work-item tables.  crop4 =
// prepadding * scale; out_row0: make_items.  Returns the bytes of the batch's device tables.
template <class TileAt>
static size_t fill_batch(Plan::Batch& b, int tile0, int count, TileAt tile_at, bool tta, int crop4, bool trim, bool fold, int out_row0)
{
    const int per = tta ? 8 : 1;
    b.tile0 = tile0;
    b.ntiles = count;
    b.nslots = count * per;
    for (int i = 0; i < count; i++)
    {
        BaseTile t = tile_at(i);
        t.slot0 = i * per;
        b.tiles.push_back(t);
        for (int k = 0; k < per; k++) b.dims.push_back(k < 4 ? TileDim{t.th, t.tw} : TileDim{t.tw, t.th});
    }
    b.trim4 = trim ? crop4 : 0;
    make_items(b, fold, tta ? -1 : crop4, b.trim4, out_row0);
    return batch_table_bytes(b);
}

// upload one batch's tables behind `d`; every copy is checked.  stage: non-null = the tables are only laid out, behind *stage on the host,
// as they will lie behind `d`; the caller copies the whole stage with one hipMemcpy (a masked call: several batches per call, every call)
static hipError_t upload_batch(Plan::Batch& b, char*& d, bool xcd_order = true, char** stage = nullptr)
{
    hipError_t err = hipSuccess;
    auto put = [&](const void* src, size_t bytes) -> void* {
        void* at = d;
        if (stage)
        {
            if (bytes) std::memcpy(*stage, src, bytes);
            *stage += al256(bytes);
        }
        else if (bytes && err == hipSuccess) err = hipMemcpy(at, src, bytes, hipMemcpyHostToDevice);
        d += al256(bytes);
        return at;
    };
    b.d_tiles = static_cast<BaseTile*>(put(b.tiles.data(), b.tiles.size() * sizeof(BaseTile)));
    b.d_dims = static_cast<TileDim*>(put(b.dims.data(), b.dims.size() * sizeof(TileDim)));
    for (int l = 0; l < 3; l++)
    {
        b.d_items[l] = static_cast<WorkItem*>(put(b.items[l].data(), b.items[l].size() * sizeof(WorkItem)));
        // The backward table.  LR level (never launched in sub-ranges): reversed INSIDE each XCD's share of the list -- the kernel
        // gives XCD x the items [x * per, (x + 1) * per), per = ceil(n / 8) -- so that a conv starts, on every XCD, with the blocks
        // that XCD itself produced last: those sit in ITS 4 MB L2.  (A whole-list reversal hands XCD 0 the blocks XCD 7 wrote:
        // Infinity-Cache hits at best, and the L2-miss path is what bounds the dense-block convs)  The 2x / 4x
        // tables are launched in slot sub-ranges (run_network) and keep the plain reversal.
        std::vector<WorkItem> rev(b.items[l].rbegin(), b.items[l].rend());
        if (l == 0 && xcd_order)
        {
            const size_t n = b.items[l].size(), per = (n + 7) / 8;
            for (size_t x = 0; x < 8; x++)
            {
                const size_t i0 = std::min(n, x * per), i1 = std::min(n, (x + 1) * per);
                for (size_t i = i0; i < i1; i++) rev[i] = b.items[l][i0 + (i1 - 1 - i)];
            }
        }
        b.d_items_rev[l] = static_cast<WorkItem*>(put(rev.data(), rev.size() * sizeof(WorkItem)));
    }
    return err;
}

static constexpr size_t kMaxPlans = 8;

// What the device can give this engine's workspace right now: 90 % of (free memory + the workspace it already holds) minus the
// image buffers its lanes may still allocate (in + 16x out per lane; what they hold already is not free any more).  < 0: unknown.
long long Engine::device_avail(int w, int h, int c)
{
    size_t f = 0, t = 0;
    if (hipMemGetInfo(&f, &t) != hipSuccess)
    {
        (void)hipGetLastError();
        return -1;
    }
    long long held = 0;
    for (const DevBuf& wb : ws) held += (long long)wb.bytes;
    long long lanes_have = 0;
    {
        std::lock_guard<std::mutex> ll(lane_mu);
        for (const auto& l : lanes) lanes_have += (long long)(l->in_bytes.load(std::memory_order_relaxed) + l->out_bytes.load(std::memory_order_relaxed));
    }
    const long long lanes_need = std::max<long long>(0, (long long)max_lanes * 17 * w * h * c - lanes_have);
    return std::max<long long>(0, ((long long)f + held) / 10 * 9 - lanes_need);
}

// The padded tiles [tile0, tile1) of a w x h image (tile grid: realsr.cpp:170-171; tile geometry: realsr.cpp:178-181,237,246-249),
// appended to `all` as tiles of image `img` of a batch; cap / mtw / mth: running maxima of tile pixels / width / height.
static void image_tiles(int w, int h, int T, int P, int scale, int tile0, int tile1, int img, std::vector<BaseTile>& all, long long& cap, int& mtw, int& mth)
{
    const int xtiles = (w + T - 1) / T;
    for (int ti = tile0; ti < tile1; ti++)
    {
        const int yi = ti / xtiles, xi = ti - yi * xtiles;
        const int twn = std::min((xi + 1) * T, w) - xi * T;
        const int thn = std::min((yi + 1) * T, h) - yi * T;
        BaseTile t;
        // Padded tile pixel (gx,gy) samples image pixel reflect101(gx + x_org), reflect101(gy + y_org).
        // The reference reflects against the uploaded row BAND (realsr_preproc.comp:56-62 with
        // crop_y = min(yi*T, P), realsr.cpp:404); the band starts at max(yi*T-P,0) and ends at
        // min((yi+1)*T+P, h), so reflection only ever triggers where the band edge IS the image edge:
        // reflecting against the image gives the same pixel, and the whole image can stay resident.
        t.x_org = xi * T - P;
        t.y_org = yi * T - P;
        t.tw = twn + 2 * P;
        t.th = thn + 2 * P;
        t.slot0 = 0;
        t.out_x = xi * T * scale;
        t.out_y = yi * T * scale;
        t.out_w = twn * scale;
        t.out_h = thn * scale;
        t.img = img;
        all.push_back(t);
        cap = std::max(cap, (long long)t.tw * t.th);
        mtw = std::max(mtw, t.tw);
        mth = std::max(mth, t.th);
    }
}

// The kernels address a plane through 32-bit byte offsets (raw buffer resources, out-of-range sentinel 2^31): the
// largest plane is the 4x level, 16 * cap pixels * 32 B (workspace.h), and an MFMA wave reaches the 2 planes of its n-tile (4 with
// two n-tiles per wave, flow_flags bit 0) from one base; the stores' range limit is "end of the plane + the plane's offset"
// (conv_flow.hip make_out), which must stay below the sentinel too.  Tiles beyond that (~1,400 px) must be split by the caller.
int Engine::check_tile_px(long long cap_px) const
{
    const long long reach = (flow_flags & kFlowNtw2) ? 4 : 2; // planes an MFMA wave addresses from one base
    constexpr long long plane_px = WsLayout::max_plane_px_bytes();
    if (cap_px * plane_px * reach + 4 * kGuard < (1ll << 31)) return RSR_OK;
    const long long max_px = ((1ll << 31) - 4 * kGuard - 1) / (plane_px * reach);
    return fail(RSR_E_ARG, "tilesize too large: a padded tile may have at most " + std::to_string(max_px) + " pixels" +
                               ((flow_flags & kFlowNtw2) ? " with flow_flags bit 0 (e.g. -t 1000)" : " (e.g. -t 1400)"));
}

// Memory policy (the reference bounds device memory through the tile size alone, main.cpp:761-774; here ALL tiles of an image
// form one batch, so the batch is what must be bounded): the budget is max_workspace_mb, but never more than 90 % of what
// the device can actually give this engine right now -- free memory + the workspace it already holds - the image buffers
// of its lanes -- and never more than a size that has already failed to allocate (ws_clamp_bytes, enqueue_images' retry).
// Returns the slots of cap_px LR pixels a batch may have: a whole number of tiles (x8 under TTA), at least one.
long long Engine::budget_slots(long long cap_px, int w, int h, int c)
{
    const int per = tta ? 8 : 1;
    const long long per_slot = cap_px * bytes_per_px();
    long long budget = max_workspace_mb * 1024 * 1024;
    {
        const long long avail = device_avail(w, h, c);
        if (avail >= 0) budget = std::min(budget, std::max<long long>(avail, per_slot * per));
    }
    if (ws_clamp_bytes >= 0) budget = std::min(budget, std::max<long long>(ws_clamp_bytes, per_slot * per));
    const long long slots = budget / std::max<long long>(per_slot, 1);
    return std::max<long long>(per, slots / per * per);
}

int Engine::get_plan(int w, int h, int c, int tile0, int tile1, int nimg, Plan*& out)
{
    const PlanKey key{w, h, c, tilesize, prepadding, tta, nimg, precise, out_ratio, (flow_flags & kFlowNtw2) != 0, tile0, tile1, max_workspace_mb,
                      trim_tail, xcd_order, fold_cols, ws_clamp_bytes}; // (in the order of its fields)
    for (auto it = plans.begin(); it != plans.end(); ++it)
        if (it->key == key)
        {
            plans.splice(plans.begin(), plans, it); // most recently used first
            out = &plans.front();
            return RSR_OK;
        }
    const int T = tilesize, P = prepadding;
    // tile grid: realsr.cpp:170-171; tile geometry: realsr.cpp:178-181,237,246-249
    int xtiles = 0;
    const int ntiles = tile_count(w, h, &xtiles);
    std::vector<BaseTile> all;
    long long cap = 0;
    int mtw = 0, mth = 0;
    if (tile0 < 0 || tile1 > ntiles || tile0 >= tile1) return fail(RSR_E_ARG, "tile range outside the image");
    if (nimg < 1 || nimg > kMaxMerge || (nimg > 1 && (tile0 != 0 || tile1 != ntiles))) return fail(RSR_E_ARG, "merged batches take whole images");
    for (int im = 0; im < nimg; im++) image_tiles(w, h, T, P, scale, tile0, tile1, im, all, cap, mtw, mth);
    if (nimg > 1) cap = std::max(cap, merged_cap_px());
    if (const int rc = check_tile_px(cap)) return rc;
    const int per = tta ? 8 : 1;
    const long long total_slots = (long long)all.size() * per;
    const int spb = int(std::min<long long>(total_slots, budget_slots(cap, w, h, c)));
    const int tiles_per_batch = spb / per;

    Plan plan;
    plan.key = key;
    plan.out_row0 = std::min((tile0 / xtiles) * T, h) * scale; // first output row of the range's first tile row
    plan.cap_px = cap; plan.max_tw = mtw; plan.max_th = mth; plan.slots_per_batch = spb;
    size_t table_bytes = 0;
    for (size_t t0 = 0; t0 < all.size(); t0 += size_t(tiles_per_batch))
    {
        Plan::Batch b;
        table_bytes += fill_batch(b, int(t0), int(std::min(all.size() - t0, size_t(tiles_per_batch))), [&](int i) { return all[t0 + size_t(i)]; }, tta != 0, P * scale,
                                  trim_tail, fold_cols, plan.out_row0);
        plan.batches.push_back(std::move(b));
    }
    if (plans.size() >= kMaxPlans)
    { // evict the least recently used plan; kernels in flight may still read its tables
        HIP_TRY(hipStreamSynchronize(stream));
        if (plans.back().d_tables) (void)hipFree(plans.back().d_tables);
        plans.pop_back();
    }
    HIP_TRY(hipMalloc(&plan.d_tables, table_bytes));
    char* d = static_cast<char*>(plan.d_tables);
    for (Plan::Batch& b : plan.batches)
    {
        const hipError_t e = upload_batch(b, d, xcd_order && nimg == 1); // (a merged plan is launched in prefixes: plain reversal, whose prefixes are suffixes)
        if (e != hipSuccess)
        {
            (void)hipFree(plan.d_tables);
            return fail(RSR_E_DEVICE, std::string("plan table upload: ") + hipGetErrorString(e));
        }
    }
    plans.push_front(std::move(plan));
    out = &plans.front();
    return RSR_OK;
}

// Every fp16 plane that a convolution may read carries a 64-byte zero GUARD in front of pixel 0 (plane = [guard |
// H*W*ppx B]).  The LDS-DMA loaders address a plane as (uniform base, 32-bit lane offset); lanes whose patch pixel
// lies outside the image use offset 0 = the guard, i.e. conv zero padding without a second base pointer.
// Invariant: every guard of the CURRENT layout inside the whole allocation is zero.  A fresh allocation is zeroed
// completely; when the layout (plane stride) changes inside an existing allocation, the guards of the new layout are
// zeroed over the WHOLE allocation (not just the slots this call uses: a later call with more slots of the same layout
// must not find stale pixels where its guards are).  Guards are never written afterwards: stat "ws_guard_dirty" counts their non-zero
// bytes, and tests/test_gpu_ws_hygiene.py finds none after any call.
int Engine::ensure_planes(DevBuf& b, size_t bytes, long long plane_bytes, bool layout_changed, bool zero_all, hipStream_t st)
{
    const bool grow = !(b.bytes >= bytes && b.p);
    if (const int rc = ensure(b, bytes)) return rc; // (does nothing unless the buffer grows)
    if (grow || (layout_changed && zero_all)) HIP_TRY(hipMemsetAsync(b.p, 0, b.bytes, st)); // same stream as the kernels that follow
    else if (layout_changed) launch_zero_guards(b.p, plane_bytes, (long long)(b.bytes / size_t(plane_bytes)), st);
    return RSR_OK;
}

int Engine::ensure_workspace(int nslots, long long cap, hipStream_t st)
{
    const WsLayout lay{cap, precise};
    // The guard positions of a buffer are a function of the slot capacity only: every plane, the lo pair planes of precise mode included
    // (conv_flow.hip lo_row), starts a whole number of plane_bytes behind the buffer's start, and plane_bytes does not depend on `precise`
    // (workspace.h; tools/host_check checks both).  So a change of `precise` alone moves no guard: nothing is zeroed for it.
    const bool lc = cap != ws_cap_px;
    bool any_grow = false;
    for (int i = 0; i < kWsCount; i++)
        if (const size_t need = size_t(lay.bytes(i, nslots)); need && !(ws[i].bytes >= need && ws[i].p)) any_grow = true;
    if (const long long total = (long long)nslots * cap * bytes_per_px(); ws_fail_above_bytes >= 0 && total > ws_fail_above_bytes)
    { // test hook (option "ws_fail_above_mb"): a device on which workspaces above this size persistently fail to allocate
        ws_failures++;
        return fail(RSR_E_NOMEM, "workspace of " + std::to_string(total >> 20) + " MiB refused (ws_fail_above_mb test hook)");
    }
    if (ws_poison)
    { // test hook (option "ws_poison"): the worst history a workspace can have.  Every byte of every buffer takes the pattern; then exactly
      // what a change of slot capacity inside an existing allocation does below -- the guards of this layout zeroed over the whole
      // allocation, the zero_all buffers zeroed -- and nothing more.  Whatever else a call reads, it must have written itself.
        for (int i = 0; i < kWsCount; i++)
            if (const int rc = ensure(ws[i], size_t(lay.bytes(i, nslots)))) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        const unsigned short pat = (unsigned short)(ws_poison & 0xFFFF);
        for (const DevBuf& b : ws)
        {
            if (!b.p || !b.bytes) continue;
            HIP_TRY(hipMemsetD16Async(b.p, pat, b.bytes / 2, st));
            if (b.bytes & 1) HIP_TRY(hipMemsetAsync(static_cast<char*>(b.p) + b.bytes - 1, pat & 0xFF, 1, st));
        }
        for (int i = 0; i < kWsCount; i++) // (no buffer grows any more: ensure_planes takes its layout-change branch)
            if (WsLayout::guarded(i))
                if (const int rc = ensure_planes(ws[i], size_t(lay.bytes(i, nslots)), lay.plane_bytes(i), true, kWsTable[i].zero_all, st)) return rc;
        HIP_TRY(hipGetLastError());
        ws_cap_px = cap;
        return RSR_OK;
    }
    if (any_grow || lc) HIP_TRY(hipStreamSynchronize(st)); // nothing in flight may use a buffer that is freed / re-laid-out
    for (int i = 0; i < kWsCount; i++)
        if (const size_t need = size_t(lay.bytes(i, nslots)); const int rc = WsLayout::guarded(i) ? ensure_planes(ws[i], need, lay.plane_bytes(i), lc, kWsTable[i].zero_all, st) : ensure(ws[i], need))
            return rc;
    HIP_TRY(hipGetLastError());
    ws_cap_px = cap;
    return RSR_OK;
}

void Engine::free_workspace(hipStream_t st)
{
    (void)hipStreamSynchronize(st);
    for (DevBuf& wb : ws) (void)hipFree(wb.p), wb = DevBuf(); // (freeing a null pointer does nothing)
    ws_cap_px = 0;
}

// Stat "ws_guard_dirty" (test hook): the two invariants of the workspace's zeros, counted on the host.  Every guard of the current layout
// over the whole allocation of every guarded buffer (one strided copy per buffer: 64 B at a stride of plane_bytes), and IN's channels
// 3 .. 31 -- the bytes behind the first three halfs of a pixel of a slot's plane 0, and all of its plane 1.  Returns the number of
// non-zero bytes, -1 without a layout, -2 when a copy failed.
long long Engine::ws_guard_dirty()
{
    static_assert(kWsTable[kWsIn].planes == 2 && !kWsTable[kWsIn].lo_planes && kPlaneCh == 16, "IN: one plane of channels 0 .. 15, one of 16 .. 31");
    if (!ws_cap_px) return -1;
    if (hipSetDevice(device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -2; // every stream of the engine: the lanes' too
    const WsLayout lay = layout();
    long long dirty = 0;
    std::vector<unsigned char> h;
    for (int b = 0; b < kWsCount; b++)
    {
        if (!WsLayout::guarded(b) || !ws[b].p) continue;
        const size_t pb = size_t(lay.plane_bytes(b)), n = ws[b].bytes / pb;
        if (!n) continue;
        h.assign(n * kGuard, 0);
        if (hipMemcpy2D(h.data(), kGuard, ws[b].p, pb, kGuard, n, hipMemcpyDeviceToHost) != hipSuccess) return -2;
        for (const unsigned char v : h) dirty += v != 0;
    }
    if (const DevBuf& in = ws[kWsIn]; in.p)
    {
        const size_t pb = size_t(lay.plane_bytes(kWsIn)), n = in.bytes / pb;
        h.assign(in.bytes, 0);
        if (hipMemcpy(h.data(), in.p, in.bytes, hipMemcpyDeviceToHost) != hipSuccess) return -2;
        for (size_t k = 0; k < n; k++) // planes alternate: channels 0 .. 15, channels 16 .. 31
            for (long long p = 0; p < ws_cap_px; p++)
                for (size_t i = (k & 1) ? 0 : 6; i < size_t(WsLayout::kPxBytes); i++) dirty += h[k * pb + kGuard + size_t(p) * WsLayout::kPxBytes + i] != 0;
    }
    return dirty;
}

// ---- profiling ------------------------------------------------------------------------------
// mark_begin() records the opening event of a call; mark() records an event AFTER a launch and labels
// the segment [previous event, this event] with the launch's class.  Events sit on the launch stream.
static hipEvent_t next_event(Engine& e)
{
    if (e.ev_used == e.ev_pool.size())
    {
        hipEvent_t ev;
        if (hipEventCreate(&ev) != hipSuccess) return nullptr;
        e.ev_pool.push_back(ev);
    }
    return e.ev_pool[e.ev_used++];
}

void Engine::mark_begin(hipStream_t st)
{
    if (!profiling) return;
    ev_used = 0;
    segs.clear();
    if (hipEvent_t ev = next_event(*this)) (void)hipEventRecord(ev, st);
}

void Engine::mark(int cls, double flops, double bytes, hipStream_t st, int conv_index)
{
    if (!profiling || ev_used == 0) return;
    if (hipEvent_t ev = next_event(*this))
    {
        (void)hipEventRecord(ev, st);
        segs.push_back(Seg{cls, flops, bytes, conv_index});
    }
}

void Engine::collect_profile(hipStream_t st)
{
    if (!profiling || ev_used < 2) { ev_used = 0; segs.clear(); return; }
    (void)hipStreamSynchronize(st);
    for (size_t i = 0; i < segs.size() && i + 1 < ev_used; i++)
    {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev_pool[i], ev_pool[i + 1]) != hipSuccess) continue;
        const Seg& s = segs[i];
        if (s.cls == 1)
        {
            prof.conv_ms += ms;
            prof.conv_flops += s.flops;
            prof.conv_launches++;
            if (s.conv_index >= 0 && size_t(s.conv_index) < conv_ms_by_index.size()) conv_ms_by_index[size_t(s.conv_index)] += ms;
        }
        else if (s.cls == 0) { prof.pre_ms += ms; prof.pre_bytes += s.bytes; }
        else if (s.cls == 2) { prof.post_ms += ms; prof.post_bytes += s.bytes; }
    }
    float tot = 0.f;
    if (hipEventElapsedTime(&tot, ev_pool[0], ev_pool[ev_used - 1]) == hipSuccess) prof.total_ms += tot;
    ev_used = 0;
    segs.clear();
}

// ---- the network schedule ---------------------------------------------------------------------
// x4.param as a fused schedule.  Buffers per slot (workspace.h kWsTable), in planes of plane_ch() channels
// (P32 = planes per 32 channels, P64 per 64):
//   IN(P32; channels 3.. zero)  FEA(P64)  RDB[3] x {x(P64) + dense x1..x4 (4 x P32)}
//   UP1(P64 @2x)  UP2(P64 @4x)  HR(P64 @4x)  OUT3 (planar [3][4H][4W] fp16; precise mode: fp32, and lo pair planes behind FEA's and RDB's)
// Concat never happens: conv k of a dense block reads planes [x | x1..x_{k-1}] in place and writes its
// 32 channels as plane(s) x_k.  Eltwise/BinaryOp/Interp are epilogue or staging-address variants.
int Engine::launch(const ConvArgs& a, int ci, const Plan::Batch& b, hipStream_t st)
{
    const PackedConv& c = convs[size_t(ci)];
    if (!launch_conv_flow(a, int(c.nt), num_cu, flow_flags, st))
        return fail(RSR_E_STATE, "conv3x3_flow has no variant for convolution " + std::to_string(ci));
    const double frac = b.items[a.lvl_out].empty() ? 1.0 : double(a.nitems) / double(b.items[a.lvl_out].size()); // split launches
    mark(1, 2.0 * 9.0 * c.cin * c.cout * b.px[a.lvl_out] * frac, 0, st, ci);
    return RSR_OK;
}

int Engine::run_network(const Plan::Batch& b, hipStream_t st, int nslots_used, const BatchIO* io, const RangeProbe* probe)
{
    const int nslots = std::min(nslots_used, b.nslots);
    const bool fused = io && conv_last_writes_image(io->c, io->out_fmt); // conv_last writes the images of io itself, else the planar OUT3 blob
    const int split_slot = io ? io->split_slot : 0;
    // the throttle event of a merged batch (Engine::submit_merged): behind the RDB that leaves about half an image's worth of network
    // ahead -- the time the next batch's launches take to enqueue
    // (a one-block model has three RDBs: the formula gives RDB 0 there; the clamp keeps it inside the loop at every depth)
    const int mid_rdb = (io && io->ev_mid) ? std::min(nrdb - 1, std::max(0, nrdb - 1 - std::max(2, nrdb / (2 * std::max(1, io->nimg))))) : -1;
    // the probe reads whole planes: they must hold exactly the pixels of the one tile, all of them computed, in fp16 storage
    if (probe && (b.nslots != 1 || b.dims.size() != 1 || ws_cap_px != (long long)b.dims[0].h * b.dims[0].w || b.trim4 || precise || fused))
        return fail(RSR_E_STATE, "range probe on a plan that is not one untrimmed tile in fp16 storage");
    const int pc = plane_ch(), P32 = 32 / pc, P64 = 64 / pc;
    // precise mode (ConvArgs::precise): the lo planes of a trunk tensor sit behind the hi / dense planes of its slot
    const long long fea_lo = layout().lo_off(kWsFea), rdb_lo = layout().lo_off(kWsRdb0);
    const char* blobp = static_cast<const char*>(blob.p);
    int ci = 0, rc = RSR_OK;
    auto base_args = [&](int lvl_in, int lvl_out) {
        ConvArgs a;
        std::memset(&a, 0, sizeof a);
        const PackedConv& c = convs[size_t(ci)];
        a.wpk16 = blobp + c.w16_off;
        a.waux = c.aux_off ? blobp + c.aux_off : nullptr;
        a.bias = reinterpret_cast<const float*>(blobp + c.b_off);
        a.lrelu = (c.act == 2);
        a.lvl_in = lvl_in;
        a.lvl_out = lvl_out;
        // Boustrophedon: every second conv walks the blocks backwards, so it starts on the tiles the previous conv
        // produced (and read) last -- those are still in the 256 MB Infinity Cache; walking forwards again would start
        // on the least recently used data.
        a.items = (alternate_order && (ci & 1) && b.d_items_rev[lvl_out]) ? b.d_items_rev[lvl_out] : b.d_items[lvl_out];
        a.nitems = int(b.items[lvl_out].size());
        if (nslots < b.nslots)
        { // the first `nslots` slots only: a prefix of the forward table = a suffix of the (plainly) reversed one
            const int n = a.nitems, cnt = b.item_start[lvl_out][size_t(nslots)];
            if (a.items == b.d_items_rev[lvl_out]) a.items = b.d_items_rev[lvl_out] + (n - cnt);
            a.nitems = cnt;
        }
        a.dims = b.d_dims;
        a.zeros = zeros.p;
        a.dbg = dbg;
        a.trace = (trace_conv == ci) ? static_cast<unsigned long long*>(trace_buf.p) : nullptr;
        a.s1 = a.s2 = 1.f;
        a.precise = precise ? 1 : 0;
        // x4.param order: ... RDB nrdb | trunk_conv nconv-5 | upconv1 -4 | upconv2 -3 | HRconv -2 | conv_last nconv-1
        const int kLast = nconv - 1, kUp1 = nconv - 4;
        a.margin = tail_margin(b.trim4, ci >= kUp1 ? kLast - ci : 4 + (kUp1 - 1 - ci));
        return a;
    };
    auto go = [&](ConvArgs& a) {
        if (rc == RSR_OK) rc = launch(a, ci, b, st);
        if (rc == RSR_OK && probe)
        { // what this convolution stored: its 2 * nt output planes of [H][W][16] halfs, or conv_last's planar [3][4h][4w] blob
            const long long npx = ((long long)b.dims[0].h * b.dims[0].w) << (2 * a.lvl_out);
            if (a.out_planar3) launch_range_probe(a.out_planar3, 0, 1, 3 * npx, probe->peak_bits + ci, probe->nonfinite + ci, st);
            else launch_range_probe(a.out16.base, a.out16.plane_stride, 2 * int(convs[size_t(ci)].nt), npx * kPlaneCh, probe->peak_bits + ci, probe->nonfinite + ci, st);
        }
        ci++;
    };
    const PlaneSrc fea = ws_planes(kWsFea);
    auto rdb_x = [&](int i) { return ws_planes(kWsRdb0 + i); };
    auto rdb_d = [&](int i, int k) { return ws_planes(kWsRdb0 + i, P64 + k * P32); };

    { // conv_first (x4.param:4): IN -> FEA
        ConvArgs a = base_args(0, 0);
        a.src0 = ws_planes(kWsIn);
        a.n0 = P32;
        a.out16 = fea;
        a.out_lo_off = fea_lo; // the stream starts here: fea keeps its rounding residue too
        go(a);
    }
    for (int j = 0; j < nrdb; j++)
    {
        const int bi = j % 3;
        const PlaneSrc xs = (j == 0) ? fea : rdb_x(bi);
        for (int k = 0; k < 4; k++)
        { // x_{k+1} = lrelu(conv([x, x1..xk]))   (x4.param:6,9,12,15)
            ConvArgs a = base_args(0, 0);
            a.src0 = xs; a.n0 = P64;
            a.src1 = rdb_d(bi, 0); a.n1 = k * P32;
            a.out16 = rdb_d(bi, k);
            go(a);
        }
        // x5 = conv([x, x1..x4]);  out = 0.2*x5 + x   (x4.param:17-18);  every third block additionally
        // out = 0.2*out + rrdb_in   (x4.param:47, Eltwise 0=1 -23301=2,0.2,1.0)
        ConvArgs a = base_args(0, 0);
        a.src0 = xs; a.n0 = P64;
        a.src1 = rdb_d(bi, 0); a.n1 = 4 * P32;
        a.s1 = 0.2f;
        a.res1 = xs; a.res1_kind = 1; a.res1_in_acc = 1; a.res1_coef = 5.f; // 1/0.2, exact in fp16
        a.lo1_off = (j == 0) ? fea_lo : rdb_lo;
        if (bi == 2)
        {
            a.s2 = 0.2f;
            a.res2 = (j == 2) ? fea : rdb_x(0); a.res2_kind = 1;
            a.lo2_off = (j == 2) ? fea_lo : rdb_lo;
        }
        a.out16 = rdb_x((j + 1) % 3);
        a.out_lo_off = rdb_lo;
        go(a);
        if (j == mid_rdb && rc == RSR_OK && hipEventRecord(io->ev_mid, st) != hipSuccess) rc = fail(RSR_E_DEVICE, "hipEventRecord failed");
    }
    { // trunk_conv + global skip: fea + conv(trunk)   (x4.param:994-995)
        ConvArgs a = base_args(0, 0);
        a.src0 = rdb_x(nrdb % 3); a.n0 = P64; // (nrdb = 3 nb: always rdb_x(0), where the last RDB of an RRDB leaves its result)
        a.res1 = fea; a.res1_kind = 1; a.s1 = 1.f;
        a.lo1_off = fea_lo;
        a.out16 = rdb_x(1); // (only upconv1 reads it: no lo planes)
        go(a);
    }
    const PlaneSrc up1 = ws_planes(kWsUp1), up2 = ws_planes(kWsUp2), hr = ws_planes(kWsHr);
    // The convs behind the trunk (upconv1 @2x, upconv2 / HRconv / conv_last @4x: ~11 % of the frame) can run per GROUP of
    // `tail_group_slots` slots (0 = the whole batch): a tile has 4x / 16x the blocks up there, so a few tiles fill the chip for
    // > 100 us per launch, and their 2 x 99 MB per tile of 4x intermediates are then read back from the 256 MB Infinity Cache
    // instead of HBM.  Measured on MI355X: <= 1.5 % on the 4x launches, a loss at 2x -- HBM bytes are not what bounds this
    // workload, so the default is off.  With split_slot > 0 a group boundary is forced there and `ev_half` is
    // recorded behind it: the caller starts downloading the finished output rows while the remaining groups are computed
    // (tiles are independent).  Items are sorted by slot, so a group is a contiguous range of the item tables (mirrored in
    // the reversed tables).
    const int ci_tail = ci;
    const int gsz = tail_group_slots > 0 ? tail_group_slots : nslots;
    for (int s0 = 0; s0 < nslots && rc == RSR_OK;)
    {
        int s1 = std::min(nslots, s0 + gsz);
        if (split_slot > s0 && split_slot < s1) s1 = split_slot;
        ci = ci_tail;
        auto sub = [&](ConvArgs& a, int lvl) {
            const int n = int(b.items[lvl].size());
            const int i0 = b.item_start[lvl][size_t(s0)], cnt = b.item_start[lvl][size_t(s1)] - i0;
            const bool rev = a.items >= b.d_items_rev[lvl] && a.items < b.d_items_rev[lvl] + n; // (base_args may have moved it to a suffix already)
            a.items = rev ? b.d_items_rev[lvl] + (n - i0 - cnt) : b.d_items[lvl] + i0;
            a.nitems = cnt;
        };
        { // nearest x2 + upconv1 + lrelu   (x4.param:996-997)
            ConvArgs a = base_args(0, 1);
            a.src0 = rdb_x(1); a.n0 = P64;
            a.out16 = up1;
            sub(a, 1);
            go(a);
        }
        { // nearest x2 + upconv2 + lrelu   (x4.param:998-999)
            ConvArgs a = base_args(1, 2);
            a.src0 = up1; a.n0 = P64;
            a.out16 = up2;
            sub(a, 2);
            go(a);
        }
        { // HRconv + lrelu   (x4.param:1000)
            ConvArgs a = base_args(2, 2);
            a.src0 = up2; a.n0 = P64;
            a.out16 = hr;
            sub(a, 2);
            go(a);
        }
        { // conv_last 64 -> 3   (x4.param:1001), planar fp16 output = the reference's `output` blob
            ConvArgs a = base_args(2, 2);
            a.src0 = hr; a.n0 = P64;
            if (fused)
            { // non-TTA RGB with conv3x3_flow: conv_last applies realsr_postproc.comp itself and writes the image(s): uint8 HWC, or --
              // out_fmt -- planar fp16 / fp32, through each image's row and plane pitch
                for (int i = 0; i < io->nimg && i < kMaxMerge; i++)
                {
                    a.out_u8s[i] = static_cast<uint8_t*>(io->out[i]);
                    a.out_pitch[i] = int(io->out_pitch[i]);
                    a.out_plane[i] = io->out_plane[i];
                }
                a.out_u8 = a.out_u8s[0];
                a.out_fmt = io->out_fmt;
                a.out_u8_w = io->w[0] * scale;
                a.out_u8_crop = prepadding * scale;
                a.out_u8_bgr = bgr ? 1 : 0;
            }
            else
            {
                a.out_planar3 = ws[kWsOut3].p;
                a.planar3_slot_stride = layout().slot_stride(kWsOut3);
            }
            sub(a, 2);
            go(a);
        }
        if (s1 == split_slot && io->ev_half && rc == RSR_OK && hipEventRecord(io->ev_half, st) != hipSuccess)
            rc = fail(RSR_E_DEVICE, "hipEventRecord failed");
        s0 = s1;
    }
    return rc;
}

// ---- process ----------------------------------------------------------------------------------
// enqueue preproc -> network -> postproc for every tile batch of the image(s) of io on `st` (mu held)
int Engine::enqueue_images(BatchIO io, int tile0, int tile1, int plan_nimg, size_t* half_rows, hipStream_t st)
{
    const int nimg = io.nimg, w = io.w[0], h = io.h[0], c = io.c;
    if (io.os != out_ratio) return fail(RSR_E_STATE, "context parameters changed while the call was in flight"); // (the images of io are sized for io.os)
    const bool merged = plan_nimg > 0; // (every caller of a merged batch reports the progress of its own image: process_host)
    if (plan_nimg < nimg) plan_nimg = nimg;
    const long long kBytesPerPx = bytes_per_px();
    if (half_rows) *half_rows = 0;
    Plan* planp = nullptr;
    int xtiles = 0;
    const int all_tiles = tile_count(w, h, &xtiles);
    if (tile1 < 0) tile1 = all_tiles;
    int rc;
    // A clamp left behind by a transient allocation failure (another process held the memory for a moment) must not halve the
    // batches for ever: a NEW call that finds the device able to give twice the clamped size again plans without it (never inside
    // the retry loop below, which would then oscillate).  But a PERSISTENT cause (fragmentation, hipMemGetInfo overstating what one
    // hipMalloc can get) makes that test true on every call -- each frame would re-plan at full size, fail, drain the stream, free
    // and rebuild the workspace.  So an un-clamp attempt is made at once only when the device reports clearly more room
    // than it did at the moment of the failure (x 1.25), and otherwise at most once per `clamp_backoff` calls, the back-off doubling
    // with every attempt that fails again.  Plans are keyed by the clamp.
    bool unclamp_attempt = false;
    if (ws_clamp_bytes >= 0)
    {
        const long long avail = device_avail(w, h, c);
        if (avail >= 2 * ws_clamp_bytes)
        {
            const bool grown = clamp_fail_avail < 0 || avail >= clamp_fail_avail + clamp_fail_avail / 4;
            if (grown || --clamp_calls_left <= 0)
            {
                clamp_saved = ws_clamp_bytes;
                ws_clamp_bytes = -1;
                unclamp_attempt = true;
            }
        }
    }
    for (;;)
    {
        rc = get_plan(w, h, c, tile0, tile1, plan_nimg, planp);
        if (rc != RSR_OK) return rc;
        // (a merged batch narrower than its plan still gets the plan's workspace: growing it image by image as wider batches form
        // would re-allocate and clear gigabytes a dozen times)
        rc = ensure_workspace(planp->slots_per_batch, planp->cap_px, st);
        if (rc != RSR_E_NOMEM) break;
        // The batch does not fit (a shared or partly used GPU): halve it and plan again, down to one tile (x8 under TTA).
        const int per = tta ? 8 : 1;
        if (planp->slots_per_batch <= per) return rc;
        const std::string why = last_error();
        long long half_slots = std::max<long long>(per, (planp->slots_per_batch / 2) / per * per);
        const long long failed_bytes = (long long)planp->slots_per_batch * planp->cap_px * kBytesPerPx;
        clamp_fail_avail = device_avail(w, h, c);
        if (unclamp_attempt && clamp_saved > 0 && clamp_saved < failed_bytes)
        { // the clamp was right after all: back to it (not to half of the full size), and wait longer before the next try
            half_slots = std::max<long long>(per, clamp_saved / (planp->cap_px * kBytesPerPx) / per * per);
            clamp_backoff = std::min(clamp_backoff * 2, 1024);
        }
        unclamp_attempt = false;
        clamp_calls_left = clamp_backoff;
        ws_clamp_bytes = half_slots * planp->cap_px * kBytesPerPx;
        std::fprintf(stderr, "realsr-hip: workspace of %d tile slots (%.1f GB) does not fit device %d (%s); batches of %lld slots, next attempt at full size "
                             "after %d calls or when the device reports > %.1f GB available\n",
                     planp->slots_per_batch, double(failed_bytes) / 1e9, device, why.c_str(), half_slots, clamp_backoff,
                     double(clamp_fail_avail) * 1.25 / 1e9);
        free_workspace(st); // partly grown buffers go back first; the stream is drained, so the plan's tables are idle too
        if (planp->d_tables) (void)hipFree(planp->d_tables);
        plans.pop_front(); // get_plan put it in front
    }
    if (rc == RSR_OK && unclamp_attempt) { clamp_backoff = 4; clamp_fail_avail = -1; } // the full size fits again: forget the history
    if (rc != RSR_OK) return rc;
    const Plan& plan = *planp;
    mark_begin(st);
    int done = 0, total = 0;
    for (const Plan::Batch& b : plan.batches) total += b.ntiles;
    const int tiles_wanted = (tile1 - tile0) * nimg; // the tiles of the first nimg images (all of the plan's unless the batch is narrower)
    io.out_row0 = plan.out_row0;
    const hipEvent_t ev_mid = io.ev_mid; // of the last batch
    for (const Plan::Batch& b : plan.batches)
    {
        const int ntiles = std::min(b.ntiles, tiles_wanted - b.tile0); // of this batch
        if (ntiles <= 0) break;
        // host calls: split the 4x tail at a tile-row boundary so that the first output rows can travel while the rest is computed
        io.split_slot = 0;
        if (conv_last_writes_image(c, io.out_fmt) && nimg == 1 && io.ev_half && half_rows && plan.batches.size() == 1 && !profiling && !(dbg & kDbgNoSplitTail))
        {
            const int xt = xtiles, yt = b.ntiles / xt;
            if (yt >= 2 && b.ntiles == xt * yt && plan.key.tile0 % xt == 0)
            {
                io.split_slot = xt * (yt / 2);
                *half_rows = size_t(b.tiles[size_t(io.split_slot)].out_y - b.tiles[0].out_y); // output rows finished at ev_half
            }
        }
        io.ev_mid = b.tile0 + b.ntiles >= tiles_wanted ? ev_mid : nullptr;
        rc = launch_batch(b, plan.max_tw, plan.max_th, ntiles, st, io);
        if (rc != RSR_OK) return rc;
        if (progress && !merged) // one call per TILE, like the reference's line per tile (realsr.cpp:481), issued when the tile's batch is enqueued
            for (int i = 1; i <= b.ntiles; i++) progress(done + i, total, progress_user); // (a merged batch: every caller reports its own image)
        done += b.ntiles;
    }
    HIP_TRY(hipGetLastError());
    if (profiling)
    {
        collect_profile(st);
        prof.calls++;
        for (const Plan::Batch& b : plan.batches) prof.tiles += b.nslots;
    }
    return RSR_OK;
}

// preproc -> network -> postproc of the first `ntiles` tiles of one tile batch on `st` (mu held; the workspace is laid out for the batch's
// slots).  The images of the batch may differ in size (io.w / io.h): every tile carries the index of its image.
int Engine::launch_batch(const Plan::Batch& b, int max_tw, int max_th, int ntiles, hipStream_t st, const BatchIO& io)
{
    const int per = tta ? 8 : 1, c = io.c;
    const int variant = (dbg & kDbgPrePostVar1) ? 1 : ((dbg & kDbgPrePostVar2) ? 2 : 0);
    PreArgs pa;
    std::memset(&pa, 0, sizeof pa);
    PostArgs po;
    std::memset(&po, 0, sizeof po);
    for (int i = 0; i < io.nimg; i++)
    {
        pa.imgs[i] = po.in_imgs[i] = static_cast<const uint8_t*>(io.in[i]);
        pa.ws[i] = io.w[i];
        pa.hs[i] = io.h[i];
        pa.pitch[i] = po.in_pitch[i] = int(io.in_pitch[i]);
        pa.plane[i] = io.in_plane[i];
        po.outs[i] = static_cast<uint8_t*>(io.out[i]);
        po.out_pitch[i] = int(io.out_pitch[i]);
        po.out_plane[i] = io.out_plane[i];
    }
    pa.nimgs = io.nimg;
    pa.fmt = io.in_fmt;
    pa.c = c;
    pa.tiles = b.d_tiles;
    pa.ntiles = ntiles;
    pa.tta = tta;
    pa.in_plane = const_cast<void*>(ws_planes(kWsIn).base);
    pa.slot_stride = ws_planes(kWsIn).slot_stride;
    pa.bgr = bgr ? 1 : 0;
    pa.plane_ch = plane_ch();
    pa.variant = variant;
    if (const int bits = pix_fmt(io.in_fmt).bits; bits && !yuv_coef(yuv_matrix, yuv_range, bits, &pa.yuv)) return fail(RSR_E_STATE, "no such YUV matrix / range");
    if (const int bits = pix_fmt(io.out_fmt).bits; bits && !yuv_coef(yuv_matrix, yuv_range, bits, &po.yuv)) return fail(RSR_E_STATE, "no such YUV matrix / range");
    pa.siting = po.siting = yuv_siting;
    // Option "alpha_net" (include/realsr_hip.h): an RGBA batch walks the network twice over the same tables and workspace -- the colour pass
    // as ever, its post launch writing the bicubic alpha too, then the alpha pass below, whose post launch overwrites sample 3 alone.  The
    // throttle event of a merged batch belongs to the pass that runs last.
    // Option "alpha_adaptive" on top: the scan goes in front of the colour pass, its bytes are read behind it (the GPU has a whole colour
    // pass queued while the host waits), and the alpha pass runs on the tiles whose alpha varies.
    const bool two_pass = alpha_net && c == 4, adaptive = two_pass && alpha_adaptive;
    int rc;
    if (adaptive && (rc = enqueue_flat_scan(b, max_th, ntiles, st, io)) != RSR_OK) return rc;
    launch_preproc_tiles(pa, max_tw, max_th, st);
    mark(0, 0, b.px[0] / per * BatchIO::image_px_bytes(io.in_fmt, c) + b.px[0] * 64, st);
    if (two_pass)
    {
        BatchIO cio = io;
        cio.ev_mid = nullptr;
        rc = run_network(b, st, ntiles * per, &cio, nullptr);
    }
    else
        rc = run_network(b, st, ntiles * per, &io, nullptr);
    if (rc != RSR_OK || conv_last_writes_image(c, io.out_fmt)) return rc;
    po.planar3 = ws[kWsOut3].p;
    po.f32 = precise ? 1 : 0;
    po.slot_stride = layout().slot_stride(kWsOut3);
    po.tiles = b.d_tiles;
    po.ntiles = ntiles;
    po.tta = tta;
    po.crop = prepadding * scale;
    po.nimgs = io.nimg;
    po.out_fmt = io.out_fmt;
    po.in_fmt = io.in_fmt;
    po.c = c;
    po.out_row0 = io.out_row0;
    po.box = io.os.is_box() ? 4 / io.os.nx : 1;
    po.num = io.os.nx;
    po.den = io.os.dx;
    po.num_y = io.os.ny;
    po.den_y = io.os.dy;
    po.area_norm = float(1.0 / (16.0 * io.os.dx * io.os.dy));
    po.tilesize = tilesize;
    po.bgr = bgr ? 1 : 0;
    po.variant = variant;
    po.dither = dither && io.out_fmt != kFmtF16 && io.out_fmt != kFmtF32 ? 1 : 0; // (the alpha pass below does not look at it)
    launch_postproc_tiles(po, (max_tw - 2 * prepadding) * scale, (max_th - 2 * prepadding) * scale, st);
    mark(2, 0, b.px[2] / per * (6.0 * per + BatchIO::image_px_bytes(io.out_fmt, c) * io.os.nx * io.os.ny / (16.0 * io.os.dx * io.os.dy)), st);
    if (!two_pass) return RSR_OK;
    // The tiles of the alpha pass: all of the batch on its own tables, or with "alpha_adaptive" those the scan marked.
    const Plan::Batch* ab = &b;
    Plan::Batch sub;
    if (adaptive)
    {
        const auto t_wait = std::chrono::steady_clock::now();
        if (flat_ring.ev[flat_ring.k]) HIP_TRY(hipEventSynchronize(flat_ring.ev[flat_ring.k])); // (no event: release waited for the stream)
        alpha_wait_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_wait).count();
        const char* const varies = flat_ring.host();
        std::vector<int> run;
        for (int i = 0; i < ntiles; i++)
            if (varies[i]) run.push_back(i);
        alpha_tiles_flat += ntiles - int(run.size());
        if (run.empty())
        { // no alpha pass: the colour pass ran last
            if (io.ev_mid && hipEventRecord(io.ev_mid, st) != hipSuccess) return fail(RSR_E_DEVICE, "hipEventRecord failed");
            return RSR_OK;
        }
        if (int(run.size()) < ntiles)
        { // The varying tiles as a batch of their own: each keeps its out_x / out_y / img and gets a compact slot0, so the pass uses a subset
          // of the batch's slots in the same workspace.  The tables travel like a masked call's: pinned image, one copy on the call's stream.
            const size_t table_bytes = fill_batch(sub, b.tile0, int(run.size()), [&](int i) { return b.tiles[size_t(run[size_t(i)])]; }, tta != 0,
                                                  prepadding * scale, trim_tail, fold_cols, io.out_row0);
            if ((rc = alpha_ring.acquire(table_bytes, true)) != RSR_OK) return rc;
            char *d = alpha_ring.dev(), *hs = alpha_ring.host();
            (void)upload_batch(sub, d, xcd_order, &hs);
            HIP_TRY(hipMemcpyAsync(alpha_ring.dev(), alpha_ring.host(), table_bytes, hipMemcpyHostToDevice, st));
            ab = &sub;
        }
    }
    const int an = ab == &b ? ntiles : ab->ntiles;
    // The alpha pass: the alpha sample of every source pixel into the three input planes (the gray image G of the header), the network,
    // and the mean of the three results into sample 3.  IN and OUT3 are free again: the stream has the colour pass's launches in front.
    pa.alpha_src = 1;
    pa.tiles = po.tiles = ab->d_tiles;
    pa.ntiles = po.ntiles = an;
    launch_preproc_tiles(pa, max_tw, max_th, st);
    mark(0, 0, ab->px[0] / per * (BatchIO::image_px_bytes(io.in_fmt, c) / c) + ab->px[0] * 64, st);
    rc = run_network(*ab, st, an * per, &io, nullptr);
    if (rc == RSR_OK)
    {
        po.alpha_dst = 1;
        launch_postproc_tiles(po, (max_tw - 2 * prepadding) * scale, (max_th - 2 * prepadding) * scale, st);
        mark(2, 0, ab->px[2] / per * (6.0 * per + BatchIO::image_px_bytes(io.out_fmt, c) / c * io.os.nx * io.os.ny / (16.0 * io.os.dx * io.os.dy)), st);
        alpha_tiles += an;
    }
    if (ab == &sub) alpha_ring.release(st); // (also behind a pass that failed to launch: what it did enqueue reads the tables)
    return rc;
}

// The scan of option "alpha_adaptive" (kernels.h FlatArgs) for the first ntiles tiles of b, in front of whatever the caller enqueues next:
// memset, kernel, and the copy of the ntiles bytes into the pinned image of flat_ring's next slot, whose event is recorded behind the
// copy.  Under profiling the three count as one segment of the preprocessing class.
int Engine::enqueue_flat_scan(const Plan::Batch& b, int max_th, int ntiles, hipStream_t st, const BatchIO& io)
{
    if (const int rc = flat_ring.acquire(al256(size_t(ntiles)), true)) return rc;
    FlatArgs fa;
    std::memset(&fa, 0, sizeof fa);
    for (int i = 0; i < io.nimg; i++)
    {
        fa.imgs[i] = static_cast<const uint8_t*>(io.in[i]);
        fa.ws[i] = io.w[i];
        fa.hs[i] = io.h[i];
        fa.pitch[i] = io.in_pitch[i];
    }
    fa.tiles = b.d_tiles;
    fa.ntiles = ntiles;
    fa.u16 = io.in_fmt == kFmtU16 ? 1 : 0;
    fa.flags = reinterpret_cast<uint8_t*>(flat_ring.dev());
    const hipError_t e = launch_alpha_flat_tiles(fa, max_th, st);
    if (e != hipSuccess) return fail(RSR_E_DEVICE, std::string("alpha_flat_tiles: ") + hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(flat_ring.host(), flat_ring.dev(), size_t(ntiles), hipMemcpyDeviceToHost, st));
    flat_ring.release(st);
    mark(0, 0, b.px[0] / (tta ? 8 : 1) * BatchIO::image_px_bytes(io.in_fmt, io.c), st);
    return RSR_OK;
}

// A merged batch of images that DIFFER in size (a directory of thumbnails, sprites, crops ...): no cached plan can serve it -- the
// tile and work-item tables are built here, for exactly these images, and uploaded into one of three rotating device buffers (the
// throttle of submit_merged leaves at most the previous batch in flight when the next one is formed; the buffer's event makes sure).
// All slots get the capacity of a full tile (merged_cap_px), whatever the images.  mu held.
int Engine::enqueue_mixed(MergeReq* const* g, int n, hipStream_t st, hipEvent_t ev_mid)
{
    const int T = tilesize, P = prepadding, c = g[0]->c;
    std::vector<BaseTile> all;
    long long cap = 0;
    int mtw = 0, mth = 0;
    for (int i = 0; i < n; i++) image_tiles(g[i]->w, g[i]->h, T, P, scale, 0, tile_count(g[i]->w, g[i]->h), i, all, cap, mtw, mth);
    cap = merged_cap_px();
    int rc = check_tile_px(cap);
    if (rc != RSR_OK) return rc;
    const long long need = (long long)all.size() * (tta ? 8 : 1) * cap * bytes_per_px();
    const long long avail = device_avail(g[0]->w, g[0]->h, c);
    if (need > max_workspace_mb * 1024 * 1024 || (avail >= 0 && need > avail)) return fail(RSR_E_NOMEM, "merged batch exceeds the workspace budget");
    Plan::Batch b;
    const size_t table_bytes = fill_batch(b, 0, int(all.size()), [&](int i) { return all[size_t(i)]; }, tta != 0, P * scale, trim_tail, fold_cols, 0);
    HIP_TRY(hipSetDevice(device));
    if ((rc = mix_ring.acquire(table_bytes, false)) != RSR_OK) return rc;
    char* d = mix_ring.dev();
    const hipError_t e = upload_batch(b, d, false);
    if (e != hipSuccess) return fail(RSR_E_DEVICE, std::string("merged batch table upload: ") + hipGetErrorString(e));
    if ((rc = ensure_workspace(b.nslots, cap, st)) != RSR_OK) return rc;
    BatchIO io(g, n);
    io.ev_mid = ev_mid;
    rc = launch_batch(b, mtw, mth, b.ntiles, st, io);
    if (rc != RSR_OK) return rc;
    mix_ring.release(st);
    HIP_TRY(hipGetLastError());
    return RSR_OK;
}

// The tiles `sel` of the one image of io -- a masked call (include/realsr_hip.h rsr_process_device_masked) -- as tile batches built here, the way
// enqueue_mixed builds its batch: no cached plan serves an arbitrary tile list.  Every BaseTile keeps the image's own out_x / out_y, so exactly
// the rectangles of the selected tiles are written.  The slots get the capacity of the FRAME's largest tile, whatever is selected: the plan of
// the plain call (get_plan, nimg == 1) lays the workspace out for that capacity too, so plain and masked calls on one geometry alternate
// without moving a guard.  The selected tiles are cut into batches by get_plan's budget arithmetic; an allocation that fails all the same
// halves the batch of THIS call and leaves no clamp behind (the next plain call plans as if nothing had happened: if the memory is still
// short it finds out, and clamps, for itself).  All tables of the call go into one of three rotating device buffers, each guarded by the
// event behind the last launch that reads it: the host waits only when the call three masked calls back is still in flight.  The tables
// travel from a pinned image of the same rotation with one asynchronous copy on `st`.  mu held.
int Engine::enqueue_masked(BatchIO io, const std::vector<int>& sel, hipStream_t st)
{
    return enqueue_sequence(io, sel, std::vector<PropRect>(), st, masked_batches, &masked_table_us);
}

// The general form (include/realsr_hip.h rsr_process_device_sequence): the io.nimg <= kMaxMerge images have ONE geometry, and sel names
// (image, tile) pairs, frame-major, as image * tiles_per_image + tile.  BaseTile::img carries the image into the pre- and post-processing
// launches and, through item_pad2, into conv_last where it writes the image itself, as in enqueue_mixed; nothing else of the tables knows
// how many images there are, so with one image this IS the masked call.  `rects`, when there are any, are copied by ONE launch of
// propagate_rects behind the last batch: their table rides behind the tile tables in the same buffer and the same asynchronous copy, and
// the event that guards the buffer is recorded behind that launch.  sel may be empty (nothing changed in any frame): then no workspace is
// touched and only the copy runs.  batches_stat / table_us: the counters of the caller's kind of call.
int Engine::enqueue_sequence(BatchIO io, const std::vector<int>& sel, const std::vector<PropRect>& rects, hipStream_t st, long long& batches_stat, double* table_us)
{
    const int T = tilesize, P = prepadding, per = tta ? 8 : 1, w = io.w[0], h = io.h[0], c = io.c;
    const int total = tile_count(w, h), nsel = int(sel.size());
    std::vector<BaseTile> all;
    long long cap = 0;
    int mtw = 0, mth = 0;
    image_tiles(w, h, T, P, scale, 0, total, 0, all, cap, mtw, mth);
    int rc = check_tile_px(cap);
    if (rc != RSR_OK) return rc;
    int tiles_per_batch = std::max(1, int(std::min<long long>((long long)nsel * per, budget_slots(cap, w, h, c))) / per);
    HIP_TRY(hipSetDevice(device));
    while (nsel && (rc = ensure_workspace(tiles_per_batch * per, cap, st)) == RSR_E_NOMEM && tiles_per_batch > 1)
    {
        free_workspace(st); // partly grown buffers go back first
        tiles_per_batch /= 2;
    }
    if (rc != RSR_OK) return rc;
    const auto t_tab = std::chrono::steady_clock::now();
    std::vector<Plan::Batch> batches;
    size_t table_bytes = 0;
    mtw = mth = 0; // of the selected tiles: the grids of the pre- and post-processing launches
    for (int t0 = 0; t0 < nsel; t0 += tiles_per_batch)
    {
        Plan::Batch b;
        auto tile_at = [&](int i) {
            BaseTile t = all[size_t(sel[size_t(t0 + i)] % total)];
            t.img = sel[size_t(t0 + i)] / total;
            mtw = std::max(mtw, t.tw), mth = std::max(mth, t.th);
            return t;
        };
        table_bytes += fill_batch(b, t0, std::min(nsel - t0, tiles_per_batch), tile_at, tta != 0, P * scale, trim_tail, fold_cols, 0);
        batches.push_back(std::move(b));
    }
    const size_t rect_at = table_bytes, rect_bytes = rects.size() * sizeof(PropRect);
    table_bytes += al256(rect_bytes);
    if ((rc = mask_ring.acquire(table_bytes, true)) != RSR_OK) return rc;
    char *d = mask_ring.dev(), *hs = mask_ring.host();
    for (Plan::Batch& b : batches) (void)upload_batch(b, d, xcd_order, &hs);
    if (rect_bytes) std::memcpy(mask_ring.host() + rect_at, rects.data(), rect_bytes);
    // on the call's own stream, in front of its launches: no other stream is involved, whatever kind the caller's is
    HIP_TRY(hipMemcpyAsync(mask_ring.dev(), mask_ring.host(), table_bytes, hipMemcpyHostToDevice, st));
    if (table_us) *table_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_tab).count();
    mark_begin(st);
    io.out_row0 = 0;
    io.split_slot = 0;
    io.ev_mid = nullptr;
    int done = 0;
    long long slots = 0;
    for (const Plan::Batch& b : batches)
    {
        rc = launch_batch(b, mtw, mth, b.ntiles, st, io);
        if (rc != RSR_OK) break;
        if (progress)
            for (int i = 1; i <= b.ntiles; i++) progress(done + i, nsel, progress_user);
        done += b.ntiles;
        slots += b.nslots;
        batches_stat++;
    }
    // The copies: every source is a rectangle some batch above computed, or the previous output, never another copy's destination, so
    // one launch in any order does.  Also behind a LATER batch that failed to launch (what ran is then propagated as usual); not when
    // the first one failed: nothing was computed, and nothing is written.
    if (rect_bytes && (done > 0 || nsel == 0))
    {
        int max_rows = 0;
        double bytes = 0;
        for (const PropRect& r : rects) max_rows = std::max(max_rows, r.rows), bytes += double(r.width) * r.rows;
        const hipError_t e = launch_propagate_rects(reinterpret_cast<const PropRect*>(mask_ring.dev() + rect_at), int(rects.size()), max_rows, st);
        if (e != hipSuccess && rc == RSR_OK) rc = fail(RSR_E_DEVICE, std::string("propagate_rects: ") + hipGetErrorString(e));
        mark(2, 0, 2 * bytes, st);
    }
    // (also behind a batch that failed to launch: the copy and the batches in front of it read the buffers)
    mask_ring.release(st);
    if (rc != RSR_OK) return rc;
    HIP_TRY(hipGetLastError());
    if (profiling)
    {
        collect_profile(st);
        prof.calls++;
        prof.tiles += slots;
    }
    return RSR_OK;
}

// ---- the call skeleton of the device entry points (engine.h) ------------------------------------------------------------------
int Engine::admit(int out_fmt, int w, int h, OutRatio os, bool enter) const
{
    if (enter)
    {
        if (!loaded) return fail(RSR_E_STATE, "process before load");
        if (scale != 4) return fail(RSR_E_ARG, "only scale 4 is supported (main.cpp:533-537)");
        if (out_ratio != os) return fail(RSR_E_STATE, "context parameters changed while the call was in flight");
    }
    if (w < 1 || h < 1) return RSR_OK;
    return out_admit(pix_fmt(out_fmt), w, h, tilesize, os, kWhoEngine);
}

template <class Body> int Engine::on_stream(std::unique_lock<std::mutex>& lk, hipStream_t user_stream, bool sync, Body body)
{
    HIP_TRY(hipSetDevice(device));
    // Idle: nothing of any earlier call is pending on the compute stream -- work an earlier direct call put on ITS caller's stream included:
    // the compute stream was made to wait for it, below.  All other network kernels run on the compute stream (there is one workspace).
    const bool direct = user_stream && hipStreamQuery(stream) == hipSuccess;
    (void)hipGetLastError(); // (hipErrorNotReady is not an error)
    if (user_stream && !direct)
    {
        hipEvent_t e = take_event();
        if (!e) return fail(RSR_E_DEVICE, "hipEventCreate failed");
        HIP_TRY(hipEventRecord(e, user_stream));
        HIP_TRY(hipStreamWaitEvent(stream, e, 0));
        give_event(e);
    }
    bool enqueued = false;
    const int rc = body(direct ? user_stream : stream, enqueued);
    if (direct)
    { // whatever the compute stream gets next uses the same workspace: it waits for this call's last kernel
        hipEvent_t e = take_event();
        if (!e || hipEventRecord(e, user_stream) != hipSuccess || hipStreamWaitEvent(stream, e, 0) != hipSuccess)
        { // cannot order the compute stream behind it: fall back to waiting here
            (void)hipGetLastError();
            (void)hipStreamSynchronize(user_stream);
        }
        give_event(e);
        if (rc == RSR_OK) device_direct++;
        return rc;
    }
    if (!enqueued || !(user_stream || sync)) return rc;
    hipEvent_t done = take_event();
    if (!done) return fail(RSR_E_DEVICE, "hipEventCreate failed");
    HIP_TRY(hipEventRecord(done, stream));
    if (user_stream) HIP_TRY(hipStreamWaitEvent(user_stream, done, 0));
    hipError_t e = hipSuccess;
    if (!user_stream)
    { // wait outside the lock: other calls may enqueue behind this one meanwhile
        lk.unlock();
        e = hipEventSynchronize(done);
        lk.lock();
    }
    give_event(done);
    if (e != hipSuccess) return fail(RSR_E_DEVICE, std::string("hipEventSynchronize: ") + hipGetErrorString(e));
    return rc;
}

int Engine::process_device(const void* d_in, int w, int h, int c, void* d_out, hipStream_t user_stream, bool sync, int in_fmt, int out_fmt)
{
    if (!d_in || !d_out || w < 1 || h < 1 || (c != 3 && c != 4)) return fail(RSR_E_ARG, "bad image arguments");
    const PixFmt fin = pix_fmt(in_fmt, c), fout = pix_fmt(out_fmt, c);
    for (const PixFmt* f : {&fin, &fout})
        if (const int rc = fmt_check(*f, c, "the planar float and the YUV formats come with c == 3 only")) return rc;
    if (const int rc = parity_check(fin, w, h, "input")) return rc;
    if ((fin.bits > 8 && (reinterpret_cast<uintptr_t>(d_in) & 1)) || (fout.bits > 8 && (reinterpret_cast<uintptr_t>(d_out) & 1)))
        return fail(RSR_E_ARG, "P010 / P210 / YUV444P10 data is not aligned to its 16-bit samples");
    if ((fin.sample > 1 && (reinterpret_cast<uintptr_t>(d_in) & 1)) || (fout.sample > 1 && (reinterpret_cast<uintptr_t>(d_out) & 1)))
        return fail(RSR_E_ARG, "16-bit RGB(A) data is not aligned to its samples");
    const bool u8 = in_fmt == RSR_FMT_U8_HWC && out_fmt == RSR_FMT_U8_HWC;
    if (!user_stream && sync && u8) // (a call with a float image on either side is not merged: it runs as a batch of its own, below)
    { // a small image: merged with whatever other calls hand in meanwhile (Engine::submit_merged)
        int T = 0, width = 1;
        OutRatio os;
        long long items = 0;
        { // (the engine's settings are read under its lock: another thread may be in rsr_set_params / rsr_set_option)
            std::lock_guard<std::mutex> lk(mu);
            if (!loaded) return fail(RSR_E_STATE, "process before load");
            if (scale != 4) return fail(RSR_E_ARG, "only scale 4 is supported (main.cpp:533-537)");
            T = tilesize;
            os = out_ratio;
            if (const int rc = out_admit(fout, w, h, T, os, kWhoEngine)) return rc;
            width = merge_width(w, h, c);
            if (width > 1) items = image_items(w, h, merge_target_items);
        }
        if (width > 1)
        {
            MergeReq r;
            r.d_in = d_in; r.d_out = d_out; r.w = w; r.h = h; r.c = c; r.T = T;
            r.os = os;
            r.items = items;
            r.width = width;
            const int rc = submit_merged(r);
            if (rc != RSR_OK) return rc;
            const hipError_t e = hipEventSynchronize(r.ev_done);
            {
                std::lock_guard<std::mutex> lk(mu);
                give_event(r.ev_done);
            }
            if (e != hipSuccess) return fail(RSR_E_DEVICE, std::string("hipEventSynchronize: ") + hipGetErrorString(e));
            return RSR_OK;
        }
    }
    std::unique_lock<std::mutex> lk(mu);
    if (const int rc = admit(out_fmt, w, h, out_ratio, true)) return rc;
    return on_stream(lk, user_stream, sync, [&](hipStream_t st, bool& enqueued) {
        enqueued = true; // (enqueue_images does not say how far it got: a failing call is ordered behind whatever it did enqueue)
        return enqueue_images(BatchIO(d_in, d_out, w, h, c, in_fmt, out_fmt, out_ratio), 0, -1, 0, nullptr, st);
    });
}

// ---- YUV surfaces: 4:2:0 and 4:2:2 semi-planar (RSR_FMT_NV12 / P010, NV16 / P210), 4:4:4 planar (RSR_FMT_YUV444P / YUV444P10) ------
// Every constant is computed in double from Kr and Kb and rounded ONCE to fp32 (include/realsr_hip.h "yuv_matrix"; tests/yuv_ref.py writes
// the same expressions).
bool yuv_coef(int matrix, int range, int bits, YuvCoef* out)
{
    double kr, kb;
    if (matrix == 709) kr = 0.2126, kb = 0.0722;
    else if (matrix == 601) kr = 0.299, kb = 0.114;
    else if (matrix == 2020) kr = 0.2627, kb = 0.0593;
    else return false;
    if ((range != 0 && range != 1) || (bits != 8 && bits != 10)) return false;
    const double kg = 1.0 - kr - kb, k = double(1 << (bits - 8)), top = double((1 << bits) - 1);
    const double yoff = range ? 0.0 : 16.0 * k, coff = double(1 << (bits - 1));
    const double yscale = range ? top : 219.0 * k, cscale = range ? top : 224.0 * k;
    YuvCoef c;
    c.yoff = float(yoff), c.ys = float(1.0 / yscale), c.coff = float(coff), c.cs = float(1.0 / cscale);
    c.rv = float(2.0 * (1.0 - kr)), c.gu = float(2.0 * kb * (1.0 - kb) / kg), c.gv = float(2.0 * kr * (1.0 - kr) / kg), c.bu = float(2.0 * (1.0 - kb));
    c.kr = float(kr), c.kg = float(kg), c.kb = float(kb);
    c.yscale = float(yscale), c.yadd = float(yoff) + 0.5f, c.cscale = float(cscale), c.cadd = float(coff) + 0.5f;
    c.icb = float(1.0 / (2.0 * (1.0 - kb))), c.icr = float(1.0 / (2.0 * (1.0 - kr))), c.maxcode = float(top);
    *out = c;
    return true;
}

// ---- rational output scales (rsr_set_out_ratio, rsr_set_out_ratio_xy) ---------------------------------------------------------------------
// num / den in lowest terms when den <= max_den and 1 <= num / den <= 4
static bool axis_reduce(int num, int den, int max_den, int* n_out, int* d_out)
{
    if (num < 1 || den < 1) return false;
    int a = num, b = den;
    while (b) { const int t = a % b; a = b; b = t; }
    const int n = num / a, d = den / a;
    if (d > max_den || n < d || n > 4 * d) return false;
    *n_out = n, *d_out = d;
    return true;
}

bool out_ratio_reduce(int num, int den, OutRatio* out)
{
    int n, d;
    if (!axis_reduce(num, den, 4, &n, &d)) return false;
    *out = OutRatio(n, d);
    return true;
}

bool out_ratio_reduce_xy(int num_x, int den_x, int num_y, int den_y, OutRatio* out)
{
    int nx, dx, ny, dy;
    if (!axis_reduce(num_x, den_x, 8, &nx, &dx) || !axis_reduce(num_y, den_y, 8, &ny, &dy)) return false;
    *out = OutRatio(nx, dx, ny, dy);
    return true;
}

// ---- the rules of a pixel format (engine.h; kernels.h PixFmt) ----------------------------------------------------------------------------
int fmt_check(const PixFmt& f, int c, const char* c_text)
{
    if (!f.known()) return Engine::fail(RSR_E_ARG, "unknown pixel format");
    return f.takes(c) ? RSR_OK : Engine::fail(RSR_E_ARG, c_text);
}

int parity_check(const PixFmt& f, int w, int h, const char* noun)
{
    if (!f.odd(w, h)) return RSR_OK;
    return Engine::fail(RSR_E_ARG, std::string("a ") + f.family + " " + noun + " needs an even width" + (f.csy ? " and height" : ""));
}

// The refusals of out_admit, worded as each caller always has.  One ratio on both axes reads "ratio n/d" and names w, h and tilesize
// together; a pair -- and everything the _xy / _fmt size functions say, and the engine's word on 4:2:2 columns -- reads "ratios" and names
// the axes apart.  The engine alone adds the sizes it was asked about.
static std::string out_refusal(const PixFmt& f, int w, int h, int T, OutRatio r, OutWho who, bool parity)
{
    const std::string rx = std::to_string(r.nx) + "/" + std::to_string(r.dx), ry = std::to_string(r.ny) + "/" + std::to_string(r.dy), fam = f.family;
    if (parity && who == kWhoEngine && r.is_box())
        return "a " + fam + " output needs w * out_scale" + (f.csy ? ", h * out_scale" : "") + " and tilesize * out_scale even";
    const bool axes = who == kWhoOutSizeXY || !r.same() || (parity && !f.csy);
    std::string s = fam.empty() ? "" : (parity || who != kWhoEngine ? "a " : "") + fam + " output at ";
    if (who == kWhoOutSizeXY || (!parity && (who == kWhoEngine || fam.empty()))) s += "output ";
    s += axes ? "ratios " + r.str() : "ratio " + rx;
    if (!parity)
        s += axes ? ": w and tilesize times " + std::to_string(r.nx) + " must be multiples of " + std::to_string(r.dx) + ", h and tilesize times " + std::to_string(r.ny) +
                        " multiples of " + std::to_string(r.dy)
                  : ": w, h and tilesize times " + std::to_string(r.nx) + " must be multiples of " + std::to_string(r.dx);
    else if (!f.csy) s += " needs w and tilesize times " + rx + " even";
    else s += axes ? " needs w and tilesize times " + rx + " and h and tilesize times " + ry + " even" : " needs w, h and tilesize times " + rx + " even";
    if (who == kWhoEngine) s += " (" + std::to_string(w) + " x " + std::to_string(h) + " at tile " + std::to_string(T) + ")";
    return s;
}

int out_admit(const PixFmt& f, int w, int h, int T, OutRatio r, OutWho who)
{
    if (!r.divides_x(w) || !r.divides_y(h) || !r.divides_x(T) || !r.divides_y(T)) return Engine::fail(RSR_E_ARG, out_refusal(f, w, h, T, r, who, false));
    const long long quotients = (f.csx ? r.of_x(w) | r.of_x(T) : 0) | (f.csy ? r.of_y(h) | r.of_y(T) : 0); // of the subsampled axes
    return quotients & 1 ? Engine::fail(RSR_E_ARG, out_refusal(f, w, h, T, r, who, true)) : RSR_OK;
}

// ---- tensor batches: n images of one geometry behind descriptors (include/realsr_hip.h rsr_process_device_batch) ------------------
int image_layout(int fmt, int w, int h, int c, long long row_pitch, long long plane_pitch, long long* row, long long* plane)
{
    if (w < 1 || h < 1) return Engine::fail(RSR_E_ARG, "bad image size");
    const PixFmt f = pix_fmt(fmt, c);
    if (const int rc = fmt_check(f, c)) return rc;
    if (const int rc = parity_check(f, w, h, "surface")) return rc;
    if (row_pitch < 0 || plane_pitch < 0) return Engine::fail(RSR_E_ARG, "negative pitch");
    const long long es = f.es, packed = w * es;
    const long long rp = row_pitch ? row_pitch : packed;
    if (rp < packed) return Engine::fail(RSR_E_ARG, "row pitch below the bytes of a row");
    if (rp > 0x7fffffffll) return Engine::fail(RSR_E_ARG, "row pitch beyond 2^31 - 1 bytes");
    long long pp = 0;
    if (f.planes > 1)
    {
        pp = plane_pitch ? plane_pitch : h * rp;
        if (rp % es || pp % es) return Engine::fail(RSR_E_ARG, "pitch is not a multiple of the element size");
    }
    else if (rp % f.sample) return Engine::fail(RSR_E_ARG, "row pitch is not a multiple of the sample size");
    *row = rp;
    *plane = pp;
    return RSR_OK;
}

int image_refs(int n, const rsr_image* im, int fmt, int w, int h, int c, const OutRatio* os, const char* what, int index0, ImageRef* out)
{
    const int iw = os ? int(os->of_x(w)) : w, ih = os ? int(os->of_y(h)) : h;
    for (int i = 0; i < n; i++)
    {
        const char* why = nullptr;
        int rc = RSR_OK;
        if (!im[i].data) why = "null data pointer";
        else if ((rc = image_layout(fmt, iw, ih, c, im[i].row_pitch, im[i].plane_pitch, &out[i].row, &out[i].plane)) != RSR_OK) why = last_error();
        else if (w > (1 << 24) || h > (1 << 24)) why = "bad image size";
        else if (reinterpret_cast<uintptr_t>(im[i].data) % uintptr_t(pix_fmt(fmt, c).align())) why = "data is not aligned to the element size";
        if (why) return Engine::fail(RSR_E_ARG, what + (index0 >= 0 ? " " + std::to_string(index0 + i) : std::string()) + ": " + why);
        out[i].data = im[i].data;
    }
    return RSR_OK;
}

int Engine::check_pairs(int n, const rsr_image* in, int in_fmt, int w, int h, int c, const rsr_image* out, int out_fmt, OutRatio* os, ImageRef* src, ImageRef* dst)
{
    {
        std::lock_guard<std::mutex> lk(mu);
        *os = out_ratio;
        if (const int rc = admit(out_fmt, w, h, *os, false)) return rc;
    }
    for (int i = 0; i < n; i++)
    {
        if (const int rc = image_refs(1, &in[i], in_fmt, w, h, c, nullptr, "image", i, &src[i])) return rc;
        if (const int rc = image_refs(1, &out[i], out_fmt, w, h, c, os, "image", i, &dst[i])) return rc;
    }
    return RSR_OK;
}

int Engine::process_device_batch(int n, const rsr_image* in, int in_fmt, int w, int h, int c, const rsr_image* out, int out_fmt, hipStream_t user_stream,
                                 bool sync, const uint8_t* mask, int nmask)
{
    // everything is checked before anything is launched
    if (n < 1 || !in || !out || (mask && n != 1)) return fail(RSR_E_ARG, "bad image arguments");
    std::vector<int> sel; // a masked call: the tiles to run
    bool masked = false;  // ... and that it is one (mask is dropped where every tile is set)
    std::vector<ImageRef> refs(size_t(n) * 2);
    ImageRef *const src = refs.data(), *const dst = src + n;
    OutRatio os; // the output windows are checked against the output ratio in force now; should it change before the launch: RSR_E_STATE
    if (const int rc = check_pairs(n, in, in_fmt, w, h, c, out, out_fmt, &os, src, dst)) return rc;
    std::unique_lock<std::mutex> lk(mu);
    if (const int rc = admit(out_fmt, w, h, os, true)) return rc;
    const int ntiles = tile_count(w, h);
    if (mask)
    {
        if (nmask != ntiles) return fail(RSR_E_ARG, "the mask has " + std::to_string(nmask) + " bytes, the tile grid " + std::to_string(ntiles) + " tiles");
        for (int t = 0; t < ntiles; t++)
            if (mask[t]) sel.push_back(t);
        if (sel.empty())
        { // nothing changed: nothing is launched
            masked_calls++;
            masked_tiles_skipped += ntiles;
            return RSR_OK;
        }
        masked = true;
        if (int(sel.size()) == ntiles) mask = nullptr; // every tile: the plain call, on its cached plan
    }
    return on_stream(lk, user_stream, sync, [&](hipStream_t st, bool& any) {
        // Groups of merge_width images, each ONE tile batch in (a prefix of) the merged plan of this geometry -- the plan and the workspace
        // the merged host calls of that geometry use.  Width 1 (a large frame, "merge" 1, profiling): every image a batch of its own.
        const int width = merge_width(w, h, c);
        int rc = RSR_OK, enqueued = 0;
        for (int g0 = 0; g0 < n; g0 += width)
        {
            const int k = std::min(width, n - g0);
            BatchIO io(k, c, in_fmt, out_fmt, os);
            for (int i = 0; i < k; i++) io.set(i, src[g0 + i], dst[g0 + i], w, h);
            // (n == 1: plan_nimg 0, the very call process_device makes; otherwise the progress of all n images is reported here)
            rc = mask ? enqueue_masked(io, sel, st) : enqueue_images(io, 0, -1, n == 1 ? 0 : width, nullptr, st);
            if (rc != RSR_OK) break;
            if (masked)
            { // counted once the call is enqueued: a call that fails has run nothing
                masked_calls++;
                masked_tiles_run += (long long)sel.size();
                masked_tiles_skipped += ntiles - (long long)sel.size();
            }
            enqueued += k;
            batch_groups++;
            if (progress && n > 1)
                for (int i = 1; i <= k * ntiles; i++) progress(g0 * ntiles + i, n * ntiles, progress_user);
        }
        batch_calls++;
        batch_images += enqueued;
        any = enqueued > 0; // a later group that failed leaves the earlier ones enqueued: they complete, and the streams are ordered around them
        return rc;
    });
}

// ---- which tiles changed (include/realsr_hip.h rsr_diff_tiles, rsr_diff_tiles_sequence) -------------------------------------------------
// The n pairs (r[0], r[1]), (r[1], r[2]), ... of checked images (an r[0] without data: pair 0 has no predecessor and marks every tile):
// one memset and one launch on the caller's stream -- the kernel touches neither the workspace nor anything of the calls in flight, so it
// needs no ordering against the compute stream.  A null stream: the context's own, and the call waits.
template <int N> static hipError_t diff_launch(int n, const ImageRef* r, int fmt, int w, int h, int c, int T, int P, uint8_t* d_masks, hipStream_t st)
{
    DiffArgs<N> da;
    std::memset(&da, 0, sizeof da);
    for (int k = 0; k < n; k++)
    {
        DiffPair& p = da.pair[k];
        p.a = static_cast<const uint8_t*>(r[k].data), p.pitch_a = r[k].row, p.plane_a = r[k].plane;
        p.b = static_cast<const uint8_t*>(r[k + 1].data), p.pitch_b = r[k + 1].row, p.plane_b = r[k + 1].plane;
    }
    da.n = n, da.fmt = fmt, da.w = w, da.h = h, da.c = c;
    da.T = T, da.P = P, da.nx = (w + T - 1) / T, da.ny = (h + T - 1) / T;
    da.mask = d_masks;
    return launch_diff_tiles(da, st);
}

int Engine::diff_pairs(int n, const ImageRef* r, int fmt, int w, int h, int c, uint8_t* d_masks, hipStream_t user_stream)
{
    {
        std::lock_guard<std::mutex> lk(mu);
        hipStream_t st = user_stream ? user_stream : stream;
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(n == 1 ? diff_launch<1>(n, r, fmt, w, h, c, tilesize, prepadding, d_masks, st) // (one pair: the small argument block)
                       : diff_launch<kMaxMerge>(n, r, fmt, w, h, c, tilesize, prepadding, d_masks, st));
    }
    if (!user_stream) HIP_TRY(hipStreamSynchronize(stream));
    return RSR_OK;
}

// rsr_diff_tiles is the sequence of one pair, with `a` as the predecessor.
int Engine::diff_tiles(const rsr_image* a, const rsr_image* b, int fmt, int w, int h, int c, uint8_t* d_mask, hipStream_t user_stream)
{
    if (!a || !b || !d_mask) return fail(RSR_E_ARG, "bad image arguments");
    ImageRef r[2];
    if (const int rc = image_refs(1, a, fmt, w, h, c, nullptr, "image a", -1, &r[0])) return rc;
    if (const int rc = image_refs(1, b, fmt, w, h, c, nullptr, "image b", -1, &r[1])) return rc;
    return diff_pairs(1, r, fmt, w, h, c, d_mask, user_stream);
}

// ---- three-plane YUV frames <-> surfaces (include/realsr_hip.h rsr_pack_planes, rsr_unpack_planes) ------------------------------------------
// Like the diff the launch touches neither the workspace nor anything of the calls in flight: it goes to the caller's stream as it is.
int Engine::move_planes(bool pack, int n, const rsr_planes* planes, const rsr_image* surf, int fmt, int w, int h, hipStream_t user_stream)
{
    const char* const who = pack ? "rsr_pack_planes" : "rsr_unpack_planes";
    if (n < 1 || n > kMaxMerge) return fail(RSR_E_ARG, std::string(who) + ": n must be 1 .. " + std::to_string(kMaxMerge));
    if (!planes || !surf) return fail(RSR_E_ARG, std::string(who) + ": null pointer");
    const PixFmt f = pix_fmt(fmt);
    if (!f.bits) return fail(RSR_E_ARG, std::string(who) + ": the format must be one of the YUV formats");
    ImageRef refs[kMaxMerge];
    if (const int rc = image_refs(n, surf, fmt, w, h, 3, nullptr, "surface", 0, refs)) return rc;
    PlanesArgs pa;
    std::memset(&pa, 0, sizeof pa);
    const long long yrow = (long long)w * f.es, crow = (long long)(w >> f.csx) * f.es;
    for (int i = 0; i < n; i++)
    {
        const rsr_planes& p = planes[i];
        const char* why = nullptr;
        const long long yp = p.y_pitch ? p.y_pitch : yrow, cp = p.c_pitch ? p.c_pitch : crow;
        const uintptr_t bits = reinterpret_cast<uintptr_t>(p.y) | reinterpret_cast<uintptr_t>(p.u) | reinterpret_cast<uintptr_t>(p.v) | uintptr_t(yp) | uintptr_t(cp);
        if (!p.y || !p.u || !p.v) why = "null plane pointer";
        else if (p.y_pitch < 0 || p.c_pitch < 0) why = "negative pitch";
        else if (yp < yrow || cp < crow) why = "pitch below the bytes of a row";
        else if (bits % uintptr_t(f.es)) why = "a plane pointer or pitch is not a multiple of the sample size";
        if (why) return fail(RSR_E_ARG, std::string(who) + ": frame " + std::to_string(i) + ": " + why);
        PlaneFrame& d = pa.f[i];
        d.y = static_cast<uint8_t*>(p.y), d.u = static_cast<uint8_t*>(p.u), d.v = static_cast<uint8_t*>(p.v);
        d.surf = static_cast<uint8_t*>(const_cast<void*>(refs[i].data));
        d.y_pitch = yp, d.c_pitch = cp, d.row = refs[i].row, d.plane = refs[i].plane;
    }
    pa.n = n, pa.fmt = fmt, pa.w = w, pa.h = h;
    {
        std::lock_guard<std::mutex> lk(mu);
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(launch_move_planes(pa, pack, user_stream ? user_stream : stream));
    }
    if (!user_stream) HIP_TRY(hipStreamSynchronize(stream));
    return RSR_OK;
}

// ---- frame sequences (include/realsr_hip.h "frame sequences") ------------------------------------------------------------------------------
int sequence_sources(int n, int ntiles, const uint8_t* masks, int has_prev, int* src)
{
    if (n < 1 || n > kMaxMerge || ntiles < 1 || !masks || !src) return Engine::fail(RSR_E_ARG, "bad sequence arguments");
    for (int t = 0; t < ntiles; t++)
    {
        int last = -1;
        for (int k = 0; k < n; k++)
        {
            if (masks[size_t(k) * ntiles + t]) last = k;
            if (last < 0 && !has_prev)
                return Engine::fail(RSR_E_ARG, "tile " + std::to_string(t) + " of frame " + std::to_string(k) + " is not set and there is no previous output to take it from");
            src[size_t(k) * ntiles + t] = last;
        }
    }
    return RSR_OK;
}

// diff_tiles for the n consecutive pairs (prev, frames[0]), (frames[0], frames[1]), ...: every descriptor is checked as diff_tiles checks
// its two.
int Engine::diff_tiles_sequence(int n, const rsr_image* frames, const rsr_image* prev, int fmt, int w, int h, int c, uint8_t* d_masks, hipStream_t user_stream)
{
    if (n < 1 || n > kMaxMerge || !frames || !d_masks) return fail(RSR_E_ARG, "bad image arguments");
    ImageRef r[kMaxMerge + 1]; // r[0]: prev (none: it stays without data), r[k + 1]: frame k
    if (prev)
        if (const int rc = image_refs(1, prev, fmt, w, h, c, nullptr, "previous frame", -1, &r[0])) return rc;
    if (const int rc = image_refs(n, frames, fmt, w, h, c, nullptr, "image", 0, &r[1])) return rc;
    return diff_pairs(n, r, fmt, w, h, c, d_masks, user_stream);
}

// The byte rectangles of output tile `tile` of an os.of_x(w) x os.of_y(h) image in out_fmt, from the image `src` to the image `dst`: one per
// plane of the format, plane q at q * plane pitch, all with the byte columns of the first; a subsampled chroma plane (the UV plane of a
// 4:2:0 surface) has half the rows -- out_admit has made the tile's edges even on that axis.
static void output_rects(int out_fmt, int w, int h, int c, int T, OutRatio os, int tile, const ImageRef& dst, const ImageRef& src, std::vector<PropRect>& out)
{
    uint8_t* const db = static_cast<uint8_t*>(const_cast<void*>(dst.data));
    const uint8_t* const sb = static_cast<const uint8_t*>(src.data);
    const PixFmt f = pix_fmt(out_fmt, c);
    const int nx = (w + T - 1) / T, yi = tile / nx, xi = tile - yi * nx;
    const long long x0 = os.of_x((long long)xi * T), y0 = os.of_y((long long)yi * T), x1 = os.of_x(std::min((xi + 1) * T, w)), y1 = os.of_y(std::min((yi + 1) * T, h));
    const int width = int((x1 - x0) * f.es), rows = int(y1 - y0);
    for (int q = 0; q < f.planes; q++)
    {
        const int cs = q ? f.csy : 0;
        out.push_back(PropRect{db + q * dst.plane + (y0 >> cs) * dst.row + x0 * f.es, sb + q * src.plane + (y0 >> cs) * src.row + x0 * f.es, dst.row, src.row, width, rows >> cs});
    }
}

int Engine::process_device_sequence(int n, const rsr_image* in, int in_fmt, int w, int h, int c, const rsr_image* out, int out_fmt, const rsr_image* prev_out,
                                    const uint8_t* masks, int nmask, hipStream_t user_stream, bool sync)
{
    // everything is checked before anything is launched
    if (n < 1 || n > kMaxMerge || !in || !out || !masks) return fail(RSR_E_ARG, "bad sequence arguments");
    ImageRef src[kMaxMerge], dst[kMaxMerge], prev;
    OutRatio os;
    if (const int rc = check_pairs(n, in, in_fmt, w, h, c, out, out_fmt, &os, src, dst)) return rc;
    if (prev_out) // an output image like the others
        if (const int rc = image_refs(1, prev_out, out_fmt, w, h, c, &os, "previous output", -1, &prev)) return rc;
    // frame 0 updated in place: its own rectangles of the previous output are already where they belong
    const bool in_place = prev_out && prev.data == dst[0].data && prev.row == dst[0].row && prev.plane == dst[0].plane;
    std::unique_lock<std::mutex> lk(mu);
    if (const int rc = admit(out_fmt, w, h, os, true)) return rc;
    const int ntiles = tile_count(w, h);
    if (nmask != (long long)n * ntiles)
        return fail(RSR_E_ARG, "the masks have " + std::to_string(nmask) + " bytes, " + std::to_string(n) + " frames of " + std::to_string(ntiles) + " tiles each");
    std::vector<int> from(static_cast<size_t>(nmask));
    if (const int rc = sequence_sources(n, ntiles, masks, prev_out != nullptr, from.data())) return rc;
    std::vector<int> sel; // (frame, tile) pairs that walk the network, frame-major
    std::vector<PropRect> rects;
    long long copied = 0;
    for (int k = 0; k < n; k++)
        for (int t = 0; t < ntiles; t++)
        {
            const int s = from[size_t(k) * ntiles + t];
            if (s == k) sel.push_back(k * ntiles + t);
            else if (!(s < 0 && k == 0 && in_place))
            {
                output_rects(out_fmt, w, h, c, tilesize, os, t, dst[k], s < 0 ? prev : dst[s], rects);
                copied++;
            }
        }
    auto count = [&]() { // once the call is enqueued (or has nothing to do): a call that fails counts nothing
        seq_calls++;
        seq_frames += n;
        seq_tiles_run += (long long)sel.size();
        seq_tiles_copied += copied;
    };
    if (sel.empty() && rects.empty())
    { // nothing changed and everything is in place: nothing is launched
        count();
        return RSR_OK;
    }
    return on_stream(lk, user_stream, sync, [&](hipStream_t st, bool& any) {
        BatchIO io(n, c, in_fmt, out_fmt, os);
        for (int i = 0; i < n; i++) io.set(i, src[i], dst[i], w, h);
        const int rc = enqueue_sequence(io, sel, rects, st, seq_batches, nullptr);
        if (rc == RSR_OK)
        {
            count();
            batch_calls++;
        }
        any = true; // (a later batch that failed leaves the earlier ones enqueued: they complete, and the streams are ordered around them)
        return rc;
    });
}

// ---- merging small images across calls (engine.h) ---------------------------------------------
// LR-level work items (16 x 32 blocks; x8 under TTA) of a w x h image at the current tile size; stops counting beyond `limit`
long long Engine::image_items(int w, int h, long long limit) const
{
    const int T = tilesize, P = prepadding;
    if (T < 1) return limit + 1;
    long long items = 0;
    for (int y0 = 0; y0 < h; y0 += T)
        for (int x0 = 0; x0 < w; x0 += T)
        {
            const long long th = std::min(y0 + T, h) - y0 + 2 * P, tw = std::min(x0 + T, w) - x0 + 2 * P;
            items += ((th + kBlkH - 1) / kBlkH) * ((tw + kBlkW - 1) / kBlkW) * (tta ? 8 : 1);
            if (items > limit) return items;
        }
    return items;
}

// How many images of this geometry one merged batch may take: 1 = the image is not small (more than a quarter of the work items a
// batch aims at: a few launches' worth of blocks per CU by itself) or merging is off; else as many as keep the batch at
// `merge_target_items` LR-level work items, at most merge_max.  ONE cached plan of that width serves every narrower batch of this
// geometry (enqueue_images: plan_nimg).
int Engine::merge_width(int w, int h, int c) const
{
    (void)c;
    const int mmax = merge_max, target = merge_target_items;
    if (mmax <= 1 || profiling) return 1;
    const long long items = image_items(w, h, target / 4);
    if (items * 4 > target) return 1;
    return int(std::max<long long>(1, std::min<long long>(std::min(mmax, kMaxMerge), target / std::max<long long>(items, 1))));
}

// Enqueue the images of g[0..n) as ONE tile batch (one geometry: the cached plan; several: tables built on the fly); records every
// request's ev_done behind it.
int Engine::run_group(MergeReq* const* g, int n)
{
    std::lock_guard<std::mutex> lk(mu);
    if (!loaded || scale != 4) return fail(RSR_E_STATE, "context parameters changed while the call was in flight");
    for (int i = 0; i < n; i++)
        if (g[i]->T != tilesize || g[i]->os != out_ratio) return fail(RSR_E_STATE, "context parameters changed while the call was in flight");
    HIP_TRY(hipSetDevice(device));
    for (int i = 0; i < n; i++)
        if (g[i]->ev_in) HIP_TRY(hipStreamWaitEvent(stream, g[i]->ev_in, 0));
    if (!merge_mid && hipEventCreateWithFlags(&merge_mid, hipEventDisableTiming) != hipSuccess) merge_mid = nullptr;
    merge_mid_used = false;
    bool same = true;
    for (int i = 1; i < n; i++) same = same && g[i]->w == g[0]->w && g[i]->h == g[0]->h;
    int rc;
    // all of one image, or of several of ONE geometry, under the plan of merge_width images; `mid`: the throttle event is recorded in this one
    auto whole = [&](MergeReq* const* r, int k, bool mid) {
        BatchIO io(r, k);
        io.ev_mid = mid ? merge_mid : nullptr;
        return enqueue_images(io, 0, -1, merge_width(r[0]->w, r[0]->h, r[0]->c), nullptr, stream);
    };
    if (same) rc = whole(g, n, true); // launched in a prefix of the cached plan
    else
    {
        rc = enqueue_mixed(g, n, stream, merge_mid);
        if (rc == RSR_OK) merged_mixed++;
        else if (rc == RSR_E_NOMEM)
        { // the batch does not fit the workspace budget / the device right now: one image at a time (each call bounds and halves its own batch)
            (void)hipStreamSynchronize(stream);
            for (int i = 0; i < n; i++)
                if ((rc = whole(g + i, 1, i == n - 1)) != RSR_OK) break;
        }
    }
    if (rc == RSR_OK)
        for (int i = 0; i < n && rc == RSR_OK; i++)
        {
            if (!g[i]->ev_done)
            {
                g[i]->ev_done = take_event();
                g[i]->pool_event = true;
                if (!g[i]->ev_done) rc = fail(RSR_E_DEVICE, "hipEventCreate failed");
            }
            if (rc == RSR_OK && hipEventRecord(g[i]->ev_done, stream) != hipSuccess) rc = fail(RSR_E_DEVICE, "hipEventRecord failed");
        }
    if (rc == RSR_OK)
    {
        merge_mid_used = merge_mid != nullptr;
        if (!merge_done && hipEventCreateWithFlags(&merge_done, hipEventDisableTiming) != hipSuccess) merge_done = nullptr;
        merge_last_n = (merge_done && hipEventRecord(merge_done, stream) == hipSuccess) ? n : 0;
        merged_batches++;
        merged_images += n;
        if (n > merged_widest.load()) merged_widest = n;
    }
    else
    {
        const std::string why = last_error();
        (void)hipStreamSynchronize(stream); // kernels of the batch that did get enqueued use the callers' buffers
        for (int i = 0; i < n; i++)
            if (g[i]->pool_event)
            {
                give_event(g[i]->ev_done);
                g[i]->ev_done = nullptr;
                g[i]->pool_event = false;
            }
        return fail(rc, why);
    }
    return RSR_OK;
}

int Engine::submit_merged(MergeReq& r)
{
    std::unique_lock<std::mutex> lk(cq_mu);
    cq.push_back(&r);
    cq_cv.notify_all(); // (a leader may be waiting for the calls it knows to be inbound)
    if (cq_leader)
    {
        cq_cv.wait(lk, [&]() { return r.done || r.lead; });
        if (r.done)
        {
            if (r.rc != RSR_OK) return fail(r.rc, r.err);
            return RSR_OK;
        }
    }
    // This caller leads: its own request is at the head of the queue (it found the queue without a leader -- i.e. empty -- or the
    // previous leader woke the head).
    cq_leader = true;
    r.lead = false;
    while (!r.done)
    {
        // Throttle: the next batch is formed when the previous one is NEARLY through the network (launch_batch: an event behind the RDB
        // that leaves about half an image's worth of network ahead) -- its ~350 launches (1 - 2 ms of host time) are then enqueued
        // underneath the rest, the GPU never waits, and while this thread waits further calls queue up behind it: that is what fills a
        // batch (measured in profiles/r06_small_images.txt).
        hipEvent_t wait_ev = merge_mid_used ? merge_mid : nullptr;
        lk.unlock();
        if (wait_ev) (void)hipEventSynchronize(wait_ev);
        lk.lock();
        // Calls that are known to be on their way (their image is still being uploaded) are worth a moment: a batch costs milliseconds,
        // they arrive within microseconds -- 16 callers that start together would otherwise open with batches of 1, 1, 7, 7.
        for (const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(400);
             merge_inbound.load() > 0 && int(cq.size()) < kMaxMerge && std::chrono::steady_clock::now() < deadline;)
            cq_cv.wait_until(lk, deadline); // (every arrival notifies)
        // The batch: the head of the queue and, in order of arrival, the calls behind it that fit -- same channel count and tile size (one
        // preproc / conv_last / postproc launch serves all), images of ANY small size (option merge_mixed 0: of the head's size only) --
        // while the batch stays within merge_target_items work items and merge_max images.
        MergeReq* g[kMaxMerge];
        int n = 0;
        const MergeReq* head = cq.front();
        const int width = merge_mixed ? std::min(merge_max.load(), kMaxMerge) : head->width;
        const long long target = merge_target_items;
        long long items = 0;
        for (MergeReq* q : cq)
        {
            if (n >= width) break;
            if (q->c != head->c || q->T != head->T || q->os != head->os) continue;
            if (!merge_mixed && (q->w != head->w || q->h != head->h)) continue;
            if (n > 0 && items + q->items > target) continue;
            g[n++] = q;
            items += q->items;
        }
        // Every width up to merge_width shares one plan (enqueue_images: plan_nimg), so any number can be taken.  All of them when the GPU
        // has run dry.  While the previous batch is still running, though, taking everything that waits makes the batch sizes
        // ALTERNATE for ever (the callers of batch n - 1 are exactly what waits when batch n + 1 is formed: 1, 15, 1, 15 ... is as stable
        // as 8, 8, 8, 8 and much slower): take half of (waiting + in flight), the rest leads the next batch.
        int take = n;
        if (merge_last_n > 0 && merge_done && hipEventQuery(merge_done) == hipErrorNotReady) take = std::min(n, std::max(1, (n + merge_last_n + 1) / 2));
        (void)hipGetLastError(); // (hipErrorNotReady is not an error)
        for (int i = 0; i < take; i++) cq.erase(std::find(cq.begin(), cq.end(), g[i]));
        static const bool trace = std::getenv("RSR_MERGE_TRACE") != nullptr; // (debug aid: one line per merged batch)
        if (trace)
            std::fprintf(stderr, "merge: t=%.3f ms take %d of %d waiting (width %d, previous batch of %d %s, %d inbound)\n",
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(), take, n, width, merge_last_n,
                         (merge_done && hipEventQuery(merge_done) == hipErrorNotReady) ? "running" : "done", merge_inbound.load());
        (void)hipGetLastError();
        lk.unlock();
        const int rc = run_group(g, take);
        const std::string why = rc == RSR_OK ? std::string() : std::string(last_error());
        lk.lock();
        for (int i = 0; i < take; i++)
        {
            g[i]->rc = rc;
            g[i]->err = why;
            g[i]->done = true;
        }
        cq_cv.notify_all();
    }
    if (!cq.empty()) cq.front()->lead = true; // hand over: the head of the queue forms the next batch
    else cq_leader = false;
    cq_cv.notify_all();
    if (r.rc != RSR_OK) return fail(r.rc, r.err);
    return RSR_OK;
}

Lane* Engine::acquire_lane()
{
    std::unique_lock<std::mutex> lk(lane_mu);
    for (;;)
    {
        for (auto& l : lanes)
            if (!l->busy)
            {
                l->busy = true;
                return l.get();
            }
        if (int(lanes.size()) < max_lanes)
        {
            lanes.emplace_back(new Lane());
            lanes.back()->busy = true;
            return lanes.back().get();
        }
        lane_cv.wait(lk);
    }
}

void Engine::release_lane(Lane* l)
{
    {
        std::lock_guard<std::mutex> lk(lane_mu);
        l->busy = false;
    }
    lane_cv.notify_one();
}

static bool is_pinned_host(const void* p)
{
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, p) != hipSuccess)
    {
        (void)hipGetLastError(); // plain malloc'd memory: "invalid value", not an error of ours
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

static int ensure_pinned(void*& p, size_t& have, size_t need)
{
    if (have >= need && p) return RSR_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    have = 0;
    const hipError_t e = hipHostMalloc(&p, need, hipHostMallocDefault);
    if (e != hipSuccess)
    {
        p = nullptr;
        (void)hipGetLastError();
        return Engine::fail(RSR_E_NOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    }
    have = need;
    return RSR_OK;
}

int Lane::open()
{
    if (copy) return RSR_OK;
    HIP_TRY(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
    for (hipEvent_t* e : events()) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return RSR_OK;
}

// A lane for the duration of one host call; `rc` says whether it is ready for use.
// Whatever way the call ends, nothing of it may still be in flight when the lane -- and with it the caller's `in` / `out`
// -- is handed back: a HIP failure half way must not turn into a use-after-free of the lane buffers by the next caller.
struct LaneHold
{
    Engine* const e;
    Lane* const l;
    bool done_recorded = false; // ev_done was recorded on behalf of this call (lane_run, or the leader of its merged batch)
    int rc;
    explicit LaneHold(Engine* e_) : e(e_), l(e_->acquire_lane()) { rc = open(); }
    LaneHold(const LaneHold&) = delete;
    ~LaneHold()
    {
        if (l->copy) (void)hipStreamSynchronize(l->copy);
        if (done_recorded) (void)hipEventSynchronize(l->ev_done);
        e->release_lane(l);
    }

private:
    int open()
    {
        HIP_TRY(hipSetDevice(e->device));
        return l->open();
    }
};

static int lane_reserve(DevBuf& b, std::atomic<size_t>& published, size_t bytes) // lane-private: nothing else can be using the old allocation
{
    const int rc = Engine::ensure(b, bytes);
    published.store(b.bytes, std::memory_order_relaxed); // what device_avail() / rsr_get_stat read (they do not hold this lane)
    return rc;
}

int Engine::lane_reserve_out(Lane& L, const void* out, size_t dev_bytes, size_t fetch_bytes, bool& out_pinned)
{
    if (const int rc = lane_reserve(L.d_out, L.out_bytes, dev_bytes)) return rc;
    out_pinned = is_pinned_host(out);
    return out_pinned ? RSR_OK : ensure_pinned(L.h_out, L.h_out_bytes, 2 * std::min(std::max<size_t>(chunk_bytes, 1 << 20), fetch_bytes));
}

int Engine::lane_upload(Lane& L, const void* in, size_t nin)
{
    if (const int rc = lane_reserve(L.d_in, L.in_bytes, nin)) return rc;
    const void* src = in;
    if (!is_pinned_host(in))
    {
        if (const int rc = ensure_pinned(L.h_in, L.h_in_bytes, nin)) return rc;
        pool.copy(L.h_in, in, nin, copy_threads);
        src = L.h_in;
    }
    HIP_TRY(hipMemcpyAsync(L.d_in.p, src, nin, hipMemcpyHostToDevice, L.copy));
    HIP_TRY(hipEventRecord(L.ev_in, L.copy));
    return RSR_OK;
}

int Engine::lane_run(LaneHold& hold, const BatchIO& io, int tile0, int tile1, int T, size_t* half_rows)
{
    std::lock_guard<std::mutex> lk(mu);
    if (!loaded || scale != 4 || tilesize != T || out_ratio != io.os)
        return fail(RSR_E_STATE, "context parameters changed while the call was in flight"); // (the hold drains the upload)
    HIP_TRY(hipStreamWaitEvent(stream, hold.l->ev_in, 0));
    const int rc = enqueue_images(io, tile0, tile1, 0, half_rows, stream);
    if (rc != RSR_OK)
    {
        (void)hipStreamSynchronize(stream); // kernels of this call that did get enqueued use the lane buffers
        return rc;
    }
    HIP_TRY(hipEventRecord(hold.l->ev_done, stream));
    hold.done_recorded = true;
    return RSR_OK;
}

// What the call for tiles [tile0, tile1) of a w x h x c uint8 image downloads (tiles are independent: realsr.cpp:377-380,458-459,490).
// A range of whole tile rows is a contiguous byte range of the output: when the engine split the 4x tail, its first `half_rows` output
// rows are complete at ev_half and travel while the second part is still being computed.  A general range is up to three rectangles --
// the tail of its first tile row, the head of its last row, the whole rows between.  No HIP call: tools/host_check checks it byte by byte.
static FetchPlan fetch_plan(int w, int h, int c, int T, const OutRatio& os, int tile0, int tile1, size_t half_rows)
{
    const int xtiles = (w + T - 1) / T;
    const size_t rowbytes = size_t(os.of_x(w)) * c; // one output row
    auto yof = [&](int tr) { return size_t(os.of_y(std::min(tr * T, h))); };  // first output row of tile row tr (whole: out_admit)
    auto xof = [&](int tc) { return size_t(os.of_x(std::min(tc * T, w))) * c; }; // byte column of tile column tc
    const int r0 = tile0 / xtiles, c0 = tile0 % xtiles, r1 = (tile1 - 1) / xtiles, c1 = (tile1 - 1) % xtiles + 1; // last tile = (r1, c1 - 1)
    FetchPlan p{yof(r0), yof(r1 + 1) - yof(r0), 0, {}};
    auto add = [&](size_t y_a, size_t y_b, size_t x_a, size_t x_b, bool early) {
        if (y_b > y_a && x_b > x_a) p.span[p.n++] = FetchSpan{y_a * rowbytes + x_a, x_b - x_a, y_b - y_a, early};
    };
    if (c0 == 0 && c1 == xtiles)
    {
        const size_t first = std::min(p.rows, half_rows);
        add(p.row0, p.row0 + first, 0, rowbytes, true);
        add(p.row0 + first, p.row0 + p.rows, 0, rowbytes, false);
    }
    else if (r0 == r1) add(yof(r0), yof(r0 + 1), xof(c0), xof(c1), false);
    else
    {
        const int full0 = c0 ? r0 + 1 : r0, full1 = c1 != xtiles ? r1 : r1 + 1; // whole tile rows [full0, full1)
        if (full0 != r0) add(yof(r0), yof(r0 + 1), xof(c0), rowbytes, false);
        if (full1 != r1 + 1) add(yof(r1), yof(r1 + 1), 0, xof(c1), false);
        add(yof(full0), yof(full1), 0, rowbytes, false);
    }
    return p;
}

// The staging chunks of a span, given the bytes of one staging slot: a contiguous span is cut by bytes (chunks of one "row" of up to
// `slot` bytes), a rectangle by whole rows.  fetch_chunks: how many there are; fetch_chunk: chunk i.
static int fetch_chunks(const FetchSpan& s, size_t rowbytes, size_t slot, size_t& n)
{
    if (s.width == rowbytes) n = (s.width * s.rows + slot - 1) / slot;
    else if (s.width > slot) return Engine::fail(RSR_E_ARG, "chunk_mb smaller than one output row");
    else n = (s.rows + slot / s.width - 1) / (slot / s.width);
    return RSR_OK;
}

static FetchSpan fetch_chunk(const FetchSpan& s, size_t rowbytes, size_t slot, size_t i)
{
    if (s.width == rowbytes) return FetchSpan{s.off + i * slot, std::min(slot, s.width * s.rows - i * slot), 1, s.early};
    const size_t rows_per = slot / s.width;
    return FetchSpan{s.off + i * rows_per * rowbytes, s.width, std::min(rows_per, s.rows - i * rows_per), s.early};
}

// The download of a host call: the spans of fp from the lane's d_out -- which holds the output rows fp.row0 .. fp.row0 + fp.rows -- to
// `out`, the full-size image, each span behind the event that completes it.  Pinned memory receives the spans directly; pageable memory
// through the two staging slots lane_reserve_out made, so that the CPU copy of a chunk runs under the PCIe transfer of the next one.
int Engine::lane_fetch(Lane& L, char* out, bool out_pinned, size_t rowbytes, const FetchPlan& fp)
{
    auto dev = [&](size_t off) { return static_cast<const char*>(L.d_out.p) + (off - fp.row0 * rowbytes); }; // device address of byte `off` of the full-size image
    hipEvent_t waited = nullptr;
    auto ready = [&](const FetchSpan& s) {
        hipEvent_t ev = s.early ? L.ev_half : L.ev_done;
        return ev == std::exchange(waited, ev) ? hipSuccess : hipStreamWaitEvent(L.copy, ev, 0);
    };
    if (out_pinned)
    {
        for (int k = 0; k < fp.n; k++)
        {
            const FetchSpan& s = fp.span[k];
            HIP_TRY(ready(s));
            if (s.width == rowbytes) HIP_TRY(hipMemcpyAsync(out + s.off, dev(s.off), s.width * s.rows, hipMemcpyDeviceToHost, L.copy));
            else HIP_TRY(hipMemcpy2DAsync(out + s.off, rowbytes, dev(s.off), rowbytes, s.width, s.rows, hipMemcpyDeviceToHost, L.copy));
        }
        HIP_TRY(hipStreamSynchronize(L.copy));
        return RSR_OK;
    }
    // ensure_pinned only grows h_out: a slot is half of it, but never more than chunk_mb says now, whatever an earlier call left on the lane
    const size_t slot = std::min(L.h_out_bytes / 2, std::max<size_t>(chunk_bytes, 1 << 20));
    size_t nch[3];
    for (int k = 0; k < fp.n; k++) // (a refusal comes before the first copy)
        if (const int rc = fetch_chunks(fp.span[k], rowbytes, slot, nch[k])) return rc;
    // chunk i travels into slot i & 1 while the CPU drains chunk i - 1 from the other one
    auto slot_of = [&](size_t i) { return static_cast<char*>(L.h_out) + (i & 1) * slot; };
    auto drain = [&](size_t i, const FetchSpan& ch) -> int {
        HIP_TRY(hipEventSynchronize(L.ev_chunk[i & 1]));
        if (ch.rows == 1) pool.copy(out + ch.off, slot_of(i), ch.width, copy_threads);
        else
            for (size_t y = 0; y < ch.rows; y++) std::memcpy(out + ch.off + y * rowbytes, slot_of(i) + y * ch.width, ch.width);
        return RSR_OK;
    };
    size_t i = 0;
    FetchSpan prev{};
    for (int k = 0; k < fp.n; k++)
    {
        HIP_TRY(ready(fp.span[k]));
        for (size_t j = 0; j < nch[k]; j++, i++)
        {
            const FetchSpan ch = fetch_chunk(fp.span[k], rowbytes, slot, j);
            // slot i & 1 was drained by the CPU copy of chunk i - 2 in the previous iteration
            if (ch.rows == 1) HIP_TRY(hipMemcpyAsync(slot_of(i), dev(ch.off), ch.width, hipMemcpyDeviceToHost, L.copy));
            else HIP_TRY(hipMemcpy2DAsync(slot_of(i), ch.width, dev(ch.off), rowbytes, ch.width, ch.rows, hipMemcpyDeviceToHost, L.copy));
            HIP_TRY(hipEventRecord(L.ev_chunk[i & 1], L.copy));
            if (i >= 1)
                if (const int rc = drain(i - 1, prev)) return rc;
            prev = ch;
        }
    }
    return i ? drain(i - 1, prev) : RSR_OK;
}

// RealSR::process for host images.  The call owns a lane: upload on the lane's copy stream, kernels on the compute
// stream (ordered by events), download on the copy stream again.  Pinned caller memory (rsr_host_alloc, hipHostMalloc,
// hipHostRegister) is copied directly; pageable memory goes through the lane's pinned staging, the download in chunks so
// that the CPU copy of chunk i overlaps the PCIe transfer of chunk i+1.
// tile0 / tile1: only tiles [tile0, tile1) of the row-major tile grid: what of the output that is, fetch_plan says.
// The steps -- check, tile range, lane, plan, reserve, upload, merged or lane_run, lane_fetch -- are DESIGN.md 6.2.
int Engine::process_host(const uint8_t* in, int w, int h, int c, uint8_t* out, int tile0, int tile1)
{
    if (!in || !out || w < 1 || h < 1 || (c != 3 && c != 4)) return fail(RSR_E_ARG, "bad image arguments");
    const size_t nin = size_t(w) * h * c;
    int T = 0, mwidth = 1;
    OutRatio os; // the output ratio in force when the call came in (the size of `out`)
    long long mitems = 0;
    { // state checks BEFORE anything is enqueued on behalf of this call (and the engine's settings read under its lock)
        std::lock_guard<std::mutex> lk(mu);
        if (!loaded) return fail(RSR_E_STATE, "process before load");
        if (scale != 4) return fail(RSR_E_ARG, "only scale 4 is supported (main.cpp:533-537)");
        T = tilesize;
        os = out_ratio;
        if (const int rrc = out_admit(pix_fmt(RSR_FMT_U8_HWC), w, h, T, os, kWhoEngine)) return rrc;
        mwidth = merge_width(w, h, c);
        if (mwidth > 1) mitems = image_items(w, h, merge_target_items);
    }
    const int xtiles = (w + T - 1) / T, ytiles = (h + T - 1) / T;
    if (tile1 < 0) tile1 = xtiles * ytiles;
    if (tile0 < 0 || tile1 > xtiles * ytiles || tile0 >= tile1) return fail(RSR_E_ARG, "tile range outside the image");
    // a small whole image is merged with the images other callers hand in meanwhile (Engine::submit_merged); a leader that is
    // forming a batch gives the calls counted here a moment to finish their upload
    const bool mergeable = tile0 == 0 && tile1 == xtiles * ytiles && mwidth > 1;
    struct Inbound
    {
        std::atomic<int>* n;
        ~Inbound() { release(); }
        void release()
        {
            if (n) --*n;
            n = nullptr;
        }
    } inbound{nullptr};
    LaneHold hold(this);
    Lane* const L = hold.l;
    if (mergeable)
    { // counted from here: a call that is still waiting for a lane is not "on its way" (lanes free up when batches complete)
        ++merge_inbound;
        inbound.n = &merge_inbound;
    }
    if (hold.rc != RSR_OK) return hold.rc;
    // The device output holds only the output ROWS of this call's tile range (a member of rsr_process_group running an eighth
    // of a 4K frame does not allocate 398 MB for it): the kernels get the REAL base of the allocation -- the plan of a tile range
    // places its tiles relative to the range's first output row (Plan::out_row0, in x4 rows, is the x4 row of fp.row0: get_plan) --
    // and only ever write inside the rectangles of the range's tiles (conv_last / postproc_tiles place by tile), i.e. inside it.
    const size_t rowbytes = size_t(os.of_x(w)) * c; // one output row
    FetchPlan fp = fetch_plan(w, h, c, T, os, tile0, tile1, 0); // (which rows are early is known once the network is enqueued)
    int rc;
    bool out_pinned = false;
    if ((rc = lane_reserve_out(*L, out + fp.span[0].off, fp.rows * rowbytes, fp.bytes(), out_pinned)) != RSR_OK || (rc = lane_upload(*L, in, nin)) != RSR_OK) return rc;

    // ---- network ----
    size_t half_rows = 0;
    if (mergeable)
    {
        MergeReq r;
        r.d_in = L->d_in.p; r.d_out = L->d_out.p; r.w = w; r.h = h; r.c = c; r.T = T;
        r.os = os;
        r.items = mitems;
        r.width = mwidth;
        r.ev_in = L->ev_in;
        r.ev_done = L->ev_done;
        inbound.release(); // (it is in the queue the moment submit_merged has the lock: the leader's wait ends either way)
        rc = submit_merged(r);
        if (rc != RSR_OK) return rc; // (a batch that failed half way has been drained by its leader: nothing of it is in flight)
        hold.done_recorded = true;
        void (*cb)(int, int, void*) = nullptr;
        void* cb_user = nullptr;
        {
            std::lock_guard<std::mutex> lk(mu);
            cb = progress;
            cb_user = progress_user;
        }
        if (cb)
            for (int i = 1; i <= xtiles * ytiles; i++) cb(i, xtiles * ytiles, cb_user);
    }
    else
    {
        BatchIO io(L->d_in.p, L->d_out.p, w, h, c, RSR_FMT_U8_HWC, RSR_FMT_U8_HWC, os);
        io.ev_half = L->ev_half;
        if ((rc = lane_run(hold, io, tile0, tile1, T, &half_rows)) != RSR_OK) return rc;
        if (half_rows) fp = fetch_plan(w, h, c, T, os, tile0, tile1, half_rows);
    }
    return lane_fetch(*L, reinterpret_cast<char*>(out), out_pinned, rowbytes, fp);
}

// rsr_process_fmt: process_host for any pair of pixel formats -- tightly packed HOST images, the device path of process_device between an
// upload and a download.  The same steps on a lane as process_host, for whole images: no tile range, no merging, no early
// half; the output -- every plane of it -- is ONE contiguous span.
int Engine::process_host_fmt(const void* in, int in_fmt, int w, int h, int c, void* out, int out_fmt)
{
    if (!in || !out || w < 1 || h < 1 || w > (1 << 24) || h > (1 << 24) || (c != 3 && c != 4)) return fail(RSR_E_ARG, "bad image arguments");
    const PixFmt fin = pix_fmt(in_fmt, c), fout = pix_fmt(out_fmt, c);
    for (const PixFmt* f : {&fin, &fout})
        if (const int rc = fmt_check(*f, c, "the planar float and the YUV formats come with c == 3 only")) return rc;
    if (const int rc = parity_check(fin, w, h, "input")) return rc;
    int T = 0;
    OutRatio os; // the output ratio in force when the call came in (the size of `out`)
    { // state checks BEFORE anything is enqueued on behalf of this call
        std::lock_guard<std::mutex> lk(mu);
        os = out_ratio;
        if (const int rc = admit(out_fmt, w, h, os, true)) return rc;
        T = tilesize;
    }
    const size_t nin = size_t(fin.rows(h)) * size_t(w) * size_t(fin.es);
    const size_t rowbytes = size_t(os.of_x(w)) * size_t(fout.es); // (a UV row has as many bytes as a Y row)
    const FetchPlan fp{0, size_t(fout.rows(os.of_y(h))), 1, {FetchSpan{0, rowbytes, size_t(fout.rows(os.of_y(h))), false}}};
    LaneHold hold(this);
    Lane* const L = hold.l;
    int rc = hold.rc;
    bool out_pinned = false;
    if (rc != RSR_OK || (rc = lane_reserve_out(*L, out, fp.bytes(), fp.bytes(), out_pinned)) != RSR_OK || (rc = lane_upload(*L, in, nin)) != RSR_OK) return rc;
    if ((rc = lane_run(hold, BatchIO(L->d_in.p, L->d_out.p, w, h, c, in_fmt, out_fmt, os), 0, -1, T, nullptr)) != RSR_OK) return rc;
    return lane_fetch(*L, static_cast<char*>(out), out_pinned, rowbytes, fp);
}

// The one-tile batch of the hooks below: one slot of exactly w x h pixels, nothing trimmed; its tables and the planar fp16
// [3][h][w] host tile go to device scratch that lives as long as `t`.
int Engine::one_tile_upload(OneTile& t, const uint16_t* tile, int w, int h)
{
    t.w = w;
    t.h = h;
    t.b.ntiles = t.b.nslots = 1;
    t.b.dims.push_back(TileDim{h, w});
    make_items(t.b, fold_cols);
    const size_t tile_bytes = size_t(w) * h * 6;
    int rc;
    if ((rc = check_tile_px((long long)w * h)) != RSR_OK || (rc = ensure(t.tab, batch_table_bytes(t.b))) != RSR_OK || (rc = ensure(t.tile, tile_bytes)) != RSR_OK)
        return rc;
    char* d = static_cast<char*>(t.tab.p);
    hipError_t he = upload_batch(t.b, d);
    if (he == hipSuccess) he = hipMemcpy(t.tile.p, tile, tile_bytes, hipMemcpyHostToDevice);
    if (he != hipSuccess) return fail(RSR_E_DEVICE, std::string("one-tile upload: ") + hipGetErrorString(he));
    return RSR_OK;
}

int Engine::one_tile_walk(const OneTile& t, const RangeProbe* probe)
{
    int rc = ensure_workspace(1, (long long)t.w * t.h, stream); // (a change of layout zeroes IN: the tile is written every time)
    if (rc != RSR_OK) return rc;
    launch_planar3_to_plane(static_cast<const uint16_t*>(t.tile.p), t.w, t.h, const_cast<void*>(ws_planes(kWsIn).base), plane_ch(), stream);
    const bool was = profiling;
    profiling = false;
    rc = run_network(t.b, stream, 1, nullptr, probe);
    profiling = was;
    return rc;
}

// one tile through the network only (layer-level parity hook); the workspace keeps this tile's layout
int Engine::net_forward(const uint16_t* in, int w, int h, uint16_t* out, float* out32)
{
    if (!in || (!out && !out32) || w < 1 || h < 1) return fail(RSR_E_ARG, "bad arguments");
    std::lock_guard<std::mutex> lk(mu);
    if (!loaded) return fail(RSR_E_STATE, "net_forward before load");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamSynchronize(stream));
    OneTile t;
    int rc;
    if ((rc = one_tile_upload(t, in, w, h)) != RSR_OK || (rc = one_tile_walk(t, nullptr)) != RSR_OK) return rc;
    const size_t npx = size_t(w) * h;
    hipError_t he = hipStreamSynchronize(stream);
    if (he == hipSuccess) he = hipGetLastError();
    if (he == hipSuccess && !precise)
    {
        if (out) he = hipMemcpy(out, ws[kWsOut3].p, npx * 16 * 6, hipMemcpyDeviceToHost);
        if (out32) rc = fail(RSR_E_STATE, "the fp32 output blob exists in precise mode only (rsr_set_option precise 1)");
    }
    else if (he == hipSuccess)
    { // precise mode: conv_last left fp32; the fp16 view of it is rounded here, on the host
        std::vector<float> tmp32(out32 ? 0 : npx * 16 * 3);
        float* dst = out32 ? out32 : tmp32.data();
        he = hipMemcpy(dst, ws[kWsOut3].p, npx * 16 * 12, hipMemcpyDeviceToHost);
        if (he == hipSuccess && out)
            for (size_t i = 0; i < npx * 16 * 3; i++)
            {
                const _Float16 hv = (_Float16)dst[i];
                std::memcpy(&out[i], &hv, 2);
            }
    }
    if (he != hipSuccess) return fail(RSR_E_DEVICE, std::string("net_forward: ") + hipGetErrorString(he));
    return rc;
}

// ---- model self-check ---------------------------------------------------------------------------
// The built-in tile: integer-only, so every build produces the same bytes.  The storage error depends on content, so the tile
// has what a photograph has: a smooth field (value noise on an 8-pixel lattice, bilinear) under a ramp per channel, saturated
// and black patches with hard edges, flat squares, and fine texture (per-pixel noise) on a checkerboard of 37-pixel cells -- the
// other cells stay smooth.  Values are k / 255 as preproc_tiles produces them (float(k) * (1 / 255.f), rounded to fp16).
static inline uint32_t sc_hash(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t v = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA77u ^ (c + 0x165667B1u) * 0xC2B2AE3Du;
    v ^= v >> 15; v *= 0x2C1B3C6Du; v ^= v >> 12; v *= 0x297A2D39u; v ^= v >> 15;
    return v;
}

void selfcheck_tile(uint16_t* dst, int w, int h)
{
    uint16_t lut[256];
    for (int k = 0; k < 256; k++)
    {
        const _Float16 v = (_Float16)(float(k) * (1 / 255.f));
        std::memcpy(&lut[k], &v, 2);
    }
    for (int c = 0; c < 3; c++)
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++)
            {
                const int lx = x >> 3, ly = y >> 3, fx = x & 7, fy = y & 7;
                const int n00 = int(sc_hash(lx, ly, c) & 255), n10 = int(sc_hash(lx + 1, ly, c) & 255), n01 = int(sc_hash(lx, ly + 1, c) & 255),
                          n11 = int(sc_hash(lx + 1, ly + 1, c) & 255);
                const int n = ((n00 * (8 - fx) + n10 * fx) * (8 - fy) + (n01 * (8 - fx) + n11 * fx) * fy + 32) >> 6;
                const int g = (c & 1) ? (h > 1 ? y * 255 / (h - 1) : 0) : (w > 1 ? x * 255 / (w - 1) : 0);
                int k = (166 * n + 89 * g + 127) / 255;
                const int cx = x / 37, cy = y / 37;
                if (((cx + cy) & 1) != 0) k += int(sc_hash(x, y, 16 + c) % 21) - 10;            // fine texture
                else if (sc_hash(cx, cy, 32) % 3 == 0 && (x % 37) >= 8 && (x % 37) < 29 && (y % 37) >= 8 && (y % 37) < 29)
                    k = int(sc_hash(cx, cy, 48 + c) & 255);                                       // a flat square
                if ((x / 7 + y / 5 + c) % 11 == 0) k = 255;                                       // hard edges: saturated ...
                if ((x / 5 + y / 9 + 2 * c) % 13 == 0) k = 0;                                     // ... and black patches
                k = k < 0 ? 0 : (k > 255 ? 255 : k);
                dst[(size_t(c) * h + y) * w + x] = lut[k];
            }
}

// One tile through the network in fp16 storage (range probe behind every convolution) and in precise mode; the two results are compared
// on the device.  `mu` held.  The context comes back in the mode it was in; the workspace is left marked "no layout", so the next call
// lays its guards out afresh, exactly as after a net_forward of another tile size.  The plan cache is not touched.
int Engine::selfcheck(const uint16_t* tile, int w, int h, rsr_selfcheck_report* out)
{
    if (!out) return fail(RSR_E_ARG, "null report");
    if (!loaded) return fail(RSR_E_STATE, "selfcheck before load");
    if (!tile && w == 0 && h == 0) w = h = 148; // C1's padded tile: the size of the storage measurements in profiles/
    if (w < 1 || h < 1) return fail(RSR_E_ARG, "bad tile size");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamSynchronize(stream));
    const size_t npx = size_t(w) * h, nout = npx * 16 * 3;
    std::vector<uint16_t> own;
    if (!tile)
    {
        own.resize(npx * 3);
        selfcheck_tile(own.data(), w, h);
        tile = own.data();
    }
    // device side of the report: nonfinite[nconv] | bytes_differ | peak_bits[nconv] | storage_err bits, max_byte_diff
    const size_t nc = size_t(nconv), kRep64 = nc + 1, kRep32 = nc + 2, kRepBytes = kRep64 * 8 + kRep32 * 4;
    OneTile t;
    ScratchBuf rep, out16;
    int rc;
    if ((rc = one_tile_upload(t, tile, w, h)) != RSR_OK || (rc = ensure(rep, kRepBytes)) != RSR_OK || (rc = ensure(out16, nout * 2)) != RSR_OK) return rc;
    hipError_t he = hipMemsetAsync(rep.p, 0, kRepBytes, stream);
    unsigned long long* r64 = static_cast<unsigned long long*>(rep.p);
    unsigned* r32 = reinterpret_cast<unsigned*>(r64 + kRep64);
    RangeProbe probe;
    probe.nonfinite = r64;
    probe.peak_bits = r32;
    struct Restore // from here on, whatever way the call ends
    {
        Engine& e;
        const bool was_precise;
        ~Restore()
        {
            e.precise = was_precise;
            e.ws_cap_px = 0; // the workspace holds this walk's layout: the next call lays out its own
        }
    } restore{*this, precise};
    for (int pass = 0; pass < 2 && he == hipSuccess; pass++)
    {
        precise = pass == 1;
        if ((rc = one_tile_walk(t, pass == 0 ? &probe : nullptr)) != RSR_OK) return rc;
        if (pass == 0) he = hipMemcpyAsync(out16.p, ws[kWsOut3].p, nout * 2, hipMemcpyDeviceToDevice, stream);
        else launch_output_compare(static_cast<const uint16_t*>(out16.p), static_cast<const float*>(ws[kWsOut3].p), (long long)nout, r32 + nc, r64 + nc, stream);
    }
    std::vector<unsigned long long> h64(kRep64);
    std::vector<unsigned> h32(kRep32);
    if (he == hipSuccess) he = hipStreamSynchronize(stream);
    if (he == hipSuccess) he = hipGetLastError();
    if (he == hipSuccess) he = hipMemcpy(h64.data(), r64, kRep64 * 8, hipMemcpyDeviceToHost);
    if (he == hipSuccess) he = hipMemcpy(h32.data(), r32, kRep32 * 4, hipMemcpyDeviceToHost);
    if (he != hipSuccess) return fail(RSR_E_DEVICE, std::string("selfcheck: ") + hipGetErrorString(he));

    rsr_selfcheck_report r;
    std::memset(&r, 0, sizeof r);
    r.tile_w = w;
    r.tile_h = h;
    std::memcpy(&r.storage_err, &h32[nc], 4);
    r.headroom = r.storage_err > 0.f ? (1.f / 255.f) / r.storage_err : 3.402823466e+38f;
    r.max_byte_diff = int(h32[nc + 1]);
    r.bytes_differ = (long long)h64[nc];
    r.peak_conv = 0;
    for (size_t i = 0; i < nc; i++)
    {
        std::memcpy(&sc_peak[i], &h32[i], 4);
        sc_nonfinite[i] = (long long)h64[i];
        r.nonfinite += sc_nonfinite[i];
        if (sc_peak[i] > r.peak_abs)
        {
            r.peak_abs = sc_peak[i];
            r.peak_conv = int(i);
        }
    }
    r.fp16_overflow = (r.nonfinite > 0 || r.peak_abs >= 65504.f) ? 1 : 0;
    r.recommend_precise = r.headroom < 1.5f ? 1 : 0;
    r.elapsed_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    sc_last = r;
    sc_have = true;
    selfcheck_runs++;
    *out = r;
    return RSR_OK;
}

int Engine::apply_precise_auto()
{
    rsr_selfcheck_report r;
    const int rc = selfcheck(nullptr, 0, 0, &r);
    if (rc == RSR_OK) precise = precise_by_auto = r.recommend_precise != 0;
    return rc;
}

// one convolution with caller-supplied weights (layer-level parity hook, include/realsr_hip.h rsr_conv3x3)
int Engine::conv_test(const uint16_t* in, int cin, int h, int w, int ups, const float* weight, const float* bias, int cout,
                      int lrelu, uint16_t* out, float s1, int own_res, const uint16_t* res, float s2, bool prec, const uint8_t* in_lo,
                      const uint8_t* res_lo, uint8_t* out_lo)
{
    if (!in || !weight || !bias || !out || cin < 1 || cout < 1 || cout > 64 || h < 1 || w < 1) return fail(RSR_E_ARG, "bad arguments");
    const bool residual = s1 != 0.f;
    if (residual && (ups || lrelu || (own_res && cin < cout) || (cout % 32))) return fail(RSR_E_ARG, "residual form: no upsampling / activation, cout 32 or 64");
    if (prec && (!residual || cout != 64 || (in_lo && !own_res) || (res_lo && !res))) return fail(RSR_E_ARG, "precise form: a residual form with 64 output channels");
    std::lock_guard<std::mutex> lk(mu);
    HIP_TRY(hipSetDevice(device));
    Model m;
    ConvRec c;
    c.cin = cin; c.cout = cout; c.act = lrelu ? 2 : 0; c.slope = 0.2f;
    c.weight.assign(weight, weight + size_t(cin) * cout * 9);
    c.bias.assign(bias, bias + cout);
    m.convs.push_back(c);
    std::vector<unsigned char> pk(packed_size(m));
    std::string e;
    int rc = pack_model(m, pk.data(), pk.size(), e);
    if (rc != RSR_OK) return fail(rc, e);
    const PackedConv pc = *reinterpret_cast<const PackedConv*>(pk.data() + sizeof(PackedHeader));
    constexpr int pch = plane_ch();
    const int np = int(pc.nplanes) * (32 / pch), nt = int(pc.nt); // input planes (cin padded to a multiple of 32)
    const int npo = nt * (32 / pch);                              // output planes
    const int H = ups ? 2 * h : h, W = ups ? 2 * w : w;
    const size_t ipx = size_t(h) * w, opx = size_t(H) * W;
    // planar [cin][h][w] -> guarded planes [np][h][w][pch]
    const size_t ipl_b = size_t(WsLayout::guarded_plane((long long)ipx)), ipl = ipl_b / 2, opl_b = opx * size_t(pch) * 2; // bytes / halfs per guarded input plane, bytes per output plane
    // precise form: the one-byte lo pair planes of a tensor follow its hi planes in the same allocation (kernels.h ConvArgs::lo1_off)
    const long long in_lo_off = in_lo ? WsLayout::lo_behind(np, ipl_b) : 0, res_lo_off = res_lo ? WsLayout::lo_behind(npo, ipl_b) : 0, out_lo_off = out_lo ? WsLayout::lo_behind(npo, opl_b) : 0;
    std::vector<uint16_t> hin(size_t(np + (in_lo ? npo : 0)) * ipl, 0), hout(size_t(npo) * (out_lo ? 2 : 1) * opx * size_t(pch), 0);
    for (int ch = 0; ch < cin; ch++)
        for (size_t p = 0; p < ipx; p++) hin[size_t(ch / pch) * ipl + kGuard / 2 + p * size_t(pch) + size_t(ch % pch)] = in[size_t(ch) * ipx + p];
    // (the lo bytes of an n-tile's two planes share one "pair plane" of the hi geometry: [pixel][half][plane][8 channels], conv_flow.hip lo_row)
    auto lo_index = [&](int ch, size_t p, size_t pair_stride) {
        return size_t(ch / 32) * pair_stride + p * 32 + size_t((ch % 16) / 8) * 16 + size_t((ch % 32) / 16) * 8 + size_t(ch % 8);
    };
    auto put_lo = [&](std::vector<uint16_t>& buf, size_t lo_off, const uint8_t* lo) {
        unsigned char* b = reinterpret_cast<unsigned char*>(buf.data()) + kGuard + lo_off;
        for (int ch = 0; ch < cout; ch++)
            for (size_t p = 0; p < ipx; p++) b[lo_index(ch, p, ipl_b)] = lo[size_t(ch) * ipx + p];
    };
    if (in_lo) put_lo(hin, size_t(in_lo_off), in_lo);
    std::vector<uint16_t> hres;
    if (residual && res)
    { // planar [cout][h][w] -> guarded planes like the input
        hres.assign(size_t(npo) * (res_lo ? 2 : 1) * ipl, 0);
        for (int ch = 0; ch < cout; ch++)
            for (size_t p = 0; p < ipx; p++) hres[size_t(ch / pch) * ipl + kGuard / 2 + p * size_t(pch) + size_t(ch % pch)] = res[size_t(ch) * ipx + p];
        if (res_lo) put_lo(hres, size_t(res_lo_off), res_lo);
    }
    ScratchBuf d_w, d_in, d_out, d_tab, d_res;
    // Option "test_redzone" (test hook): input, residual and output lie between two red zones of rz bytes that hold the ws_poison pattern
    // (0xFFFF without one), and so does the whole output in place of zeros: a store outside a buffer changes a red zone, a store that is
    // never made leaves NaN, and a read outside a buffer meets NaN where the next plane's zero guard used to be.  The kernel is handed the
    // same pointers relative to the payload; the input's own guards and padded channels stay zero.
    const size_t rz = size_t(test_redzone);
    const uint16_t rz_pat = uint16_t(ws_poison ? ws_poison & 0xFFFF : 0xFFFF);
    test_redzone_dirty = -1;
    auto with_zones = [&](std::vector<uint16_t>& v) { // [rz | v | rz]
        if (!rz || v.empty()) return;
        v.insert(v.begin(), rz / 2, rz_pat);
        v.insert(v.end(), rz / 2, rz_pat);
    };
    const size_t in_bytes = hin.size() * 2, res_bytes = hres.size() * 2, out_bytes = hout.size() * 2; // of the payloads
    with_zones(hin);
    with_zones(hres);
    std::vector<WorkItem> items;
    // test_repeat > 1 (measurement aid): the same blocks N times in ONE launch -- after the first pass every patch and every
    // output line is in the L2s, i.e. the launch shows what this conv costs when nothing goes to HBM (tools/l2_bound_probe.py)
    for (int rep = 0; rep < std::max(1, test_repeat); rep++)
        append_block_items(items, 0, H, W, 0, 0, 0, 0, 0, fold_cols);
    const TileDim td{h, w};
    if ((rc = ensure(d_w, pk.size())) != RSR_OK || (rc = ensure(d_in, hin.size() * 2)) != RSR_OK ||
        (rc = ensure(d_out, out_bytes + 2 * rz)) != RSR_OK || (rc = ensure(d_tab, 256 + items.size() * sizeof(WorkItem))) != RSR_OK ||
        (!hres.empty() && (rc = ensure(d_res, hres.size() * 2)) != RSR_OK))
        return rc;
    hipError_t he = hipMemcpy(d_w.p, pk.data(), pk.size(), hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(d_in.p, hin.data(), hin.size() * 2, hipMemcpyHostToDevice);
    if (he == hipSuccess) he = rz ? hipMemsetD16Async(d_out.p, rz_pat, (out_bytes + 2 * rz) / 2, stream) : hipMemsetAsync(d_out.p, 0, out_bytes, stream);
    if (he == hipSuccess) he = hipMemcpy(d_tab.p, &td, sizeof td, hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(static_cast<char*>(d_tab.p) + 256, items.data(), items.size() * sizeof(WorkItem), hipMemcpyHostToDevice);
    if (he == hipSuccess && !hres.empty()) he = hipMemcpy(d_res.p, hres.data(), hres.size() * 2, hipMemcpyHostToDevice);
    if (he == hipSuccess)
    {
        ConvArgs a;
        std::memset(&a, 0, sizeof a);
        a.src0 = PlaneSrc{static_cast<char*>(d_in.p) + rz + kGuard, 0, (long long)ipl_b};
        a.n0 = np;
        a.lvl_in = 0;
        a.lvl_out = ups ? 1 : 0;
        a.wpk16 = static_cast<const char*>(d_w.p) + pc.w16_off;
        a.waux = pc.aux_off ? static_cast<const char*>(d_w.p) + pc.aux_off : nullptr;
        a.bias = reinterpret_cast<const float*>(static_cast<const char*>(d_w.p) + pc.b_off);
        a.lrelu = lrelu;
        a.s1 = a.s2 = 1.f;
        if (residual)
        { // the epilogue forms of RDB conv5 / trunk_conv (run_network)
            a.s1 = s1;
            a.precise = prec ? 1 : 0;
            if (own_res)
            {
                a.res1 = a.src0;
                a.res1_kind = 1;
                a.res1_in_acc = 1;
                a.res1_coef = 1.f / s1;
                a.lo1_off = in_lo_off;
            }
            if (res)
            {
                const PlaneSrc rp{static_cast<char*>(d_res.p) + rz + kGuard, 0, (long long)ipl_b};
                if (own_res) { a.res2 = rp; a.res2_kind = 1; a.s2 = s2; a.lo2_off = res_lo_off; }
                else { a.res1 = rp; a.res1_kind = 1; a.lo1_off = res_lo_off; } // trunk_conv form: v = s1*(conv+b) + res  (s2 unused)
            }
            a.out_lo_off = out_lo_off;
        }
        a.out16 = PlaneSrc{static_cast<char*>(d_out.p) + rz, 0, (long long)opx * pch * 2};
        a.items = reinterpret_cast<const WorkItem*>(static_cast<const char*>(d_tab.p) + 256);
        a.nitems = int(items.size());
        a.dims = static_cast<const TileDim*>(d_tab.p);
        a.zeros = zeros.p;
        a.dbg = dbg;
        hipEvent_t e0 = take_event_timed(), e1 = take_event_timed();
        if (e0) (void)hipEventRecord(e0, stream);
        if (!launch_conv_flow(a, nt, num_cu, flow_flags, stream)) rc = fail(RSR_E_STATE, "conv3x3_flow: no variant");
        if (e1) (void)hipEventRecord(e1, stream);
        he = hipStreamSynchronize(stream);
        float ms = 0.f;
        if (e0 && e1 && he == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) last_test_us = double(ms) * 1e3;
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (he == hipSuccess) he = hipGetLastError();
        if (he == hipSuccess) he = hipMemcpy(hout.data(), static_cast<char*>(d_out.p) + rz, out_bytes, hipMemcpyDeviceToHost);
        if (he == hipSuccess && rz)
        { // the six red zones, byte by byte against the pattern
            std::vector<uint16_t> z(rz / 2);
            long long dirty = 0;
            const std::pair<const DevBuf*, size_t> bufs[3] = {{&d_in, in_bytes}, {&d_res, res_bytes}, {&d_out, out_bytes}};
            for (const auto& [buf, payload] : bufs)
                for (int side = 0; side < 2 && payload && he == hipSuccess; side++)
                {
                    he = hipMemcpy(z.data(), static_cast<const char*>(buf->p) + (side ? rz + payload : 0), rz, hipMemcpyDeviceToHost);
                    for (const uint16_t v : z) dirty += ((v ^ rz_pat) & 0xFF ? 1 : 0) + ((v ^ rz_pat) >> 8 ? 1 : 0);
                }
            if (he == hipSuccess) test_redzone_dirty = dirty;
        }
    }
    if (he != hipSuccess) return fail(RSR_E_DEVICE, std::string("conv_test: ") + hipGetErrorString(he));
    if (rc != RSR_OK) return rc;
    for (int ch = 0; ch < cout; ch++)
        for (size_t p = 0; p < opx; p++)
        {
            out[size_t(ch) * opx + p] = hout[(size_t(ch / pch) * opx + p) * size_t(pch) + size_t(ch % pch)];
            if (out_lo) out_lo[size_t(ch) * opx + p] = reinterpret_cast<const unsigned char*>(hout.data())[size_t(out_lo_off) + lo_index(ch, p, opl_b)];
        }
    return RSR_OK;
}

} // namespace rsr
