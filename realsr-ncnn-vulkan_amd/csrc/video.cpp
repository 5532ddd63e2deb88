// video.cpp -- the host video session (include/realsr_hip.h "A video session"): three-plane YUV frames in HOST memory in, upscaled frames out,
// through the device entry points that exist.  Nothing here touches the network: a window of frames is uploaded, packed into surfaces
// (rsr_pack_planes), diffed against its predecessor (rsr_diff_tiles_sequence), run (rsr_process_device_sequence), unpacked and downloaded.
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "engine.h"

using namespace rsr;

#define HIP_TRY(expr)                                                                              \
    do                                                                                             \
    {                                                                                              \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return Engine::fail(RSR_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace
{
struct PlaneDims
{
    long long yrow, crow; // bytes of a Y row, of a U / V row
    int rows, crows;      // rows of the Y plane, of the U and the V plane
    long long bytes() const { return yrow * rows + 2 * crow * crows; } // of a tightly packed frame: what rsr_image_bytes says of its surface
};
PlaneDims plane_dims(int fmt, int w, int h)
{
    const PixFmt f = pix_fmt(fmt);
    return {(long long)w * f.es, (long long)(w >> f.csx) * f.es, h, h >> f.csy};
}

bool is_pinned_at(const void* p)
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
// Is the whole plane -- `rows` rows of `row` bytes, `pitch` apart -- pinned?  Its first and its last byte are asked (one allocation or
// registration is one range).
bool is_pinned(const void* p, long long pitch, long long row, int rows)
{
    return is_pinned_at(p) && is_pinned_at(static_cast<const uint8_t*>(p) + (rows - 1) * pitch + row - 1);
}
} // namespace

struct rsr_video
{
    rsr_ctx* ctx = nullptr;
    int fmt = 0, w = 0, h = 0, ow = 0, oh = 0, window = 0, ntiles = 0;
    OutRatio ratio;              // the context's at open: another one in force makes send fail
    int tilesize = 0;            // likewise
    // what the bytes of an output rectangle depend on beside its source bytes: "precise", the YUV matrix / range / siting, the prepadding.
    // A window that runs under another mode than the one before compares its first frame with nothing (have_prev is dropped), so no
    // rectangle computed under the old mode is propagated.  (A model loaded in between: rsr_video_reset is the caller's.)
    int mode[5] = {0, 0, 0, 0, 0};
    PlaneDims in, out;           // of one input / output frame
    long long in_surf = 0, out_surf = 0; // bytes of one surface
    hipStream_t st = nullptr;
    // device: window + 1 surfaces on each side (slot `prev` holds the last frame of the window before), the planar frames of one window
    // on each side, the masks
    uint8_t *d_in = nullptr, *d_out = nullptr, *d_pin = nullptr, *d_pout = nullptr, *d_masks = nullptr;
    uint8_t *h_in = nullptr, *h_out = nullptr, *h_masks = nullptr; // pinned staging: one window in, ONE frame out, the masks
    int prev = 0;            // slot of the predecessor
    bool have_prev = false;  // (false after open and reset: the next frame is compared with nothing)
    int pending = 0, ready = 0, first_ready = 0; // frames staged; frames receive can hand out, and the first of them

    int slot(int k) const { return (prev + 1 + k) % (window + 1); }
};

static void video_free(rsr_video* v)
{
    if (!v) return;
    (void)hipSetDevice(v->ctx->e.device);
    if (v->st) (void)hipStreamSynchronize(v->st);
    for (uint8_t* p : {v->d_in, v->d_out, v->d_pin, v->d_pout, v->d_masks})
        if (p) (void)hipFree(p);
    for (uint8_t* p : {v->h_in, v->h_out, v->h_masks})
        if (p) (void)hipHostFree(p);
    if (v->st) (void)hipStreamDestroy(v->st);
    delete v;
}

// The host planes of one frame, checked as rsr_pack_planes checks device planes; *yp, *cp: the pitches resolved.
static int check_host_planes(const rsr_video* v, const rsr_planes* p, const PlaneDims& d, const char* who, long long* yp, long long* cp)
{
    if (!p || !p->y || !p->u || !p->v) return Engine::fail(RSR_E_ARG, std::string(who) + ": null plane pointer");
    if (p->y_pitch < 0 || p->c_pitch < 0) return Engine::fail(RSR_E_ARG, std::string(who) + ": negative pitch");
    *yp = p->y_pitch ? p->y_pitch : d.yrow, *cp = p->c_pitch ? p->c_pitch : d.crow;
    if (*yp < d.yrow || *cp < d.crow) return Engine::fail(RSR_E_ARG, std::string(who) + ": pitch below the bytes of a row");
    const uintptr_t bits = reinterpret_cast<uintptr_t>(p->y) | reinterpret_cast<uintptr_t>(p->u) | reinterpret_cast<uintptr_t>(p->v) | uintptr_t(*yp) | uintptr_t(*cp);
    if (bits % uintptr_t(pix_fmt(v->fmt).es)) return Engine::fail(RSR_E_ARG, std::string(who) + ": a plane pointer or pitch is not a multiple of the sample size");
    return RSR_OK;
}

// Has the context left the geometry the session was opened with?
static int check_geometry(const rsr_video* v, const char* who)
{
    Engine& e = v->ctx->e;
    std::lock_guard<std::mutex> lk(e.mu);
    const OutRatio& r = e.out_ratio;
    if (r.nx != v->ratio.nx || r.dx != v->ratio.dx || r.ny != v->ratio.ny || r.dy != v->ratio.dy || e.tilesize != v->tilesize)
        return Engine::fail(RSR_E_STATE, std::string(who) + ": the output ratio or the tile size of the context changed while the session is open");
    return RSR_OK;
}

// The mode the window about to run runs in; another one than the last window's: its first frame has no predecessor.
static void note_mode(rsr_video* v)
{
    Engine& e = v->ctx->e;
    int now[5];
    {
        std::lock_guard<std::mutex> lk(e.mu);
        now[0] = e.precise ? 1 : 0, now[1] = e.yuv_matrix, now[2] = e.yuv_range, now[3] = e.yuv_siting, now[4] = e.prepadding;
    }
    if (std::memcmp(now, v->mode, sizeof now)) v->have_prev = false;
    std::memcpy(v->mode, now, sizeof now);
}

// The three planes of a tightly packed frame at `base`, as an rsr_planes entry.
static rsr_planes packed_planes(uint8_t* base, const PlaneDims& d)
{
    rsr_planes p;
    p.y = base, p.u = base + d.yrow * d.rows, p.v = base + d.yrow * d.rows + d.crow * d.crows;
    p.y_pitch = d.yrow, p.c_pitch = d.crow;
    return p;
}

// Run the pending frames as one window (the header's seven steps; the download is receive's).
static int video_run_pending(rsr_video* v);
static int video_run(rsr_video* v)
{
    note_mode(v);
    const int rc = video_run_pending(v);
    if (rc != RSR_OK)
    { // a window that failed is dropped whole: the next frame is compared with nothing, and nothing of it is in flight when its staging is reused
        v->pending = 0, v->have_prev = false;
        (void)hipStreamSynchronize(v->st);
        (void)hipGetLastError();
    }
    return rc;
}
static int video_run_pending(rsr_video* v)
{
    const int n = v->pending;
    if (n == 0) return RSR_OK;
    Engine& e = v->ctx->e;
    HIP_TRY(hipSetDevice(e.device));
    rsr_planes pin[kMaxMerge], pout[kMaxMerge];
    rsr_image sin[kMaxMerge], sout[kMaxMerge];
    for (int k = 0; k < n; k++)
    {
        pin[k] = packed_planes(v->d_pin + k * v->in.bytes(), v->in);
        pout[k] = packed_planes(v->d_pout + k * v->out.bytes(), v->out);
        sin[k] = rsr_image{v->d_in + v->slot(k) * v->in_surf, 0, 0};
        sout[k] = rsr_image{v->d_out + v->slot(k) * v->out_surf, 0, 0};
    }
    const rsr_image prev_in{v->d_in + v->prev * v->in_surf, 0, 0}, prev_out{v->d_out + v->prev * v->out_surf, 0, 0};
    if (const int rc = rsr_pack_planes(v->ctx, n, pin, sin, v->fmt, v->w, v->h, v->st)) return rc;
    if (const int rc = rsr_diff_tiles_sequence(v->ctx, n, sin, v->have_prev ? &prev_in : nullptr, v->fmt, v->w, v->h, 3, v->d_masks, v->st)) return rc;
    const size_t nmask = size_t(n) * size_t(v->ntiles);
    HIP_TRY(hipMemcpyAsync(v->h_masks, v->d_masks, nmask, hipMemcpyDeviceToHost, v->st));
    HIP_TRY(hipStreamSynchronize(v->st)); // the one host wait of a window: the grid of every launch depends on the masks
    if (const int rc = rsr_process_device_sequence(v->ctx, n, sin, v->fmt, v->w, v->h, 3, sout, v->fmt, v->have_prev ? &prev_out : nullptr, v->h_masks, int(nmask), v->st))
        return rc;
    if (const int rc = rsr_unpack_planes(v->ctx, n, sout, pout, v->fmt, v->ow, v->oh, v->st)) return rc;
    long long run = 0;
    for (size_t i = 0; i < nmask; i++) run += v->h_masks[i] != 0;
    {
        std::lock_guard<std::mutex> lk(e.mu);
        e.video_frames += n, e.video_windows++, e.video_tiles_run += run, e.video_tiles_skipped += (long long)nmask - run;
    }
    v->prev = v->slot(n - 1), v->have_prev = true;
    v->pending = 0, v->ready = n, v->first_ready = 0;
    return RSR_OK;
}

#pragma GCC visibility push(default)
extern "C" {

int rsr_video_open(rsr_ctx* ctx, int fmt, int w, int h, int window, rsr_video** out)
{
    if (out) *out = nullptr;
    if (!ctx || !out) return RSR_E_ARG;
    Engine& e = ctx->e;
    if (!pix_fmt(fmt).bits) return e.fail(RSR_E_ARG, "rsr_video_open: the format must be one of the YUV formats");
    if (window < 0 || window > RSR_SEQ_MAX) return e.fail(RSR_E_ARG, "rsr_video_open: window must be 0 (= 8) or 1 .. " + std::to_string(RSR_SEQ_MAX));
    if (window == 0) window = 8;
    rsr_video* v = nullptr;
    try
    {
        v = new rsr_video;
    }
    catch (const std::bad_alloc&)
    {
        return e.fail(RSR_E_NOMEM, "rsr_video_open: out of host memory");
    }
    v->ctx = ctx, v->fmt = fmt, v->w = w, v->h = h;
    {
        std::lock_guard<std::mutex> lk(e.mu);
        v->ratio = e.out_ratio, v->tilesize = e.tilesize;
    }
    int rc = rsr_image_bytes(fmt, w, h, 3) < 0 ? RSR_E_ARG : RSR_OK; // the size and parity rule of the input surface (rsr_image_bytes has set the message)
    if (rc == RSR_OK) rc = rsr_out_size_fmt(fmt, v->ratio.nx, v->ratio.dx, v->ratio.ny, v->ratio.dy, v->tilesize, w, h, &v->ow, &v->oh);
    if (rc == RSR_OK) rc = rsr_tile_count(w, h, v->tilesize, nullptr, nullptr);
    if (rc != RSR_OK)
    {
        delete v;
        return rc;
    }
    int nx = 0, ny = 0;
    (void)rsr_tile_count(w, h, v->tilesize, &nx, &ny);
    v->ntiles = nx * ny;
    v->in = plane_dims(fmt, w, h), v->out = plane_dims(fmt, v->ow, v->oh);
    v->in_surf = v->in.bytes(), v->out_surf = v->out.bytes(); // (a packed surface holds the samples of the planes: rsr_image_bytes)
    const hipError_t se = hipSetDevice(e.device);
    size_t free_b = 0, total_b = 0;
    if (se != hipSuccess || hipMemGetInfo(&free_b, &total_b) != hipSuccess)
    {
        (void)hipGetLastError();
        delete v;
        return e.fail(RSR_E_DEVICE, "rsr_video_open: hipMemGetInfo failed");
    }
    // window + 1 surfaces and `window` planar frames on each side, and the masks: lowered until they fit half of what is free now
    const auto need = [&](int win) { return (long long)(2 * win + 1) * (v->in_surf + v->out_surf) + (long long)win * v->ntiles; };
    while (window > 1 && need(window) > (long long)(free_b / 2)) window--;
    if (need(window) > (long long)(free_b / 2))
    {
        delete v;
        return e.fail(RSR_E_NOMEM, "rsr_video_open: one frame and its predecessor need " + std::to_string(need(1) >> 20) + " MiB, more than half of the free device memory");
    }
    v->window = window;
    const size_t slots = size_t(window) + 1, win = size_t(window);
    hipError_t he = hipStreamCreateWithFlags(&v->st, hipStreamNonBlocking);
    if (he != hipSuccess)
    {
        (void)hipGetLastError();
        v->st = nullptr;
        video_free(v);
        return e.fail(RSR_E_DEVICE, std::string("rsr_video_open: hipStreamCreateWithFlags: ") + hipGetErrorString(he));
    }
    if (he == hipSuccess) he = hipMalloc(reinterpret_cast<void**>(&v->d_in), slots * size_t(v->in_surf));
    if (he == hipSuccess) he = hipMalloc(reinterpret_cast<void**>(&v->d_out), slots * size_t(v->out_surf));
    if (he == hipSuccess) he = hipMalloc(reinterpret_cast<void**>(&v->d_pin), win * size_t(v->in_surf));
    if (he == hipSuccess) he = hipMalloc(reinterpret_cast<void**>(&v->d_pout), win * size_t(v->out_surf));
    if (he == hipSuccess) he = hipMalloc(reinterpret_cast<void**>(&v->d_masks), win * size_t(v->ntiles));
    if (he == hipSuccess) he = hipHostMalloc(reinterpret_cast<void**>(&v->h_in), win * size_t(v->in_surf), hipHostMallocDefault);
    if (he == hipSuccess) he = hipHostMalloc(reinterpret_cast<void**>(&v->h_out), size_t(v->out_surf), hipHostMallocDefault);
    if (he == hipSuccess) he = hipHostMalloc(reinterpret_cast<void**>(&v->h_masks), win * size_t(v->ntiles), hipHostMallocDefault);
    if (he != hipSuccess)
    {
        (void)hipGetLastError();
        video_free(v);
        return e.fail(RSR_E_NOMEM, std::string("rsr_video_open: ") + hipGetErrorString(he));
    }
    *out = v;
    return RSR_OK;
}

int rsr_video_send(rsr_video* v, const rsr_planes* frame)
{
    if (!v) return RSR_E_ARG;
    if (v->ready > 0) return Engine::fail(RSR_E_STATE, "rsr_video_send: " + std::to_string(v->ready) + " frames are waiting for rsr_video_receive");
    if (const int rc = check_geometry(v, "rsr_video_send")) return rc;
    long long yp = 0, cp = 0;
    if (const int rc = check_host_planes(v, frame, v->in, "rsr_video_send", &yp, &cp)) return rc;
    HIP_TRY(hipSetDevice(v->ctx->e.device));
    const PlaneDims& d = v->in;
    uint8_t* const dst = v->d_pin + v->pending * d.bytes();
    const rsr_planes dp = packed_planes(dst, d);
    const bool direct = is_pinned(frame->y, yp, d.yrow, d.rows) && is_pinned(frame->u, cp, d.crow, d.crows) && is_pinned(frame->v, cp, d.crow, d.crows);
    if (direct)
    { // pinned caller memory travels as it is; the caller owns it again when send returns
        HIP_TRY(hipMemcpy2DAsync(dp.y, size_t(d.yrow), frame->y, size_t(yp), size_t(d.yrow), size_t(d.rows), hipMemcpyHostToDevice, v->st));
        HIP_TRY(hipMemcpy2DAsync(dp.u, size_t(d.crow), frame->u, size_t(cp), size_t(d.crow), size_t(d.crows), hipMemcpyHostToDevice, v->st));
        HIP_TRY(hipMemcpy2DAsync(dp.v, size_t(d.crow), frame->v, size_t(cp), size_t(d.crow), size_t(d.crows), hipMemcpyHostToDevice, v->st));
        HIP_TRY(hipStreamSynchronize(v->st));
    }
    else
    { // pageable memory: row by row into the pinned staging of this window, one asynchronous copy from there
        uint8_t* const hs = v->h_in + v->pending * d.bytes();
        const rsr_planes hp = packed_planes(hs, d);
        for (int r = 0; r < d.rows; r++) std::memcpy(static_cast<uint8_t*>(hp.y) + r * d.yrow, static_cast<const uint8_t*>(frame->y) + r * yp, size_t(d.yrow));
        for (int r = 0; r < d.crows; r++)
        {
            std::memcpy(static_cast<uint8_t*>(hp.u) + r * d.crow, static_cast<const uint8_t*>(frame->u) + r * cp, size_t(d.crow));
            std::memcpy(static_cast<uint8_t*>(hp.v) + r * d.crow, static_cast<const uint8_t*>(frame->v) + r * cp, size_t(d.crow));
        }
        HIP_TRY(hipMemcpyAsync(dst, hs, size_t(d.bytes()), hipMemcpyHostToDevice, v->st));
    }
    v->pending++;
    return v->pending == v->window ? video_run(v) : RSR_OK;
}

int rsr_video_ready(rsr_video* v) { return v ? v->ready : RSR_E_ARG; }

int rsr_video_receive(rsr_video* v, const rsr_planes* frame)
{
    if (!v) return RSR_E_ARG;
    if (v->ready == 0) return Engine::fail(RSR_E_STATE, "rsr_video_receive: no frame is ready");
    long long yp = 0, cp = 0;
    if (const int rc = check_host_planes(v, frame, v->out, "rsr_video_receive", &yp, &cp)) return rc;
    HIP_TRY(hipSetDevice(v->ctx->e.device));
    const PlaneDims& d = v->out;
    uint8_t* const src = v->d_pout + v->first_ready * d.bytes();
    const rsr_planes sp = packed_planes(src, d);
    if (is_pinned(frame->y, yp, d.yrow, d.rows) && is_pinned(frame->u, cp, d.crow, d.crows) && is_pinned(frame->v, cp, d.crow, d.crows))
    {
        HIP_TRY(hipMemcpy2DAsync(frame->y, size_t(yp), sp.y, size_t(d.yrow), size_t(d.yrow), size_t(d.rows), hipMemcpyDeviceToHost, v->st));
        HIP_TRY(hipMemcpy2DAsync(frame->u, size_t(cp), sp.u, size_t(d.crow), size_t(d.crow), size_t(d.crows), hipMemcpyDeviceToHost, v->st));
        HIP_TRY(hipMemcpy2DAsync(frame->v, size_t(cp), sp.v, size_t(d.crow), size_t(d.crow), size_t(d.crows), hipMemcpyDeviceToHost, v->st));
        HIP_TRY(hipStreamSynchronize(v->st));
    }
    else
    {
        HIP_TRY(hipMemcpyAsync(v->h_out, src, size_t(d.bytes()), hipMemcpyDeviceToHost, v->st));
        HIP_TRY(hipStreamSynchronize(v->st));
        const rsr_planes hp = packed_planes(v->h_out, d);
        for (int r = 0; r < d.rows; r++) std::memcpy(static_cast<uint8_t*>(frame->y) + r * yp, static_cast<const uint8_t*>(hp.y) + r * d.yrow, size_t(d.yrow));
        for (int r = 0; r < d.crows; r++)
        {
            std::memcpy(static_cast<uint8_t*>(frame->u) + r * cp, static_cast<const uint8_t*>(hp.u) + r * d.crow, size_t(d.crow));
            std::memcpy(static_cast<uint8_t*>(frame->v) + r * cp, static_cast<const uint8_t*>(hp.v) + r * d.crow, size_t(d.crow));
        }
    }
    v->first_ready++, v->ready--;
    return RSR_OK;
}

int rsr_video_flush(rsr_video* v)
{
    if (!v) return RSR_E_ARG;
    if (v->pending == 0) return RSR_OK;
    if (v->ready > 0) return Engine::fail(RSR_E_STATE, "rsr_video_flush: " + std::to_string(v->ready) + " frames are waiting for rsr_video_receive");
    if (const int rc = check_geometry(v, "rsr_video_flush")) return rc;
    return video_run(v);
}

int rsr_video_reset(rsr_video* v)
{
    if (!v) return RSR_E_ARG;
    if (v->pending > 0) return Engine::fail(RSR_E_STATE, "rsr_video_reset: " + std::to_string(v->pending) + " frames are pending: flush first");
    v->have_prev = false; // (frames that are ready stay ready)
    return RSR_OK;
}

int rsr_video_info(rsr_video* v, int* ow, int* oh, int* window)
{
    if (!v) return RSR_E_ARG;
    if (ow) *ow = v->ow;
    if (oh) *oh = v->oh;
    if (window) *window = v->window;
    return RSR_OK;
}

void rsr_video_close(rsr_video* v) { video_free(v); }

} // extern "C"
#pragma GCC visibility pop
