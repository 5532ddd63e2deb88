// main.cpp -- command-line front end with the reference tool's surface
// (/root/reference/src/main.cpp:101-115 usage, :484-603 flags/validation, :605-659 path expansion, :661-693 model
// dir, :748-775 tile policy, :117-177/:190-416/:793-867 load -> proc -> save pipeline), re-implemented on
// std::thread + the C-ABI engine.  SURVEY.md 8(f-1).  Differences, all deliberate:
//   * -g ids are HIP devices; "-g -1" (ncnn CPU path) is refused: this build has no CPU fallback;
//   * the model is parsed + packed ONCE and reaches the GPUs of "-g 0,1,.." by one RCCL broadcast (rsr_create_group; the
//     reference re-reads x4.bin per GPU, main.cpp:784-786);
//   * a single input image with several GPUs is split by tile rows over all of them (rsr_process_group); directories are
//     dealt image by image from the shared queue exactly like the reference (main.cpp:811-828);
//   * codecs: stb_image / stb_image_write as in the reference (jpg, png, ... in; png, jpg out) + binary pnm; webp in / lossless
//     webp out through the system's libwebp, bound at run time (webp_dl.h) -- without it webp files fail like a broken image;
//   * "-j l:p:s" accepts a single proc count for several GPUs (the reference insists on one per GPU);
//   * RSR_DEPTH=16|auto (no counterpart: the reference is 8-bit throughout): 16-bit PNG / PNM in, 16-bit PNG out through
//     rsr_process_fmt (RSR_FMT_U16_HWC); unset or 8, every byte of the 8-bit route is what it was;
//   * RSR_ALPHA=net (no counterpart): the alpha of an RGBA image walks the network as a gray image (rsr_set_option "alpha_net") instead
//     of taking the bicubic; an image whose alpha is fully opaque keeps the bicubic and its one pass; RSR_ALPHA=adaptive: the library
//     decides per tile (rsr_set_option "alpha_adaptive"): tiles of constant alpha keep the bicubic, the others go through the network;
//   * RSR_BLEND=<model-dir>:<t> (no counterpart): beside -m, a second model of the same depth and a strength t in [0, 1]; every context
//     loads it (rsr_load_second) and runs on the weights (1 - t) * <-m model> + t * <model-dir> (rsr_set_blend): network interpolation,
//     e.g. -m models-DF2K with RSR_BLEND=models-DF2K_JPEG:0.4;
//   * RSR_DITHER=1 (no counterpart): the colour samples of every integer output -- 8- and 16-bit images, Y4M frames -- are rounded against
//     the library's position-keyed threshold instead of 0.5 (rsr_set_option "dither"): gradients leave as fine static noise, not as bands;
//   * video mode (no counterpart): an input that ends in .y4m, or is "-" (stdin), is a YUV4MPEG2 stream and runs through one rsr_video
//     session to a .y4m output or "-" (stdout) -- run_video below, y4m_io.h.
#include <dirent.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <queue>
#include <string>
#include <thread>
#include <vector>

#include "image_io.h"
#include "realsr.h"
#include "y4m_io.h"

static void print_usage()
{
    fprintf(stderr, "Usage: realsr-hip -i infile -o outfile [options]...\n\n");
    fprintf(stderr, "  -h                   show this help\n");
    fprintf(stderr, "  -v                   verbose output\n");
    fprintf(stderr, "  -i input-path        input image path (jpg/png/pnm) or directory; a YUV4MPEG2 stream: file.y4m, or - for stdin\n");
    fprintf(stderr, "  -o output-path       output image path (jpg/png) or directory; for a YUV4MPEG2 input: file.y4m, or - for stdout\n");
    fprintf(stderr, "  -s scale             upscale ratio (4, default=4)\n");
    fprintf(stderr, "  -t tile-size         tile size (>=32/0=auto, default=0) can be 0,0,0 for multi-gpu\n");
    fprintf(stderr, "  -m model-path        realsr model path (default=models-DF2K_JPEG)\n");
    fprintf(stderr, "  -g gpu-id            gpu device to use (default=0) can be 0,1,2 for multi-gpu\n");
    fprintf(stderr, "  -j load:proc:save    thread count for load/proc/save (default=1:2:2) can be 1:2,2,2:2 for multi-gpu\n");
    fprintf(stderr, "  -x                   enable tta mode\n");
    fprintf(stderr, "  -f format            output image format (jpg/png/webp, default=ext/png)\n");
    fprintf(stderr, "\nenvironment:\n");
    fprintf(stderr, "  RSR_DEPTH=8|16|auto  sample depth (default=8): 16 = every image runs as 16-bit RGB(A) and is written as a 16-bit .png\n");
    fprintf(stderr, "                       (8-bit sources widened by x257); auto = 16-bit png/pnm inputs with a .png output keep their 16 bits\n");
    fprintf(stderr, "  RSR_ALPHA=net|bicubic alpha of RGBA images (default=bicubic): net = through the network as a gray image, about twice the\n");
    fprintf(stderr, "                       time; a fully opaque alpha stays opaque and costs one pass\n");
    fprintf(stderr, "  RSR_DITHER=0|1       ordered dither of the integer outputs (default=0): 1 = colour samples of 8- / 16-bit images and Y4M\n");
    fprintf(stderr, "                       frames are rounded against a position-keyed threshold, so smooth gradients do not band\n");
    fprintf(stderr, "  RSR_BLEND=dir:t      a second model directory of the same depth and a strength t in [0, 1]: the weights are\n");
    fprintf(stderr, "                       (1 - t) * the -m model + t * the model of dir (network interpolation)\n");
}

static std::vector<int> parse_int_list(const char* s)
{
    std::vector<int> v;
    while (s && *s)
    {
        char* e = nullptr;
        const long n = std::strtol(s, &e, 10);
        if (e == s) break;
        v.push_back(int(n));
        s = (*e == ',') ? e + 1 : e;
        if (*e != ',') break;
    }
    return v;
}

static bool is_dir(const std::string& p)
{
    struct stat st;
    return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}
static bool exists(const std::string& p)
{
    struct stat st;
    return stat(p.c_str(), &st) == 0;
}
static int list_files(const std::string& dir, std::vector<std::string>& names)
{
    DIR* d = opendir(dir.c_str());
    if (!d)
    {
        fprintf(stderr, "opendir failed %s\n", dir.c_str());
        return -1;
    }
    while (dirent* e = readdir(d))
    {
        if (e->d_type == DT_REG || (e->d_type == DT_UNKNOWN && !is_dir(dir + "/" + e->d_name))) names.push_back(e->d_name);
    }
    closedir(d);
    std::sort(names.begin(), names.end());
    return 0;
}
static std::string strip_ext(const std::string& n)
{
    const size_t dot = n.find_last_of('.');
    return dot == std::string::npos ? n : n.substr(0, dot);
}
static std::string exe_dir()
{
    char buf[4096];
    const ssize_t n = readlink("/proc/self/exe", buf, sizeof buf - 1);
    if (n <= 0) return ".";
    buf[n] = 0;
    std::string p(buf);
    const size_t s = p.find_last_of('/');
    return s == std::string::npos ? "." : p.substr(0, s);
}
// relative model paths fall back to the executable's directory (filesystem_utils.h:167-173)
static std::string sanitize_filepath(const std::string& p)
{
    if (p.empty() || p[0] == '/' || exists(p)) return p;
    return exe_dir() + "/" + p;
}

struct Task
{
    int id = 0;
    std::string inpath, outpath;
    Image inimage, outimage;
    bool opaque = false; // RSR_ALPHA=net: an RGBA image whose alpha samples all hold the maximum (it runs with "alpha_net" 0)
};

// Do all alpha samples of an RGBA image hold the maximum of its depth (255 / 65535)?  One pass over the decoded image on the host.
static bool alpha_all_max(const Image& im)
{
    if (im.elempack != 4) return false;
    const size_t n = size_t(im.w) * size_t(im.h);
    if (im.depth == 16)
    {
        const uint16_t* p = im.data16();
        for (size_t i = 0; i < n; i++)
            if (p[4 * i + 3] != 65535) return false;
    }
    else
    {
        const uint8_t* p = im.data();
        for (size_t i = 0; i < n; i++)
            if (p[4 * i + 3] != 255) return false;
    }
    return true;
}

class TaskQueue // bounded at 8 like the reference (main.cpp:141)
{
public:
    void put(std::unique_ptr<Task> t)
    {
        std::unique_lock<std::mutex> lk(mu);
        not_full.wait(lk, [&] { return q.size() < 8; });
        q.push(std::move(t));
        not_empty.notify_one();
    }
    std::unique_ptr<Task> get()
    {
        std::unique_lock<std::mutex> lk(mu);
        not_empty.wait(lk, [&] { return !q.empty(); });
        std::unique_ptr<Task> t = std::move(q.front());
        q.pop();
        not_full.notify_one();
        return t;
    }

private:
    std::mutex mu;
    std::condition_variable not_full, not_empty;
    std::queue<std::unique_ptr<Task>> q;
};

static const int kEnd = -233; // same sentinel id as main.cpp:322,350

// ---- video mode: a YUV4MPEG2 stream through one rsr_video session ---------------------------------------------------------------------
static bool is_y4m_path(const std::string& p) { return p == "-" || imgio::lower_ext(p) == "y4m"; }

// An integer from the environment, or `fallback` where the variable is not set (or is no number).
static long long env_int(const char* name, long long fallback)
{
    const char* e = getenv(name);
    if (!e || !*e) return fallback;
    char* end = nullptr;
    const long long v = std::strtoll(e, &end, 10);
    return end && *end == 0 ? v : fallback;
}

// The C tag picks the format and the chroma siting, XCOLORRANGE the range; RSR_YUV_MATRIX / RSR_YUV_RANGE / RSR_YUV_SITING override
// (matrix: the library's 709 unless said).  The context comes configured (tile size, output ratio, TTA, precise).  Every complete
// frame of the input is written, also in front of a stream that is cut inside a frame -- which then ends with exit code 1.
static int run_video(rsr_ctx* ctx, const std::string& inpath, const std::string& outpath, int nx, int dx, int ny, int dy, int verbose)
{
    FILE* fi = inpath == "-" ? stdin : fopen(inpath.c_str(), "rb");
    if (!fi)
    {
        fprintf(stderr, "cannot open %s\n", inpath.c_str());
        return 1;
    }
    y4m::Header hd;
    std::string line;
    const int lrc = y4m::read_line(fi, line);
    std::string err = lrc == 0 ? y4m::parse_header(line, hd) : lrc == 1 ? std::string("empty input") : std::string("header line without a newline within 256 bytes");
    if (!err.empty())
    {
        fprintf(stderr, "%s: %s\n", inpath.c_str(), err.c_str());
        return 1;
    }
    const long long siting = env_int("RSR_YUV_SITING", hd.siting >= 0 ? hd.siting : 0), range = env_int("RSR_YUV_RANGE", hd.range >= 0 ? hd.range : 0);
    if (rsr_set_option(ctx, "yuv_matrix", env_int("RSR_YUV_MATRIX", 709)) != RSR_OK || rsr_set_option(ctx, "yuv_range", range) != RSR_OK ||
        rsr_set_option(ctx, "yuv_siting", siting) != RSR_OK)
    {
        fprintf(stderr, "invalid RSR_YUV_MATRIX / RSR_YUV_RANGE / RSR_YUV_SITING: %s\n", rsr_last_error(ctx));
        return 1;
    }
    rsr_video* v = nullptr;
    if (rsr_video_open(ctx, hd.fmt, hd.w, hd.h, int(env_int("RSR_VIDEO_WINDOW", 0)), &v) != RSR_OK)
    {
        fprintf(stderr, "%s: %s\n", inpath.c_str(), rsr_last_error(ctx));
        return 1;
    }
    int ow = 0, oh = 0, window = 0;
    rsr_video_info(v, &ow, &oh, &window);
    FILE* fo = outpath == "-" ? stdout : fopen(outpath.c_str(), "wb");
    if (!fo)
    {
        fprintf(stderr, "cannot open %s\n", outpath.c_str());
        rsr_video_close(v);
        return 1;
    }
    if (verbose) fprintf(stderr, "video: %d x %d -> %d x %d, windows of %d frames, yuv_range %lld, yuv_siting %lld\n", hd.w, hd.h, ow, oh, window, range, siting);
    const std::string head = y4m::format_header(hd, ow, oh, nx, dx, ny, dy);
    bool ok = fwrite(head.data(), 1, head.size(), fo) == head.size();
    const size_t es = size_t(y4m::sample_bytes(hd.fmt));
    const auto planes_of = [&](unsigned char* base, int w, int h) {
        rsr_planes p;
        const size_t ybytes = es * size_t(w) * size_t(h), cbytes = es * size_t(w >> y4m::chroma_shift_x(hd.fmt)) * size_t(h >> y4m::chroma_shift_y(hd.fmt));
        p.y = base, p.u = base + ybytes, p.v = base + ybytes + cbytes, p.y_pitch = 0, p.c_pitch = 0;
        return p;
    };
    std::vector<unsigned char> in, out(y4m::frame_bytes(hd.fmt, ow, oh));
    std::queue<std::string> params; // the FRAME lines of the frames in flight, in order
    double run0 = 0, skip0 = 0;
    rsr_get_stat(ctx, "video_tiles_run", &run0);
    rsr_get_stat(ctx, "video_tiles_skipped", &skip0);
    long long frames = 0;
    // hand out what is ready; one line per window under -v
    const auto drain = [&]() {
        const int n = rsr_video_ready(v);
        if (n > 0 && verbose)
        {
            double run = 0, skip = 0;
            rsr_get_stat(ctx, "video_tiles_run", &run);
            rsr_get_stat(ctx, "video_tiles_skipped", &skip);
            fprintf(stderr, "window: %d frames, %.0f tiles run, %.0f skipped\n", n, run - run0, skip - skip0);
            run0 = run, skip0 = skip;
        }
        while (ok && rsr_video_ready(v) > 0)
        {
            const rsr_planes op = planes_of(out.data(), ow, oh);
            if (rsr_video_receive(v, &op) != RSR_OK)
            {
                fprintf(stderr, "%s\n", rsr_last_error(ctx));
                ok = false;
                break;
            }
            ok = y4m::write_frame(fo, params.front(), out.data(), out.size());
            if (!ok) fprintf(stderr, "write to %s failed\n", outpath.c_str());
            params.pop();
            frames++;
        }
    };
    int rc = 0;
    while (ok)
    {
        std::string fl;
        const int fr = y4m::read_frame(fi, hd, in, fl, err);
        if (fr <= 0)
        { // the end, clean or not: what is pending still runs and is written
            if (rsr_video_flush(v) != RSR_OK)
            {
                fprintf(stderr, "%s\n", rsr_last_error(ctx));
                ok = false;
            }
            else drain();
            if (fr < 0)
            {
                fprintf(stderr, "%s: %s (after %lld complete frames)\n", inpath.c_str(), err.c_str(), frames);
                rc = 1;
            }
            break;
        }
        params.push(fl);
        const rsr_planes ip = planes_of(in.data(), hd.w, hd.h);
        if (rsr_video_send(v, &ip) != RSR_OK)
        {
            fprintf(stderr, "%s\n", rsr_last_error(ctx));
            ok = false;
            break;
        }
        drain();
    }
    rsr_video_close(v);
    if (fo != stdout) ok = fclose(fo) == 0 && ok;
    else fflush(fo);
    if (fi != stdin) fclose(fi);
    if (verbose) fprintf(stderr, "%s -> %s done: %lld frames\n", inpath.c_str(), outpath.c_str(), frames);
    return ok ? rc : 1;
}

int main(int argc, char** argv)
{
    std::string inputpath, outputpath, model = "models-DF2K_JPEG", format = "png";
    int scale = 4, jobs_load = 1, jobs_save = 2, verbose = 0, tta_mode = 0;
    std::vector<int> tilesize, gpuid, jobs_proc;

    int opt;
    while ((opt = getopt(argc, argv, "i:o:s:t:m:g:j:f:vxh")) != -1)
    {
        switch (opt)
        {
        case 'i': inputpath = optarg; break;
        case 'o': outputpath = optarg; break;
        case 's': scale = atoi(optarg); break;
        case 't': tilesize = parse_int_list(optarg); break;
        case 'm': model = optarg; break;
        case 'g': gpuid = parse_int_list(optarg); break;
        case 'j':
        {
            const char* c1 = strchr(optarg, ':');
            const char* c2 = c1 ? strchr(c1 + 1, ':') : nullptr;
            if (!c1 || !c2)
            {
                fprintf(stderr, "invalid thread count argument\n");
                return -1;
            }
            jobs_load = atoi(optarg);
            jobs_proc = parse_int_list(c1 + 1);
            jobs_save = atoi(c2 + 1);
            break;
        }
        case 'f': format = optarg; break;
        case 'v': verbose = 1; break;
        case 'x': tta_mode = 1; break;
        case 'h':
        default: print_usage(); return -1;
        }
    }
    if (inputpath.empty() || outputpath.empty())
    {
        print_usage();
        return -1;
    }
    if (scale != 4)
    {
        fprintf(stderr, "invalid scale argument\n");
        return -1;
    }
    // RSR_OUT_SCALE=1|2|4 (no flag of the reference's surface is taken for it; -s stays the MODEL's scale): the size of the output
    // image relative to the input -- the x4 result box-reduced on the device (rsr_set_option "out_scale") --, or n/d (3/2, 4/3, 9/4,
    // 3/1 ...: rsr_set_out_ratio, area-averaged on the device).  A single number other than 1, 2 and 4 stays refused: x3 is written 3/1.
    // RSR_OUT_SCALE=8/3,9/4 gives a ratio per axis, x then y (rsr_set_out_ratio_xy: 720 x 480 -> 1920 x 1080), each member n/d or a whole
    // number, d in 1..8; a value without a comma is parsed exactly as above.
    int out_scale = 4, out_num = 4, out_den = 1, out_num_y = 0, out_den_y = 0; // out_den_y 0: one ratio on both axes
    if (const char* oe = getenv("RSR_OUT_SCALE"))
    {
        const std::string v(oe);
        int n = 0, d = 0, ow = 0, oh = 0;
        char tail = 0;
        const size_t comma = v.find(',');
        auto member = [](const std::string& m, int* mn, int* md) { // "n/d" or "n", digits only
            char t = 0;
            if (m.empty() || m.size() > 9 || m.find_first_not_of("0123456789/") != std::string::npos) return false;
            if (m.find('/') == std::string::npos) { *md = 1; return sscanf(m.c_str(), "%d%c", mn, &t) == 1; }
            return sscanf(m.c_str(), "%d/%d%c", mn, md, &t) == 2;
        };
        if (comma != std::string::npos)
        {
            int ny = 0, dy = 0;
            if (v.find(',', comma + 1) == std::string::npos && member(v.substr(0, comma), &n, &d) && member(v.substr(comma + 1), &ny, &dy) &&
                rsr_out_size_xy(n, d, ny, dy, 840, 840, 840, &ow, &oh) == RSR_OK) // (840: every permitted d divides it, so the pair alone is judged)
            {
                out_num = n, out_den = d, out_num_y = ny, out_den_y = dy;
                out_scale = 0; // the library itself takes equal box members back to out_scale
            }
            else
            {
                fprintf(stderr, "invalid RSR_OUT_SCALE '%s' (x,y: each n/d or n with d in 1..8 and 1 <= n/d <= 4)\n", oe);
                return -1;
            }
        }
        else if (v == "1" || v == "2" || v == "4") out_num = out_scale = v[0] - '0';
        else if (v.find('/') != std::string::npos && v.find_first_not_of("0123456789/") == std::string::npos && sscanf(oe, "%d/%d%c", &n, &d, &tail) == 2 &&
                 rsr_out_size(n, d, 12, 12, 12, &ow, &oh) == RSR_OK) // (12: every permitted d divides it, so the ratio alone is judged)
        {
            out_num = n, out_den = d;
            out_scale = (n == 4 * d || n == 2 * d || n == d) ? n / d : 0; // 4/1, 2/1, 1/1 are the box scales; 0 = another ratio
        }
        else
        {
            fprintf(stderr, "invalid RSR_OUT_SCALE '%s' (1, 2 or 4, or n/d with d in 1..4 and 1 <= n/d <= 4)\n", oe);
            return -1;
        }
    }
    // RSR_DEPTH=8|16|auto (no flag of the reference's surface is taken for it, like RSR_OUT_SCALE): the sample depth of the still-image
    // route.  8 / unset: what it always was.  16: every image runs U16 -> U16 (an 8-bit source widened by x257: the same network input) and
    // is written as a 16-bit PNG.  auto: a 16-bit PNG / PNM input whose output is a .png takes the 16-bit route, everything else the 8-bit one.
    enum { kDepth8, kDepth16, kDepthAuto } depth_mode = kDepth8;
    if (const char* de = getenv("RSR_DEPTH"))
    {
        const std::string v(de);
        if (v == "16") depth_mode = kDepth16;
        else if (v == "auto") depth_mode = kDepthAuto;
        else if (!v.empty() && v != "8")
        {
            fprintf(stderr, "invalid RSR_DEPTH '%s' (8, 16 or auto)\n", de);
            return -1;
        }
    }
    // RSR_ALPHA=net|bicubic (no flag of the reference's surface is taken for it): how the alpha of an RGBA image is made.  bicubic / unset:
    // ncnn's bicubic x4, as ever.  net: the alpha walks the network as a gray image (rsr_set_option "alpha_net": a second pass over the
    // image's tiles, about twice the time) -- except for an image whose alpha is fully opaque, the usual opaque PNG saved as RGBA, which
    // keeps its opaque alpha and its one pass.  On the 8-bit and the RSR_DEPTH 16-bit route alike.
    // adaptive: "alpha_net" 1 and "alpha_adaptive" 1, set ONCE per context: the library skips the alpha pass tile by tile wherever a tile's
    // source rectangle holds one alpha value (an opaque image: everywhere), so no image needs an option of its own.
    bool alpha_net = false, alpha_adaptive = false;
    if (const char* ae = getenv("RSR_ALPHA"))
    {
        const std::string v(ae);
        if (v == "net") alpha_net = true;
        else if (v == "adaptive") alpha_adaptive = true;
        else if (!v.empty() && v != "bicubic")
        {
            fprintf(stderr, "invalid RSR_ALPHA '%s' (net, adaptive or bicubic)\n", ae);
            return -1;
        }
    }
    // RSR_DITHER=0|1 (no flag of the reference's surface is taken for it): option "dither" of every context, set ONCE below -- the 8-bit and
    // the RSR_DEPTH 16-bit image routes and the Y4M route alike.  Anything else is refused here, before any GPU work.
    bool dither = false;
    if (const char* di = getenv("RSR_DITHER"))
    {
        const std::string v(di);
        if (v == "1") dither = true;
        else if (!v.empty() && v != "0")
        {
            fprintf(stderr, "invalid RSR_DITHER '%s' (0 or 1)\n", di);
            return -1;
        }
    }
    // RSR_BLEND=<model-dir>:<t> (no flag of the reference's surface is taken for it): network interpolation between the -m model and the
    // one of <model-dir>, t a plain decimal in [0, 1] behind the LAST colon (digits with at most one point: no sign, no exponent, no blanks).
    std::string blend_dir, blend_text;
    float blend_t = 0.f;
    const char* be = getenv("RSR_BLEND");
    if (be && *be) // (empty is unset, as for RSR_ALPHA)
    {
        const std::string v(be);
        const size_t colon = v.rfind(':');
        bool ok = colon != std::string::npos && colon > 0 && colon + 1 < v.size();
        if (ok)
        {
            blend_dir = v.substr(0, colon), blend_text = v.substr(colon + 1);
            size_t digits = 0, points = 0;
            for (char ch : blend_text)
                if (ch >= '0' && ch <= '9') digits++;
                else if (ch == '.') points++;
                else ok = false;
            ok = ok && digits >= 1 && points <= 1 && blend_text.size() <= 32;
            if (ok) blend_t = std::strtof(blend_text.c_str(), nullptr);
            ok = ok && blend_t >= 0.f && blend_t <= 1.f;
        }
        if (!ok)
        {
            fprintf(stderr, "invalid RSR_BLEND '%s' (<model-dir>:<t>, t a decimal in [0, 1], e.g. models-DF2K_JPEG:0.4)\n", be);
            return -1;
        }
    }
    if (gpuid.empty()) gpuid.push_back(0);
    const int ngpu = int(gpuid.size());
    const bool video = is_y4m_path(inputpath) && !is_dir(inputpath); // a YUV4MPEG2 stream: one session on one GPU
    if (video && (!is_y4m_path(outputpath) || is_dir(outputpath)))
    {
        fprintf(stderr, "a YUV4MPEG2 input needs a .y4m output path or - (stdout)\n");
        return -1;
    }
    if (video && ngpu > 1)
    {
        fprintf(stderr, "a YUV4MPEG2 stream runs on one gpu\n");
        return -1;
    }
    for (int g : gpuid)
        if (g < 0)
        {
            fprintf(stderr, "invalid gpu device %d (the ncnn cpu path '-g -1' does not exist in this build: no CPU fallback)\n", g);
            return -1;
        }
    if (!tilesize.empty() && int(tilesize.size()) != ngpu)
    {
        fprintf(stderr, "invalid tilesize argument\n");
        return -1;
    }
    for (int t : tilesize)
        if (t != 0 && t < 32)
        {
            fprintf(stderr, "invalid tilesize argument\n");
            return -1;
        }
    if (jobs_load < 1 || jobs_save < 1)
    {
        fprintf(stderr, "invalid thread count argument\n");
        return -1;
    }
    if (jobs_proc.size() == 1 && ngpu > 1) jobs_proc.assign(size_t(ngpu), jobs_proc[0]);
    if (!jobs_proc.empty() && int(jobs_proc.size()) != ngpu)
    {
        fprintf(stderr, "invalid jobs_proc thread count argument\n");
        return -1;
    }
    for (int j : jobs_proc)
        if (j < 1)
        {
            fprintf(stderr, "invalid jobs_proc thread count argument\n");
            return -1;
        }
    if (!video && !is_dir(outputpath))
    {
        const std::string ext = imgio::lower_ext(outputpath); // format guessed from the output path, whatever -f says
        if (ext == "png") format = "png";
        else if (ext == "webp") format = "webp";
        else if (ext == "jpg" || ext == "jpeg") format = "jpg";
        else
        {
            fprintf(stderr, "invalid outputpath extension type\n");
            return -1;
        }
    }
    if (format != "png" && format != "webp" && format != "jpg")
    {
        fprintf(stderr, "invalid format argument\n");
        return -1;
    }
    if (depth_mode == kDepth16 && !video && format != "png")
    { // (before any GPU work: nothing but PNG holds 16-bit samples here)
        fprintf(stderr, "RSR_DEPTH=16 writes 16-bit images, which only .png holds: give a .png output path or -f png, not %s\n", format.c_str());
        return -1;
    }
    if (format == "webp" && !webpdl::api().error.empty())
    {
        fprintf(stderr, "%s\n", webpdl::api().error.c_str());
        return -1;
    }

    // collect input and output file paths
    std::vector<std::string> input_files, output_files;
    if (video) input_files.push_back(inputpath), output_files.push_back(outputpath); // (one stream: run_video opens it)
    else if (is_dir(inputpath) && is_dir(outputpath))
    {
        std::vector<std::string> names;
        if (list_files(inputpath, names) != 0) return -1;
        std::string last, last_noext;
        for (const std::string& fn : names)
        {
            const std::string noext = strip_ext(fn);
            std::string outname = noext + "." + format;
            if (noext == last_noext) // sorted list: two inputs would write the same output (main.cpp:625-637)
            {
                const std::string out2 = fn + "." + format;
                fprintf(stderr, "both %s and %s output %s ! %s will output %s\n", fn.c_str(), last.c_str(), outname.c_str(), fn.c_str(), out2.c_str());
                outname = out2;
            }
            else
            {
                last = fn;
                last_noext = noext;
            }
            input_files.push_back(inputpath + "/" + fn);
            output_files.push_back(outputpath + "/" + outname);
        }
    }
    else if (!is_dir(inputpath) && !is_dir(outputpath))
    {
        input_files.push_back(inputpath);
        output_files.push_back(outputpath);
    }
    else
    {
        fprintf(stderr, "inputpath and outputpath must be either file or directory at the same time\n");
        return -1;
    }

    int prepadding = 0;
    if (model.find("models-DF2K") != std::string::npos) prepadding = 10; // also matches models-DF2K_JPEG
    else
    {
        fprintf(stderr, "unknown model dir type\n");
        return -1;
    }
    const std::string parampath = sanitize_filepath(model + "/x4.param");
    const std::string modelpath = sanitize_filepath(model + "/x4.bin");
    // RSR_BLEND: both models are read on the host first -- a missing directory, a file that is no model, two depths: refused before any GPU work
    const std::string blend_param = blend_dir.empty() ? std::string() : sanitize_filepath(blend_dir + "/x4.param");
    const std::string blend_model = blend_dir.empty() ? std::string() : sanitize_filepath(blend_dir + "/x4.bin");
    int blend_blocks = 0;
    if (!blend_dir.empty())
    {
        int convs_a = 0, convs_b = 0;
        if (!is_dir(blend_dir) || rsr_model_info(blend_param.c_str(), blend_model.c_str(), nullptr, &convs_b, nullptr, nullptr, nullptr) != RSR_OK)
        {
            fprintf(stderr, "RSR_BLEND: %s holds no model: %s\n", blend_dir.c_str(), is_dir(blend_dir) ? rsr_last_error(nullptr) : "no such directory");
            return -1;
        }
        if (rsr_model_info(parampath.c_str(), modelpath.c_str(), nullptr, &convs_a, nullptr, nullptr, nullptr) != RSR_OK)
        {
            fprintf(stderr, "model load failed: %s\n", rsr_last_error(nullptr));
            return -1;
        }
        if (convs_a != convs_b)
        {
            fprintf(stderr, "RSR_BLEND: %s has %d RRDB blocks, %s has %d: only models of one depth can be blended\n", blend_dir.c_str(), (convs_b - 6) / 15, model.c_str(), (convs_a - 6) / 15);
            return -1;
        }
        blend_blocks = (convs_b - 6) / 15;
    }

    if (jobs_proc.empty()) jobs_proc.assign(size_t(ngpu), 2);
    if (tilesize.empty()) tilesize.assign(size_t(ngpu), 0);
    for (size_t i = 0; i < tilesize.size(); i++)
    {
        if (tilesize[i] != 0) continue;
        // the reference's policy on the device's free memory in MB (main.cpp:761-774); an idle MI355X always lands on 200
        long long budget = 0;
        if (rsr_device_memory(gpuid[i], &budget, nullptr) != RSR_OK)
        {
            fprintf(stderr, "%s\n", rsr_last_error(nullptr));
            return -1;
        }
        tilesize[i] = budget > 1900 ? 200 : budget > 550 ? 100 : budget > 190 ? 64 : 32;
    }

    // one context per GPU: parsed + packed once, one RCCL broadcast (rsr_create_group)
    std::vector<rsr_ctx*> ctxs(size_t(ngpu), nullptr);
    if (rsr_create_group(ctxs.data(), gpuid.data(), ngpu, tta_mode, parampath.c_str(), modelpath.c_str()) != RSR_OK)
    {
        fprintf(stderr, "model load failed: %s\n", rsr_last_error(nullptr));
        return -1;
    }
    if (verbose && ngpu > 1) fprintf(stderr, "weights reached %d gpus by: %s\n", ngpu, rsr_group_transport());
    if (!blend_dir.empty())
    { // every context gets the pair and the strength (rsr_process_group insists that they agree)
        for (int i = 0; i < ngpu; i++)
            if (rsr_load_second(ctxs[size_t(i)], blend_param.c_str(), blend_model.c_str()) != RSR_OK || rsr_set_blend(ctxs[size_t(i)], blend_t) != RSR_OK)
            {
                fprintf(stderr, "RSR_BLEND: gpu %d: %s\n", gpuid[size_t(i)], rsr_last_error(ctxs[size_t(i)]));
                return -1;
            }
        if (verbose) fprintf(stderr, "blend %s of %s (%d blocks)\n", blend_text.c_str(), blend_dir.c_str(), blend_blocks);
    }
    std::vector<std::unique_ptr<RealSR>> realsr;
    for (int i = 0; i < ngpu; i++)
    {
        std::unique_ptr<RealSR> r(new RealSR(ctxs[size_t(i)]));
        r->scale = scale;
        r->tilesize = tilesize[size_t(i)];
        r->prepadding = prepadding;
        r->out_scale = out_scale ? out_scale : 4;
        double model_blocks = 0, model_convs = 0; // the depth of the model that was loaded (stats "model_blocks" / "model_convs")
        rsr_get_stat(ctxs[size_t(i)], "model_blocks", &model_blocks);
        rsr_get_stat(ctxs[size_t(i)], "model_convs", &model_convs);
        const int nconv = int(model_convs);
        if (verbose) fprintf(stderr, "gpu %d: model: %d blocks, %d convolutions\n", gpuid[size_t(i)], int(model_blocks), nconv);
        if (!out_scale) r->out_num = out_num, r->out_den = out_den, r->out_num_y = out_num_y, r->out_den_y = out_den_y;
        if (verbose && out_scale) fprintf(stderr, "gpu %d: output scale %d%s\n", gpuid[size_t(i)], out_scale, out_scale == 4 ? "" : " (RSR_OUT_SCALE: the x4 result box-reduced)");
        if (verbose && !out_scale && !out_den_y) fprintf(stderr, "gpu %d: output scale %d/%d (RSR_OUT_SCALE: the x4 result area-averaged)\n", gpuid[size_t(i)], out_num, out_den);
        if (verbose && out_den_y) fprintf(stderr, "gpu %d: output scale %d/%d along x, %d/%d along y (RSR_OUT_SCALE: the x4 result area-averaged)\n", gpuid[size_t(i)], out_num, out_den, out_num_y, out_den_y);
        // the reference prints one line per tile, "%.2f%%" of (yi * xtiles + xi) / (ytiles * xtiles) (realsr.cpp:481): the same lines
        // here, one per tile of every batch (a batch of tiles runs at once, so they arrive in bursts)
        rsr_set_progress_callback(ctxs[size_t(i)], [](int done, int total, void*) { fprintf(stderr, "%.2f%%\n", total ? 100.f * float(done - 1) / float(total) : 0.f); }, nullptr);
        // every proc thread of this GPU may have a call in flight (small images of concurrent calls are merged into one tile batch: the
        // reference's "-j 4:4:4 for many small images", README.md:61 -- here the more proc threads, the fuller the launches)
        rsr_set_option(ctxs[size_t(i)], "max_lanes", std::max(16, std::min(64, jobs_proc[size_t(i)])));
        if (alpha_adaptive)
        { // RSR_ALPHA=adaptive: the same for every image of this context
            rsr_set_option(ctxs[size_t(i)], "alpha_net", 1);
            rsr_set_option(ctxs[size_t(i)], "alpha_adaptive", 1);
        }
        if (dither)
        { // RSR_DITHER=1: the same for every image and frame of this context
            rsr_set_option(ctxs[size_t(i)], "dither", 1);
            if (verbose) fprintf(stderr, "gpu %d: ordered dither of the integer outputs (RSR_DITHER)\n", gpuid[size_t(i)]);
        }
        // no flag of the reference's surface is taken for it: RSR_PRECISE=1 keeps a byte of rounding residue per element of the residual
        // trunk (rsr_set_option "precise"; what tools/check_real_model.py recommends for weights with a wide output swing)
        // RSR_PRECISE_AUTO=1: the loaded model decides (rsr_set_option "precise_auto": one built-in tile through both storages on the
        // device, precise when fp16 storage leaves less than 1.5 x headroom to the +-1 bar).  RSR_PRECISE, when also set, wins.
        const char* pa = getenv("RSR_PRECISE_AUTO");
        const bool precise_auto = pa && pa[0] && pa[0] != '0';
        const char* pe = getenv("RSR_PRECISE");
        bool auto_ok = false;
        if (precise_auto)
        {
            if (rsr_set_option(ctxs[size_t(i)], "precise_auto", 1) != RSR_OK)
                fprintf(stderr, "gpu %d: model self-check failed: %s\n", gpuid[size_t(i)], rsr_last_error(ctxs[size_t(i)]));
            else
                auto_ok = true;
            if (pe) rsr_set_option(ctxs[size_t(i)], "precise", (pe[0] && pe[0] != '0') ? 1 : 0);
        }
        else if (pe && pe[0] && pe[0] != '0')
        {
            rsr_set_option(ctxs[size_t(i)], "precise", 1);
            if (verbose) fprintf(stderr, "gpu %d: precise residual trunk (RSR_PRECISE)\n", gpuid[size_t(i)]);
        }
        if (auto_ok)
        {
            double headroom = 0, peak = 0, overflow = 0, active = 0, ms = 0;
            rsr_get_stat(ctxs[size_t(i)], "selfcheck_headroom", &headroom);
            rsr_get_stat(ctxs[size_t(i)], "selfcheck_peak_abs", &peak);
            rsr_get_stat(ctxs[size_t(i)], "selfcheck_overflow", &overflow);
            rsr_get_stat(ctxs[size_t(i)], "selfcheck_ms", &ms);
            rsr_get_stat(ctxs[size_t(i)], "precise_active", &active);
            std::vector<float> pk(size_t(std::max(1, nconv)), 0.f);
            std::vector<long long> bad(pk.size(), 0);
            rsr_selfcheck_ranges(ctxs[size_t(i)], pk.data(), bad.data(), nconv);
            int peak_conv = 0;
            long long nonfinite = 0;
            for (int k = 0; k < nconv; k++)
            {
                nonfinite += bad[size_t(k)];
                if (pk[size_t(k)] > pk[size_t(peak_conv)]) peak_conv = k;
            }
            if (verbose)
                fprintf(stderr, "gpu %d: self-check 148x148 tile: storage_err %.3e, headroom %.2f, peak |activation| %.4g at conv %d, %lld non-finite, %.1f ms -> %s%s%s\n",
                        gpuid[size_t(i)], headroom > 0 ? (1.0 / 255.0) / headroom : 0.0, headroom, peak, peak_conv, nonfinite, ms,
                        active != 0 ? "precise residual trunk" : "fp16 storage", pe ? " (RSR_PRECISE)" : "",
                        overflow != 0 ? "; warning: activations overflow fp16, the output is not reliable" : "");
            else if (overflow != 0)
                fprintf(stderr, "gpu %d: warning: the model's activations overflow fp16 (peak %.4g, %lld non-finite values): the output is not reliable\n",
                        gpuid[size_t(i)], peak, nonfinite);
        }
        realsr.push_back(std::move(r));
    }
    if (video)
    { // -v prints one line per window, no per-tile percent lines
        rsr_set_progress_callback(ctxs[0], nullptr, nullptr);
        const RealSR& r = *realsr[0];
        int vrc = rsr_set_params(ctxs[0], r.scale, r.tilesize, r.prepadding);
        if (vrc == RSR_OK) vrc = r.set_ratio(ctxs[0]);
        if (vrc != RSR_OK)
        {
            fprintf(stderr, "%s\n", rsr_last_error(ctxs[0]));
            return 1;
        }
        const int vny = out_den_y ? out_num_y : out_num, vdy = out_den_y ? out_den_y : out_den;
        return run_video(ctxs[0], inputpath, outputpath, out_num, out_den, vny, vdy, verbose);
    }
    // one image, several GPUs: every GPU takes a share of the tile rows
    const bool split_one_image = ngpu > 1 && input_files.size() == 1;

    // load -> proc -> save
    TaskQueue toproc, tosave;
    int failures = 0;
    std::mutex fail_mu;
    const int total_proc = [&] { int n = 0; for (int j : jobs_proc) n += j; return n; }();

    std::vector<std::thread> loaders;
    std::mutex next_mu;
    size_t next = 0;
    for (int t = 0; t < jobs_load; t++)
        loaders.emplace_back([&] {
            for (;;)
            {
                size_t i;
                {
                    std::lock_guard<std::mutex> lk(next_mu);
                    if (next >= input_files.size()) return;
                    i = next++;
                }
                std::unique_ptr<Task> v(new Task);
                v->id = int(i);
                v->inpath = input_files[i];
                v->outpath = output_files[i];
                // the route of this image: 16 bits where RSR_DEPTH says so (auto: a 16-bit source into a .png), else the 8-bit route untouched
                std::string err;
                bool deep = false;
                if (depth_mode != kDepth8)
                {
                    std::vector<uint8_t> bytes;
                    const bool sixteen = imgio::read_file(v->inpath, bytes) && imgio::is_16bit(bytes);
                    deep = depth_mode == kDepth16 || (sixteen && imgio::lower_ext(v->outpath) == "png");
                    if (deep && sixteen) err = imgio::load_image16(bytes, v->inimage);
                    else if (deep)
                    {
                        Image narrow;
                        err = imgio::load_image(v->inpath, narrow);
                        if (err.empty()) err = imgio::widen_image(narrow, v->inimage);
                    }
                    if (verbose) fprintf(stderr, "%s: %s\n", v->inpath.c_str(), deep ? (sixteen ? "16-bit route" : "16-bit route (8-bit source widened by x257)") : (sixteen ? "8-bit route (16-bit source reduced: the output is no .png)" : "8-bit route"));
                }
                if (!deep) err = imgio::load_image(v->inpath, v->inimage);
                if (!err.empty())
                {
                    fprintf(stderr, "decode image %s failed: %s\n", v->inpath.c_str(), err.c_str());
                    std::lock_guard<std::mutex> lk(fail_mu);
                    failures++;
                    continue;
                }
                if (alpha_net && v->inimage.elempack == 4)
                {
                    v->opaque = alpha_all_max(v->inimage);
                    if (verbose) fprintf(stderr, "%s: %s\n", v->inpath.c_str(), v->opaque ? "alpha is fully opaque: bicubic alpha, one pass (RSR_ALPHA=net)" : "alpha through the network, two passes (RSR_ALPHA=net)");
                }
                // an RGBA image cannot be a jpg: write <name>.png instead (main.cpp:278-288)
                const std::string oext = imgio::lower_ext(v->outpath);
                if (!deep && v->inimage.elempack == 4 && (oext == "jpg" || oext == "jpeg"))
                {
                    const std::string out2 = v->outpath + ".png";
                    fprintf(stderr, "image %s has alpha channel ! %s will output %s\n", v->inpath.c_str(), v->inpath.c_str(), out2.c_str());
                    v->outpath = out2;
                }
                // (a size the ratio does not divide is refused by RealSR::process, which sizes the image through rsr_out_size)
                v->outimage.create(std::max(1, v->inimage.w * out_num / out_den), std::max(1, out_den_y ? v->inimage.h * out_num_y / out_den_y : v->inimage.h * out_num / out_den), v->inimage.elempack, true, v->inimage.depth);
                toproc.put(std::move(v));
            }
        });

    // RSR_ALPHA=net: "alpha_net" is an option of the context, and the proc threads of a gpu share one: an RGBA image sets it for itself --
    // 0 when opaque -- and keeps the other RGBA images of its gpu out until its call returns.  RGB images, which the option does not
    // concern, run beside it as ever.
    std::vector<std::mutex> alpha_mu(static_cast<size_t>(ngpu));
    std::vector<std::thread> procs;
    for (int g = 0; g < ngpu; g++)
        for (int j = 0; j < jobs_proc[size_t(g)]; j++)
            procs.emplace_back([&, g] {
                for (;;)
                {
                    std::unique_ptr<Task> v = toproc.get();
                    if (v->id == kEnd) return;
                    int prc;
                    std::unique_lock<std::mutex> alpha_lk;
                    if (alpha_net && v->inimage.elempack == 4)
                    { // (a split image is the only one there is: every context of the group gets the value)
                        alpha_lk = std::unique_lock<std::mutex>(alpha_mu[split_one_image ? 0 : size_t(g)]);
                        for (int k = 0; k < ngpu; k++)
                            if (split_one_image || k == g) rsr_set_option(ctxs[size_t(k)], "alpha_net", v->opaque ? 0 : 1);
                    }
                    // RSR_ALPHA=adaptive: the option is the context's, RGBA images need not keep each other out -- except under -v, where
                    // the tiles an image sent through the alpha pass are read off the context's counters around its call
                    const bool count_alpha = alpha_adaptive && verbose && v->inimage.elempack == 4;
                    double ran0 = 0, flat0 = 0;
                    if (count_alpha)
                    {
                        alpha_lk = std::unique_lock<std::mutex>(alpha_mu[split_one_image ? 0 : size_t(g)]);
                        for (int k = 0; k < ngpu; k++)
                            if (split_one_image || k == g)
                            {
                                double a = 0, b = 0;
                                rsr_get_stat(ctxs[size_t(k)], "alpha_tiles", &a);
                                rsr_get_stat(ctxs[size_t(k)], "alpha_tiles_flat", &b);
                                ran0 += a, flat0 += b;
                            }
                    }
                    if (split_one_image && v->inimage.depth == 16)
                    { // rsr_process_fmt has no tile ranges: a single 16-bit image runs on the first gpu
                        if (verbose) fprintf(stderr, "%s: a 16-bit image is not split over gpus: it runs on gpu %d\n", v->inpath.c_str(), gpuid[0]);
                        prc = realsr[0]->process(v->inimage, v->outimage);
                    }
                    else if (split_one_image)
                    {
                        std::vector<RealSR*> grp;
                        for (auto& r : realsr) grp.push_back(r.get());
                        prc = RealSR::process_group(grp, v->inimage, v->outimage);
                    }
                    else
                        prc = realsr[size_t(g)]->process(v->inimage, v->outimage);
                    if (count_alpha && prc == RSR_OK)
                    {
                        double ran = 0, flat = 0;
                        for (int k = 0; k < ngpu; k++)
                            if (split_one_image || k == g)
                            {
                                double a = 0, b = 0;
                                rsr_get_stat(ctxs[size_t(k)], "alpha_tiles", &a);
                                rsr_get_stat(ctxs[size_t(k)], "alpha_tiles_flat", &b);
                                ran += a, flat += b;
                            }
                        fprintf(stderr, "%s: %d of %d tiles ran the alpha pass (RSR_ALPHA=adaptive)\n", v->inpath.c_str(), int(ran - ran0), int(ran - ran0 + flat - flat0));
                    }
                    if (prc != RSR_OK)
                    {
                        std::lock_guard<std::mutex> lk(fail_mu);
                        failures++;
                        continue;
                    }
                    tosave.put(std::move(v));
                }
            });

    std::vector<std::thread> savers;
    for (int t = 0; t < jobs_save; t++)
        savers.emplace_back([&] {
            for (;;)
            {
                std::unique_ptr<Task> v = tosave.get();
                if (v->id == kEnd) return;
                const std::string err = v->outimage.depth == 16 ? imgio::save_png16(v->outpath, v->outimage) : imgio::save_image(v->outpath, v->outimage);
                if (!err.empty())
                {
                    fprintf(stderr, "encode image %s failed: %s\n", v->outpath.c_str(), err.c_str());
                    std::lock_guard<std::mutex> lk(fail_mu);
                    failures++;
                }
                else if (verbose)
                    fprintf(stderr, "%s -> %s done\n", v->inpath.c_str(), v->outpath.c_str());
            }
        });

    for (auto& t : loaders) t.join();
    for (int i = 0; i < total_proc; i++)
    {
        std::unique_ptr<Task> e(new Task);
        e->id = kEnd;
        toproc.put(std::move(e));
    }
    for (auto& t : procs) t.join();
    for (int i = 0; i < jobs_save; i++)
    {
        std::unique_ptr<Task> e(new Task);
        e->id = kEnd;
        tosave.put(std::move(e));
    }
    for (auto& t : savers) t.join();
    return failures ? 1 : 0;
}
