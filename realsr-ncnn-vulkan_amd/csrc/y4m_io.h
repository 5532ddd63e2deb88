// y4m_io.h -- YUV4MPEG2 streams for the CLI's video mode (main.cpp): the stream header, the frame headers and the planes of a frame.
// Header-only, host-only, stdio only; nothing here knows the engine beyond the RSR_FMT_* ids of include/realsr_hip.h.
//
//   YUV4MPEG2 W<w> H<h> [F<n>:<d>] [I<p|t|b|m|?>] [A<a>:<b>] [C<tag>] [X<anything>]...\n      one line, at most kMaxLine bytes
//   FRAME[ <parameters>]\n  followed by the planes Y, U, V, tightly packed; 10-bit samples are 16-bit little-endian words, code low
//
// Every refusal is a message (the empty string: fine); no input makes the reader allocate more than one frame or read past a buffer.
#ifndef RSR_Y4M_IO_H
#define RSR_Y4M_IO_H

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/realsr_hip.h"

namespace y4m
{
constexpr size_t kMaxLine = 256; // bytes of a header line, the newline included
constexpr int kMaxSize = 65536;  // W and H

struct Header
{
    int w = 0, h = 0;
    int fmt = RSR_FMT_NV12; // the surface format whose three-plane form the frames have
    int siting = 0;         // option "yuv_siting" of the C tag; -1: the format has none (4:4:4)
    int range = -1;         // XCOLORRANGE: 1 = FULL, 0 = LIMITED, -1 = not said
    long long a_num = 0, a_den = 0; // the A tag
    bool has_a = false;
    std::vector<std::string> tokens; // every tag of the line in its order, W, H and A among them (they are rewritten on output)
};

struct CTag
{
    const char* tag;
    int fmt, siting;
};
inline const CTag* ctags(size_t* n)
{
    static const CTag t[] = {{"420", RSR_FMT_NV12, 0},     {"420jpeg", RSR_FMT_NV12, 0}, {"420mpeg2", RSR_FMT_NV12, 1}, {"420paldv", RSR_FMT_NV12, 2},
                             {"420p10", RSR_FMT_P010, 1},  {"422", RSR_FMT_NV16, 1},     {"422p10", RSR_FMT_P210, 1},   {"444", RSR_FMT_YUV444P, -1},
                             {"444p10", RSR_FMT_YUV444P10, -1}};
    *n = sizeof t / sizeof t[0];
    return t;
}

inline int sample_bytes(int fmt) { return fmt == RSR_FMT_NV12 || fmt == RSR_FMT_NV16 || fmt == RSR_FMT_YUV444P ? 1 : 2; }
inline int chroma_shift_x(int fmt) { return fmt == RSR_FMT_YUV444P || fmt == RSR_FMT_YUV444P10 ? 0 : 1; }
inline int chroma_shift_y(int fmt) { return fmt == RSR_FMT_NV12 || fmt == RSR_FMT_P010 ? 1 : 0; }
// bytes of the planes of one w x h frame (w, h <= kMaxSize: below 2^35)
inline size_t frame_bytes(int fmt, int w, int h)
{
    const size_t es = size_t(sample_bytes(fmt));
    return es * (size_t(w) * size_t(h) + 2 * size_t(w >> chroma_shift_x(fmt)) * size_t(h >> chroma_shift_y(fmt)));
}

// One line, the newline consumed and dropped.  0: a line; 1: end of file before any byte; -1: no newline within kMaxLine bytes, or the
// file ends inside the line.
inline int read_line(FILE* f, std::string& line)
{
    line.clear();
    for (size_t i = 0; i < kMaxLine; i++)
    {
        const int c = std::fgetc(f);
        if (c == EOF) return line.empty() ? 1 : -1;
        if (c == '\n') return 0;
        line.push_back(char(c));
    }
    return -1;
}

// A decimal number of 1 .. 9 digits and nothing else.
inline bool number(const std::string& s, long long* v)
{
    if (s.empty() || s.size() > 9) return false;
    long long n = 0;
    for (char c : s)
    {
        if (c < '0' || c > '9') return false;
        n = n * 10 + (c - '0');
    }
    *v = n;
    return true;
}
inline bool ratio(const std::string& s, long long* a, long long* b)
{
    const size_t colon = s.find(':');
    return colon != std::string::npos && number(s.substr(0, colon), a) && number(s.substr(colon + 1), b);
}

// The stream header from its line (without the newline).  Returns the refusal, or "" and a filled Header.
inline std::string parse_header(const std::string& line, Header& hd)
{
    hd = Header();
    static const char magic[] = "YUV4MPEG2";
    if (line.compare(0, sizeof magic - 1, magic) != 0 || (line.size() > sizeof magic - 1 && line[sizeof magic - 1] != ' ')) return "not a YUV4MPEG2 stream";
    bool have_w = false, have_h = false, have_c = false;
    size_t pos = sizeof magic - 1;
    while (pos < line.size())
    {
        while (pos < line.size() && line[pos] == ' ') pos++;
        size_t end = line.find(' ', pos);
        if (end == std::string::npos) end = line.size();
        if (end == pos) break;
        const std::string tok = line.substr(pos, end - pos);
        pos = end;
        const std::string val = tok.substr(1);
        long long n = 0, d = 0;
        switch (tok[0])
        {
        case 'W':
        case 'H':
            if (!number(val, &n) || n < 1 || n > kMaxSize) return "bad " + tok.substr(0, 1) + " tag '" + tok + "' (1 .. 65536)";
            if (tok[0] == 'W') hd.w = int(n), have_w = true;
            else hd.h = int(n), have_h = true;
            break;
        case 'F':
            if (!ratio(val, &n, &d)) return "bad frame rate tag '" + tok + "'";
            break;
        case 'A':
            if (!ratio(val, &n, &d)) return "bad aspect tag '" + tok + "'";
            hd.a_num = n, hd.a_den = d, hd.has_a = true;
            break;
        case 'I':
            if (val == "t" || val == "b" || val == "m") return "interlaced streams are not supported (tag '" + tok + "')";
            if (val != "p" && val != "?") return "bad interlacing tag '" + tok + "'";
            break;
        case 'C':
        {
            size_t nt = 0;
            const CTag* t = ctags(&nt);
            const CTag* hit = nullptr;
            for (size_t i = 0; i < nt; i++)
                if (val == t[i].tag) hit = &t[i];
            if (!hit) return "chroma tag '" + tok + "' is not supported (C420, C420jpeg, C420mpeg2, C420paldv, C420p10, C422, C422p10, C444, C444p10)";
            hd.fmt = hit->fmt, hd.siting = hit->siting, have_c = true;
            break;
        }
        case 'X':
            if (val == "COLORRANGE=FULL") hd.range = 1;
            else if (val == "COLORRANGE=LIMITED") hd.range = 0;
            break;
        default: return "unknown header tag '" + tok + "'";
        }
        hd.tokens.push_back(tok);
    }
    (void)have_c; // (no C tag: C420jpeg, the defaults of Header)
    if (!have_w || !have_h) return "the header has no W or no H tag";
    if ((hd.w & chroma_shift_x(hd.fmt)) || (hd.h & chroma_shift_y(hd.fmt))) return "odd frame size for the chroma subsampling of the stream";
    return "";
}

inline long long gcd(long long a, long long b)
{
    while (b)
    {
        const long long t = a % b;
        a = b, b = t;
    }
    return a;
}

// The header line of the output (with its newline): W, H and A rewritten for an ow x oh result at the ratios nx / dx and ny / dy, every
// other tag as it came.  A a:b becomes a ny dx : b nx dy, reduced; 0:0 (unknown) stays.
inline std::string format_header(const Header& hd, int ow, int oh, int nx, int dx, int ny, int dy)
{
    std::string out = "YUV4MPEG2";
    for (const std::string& tok : hd.tokens)
    {
        out += ' ';
        if (tok[0] == 'W') out += "W" + std::to_string(ow);
        else if (tok[0] == 'H') out += "H" + std::to_string(oh);
        else if (tok[0] == 'A' && hd.a_num && hd.a_den)
        {
            long long a = hd.a_num * ny * dx, b = hd.a_den * nx * dy; // (9 digits times two factors of at most 32: no overflow)
            const long long g = gcd(a, b);
            out += "A" + std::to_string(a / g) + ":" + std::to_string(b / g);
        }
        else out += tok;
    }
    return out + "\n";
}

// The next frame: its header line into `params` ("FRAME" and what follows it), its planes into buf (frame_bytes of the header).
// 1: a frame; 0: the stream ends cleanly in front of a frame; -1: refusal in `err` (a broken magic, a stream cut inside a frame).
inline int read_frame(FILE* f, const Header& hd, std::vector<unsigned char>& buf, std::string& params, std::string& err)
{
    const int rc = read_line(f, params);
    if (rc == 1) return 0;
    if (rc < 0)
    {
        err = "frame header without a newline within 256 bytes";
        return -1;
    }
    if (params.compare(0, 5, "FRAME") != 0 || (params.size() > 5 && params[5] != ' '))
    {
        err = "a frame does not start with FRAME";
        return -1;
    }
    const size_t need = frame_bytes(hd.fmt, hd.w, hd.h);
    // in pieces of 1 MiB, the buffer growing with what has arrived: a wild W x H in front of a short stream allocates no 25 GB
    size_t got = 0;
    buf.clear();
    while (got < need)
    {
        const size_t piece = need - got < (size_t(1) << 20) ? need - got : (size_t(1) << 20);
        buf.resize(got + piece);
        const size_t r = std::fread(buf.data() + got, 1, piece, f);
        got += r;
        if (r != piece) break;
    }
    if (got != need)
    {
        err = "the stream ends inside a frame (" + std::to_string(got) + " of " + std::to_string(need) + " bytes)";
        return -1;
    }
    return 1;
}

inline bool write_frame(FILE* f, const std::string& params, const unsigned char* data, size_t bytes)
{
    return std::fwrite(params.data(), 1, params.size(), f) == params.size() && std::fputc('\n', f) != EOF && std::fwrite(data, 1, bytes, f) == bytes;
}
} // namespace y4m

#endif
