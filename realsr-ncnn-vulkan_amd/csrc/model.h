// model.h -- ncnn .param/.bin reader, graph validation and weight packing (host only, no HIP).
//
// Replaces what the reference gets from ncnn::Net::load_param / load_model
// (/root/reference/src/realsr.cpp:75-76) for the one graph it ships:
// models/models-DF2K*/x4.param = ESRGAN RRDBNet(in 3, out 3, nf 64, nb 23, gc 32), 999 layers -- and the same graph at any
// other depth nb in 1..RSR_MAX_RRDB (the 6-block anime networks, 16-block "lite" trainings): 15 nb + 6 convolutions.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace rsr {

struct ParamLayer
{
    std::string type, name;
    std::vector<std::string> bottoms, tops;
    // scalar params by id, array params by id (id = -23300 - key)
    std::vector<std::pair<int, std::string>> scalars;
    std::vector<std::pair<int, std::vector<float>>> arrays;
    int geti(int id, int def) const;
    float getf(int id, float def) const;
    const std::vector<float>* geta(int id) const;
};

struct ConvRec
{
    int cin = 0, cout = 0;
    int act = 0; // 0 none, 2 leakyrelu
    float slope = 0.f;
    std::vector<float> weight; // OIHW
    std::vector<float> bias;
};

struct Model
{
    int n_layers = 0, n_blobs = 0;
    std::vector<ParamLayer> layers;
    std::vector<ConvRec> convs; // file order == canonical RRDBNet order (validated)
    int nb = 0;                 // RRDB blocks of the validated graph (validate_graph); convs.size() == num_convs(nb) after load_model
    int bin_encoding = -1;      // 1 fp16-tagged, 0 raw fp32, 2 mixed/table
    long long n_weights = 0, n_biases = 0;
};

// Network constants of the validated graph at the DEFAULT depth (x4.param of the reference's model directories).  The depth a
// model really has is Model::nb / PackedHeader::nconv; these size nothing that a loaded model is held in.
constexpr int kNumRRDB = 23;
constexpr int kNumRDB = kNumRRDB * 3; // 69
constexpr int kNumConvs = 1 + kNumRDB * 5 + 5; // 351
constexpr int kNF = 64, kGC = 32;
constexpr int kMaxRRDB = 64;                        // == RSR_MAX_RRDB (include/realsr_hip.h): bounds a table size read from a blob header
constexpr int num_convs(int nb) { return 15 * nb + 6; } // conv_first + 3 nb RDBs of 5 + trunk_conv, upconv1, upconv2, HRconv, conv_last
constexpr int kMaxConvs = num_convs(kMaxRRDB);      // 966
// the depth with num_convs(nb) == nconv, or 0 when there is none in 1..kMaxRRDB
constexpr int depth_of_convs(uint32_t nconv) { return (nconv >= 21u && nconv <= uint32_t(kMaxConvs) && (nconv - 6u) % 15u == 0u) ? int((nconv - 6u) / 15u) : 0; }

// Error codes match include/realsr_hip.h
int parse_param(const std::string& path, Model& m, std::string& err);
int validate_graph(const Model& m, std::string& err, int* nb = nullptr); // checks DAG == canonical RRDBNet of some depth 1..kMaxRRDB (*nb), fills nothing else
int read_bin(const std::string& path, Model& m, std::string& err);
int load_model(const std::string& param, const std::string& bin, Model& m, std::string& err);

// ---- packed blob ---------------------------------------------------------------------------
// One relocatable byte blob holding every conv's weights in the exact LDS images the MFMA kernel stages (conv3x3_flow,
// 16-channel planes): per conv, per 16-input-channel plane
//     [tap 0..8][cout row 0..NT*32-1][16 cin] fp16, 32 B per row, the two 16-B slots of a row swapped when (cout>>3)&1
// followed by NT*32 fp32 biases.  Cin is zero-padded to a multiple of 32 (conv_first 3 -> 32: two 16-channel planes,
// the second all zero), Cout to a multiple of 32 (conv_last 3 -> 32).  33.5 MB for x4.param: what rsr_load uploads and
// what the multi-GPU broadcast carries.  A conv with <= 4 output channels (conv_last, 64 -> 3) additionally carries the aux image
// of conv3x3_flow's (dy, cout)-in-M variant: per plane [dx][32 rows][16 cin], row dy*8 + c = tap (dy, dx) of output channel c.
struct PackedHeader
{
    uint32_t magic;   // 'RSRP'
    uint32_t version; // kPackedVersion
    uint32_t nconv;   // 15 nb + 6: the depth of the model (depth_of_convs)
    uint32_t flags;   // 0 (version 3 carried the 32-channel images of the round-1 kernels behind bit 0)
    uint64_t total_bytes;
};
struct PackedConv
{
    uint32_t cin, cout;     // true channel counts
    uint32_t act;           // 0 / 2
    uint32_t nplanes;       // ceil(cin/32): 32-channel chunks (= half the number of 16-channel planes)
    uint32_t nt;            // ceil(cout/32)
    float slope;
    uint64_t b_off;         // byte offsets from blob start (256-B aligned)
    uint64_t w16_off;       // 16-channel-plane images
    uint64_t aux_off;       // convs with <= 4 output channels (conv_last): [plane][dx 0..2][row = dy*8 + cout][16 cin], 3 KB per plane; else 0
};
constexpr uint32_t kPackedVersion = 6;

// Which output channel sits in row i (0..31) of a 32-row weight image (and of the bias block): the v_mfma_f32_32x32x16_f16 result
// leaves row q*8 + hi*4 + e in register q*4 + e of lane (pixel, hi).  With the rows ordered like this a lane's registers 0..7 are
// the 8 CONSECUTIVE channels hi*8 .. hi*8+7 of the first output plane and 8..15 those of the second: 16 bytes of fp16 that go to
// memory as they are -- no transpose through LDS in the epilogue (conv_flow.hip).  A bijection on 0..31 (swaps 4-7 <-> 8-11 and
// 20-23 <-> 24-27); rows 0..3 stay channels 0..3 (conv_last's three outputs).
constexpr int row_cout(int i) { return ((i >> 4) & 1) * 16 + ((i >> 2) & 1) * 8 + ((i >> 3) & 1) * 4 + (i & 3); }
constexpr uint32_t kPackedMagic = 0x50525352u; // "RSRP"

size_t packed_size(const Model& m);
int pack_model(const Model& m, void* dst, size_t cap, std::string& err);
// Full validation of a blob that may come from anywhere (a broadcast, a file): header, every offset + extent inside the
// blob, and the conv table equal to the canonical RRDBNet schedule (cin/cout/act per index) of the depth the header names.
// The header is read first (head_bytes >= sizeof(PackedHeader)); its nconv must be num_convs(nb) for some nb in 1..kMaxRRDB and
// head_bytes at least packed_table_bytes(nconv) before any table entry is looked at.  Only those bytes are dereferenced.
int check_packed(const void* head, size_t head_bytes, size_t total_bytes, std::string& err);
size_t packed_table_bytes();               // header + table of the default depth (kNumConvs entries)
size_t packed_table_bytes(uint32_t nconv); // ... of nconv entries
// cin / cout of convolution `index` (0..350) in x4.param order at the default depth ...
void canonical_conv(int index, int& cin, int& cout, int& act);
// ... and at depth nb (index 0 .. num_convs(nb) - 1)
void canonical_conv(int nb, int index, int& cin, int& cout, int& act);

// ---- blending two packed blobs (include/realsr_hip.h "network interpolation") ------------------------------------------------------------
// What a blend computes: the segments of a blob that hold numbers.  Per convolution, in table order: the fp32 biases, the fp16 w16
// image, and the fp16 aux image where aux_off != 0.  Every segment starts 256-byte aligned and is a multiple of 16 bytes (nt * 128,
// np * nt * 18432, np * 6144).  Everything else of a blob -- header, table, the padding behind a segment -- is not a number.
struct BlendSeg
{
    uint64_t off, bytes;
    bool f32; // fp32 elements (biases), else fp16
};
// The segments of the table T of nconv entries (a table check_packed has passed), appended to out
void blend_segments(const PackedConv* T, uint32_t nconv, std::vector<BlendSeg>& out);
// Are header + table of two checked blobs byte-identical (head_a, head_b: at least packed_table_bytes of their nconv)?  RSR_E_GRAPH
// otherwise, err naming the depths, or the first convolution and field that differ.
int compare_tables(const void* head_a, const void* head_b, std::string& err);
// THE rule in C++ (rsr_model_blend): check_packed of both, compare_tables, then dst = a outside the segments and
// fp16_rne((u * a) + (t * b)) / (u * a) + (t * b) inside, u = 1 - t, every operation rounded by itself in fp32.  t == 0 / t == 1 copy
// a / b.  *need (may be null) = the size of the result whenever the two blobs passed; dst == null only reports it.  dst must not
// overlap a or b.
int blend_packed(const void* a, size_t a_bytes, const void* b, size_t b_bytes, float t, void* dst, size_t cap, size_t* need, std::string& err);

uint16_t f32_to_f16(float f);
float f16_to_f32(uint16_t h);

} // namespace rsr
