// xvector_plan.hpp -- what the x-vector forward pass (xvector.hip: time-delay layers as one implicit GEMM on the bf16 matrix cores,
// mean / standard-deviation pooling, affine layers on the pooled matrix) decides before it touches the device: the refusals, the
// padded widths, every segment's rows at every layer, the tile lists, and the chunking of the segment list under a scratch bound --
// a pure function of the layer descriptors, the segments' frame counts and the bound.  Host-only C++17, nothing of HIP:
// xvector.hip consumes it, sr_xvector_plan hands it to tests, tests/host/xvector_checks.cpp runs it under the host sanitizers.
//
// Stages: stage s is the input of layer s and the output of layer s - 1.  A frame layer (before the pooling) keeps one row per
// remaining frame of a segment: a segment of n frames has n - (spans of the layers before s) rows at stage s.  After the pooling a
// segment is one row.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace sr {

constexpr int XV_TDNN = 0, XV_POOL = 1, XV_AFFINE = 2;
constexpr int XV_ACT_NONE = 0, XV_ACT_RELU = 1;
constexpr int XV_TM = 128, XV_TN = 128;            // the layer kernel's tile: rows (frames) x columns (output channels)
constexpr int XV_KC = 64;                          // K per LDS stage: two granules, each one (offset, 32 channels)
constexpr int XV_GRAN = 32;                        // channels are padded to this with zero weights
constexpr int XV_WG = 256;                         // four waves, each 64 x 64 of the tile
constexpr int XV_LDS_ROW = XV_KC * 2;              // bytes of one staged row; its eight 16-byte pieces are XOR-swizzled by (row >> 1) & 7
constexpr int XV_LDS_BYTES = 2 * (XV_TM + XV_TN) * XV_LDS_ROW;      // two buffers of an A and a B image: 64 KiB
constexpr int XV_MAX_C = 4096, XV_MAX_OFFSETS = 9, XV_MAX_OFFSET = 16, XV_MAX_LAYERS = 64;
constexpr int XV_POOL_COLS = 64, XV_POOL_LANES = 4;               // the pooling workgroup: 64 channels x 4 row lanes
constexpr int XV_CONVERT_ROWS = 64;                // rows a convert workgroup takes
constexpr int64_t XV_DEFAULT_SCRATCH = (int64_t)1024 << 20;
constexpr int XV_DESC = 16;                        // int32 per layer in the C ABI's descriptor table

struct XvLayer {
    int kind = XV_TDNN;
    int c_in = 0, c_out = 0;
    int act = XV_ACT_NONE;
    int n_off = 0;
    int off[XV_MAX_OFFSETS] = {};
    bool has_affine = false;      // scale / shift given
    double var_floor = 0.0;       // pooling only
};

// C ABI descriptor row: {kind, c_in, c_out, act, has scale/shift, n_offsets, offsets[9], 0}
XvLayer xv_layer_from_desc(const int32_t *d, double var_floor);

struct XvModelInfo {
    int n_layers = 0;
    int pool = -1;                 // index of the pooling layer
    int input_dim = 0;
    int embedding_dim = 0;
    int context = 0;               // frames consumed: sum of (last offset - first offset); a segment needs context + 1 frames
    std::vector<int> width;        // [n_layers + 1] channels of every stage
    std::vector<int> width_pad;    // the same, padded to XV_GRAN
    std::vector<int> span;         // [n_layers] frames a layer consumes (0 for pooling and affine)
    std::vector<int> k_pad;        // [n_layers] K of the layer's weight image: n_off * width_pad[l], up to a multiple of XV_KC
    std::vector<int> n_pad;        // [n_layers] rows of the weight image: c_out up to a multiple of XV_TN
};

// Fills `info` and returns true, or returns false with the refusal (which names the remedy) in `why`.
bool xv_check_model(const XvLayer *layers, int n_layers, XvModelInfo &info, std::string &why);

struct XvTile {
    int32_t seg;       // segment within the chunk (segment layers: 0, the pooled matrix is one run of rows)
    int32_t first;     // first output row of the tile within the segment
    int32_t rows;      // 1 .. XV_TM
    int32_t pad;
};

struct XvChunk {
    int64_t seg_begin = 0, seg_end = 0;
    int64_t bytes = 0;                       // what the chunk's buffers take
    std::vector<int64_t> stage_rows;         // [n_layers + 1] rows of every stage, all its segments together
};

struct XvPlan {
    XvModelInfo info;
    int last = 0;                            // the last layer that runs (the tapped one, or n_layers - 1)
    int64_t n_seg = 0;
    std::vector<XvChunk> chunks;
    int64_t buf_bytes[2] = {0, 0};           // the two ping-ponged frame-level buffers, sized for the largest chunk
    int64_t out_rows = 0;                    // rows of the call's result
    int out_cols = 0;
};

// rows of a segment of n frames at stage s
inline int64_t xv_stage_rows(const XvModelInfo &m, int64_t n_frames, int s) {
    if (s > m.pool) return 1;
    int64_t r = n_frames;
    for (int l = 0; l < s; l++) r -= m.span[(size_t)l];
    return r;
}

// the bytes one segment of n frames adds to a chunk: its two largest frame-level stages (bf16), its pooled row (fp32), its rows of
// the segment-level stages (bf16), its rows of the result (fp32)
int64_t xv_segment_bytes(const XvModelInfo &m, int64_t n_frames, int last, bool tap_bf16);

// `tap`: -1 for the embedding, or the layer whose output is returned.  lengths[i]: frames of segment i.
bool plan_xvector(const XvLayer *layers, int n_layers, const int64_t *lengths, int64_t n_seg, int tap, bool tap_bf16, int64_t scratch_bytes,
                  XvPlan &p, std::string &why);

// tiles of layer `l` over the chunk's segments; never more than XV_TM rows, never rows of two segments
void xv_layer_tiles(const XvModelInfo &m, const int64_t *lengths, int64_t seg_begin, int64_t seg_end, int l, std::vector<XvTile> &tiles);

// a segment table against its batch: false with the reason when a segment lies outside its utterance or is shorter than context + 1
bool xv_check_segments(const XvModelInfo &m, const int64_t *utt_offsets, int n_utt, const int32_t *segs, int64_t n_seg, std::string &why);

}  // namespace sr
