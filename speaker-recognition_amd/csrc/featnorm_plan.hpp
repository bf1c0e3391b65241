// featnorm_plan.hpp -- what the short-time feature normalisation (featnorm.hip: feature warping, sliding-window mean and
// mean-and-variance normalisation) decides before it touches the device: the refusals, the frames a workgroup takes, the rows it
// stages, the columns that fit LDS in one pass, the grid, and whether warped values come from a table -- a pure function of the
// call's parameters, the longest utterance and the option "norm_tile".  Host-only C++17, nothing of HIP: featnorm.hip consumes it,
// sr_feature_norm_plan hands it to tests, tests/host/featnorm_checks.cpp runs it under the host sanitizers.
//
// The window of frame t of an utterance of T frames, W the window option: N = min(W, T) rows from s0(t) = min(max(t - W / 2, 0),
// T - N) -- centred in the interior, shifted (not shortened) at both ends.
#pragma once

#include <cstdint>
#include <string>

namespace sr {

constexpr int FEATNORM_WARP = 0, FEATNORM_CMN = 1, FEATNORM_CMVN = 2;
constexpr int FEATNORM_MIN_W = 2, FEATNORM_MAX_W = 1024;
constexpr int FEATNORM_WG = 256;                    // lanes of a workgroup: four waves
constexpr int FEATNORM_WAVE = 64;                   // a wave takes 64 consecutive frames of one column, a lane per frame
constexpr int FEATNORM_AUTO_TILE = 256;             // frames per workgroup under norm_tile = 0
constexpr int FEATNORM_MAX_TILE = 1024;
constexpr int FEATNORM_LDS_FLOATS = 16384;          // 64 KiB of the CU's 160: two workgroups stay resident beside each other
constexpr int FEATNORM_MAX_COLS = 64;               // columns per pass
constexpr int FEATNORM_WGS_PER_CU = 32;

struct FeatNormPlan {
    int mode = 0, W = 0, dim = 0;
    int F = 0;                      // frames per workgroup (a tile): a multiple of 64
    int span_max = 0;               // rows a tile stages at most: F + min(W, max_frames) - 1, never more than max_frames
    int stride = 0;                 // floats between two columns in LDS: the least 4 x odd number >= span_max
    int passes = 0;                 // ceil(dim / min(dim, 64, LDS floats / stride))
    int cols = 0;                   // columns per pass: ceil(dim / passes)
    int lds_bytes = 0;              // cols * stride * 4
    int64_t tiles_max = 0;          // tiles of the longest utterance
    bool table = false;             // warp: the values of a full window (N = W) are read from a table of 2 W - 1 floats
    int table_len = 0;              // 2 W - 1, or 0
};

// Fills `p` and returns true, or returns false with the reason in `why`: a mode other than 0 / 1 / 2, a window outside 2 .. 1024,
// a batch that holds no fp32 features (is_features false), dim < 1, max_frames < 0, a tile option that is negative, above 1024 or
// no multiple of 64, n_cu < 1.  tile_option 0: FEATNORM_AUTO_TILE.
bool plan_feature_norm(int mode, int window, bool is_features, int dim, int64_t max_frames, long tile_option, int n_cu, FeatNormPlan &p,
                       std::string &why);

// the first row of frame t's window, relative to the utterance
inline int64_t featnorm_window_start(int64_t t, int64_t T, int W) {
    const int64_t N = T < W ? T : W;
    int64_t s = t - W / 2;
    if (s < 0) s = 0;
    if (s > T - N) s = T - N;
    return s;
}

// tiles of an utterance of T frames
inline int64_t featnorm_tiles(int64_t T, int F) { return T / F + (T % F != 0); }

// workgroups of a launch over n_tiles tiles: one per tile up to 32 per compute unit (the kernel strides over the rest)
int featnorm_grid(int64_t n_tiles, int n_cu);

}  // namespace sr
