// bw_plan.hpp -- what the batched Baum-Welch statistics call (bw_stats.hip: per utterance the zero- and first-order statistics
// N[u][k] = sum_t gamma_k(t), F[u][k][d] = sum_t gamma_k(t) x_t[d] against ONE diagonal model, the front of a JFA / i-vector leg)
// decides before it touches the device: whether the call qualifies, the cut of every utterance into frame ranges, the cut of the
// range table into groups whose float64 slabs fit the scratch bound, and the launch shapes -- as a pure function of the model's
// shape, the utterances' lengths, the option bw_range_frames, the bound and the number of compute units.
// Host-only C++17, nothing of HIP: bw_stats.hip consumes it, sr_bw_plan hands it to tests, tests/host/bw_checks.cpp runs it under
// the host sanitizers.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace sr {

constexpr int BW_MAX_DIM = 40;              // widest row the fp64 matrix-core statistics kernel is instantiated for (as em.hip's)
constexpr int BW_TILE = 128;                // frames a statistics workgroup holds in LDS at a time
constexpr int BW_WG_MIX = 64;               // mixtures of a statistics workgroup: 4 waves x 16
constexpr int BW_WG = 256;                  // lanes of every workgroup of the path
constexpr int BW_DEFAULT_RANGE = 1024;      // frames per range when bw_range_frames is 0 ...
constexpr int BW_MAX_AUTO_RANGES = 256;     // ... grown in whole tiles so that one utterance has at most this many ranges
constexpr int64_t BW_MAX_RANGE_FRAMES = (int64_t)1 << 30;
constexpr int64_t BW_MAX_MIXTURES = (int64_t)65535 * 64;    // the mixture blocks are the statistics launch's grid y
constexpr int64_t BW_DEFAULT_SCRATCH = (int64_t)1 << 30;

// One range: `rows` consecutive frames of ONE utterance from row `first` of the batch.  (The layout of batch.hpp's TileDesc: the
// device reads the table as such.)
struct BwRange {
    int64_t first;
    int32_t rows;
    int32_t utt;
};

struct BwPlan {
    int dp = 0;                     // padded row width the kernels are instantiated for (the vector layout's: gmm_model.hpp)
    int ncb = 0;                    // blocks of 16 statistic columns [x_0 .. x_{dp-1} | 1 | padding]
    int n_mix_blocks = 0;           // ceil(K / 64): the last one padded with dead mixtures
    int64_t slab_bytes = 0;         // float64 scratch of one range: n_mix_blocks x 64 x ncb x 16 x 8
    int64_t range_frames = 0;       // bw_range_frames as given (0 = automatic)
    std::vector<BwRange> ranges;    // every frame of the batch exactly once, in batch order; an empty utterance has none
    int64_t group_ranges = 0;       // ranges per group: group g holds ranges [g group_ranges, (g + 1) group_ranges)
    int64_t n_groups = 0;
    int64_t lse_grid = 0;           // pass A: a lane per frame of the whole batch
    int stats_lds = 0;              // pass B: bytes of LDS of a workgroup; its grid is (ranges of the group, n_mix_blocks)
    int64_t reduce_blocks = 0;      // reduce: ceil(K (D + 1) / 256) workgroups per (utterance, group) segment
    int64_t stats_rounds = 0;       // rounds the largest group's statistics launch makes over the chip at two workgroups a unit
};

// The refusals of the call itself, in the order the entry point applies them; true, or false with the text (it names the remedy).
// S: models of the set, K / D: mixtures / dimension of model `model` (any values when the index is out of range).
bool bw_check(bool batch_is_features, int S, int model, int K, int D, int feat_dim, std::string &why);

// Rows per range of an utterance of `len` frames: a function of the utterance's own length, the model's shape and the option only.
int64_t bw_range_rows(int64_t len, int K, int D, int64_t range_frames);

// Fills `p` and returns true, or false with the reason: a shape bw_check refuses, a negative length, range_frames outside
// 0 .. 2^30, a bound below one range's slab.  lengths: [U] frames per utterance; n_cu: compute units of the device (>= 1).
bool plan_bw(int K, int D, const int64_t *lengths, int64_t U, int64_t range_frames, int64_t scratch_bytes, int n_cu, BwPlan &p,
             std::string &why);

}  // namespace sr
