// topc_plan.hpp -- what the top-C scoring path (gmm_topc.hip: Reynolds, Quatieri & Dunn 2000 -- per frame the C best components of
// the UBM, then only those in every adapted speaker) decides before it touches the device: whether the call qualifies, the padded
// row width, the selection variant, the cut of the batch into chunks of frames under the scratch bound, and the shapes of the four
// stages' launches, as a pure function of the set's shape, the batch's length, the bound and the number of compute units.
// Host-only C++17, nothing of HIP: gmm_topc.hip consumes it, sr_topc_plan hands it to tests, tests/host/topc_checks.cpp runs it
// under the host sanitizers.
#pragma once

#include <cstdint>
#include <string>

namespace sr {

constexpr int TOPC_MAX_DIM = 64;            // widest row a lane of the select / evaluate kernels keeps in registers
constexpr int TOPC_MAX_REG_C = 8;           // largest C whose running selection lives in registers; above it: the rank kernel
constexpr int TOPC_MAX_RANK_K = 8192;       // the rank kernel holds a frame's K keys in LDS (32 KiB)
constexpr int TOPC_TILE = 64;               // frames of one utterance (and one chunk) a combine workgroup sums in order
constexpr int TOPC_STAGE = 64;              // (frame, slot) entries an evaluate workgroup stages in LDS at a time
constexpr int TOPC_WG = 256;                // lanes of the select, route and rank workgroups
constexpr int64_t TOPC_DEFAULT_SCRATCH = (int64_t)1 << 30;

struct TopcPlan {
    int tp = 0;                 // padded row width: 16, 40 or 64
    int cr = 0;                 // register slots of the running selection (1, 5, 8); 0: all K keys to scratch + the rank kernel
    int64_t row_bytes = 0;      // scratch one frame needs: terms [C][S] fp32, selection + routed pair [C] int32 each, LL_bg, (cr == 0: K keys)
    int64_t chunk = 0;          // frames per chunk (the last one may be shorter); 0 for a batch without frames
    int64_t n_chunks = 0;
    int run = 0;                // entries of ONE component an evaluate workgroup takes: 256, or 64 when the chunk is small
    int eval_waves = 0;         // waves of an evaluate workgroup: a lane per model, min(4, ceil(S / 64))
    int64_t eval_grid_x = 0;    // upper bound of the runs of a full chunk: ceil(chunk C / run) + K (the rest exit at once)
    int eval_grid_y = 0;        // blocks of 64 eval_waves models
    int64_t select_grid = 0;    // ceil(chunk / 256): a lane per frame
    int64_t route_grid = 0;     // ceil(chunk C / 256): a lane per (frame, slot)
    int combine_wg = 0;         // lanes of a combine workgroup: a lane per model, 64 .. 256
    int rank_lds = 0;           // bytes of LDS the rank kernel asks for (cr == 0), else 0
};

// The refusals of the call itself, in the order the entry points apply them; true, or false with the text (it names the remedy).
// `tied`: the set shares sigma and weights (or holds one model); batch_is_features: the batch's kind.
bool topc_check(bool tied, int S, int K, int D, int bg, int top_c, bool batch_is_features, std::string &why);

// Fills `p` and returns true, or false with the reason: a shape topc_check refuses, n_frames < 0, a bound below one frame's row.
// n_cu: compute units of the device (>= 1).
bool plan_topc(int K, int D, int S, int top_c, int64_t n_frames, int64_t scratch_bytes, int n_cu, TopcPlan &p, std::string &why);

}  // namespace sr
