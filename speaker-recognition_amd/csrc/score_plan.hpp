// score_plan.hpp -- what a scoring pass decides before it touches the device: which layouts a set is packed with
// (pack_model_set), then engine, workgroup shape and model groups of a pass over it (plan_score, plan_groups), as pure
// functions of the set's host-side summary, the batch's counts, the options, the flags and the CU count.  Host-only
// C++17: score_plan.cpp calls nothing of HIP, and tests/host/host_checks.cpp pins the decisions on the CPU.
#pragma once

#include "gmm_model.hpp"
#include "score_shapes.hpp"

namespace sr {

struct ScoreOptions {
    int frames_per_lane = 0;   // 0 = auto; 1, 2 or 4 frames resident per lane
    int model_groups = 0;      // 0 = auto; workgroups per frame tile along the model axis
    int packed = 0;            // -1 = scalar v_fma_f32; 0 (auto) / 1 = v_pk_fma_f32, two frames per VGPR pair
    int engine = 0;            // 0 = auto; 1 = vector-ALU 2-FMA kernel; (2 = the fp32 matrix-core kernel of round 1, removed);
                               // 3 = split-bf16 (3 parts, 6 products) matrix-core kernel;
                               // 4 = split-bf16, shared-sigma form (sets whose models share sigma and weights)
                               // 5 = split-fp16 (2 parts, 3 products) matrix-core kernel;
                               // 6 = split-fp16, shared-sigma form
    int mfma_ft = 0;           // 32-frame column tiles per wave in the 4-wave generic split kernels (0 = one)
    int h2s_shape = 0;         // workgroup shape of the split-fp16 shared-sigma engine: 0 = automatic; 1 = 4 waves (three
                               // workgroups per CU); 2 = 12 waves (one per CU, one copy of the stream in LDS); 3 = 12 waves with the
                               // image loop software-pipelined inside each wave (gmm_score_h2p_kernel; on the compact image where that
                               // form applies, score_shapes.hpp: h2c_built); 4 = 4 waves on one tile, the block's models split between
                               // them; 5 = as 3, always on the flat image (A/B, and what 3 runs for the other sets); 6 = as 3, the
                               // quadratic half once per block of 15 models where 3 forms it once per two blocks (A/B)
    int split_shape = 0;       // workgroup shape of the generic split-fp16 engine: 0 = automatic; 1 = 4 waves (gmm_score_split_kernel);
                               // 16 / 12 / 8 = gmm_score_splitp_kernel with that many waves (one 32-frame tile each, log-sum-exp pipelined
                               // under the next chunk's MFMAs; 16 and 12: one workgroup per CU, 8: two)
    int h2s_pack_tails = 1;    // 0: the pipelined shared-sigma kernel takes one tile per wave even when it is a ragged tail (A/B, tests)
    int h2s_force_exc = 0;     // testing: send every workgroup of the split-fp16 shared-sigma engine through its exception pass
    int flush_list_cap = 0;    // testing: capacity of the list of (tile, model) pairs in the partial-product band (0 = automatic);
                               // a pass that notes more re-runs with a list of the counted length
    int verify_clean_counters = 0;  // testing: a delivering pass that skips the counters' clear reads them back first and fails
                                    // unless every one is zero (sr_set_option("debug_verify_clean_counters", 1))
};
ScoreOptions &score_options();

// The matrix-core engines are used when the expanded form is well conditioned in fp32 and the
// 32-mixture tiles are not mostly padding; otherwise the 2-FMA vector kernel (direct form).
constexpr double MFMA_MAX_AMP = 2000.0;      // max_k sum_d (mu'_d/sigma_d)^2
constexpr double MFMA_MAX_PAD_WASTE = 0.25;
// The two-part fp16 engines carry 22 significand bits per operand (error ~4x an fp32 FMA chain's per
// term, scripts/emulate_split.py) and fp16's 5-bit exponent: offered when the cancellation is
// moderate, every dimension's sigmas stay within a factor the gradual-underflow error analysis
// covers (HISTORY.md 2.1), and the scaled coefficients fit fp16.
constexpr double F16_MAX_AMP = 1000.0;
// Hybrid form: a set the expanded form is ill conditioned for (amp above the limits) because of FEW of its mixtures
// -- collapsed components at the sigma floor, outlier catchers -- is cut in two: those mixtures (at most
// HYBRID_MAX_BAD_FRACTION of them) run on the direct-form vector engine, the rest on the matrix cores.
constexpr double HYBRID_MAX_BAD_FRACTION = 0.25;
constexpr double F16_MAX_SIGMA_RATIO = 256.0;
constexpr double F16_MAX_COEF = 30000.0;
// is the layout there and inside its engine's range?  fp32-grade (split-bf16: PackedSplit, PackedBx3Shared) ...
template <class P>
inline bool mfma_ok(const P &p) { return !p.params.empty() && p.amp <= MFMA_MAX_AMP && p.pad_waste <= MFMA_MAX_PAD_WASTE; }
// ... and two-part fp16 (PackedSplit, PackedH2Shared)
template <class P>
inline bool f16_ok(const P &p) {
    return !p.params.empty() && p.amp <= F16_MAX_AMP && p.pad_waste <= MFMA_MAX_PAD_WASTE &&
           p.sigma_ratio <= F16_MAX_SIGMA_RATIO && p.coef_max <= F16_MAX_COEF;
}
// internal scoring flag (beside SR_CLAMP_COMPAT): keep to the fp32-grade engines (EM, serving stream)
constexpr int SCORE_PRECISE = 0x200;
// Minimum set size for the shared-sigma engine (blocks of SHARED_SB models; smaller sets would be
// mostly phantom models).
constexpr int SHARED_MIN_MODELS = 12;
constexpr int H2S_WIDE_SHAPE = 1;       // the one-workgroup-per-CU shape
constexpr int H2S_MSPLIT_SHAPE = 3;     // four waves on ONE tile, the block's models split between them: the smallest batches (round 4)
constexpr int H2S_PIPELINED_SHAPE = 2;  // the same with the image loop pipelined inside each wave: what the dispatcher takes for large batches

enum class Engine { VECTOR, SPLIT_BF16, SPLIT_F16, SHARED_BF16, SHARED_F16 };

struct ScorePlan {
    Engine engine = Engine::VECTOR;
    int F = 1;               // vector engine: frames per lane
    int FT = 1;              // 4-wave generic split kernels: 32-frame column tiles per wave
    int h2s_shape = 0;       // SHARED_F16: 0 = 4 waves, H2S_WIDE_SHAPE, H2S_PIPELINED_SHAPE, H2S_MSPLIT_SHAPE
    int splitp_w = 0;        // SPLIT_F16: waves of the wide workgroup (gmm_score_splitp_kernel), 0 = the 4-wave kernel
    int split_cpm = 0;       // ... and the 32-mixture chunks of every model
    int tile_frames = 256;   // frames per tile of the batch's tile table
    int per_tile = 4;        // doubles per (tile, model) in the partial sums: one per wave (vector engine), or combined
    bool writes_oor = false; // the pass writes the fp16 engines' saturation flag
    bool split() const { return engine == Engine::SPLIT_BF16 || engine == Engine::SPLIT_F16; }
    bool shared() const { return engine == Engine::SHARED_BF16 || engine == Engine::SHARED_F16; }
    bool operator==(const ScorePlan &o) const {
        return engine == o.engine && F == o.F && FT == o.FT && h2s_shape == o.h2s_shape && splitp_w == o.splitp_w &&
               split_cpm == o.split_cpm && tile_frames == o.tile_frames && per_tile == o.per_tile && writes_oor == o.writes_oor;
    }
};
// The engine the dispatcher takes by itself (options.engine == 0).
Engine auto_engine(const SRModelSet &set, bool precise);
// Throws (fail) where a forced engine's layout is missing.  `set` is a plain set or one half of a hybrid one.
ScorePlan plan_score(const SRModelSet &set, int64_t n_rows, int n_utt, const ScoreOptions &opt, int flags, int n_cu);
// Model groups of a pass over `n_tiles` > 0 tiles of plan.tile_frames frames: gcb[g] .. gcb[g + 1] = group g's chunks (blocks for the
// shared-sigma engines); G = gcb.size() - 1.
std::vector<int> plan_groups(const SRModelSet &set, const ScorePlan &plan, int n_tiles, const ScoreOptions &opt, int n_cu);
// Work items of the pipelined shared-sigma kernel over a table of tiles with `counts[t]` frames each (<= frames_per_tile): item =
// {tile, tile or -1, tile or -1, tile or -1}.  Every FULL tile is an item of its own, in order; with `pack_tails` the ragged ones are
// packed greedily, in order, up to four and up to frames_per_tile columns to an item, and all packed items come LAST (their waves
// close several tiles per model block: together at the end of the grid they stay in step with each other, scattered they push their
// workgroups out of phase with the others of their XCD and the parameter stream out of its L2).  Host-only: tests/host/host_checks.cpp.
struct WorkItem { int t[4]; };
std::vector<WorkItem> pack_tail_tiles(const std::vector<int> &counts, int frames_per_tile, bool pack_tails);

// Packs the layouts a set needs (all of them for small sets; for large ones the vector layout plus
// the one the dispatcher will pick, or the one forced by score_engine at creation time).
void pack_model_set(SRModelSet &s, const std::vector<const GMM *> &models);

}  // namespace sr
