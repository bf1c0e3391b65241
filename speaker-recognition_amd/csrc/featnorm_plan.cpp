// featnorm_plan.cpp -- the launch decisions of the short-time feature normalisation (featnorm_plan.hpp): pure host code, nothing of
// HIP is called here.
#include "featnorm_plan.hpp"

#include <algorithm>

namespace sr {

bool plan_feature_norm(int mode, int window, bool is_features, int dim, int64_t max_frames, long tile_option, int n_cu, FeatNormPlan &p,
                       std::string &why) {
    p = FeatNormPlan();
    if (mode != FEATNORM_WARP && mode != FEATNORM_CMN && mode != FEATNORM_CMVN) {
        why = "mode must be 0 (warp), 1 (cmn) or 2 (cmvn), got " + std::to_string(mode);
        return false;
    }
    if (window < FEATNORM_MIN_W || window > FEATNORM_MAX_W) {
        why = "the window must hold 2 .. 1024 frames, got " + std::to_string(window);
        return false;
    }
    if (!is_features) {
        why = "feature normalisation takes an fp32 feature batch (PCM batches are refused)";
        return false;
    }
    if (dim < 1) {
        why = "a feature batch of dim " + std::to_string(dim);
        return false;
    }
    if (max_frames < 0) {
        why = "a negative frame count";
        return false;
    }
    if (tile_option < 0 || tile_option > FEATNORM_MAX_TILE || tile_option % FEATNORM_WAVE != 0) {
        why = "norm_tile must be 0 (automatic) or a multiple of 64 up to 1024 frames per workgroup";
        return false;
    }
    if (n_cu < 1) {
        why = "a device of " + std::to_string(n_cu) + " compute units";
        return false;
    }
    p.mode = mode;
    p.W = window;
    p.dim = dim;
    p.F = tile_option ? (int)tile_option : FEATNORM_AUTO_TILE;
    // a tile of F frames reads the rows from its first frame's window start to its last frame's window end: at most F - 1 rows
    // more than one window, and never more than the utterance holds
    const int64_t n_max = std::min<int64_t>(window, max_frames);
    p.span_max = (int)std::max<int64_t>(1, std::min<int64_t>(p.F + n_max - 1, max_frames));
    // 4 x an odd number of floats: a column starts on 16 bytes (the walk reads four values at once), and the staging's transposed
    // writes -- neighbouring lanes a stride apart -- spread over the banks four ways at worst
    p.stride = (p.span_max + 3) / 4 * 4;
    if (p.stride % 8 == 0) p.stride += 4;
    const int cols_max = std::max(1, std::min({dim, FEATNORM_MAX_COLS, FEATNORM_LDS_FLOATS / p.stride}));
    p.passes = dim / cols_max + (dim % cols_max != 0);
    p.cols = dim / p.passes + (dim % p.passes != 0);            // the passes even out: 39 columns at 29 a pass go as 20 + 19
    p.lds_bytes = p.cols * p.stride * (int)sizeof(float);
    p.tiles_max = featnorm_tiles(max_frames, p.F);
    // a table pays once its 2 W - 1 evaluations are few beside the outputs that read it; only utterances of at least W frames do
    p.table = mode == FEATNORM_WARP && max_frames >= window && max_frames >= (4 * (2 * (int64_t)window - 1) + dim - 1) / dim;
    p.table_len = p.table ? 2 * window - 1 : 0;
    return true;
}

int featnorm_grid(int64_t n_tiles, int n_cu) {
    const int64_t cap = (int64_t)std::max(1, n_cu) * FEATNORM_WGS_PER_CU;
    return (int)std::max<int64_t>(1, std::min(n_tiles, cap));
}

}  // namespace sr
