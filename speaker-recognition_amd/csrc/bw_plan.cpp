// bw_plan.cpp -- the decisions of the batched Baum-Welch statistics call (bw_plan.hpp).  Host-only.
#include "bw_plan.hpp"

#include <algorithm>
#include <cstdio>

namespace sr {

static std::string fmt(const char *f, long long a = 0, long long b = 0) {
    char buf[320];
    snprintf(buf, sizeof buf, f, a, b);
    return buf;
}

// the padded widths the vector layout packs rows of up to BW_MAX_DIM dimensions at (model_pack.cpp: pick_padded_dim)
static int bw_padded_dim(int D) {
    static const int dims[] = {8, 13, 16, 24, 26, 32, 34, 39, 40};
    for (int d : dims)
        if (d >= D) return d;
    return 0;
}

bool bw_check(bool batch_is_features, int S, int model, int K, int D, int feat_dim, std::string &why) {
    if (S < 1) {
        why = "Baum-Welch statistics: empty model set";
        return false;
    }
    if (!batch_is_features) {
        why = "Baum-Welch statistics take a feature batch: extract the PCM batch first (sr_mfcc_extract_batch)";
        return false;
    }
    if (model < 0 || model >= S) {
        why = fmt("Baum-Welch statistics: model index %lld outside [0, %lld); pass the column the UBM was packed at", model, S);
        return false;
    }
    if (K < 1 || D < 1) {
        why = "Baum-Welch statistics: the model has no mixtures";
        return false;
    }
    if (D > BW_MAX_DIM) {
        why = fmt("Baum-Welch statistics are built for rows of up to %lld dimensions, the model has %lld", BW_MAX_DIM, D);
        return false;
    }
    if (K > BW_MAX_MIXTURES) {
        why = fmt("Baum-Welch statistics: %lld mixtures, at most %lld", K, BW_MAX_MIXTURES);
        return false;
    }
    if (feat_dim != D) {
        why = fmt("Baum-Welch statistics: feature dim %lld != model dim %lld", feat_dim, D);
        return false;
    }
    return true;
}

int64_t bw_range_rows(int64_t len, int /*K*/, int /*D*/, int64_t range_frames) {
    if (range_frames > 0) return range_frames;
    // a long utterance keeps a bounded number of slabs: whole tiles, so that only its last range has a ragged one
    const int64_t per = (len + BW_MAX_AUTO_RANGES - 1) / BW_MAX_AUTO_RANGES;
    return std::max<int64_t>(BW_DEFAULT_RANGE, (per + BW_TILE - 1) / BW_TILE * BW_TILE);
}

bool plan_bw(int K, int D, const int64_t *lengths, int64_t U, int64_t range_frames, int64_t scratch_bytes, int n_cu, BwPlan &p,
             std::string &why) {
    p = BwPlan();
    if (!bw_check(true, 1, 0, K, D, D, why)) return false;
    if (U < 0 || (U > 0 && !lengths)) {
        why = "Baum-Welch statistics: bad utterance table";
        return false;
    }
    if (range_frames < 0 || range_frames > BW_MAX_RANGE_FRAMES) {
        why = fmt("bw_range_frames must be 0 (automatic) or 1 .. %lld frames", BW_MAX_RANGE_FRAMES);
        return false;
    }
    if (n_cu < 1) {
        why = "Baum-Welch statistics: the plan needs the number of compute units";
        return false;
    }
    p.dp = bw_padded_dim(D);
    p.ncb = (p.dp + 1 + 15) / 16;
    p.n_mix_blocks = (K + BW_WG_MIX - 1) / BW_WG_MIX;
    p.slab_bytes = (int64_t)p.n_mix_blocks * BW_WG_MIX * p.ncb * 16 * (int64_t)sizeof(double);
    p.range_frames = range_frames;
    if (scratch_bytes < p.slab_bytes) {
        why = fmt("Baum-Welch statistics: the scratch bound of %lld bytes is below one range's slab of %lld; raise the option bw_scratch_mib",
                  scratch_bytes, p.slab_bytes);
        return false;
    }
    p.stats_lds = (BW_WG_MIX / 4) * (2 * p.dp + 1) * 16 + p.dp * (BW_TILE + 2) * 4 + BW_WG_MIX * (BW_TILE + 2) * 4;
    p.reduce_blocks = ((int64_t)K * (D + 1) + BW_WG - 1) / BW_WG;
    int64_t first = 0;
    for (int64_t u = 0; u < U; u++) {
        const int64_t len = lengths[u];
        if (len < 0) {
            why = fmt("Baum-Welch statistics: utterance %lld has a negative length", u);
            return false;
        }
        if (u > INT32_MAX || len > ((int64_t)1 << 38) - first) {       // (a range's rows and the launch dimensions are int32)
            why = "Baum-Welch statistics: more than 2^31 - 1 utterances or 2^38 frames in one batch";
            return false;
        }
        const int64_t rows = bw_range_rows(len, K, D, range_frames);
        for (int64_t r0 = 0; r0 < len; r0 += rows)
            p.ranges.push_back(BwRange{first + r0, (int32_t)std::min(rows, len - r0), (int32_t)u});
        first += len;
    }
    p.lse_grid = (first + BW_WG - 1) / BW_WG;
    const int64_t n = (int64_t)p.ranges.size();
    // (the ranges of a group are the statistics launch's grid x)
    p.group_ranges = std::min<int64_t>(scratch_bytes / p.slab_bytes, (int64_t)1 << 30);
    p.n_groups = (n + p.group_ranges - 1) / p.group_ranges;
    const int64_t largest = std::min(n, p.group_ranges);
    p.stats_rounds = (largest * p.n_mix_blocks + 2 * (int64_t)n_cu - 1) / (2 * (int64_t)n_cu);
    return true;
}

}  // namespace sr
