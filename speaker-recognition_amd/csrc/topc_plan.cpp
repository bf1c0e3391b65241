// topc_plan.cpp -- the decisions of the top-C scoring path (topc_plan.hpp).  Host-only.
#include "topc_plan.hpp"

#include <algorithm>
#include <cstdio>

namespace sr {

static std::string fmt(const char *f, long long a = 0, long long b = 0) {
    char buf[320];
    snprintf(buf, sizeof buf, f, a, b);
    return buf;
}

bool topc_check(bool tied, int S, int K, int D, int bg, int top_c, bool batch_is_features, std::string &why) {
    if (S < 1 || K < 1 || D < 1) {
        why = "top-C scoring: empty model set";
        return false;
    }
    if (!batch_is_features) {
        why = "top-C scoring takes a feature batch: extract the PCM batch first (sr_mfcc_extract_batch) or call sr_predict_pcm_batch_topc";
        return false;
    }
    if (!tied) {
        why = "top-C scoring needs models that share sigma and weights with the background model (speakers MAP-adapted from one UBM, "
              "means only); score this set with sr_score_batch_set";
        return false;
    }
    if (bg < 0 || bg >= S) {
        why = fmt("top-C scoring: background column %lld outside [0, %lld); pass the column the UBM was packed at", bg, S);
        return false;
    }
    if (top_c < 1 || top_c > K) {
        why = fmt("top-C scoring: top_c %lld outside [1, %lld] (the models' mixture count); choose 1 <= top_c <= K", top_c, K);
        return false;
    }
    if (D > TOPC_MAX_DIM) {
        why = fmt("top-C scoring is built for rows of up to %lld dimensions, the set has %lld; score it with sr_score_batch_set", TOPC_MAX_DIM, D);
        return false;
    }
    if (top_c > TOPC_MAX_REG_C && K > TOPC_MAX_RANK_K) {
        why = fmt("top-C scoring: top_c above %lld needs models of at most %lld mixtures; lower top_c", TOPC_MAX_REG_C, TOPC_MAX_RANK_K);
        return false;
    }
    return true;
}

bool plan_topc(int K, int D, int S, int top_c, int64_t n_frames, int64_t scratch_bytes, int n_cu, TopcPlan &p, std::string &why) {
    p = TopcPlan();
    if (!topc_check(true, S, K, D, 0, top_c, true, why)) return false;
    if (n_frames < 0) {
        why = "top-C scoring: negative frame count";
        return false;
    }
    if (n_cu < 1) {
        why = "top-C scoring: the plan needs the number of compute units";
        return false;
    }
    const int64_t C = top_c;
    p.tp = D <= 16 ? 16 : D <= 40 ? 40 : 64;
    p.cr = C == 1 ? 1 : C <= 5 ? 5 : C <= TOPC_MAX_REG_C ? TOPC_MAX_REG_C : 0;
    p.row_bytes = C * (int64_t)S * 4 + C * 8 + 4 + (p.cr == 0 ? (int64_t)K * 4 : 0);
    if (scratch_bytes < p.row_bytes) {
        why = fmt("top-C scoring: the scratch bound of %lld bytes is below one frame's row of %lld; raise the option topc_scratch_mib", scratch_bytes,
                  p.row_bytes);
        return false;
    }
    p.eval_waves = (int)std::min<int64_t>(4, (S + 63) / 64);
    p.eval_grid_y = (S + 64 * p.eval_waves - 1) / (64 * p.eval_waves);
    p.combine_wg = (int)std::min<int64_t>(256, ((int64_t)S + 63) / 64 * 64);
    p.rank_lds = p.cr == 0 ? K * 4 : 0;
    if (n_frames == 0) return true;
    // a routed pair (frame of the chunk, slot) is one int32, and so are the launch dimensions
    const int64_t pair_cap = (((int64_t)1 << 31) - 1 - TOPC_WG) / C;
    p.chunk = std::min(std::min(n_frames, scratch_bytes / p.row_bytes), pair_cap);
    p.n_chunks = (n_frames + p.chunk - 1) / p.chunk;
    const int64_t entries = p.chunk * C;
    // long runs amortise a workgroup's load of its component's means; a small chunk is cut finer so that every unit gets work
    p.run = entries / 256 >= 4 * (int64_t)n_cu ? 256 : TOPC_STAGE;
    p.eval_grid_x = (entries + p.run - 1) / p.run + K;
    p.select_grid = (p.chunk + TOPC_WG - 1) / TOPC_WG;
    p.route_grid = (entries + TOPC_WG - 1) / TOPC_WG;
    return true;
}

}  // namespace sr
