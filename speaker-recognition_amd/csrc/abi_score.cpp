// abi_score.cpp -- scoring a batch against a model set: exact, fused from PCM, open-set, top-C.
#include "abi_internal.hpp"

#include "mfcc.hpp"
#include "score.hpp"
#include "topc.hpp"
#include "topc_plan.hpp"

#include <algorithm>
#include <string>

using namespace sr;

// The fused serving step: PCM batch -> MFCC -> CMVN / deltas -> all models -> sums + argmax on the host, one pass.
// (Rounds 1-3 carried an option that cut the batch into chunks and ran the feature kernels of chunk i + 1 on a second stream under the
// scoring of chunk i.  It measured slower on every workload -- configs[1] 5.12 ms in one pass against 5.17 / 5.43 / 5.87 ms with 2 / 4 /
// 8 chunks, configs[2] 337 against 350 ms and later 267 against 538: next to the power-capped scoring kernel the feature launches stretch
// from 20 to 271 ms and the scoring chunks pay their tails, profiles/r02_overlap.txt -- and its second stream did not wait for the
// uploads of sr_multi_predict_pcm's pieces.  Removed in round 4.)
static void predict_unpipelined(SRMfcc *m, SRModelSet *set, SRBatch *pcm, int nd, double *sums_out, int *argmax_out,
                                int flags, const OpenSetFetch *open) {
    SRBatch *feat_ws = &per_device<SRBatch>();   // reused across steps: the serving loop allocates nothing
    mfcc_extract_batch(*m, *pcm, nd, 1, *feat_ws);
    if (open) {      // the decision kernel reads the device's sums: no delivery by finalize itself (open_set.hip)
        score_resolved(*set, *feat_ws, false, flags, 0, sums_out, argmax_out, nullptr, open);
        return;
    }
    // (small result sets land in host memory by themselves: SCORE_HOST_DELIVER, score.hpp)
    const int deliver = (sums_out && argmax_out && host_deliverable((size_t)pcm->n_utt, (size_t)set->host.n_models)) ? SCORE_HOST_DELIVER : 0;
    score_resolved(*set, *feat_ws, false, flags, deliver, sums_out, argmax_out, nullptr);
}

namespace sr {
void predict_pcm(SRMfcc *m, SRModelSet *set, SRBatch *pcm, int nd, double *sums_out, int *argmax_out, int flags,
                 const OpenSetFetch *open) {
    if (!m || !set || !pcm) fail("null argument");
    ensure_device();
    predict_unpipelined(m, set, pcm, nd, sums_out, argmax_out, flags, open);
}
}  // namespace sr

extern "C" {

int sr_score_batch_set(SRModelSet *set, SRBatch *features, double *sums_out, int *argmax_out,
                       float *frame_ll_out, int flags) {
    SR_TRY
    if (!set || !features) fail("null argument");
    score_batch_set(*set, *features, sums_out, argmax_out, frame_ll_out, flags);
    return 0;
    SR_CATCH(-1)
}

int sr_predict_pcm_batch(SRMfcc *m, SRModelSet *set, SRBatch *pcm, int nd, double *sums_out,
                         int *argmax_out, int flags) {
    SR_TRY
    predict_pcm(m, set, pcm, nd, sums_out, argmax_out, flags, nullptr);
    return 0;
    SR_CATCH(-1)
}

// ---- the open-set decision (open_set.hip).  Every argument is checked before the device is touched. ----

int sr_open_set_decide(const double *sums, int U, int S, int bg, const int64_t *n_frames, double threshold, int *label_out,
                       double *margin_out) {
    SR_TRY
    if (U < 0 || S <= 0) fail("sr_open_set_decide: bad shape (%d utterances x %d models)", U, S);
    if (!label_out || !margin_out) fail("sr_open_set_decide: null output (labels and margins are both required)");
    if (U > 0 && (!sums || !n_frames)) fail("sr_open_set_decide: null argument");
    const OpenSetRule rule{bg, threshold};
    open_set_check(rule, S);
    for (int u = 0; u < U; u++)
        if (n_frames[u] < 0) fail("sr_open_set_decide: utterance %d has a negative frame count", u);
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_open_set_decide");
    open_set_decide_host(sums, U, S, rule, n_frames, label_out, margin_out);
    return 0;
    SR_CATCH(-1)
}

int sr_score_batch_set_open(SRModelSet *set, SRBatch *features, int bg, double threshold, double *sums_out, int *label_out,
                            double *margin_out, int flags) {
    SR_TRY
    if (!set || !features) fail("sr_score_batch_set_open: null argument");
    if (!label_out || !margin_out) fail("sr_score_batch_set_open: null output (labels and margins are both required)");
    const OpenSetFetch open{{bg, threshold}, label_out, margin_out};
    open_set_check(open.rule, set->host.n_models);
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_score_batch_set_open");
    score_batch_set_open(*set, *features, sums_out, open, flags);
    return 0;
    SR_CATCH(-1)
}

int sr_predict_pcm_batch_open(SRMfcc *m, SRModelSet *set, SRBatch *pcm, int nd, int bg, double threshold, double *sums_out,
                              int *label_out, double *margin_out, int flags) {
    SR_TRY
    if (!m || !set || !pcm) fail("sr_predict_pcm_batch_open: null argument");
    if (!label_out || !margin_out) fail("sr_predict_pcm_batch_open: null output (labels and margins are both required)");
    const OpenSetFetch open{{bg, threshold}, label_out, margin_out};
    open_set_check(open.rule, set->host.n_models);
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_predict_pcm_batch_open");
    predict_pcm(m, set, pcm, nd, sums_out, nullptr, flags, &open);
    return 0;
    SR_CATCH(-1)
}

// ---- top-C Gaussian selection (gmm_topc.hip).  Every refusal comes before the device is touched. ----

int sr_score_batch_set_topc(SRModelSet *set, SRBatch *features, int bg, int top_c, double *sums_out, int *argmax_out, int *topc_out,
                            float *frame_ll_out, int flags) {
    SR_TRY
    if (!set || !features) fail("sr_score_batch_set_topc: null argument");
    score_batch_set_topc(*set, *features, bg, top_c, sums_out, argmax_out, topc_out, frame_ll_out, flags);
    return 0;
    SR_CATCH(-1)
}

int sr_predict_pcm_batch_topc(SRMfcc *m, SRModelSet *set, SRBatch *pcm, int nd, int bg, int top_c, double *sums_out, int *argmax_out,
                              int flags) {
    SR_TRY
    if (!m || !set || !pcm) fail("sr_predict_pcm_batch_topc: null argument");
    if (pcm->kind == SRBatch::FEATURES) fail("sr_predict_pcm_batch_topc takes a PCM batch; score a feature batch with sr_score_batch_set_topc");
    {   // the set's and the rule's refusals before the feature stage runs (the batch is PCM here: that check is the other entry point's)
        const int K = set->host.model_mixtures.empty() ? 0 : set->host.model_mixtures[0];
        std::string why;
        if (!topc_check(topc_set_tied(*set), set->host.n_models, K, set->host.dim, bg, top_c, true, why)) fail("%s", why.c_str());
    }
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_predict_pcm_batch_topc");
    ensure_device();
    SRBatch *feat_ws = &per_device<SRBatch>();   // the fused calls' feature workspace: nothing leaves the device
    mfcc_extract_batch(*m, *pcm, nd, 1, *feat_ws);
    score_batch_set_topc(*set, *feat_ws, bg, top_c, sums_out, argmax_out, nullptr, nullptr, flags);
    return 0;
    SR_CATCH(-1)
}

int sr_topc_plan(int K, int D, int S, int top_c, int64_t n_frames, int64_t scratch_bytes, int n_cu, int32_t *out, int n_out) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 16) fail("sr_topc_plan writes 16 fields");
    n_cu = plan_n_cu(n_cu);
    TopcPlan p;
    std::string why;
    if (!plan_topc(K, D, S, top_c, n_frames, scratch_bytes, n_cu, p, why)) fail("%s", why.c_str());
    const int64_t v[16] = {p.tp, p.cr, p.row_bytes, p.chunk, p.n_chunks, p.run, TOPC_STAGE, p.eval_waves, p.eval_grid_x, p.eval_grid_y,
                           p.select_grid, p.route_grid, p.combine_wg, TOPC_TILE, p.rank_lds, 0};
    for (int i = 0; i < 16; i++) out[i] = (int32_t)std::min<int64_t>(v[i], INT32_MAX);
    return 16;
    SR_CATCH(-1)
}

}  // extern "C"
