// abi_fullcov.cpp -- full-covariance models and sets.
#include "abi_internal.hpp"

#include "gmm_full.hpp"
#include "mfcc.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace sr;

extern "C" {

// ---- full-covariance GMMs (gmm_full.hip) ----
SRFullGMM *sr_fullgmm_create(int K, int D, const double *weights, const double *means, const double *prec_chol) {
    SR_TRY
    if (K < 1) fail("n_components must be >= 1 (got %d)", K);
    if (D < 1 || D > FULL_MAX_D) fail("full-covariance models support 1 <= D <= %d dims (got %d)", FULL_MAX_D, D);
    const int given = (weights != nullptr) + (means != nullptr) + (prec_chol != nullptr);
    if (given != 0 && given != 3) fail("give weights, means and prec_chol together, or none of them");
    auto g = std::make_unique<SRFullGMM>();
    g->K = K;
    g->D = D;
    if (given) {
        g->weights.assign(weights, weights + K);
        g->means.assign(means, means + (size_t)K * D);
        g->prec_chol.assign(prec_chol, prec_chol + (size_t)K * D * D);
        for (int k = 0; k < K; k++) {
            if (!(g->weights[k] >= 0.0) || !std::isfinite(g->weights[k])) fail("weight %d is not a finite value >= 0", k);
            for (int i = 0; i < D; i++) {
                if (!(g->prec_chol[((size_t)k * D + i) * D + i] > 0.0)) fail("precisions_cholesky[%d] has a diagonal entry <= 0", k);
                for (int j = 0; j < i; j++)
                    if (g->prec_chol[((size_t)k * D + i) * D + j] != 0.0) fail("precisions_cholesky[%d] is not upper triangular", k);
            }
        }
        for (double v : g->means)
            if (!std::isfinite(v)) fail("means must be finite");
        for (double v : g->prec_chol)
            if (!std::isfinite(v)) fail("precisions_cholesky must be finite");
        g->trained = true;
    }
    return g.release();
    SR_CATCH(nullptr)
}

int sr_fullgmm_fit(SRFullGMM *g, const double *X, int64_t n, int D, const SRFullFitParams *params, SRFullFitStats *out) {
    SR_TRY
    if (!g || !X || !params || !out) fail("null argument");
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_fullgmm_fit");
    fullgmm_fit(*g, X, (long)n, D, *params, *out);
    return 0;
    SR_CATCH(-1)
}

namespace {
thread_local std::vector<std::string> g_fit_batch_messages;      // of the calling thread's last sr_fullgmm_fit_batch
}  // namespace

int sr_fullgmm_fit_batch(SRFullGMM *const *models, int S, const double *X, const int64_t *row_offsets, int D, const SRFullFitParams *params,
                         SRFullFitStats *out, int *status) {
    SR_TRY
    g_fit_batch_messages.clear();
    if (!models || !X || !row_offsets || !params || !out || !status) fail("null argument");
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_fullgmm_fit_batch");
    fullgmm_fit_batch(models, S, X, row_offsets, D, params, out, status, g_fit_batch_messages);
    return 0;
    SR_CATCH(-1)
}

const char *sr_fullgmm_fit_batch_error(int s) {
    const auto &m = g_fit_batch_messages;
    return s >= 0 && (size_t)s < m.size() ? m[(size_t)s].c_str() : "";
}

void sr_full_fit_batch_stats(long *calls, long *speakers, long *iterations) { full_fit_batch_stats(calls, speakers, iterations); }

long sr_full_fit_batch_bytes(void) { return full_fit_batch_bytes(); }

int sr_full_fit_plan(int K, int D, const int64_t *lengths, const int *init_given, const int *max_iter, int S, int64_t bound_bytes,
                     int64_t *speakers_out, int64_t *groups_out, int64_t group_cap, int64_t *out, int n_out) {
    SR_TRY
    if (!out || !lengths) fail("null argument");
    if (n_out < 7) fail("sr_full_fit_plan writes 7 fields");
    if (S < 1) fail("a plan needs at least one speaker (S = %d)", S);
    std::vector<int> given((size_t)S, 0), iters((size_t)S, 100);
    if (init_given) given.assign(init_given, init_given + S);
    if (max_iter) iters.assign(max_iter, max_iter + S);
    FullFitPlan p;
    std::string why;
    if (!plan_full_fit(K, D, lengths, given.data(), iters.data(), S, bound_bytes == 0 ? (int64_t)full_fit_batch_bytes() : bound_bytes, p, why))
        fail("%s", why.c_str());
    const int64_t v[7] = {(int64_t)p.groups.size(), (int64_t)p.wl_lp.size(), (int64_t)p.wl_lse.size(), (int64_t)p.wl_cov.size(),
                          (int64_t)p.lds_logprob, p.max_group_bytes, full_speaker_bytes(K, D, lengths[0])};
    std::memcpy(out, v, sizeof v);
    if (speakers_out)
        for (int s = 0; s < S; s++) {
            const FullSpeakerPlan &sp = p.speakers[(size_t)s];
            const int64_t r[8] = {sp.n, sp.row0, sp.n_chunks, sp.chunk, sp.o_partial, sp.bytes, sp.group, sp.slot};
            std::memcpy(speakers_out + 8 * (size_t)s, r, sizeof r);
        }
    if (groups_out)
        for (int64_t g = 0; g < std::min<int64_t>((int64_t)p.groups.size(), group_cap); g++) {
            const FullGroupPlan &gp = p.groups[(size_t)g];
            const FullCounts &c = gp.counts;
            const int64_t r[28] = {gp.first, gp.count, gp.rows, gp.lp0, gp.lse0, gp.cov0, gp.max_iter, gp.any_kmeans, gp.any_given, gp.bytes,
                                   c.X, c.w, c.logw, c.mu, c.prec, c.logdet, c.cov, c.lp, c.lpn, c.nk, c.partial, c.head,
                                   c.spk, c.rec, c.wl_lp, c.wl_lse, c.wl_cov, c.label};
            std::memcpy(groups_out + 28 * g, r, sizeof r);
        }
    return 7;
    SR_CATCH(-1)
}

int sr_fullgmm_info(SRFullGMM *g, int *K, int *D) {
    SR_TRY
    if (!g) fail("null handle");
    if (K) *K = g->K;
    if (D) *D = g->D;
    return g->trained ? 1 : 0;
    SR_CATCH(-1)
}

int sr_fullgmm_get(SRFullGMM *g, double *weights, double *means, double *covariances, double *prec_chol) {
    SR_TRY
    if (!g) fail("null handle");
    if (!g->trained) fail("the model has no parameters yet (fit it first)");
    const size_t K = g->K, D = g->D;
    if (weights) std::memcpy(weights, g->weights.data(), sizeof(double) * K);
    if (means) std::memcpy(means, g->means.data(), sizeof(double) * K * D);
    if (prec_chol) std::memcpy(prec_chol, g->prec_chol.data(), sizeof(double) * K * D * D);
    if (covariances) {
        if (g->covariances.empty()) std::memset(covariances, 0, sizeof(double) * K * D * D);
        else std::memcpy(covariances, g->covariances.data(), sizeof(double) * K * D * D);
    }
    return 0;
    SR_CATCH(-1)
}

void sr_fullgmm_free(SRFullGMM *g) { delete g; }

SRFullSet *sr_fullset_create(SRFullGMM *const *models, int S) {
    SR_TRY
    if (!models) fail("null argument");
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_fullset_create");
    auto set = std::make_unique<SRFullSet>();
    fullset_pack(*set, models, S);
    return set.release();
    SR_CATCH(nullptr)
}

int sr_fullset_score_batch(SRFullSet *set, SRBatch *batch, double *sums_out, int *argmax_out, float *frame_ll_out) {
    SR_TRY
    if (!set || !batch) fail("null argument");
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_fullset_score_batch");
    fullset_score(*set, *batch, sums_out, argmax_out, frame_ll_out);
    return 0;
    SR_CATCH(-1)
}

int sr_fullset_predict_pcm_batch(SRMfcc *m, SRFullSet *set, SRBatch *pcm, int nd, double *sums_out, int *argmax_out) {
    SR_TRY
    if (!m || !set || !pcm) fail("null argument");
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_fullset_predict_pcm_batch");
    fullset_predict_pcm(*m, *set, *pcm, nd, sums_out, argmax_out);
    return 0;
    SR_CATCH(-1)
}

void sr_fullset_free(SRFullSet *set) { delete set; }

}  // extern "C"
