// abi_diar.cpp -- who spoke when with nobody enrolled (diar.hip): the base segments' statistics, the delta-BIC of every pair of given
// statistics, the whole chain on a feature batch and from resident PCM, the merge loop on a caller's matrix, the plan and the re-cut
// of a merge log.  Every argument is checked before the device is touched.
#include "abi_internal.hpp"

#include "diar.hpp"
#include "diar_plan.hpp"
#include "mfcc.hpp"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

using namespace sr;

namespace {

DiarParams checked_params(const char *what, int D, int L, int change, int m, double lambda, double ridge, double threshold, int k_min, int k_max) {
    DiarParams p;
    p.L = L;
    p.change = change;
    p.m = m;
    p.lambda = lambda;
    p.ridge = ridge;
    p.threshold = threshold;
    p.k_min = k_min;
    p.k_max = k_max;
    std::string why;
    if (!diar_check_params(D, p, why)) fail("%s: %s", what, why.c_str());
    return p;
}

// the chain on a feature batch; the per-cluster outputs hold `cap` entries (the batch's base segments are always enough)
void cluster_into(const char *what, SRBatch &feat, const DiarParams &prm, int64_t cap, int64_t *init_cl_off_out, int64_t *init_off_out,
                  int32_t *merge_i_out, int32_t *merge_j_out, double *merge_d_out, int32_t *label_out, int64_t *n_merges_out,
                  int64_t *n_clusters_out, int64_t *fail_out) {
    DiarResult r;
    diar_cluster_batch(feat, prm, r);
    const int U = feat.n_utt;
    const int64_t n_cl = r.init_cl_off[(size_t)U];
    if (n_cl > cap) fail("%s: %lld initial clusters, the outputs hold %lld (the batch's base segments, sr_diar_segments, are enough)", what,
                         (long long)n_cl, (long long)cap);
    std::copy(r.init_cl_off.begin(), r.init_cl_off.end(), init_cl_off_out);
    std::copy(r.init_off.begin(), r.init_off.end(), init_off_out);
    std::copy(r.label.begin(), r.label.end(), label_out);
    if (merge_i_out) std::copy(r.merge_i.begin(), r.merge_i.end(), merge_i_out);
    if (merge_j_out) std::copy(r.merge_j.begin(), r.merge_j.end(), merge_j_out);
    if (merge_d_out) std::copy(r.merge_d.begin(), r.merge_d.end(), merge_d_out);
    for (int u = 0; u < U; u++) {
        if (n_merges_out) n_merges_out[u] = r.n_merges[(size_t)u];
        if (n_clusters_out) n_clusters_out[u] = r.n_clusters[(size_t)u];
        if (fail_out) fail_out[u] = r.fail[(size_t)u];
    }
}

}  // namespace

extern "C" {

int64_t sr_diar_segments(int64_t n_frames, int64_t L) { return diar_segments(n_frames, L); }

int sr_diar_plan(int D, int L, int change, const int64_t *lengths, int U, int64_t scratch_bytes, int64_t *out, int n_out,
                 int32_t *group_begin_out, int64_t *rec_out) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 16) fail("sr_diar_plan writes 16 fields");
    DiarParams prm;
    prm.L = L;
    prm.change = change;
    if (scratch_bytes <= 0) scratch_bytes = (int64_t)diar_scratch_mib() << 20;
    DiarPlan p;
    std::string why;
    if (!plan_diar(D, prm, lengths, U, scratch_bytes, p, why)) fail("sr_diar_plan: %s", why.c_str());
    int64_t total = 0;
    for (int u = 0; u < U; u++) total += p.bytes[(size_t)u];
    const int n_groups = p.group_begin.empty() ? 0 : (int)p.group_begin.size() - 1;
    const int64_t v[16] = {p.bucket, p.stat_len, p.entries_per_lane, DIAR_STATS_WG, DIAR_STATS_CHUNK, p.stats_lds_bytes, p.change_lds_bytes,
                           n_groups, DIAR_MAX_D, DIAR_MAX_INIT, DIAR_WAVES, DIAR_ARGMIN_BLOCKS, DIAR_CADENCE, total, scratch_bytes, 0};
    for (int i = 0; i < 16; i++) out[i] = v[i];
    if (group_begin_out)
        for (int g = 0; g <= n_groups && U > 0; g++) group_begin_out[g] = p.group_begin[(size_t)g];
    if (rec_out)
        for (int u = 0; u < U; u++) {
            rec_out[3 * u] = p.n_seg[(size_t)u];
            rec_out[3 * u + 1] = p.n_init_bound[(size_t)u];
            rec_out[3 * u + 2] = p.bytes[(size_t)u];
        }
    return n_groups;
    SR_CATCH(-1)
}

int sr_diar_stats_batch(SRBatch *features, int L, int64_t cap, int64_t *seg_off_out, double *stats_out) {
    SR_TRY
    if (!features || !seg_off_out) fail("sr_diar_stats_batch: null argument");
    if (features->kind != SRBatch::FEATURES) fail("sr_diar_stats_batch takes a feature batch");
    checked_params("sr_diar_stats_batch", features->dim, L, DIAR_CHANGE_BIC, 1, 1.0, 0.0, 0.0, 1, 0);
    int64_t n_seg = 0;
    for (int u = 0; u < features->n_utt; u++) n_seg += diar_segments(features->offsets[(size_t)u + 1] - features->offsets[(size_t)u], L);
    if (n_seg > cap) fail("sr_diar_stats_batch: %lld base segments, the output holds %lld (sr_diar_segments counts them)", (long long)n_seg, (long long)cap);
    if (n_seg > 0 && !stats_out) fail("sr_diar_stats_batch: null output (the statistics)");
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_diar_stats_batch");
    diar_stats_batch(*features, L, seg_off_out, stats_out);
    return 0;
    SR_CATCH(-1)
}

int sr_diar_bic_matrix(int D, int64_t n, const double *stats, double lambda, double ridge, double *out, double *ld_out, int64_t *fail_out) {
    SR_TRY
    checked_params("sr_diar_bic_matrix", D, 1, DIAR_CHANGE_BIC, 1, lambda, ridge, 0.0, 1, 0);
    if (n < 0 || n > DIAR_MAX_INIT) fail("sr_diar_bic_matrix: %lld clusters; one call takes 0 .. %d", (long long)n, DIAR_MAX_INIT);
    if (n > 0 && (!stats || !out)) fail("sr_diar_bic_matrix: null argument");
    const int P = diar_stat_len(D);
    for (int64_t c = 0; c < n; c++) {
        if (!(stats[c * P] >= 1.0) || !std::isfinite(stats[c * P]))
            fail("sr_diar_bic_matrix: cluster %lld holds %g frames; a cluster holds at least one", (long long)c, stats[c * P]);
        for (int e = 1; e < P; e++)
            if (!std::isfinite(stats[c * P + e])) fail("sr_diar_bic_matrix: cluster %lld holds a non-finite statistic at entry %d", (long long)c, e);
    }
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_diar_bic_matrix");
    diar_bic_matrix(D, n, stats, lambda, ridge, out, ld_out, fail_out);
    return 0;
    SR_CATCH(-1)
}

int sr_diar_cluster_batch(SRBatch *features, int L, int change, int m, double lambda, double ridge, double threshold, int k_min, int k_max,
                          int64_t cap, int64_t *init_cl_off_out, int64_t *init_off_out, int32_t *merge_i_out, int32_t *merge_j_out,
                          double *merge_d_out, int32_t *label_out, int64_t *n_merges_out, int64_t *n_clusters_out, int64_t *fail_out) {
    SR_TRY
    if (!features) fail("sr_diar_cluster_batch: null argument");
    if (features->kind != SRBatch::FEATURES) fail("sr_diar_cluster_batch takes a feature batch; sr_diar_cluster_pcm_batch takes PCM");
    const DiarParams prm = checked_params("sr_diar_cluster_batch", features->dim, L, change, m, lambda, ridge, threshold, k_min, k_max);
    if (!init_cl_off_out || !init_off_out || (cap > 0 && !label_out))
        fail("sr_diar_cluster_batch: null output (the cluster offsets, the run boundaries and the labels are required)");
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_diar_cluster_batch");
    cluster_into("sr_diar_cluster_batch", *features, prm, cap, init_cl_off_out, init_off_out, merge_i_out, merge_j_out, merge_d_out, label_out,
                 n_merges_out, n_clusters_out, fail_out);
    return 0;
    SR_CATCH(-1)
}

int sr_diar_cluster_pcm_batch(SRMfcc *mf, SRBatch *pcm, int nd, int L, int change, int m, double lambda, double ridge, double threshold,
                              int k_min, int k_max, int64_t cap, int64_t *init_cl_off_out, int64_t *init_off_out, int32_t *merge_i_out,
                              int32_t *merge_j_out, double *merge_d_out, int32_t *label_out, int64_t *n_merges_out, int64_t *n_clusters_out,
                              int64_t *fail_out) {
    SR_TRY
    if (!mf || !pcm) fail("sr_diar_cluster_pcm_batch: null argument");
    if (pcm->kind == SRBatch::FEATURES) fail("sr_diar_cluster_pcm_batch takes a PCM batch; sr_diar_cluster_batch takes features");
    if (nd < 0 || nd > 2) fail("sr_diar_cluster_pcm_batch: nd is %d; 0, 1 or 2 orders of deltas", nd);
    const DiarParams prm = checked_params("sr_diar_cluster_pcm_batch", (mf->n_ceps + mf->n_lpc) * (nd + 1), L, change, m, lambda, ridge, threshold,
                                          k_min, k_max);
    if (!init_cl_off_out || !init_off_out || (cap > 0 && !label_out))
        fail("sr_diar_cluster_pcm_batch: null output (the cluster offsets, the run boundaries and the labels are required)");
    {
        // the plan's refusals (a recording above the bound, more than 4096 initial clusters in uniform mode) from the frame counts
        // the feature stage will produce: before the device is touched
        std::vector<int64_t> frames((size_t)pcm->n_utt);
        for (int u = 0; u < pcm->n_utt; u++)
            frames[(size_t)u] = std::max<int64_t>(0, mfcc_num_frames(*mf, pcm->offsets[(size_t)u + 1] - pcm->offsets[(size_t)u]) - nd);
        DiarPlan pl;
        std::string why;
        if (!plan_diar((mf->n_ceps + mf->n_lpc) * (nd + 1), prm, frames.data(), pcm->n_utt, (int64_t)diar_scratch_mib() << 20, pl, why))
            fail("sr_diar_cluster_pcm_batch: %s", why.c_str());
    }
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_diar_cluster_pcm_batch");
    ensure_device();
    SRBatch *feat_ws = &per_device<SRBatch>();   // the fused calls' feature workspace: nothing leaves the device
    mfcc_extract_batch(*mf, *pcm, nd, 1, *feat_ws);
    cluster_into("sr_diar_cluster_pcm_batch", *feat_ws, prm, cap, init_cl_off_out, init_off_out, merge_i_out, merge_j_out, merge_d_out, label_out,
                 n_merges_out, n_clusters_out, fail_out);
    return 0;
    SR_CATCH(-1)
}

int sr_ahc_matrix(int64_t n, const double *dist, int linkage, double threshold, int k_min, int k_max, int32_t *merge_i_out, int32_t *merge_j_out,
                  double *merge_d_out, int64_t *n_merges_out, int32_t *label_out, int64_t *n_clusters_out) {
    SR_TRY
    std::string why;
    if (!ahc_check_stop(threshold, k_min, k_max, why)) fail("sr_ahc_matrix: %s", why.c_str());
    if (!ahc_check_matrix(n, dist, linkage, why)) fail("sr_ahc_matrix: %s", why.c_str());
    if (!n_merges_out || !n_clusters_out || (n > 0 && !label_out) || (n > 1 && (!merge_i_out || !merge_j_out || !merge_d_out)))
        fail("sr_ahc_matrix: null output");
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_ahc_matrix");
    ahc_matrix(n, dist, linkage, threshold, k_min, k_max, merge_i_out, merge_j_out, merge_d_out, n_merges_out, label_out, n_clusters_out);
    return 0;
    SR_CATCH(-1)
}

int64_t sr_diar_cut(int64_t n, const int32_t *merge_i, const int32_t *merge_j, const double *merge_d, int64_t n_merges, double threshold,
                    int k_min, int k_max, int32_t *label_out, int64_t *n_merges_out) {
    SR_TRY
    std::string why;
    if (!ahc_check_stop(threshold, k_min, k_max, why)) fail("sr_diar_cut: %s", why.c_str());
    if (n < 0 || n_merges < 0 || n_merges > std::max<int64_t>(0, n - 1)) fail("sr_diar_cut: %lld merges over %lld clusters", (long long)n_merges, (long long)n);
    if ((n_merges > 0 && (!merge_i || !merge_j || !merge_d)) || (n > 0 && !label_out)) fail("sr_diar_cut: null argument");
    const int64_t taken = diar_cut_steps(n, merge_d, n_merges, threshold, k_min, k_max);
    const int k = diar_labels(n, merge_i, merge_j, taken, label_out);
    if (k < 0) fail("sr_diar_cut: not a merge log (an index out of range, i >= j, or a cluster merged twice)");
    if (n_merges_out) *n_merges_out = taken;
    return k;
    SR_CATCH(-1)
}

}  // extern "C"
