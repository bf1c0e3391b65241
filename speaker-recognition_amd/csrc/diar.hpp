// diar.hpp -- who spoke when with nobody enrolled, on the device (diar.hip): per-segment full-covariance statistics, BIC change
// detection, agglomerative clustering under delta-BIC; the same merge loop on a caller's dissimilarity matrix.
#pragma once

#include "diar_plan.hpp"

#include <cstdint>
#include <vector>

struct SRBatch;

namespace sr {

// Statistics of the base segments of every recording of a feature batch, brought home: seg_off_out [U + 1] (segment offsets of
// the recordings), stats_out [n_seg_total][diar_stat_len(D)].
void diar_stats_batch(SRBatch &feat, int L, int64_t *seg_off_out, double *stats_out);

// delta-BIC of every pair of n clusters from statistics in host memory [n][diar_stat_len(D)]: out [n][n] (symmetric, 0 on the
// diagonal, +inf where a factorisation failed), ld_out [n] (NaN where the cluster's own failed), *fail_out the count of those.
void diar_bic_matrix(int D, int64_t n, const double *stats, double lambda, double ridge, double *out, double *ld_out, int64_t *fail_out);

// The whole chain's results, recording by recording (offsets over the batch).
struct DiarResult {
    std::vector<int64_t> init_cl_off;    // [U + 1] initial clusters of the recordings
    std::vector<int64_t> init_off;       // [n_init_total + U] per recording n_init + 1 run boundaries, in base-segment indices
    std::vector<int32_t> merge_i, merge_j, label;    // [n_init_total] (a recording's first n_merges entries are its log)
    std::vector<double> merge_d;         // [n_init_total]
    std::vector<int64_t> n_merges, n_clusters, fail, n_seg;     // [U]
};

void diar_cluster_batch(SRBatch &feat, const DiarParams &prm, DiarResult &out);

// The merge loop on a symmetric dissimilarity matrix [n][n] in host memory.  merge_* [max(n - 1, 0)], label_out [n].
void ahc_matrix(int64_t n, const double *dist, int linkage, double threshold, int k_min, int k_max, int32_t *merge_i, int32_t *merge_j,
                double *merge_d, int64_t *n_merges_out, int32_t *label_out, int64_t *n_clusters_out);

void set_diar_scratch_mib(long v);
long diar_scratch_mib();

}  // namespace sr
