// diar_plan.hpp -- what the diarisation of unknown speakers (diar.hip: per-segment full-covariance statistics, BIC change
// detection, agglomerative clustering under delta-BIC, and the same merge loop on a caller's dissimilarity matrix) decides before
// it touches the device: the refusals, the base segments of a recording, the bucket width of the wave-level factorisation, the
// workgroup shapes, the bytes a recording keeps on the device and the grouping of the recordings under the bound -- and the two
// small host functions on a merge log (the labels, a re-cut).
// Host-only C++17, nothing of HIP: diar.hip consumes it, sr_diar_plan hands it to tests, tests/host/diar_checks.cpp runs it under
// the host sanitizers.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace sr {

constexpr int DIAR_MAX_D = 64;                  // the factorisation keeps a row of the matrix in a lane's registers: 64 lanes, 64 rows
constexpr int DIAR_MAX_INIT = 4096;             // initial clusters of one recording (its table: 4096^2 float64 = 128 MiB)
constexpr int DIAR_STATS_WG = 256;              // lanes of the statistics, gather and argmin kernels
constexpr int DIAR_STATS_CHUNK = 64;            // frames the statistics kernel stages in LDS at a time
constexpr int DIAR_STATS_MAX_ENTRIES = 9;       // entries of (s, Q) a lane owns at most: ceil((64 + 2080) / 256)
constexpr int DIAR_WAVES = 4;                   // waves (matrices) per workgroup of the pair, row and logdet kernels
constexpr int DIAR_ARGMIN_BLOCKS = 64;          // workgroups of the argmin kernel per recording at most (rows strided over them)
constexpr int DIAR_MAX_GROUP = 65535;          // recordings of one group: they sit on the grid's y
constexpr int DIAR_CADENCE = 16;                // the host reads the stop word back after every CADENCE-th step
constexpr int DIAR_CHANGE_UNIFORM = 0, DIAR_CHANGE_BIC = 1;
constexpr int AHC_AVERAGE = 0, AHC_COMPLETE = 1, AHC_SINGLE = 2;
constexpr int64_t DIAR_DEFAULT_SCRATCH = (int64_t)1024 << 20;

// the widths the factorisation is instantiated on: D rounded up (register indexing is static)
constexpr int diar_bucket(int D) { return D <= 16 ? 16 : D <= 32 ? 32 : D <= 48 ? 48 : 64; }
constexpr int diar_tri(int D) { return D * (D + 1) / 2; }
// the statistics of a segment or a cluster: N, s [D], Q [D (D + 1) / 2] (lower triangle by rows), float64
constexpr int diar_stat_len(int D) { return 1 + D + diar_tri(D); }

// base segments of a recording of n frames: floor(n / L), 1 if that is 0 and n > 0, 0 if n <= 0 (or L < 1)
int64_t diar_segments(int64_t n, int64_t L);

struct DiarParams {
    int L = 100;               // frames per base segment
    int change = DIAR_CHANGE_BIC;
    int m = 2;                 // half-width of the change detector, in segments
    double lambda = 1.0;       // the BIC penalty's weight
    double ridge = 1e-3;       // added to the covariance's diagonal
    double threshold = 0.0;    // a pair merges while its distance is below
    int k_min = 1, k_max = 0;  // never fewer clusters than k_min; k_max > 0: merge until at most k_max, whatever the distance
};

// The refusals of the parameters; true, or false with the text (it names the remedy).
bool diar_check_params(int D, const DiarParams &p, std::string &why);
bool ahc_check_stop(double threshold, int k_min, int k_max, std::string &why);
// The matrix's: n, the linkage, a NaN or -inf entry, asymmetry.
bool ahc_check_matrix(int64_t n, const double *dist, int linkage, std::string &why);

struct DiarPlan {
    int D = 0, bucket = 0, stat_len = 0, entries_per_lane = 0;
    int stats_lds_bytes = 0, change_lds_bytes = 0;
    std::vector<int64_t> n_seg;          // [U] base segments
    std::vector<int64_t> n_init_bound;   // [U] the most initial clusters the recording can have (its segments)
    std::vector<int64_t> bytes;          // [U] what the recording keeps on the device at that count
    std::vector<int32_t> group_begin;    // [n_groups + 1] recordings [g, g + 1) run together
};

// bytes of one recording with n_seg base segments and n_init initial clusters
int64_t diar_recording_bytes(int D, int64_t n_seg, int64_t n_init);
// bytes of the matrix mode's call
int64_t ahc_matrix_bytes(int64_t n);

// Fills `p` and returns true, or false with the reason: a recording whose tables exceed the bound on its own is refused with the
// byte count and the remedy; so is one of more than 4096 base segments in uniform mode (every segment is an initial cluster).
bool plan_diar(int D, const DiarParams &prm, const int64_t *lengths, int U, int64_t scratch_bytes, DiarPlan &p, std::string &why);

// Pair p of the n (n - 1) / 2 pairs i < j of n clusters in row-major order (the pair kernel's grid): row i starts at
// i (2 n - i - 1) / 2; the row from a square root (n <= 4096: exact in float64), then a bounded correction.  n >= 2, 0 <= p < n (n - 1) / 2.
#if defined(__HIPCC__)
#define SR_DIAR_HD __host__ __device__
#else
#define SR_DIAR_HD
#endif
SR_DIAR_HD inline void diar_pair_of(int64_t n, int64_t p, int64_t &i, int64_t &j) {
    int64_t r = (int64_t)(((double)(2 * n - 1) - sqrt((double)((2 * n - 1) * (2 * n - 1) - 8 * p))) / 2.0);
    r = r < 0 ? 0 : r > n - 2 ? n - 2 : r;
    while (r < n - 2 && (r + 1) * (2 * n - r - 2) / 2 <= p) r++;
    while (r > 0 && r * (2 * n - r - 1) / 2 > p) r--;
    i = r;
    j = r + 1 + (p - r * (2 * n - r - 1) / 2);
}

// argmin workgroups of a recording of n initial clusters
constexpr int diar_argmin_blocks(int64_t n) { return n < 1 ? 1 : n < DIAR_ARGMIN_BLOCKS ? (int)n : DIAR_ARGMIN_BLOCKS; }

// The labels of a merge log over n initial clusters: the root of a cluster is its smallest member, the final clusters are
// numbered by first appearance.  Uses the first `n_merges` entries; returns the number of clusters (0 for n = 0), -1 when the
// log is not one (an index out of range, i >= j, a merge of a cluster that is gone).
int diar_labels(int64_t n, const int32_t *merge_i, const int32_t *merge_j, int64_t n_merges, int32_t *label_out);
// How many steps of a log a stop rule takes: step t is taken while live > k_max (k_max > 0), or live > k_min and d[t] < threshold;
// never one whose distance is +inf.
int64_t diar_cut_steps(int64_t n, const double *merge_d, int64_t n_merges, double threshold, int k_min, int k_max);

}  // namespace sr
