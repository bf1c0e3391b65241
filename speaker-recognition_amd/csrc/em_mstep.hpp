// em_mstep.hpp -- the host's float64 half of an EM / MAP iteration (train_em, em.hip): everything between the statistics coming
// back from the device and the next model -- re-centring of sums taken about the origin, the float64 redo of mixtures without
// fp32 support, the M-step with the reference's formulas (gmm.cc:388-437, :502-509; gmmubm.cc:53-74) and the stop rule
// (gmm.cc:643-650).  Host-only C++17, nothing of HIP: tests/host/em_checks.cpp runs it under the host sanitizers.
// (em_small.hip and em_f64_dev.hpp restate the M-step for the device, under the device's contraction rules; they stay apart.)
#pragma once

#include <vector>

namespace sr {

// An iteration's sums: stats[k * rec + ..], rec = 2 DP + 1: [d] sum g (x_d - m_kd), [DP + d] sum g (x_d - m_kd)^2, [2 DP] sum g,
// m = the model's mean rounded to fp32 (what the device centres on).
struct EmModelRef {             // a model's parameters where they live (GMM: gmm_model.hpp), sigma = standard deviations
    int K, dim;
    double *weights, *mean, *sigma;
};

// sums about the ORIGIN (the matrix-core forms: T1 = sum g x, T2 = sum g x^2, N) -> the centred ones, in place
void recentre_origin_sums(double *stats, int DP, const EmModelRef &m);

// the mixtures whose occupancy is below 1e-25: a responsibility below fp32's range (~1e-38) is 0 on the device, while the
// reference's float64 keeps it down to DBL_MIN
std::vector<int> weak_mixtures(const double *stats, int DP, int K);

// mixture k's three sums again in float64 with the reference's rules (terms below DBL_MIN are 0; frames whose likelihood `ll`
// underflowed carry none), into its row of stats.  X: [n][dim] frames, ll: [n] natural-log likelihoods under the model.
void redo_weak_mixture(double *stats, int DP, const EmModelRef &m, int k, const float *X, long n, const float *ll);

// ... of every mixture in `weak`, dealt to at most max_threads host threads (one below 2^20 mixture-frame-dimensions of work):
// each mixture writes its own row, in the same order of operations -- the same bits for any number of threads
void redo_weak_mixtures(double *stats, int DP, const EmModelRef &m, const std::vector<int> &weak, const float *X, long n, const float *ll,
                        int max_threads = 16);

// The M-step, in place.  ubm_mean == nullptr: EM -- weights, means, sigmas (floored at min_sigma).  Else MAP: the means alone,
// alpha = N_k / (N_k + relevance) between the data's and the UBM's.  A mixture without any responsibility (N_k an exact 0) has
// E_k[x] = 0, not its old mean (the reference divides exact zeros by min_n_k = 1e-6).
void em_mstep(const double *stats, int DP, const EmModelRef &m, long n, const double *ubm_mean, double relevance, double min_sigma);

// gmm.cc:643-650, checked after every second iteration
bool em_converged(double ll, double last_ll, double threshold);

}  // namespace sr
