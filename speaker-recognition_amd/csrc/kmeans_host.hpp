// kmeans_host.hpp -- the reference's initialisation of a GMM before EM, decision for decision, stage by stage:
// GMMTrainerBaseline::init_gaussians (src/gmm/src/gmm.cc:306-361): data variance, then either K random frames
// (init_with_kmeans = 0, the reference's default) or k-means|| (KMeansIISolver::cluster, kmeansII.cc:82-171: oversampling rounds
// -> weighted k-means++ on the candidates, kmeans++.cc:161-212 -> weighted Lloyd, kmeans.cc:249-342 -> Lloyd on the full data,
// kmeans.cc:150-246).  Every draw is the reference's, in its order (ref_rand.hpp); every sum that feeds a decision is formed in
// float64 in the reference's order (per worker block of ceil(n / concurrency) points, then over the blocks).
// The O(n K D) part -- nearest centre and squared distance of every point, and the cluster sums of a Lloyd step on the full data
// -- belongs to a back end of two operations (kmeans_init.hip: the device; tests/host/kmeans_checks.cpp: a plain loop).
// Host-only C++17, nothing of HIP.
#pragma once

#include "kmeans_plan.hpp"
#include "ref_rand.hpp"

#include <cmath>
#include <functional>
#include <string>
#include <vector>

namespace sr {

struct KmBackend {
    // Nearest centre among centres [c_begin, c_end) of C [c_end][dim]: dist[i] / belong[i] are updated when a centre is STRICTLY
    // closer (kmeansII.cc:59-72); reset: a fresh search (dist = DBL_MAX, no centre yet: the full search of kmeans.cc:87-99), the
    // vectors are not read.  download = false: the result stays with the back end for lloyd_sums, the vectors are not written.
    std::function<void(const std::vector<double> &C, int c_begin, int c_end, std::vector<double> &dist, std::vector<int> &belong,
                       bool reset, bool download)> assign;
    // Of the assignment the last assign(reset, no download) left: every worker block's sum of distances in point order -> bsum
    // [n_blocks]; per cluster the blocks' sums of their members (in point order, from 0.0) in block order, from 0.0 -> csum [K][dim];
    // the cluster sizes -> csize [K] (calc_belonging and Lloyds_iteration, kmeans.cc:72-107, :189-212).  Returns the points that
    // assignment had to look at twice (0 where there is one search only): for the caller's information, the drivers decide nothing
    // by it and a back end that counts them (kmeans_fast_stats) does so itself.
    std::function<long(const KmLloydPlan &plan, std::vector<double> &bsum, std::vector<double> &csum, std::vector<int> &csize)> lloyd_sums;
};

// ---- the stages ----
// the data's standard deviation per dimension, unbiased (gmm.cc:309-325, :352-354)
std::vector<double> data_sigma(const float *X, long n, int dim);
// K random frames (gmm.cc:346-349) -> [K][dim]
std::vector<double> random_frames_start(const float *X, long n, int dim, int K, RefRandom &trainer_random);
// sum of v[0..n) as the reference's workers form it: sequentially inside blocks of ceil(n / concurrency),
// then over the blocks (kmeansII.cc:103-129, kmeans.cc:166-187)
double blocked_sum(const std::vector<double> &v, long n, int concurrency);
// squared distance over the coordinates a sparse instance keeps (|x| >= 1e-15, kmeans++.cc:43-51, :53-60)
inline double sparse_distsqr(const double *x, const double *c, int dim) {
    double dist = 0;
    for (int d = 0; d < dim; d++) {
        if (std::fabs(x[d]) < 1e-15) continue;
        const double delta = x[d] - c[d];
        dist += delta * delta;
    }
    return dist;
}
// one oversampling round's selection (kmeansII.cc:131-141): a draw per point; the chosen rows are appended to cand [count][dim]
void oversample_round(const float *X, long n, int dim, int K, double oversampling_factor, const std::vector<double> &dist,
                      double distsqr_sum, RandStream &rs, std::vector<double> &cand);
// random rows until there are more than size_factor * K candidates (kmeansII.cc:147-150)
void top_up_candidates(const float *X, long n, int dim, int K, double size_factor, RefRandom &solver_random, std::vector<double> &cand);
// the points every candidate is nearest to (kmeansII.cc:152-155)
std::vector<double> candidate_weights(const std::vector<int> &belong, long n, int np);
// weighted k-means++ over the candidates (KMeansppSolver::cluster_weighted, kmeans++.cc:161-212) -> [K][dim].  pp_random: the
// solver's generator, drawn from once for the first centre and once per round; n_threads host threads share the candidates' distance
// updates.  each_round: when set, called with k at the start of round k (the host checks' round that throws).
std::vector<double> kmeanspp_weighted(const std::vector<double> &cand, const std::vector<double> &weight, int np, int dim, int K,
                                      int concurrency, RefRandom &pp_random, int n_threads, void (*each_round)(int) = nullptr);
// Weighted Lloyd on the candidate set (kmeans.cc:249-342).  centroids: [K][dim] in/out; up to n_threads host threads share the blocks.
void lloyd_weighted(const std::vector<double> &P, const std::vector<double> &weight, int np, int dim, int K, int concurrency,
                    int n_threads, std::vector<double> &centroids);
// The host half of a Lloyd step on the full data (kmeans.cc:213-243): the total of the block sums, best / last, the two stop rules,
// the division by the cluster size.  -> true: the loop ends (centroids untouched).
struct LloydFullState {
    std::vector<double> best_centroids;
    double best = std::numeric_limits<double>::max(), last = std::numeric_limits<double>::max();
};
bool lloyd_full_step(LloydFullState &s, int iter, const std::vector<double> &bsum, const std::vector<double> &csum,
                     const std::vector<int> &csize, int K, int dim, std::vector<double> &centroids, int verbosity);

// ---- the drivers.  Each returns its refusal, empty when there is none. ----
// KMeansIISolver::cluster (kmeansII.cc:82-171) with its defaults oversampling_factor = size_factor = 2 -> centroids [K][dim]
std::string kmeans_parallel_init(const KmBackend &be, const float *X, long n, int dim, int K, int concurrency, RandStream &rs, int verbosity,
                                 std::vector<double> &centroids);
// init_gaussians (gmm.cc:306-361).  seed < 0: the reference's stream (the library-wide restated rand()).  sigma [dim] (one vector
// shared by all mixtures) and mean [K][dim] are filled as far as the start got.
struct KmStart {
    std::vector<double> sigma, mean;
};
std::string init_like_reference(const KmBackend &be, const float *X, long n, int dim, int K, int concurrency, int init_with_kmeans, int verbosity,
                                long seed, KmStart &out);
// Labels of the library's seeded k-means (k-means|| + Lloyd on the full data, then the nearest centre of every point)
std::string kmeans_labels_on(const KmBackend &be, const float *X, long n, int dim, int K, long seed, std::vector<int> &labels);

}  // namespace sr
