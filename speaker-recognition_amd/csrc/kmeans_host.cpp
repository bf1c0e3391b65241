// kmeans_host.cpp -- the stages and drivers of the start in front of EM (kmeans_host.hpp).  Host-only.
// The full data keeps every coordinate (gmm.cc:288-294 dense2sparse; only the CANDIDATE centres of the weighted
// k-means++ / weighted Lloyd stages go through Vector2Instance, which drops |x| < 1e-15, kmeans++.cc:42-51), so
// the back end's distance is the dense one.
#include "kmeans_host.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <thread>

namespace sr {

std::vector<double> data_sigma(const float *X, long n, int dim) {
    std::vector<double> mean(dim, 0.0), var(dim, 0.0);
    for (long i = 0; i < n; i++)
        for (int d = 0; d < dim; d++) mean[d] += X[(size_t)i * dim + d];
    for (int d = 0; d < dim; d++) mean[d] /= (double)n;
    for (long i = 0; i < n; i++)
        for (int d = 0; d < dim; d++) {
            const double v = X[(size_t)i * dim + d] - mean[d];
            var[d] += v * v;
        }
    std::vector<double> sigma(dim);
    for (int d = 0; d < dim; d++) sigma[d] = std::sqrt(var[d] * (1.0 / (double)(n - 1)));
    return sigma;
}

std::vector<double> random_frames_start(const float *X, long n, int dim, int K, RefRandom &trainer_random) {
    std::vector<double> mean((size_t)K * dim, 0.0);
    for (int k = 0; k < K; k++) {                         // gmm.cc:346-349
        const long pick = trainer_random.rand_int((int)n);        // n <= INT_MAX: the drivers refuse more
        for (int d = 0; d < dim; d++) mean[(size_t)k * dim + d] = X[(size_t)pick * dim + d];
    }
    return mean;
}

double blocked_sum(const std::vector<double> &v, long n, int concurrency) {
    const long block = (long)std::ceil((double)n / concurrency);
    double total = 0;
    for (long b = 0; b < n; b += block) {
        double s = 0;
        const long e = std::min(n, b + block);
        for (long i = b; i < e; i++) s += v[i];
        total += s;
    }
    return total;
}

static void push_point(const float *X, int dim, long i, std::vector<double> &cand) {
    for (int d = 0; d < dim; d++) cand.push_back((double)X[(size_t)i * dim + d]);
}

void oversample_round(const float *X, long n, int dim, int K, double oversampling_factor, const std::vector<double> &dist,
                      double distsqr_sum, RandStream &rs, std::vector<double> &cand) {
    for (long i = 0; i < n; i++) {
        const double random_weight = rs() / (double)RAND_MAX * distsqr_sum;
        if (random_weight < dist[i] * oversampling_factor * K) push_point(X, dim, i, cand);
    }
}

void top_up_candidates(const float *X, long n, int dim, int K, double size_factor, RefRandom &solver_random, std::vector<double> &cand) {
    while ((double)(cand.size() / dim) <= size_factor * K) push_point(X, dim, solver_random.rand_int((int)n), cand);   // n <= INT_MAX (the drivers)
}

std::vector<double> candidate_weights(const std::vector<int> &belong, long n, int np) {
    std::vector<double> weight((size_t)np, 0.0);
    for (long i = 0; i < n; i++) weight[belong[i]] += 1.0;
    return weight;
}

std::vector<double> kmeanspp_weighted(const std::vector<double> &cand, const std::vector<double> &weight, int np, int dim, int K,
                                      int concurrency, RefRandom &pp_random, int n_threads, void (*each_round)(int)) {
    std::vector<double> centroids((size_t)K * dim, 0.0);
    auto copy_sparse = [&](int from, int k) {                 // Vector2Instance drops |x| < 1e-15, Instance2Vector leaves those 0
        for (int d = 0; d < dim; d++) {
            const double v = cand[(size_t)from * dim + d];
            centroids[(size_t)k * dim + d] = std::fabs(v) < 1e-15 ? 0.0 : v;
        }
    };
    copy_sparse(pp_random.rand_int() % np, 0);
    std::vector<double> pdist((size_t)np, std::numeric_limits<double>::max());
    // The candidates' distance updates are independent of one another (only the blocked sum below has an order): when the
    // candidate set is large (2 K+ candidates x K centres x dim: 0.24 s on one thread at K = 2048) a few host threads,
    // started once and stepped through the K rounds by a pair of counters, share them.
    const int pp_threads = std::max(1, n_threads);
    std::atomic<int> round_go{0}, round_done{0};
    auto upd = [&](int t, int k) {
        const double *c = centroids.data() + (size_t)(k - 1) * dim;
        const int lo = (int)((long)np * t / pp_threads), hi = (int)((long)np * (t + 1) / pp_threads);
        for (int i = lo; i < hi; i++)
            pdist[i] = std::min(pdist[i], sparse_distsqr(cand.data() + (size_t)i * dim, c, dim) * weight[i]);
    };
    // (joined on every way out: an exception between here and the end -- bad_alloc, a round that throws -- would otherwise destroy
    // joinable threads, i.e. std::terminate, with the workers spinning on a round that never comes)
    std::atomic<bool> abort_workers{false};
    struct Joiner {
        std::vector<std::thread> th;
        std::atomic<bool> &abort;
        ~Joiner() {
            abort.store(true, std::memory_order_release);
            for (auto &t : th)
                if (t.joinable()) t.join();
        }
    } workers{{}, abort_workers};
    auto &pp_workers = workers.th;
    for (int t = 1; t < pp_threads; t++)
        pp_workers.emplace_back([&, t] {
            for (int k = 1; k < K; k++) {
                while (round_go.load(std::memory_order_acquire) < k) {
                    if (abort_workers.load(std::memory_order_acquire)) return;
                    std::this_thread::yield();
                }
                upd(t, k);
                round_done.fetch_add(1, std::memory_order_release);
            }
        });
    for (int k = 1; k < K; k++) {
        if (each_round) each_round(k);
        round_go.store(k, std::memory_order_release);              // centroid k - 1 is in place
        upd(0, k);
        while (round_done.load(std::memory_order_acquire) < (pp_threads - 1) * k) std::this_thread::yield();
        const double distsqr_sum = blocked_sum(pdist, np, concurrency);
        double random_weight = pp_random.rand_int() / (double)RAND_MAX * distsqr_sum;
        for (int i = 0; i < np; i++) {
            random_weight -= pdist[i];
            if (random_weight <= 0) {
                copy_sparse(i, k);
                break;
            }
        }
    }
    for (auto &t : pp_workers) t.join();
    return centroids;
}

void lloyd_weighted(const std::vector<double> &P, const std::vector<double> &weight, int np, int dim, int K, int concurrency,
                    int n_threads, std::vector<double> &centroids) {
    std::vector<double> best_centroids;
    double best = std::numeric_limits<double>::max(), last = std::numeric_limits<double>::max();
    const int block = (int)std::ceil((double)np / concurrency);
    const int n_blocks = (np + block - 1) / block;
    n_threads = std::max(1, std::min(n_threads, n_blocks));
    std::vector<std::vector<double>> buf((size_t)n_blocks, std::vector<double>((size_t)K * dim)), csz((size_t)n_blocks, std::vector<double>((size_t)K));
    for (int iter = 0; iter < KM_MAX_ITER; iter++) {
        std::vector<double> block_sum((size_t)n_blocks, 0.0);
        auto work = [&](int b) {
            std::fill(buf[b].begin(), buf[b].end(), 0.0);
            std::fill(csz[b].begin(), csz[b].end(), 0.0);
            double s = 0;
            for (int i = b * block; i < std::min(np, (b + 1) * block); i++) {
                const double *x = P.data() + (size_t)i * dim;
                double mind = std::numeric_limits<double>::max();
                int id = -1;
                for (int j = 0; j < K; j++) {
                    const double dq = sparse_distsqr(x, centroids.data() + (size_t)j * dim, dim) * weight[i];
                    if (dq < mind) {
                        mind = dq;
                        id = j;
                    }
                }
                if (id >= 0) {
                    csz[b][id] += weight[i];
                    double *c = buf[b].data() + (size_t)id * dim;
                    for (int d = 0; d < dim; d++)
                        if (std::fabs(x[d]) >= 1e-15) c[d] += x[d] * weight[i];
                }
                s += mind;
            }
            block_sum[b] = s;
        };
        {
            auto run = [&](int t) { for (int b = t; b < n_blocks; b += n_threads) work(b); };
            std::vector<std::thread> th;
            for (int t = 1; t < n_threads; t++) th.emplace_back(run, t);
            run(0);
            for (auto &t : th) t.join();
        }
        double sum = 0;
        for (int b = 0; b < n_blocks; b++) sum += block_sum[b];
        if (sum < best) {
            best = sum;
            best_centroids = centroids;
        }
        if (std::fabs(last - sum) < 1e-6) break;
        std::vector<int> size((size_t)K, 0);                  // an int accumulator, as kmeans.cc:303-308
        for (int b = 0; b < n_blocks; b++)
            for (int k = 0; k < K; k++) size[k] += csz[b][k];
        std::fill(centroids.begin(), centroids.end(), 0.0);
        for (int b = 0; b < n_blocks; b++)
            for (size_t e = 0; e < (size_t)K * dim; e++) centroids[e] += buf[b][e];
        for (int k = 0; k < K; k++)
            for (int d = 0; d < dim; d++) centroids[(size_t)k * dim + d] /= size[k];
        last = sum;
    }
    centroids = best_centroids;
}

bool lloyd_full_step(LloydFullState &s, int iter, const std::vector<double> &bsum, const std::vector<double> &csum,
                     const std::vector<int> &csize, int K, int dim, std::vector<double> &centroids, int verbosity) {
    double sum = 0;
    for (size_t b = 0; b < bsum.size(); b++) sum += bsum[b];
    if (sum < s.best) {
        s.best = sum;
        s.best_centroids = centroids;
    }
    if (verbosity >= 2) printf("k-means iteration %3d: %f\n", iter, sum);
    if (std::fabs(s.last - sum) < 1e-6) return true;
    if (sum > s.best * 1.5) return true;                      // terminate_cost_factor
    for (int k = 0; k < K; k++)
        for (int d = 0; d < dim; d++)
            centroids[(size_t)k * dim + d] = csum[(size_t)k * dim + d] / (double)csize[k];    // an empty cluster divides by 0, as the reference
    s.last = sum;
    return false;
}

// Lloyd on the full data (kmeans.cc:150-246).  centroids: [K][dim] in/out.
static std::string lloyd_full(const KmBackend &be, long n, int dim, int K, int concurrency, std::vector<double> &centroids, int verbosity) {
    const KmLloydPlan plan = plan_lloyd_full(n, dim, K, concurrency);
    if (!plan.refusal.empty()) return plan.refusal;
    LloydFullState s;
    std::vector<double> dummy_d, bsum, csum;
    std::vector<int> dummy_i, csize;
    for (int iter = 0; iter < KM_MAX_ITER; iter++) {
        be.assign(centroids, 0, K, dummy_d, dummy_i, true, false);
        be.lloyd_sums(plan, bsum, csum, csize);
        if (lloyd_full_step(s, iter, bsum, csum, csize, K, dim, centroids, verbosity)) break;
    }
    centroids = s.best_centroids;
    return "";
}

// rand_int((int)n), n % n's int operand and the points' int labels: the start takes what an int counts
static std::string refuse_points(long n) {
    if (n <= INT_MAX) return "";
    char buf[128];
    snprintf(buf, sizeof buf, "k-means: %ld points are more than the start's 32-bit draws and labels reach (at most %d)", n, INT_MAX);
    return buf;
}

std::string kmeans_parallel_init(const KmBackend &be, const float *X, long n, int dim, int K, int concurrency, RandStream &rs, int verbosity,
                                 std::vector<double> &centroids) {
    const double oversampling_factor = 2.0, size_factor = 2.0;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_start = now();
    RefRandom solver_random(rs());                            // KMeansIISolver::random (kmeansII.hh:41)
    std::vector<double> cand;                                 // candidate centres, [count][dim]
    push_point(X, dim, (long)(rs() % n), cand);
    std::vector<double> dist((size_t)n, std::numeric_limits<double>::max());
    std::vector<int> belong((size_t)n, 0);                    // vector<int> belong(n): zero-initialised (kmeansII.cc:97)
    long last_size = 0;
    for (int iter = 0;; iter++) {
        const long size = (long)(cand.size() / dim);
        be.assign(cand, (int)last_size, (int)size, dist, belong, false, true);
        if ((double)size > size_factor * K) break;
        const double distsqr_sum = blocked_sum(dist, n, concurrency);
        last_size = size;
        oversample_round(X, n, dim, K, oversampling_factor, dist, distsqr_sum, rs, cand);
        const long added = (long)(cand.size() / dim) - last_size;
        if (verbosity >= 2) printf("k-means|| round %d: %f, new %ld, all %ld\n", iter, distsqr_sum, added, last_size + added);
        if (added == 0) break;
    }
    top_up_candidates(X, n, dim, K, size_factor, solver_random, cand);
    const int np = (int)(cand.size() / dim);
    const double t_rounds = now();
    const std::vector<double> weight = candidate_weights(belong, n, np);

    RefRandom pp_random(rs());                                // KMeansppSolver::random (kmeans++.hh:32)
    const int hw = (int)std::thread::hardware_concurrency();
    const int pp_threads = (size_t)np * dim > ((size_t)1 << 16) ? std::max(1, std::min(hw, 16)) : 1;
    centroids = kmeanspp_weighted(cand, weight, np, dim, K, concurrency, pp_random, pp_threads);
    const double t_pp = now();
    const int lw_threads = (size_t)np * K * dim > ((size_t)1 << 22) ? std::min(hw, 64) : 1;       // (and at most one a block: lloyd_weighted)
    lloyd_weighted(cand, weight, np, dim, K, concurrency, lw_threads, centroids);
    const double t_lw = now();
    const std::string why = lloyd_full(be, n, dim, K, concurrency, centroids, verbosity);
    if (!why.empty()) return why;
    if (verbosity >= 2)
        printf("k-means|| phases: oversampling rounds %.3f s (%d candidates), weighted k-means++ %.3f s, weighted Lloyd %.3f s, "
               "Lloyd on the full data %.3f s\n", t_rounds - t_start, np, t_pp - t_rounds, t_lw - t_pp, now() - t_lw);
    return "";
}

std::string init_like_reference(const KmBackend &be, const float *X, long n, int dim, int K, int concurrency, int init_with_kmeans, int verbosity,
                                long seed, KmStart &out) {
    const std::string many = refuse_points(n);
    if (!many.empty()) return many;
    RandStream rs(seed);
    RefRandom trainer_random(rs());                           // GMMTrainerBaseline::random, seeded when the trainer is built (pygmm.cc:65)
    for (int k = 0; k < K; k++) (void)rs();                   // every `new Gaussian` seeds a Random of its own (gmm.hh:44, gmm.cc:327-329)
    out.sigma = data_sigma(X, n, dim);
    for (double s : out.sigma)
        if (!(s > 0)) return "training data has zero variance in some dimension";
    out.mean.assign((size_t)K * dim, 0.0);
    if (init_with_kmeans > 0) {
        std::vector<double> c;
        const std::string why = kmeans_parallel_init(be, X, n, dim, K, concurrency, rs, verbosity, c);
        if (!why.empty()) return why;
        out.mean = c;
        for (double v : out.mean)
            if (!std::isfinite(v)) return "k-means initialisation left an empty cluster (the reference divides by zero here as well)";
    } else {
        out.mean = random_frames_start(X, n, dim, K, trainer_random);
    }
    return "";
}

std::string kmeans_labels_on(const KmBackend &be, const float *X, long n, int dim, int K, long seed, std::vector<int> &labels) {
    const std::string many = refuse_points(n);
    if (!many.empty()) return many;
    RandStream rs(seed);
    std::vector<double> c;
    const std::string why = kmeans_parallel_init(be, X, n, dim, K, 1, rs, 0, c);
    if (!why.empty()) return why;
    std::vector<double> dist((size_t)n);
    labels.assign((size_t)n, 0);
    be.assign(c, 0, K, dist, labels, true, true);
    return "";
}

}  // namespace sr
