// em_mstep.cpp -- the host's float64 half of an EM / MAP iteration (em_mstep.hpp).  The statements stand in the order they had
// inside train_em: fits are compared bit for bit across this file's history (tests/test_gpu_em_parent_bits.py).
#include "em_mstep.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <future>
#include <system_error>
#include <thread>

namespace sr {

void recentre_origin_sums(double *stats, int DP, const EmModelRef &g) {
    const int K = g.K, dim = g.dim, REC = 2 * DP + 1;
    // T1 = sum g x, T2 = sum g x^2, N = sum g  ->  the centred sums the M-step works on, about the fp32 mean
    // the vector form centres on: sum g (x - m) = T1 - N m, sum g (x - m)^2 = T2 - 2 m T1 + N m^2 (float64)
    for (int k = 0; k < K; k++) {
        double *st = stats + (size_t)k * REC;
        const double N = st[2 * DP];
        for (int d = 0; d < dim; d++) {
            const double m = (double)(float)g.mean[(size_t)k * dim + d];
            const double t1 = st[d], t2 = st[DP + d];
            st[d] = t1 - N * m;
            st[DP + d] = t2 - 2.0 * m * t1 + N * m * m;
        }
    }
}

std::vector<int> weak_mixtures(const double *stats, int DP, int K) {
    const int REC = 2 * DP + 1;
    std::vector<int> weak;
    for (int k = 0; k < K; k++)
        if (stats[(size_t)k * REC + 2 * DP] < 1e-25) weak.push_back(k);
    return weak;
}

void redo_weak_mixture(double *stats, int DP, const EmModelRef &g, int k, const float *X, long n, const float *ll_p) {
    const int dim = g.dim, REC = 2 * DP + 1;
    const double SQRT_2_PI = 2.5066282746310002, MINLOG = -708.396418532264;
    double *st = stats + (size_t)k * REC;
    for (int e = 0; e < REC; e++) st[e] = 0.0;
    const double *mu = g.mean + (size_t)k * dim, *sg = g.sigma + (size_t)k * dim;
    double c = g.weights[k] > 0 ? std::log(g.weights[k]) : -INFINITY;
    for (int d = 0; d < dim; d++) c -= std::log(SQRT_2_PI * sg[d]);
    for (long i = 0; i < n; i++) {
        if (!(ll_p[i] >= (float)MINLOG)) continue;
        const float *x = X + (size_t)i * dim;
        double lp = c;
        for (int d = 0; d < dim; d++) {
            const double v = ((double)x[d] - mu[d]) / sg[d];
            lp -= 0.5 * v * v;
        }
        if (!(lp >= MINLOG)) continue;
        const double gam = std::exp(lp - (double)ll_p[i]);
        for (int d = 0; d < dim; d++) {
            const double dv = (double)x[d] - (double)(float)mu[d];       // centred on the fp32 mean the device used
            st[d] += gam * dv;
            st[DP + d] += gam * dv * dv;
        }
        st[2 * DP] += gam;
    }
}

void redo_weak_mixtures(double *stats, int DP, const EmModelRef &g, const std::vector<int> &weak, const float *X, long n, const float *ll,
                        int max_threads) {
    auto redo = [&](int k) { redo_weak_mixture(stats, DP, g, k, X, n, ll); };
    // A large UBM adapted on a short utterance leaves MANY mixtures without support (2048 mixtures, 3000 frames: this
    // loop was 4.6 of an iteration's 6.5 ms -- one division per (mixture, frame, dimension) on one core).  The mixtures
    // are independent -- each writes its own row of sums -- so they are dealt to a few host threads: same operations
    // in the same order per mixture, same bits for any number of threads.
    const size_t work = weak.size() * (size_t)n * (size_t)g.dim;
    const int n_thr = work < ((size_t)1 << 20) ? 1 : (int)std::max<size_t>(1, std::min<size_t>({weak.size(), (size_t)std::thread::hardware_concurrency(), (size_t)max_threads}));
    if (n_thr <= 1) {
        for (int k : weak) redo(k);
        return;
    }
    std::atomic<size_t> next{0};
    auto worker = [&]() {
        for (size_t j; (j = next.fetch_add(1)) < weak.size();) redo(weak[j]);
    };
    std::vector<std::future<void>> helpers;
    for (int t = 1; t < n_thr; t++) {
        try {
            helpers.push_back(std::async(std::launch::async, worker));
        } catch (const std::system_error &) {      // (no thread to be had: the others take its share)
            break;
        }
    }
    worker();
    for (auto &h : helpers) h.get();
}

void em_mstep(const double *stats, int DP, const EmModelRef &g, long n, const double *ubm_mean, double relevance, double min_sigma) {
    const int K = g.K, dim = g.dim, REC = 2 * DP + 1;
    std::vector<double> Nk(K);
    for (int k = 0; k < K; k++) {
        double v = stats[(size_t)k * REC + 2 * DP];
        if (v == 0) v = 1e-6;                            // min_n_k, gmm.cc:502-509
        Nk[k] = v;
    }
    if (!ubm_mean) {                                     // update_weights, gmm.cc:388-394
        double wsum = 0;
        for (int k = 0; k < K; k++) {
            g.weights[k] = Nk[k] / (double)n;
            wsum += g.weights[k];
        }
        for (int k = 0; k < K; k++) g.weights[k] /= wsum;
    }
    for (int k = 0; k < K; k++) {
        for (int d = 0; d < dim; d++) {
            const double sd = stats[(size_t)k * REC + d];
            const double sdd = stats[(size_t)k * REC + DP + d];
            const double mu_old = g.mean[(size_t)k * dim + d];
            const double shift = sd / Nk[k];             // E_k[x] - mu_old
            // no responsibility at all (raw N_k 0, the sums above exact zeros): the reference's E_k[x] = sum g x / 1e-6
            // is 0, not the old mean (gmm.cc:396-412)
            const double ex = stats[(size_t)k * REC + 2 * DP] == 0 ? 0.0 : mu_old + shift;
            if (ubm_mean) {                              // update_means, gmmubm.cc:53-74
                const double alpha = Nk[k] / (Nk[k] + relevance);
                g.mean[(size_t)k * dim + d] = alpha * ex + (1 - alpha) * ubm_mean[(size_t)k * dim + d];
            } else {                                     // gmm.cc:396-412, :415-437
                g.mean[(size_t)k * dim + d] = ex;
                // sum g (x - mu_new)^2 = sdd - 2 shift sd + shift^2 N = sdd - N shift^2
                double var = sdd / Nk[k] - shift * shift;
                if (var < 0) var = 0;
                g.sigma[(size_t)k * dim + d] = std::max(min_sigma, std::sqrt(var));
            }
        }
    }
}

bool em_converged(double ll, double last_ll, double threshold) {
    const double ll_diff = ll - last_ll;
    return std::fabs(ll_diff) / std::fabs(ll) < threshold && ll_diff < threshold;
}

}  // namespace sr
