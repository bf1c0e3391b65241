// em_checks.cpp -- what train_em (csrc/em.hip) decides and computes on the host, under the host sanitizers: a stand-alone program,
// built by tests/test_em_host.py with g++ -fsanitize=address,undefined from csrc/em_plan.cpp, csrc/em_mstep.cpp and csrc/map_plan.cpp.
//   * plan_em_stats swept over mixture counts, every built padded dim and some that are not, frame counts around the tile sizes,
//     device sizes, the four option values and both answers of the split-bf16 range test: the grid covers every record and tile
//     and is inside the launch limits, the slabs are what the chosen kernel indexes, its LDS fits, the engine is the one the
//     formulas that stood in train_em choose, and never one that em_shapes.hpp does not list;
//   * em_route against the restatement of tests/test_map_batch_cpu.py, the else-if included;
//   * the float64 M-step: re-centring about a zero mean is the identity, the redo of unsupported mixtures has the same bits on
//     1, 2 and 16 threads, MAP leaves weights and sigmas alone, an empty mixture goes to 0 / sqrt(min_covar) (EM) or the
//     alpha-weighted UBM mean (MAP), weights sum to 1, the stop rule is the two-clause one;
//   * one full host iteration (K = 3, D = 2, n = 50): exact responsibilities -> sums centred on the fp32 means -> em_mstep, against
//     sum g x / sum g and sum g (x - mu_new)^2 / N formed directly.  Both sides float64 and algebraically equal; MEASURED worst
//     relative difference over weights, means and sigmas: 5.8e-16 (x86-64, g++ -O1).  Gate: 4 x that, for reordering.
// `em_checks --table` prints the built instantiations of em_shapes.hpp, for the comparison with what em.hip compiled to.
#include "em_mstep.hpp"
#include "em_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace sr;

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            if (failures < 20) std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                             \
        }                                                                           \
    } while (0)

static const double FULL_ITERATION_GATE = 4 * 5.8e-16;

static Parameter params(int nit = 200, int verbosity = 0) {
    Parameter p = {};
    p.nr_iteration = nit;
    p.verbosity = verbosity;
    p.threshold = 0.01;
    p.min_covar = 1e-3;
    return p;
}

static uint64_t rng_state = 12345;
static double uniform() {          // [0, 1), 24 bits
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 40) / (double)(1 << 24);
}
static double gauss() { return (uniform() + uniform() + uniform() + uniform() - 2.0) * std::sqrt(3.0); }

// ---- the plan ----
static int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

static void check_plan(int K, int dim, int DP, long n, int n_cu, int option, bool in_range) {
    const int ks = ems_steps(dim), n_mix_tiles = ceil_div(K, 32);
    const EmStatsPlan p = plan_em_stats(K, dim, DP, n, option, in_range, ks, n_mix_tiles, n_cu);
    // the engine by the formulas that stood in train_em: DP <= 40; the (DP, KS) rule of stats_split_available(DP, dim)
    const bool built = stats_vector_available(DP) || DP > EM_MAX_REG_DIM;
    const bool use_mfma = built && DP <= 40 && option != 1;
    const bool use_split = use_mfma && (option == 0 || option == 3) && in_range && 8 * ks >= DP && ems_lds_bytes(ks) <= 160 * 1024;
    CHECK(p.engine == (!built ? 0 : use_split ? 3 : use_mfma ? 2 : 1));
    CHECK(p.dp == DP && p.n_records == ceil_div(K, 4) && p.k_pad == 4 * p.n_records && p.rec == 2 * DP + 1 && p.n_elem == (size_t)p.k_pad * p.rec);
    CHECK(p.wide == (DP > 96));
    if (p.engine == 0) return;
    CHECK(p.grid_x >= 1 && p.grid_y >= 1 && p.grid_y <= 65535 && p.block >= 64 && p.block <= 1024 && p.block % 64 == 0);
    CHECK((int64_t)p.grid_x * p.grid_y < ((int64_t)1 << 32) && p.reduce_grid >= 1);
    CHECK((size_t)p.reduce_grid * 256 >= p.n_elem && (size_t)(p.reduce_grid - 1) * 256 < p.n_elem);
    CHECK(p.lds_bytes <= (size_t)EM_LDS_BOUND);
    if (p.engine == 1) {
        CHECK(p.wide || stats_vector_available(DP));
        CHECK(!p.slab_f64 && p.block == 256 && p.lds_bytes == 0);
        CHECK(p.n_tiles == ceil_div(n, 256) && (int64_t)p.n_tiles * 256 >= n && (int64_t)(p.n_tiles - 1) * 256 < n);
        CHECK(p.grid_x <= p.n_tiles && p.grid_x <= n_cu * (p.wide ? 1 : 4));          // a grid-stride loop over the tiles: none dropped
        // the kernels' cut of the records along y
        int rec_per = ceil_div(p.n_records, p.grid_y);
        if (p.wide) rec_per = ceil_div(rec_per, EM_CB) * EM_CB;
        CHECK((int64_t)rec_per * p.grid_y >= p.n_records);
        CHECK(p.grid_y <= p.n_records && p.grid_y <= std::max(1, ceil_div(4 * n_cu, p.grid_x)));
        CHECK(p.slab_elems == (size_t)p.grid_x * p.n_elem);
        return;
    }
    CHECK(stats_mfma_available(DP) && p.slab_f64);
    CHECK(p.n_tiles == ceil_div(n, EMM_FT) && (int64_t)p.n_tiles * EMM_FT >= n && (int64_t)(p.n_tiles - 1) * EMM_FT < n);
    const int tiles_per = ceil_div(p.n_tiles, p.grid_y);                              // the kernels' cut of the tiles along y
    CHECK((int64_t)tiles_per * p.grid_y >= p.n_tiles && p.grid_y <= p.n_tiles);
    CHECK(p.slab_elems == (size_t)p.grid_y * p.grid_x * p.wg_mix * emm_ncb(DP) * 16);
    CHECK((int64_t)p.grid_x * p.wg_mix >= p.k_pad);                                   // the reduce finds every mixture's range
    CHECK(emm_ncb(DP) * 16 >= 2 * DP + 1 && (emm_ncb(DP) - 1) * 16 < 2 * DP + 1);
    if (p.engine == 2) {
        CHECK(p.wg_mix == EMM_WG_MIX && p.block == EMM_WAVES * 64 && p.lds_bytes == emm_lds_bytes(DP));
        CHECK(p.grid_x * (EMM_WG_MIX / EM_KB) >= p.n_records && (p.grid_x - 1) * (EMM_WG_MIX / EM_KB) < p.n_records);
    } else {
        CHECK(stats_split_available(DP, p.ks) && p.ks == ks && 8 * p.ks >= DP);
        CHECK(p.wg_mix == EMS_WG_MIX && p.block == EMS_WAVES * 64 && p.lds_bytes == (size_t)ems_lds_bytes(p.ks));
        CHECK(p.grid_x * EMS_TILES >= n_mix_tiles && (p.grid_x - 1) * EMS_TILES < n_mix_tiles);
    }
}

static void sweep_plans() {
    // (dim, padded dim): every built one at its own width and one below, a width nothing is built for, the wide rows
    static const int shapes[][2] = {{7, 8}, {8, 8}, {12, 13}, {13, 13}, {15, 16}, {16, 16}, {23, 24}, {24, 24}, {25, 26}, {26, 26}, {31, 32},
                                    {32, 32}, {33, 34}, {34, 34}, {38, 39}, {39, 39}, {40, 40}, {48, 48}, {56, 56}, {64, 64}, {80, 80},
                                    {96, 96}, {20, 20}, {44, 44}, {97, 128}, {200, 256}};
    static const long ns[] = {1, 2, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 1000, 3000, 100000, 4000000};
    std::vector<int> Ks;
    for (int K = 1; K <= 140; K++) Ks.push_back(K);
    for (int K = 141; K <= 2100; K += 37) Ks.push_back(K);
    Ks.push_back(2048);
    Ks.push_back(2100);
    long count = 0;
    for (int K : Ks)
        for (const auto &s : shapes)
            for (long n : ns)
                for (int n_cu : {1, 8, 256, 304})
                    for (int option = 0; option <= 3; option++)
                        for (int in_range = 0; in_range <= 1; in_range++, count++) check_plan(K, s[0], s[1], n, n_cu, option, in_range != 0);
    // a forced matrix-core option that is not available falls back to the vector engine
    for (int option : {2, 3}) {
        CHECK(plan_em_stats(64, 48, 48, 1000, option, true, ems_steps(48), 2, 256).engine == 1);
        CHECK(plan_em_stats(64, 97, 128, 1000, option, true, 0, 0, 256).engine == 1);
    }
    CHECK(plan_em_stats(64, 40, 40, 1000, 3, true, ems_steps(40), 2, 256).engine == 2);     // six steps: 164 KB of LDS
    CHECK(plan_em_stats(64, 39, 39, 1000, 3, true, ems_steps(39), 2, 256).engine == 3);
    CHECK(plan_em_stats(64, 39, 39, 1000, 3, true, ems_steps(39), 0, 256).engine == 2);     // a set without the split layout
    CHECK(plan_em_stats(64, 39, 39, 1000, 2, true, ems_steps(39), 2, 256).engine == 2);
    std::printf("plans checked: %ld\n", count);
}

// ---- the route: tests/test_map_batch_cpu.py's restatement ----
static int small_grid(int K, int D, long n) {
    const int R = K * (D + 1);
    for (int fr : {128, 64}) {
        if (fr > 64 && (n + fr / 2 - 1) / (fr / 2) == (n + fr - 1) / fr) continue;
        int seg = 1;
        while (seg * 2 <= fr / 64 && R * seg * 2 <= 1024) seg *= 2;
        const long lds = (long)(3 * K + 3 * K * D + K * fr + 1024 + fr + K * (2 * D + 1) + 2 + 2 * R * seg) * 8 + (long)fr * (D + 1) * 4;
        if (lds > 150 * 1024) continue;
        return (int)((n + fr - 1) / fr);
    }
    return 0;
}

static void check_routes() {
    for (int K : {1, 16, 32, 33, 64, 65, 2048})
        for (int D : {1, 13, 40, 41, 64, 65})
            for (long n : {1L, 64L, 128L, 129L, 3000L, 8192L, 8193L})
                for (int n_cu : {256, 8})
                    for (int nit : {0, 200})
                        for (int verbosity : {0, 2})
                            for (int option = 0; option <= 3; option++)
                                for (int side = 0; side <= 1; side++) {
                                    const bool small = K >= 1 && K <= 32 && D >= 1 && D <= 40 && n >= 1 && n <= 8192 && small_grid(K, D, n) >= 1 &&
                                                       small_grid(K, D, n) <= n_cu / 2 && nit >= 1 && verbosity < 2;
                                    const bool f64 = K >= 1 && D >= 1 && D <= 64 && n >= 1 && n <= 8192 && nit >= 1 && verbosity < 2 &&
                                                     (long)((K + 63) / 64 * 64) * ((n + 127) / 128 * 128) <= (32L << 20);
                                    const bool automatic = option == 0 && !side;
                                    // else-if: a fit the whole-fit kernel is eligible for never goes to the float64 engine
                                    const int want = automatic && small ? EM_ROUTE_WHOLE_FIT : automatic && f64 ? EM_ROUTE_F64 : EM_ROUTE_ITERATION;
                                    CHECK(em_route(K, D, n, params(nit, verbosity), option, side != 0, n_cu) == want);
                                }
    CHECK(em_route(16, 13, 3000, params(), 0, false, 256) == EM_ROUTE_WHOLE_FIT);       // eligible for both: the whole-fit kernel's
    CHECK(em_f64_shape_eligible(16, 13, 3000, params()));
    CHECK(em_route(512, 39, 3000, params(), 0, false, 256) == EM_ROUTE_F64);
    CHECK(em_route(512, 39, 3000, params(), 3, false, 256) == EM_ROUTE_ITERATION);
    CHECK(em_route(512, 39, 3000, params(), 0, true, 256) == EM_ROUTE_ITERATION);
}

// ---- the M-step ----
struct Model {
    int K, dim;
    std::vector<double> w, mu, sg;
    Model(int K_, int dim_) : K(K_), dim(dim_), w(K_, 1.0 / K_), mu((size_t)K_ * dim_), sg((size_t)K_ * dim_, 0.9) {
        for (double &v : mu) v = 2.0 * gauss();
    }
    EmModelRef ref() { return EmModelRef{K, dim, w.data(), mu.data(), sg.data()}; }
};
static bool same_bits(const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

static void check_recentre() {
    const int K = 5, dim = 13, DP = 16, REC = 2 * DP + 1;
    Model m(K, dim);
    std::fill(m.mu.begin(), m.mu.end(), 0.0);
    std::vector<double> st((size_t)K * REC);
    for (double &v : st) v = 100.0 * gauss();
    const std::vector<double> before = st;
    recentre_origin_sums(st.data(), DP, m.ref());
    CHECK(same_bits(st, before));
}

static void check_weak_threads() {
    // (work = weak mixtures x frames x dims: above and below the 2^20 where the driver takes threads)
    for (long n : {3000L, 40L}) {
        const int K = 48, dim = 13, DP = 13, REC = 2 * DP + 1;
        Model m(K, dim);
        std::vector<float> X((size_t)n * dim), ll((size_t)n);
        for (float &v : X) v = (float)(2.0 * gauss());
        for (long i = 0; i < n; i++) ll[(size_t)i] = i % 17 == 3 ? -800.0f : (float)(-20.0 + gauss());     // some frames underflowed
        std::vector<double> st((size_t)K * REC);
        for (double &v : st) v = gauss();
        for (int k = 0; k < K; k++) st[(size_t)k * REC + 2 * DP] = k % 4 == 1 ? 1.0 + uniform() : k % 4 == 2 ? 0.0 : 1e-30 * uniform();
        const std::vector<int> weak = weak_mixtures(st.data(), DP, K);
        CHECK((int)weak.size() == K - K / 4);
        CHECK(((size_t)weak.size() * n * dim >= ((size_t)1 << 20)) == (n == 3000));
        std::vector<double> got[3];
        const int threads[3] = {1, 2, 16};
        for (int t = 0; t < 3; t++) {
            got[t] = st;
            redo_weak_mixtures(got[t].data(), DP, m.ref(), weak, X.data(), n, ll.data(), threads[t]);
        }
        CHECK(same_bits(got[0], got[1]) && same_bits(got[0], got[2]));
        // one by one: the same rows; the supported mixtures' rows untouched
        std::vector<double> one = st;
        for (int k : weak) redo_weak_mixture(one.data(), DP, m.ref(), k, X.data(), n, ll.data());
        CHECK(same_bits(one, got[0]));
        for (int k = 1; k < K; k += 4) CHECK(std::memcmp(&one[(size_t)k * REC], &st[(size_t)k * REC], REC * sizeof(double)) == 0);
        double total = 0;
        for (int k : weak) total += one[(size_t)k * REC + 2 * DP];
        CHECK(total > 0 && std::isfinite(total));
    }
}

static void check_mstep_rules() {
    const int K = 7, dim = 5, DP = 8, REC = 2 * DP + 1;
    const long n = 400;
    const double min_covar = 1e-3, min_sigma = std::sqrt(min_covar), relevance = 16.0;
    std::vector<double> st((size_t)K * REC, 0.0);
    for (int k = 0; k < K; k++) {
        if (k == 2) continue;                            // an exactly empty mixture: every sum an exact 0
        const double N = 20.0 + 50.0 * uniform();
        st[(size_t)k * REC + 2 * DP] = N;
        for (int d = 0; d < dim; d++) {
            st[(size_t)k * REC + d] = N * 0.1 * gauss();
            st[(size_t)k * REC + DP + d] = N * (0.5 + uniform());
        }
    }
    {   // EM
        Model m(K, dim);
        em_mstep(st.data(), DP, m.ref(), n, nullptr, relevance, min_sigma);
        for (int d = 0; d < dim; d++) CHECK(m.mu[2 * dim + d] == 0.0 && m.sg[2 * dim + d] == min_sigma);
        double sum = 0;
        for (int k = 0; k < K; k++) sum += m.w[(size_t)k];
        CHECK(std::fabs(sum - 1.0) <= K * 1.1102230246251565e-16);       // the last bit of a K-term float64 sum
        CHECK(m.w[2] > 0 && m.w[2] < 1e-6);
        for (double v : m.sg) CHECK(v >= min_sigma);
    }
    {   // MAP
        Model m(K, dim), ubm(K, dim);
        const std::vector<double> w0 = m.w, sg0 = m.sg, mu0 = m.mu;
        em_mstep(st.data(), DP, m.ref(), n, ubm.mu.data(), relevance, min_sigma);
        CHECK(same_bits(m.w, w0) && same_bits(m.sg, sg0) && !same_bits(m.mu, mu0));
        const double alpha = 1e-6 / (1e-6 + relevance);
        for (int d = 0; d < dim; d++) CHECK(m.mu[2 * dim + d] == alpha * 0.0 + (1 - alpha) * ubm.mu[2 * dim + d]);
    }
}

static void check_converged() {
    const double big = -1.7976931348623157e308;
    for (double thr : {0.01, 1e-5, 0.0, 1e6})
        for (double ll : {-5000.0, -1.0, 3.0})
            for (double last : {big, ll - 100.0, ll - 1e-3, ll, ll + 1e-3, ll + 100.0}) {
                const double diff = ll - last;
                CHECK(em_converged(ll, last, thr) == (std::fabs(diff) / std::fabs(ll) < thr && diff < thr));
            }
    CHECK(!em_converged(-5000.0, big, 0.01));                 // the first check of a fit
    CHECK(em_converged(-5000.0, -5000.0, 0.01));              // equal totals stop it
    CHECK(!em_converged(-5000.0, -5000.0, 0.0));
    CHECK(em_converged(-5000.0, -4000.0, 0.5) && !em_converged(-4000.0, -5000.0, 0.5));     // the second clause is signed
}

static double full_iteration() {
    const int K = 3, dim = 2, DP = 8, REC = 2 * DP + 1;
    const long n = 50;
    const double min_sigma = std::sqrt(1e-3);
    Model m(K, dim);
    m.w = {0.5, 0.3, 0.2};
    // (means that fp32 holds: the sums are centred on the fp32 mean and em_mstep adds the shift to the float64 one -- equal only then)
    for (double &v : m.mu) v = (double)(float)v;
    std::vector<float> X((size_t)n * dim);
    for (long i = 0; i < n; i++)
        for (int d = 0; d < dim; d++) X[(size_t)i * dim + d] = (float)(m.mu[(size_t)(i % K) * dim + d] + 0.8 * gauss());
    // exact responsibilities
    std::vector<double> g((size_t)n * K);
    for (long i = 0; i < n; i++) {
        double lp[K], mx = -INFINITY, s = 0;
        for (int k = 0; k < K; k++) {
            lp[k] = std::log(m.w[(size_t)k]);
            for (int d = 0; d < dim; d++) {
                const double v = ((double)X[(size_t)i * dim + d] - m.mu[(size_t)k * dim + d]) / m.sg[(size_t)k * dim + d];
                lp[k] -= 0.5 * v * v + std::log(2.5066282746310002 * m.sg[(size_t)k * dim + d]);
            }
            mx = std::max(mx, lp[k]);
        }
        for (int k = 0; k < K; k++) s += std::exp(lp[k] - mx);
        for (int k = 0; k < K; k++) g[(size_t)i * K + k] = std::exp(lp[k] - mx) / s;
    }
    // the device's sums: centred on the fp32 mean
    std::vector<double> st((size_t)K * REC, 0.0);
    for (int k = 0; k < K; k++)
        for (long i = 0; i < n; i++) {
            const double gam = g[(size_t)i * K + k];
            for (int d = 0; d < dim; d++) {
                const double dv = (double)X[(size_t)i * dim + d] - (double)(float)m.mu[(size_t)k * dim + d];
                st[(size_t)k * REC + d] += gam * dv;
                st[(size_t)k * REC + DP + d] += gam * dv * dv;
            }
            st[(size_t)k * REC + 2 * DP] += gam;
        }
    em_mstep(st.data(), DP, m.ref(), n, nullptr, 16.0, min_sigma);
    // directly
    double worst = 0;
    for (int k = 0; k < K; k++) {
        double N = 0;
        for (long i = 0; i < n; i++) N += g[(size_t)i * K + k];
        worst = std::max(worst, std::fabs(m.w[(size_t)k] - N / (double)n) / (N / (double)n));
        for (int d = 0; d < dim; d++) {
            double sx = 0, sxx = 0;
            for (long i = 0; i < n; i++) sx += g[(size_t)i * K + k] * (double)X[(size_t)i * dim + d];
            const double mu = sx / N;
            for (long i = 0; i < n; i++) {
                const double dv = (double)X[(size_t)i * dim + d] - mu;
                sxx += g[(size_t)i * K + k] * dv * dv;
            }
            const double sg = std::max(min_sigma, std::sqrt(sxx / N));
            worst = std::max(worst, std::fabs(m.mu[(size_t)k * dim + d] - mu) / std::max(1.0, std::fabs(mu)));
            worst = std::max(worst, std::fabs(m.sg[(size_t)k * dim + d] - sg) / sg);
            CHECK(sg > min_sigma);
        }
    }
    return worst;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--table") == 0) {
#define PRINT1(V) std::printf(" %d", V);
#define PRINT2(V, W) std::printf(" %d,%d", V, W);
        std::printf("vector:");
        SR_EM_VECTOR_DPS(PRINT1)
        std::printf("\nmfma:");
        SR_EM_MFMA_DPS(PRINT1)
        std::printf("\nsplit:");
        SR_EM_SPLIT_SHAPES(PRINT2)
        std::printf("\n");
        return 0;
    }
    sweep_plans();
    check_routes();
    check_recentre();
    check_weak_threads();
    check_mstep_rules();
    check_converged();
    const double worst = full_iteration();
    std::printf("full host iteration: worst relative difference %.3g (gate %.3g)\n", worst, FULL_ITERATION_GATE);
    CHECK(worst <= FULL_ITERATION_GATE);
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("em checks ok\n");
    return 0;
}
