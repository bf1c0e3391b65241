// kmeans_checks.cpp -- the host half of the start in front of EM (csrc/ref_rand.cpp, csrc/kmeans_plan.cpp, csrc/kmeans_host.cpp) without
// a GPU: a stand-alone program, built by tests/test_kmeans_host_cpu.py with g++ -fsanitize=address,undefined and a second time with
// -fsanitize=thread.
//   kmeans_checks plans                     the two plans swept, every refusal; the restated rand() against the C library's
//   kmeans_checks driver MANIFEST OUTDIR    the drivers of kmeans_host.cpp on a host back end (a plain loop, below), a fit per line
//                                           of MANIFEST (name n K D concurrency seed init_with_kmeans file-of-float32-rows): the means
//                                           (or the refusal) go to OUTDIR/name.means (.error)
//   kmeans_checks threads                   the weighted k-means++ and the weighted Lloyd on 1 and on 16 threads: the same bits;
//                                           an exception in round 3: the workers are joined
//
// What the plans must guarantee, read from the kernels' bodies (csrc/kmeans_init.hip):
//   kmeans_assign_kernel / kmeans_assign_fast_kernel
//       idx[p] = ((long)blockIdx.x * KM_PP + p) * 256 + threadIdx.x;  valid[p] = idx[p] < n_work;
//     a workgroup takes KM_PP * 256 consecutive points: grid * KM_PP * 256 >= n.
//       list[at] = (int)idx[p];            (fast)   at = atomicAdd(n_list, 1): at most every point once: list holds n, n < 2^31
//       const double *src = rec + (size_t)chunk * REC;   chunk < n_chunks = (K + KM_CH - 1) / KM_CH,  REC = km_rec_doubles(DIM_MAX)
//   kmeans_centre_prep_kernel
//       const int j = blockIdx.x * 256 + threadIdx.x;  if (j >= k_pad) return;  k_pad = (K + KM_CH - 1) / KM_CH * KM_CH
//       double *r = rec + (size_t)(j / KM_CH) * km_rec_doubles(dim_max);      every j < k_pad must be covered: prep_grid * 256 >= k_pad
//   lloyd_keys_kernel
//       key[i] = j >= 0 ? (unsigned)(i / block) * (unsigned)K + (unsigned)j : n_keys;   idx[i] = (unsigned)i;
//     (i / block) < n_blocks for every i < n, so every key <= n_keys; the sort looks at bits [0, end_bit): n_keys < 2^end_bit
//   lloyd_segments_kernel
//       const unsigned k = blockIdx.x * 256 + threadIdx.x;  if (k > n_keys) return;  seg[k] = (unsigned)lo;      seg[0 .. n_keys]
//   lloyd_segment_sum_kernel
//       const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;  if (e >= n_seg_elems) return;  lo = seg[k], hi = seg[k + 1];  buf[e] = s;
//   lloyd_centroid_kernel
//       const int e = blockIdx.x * 256 + threadIdx.x;  if (e >= K * dim) return;      both in an int
//       buf[(size_t)b * K * dim + e]      b < n_blocks: segsum holds n_blocks * K * dim = n_keys * dim
//   lloyd_block_sum_kernel
//       const int b = blockIdx.x;  lo = (long)b * block, hi = min(n, lo + block);  bsum[b] = s;                  a workgroup per block
#include "kmeans_host.hpp"

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>

using namespace sr;

static int failures = 0;
static long plans = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                             \
        }                                                                           \
    } while (0)

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

// splitmix64 of (seed, index), as tests/em_parent_cases.py's _uniform
static uint64_t hash64(uint64_t seed, uint64_t i) {
    uint64_t z = (i + 1) * 0x9E3779B97F4A7C15ull + seed * 0xD1342543DE82EF95ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double uniform(uint64_t seed, uint64_t i) { return (double)(hash64(seed, i) >> 40) / (double)(1 << 24); }

// ---- (a) the plans ----
static void check_assign(long n, int dim, int c_begin, int c_end, bool reset, int engine) {
    const KmAssignPlan p = plan_kmeans_assign(n, dim, c_begin, c_end, reset, engine);
    plans++;
    if (n >= ((long)1 << 32)) { CHECK(has(p.refusal, "nearest-centre grid")); return; }      // 256 threads x the grid: counted in 32 bits
    CHECK(p.refusal.empty());
    if (!p.refusal.empty()) return;
    CHECK((unsigned long long)p.grid * 256 < (1ull << 32));
    CHECK(p.fast == (reset && c_begin == 0 && dim <= 40 && engine == 0 && n < ((long)1 << 31)));      // the parent's condition, verbatim
    CHECK(p.exact_dim_max == (dim <= 16 ? 16 : dim <= 40 ? 40 : dim <= 64 ? 64 : 128));
    CHECK((long)p.grid * KM_PP * 256 >= n && ((long)p.grid - 1) * KM_PP * 256 < n);
    CHECK(p.C == (size_t)c_end * dim && p.dist == (size_t)n && p.belong == (size_t)n);
    if (!p.fast) {
        CHECK(p.fast_dim_max == 0 && p.n_chunks == 0 && p.prep_grid == 0 && p.m2c + p.cn_max + p.list + p.n_list == 0);
        return;
    }
    CHECK(p.fast_dim_max == (dim <= 16 ? 16 : 40) && dim <= p.fast_dim_max);
    const int k_pad = (c_end + KM_CH - 1) / KM_CH * KM_CH;
    CHECK(p.n_chunks * KM_CH == k_pad && (long)p.prep_grid * 256 >= k_pad && ((long)p.prep_grid - 1) * 256 < std::max(k_pad, 1));
    CHECK(p.m2c == (size_t)p.n_chunks * km_rec_doubles(p.fast_dim_max));
    CHECK(km_rec_doubles(p.fast_dim_max) % 128 == 0 && km_rec_doubles(p.fast_dim_max) >= p.fast_dim_max * KM_CH + KM_CH);     // whole KiB; [d][16] and the 16 norms
    CHECK(p.list == (size_t)n && p.n_list == 1 && p.cn_max == 1);
}

static void check_lloyd(long n, int dim, int K, int concurrency) {
    const KmLloydPlan p = plan_lloyd_full(n, dim, K, concurrency);
    plans++;
    const long block = (long)std::ceil((double)n / concurrency);               // the parent's expression
    const long n_blocks = (n + block - 1) / block;
    const bool keys_refused = (double)n_blocks * K >= 4.0e9 || n >= ((long)1 << 32);
    const bool kd_refused = (long)K * dim > (long)INT_MAX - 256;
    const bool seg_refused = !keys_refused && !kd_refused && (unsigned long long)n_blocks * K * dim > (1ull << 32) - 256;
    if (keys_refused) { CHECK(has(p.refusal, "do not fit 32-bit sort keys")); return; }
    if (kd_refused) { CHECK(has(p.refusal, "centroid kernel")); return; }
    if (seg_refused) { CHECK(has(p.refusal, "segment-sum grid")); return; }
    CHECK(p.refusal.empty());
    if (!p.refusal.empty()) return;
    CHECK(p.n == n && p.dim == dim && p.K == K && p.block == block && p.n_blocks == n_blocks && p.n_blocks <= concurrency);
    CHECK((n - 1) / p.block < p.n_blocks && (long)(p.n_blocks - 1) * p.block < n);      // (i / block) < n_blocks for every i; no empty block
    CHECK((unsigned long long)p.n_keys == (unsigned long long)n_blocks * K);
    CHECK((unsigned long long)((n - 1) / p.block) * K + (K - 1) < p.n_keys);            // the largest (block, cluster) key
    CHECK(p.end_bit >= 1 && p.end_bit <= 32 && ((unsigned long long)p.n_keys < (1ull << p.end_bit)));
    CHECK(p.end_bit == 1 || (unsigned long long)p.n_keys >= (1ull << (p.end_bit - 1)));  // minimal
    CHECK(p.seg == (size_t)p.n_keys + 2);
    CHECK(p.n_seg_elems == (size_t)p.n_keys * dim && p.segsum == p.n_seg_elems);
    CHECK(p.key == (size_t)n && p.csum == (size_t)K * dim && p.csize == (size_t)K && p.bsum == (size_t)p.n_blocks);
    CHECK(p.grid_block_sum == (unsigned)p.n_blocks);
    CHECK((long)p.grid_keys * 256 >= n && ((long)p.grid_keys - 1) * 256 < n);
    CHECK((unsigned long long)p.grid_segments * 256 >= (unsigned long long)p.n_keys + 1);
    CHECK((unsigned long long)p.grid_segment_sum * 256 >= p.n_seg_elems && (unsigned long long)p.grid_segment_sum * 256 < (1ull << 32));
    CHECK((long)p.grid_centroid * 256 >= (long)K * dim && (long)K * dim + 255 <= INT_MAX);
}

static void check_plans() {
    const long edges[] = {1, 2, 50, 511, 512, 513, 3001, 9001, ((long)1 << 31) - 1, (long)1 << 31, ((long)1 << 31) + 1,
                          ((long)1 << 32) - 1, (long)1 << 32, ((long)1 << 32) + 1};
    for (long n : edges)
        for (int dim = 1; dim <= 200; dim++)
            for (int K = 1; K <= 70; K++) {
                for (int reset = 0; reset < 2; reset++)
                    for (int engine = 0; engine < 2; engine++) {
                        check_assign(n, dim, 0, K, reset != 0, engine);
                        if (K > 1) check_assign(n, dim, K / 2, K, reset != 0, engine);
                    }
                const long conc[] = {1, 2, 3, 16, 37, 64, 1000, n - 1, n, n + 1, INT_MAX};
                for (long c : conc)
                    if (c >= 1 && c <= INT_MAX) check_lloyd(n, dim, K, (int)c);
            }
    for (long n : {1L, 2L, 50L, 511L, 512L, 513L})              // concurrency 1 .. n + 1, all of them
        for (int dim : {1, 13, 200})
            for (int K : {1, 17, 70})
                for (int c = 1; c <= n + 1; c++) check_lloyd(n, dim, K, c);
    // every refusal
    CHECK(has(plan_kmeans_assign(0, 13, 0, 4, true, 0).refusal, "0 points"));
    CHECK(has(plan_kmeans_assign(100, 0, 0, 4, true, 0).refusal, "0 dimensions"));
    CHECK(has(plan_kmeans_assign(100, 13, -1, 4, true, 0).refusal, "centres [-1, 4)"));
    CHECK(has(plan_kmeans_assign(100, 13, 5, 4, true, 0).refusal, "centres [5, 4)"));
    CHECK(has(plan_kmeans_assign(100, 13, 0, KM_MAX_CENTRES + 1, true, 0).refusal, "centres (at most"));
    CHECK(plan_kmeans_assign(100, 13, 0, KM_MAX_CENTRES, true, 0).refusal.empty());
    CHECK(has(plan_kmeans_assign(KM_ASSIGN_MAX_N, 13, 0, 4, true, 0).refusal, "nearest-centre grid"));
    CHECK(plan_kmeans_assign(KM_ASSIGN_MAX_N - 1, 13, 0, 4, true, 0).grid == (1u << 23));         // the largest grid: 2^32 / 512
    CHECK(has(plan_lloyd_full(0, 13, 4, 1).refusal, "0 points"));
    CHECK(has(plan_lloyd_full(100, 13, 0, 1).refusal, "0 clusters"));
    CHECK(has(plan_lloyd_full(100, 13, 4, 0).refusal, "0 workers"));
    CHECK(has(plan_lloyd_full((long)1 << 32, 13, 4, 1).refusal, "32-bit sort keys"));
    CHECK(plan_lloyd_full(((long)1 << 32) - 1, 13, 4, 1).refusal.empty());
    CHECK(has(plan_lloyd_full((long)1 << 31, 13, 4, INT_MAX).refusal, "1073741824 worker blocks x 4 clusters"));     // blocks of 2 points
    CHECK(has(plan_lloyd_full(100000, 40000, 70000, 1).refusal, "centroid kernel"));
    CHECK(has(plan_lloyd_full(1000000, 4000, 2048, 1000).refusal, "segment-sum grid"));
    CHECK(plan_lloyd_full(1000000, 39, 2048, 64).refusal.empty());
}

// ---- (c) the stream ----
static void check_stream() {
    GlibcRand g;
    for (int i = 0; i < 3000; i++) CHECK(g.next() == rand());       // (this process has not called rand() or srand() before)
    int first[3000];
    reference_rand_sample(first, 3000);
    GlibcRand h;
    for (int i = 0; i < 3000; i++) CHECK(first[i] == h.next());
    int32_t a[36], b[36], c[36];
    RandStream shared(-1), own(5);
    burn_reference_rand(7);
    reference_rand_state(a, false);
    int want[20], got[20];
    for (int i = 0; i < 20; i++) want[i] = shared();
    reference_rand_state(b, false);
    CHECK(std::memcmp(a, b, sizeof a) != 0);
    reference_rand_state(a, true);
    reference_rand_state(c, false);
    CHECK(std::memcmp(a, c, sizeof a) == 0);                           // through a get / set round trip unchanged
    for (int i = 0; i < 20; i++) got[i] = shared();
    CHECK(std::memcmp(want, got, sizeof want) == 0);
    GlibcRand six(6);
    for (int i = 0; i < 20; i++) CHECK(own() == six.next());        // a seeded stream: GlibcRand(seed + 1), untouched by the shared one
}

// ---- (b) the drivers on a host back end: subtract, multiply, add in dimension order; a strictly closer centre wins; the
// reference's block-ordered sums ----
struct HostBackend {
    const float *X;
    long n;
    int dim;
    std::vector<double> dist;
    std::vector<int> belong;
    KmBackend ops() {
        KmBackend be;
        be.assign = [this](const std::vector<double> &C, int c_begin, int c_end, std::vector<double> &d_io, std::vector<int> &b_io, bool reset, bool download) {
            if (reset) {
                dist.assign((size_t)n, 1.7976931348623157e308);
                belong.assign((size_t)n, -1);
            } else {
                dist = d_io;
                belong = b_io;
            }
            for (long i = 0; i < n; i++)
                for (int j = c_begin; j < c_end; j++) {
                    double s = 0.0;
                    for (int d = 0; d < dim; d++) {
                        const double t = (double)X[(size_t)i * dim + d] - C[(size_t)j * dim + d];
                        s = s + t * t;
                    }
                    if (s < dist[(size_t)i]) {
                        dist[(size_t)i] = s;
                        belong[(size_t)i] = j;
                    }
                }
            if (download) {
                d_io = dist;
                b_io = belong;
            }
        };
        be.lloyd_sums = [this](const KmLloydPlan &p, std::vector<double> &bsum, std::vector<double> &csum, std::vector<int> &csize) {
            bsum.assign(p.bsum, 0.0);
            csum.assign(p.csum, 0.0);
            csize.assign(p.csize, 0);
            std::vector<double> part(p.csum);
            for (int b = 0; b < p.n_blocks; b++) {
                std::fill(part.begin(), part.end(), 0.0);
                double s = 0.0;
                for (long i = b * p.block; i < std::min(p.n, (b + 1) * p.block); i++) {
                    s += dist[(size_t)i];
                    if (belong[(size_t)i] < 0) continue;
                    csize[(size_t)belong[(size_t)i]]++;
                    for (int d = 0; d < dim; d++) part[(size_t)belong[(size_t)i] * dim + d] += (double)X[(size_t)i * dim + d];
                }
                bsum[(size_t)b] = s;
                for (size_t e = 0; e < p.csum; e++) csum[e] += part[e];
            }
            return 0L;
        };
        return be;
    }
};

static int run_driver(const char *manifest, const char *outdir) {
    std::ifstream in(manifest);
    std::string line;
    int cases = 0;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string name, path;
        long n, seed;
        int K, D, conc, km;
        if (!(ls >> name >> n >> K >> D >> conc >> seed >> km >> path)) continue;
        std::vector<float> X((size_t)n * D);
        std::ifstream xf(path, std::ios::binary);
        xf.read(reinterpret_cast<char *>(X.data()), (std::streamsize)(X.size() * sizeof(float)));
        CHECK((size_t)xf.gcount() == X.size() * sizeof(float));
        HostBackend hb{X.data(), n, D, {}, {}};
        KmStart s;
        const std::string why = init_like_reference(hb.ops(), X.data(), n, D, K, std::max(1, conc), km, 0, seed, s);
        const std::string out = std::string(outdir) + "/" + name + (why.empty() ? ".means" : ".error");
        std::ofstream of(out, std::ios::binary);
        if (why.empty()) {
            CHECK(s.mean.size() == (size_t)K * D && s.sigma.size() == (size_t)D);
            of.write(reinterpret_cast<const char *>(s.mean.data()), (std::streamsize)(s.mean.size() * sizeof(double)));
            of.write(reinterpret_cast<const char *>(s.sigma.data()), (std::streamsize)(s.sigma.size() * sizeof(double)));
        } else {
            of << why;
        }
        cases++;
    }
    // the drivers' own refusals and the labels entry
    {
        std::vector<float> X = {0.f, 1.f, 0.f, 2.f, 0.f, 4.f};              // the first of two dimensions is constant
        HostBackend hb{X.data(), 3, 2, {}, {}};
        KmStart s;
        CHECK(has(init_like_reference(hb.ops(), X.data(), 3, 2, 2, 1, 1, 0, 3, s), "zero variance"));
        CHECK(s.sigma.size() == 2 && s.mean.empty());
        CHECK(has(init_like_reference(hb.ops(), X.data(), (long)INT_MAX + 1, 2, 2, 1, 0, 0, 3, s), "32-bit draws and labels"));      // (refused before X is read)
        std::vector<int> labels;
        CHECK(has(kmeans_labels_on(hb.ops(), X.data(), (long)INT_MAX + 1, 2, 2, 3, labels), "32-bit draws and labels"));
        std::vector<float> Y((size_t)300 * 3);
        for (size_t e = 0; e < Y.size(); e++) Y[e] = (float)(uniform(91, e) + 4.0 * (double)((e / 3) % 3));
        HostBackend hy{Y.data(), 300, 3, {}, {}};
        CHECK(kmeans_labels_on(hy.ops(), Y.data(), 300, 3, 3, 7, labels).empty() && labels.size() == 300);
        for (size_t i = 3; i < labels.size(); i++) CHECK(labels[i] >= 0 && labels[i] < 3 && labels[i] == labels[i % 3]);      // three blobs 4 apart
        CHECK(labels[0] != labels[1] && labels[1] != labels[2] && labels[0] != labels[2]);
    }
    std::printf("%d driver cases\n", cases);
    return cases;
}

// ---- (d) threads ----
static void check_threads() {
    const int np = 1801, dim = 39, K = 900, conc = 16;                 // np * dim > 2^16: where the driver starts its k-means++ workers
    std::vector<double> cand((size_t)np * dim), weight((size_t)np);
    for (size_t e = 0; e < cand.size(); e++) cand[e] = 8.0 * uniform(5, e) - 4.0;
    for (int i = 0; i < np; i++) {
        weight[(size_t)i] = 1.0 + (double)(hash64(6, (uint64_t)i) % 9);
        if (i % 11 == 0) cand[(size_t)i * dim + 3] = 0.0;               // a coordinate a sparse instance drops
    }
    std::vector<double> pp[2], lw[2];
    const int threads[2] = {1, 16};
    for (int v = 0; v < 2; v++) {
        RefRandom r(12345);
        pp[v] = kmeanspp_weighted(cand, weight, np, dim, K, conc, r, threads[v]);
        CHECK(pp[v].size() == (size_t)K * dim);
    }
    CHECK(pp[0] == pp[1] && std::memcmp(pp[0].data(), pp[1].data(), pp[0].size() * sizeof(double)) == 0);
    const int KL = 64;                                                  // np * KL * dim > 2^22: where the driver gives lloyd_weighted threads
    CHECK((size_t)np * KL * dim > ((size_t)1 << 22) && (size_t)np * dim > ((size_t)1 << 16));
    for (int v = 0; v < 2; v++) {
        lw[v].assign(pp[0].begin(), pp[0].begin() + (size_t)KL * dim);
        lloyd_weighted(cand, weight, np, dim, KL, conc, threads[v], lw[v]);
        CHECK(lw[v].size() == (size_t)KL * dim);
    }
    CHECK(lw[0].size() == lw[1].size() && std::memcmp(lw[0].data(), lw[1].data(), lw[0].size() * sizeof(double)) == 0);
    // an exception in round 3, with the workers waiting for it to begin: they are joined, the program goes on
    static int rounds = 0;
    bool thrown = false;
    try {
        RefRandom r(12345);
        (void)kmeanspp_weighted(cand, weight, np, dim, K, conc, r, 16, [](int k) {
            rounds++;
            if (k == 3) throw std::runtime_error("round 3");
        });
    } catch (const std::runtime_error &e) {
        thrown = std::string(e.what()) == "round 3";
    }
    CHECK(thrown && rounds == 3);
    RefRandom r(12345);
    const std::vector<double> again = kmeanspp_weighted(cand, weight, np, dim, K, conc, r, 16);
    CHECK(again == pp[0]);
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "plans") {
        check_stream();                     // first: before anything else could call rand()
        check_plans();
        std::printf("%ld plans\n", plans);
    } else if (mode == "driver" && argc == 4) {
        CHECK(run_driver(argv[2], argv[3]) > 0);
    } else if (mode == "threads") {
        check_threads();
    } else {
        std::fprintf(stderr, "usage: kmeans_checks plans | driver MANIFEST OUTDIR | threads\n");
        return 2;
    }
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("kmeans checks ok\n");
    return 0;
}
