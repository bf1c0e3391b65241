// kmeans_plan.cpp -- the k-means start's two plans (kmeans_plan.hpp).  Host-only.
#include "kmeans_plan.hpp"

#include <climits>
#include <cmath>
#include <cstdio>

namespace sr {

namespace {
template <typename... A>
std::string text(const char *fmt, A... a) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a...);
    return buf;
}
}  // namespace

KmAssignPlan plan_kmeans_assign(long n, int dim, int c_begin, int c_end, bool reset, int engine) {
    KmAssignPlan p;
    if (n < 1 || dim < 1) p.refusal = text("k-means: %ld points of %d dimensions", n, dim);
    else if (c_begin < 0 || c_end < c_begin) p.refusal = text("k-means: centres [%d, %d)", c_begin, c_end);
    else if (c_end > KM_MAX_CENTRES) p.refusal = text("k-means: %d centres (at most %d)", c_end, KM_MAX_CENTRES);
    else if (n >= KM_ASSIGN_MAX_N) p.refusal = text("k-means: %ld points do not fit the nearest-centre grid", n);
    if (!p.refusal.empty()) return p;
    p.fast = reset && c_begin == 0 && dim <= KM_FAST_MAX_DIM && engine == 0 && n < KM_FAST_MAX_N;
    p.exact_dim_max = dim <= 16 ? 16 : dim <= 40 ? 40 : dim <= 64 ? 64 : 128;
    p.grid = (unsigned)((n + 256 * KM_PP - 1) / (256 * KM_PP));       // n < 2^32 (KM_ASSIGN_MAX_N): at most 2^23
    p.C = (size_t)c_end * dim;
    p.dist = p.belong = (size_t)n;
    if (p.fast) {
        p.fast_dim_max = dim <= 16 ? 16 : 40;
        p.n_chunks = (c_end + KM_CH - 1) / KM_CH;                      // c_end <= 2^30 (KM_MAX_CENTRES): no overflow, here or in n_chunks * KM_CH
        p.prep_grid = (unsigned)((p.n_chunks * KM_CH + 255) / 256);
        p.m2c = (size_t)p.n_chunks * km_rec_doubles(p.fast_dim_max);
        p.cn_max = p.n_list = 1;
        p.list = (size_t)n;
    }
    return p;
}

KmLloydPlan plan_lloyd_full(long n, int dim, int K, int concurrency) {
    KmLloydPlan p;
    if (n < 1 || dim < 1 || K < 1 || concurrency < 1) {
        p.refusal = text("k-means: %ld points of %d dimensions, %d clusters, %d workers", n, dim, K, concurrency);
        return p;
    }
    p.n = n;
    p.dim = dim;
    p.K = K;
    p.block = (long)std::ceil((double)n / concurrency);
    p.n_blocks = (int)((n + p.block - 1) / p.block);                  // block >= n / concurrency: at most `concurrency` blocks, an int
    if ((double)p.n_blocks * K >= 4.0e9 || n >= ((long)1 << 32)) {
        p.refusal = text("k-means: %d worker blocks x %d clusters x %ld points do not fit 32-bit sort keys", p.n_blocks, K, n);
        return p;
    }
    // lloyd_centroid_kernel holds K * dim and its own element index (up to K * dim + 255) in an int
    if ((long)K * dim > (long)INT_MAX - 256) {
        p.refusal = text("k-means: %d clusters x %d dimensions do not fit the centroid kernel's 32-bit index", K, dim);
        return p;
    }
    p.n_keys = (unsigned)p.n_blocks * (unsigned)K;                    // < 4e9 < 2^32 (above)
    p.end_bit = 1;
    while (p.end_bit < 32 && (1ull << p.end_bit) <= (unsigned long long)p.n_keys) p.end_bit++;      // keys 0 .. n_keys inclusive
    p.n_seg_elems = (size_t)p.n_keys * dim;                           // < 2^32 x 2^31
    // lloyd_segment_sum_kernel: one thread per element, ceil(n_seg_elems / 256) workgroups of 256 in an unsigned grid whose threads
    // the runtime counts in 32 bits
    if (p.n_seg_elems > ((size_t)1 << 32) - 256) {
        p.refusal = text("k-means: %d worker blocks x %d clusters x %d dimensions do not fit the segment-sum grid", p.n_blocks, K, dim);
        return p;
    }
    p.grid_block_sum = (unsigned)p.n_blocks;
    p.grid_keys = (unsigned)((n + 255) / 256);                        // n < 2^32: at most 2^24
    p.grid_segments = (p.n_keys + 1 + 255) / 256;                     // n_keys < 4e9: n_keys + 256 < 2^32, no wrap
    p.grid_segment_sum = (unsigned)((p.n_seg_elems + 255) / 256);     // <= 2^24 (above)
    p.grid_centroid = (unsigned)((K * dim + 255) / 256);              // K * dim + 255 <= INT_MAX (above)
    p.key = (size_t)n;
    p.seg = (size_t)p.n_keys + 2;
    p.csum = (size_t)K * dim;
    p.csize = (size_t)K;
    p.bsum = (size_t)p.n_blocks;
    p.segsum = p.n_seg_elems;
    return p;
}

}  // namespace sr
