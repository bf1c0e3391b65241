// kmeans_init.hip -- the device back end of the start in front of EM (kmeans_host.cpp has the stages and the drivers, decision for
// decision the reference's; kmeans_plan.cpp what is decided before a launch).
//
// Arithmetic: the reference works in float64 and sums in a fixed order (per worker block of
// ceil(n / concurrency) points, then over the blocks); sums that feed a decision are formed in that
// order here as well.  The O(n K D) part -- nearest centre and squared distance of every point -- runs on
// the device in float64, dimension by dimension with separate multiply and add as the reference's SSE2
// build does (no FMA).  The per-cluster sums of a Lloyd step on the full data are formed on the device too
// (round 3), in the reference's order: a stable radix sort of the points by (worker block, cluster) puts every
// (block, cluster)'s members side by side in point order; one thread per (block, cluster, dimension) adds them one
// after the other, one per (cluster, dimension) the blocks' sums in block order -- the additions calc_belonging and
// Lloyds_iteration make (kmeans.cc:72-107, :189-212), bit for bit, at device bandwidth instead of 9 s of host
// loops in front of a 2048-mixture UBM.
#include "kmeans_init.hpp"

#include "kmeans_host.hpp"
#include "score.hpp"

#include "../../include/pygmm_hip.h"

#include <rocprim/device/device_radix_sort.hpp>     // the device radix sort of the Lloyd step (rocPRIM: the native library; hipCUB wraps it in CUB's API)

#include <algorithm>
#include <atomic>

namespace sr {

namespace {

typedef double km_d2 __attribute__((ext_vector_type(2)));

// Nearest centre among centres [c_begin, c_end): dist[i] / belong[i] are updated when a centre is STRICTLY
// closer (kmeansII.cc:59-72; with dist preset to DBL_MAX it is the full search of kmeans.cc:87-99).
// float64, dimension by dimension, subtract - multiply - add as the reference's SSE2 build (no FMA): the distances
// and therefore every decision taken on them are the reference's, bit for bit.  A lane keeps two points in registers
// (fp32, widened per use) and 2 x 16 running sums; a chunk of 16 centres sits in LDS transposed ([d][centre]), so one
// 16-byte broadcast read feeds two centres x two points x three operations: the kernel is bound by the fp64 vector rate
// (round 2's one point per lane and one 8-byte read per three operations was bound by LDS issue: 21 ms per pass of
// 1 M points x 2048 centres x 39 dims).
template <int DIM_MAX>
__global__ __launch_bounds__(256, 2)
void kmeans_assign_kernel(const float *__restrict__ X, long n, int dim, const double *__restrict__ C,
                          int c_begin, int c_end, double *__restrict__ dist, int *__restrict__ belong, int reset,
                          const int *__restrict__ list, const int *__restrict__ n_list) {
    // (list != nullptr: only the points list[0 .. *n_list), the ones the fast pass below could not decide)
    const long n_work = list ? (long)*n_list : n;
    __shared__ km_d2 cs[DIM_MAX * KM_CH / 2];    // [d][KM_CH]
    double *csd = reinterpret_cast<double *>(cs);
    constexpr bool XREG = DIM_MAX <= 40;         // wider rows are re-read (L1 / L2) instead of held: 2 x 128 registers would spill
    float x[KM_PP][XREG ? DIM_MAX : 1];
    const float *xsrc[KM_PP];
    long idx[KM_PP];
    bool valid[KM_PP];
    double best[KM_PP];
    int best_j[KM_PP];
#pragma unroll
    for (int p = 0; p < KM_PP; p++) {
        idx[p] = ((long)blockIdx.x * KM_PP + p) * 256 + threadIdx.x;
        valid[p] = idx[p] < n_work;
        if (list) idx[p] = valid[p] ? (long)list[idx[p]] : 0;
        const float *src = X + (valid[p] ? idx[p] : 0) * dim;
        xsrc[p] = src;
        if constexpr (XREG) {
#pragma unroll
            for (int d = 0; d < DIM_MAX; d++) x[p][d] = d < dim ? src[d] : 0.f;
        }
        best[p] = reset ? 1.7976931348623157e308 : valid[p] ? dist[idx[p]] : 0.0;     // reset: a fresh search (DBL_MAX, no centre yet)
        best_j[p] = reset ? -1 : valid[p] ? belong[idx[p]] : 0;
    }
    if ((long)blockIdx.x * KM_PP * 256 >= n_work) return;         // (list mode: the grid is sized for the worst case)
    for (int c0 = c_begin; c0 < c_end; c0 += KM_CH) {
        const int nc = min(KM_CH, c_end - c0);
        double acc[KM_PP][KM_CH];
#pragma unroll
        for (int p = 0; p < KM_PP; p++)
#pragma unroll
            for (int j = 0; j < KM_CH; j++) acc[p][j] = 0.0;
        // (rows wider than DIM_MAX -- the reference has no limit -- take the chunk's centres DIM_MAX dimensions at a time; the
        // running sums go on in dimension order, so the distances are still the reference's bit for bit)
        for (int d0 = 0; d0 < dim; d0 += DIM_MAX) {
        const int dn = min(DIM_MAX, dim - d0);
        __syncthreads();
        for (int e = threadIdx.x; e < KM_CH * dn; e += 256) {
            const int j = e / dn, d = e - j * dn;
            csd[d * KM_CH + j] = j < nc ? C[(size_t)(c0 + j) * dim + d0 + d] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int d = 0; d < DIM_MAX; d++) {
            if (d < dn) {
                double xv[KM_PP];
#pragma unroll
                for (int p = 0; p < KM_PP; p++) xv[p] = XREG ? (double)x[p][XREG ? d : 0] : (double)xsrc[p][d0 + d];
#pragma unroll
                for (int j2 = 0; j2 < KM_CH / 2; j2++) {
                    const km_d2 c = cs[d * (KM_CH / 2) + j2];
#pragma unroll
                    for (int p = 0; p < KM_PP; p++) {
                        const double d0 = __dsub_rn(xv[p], c.x), d1 = __dsub_rn(xv[p], c.y);
                        acc[p][2 * j2] = __dadd_rn(acc[p][2 * j2], __dmul_rn(d0, d0));      // mul, then add: the reference has no FMA
                        acc[p][2 * j2 + 1] = __dadd_rn(acc[p][2 * j2 + 1], __dmul_rn(d1, d1));
                    }
                }
                __builtin_amdgcn_sched_barrier(0);      // (keeps the next dimensions' LDS reads from being hoisted: registers)
            }
        }
        }
#pragma unroll
        for (int p = 0; p < KM_PP; p++)
#pragma unroll
            for (int j = 0; j < KM_CH; j++)
                if (j < nc && acc[p][j] < best[p]) {
                    best[p] = acc[p][j];
                    best_j[p] = c0 + j;
                }
    }
#pragma unroll
    for (int p = 0; p < KM_PP; p++)
        if (valid[p]) {
            dist[idx[p]] = best[p];
            belong[idx[p]] = best_j[p];
        }
}

// ---- the full search, fast (round 3) ----
// 99 Lloyd steps of the exact pass above (10 ms each at K = 2048 on 1 M points: 3 float64 operations per point, centre and
// dimension) were three quarters of the k-means|| start.  The DECISION only needs the exact arithmetic where two centres are
// nearly equally close: ||x - c||^2 - ||x||^2 = ||c||^2 - 2 x.c is ONE fused multiply-add per dimension, and its error is
// bounded by (D + 2) 2^-53 x 2 (||x||^2 + ||c||^2) < 1e-14 (||x||^2 + max ||c||^2).  A point whose best and second-best values
// are further apart than tau = 2^-40 (||x||^2 + max ||c||^2) -- ~50 x that bound on each side, and far above the rounding of
// the reference's own sums -- has the same nearest centre in the reference's arithmetic; its distance is then formed the
// reference's way (subtract, multiply, add, dimension by dimension) for that one centre.  The others (exact ties between
// duplicate centres, the odd near-tie) go on a list and through the exact pass: same belong[] and dist[], bit for bit
// (test_kmeans_fast_assign_equals_the_exact_pass), 4 ms instead of 10.

__global__ __launch_bounds__(256)
void kmeans_centre_prep_kernel(const double *__restrict__ C, int K, int dim, int dim_max, double *__restrict__ rec,
                               double *__restrict__ cn_max_bits) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int k_pad = (K + KM_CH - 1) / KM_CH * KM_CH;
    if (j >= k_pad) return;
    double *r = rec + (size_t)(j / KM_CH) * km_rec_doubles(dim_max);
    const int col = j % KM_CH;
    if (j >= K) {                                       // padding of the last record: never wins, never the runner-up that matters
        for (int d = 0; d < dim_max; d++) r[d * KM_CH + col] = 0.0;
        r[dim_max * KM_CH + col] = 1.7976931348623157e308;
        return;
    }
    double s = 0.0;
    for (int d = 0; d < dim; d++) {
        const double c = C[(size_t)j * dim + d];
        s = fma(c, c, s);
    }
    // a centre with a NaN or infinite coordinate (an empty cluster: the reference divides by zero, kmeans.cc:229-233) is never
    // STRICTLY closer than anything in the exact pass; here it gets the value 1e300 for every point, so that the search below
    // can use plain min / max (no NaN handling) -- and if nothing else exists, the exact pass decides
    const bool finite = s == s && s < 1.0e300;
    for (int d = 0; d < dim_max; d++) r[d * KM_CH + col] = (finite && d < dim) ? -2.0 * C[(size_t)j * dim + d] : 0.0;
    r[dim_max * KM_CH + col] = finite ? s : 1.0e300;
    if (finite)
        atomicMax(reinterpret_cast<unsigned long long *>(cn_max_bits), (unsigned long long)__double_as_longlong(s));   // s >= 0: bit order = value order
}

template <int DIM_MAX>
__global__ __launch_bounds__(256, 2)
void kmeans_assign_fast_kernel(const float *__restrict__ X, long n, int dim, const double *__restrict__ C, const double *__restrict__ rec,
                               const double *__restrict__ cn_max, int K, double *__restrict__ dist,
                               int *__restrict__ belong, int *__restrict__ list, int *__restrict__ n_list) {
    constexpr int REC = km_rec_doubles(DIM_MAX);
    constexpr int PIECES = REC / 128;                       // 1 KiB wave-instructions per record
    __shared__ double buf_a[REC];                           // (two arrays, not one: hipcc then knows a read of one cannot alias the
    __shared__ double buf_b[REC];                           //  LDS-DMA in flight into the other, and does not drain vmcnt in front of it)
    static_assert(DIM_MAX <= 40, "rows held in registers");
    float x[KM_PP][DIM_MAX];
    long idx[KM_PP];
    bool valid[KM_PP];
    double best[KM_PP], second[KM_PP];
    int best_j[KM_PP];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
    for (int p = 0; p < KM_PP; p++) {
        idx[p] = ((long)blockIdx.x * KM_PP + p) * 256 + threadIdx.x;
        valid[p] = idx[p] < n;
        const float *src = X + (valid[p] ? idx[p] : 0) * dim;
#pragma unroll
        for (int d = 0; d < DIM_MAX; d++) x[p][d] = d < dim ? src[d] : 0.f;
        best[p] = second[p] = 1.7976931348623157e308;
        best_j[p] = -1;
    }
    // A record is fetched by LDS-DMA while the one before it is being used (staging through registers under the arithmetic
    // cost seven registers this kernel does not have: 1.15 s instead of 1.07 for the K = 2048 start; two barriers and an exposed
    // L2 round trip per chunk, as the exact pass has them, are a third of that pass's time).
    auto fetch = [&](double *dst, int chunk) {
        const double *src = rec + (size_t)chunk * REC;
#pragma unroll
        for (int i = 0; i < (PIECES + 3) / 4; i++) {
            const int piece = i * 4 + wave;
            if (piece < PIECES)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + piece * 128 + lane * 2),
                                                 (__attribute__((address_space(3))) void *)(dst + piece * 128), 16, 0, 0);
        }
    };
    auto chunk_pass = [&](const double *cur, int c0) {
        const km_d2 *cs = reinterpret_cast<const km_d2 *>(cur);
        const double *cns = cur + DIM_MAX * KM_CH;
        double acc[KM_PP][KM_CH];
#pragma unroll
        for (int p = 0; p < KM_PP; p++)
#pragma unroll
            for (int j = 0; j < KM_CH; j++) acc[p][j] = cns[j];
#pragma unroll
        for (int d = 0; d < DIM_MAX; d++) {
            if (d < dim) {
                double xv[KM_PP];
#pragma unroll
                for (int p = 0; p < KM_PP; p++) xv[p] = (double)x[p][d];
#pragma unroll
                for (int j2 = 0; j2 < KM_CH / 2; j2++) {
                    const km_d2 c = cs[d * (KM_CH / 2) + j2];
#pragma unroll
                    for (int p = 0; p < KM_PP; p++) {
                        acc[p][2 * j2] = fma(xv[p], c.x, acc[p][2 * j2]);
                        acc[p][2 * j2 + 1] = fma(xv[p], c.y, acc[p][2 * j2 + 1]);
                    }
                }
            }
        }
#pragma unroll
        for (int p = 0; p < KM_PP; p++)
#pragma unroll
            for (int j = 0; j < KM_CH; j++) {                     // (the padding of the last record holds DBL_MAX: it loses to everything)
                const double v = acc[p][j];
                second[p] = fmin(second[p], fmax(v, best[p]));    // the loser of (v, best) against the runner-up so far
                best_j[p] = v < best[p] ? c0 + j : best_j[p];
                best[p] = fmin(best[p], v);
            }
    };
    const int n_chunks = (K + KM_CH - 1) / KM_CH;
    fetch(buf_a, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int ch = 0; ch < n_chunks; ch += 2) {
        if (ch + 1 < n_chunks) fetch(buf_b, ch + 1);
        chunk_pass(buf_a, ch * KM_CH);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's pieces of the next record have landed ...
        __syncthreads();                                          // ... and everybody's; and everybody is done with buf_a
        if (ch + 1 >= n_chunks) break;
        if (ch + 2 < n_chunks) fetch(buf_a, ch + 2);
        chunk_pass(buf_b, (ch + 1) * KM_CH);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    const double cmax = *cn_max;
#pragma unroll
    for (int p = 0; p < KM_PP; p++) {
        if (!valid[p]) continue;
        double xn = 0.0, d2 = 1.7976931348623157e308;
        if (best_j[p] >= 0) {
            const double *c = C + (size_t)best_j[p] * dim;
            d2 = 0.0;
#pragma unroll
            for (int d = 0; d < DIM_MAX; d++)
                if (d < dim) {
                    const double xd = (double)x[p][d];
                    const double t = __dsub_rn(xd, c[d]);
                    d2 = __dadd_rn(d2, __dmul_rn(t, t));          // the reference's arithmetic for the centre that won
                    xn = fma(xd, xd, xn);
                }
        }
        dist[idx[p]] = d2;
        belong[idx[p]] = best_j[p];
        const double tau = ldexp(xn + cmax, -40);
        if (best_j[p] >= 0 && !(second[p] - best[p] >= tau && best[p] < 1.0e299)) {     // too close to call (or no finite centre): the exact pass decides
            const int at = atomicAdd(n_list, 1);
            list[at] = (int)idx[p];
        }
    }
}

struct KmWorkspace {
    DevBuf<float> X;
    DevBuf<double> C, dist;
    DevBuf<int> belong;
    DevBuf<double> m2c, cn_max;          // the fast full search: its chunk records (-2 c, ||c||^2), the largest ||c||^2
    DevBuf<int> list, n_list;           // points it leaves to the exact pass
    // Lloyd on the full data, cluster sums on the device
    DevBuf<unsigned> key_in, key_out, idx_in, idx_out, seg;
    DevBuf<char> sort_tmp;
    DevBuf<double> csum, bsum, segsum;
    DevBuf<int> csize;
};
KmWorkspace &kws() { return per_device<KmWorkspace>(); }
int &kmeans_assign_engine_option() {        // 0: the fast full search with the exact pass behind it; 1: the exact pass alone
    static int v = 0;
    return v;
}
std::atomic<long> g_km_fast_passes{0}, g_km_fast_rechecked{0};     // full searches taken the fast way; points they left to the exact pass

// key = worker block * K + cluster (a point without a cluster -- NaN centres -- sorts behind everything); value = the point
__global__ __launch_bounds__(256)
void lloyd_keys_kernel(const int *__restrict__ belong, long n, long block, int K, unsigned n_keys, unsigned *__restrict__ key,
                       unsigned *__restrict__ idx) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int j = belong[i];
    key[i] = j >= 0 ? (unsigned)(i / block) * (unsigned)K + (unsigned)j : n_keys;
    idx[i] = (unsigned)i;
}

// seg[k] = first position of key k in the sorted keys (k = 0 .. n_keys inclusive)
__global__ __launch_bounds__(256)
void lloyd_segments_kernel(const unsigned *__restrict__ sorted, long n, unsigned n_keys, unsigned *__restrict__ seg) {
    const unsigned k = blockIdx.x * 256 + threadIdx.x;
    if (k > n_keys) return;
    long lo = 0, hi = n;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (sorted[mid] < k) lo = mid + 1; else hi = mid;
    }
    seg[k] = (unsigned)lo;
}

// One thread per (block b, cluster j, dimension d): the members of (b, j) one after the other in point order into a sum
// that starts at 0.0 (calc_belonging's new_centroids, kmeans.cc:78-103); consecutive threads take consecutive dimensions of
// the same member rows.
__global__ __launch_bounds__(256)
void lloyd_segment_sum_kernel(const float *__restrict__ X, int dim, size_t n_seg_elems, const unsigned *__restrict__ seg,
                              const unsigned *__restrict__ idx, double *__restrict__ buf) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_seg_elems) return;
    const size_t k = e / dim;
    const int d = (int)(e - k * dim);
    const unsigned lo = seg[k], hi = seg[k + 1];
    double s = 0.0;
    for (unsigned p = lo; p < hi; p++) s = __dadd_rn(s, (double)X[(size_t)idx[p] * dim + d]);
    buf[e] = s;
}

// One thread per (cluster j, dimension d): the blocks' sums in block order into a total that starts at 0.0 (Lloyds_iteration,
// kmeans.cc:198-204) -- an empty (block, cluster) adds its 0.0 like the reference -- and the cluster's size.
__global__ __launch_bounds__(256)
void lloyd_centroid_kernel(int dim, int K, int n_blocks, const unsigned *__restrict__ seg, const double *__restrict__ buf,
                           double *__restrict__ csum, int *__restrict__ csize) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= K * dim) return;
    const int j = e / dim;
    double total = 0.0;
    int count = 0;
    for (int b = 0; b < n_blocks; b++) {
        total = __dadd_rn(total, buf[(size_t)b * K * dim + e]);
        count += (int)(seg[(size_t)b * K + j + 1] - seg[(size_t)b * K + j]);
    }
    csum[e] = total;
    if (e == j * dim) csize[j] = count;
}

// the sum of a worker block's distances in point order (calc_belonging's distsqr_sum, kmeans.cc:85-106): a workgroup per
// block stages the distances through LDS with coalesced loads, one thread adds them one after the other (a lone thread
// walking global memory pays a cache-miss latency per addend: 8 ms per Lloyd step at 4 k points per block)
__global__ __launch_bounds__(256)
void lloyd_block_sum_kernel(const double *__restrict__ dist, long n, long block, int n_blocks, double *__restrict__ bsum) {
    __shared__ double stage[KM_BS_CHUNK];
    const int b = blockIdx.x;
    const long lo = (long)b * block, hi = min(n, lo + block);
    double s = 0.0;
    for (long c0 = lo; c0 < hi; c0 += KM_BS_CHUNK) {
        const int m = (int)min((long)KM_BS_CHUNK, hi - c0);
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += 256) stage[i] = dist[c0 + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < m; i++) s = __dadd_rn(s, stage[i]);
    }
    if (threadIdx.x == 0) bsum[b] = s;
}


// The two operations of the start's back end (kmeans_host.hpp: KmBackend) on the current device, each following its plan.  The
// data go up with the first pass and stay (kws().X); dist / belong stay for lloyd_sums.
struct DeviceBackend {
    const float *X;
    long n;
    int dim;
    bool resident = false;
    KmAssignPlan last;                      // of the latest pass: was it a fast one?
    long sort_n = -1;                       // what sort_tmp was last sized for
    int sort_bits = -1;

    void assign(const std::vector<double> &C, int c_begin, int c_end, std::vector<double> &dist, std::vector<int> &belong, bool reset, bool download) {
        const KmAssignPlan p = plan_kmeans_assign(n, dim, c_begin, c_end, reset, kmeans_assign_engine_option());
        if (!p.refusal.empty()) fail("%s", p.refusal.c_str());
        auto &w = kws();
        if (!resident) {
            ensure_device();
            w.X.upload(X, (size_t)n * dim);
            resident = true;
        }
        w.C.upload(C.data(), p.C);
        if (reset) {
            w.dist.ensure(p.dist);
            w.belong.ensure(p.belong);
        } else {
            w.dist.upload(dist.data(), p.dist);
            w.belong.upload(belong.data(), p.belong);
        }
        if (p.fast) {
            // one fused multiply-add per point, centre and dimension decides wherever it can; the rest goes through the exact pass
            const int K = c_end;
            w.m2c.ensure(p.m2c);
            w.cn_max.ensure(p.cn_max);
            w.list.ensure(p.list);
            w.n_list.ensure(p.n_list);
            SR_HIP(hipMemsetAsync(w.cn_max.p, 0, sizeof(double), ctx().stream));
            SR_HIP(hipMemsetAsync(w.n_list.p, 0, sizeof(int), ctx().stream));
            hipLaunchKernelGGL(kmeans_centre_prep_kernel, dim3(p.prep_grid), dim3(256), 0, ctx().stream, w.C.p, K, dim, p.fast_dim_max, w.m2c.p,
                               w.cn_max.p);
            if (p.fast_dim_max == 16)
                hipLaunchKernelGGL(kmeans_assign_fast_kernel<16>, dim3(p.grid), dim3(256), 0, ctx().stream, w.X.p, n, dim, w.C.p, w.m2c.p,
                                   w.cn_max.p, K, w.dist.p, w.belong.p, w.list.p, w.n_list.p);
            else
                hipLaunchKernelGGL(kmeans_assign_fast_kernel<40>, dim3(p.grid), dim3(256), 0, ctx().stream, w.X.p, n, dim, w.C.p, w.m2c.p,
                                   w.cn_max.p, K, w.dist.p, w.belong.p, w.list.p, w.n_list.p);
        }
        const int *list = p.fast ? w.list.p : nullptr;
        const int *n_list = p.fast ? w.n_list.p : nullptr;
#define SR_KM_LAUNCH(DM)                                                                                                      \
    hipLaunchKernelGGL(kmeans_assign_kernel<DM>, dim3(p.grid), dim3(256), 0, ctx().stream, w.X.p, n, dim, w.C.p, c_begin, c_end, \
                       w.dist.p, w.belong.p, reset ? 1 : 0, list, n_list)
        if (p.exact_dim_max == 16) SR_KM_LAUNCH(16);
        else if (p.exact_dim_max == 40) SR_KM_LAUNCH(40);
        else if (p.exact_dim_max == 64) SR_KM_LAUNCH(64);
        else SR_KM_LAUNCH(128);
#undef SR_KM_LAUNCH
        SR_HIP(hipGetLastError());
        last = p;
        if (!download) return;                    // (Lloyd on the full data goes on with them on the device)
        w.dist.download(dist.data(), p.dist);
        w.belong.download(belong.data(), p.belong);
        sync_stream();
    }

    long lloyd_sums(const KmLloydPlan &p, std::vector<double> &bsum, std::vector<double> &csum, std::vector<int> &csize) {
        auto &w = kws();
        w.key_in.ensure(p.key);
        w.key_out.ensure(p.key);
        w.idx_in.ensure(p.key);
        w.idx_out.ensure(p.key);
        w.seg.ensure(p.seg);
        w.csum.ensure(p.csum);
        w.csize.ensure(p.csize);
        w.bsum.ensure(p.bsum);
        w.segsum.ensure(p.segsum);
        if (sort_n != p.n || sort_bits != p.end_bit) {
            size_t tmp_bytes = 0;
            SR_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, w.key_in.p, w.key_out.p, w.idx_in.p, w.idx_out.p, (size_t)p.n, 0u, (unsigned)p.end_bit, ctx().stream));
            w.sort_tmp.ensure(tmp_bytes);
            sort_n = p.n;
            sort_bits = p.end_bit;
        }
        bsum.resize(p.bsum);
        csum.resize(p.csum);
        csize.resize(p.csize);
        hipLaunchKernelGGL(lloyd_block_sum_kernel, dim3(p.grid_block_sum), dim3(256), 0, ctx().stream, w.dist.p, p.n, p.block, p.n_blocks, w.bsum.p);
        hipLaunchKernelGGL(lloyd_keys_kernel, dim3(p.grid_keys), dim3(256), 0, ctx().stream, w.belong.p, p.n, p.block, p.K, p.n_keys, w.key_in.p, w.idx_in.p);
        size_t tb = w.sort_tmp.n;
        SR_HIP(rocprim::radix_sort_pairs(w.sort_tmp.p, tb, w.key_in.p, w.key_out.p, w.idx_in.p, w.idx_out.p, (size_t)p.n, 0u, (unsigned)p.end_bit,
                                         ctx().stream));                                     // stable: point order inside a key
        hipLaunchKernelGGL(lloyd_segments_kernel, dim3(p.grid_segments), dim3(256), 0, ctx().stream, w.key_out.p, p.n, p.n_keys, w.seg.p);
        hipLaunchKernelGGL(lloyd_segment_sum_kernel, dim3(p.grid_segment_sum), dim3(256), 0, ctx().stream, w.X.p, p.dim, p.n_seg_elems, w.seg.p,
                           w.idx_out.p, w.segsum.p);
        hipLaunchKernelGGL(lloyd_centroid_kernel, dim3(p.grid_centroid), dim3(256), 0, ctx().stream, p.dim, p.K, p.n_blocks, w.seg.p, w.segsum.p,
                           w.csum.p, w.csize.p);
        SR_HIP(hipGetLastError());
        w.bsum.download(bsum.data(), bsum.size());
        w.csum.download(csum.data(), csum.size());
        w.csize.download(csize.data(), csize.size());
        int rechecked = 0;
        if (last.fast) w.n_list.download(&rechecked, 1);
        sync_stream();
        if (last.fast) {
            g_km_fast_passes++;
            g_km_fast_rechecked += rechecked;
        }
        return rechecked;
    }

    KmBackend ops() {
        return {[this](auto &&...a) { assign(a...); }, [this](auto &&...a) { return lloyd_sums(a...); }};
    }
};

}  // namespace

void set_kmeans_assign_engine(int v) { kmeans_assign_engine_option() = v; }
void kmeans_fast_stats(long *passes, long *rechecked) {
    if (passes) *passes = g_km_fast_passes.load();
    if (rechecked) *rechecked = g_km_fast_rechecked.load();
}

void init_gmm_like_reference(GMM &g, const float *X, long n, int dim, const Parameter &param, long seed) {
    const int K = g.nr_mixtures;
    g.dim = dim;
    DeviceBackend dev{X, n, dim};
    KmStart s;
    const std::string why = init_like_reference(dev.ops(), X, n, dim, K, std::max(1, param.concurrency), param.init_with_kmeans, param.verbosity, seed, s);
    // (a refused start leaves the handle what it got as far as: sigma, then mean)
    if (!s.sigma.empty()) {
        g.sigma.resize((size_t)K * dim);
        for (int k = 0; k < K; k++) std::copy(s.sigma.begin(), s.sigma.end(), g.sigma.begin() + (size_t)k * dim);
    }
    if (!s.mean.empty()) g.mean = s.mean;
    if (!why.empty()) fail("%s", why.c_str());
    g.weights.assign(K, 1.0 / K);                             // gmm.cc:356-360
    g.drop_single();
}

std::vector<int> kmeans_labels(const float *X, long n, int dim, int K, long seed) {
    DeviceBackend dev{X, n, dim};
    std::vector<int> labels;
    const std::string why = kmeans_labels_on(dev.ops(), X, n, dim, K, seed, labels);
    if (!why.empty()) fail("%s", why.c_str());
    return labels;
}

}  // namespace sr
