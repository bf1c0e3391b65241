// diar.hip -- who spoke when with nobody enrolled: a feature batch [n_u][D] (fp32, resident) -> initial clusters and a merge log
// per recording.  The definitions (include/pygmm_hip.h states them in full; tests/diar_oracle.py restates them line by line):
//   segments    L frames each, n_seg = floor(n / L) (1 if that is 0 and n > 0), the last reaches to n.
//   statistics  N, s = sum x, Q = sum x x^T (lower triangle by rows), float64, every entry summed in frame order with one product
//               and one add per frame; a merge adds element by element.
//   logdet      Sigma = (Q - s s^T / N) / N + ridge I, 2 sum log L_rr of its Cholesky factor; a pivot that is not finite or not
//               positive fails the cluster: every distance that involves it is +inf.
//   dBIC(a, b)  1/2 [(Na + Nb) ld_ab - Na ld_a - Nb ld_b] - lambda 1/2 (D + D (D + 1) / 2) log(Na + Nb).
//   change      c[b] = dBIC(segments [b - m, b), segments [b, b + m)) (clipped, summed in index order); b is kept iff c[b] > 0,
//               c[b] > c[b'] for the earlier and c[b] >= c[b'] for the later b' with |b - b'| < m.
//   merge loop  the live pair (i < j) of smallest distance, the first in row-major order among equals; stop unless live > k_max, or
//               live > k_min and d < threshold; stop at +inf; else j into i, ld_i and row i again.
//
// Kernels:
//   diar_stats_kernel        a workgroup per base segment; the frames are staged through LDS 64 at a time, a lane owns up to nine
//                            entries of (s, Q) in registers and adds in frame order.  No atomics: a sum has one owner.
//   wave_logdet<DB>          a wave per matrix, a lane per row, the row in registers (D rounded up to 16 / 32 / 48 / 64 so that every
//                            register index is static); the merged Sigma is formed straight from two clusters' statistics; the
//                            right-looking factorisation passes column k's entries between lanes by readlane.  No LDS, no scratch.
//   diar_change_kernel       a wave per boundary: both sides' sums into LDS (a lane per entry, in index order), three logdets.
//   diar_peak_kernel         a lane per boundary: the peak rule.
//   diar_gather_kernel       a workgroup per initial cluster: the sum of its segments in index order.
//   diar_ld_kernel           a wave per cluster: its own logdet and whether it failed.
//   diar_pairs_kernel        a wave per pair (i < j) of a recording: the table.
//   ahc_argmin_kernel        up to 64 workgroups per recording, rows strided over them: first minimum of (distance, row-major rank)
//                            by wave_first_max_f64 on the negated value, then across the waves through LDS.
//   ahc_merge_kernel<DB>     a workgroup per recording: the second level of the reduction, the stop rule, the log, the merge of the
//                            statistics and ld_i (DB > 0) or of the sizes (DB = 0, the matrix mode).
//   diar_row_kernel<DB>      a wave per live k: dist(i, k).      ahc_row_matrix_kernel: a lane per k, the Lance-Williams update.
//   ahc_all_stopped_kernel   one word for the host, read back after every 16th step.
// The recordings of a group advance in lock-step on the grid's y; one that has stopped returns at once.  No grid-wide barrier, no
// atomics, no unbounded loop: the host enqueues at most max(n_init) - 1 steps.  The decisions are diar_plan.cpp's.
#pragma clang fp contract(off)

#include "diar.hpp"

#include "batch.hpp"
#include "wave_ops.hpp"

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

namespace sr {

namespace {

// the per-recording state of the merge loop: int32 [8]
constexpr int ST_STOP = 0, ST_LIVE = 1, ST_MERGES = 2, ST_I = 3, ST_J = 4, ST_CI = 5, ST_CJ = 6, ST_LEN = 8;

__device__ __forceinline__ double readlane_f64(double v, int lane) {
    union { double d; int i[2]; } a, b;
    a.d = v;
    b.i[0] = __builtin_amdgcn_readlane(a.i[0], lane);
    b.i[1] = __builtin_amdgcn_readlane(a.i[1], lane);
    return b.d;
}

__device__ __forceinline__ void take_first_max(double &v, int &r, double ov, int orank) {
    if (ov > v || (ov == v && orank < r)) {
        v = ov;
        r = orank;
    }
}

// ---- the wave-level factorisation ----
// log det of Sigma = (Q - s s^T / N) / N + ridge I of the cluster whose statistics are sa (+ sb, element by element, when sb is
// not null).  All 64 lanes of the wave call it with the same arguments; the result is the same in every lane.  Lane r keeps
// row r: a[j], j <= r (the rest of the register row stays 0 and is never read by a lane that matters).
template <int DB>
__device__ __forceinline__ double wave_logdet(const double *sa, const double *sb, int D, double ridge, bool &ok) {
    const int r = threadIdx.x & 63;
    const bool row = r < D;
    const double N = sb ? sa[0] + sb[0] : sa[0];
    double a[DB];
    double s_r = 0.0;
    if (row) s_r = sb ? sa[1 + r] + sb[1 + r] : sa[1 + r];
    const int base = 1 + D + r * (r + 1) / 2;
#pragma unroll
    for (int j = 0; j < DB; j++) {
        double v = 0.0;
        if (row && j <= r) {                                         // (j <= r < D)
            const double q = sb ? sa[base + j] + sb[base + j] : sa[base + j];
            const double s_j = sb ? sa[1 + j] + sb[1 + j] : sa[1 + j];
            v = (q - s_r * s_j / N) / N;
            if (j == r) v = v + ridge;
        }
        a[j] = v;
    }
    double ld = 0.0;
    ok = true;
#pragma unroll
    for (int k = 0; k < DB; k++) {
        if (k < D) {                                                 // (the same in every lane)
            const double piv = readlane_f64(a[k], k);
            if (!(piv > 0.0) || piv > DBL_MAX) ok = false;
            const double lkk = sqrt(piv);
            ld = ld + log(lkk);
            const double c = a[k] / lkk;                             // lane r >= k: L[r][k]
#pragma unroll
            for (int j = k + 1; j < DB; j++) {
                const double ljk = readlane_f64(c, j);
                a[j] = a[j] - c * ljk;
            }
        }
    }
    return 2.0 * ld;
}

__device__ __forceinline__ double delta_bic(double Na, double Nb, double ld_ab, double ld_a, double ld_b, double pen) {
    const double N = Na + Nb;
    return 0.5 * (N * ld_ab - Na * ld_a - Nb * ld_b) - pen * log(N);
}

// ---- segment statistics ----

__global__ __launch_bounds__(DIAR_STATS_WG)
void diar_stats_kernel(const float *__restrict__ X, const int64_t *__restrict__ frame_off, const int32_t *__restrict__ seg_rec,
                       const int64_t *__restrict__ seg_off, int D, int64_t L, double *__restrict__ stats) {
    extern __shared__ float lds_x[];                                 // [DIAR_STATS_CHUNK][D]
    const int tid = threadIdx.x;
    const int64_t seg = blockIdx.x;
    const int g = seg_rec[seg];
    const int64_t i = seg - seg_off[g], nseg = seg_off[g + 1] - seg_off[g];
    const int64_t row0 = frame_off[g], n = frame_off[g + 1] - row0;
    const int64_t fb = i * L, fe = i == nseg - 1 ? n : fb + L;
    const int P = diar_stat_len(D), E = P - 1;
    int er[DIAR_STATS_MAX_ENTRIES], ec[DIAR_STATS_MAX_ENTRIES];
    double acc[DIAR_STATS_MAX_ENTRIES];
#pragma unroll
    for (int q = 0; q < DIAR_STATS_MAX_ENTRIES; q++) {
        const int e = tid + q * DIAR_STATS_WG;
        acc[q] = 0.0;
        er[q] = -1;
        ec[q] = -1;
        if (e < D) {
            er[q] = e;
        } else if (e < E) {
            const int t = e - D;
            int r = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) / 2.0);
            while (r * (r + 1) / 2 > t) r--;
            while ((r + 1) * (r + 2) / 2 <= t) r++;
            er[q] = r;
            ec[q] = t - r * (r + 1) / 2;
        }
    }
    for (int64_t c0 = fb; c0 < fe; c0 += DIAR_STATS_CHUNK) {
        const int cn = (int)min((int64_t)DIAR_STATS_CHUNK, fe - c0);
        __syncthreads();                                             // the chunk before is read out
        const float *src = X + (row0 + c0) * D;                      // cn whole rows: inside the recording
        for (int idx = tid; idx < cn * D; idx += DIAR_STATS_WG) lds_x[idx] = src[idx];
        __syncthreads();
        for (int f = 0; f < cn; f++) {
#pragma unroll
            for (int q = 0; q < DIAR_STATS_MAX_ENTRIES; q++)
                if (er[q] >= 0) {
                    const double x = (double)lds_x[f * D + er[q]];
                    const double y = ec[q] >= 0 ? (double)lds_x[f * D + ec[q]] : 1.0;     // (s: x * 1 is x)
                    acc[q] = acc[q] + x * y;
                }
        }
    }
    double *out = stats + seg * P;
    if (tid == 0) out[0] = (double)(fe - fb);
#pragma unroll
    for (int q = 0; q < DIAR_STATS_MAX_ENTRIES; q++)
        if (er[q] >= 0) out[1 + tid + q * DIAR_STATS_WG] = acc[q];
}

// ---- change detection ----

template <int DB>
__global__ __launch_bounds__(64)
void diar_change_kernel(const double *__restrict__ seg_stats, const int32_t *__restrict__ bnd_rec, const int64_t *__restrict__ bnd_off,
                        const int64_t *__restrict__ seg_off, int D, int64_t m, double ridge, double pen, double *__restrict__ c_out) {
    extern __shared__ __attribute__((aligned(16))) double lds_s[];   // [2][P]
    const int lane = threadIdx.x;
    const int64_t bi = blockIdx.x;
    const int g = bnd_rec[bi];
    const int64_t b = bi - bnd_off[g] + 1, nseg = seg_off[g + 1] - seg_off[g], s0 = seg_off[g];
    const int64_t lo = max((int64_t)0, b - m), hi = min(nseg, b + m);
    const int P = diar_stat_len(D);
    for (int e = lane; e < P; e += 64) {
        double l = 0.0, r = 0.0;
        for (int64_t t = lo; t < b; t++) l = l + seg_stats[(s0 + t) * P + e];
        for (int64_t t = b; t < hi; t++) r = r + seg_stats[(s0 + t) * P + e];
        lds_s[e] = l;
        lds_s[P + e] = r;
    }
    wave_sync();
    double ld_a = 0.0, ld_b = 0.0, ld_ab = 0.0;
    bool all_ok = true;
#pragma unroll 1
    for (int t = 0; t < 3; t++) {                                    // a, b, a + b: one copy of the factorisation's code
        bool ok;
        const double v = wave_logdet<DB>(t == 1 ? lds_s + P : lds_s, t == 2 ? lds_s + P : nullptr, D, ridge, ok);
        if (t == 0) ld_a = v;
        else if (t == 1) ld_b = v;
        else ld_ab = v;
        all_ok = all_ok && ok;
    }
    if (lane == 0) c_out[bi] = all_ok ? delta_bic(lds_s[0], lds_s[P], ld_ab, ld_a, ld_b, pen) : (double)INFINITY;
}

__global__ __launch_bounds__(64)
void diar_peak_kernel(const double *__restrict__ c, const int32_t *__restrict__ bnd_rec, const int64_t *__restrict__ bnd_off, int64_t n_bnd,
                      int64_t m, int32_t *__restrict__ kept) {
    const int64_t bi = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (bi >= n_bnd) return;
    const int g = bnd_rec[bi];
    const int64_t b0 = bnd_off[g], nb = bnd_off[g + 1] - b0, b = bi - b0;        // b: 0-based among the recording's boundaries
    const double v = c[bi];
    bool keep = v > 0.0;
    const int64_t lo = max((int64_t)0, b - (m - 1)), hi = min(nb - 1, b + (m - 1));
    for (int64_t k = lo; k <= hi && keep; k++) {
        if (k == b) continue;
        const double w = c[b0 + k];
        if (k < b ? !(v > w) : !(v >= w)) keep = false;
    }
    kept[bi] = keep ? 1 : 0;
}

// ---- initial clusters ----

__global__ __launch_bounds__(DIAR_STATS_WG)
void diar_gather_kernel(const double *__restrict__ seg_stats, const int32_t *__restrict__ cl_rec, const int64_t *__restrict__ cl_off,
                        const int64_t *__restrict__ seg_off, const int64_t *__restrict__ init_off, int D, double *__restrict__ cl_stats) {
    const int64_t cl = blockIdx.x;
    const int g = cl_rec[cl];
    const int64_t c = cl - cl_off[g];
    const int64_t *io = init_off + cl_off[g] + g;                    // the recording's n_init + 1 run boundaries
    const int64_t s0 = seg_off[g] + io[c], s1 = seg_off[g] + io[c + 1];
    const int P = diar_stat_len(D);
    for (int e = threadIdx.x; e < P; e += DIAR_STATS_WG) {
        double a = 0.0;
        for (int64_t t = s0; t < s1; t++) a = a + seg_stats[t * P + e];
        cl_stats[cl * P + e] = a;
    }
}

template <int DB>
__global__ __launch_bounds__(64 * DIAR_WAVES)
void diar_ld_kernel(const double *__restrict__ cl_stats, int64_t n_cl, int D, double ridge, double *__restrict__ ld, int32_t *__restrict__ bad) {
    const int64_t cl = (int64_t)blockIdx.x * DIAR_WAVES + (threadIdx.x >> 6);
    if (cl >= n_cl) return;                                          // (whole wave)
    bool ok;
    const double v = wave_logdet<DB>(cl_stats + cl * diar_stat_len(D), nullptr, D, ridge, ok);
    if ((threadIdx.x & 63) == 0) {
        ld[cl] = v;
        bad[cl] = ok ? 0 : 1;
    }
}

template <int DB>
__global__ __launch_bounds__(64 * DIAR_WAVES)
void diar_pairs_kernel(const double *__restrict__ cl_stats, const int64_t *__restrict__ cl_off, const int64_t *__restrict__ tab_off,
                       const double *__restrict__ ld, const int32_t *__restrict__ bad, int D, double ridge, double pen, double *__restrict__ tab) {
    const int g = blockIdx.y;
    const int64_t c0 = cl_off[g], n = cl_off[g + 1] - c0;
    const int64_t p = (int64_t)blockIdx.x * DIAR_WAVES + (threadIdx.x >> 6);
    if (p >= n * (n - 1) / 2) return;                                // (whole wave)
    int64_t i, j;
    diar_pair_of(n, p, i, j);                                        // i < j < n (diar_plan.hpp)
    const int P = diar_stat_len(D);
    const double *sa = cl_stats + (c0 + i) * P, *sb = cl_stats + (c0 + j) * P;
    bool ok;
    const double ld_ab = wave_logdet<DB>(sa, sb, D, ridge, ok);
    if ((threadIdx.x & 63) == 0) {
        const bool good = ok && !bad[c0 + i] && !bad[c0 + j];
        tab[tab_off[g] + i * n + j] = good ? delta_bic(sa[0], sb[0], ld_ab, ld[c0 + i], ld[c0 + j], pen) : (double)INFINITY;
    }
}

// ---- the merge loop ----

__global__ __launch_bounds__(DIAR_STATS_WG)
void ahc_argmin_kernel(const double *__restrict__ tab, const int64_t *__restrict__ tab_off, const int64_t *__restrict__ cl_off,
                       const int32_t *__restrict__ alive, const int32_t *__restrict__ state, double *__restrict__ part_v,
                       int32_t *__restrict__ part_r) {
    __shared__ double red_v[DIAR_STATS_WG / 64];
    __shared__ int red_r[DIAR_STATS_WG / 64];
    const int g = blockIdx.y, tid = threadIdx.x;
    if (state[g * ST_LEN + ST_STOP]) return;                         // (the whole workgroup)
    const int64_t c0 = cl_off[g], n = cl_off[g + 1] - c0;
    const int32_t *al = alive + c0;
    const double *t = tab + tab_off[g];
    double bv = -INFINITY;
    int br = INT_MAX;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        if (!al[i]) continue;
        for (int64_t j = i + 1 + tid; j < n; j += DIAR_STATS_WG)
            if (al[j]) take_first_max(bv, br, -t[i * n + j], (int)(i * n + j));
    }
    wave_first_max_f64(bv, br);
    if ((tid & 63) == 0) {
        red_v[tid >> 6] = bv;
        red_r[tid >> 6] = br;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < DIAR_STATS_WG / 64; w++) take_first_max(bv, br, red_v[w], red_r[w]);
        part_v[g * DIAR_ARGMIN_BLOCKS + blockIdx.x] = bv;
        part_r[g * DIAR_ARGMIN_BLOCKS + blockIdx.x] = br;
    }
}

// DB > 0: the statistics' mode (merge the statistics, ld_i again); DB = 0: the matrix mode (merge the sizes).
template <int DB>
__global__ __launch_bounds__(DIAR_STATS_WG)
void ahc_merge_kernel(const double *__restrict__ part_v, const int32_t *__restrict__ part_r, int nb, const int64_t *__restrict__ cl_off,
                      int32_t *__restrict__ alive, int32_t *__restrict__ state, double *__restrict__ stats, double *__restrict__ ld,
                      int32_t *__restrict__ bad, int32_t *__restrict__ cnt, int32_t *__restrict__ merge_i, int32_t *__restrict__ merge_j,
                      double *__restrict__ merge_d, int D, double ridge, double threshold, int k_min, int k_max) {
    __shared__ double red_v[DIAR_STATS_WG / 64];
    __shared__ int red_r[DIAR_STATS_WG / 64];
    const int g = blockIdx.x, tid = threadIdx.x;
    int32_t *st = state + g * ST_LEN;
    // every lane reads the state before the barrier below; lane 0 writes it behind it
    const int stopped = st[ST_STOP], live = st[ST_LIVE], taken = st[ST_MERGES];
    if (stopped) return;                                             // (the whole workgroup)
    const int64_t c0 = cl_off[g], n = cl_off[g + 1] - c0;
    double bv = -INFINITY;
    int br = INT_MAX;
    for (int b = tid; b < nb; b += DIAR_STATS_WG) take_first_max(bv, br, part_v[g * DIAR_ARGMIN_BLOCKS + b], part_r[g * DIAR_ARGMIN_BLOCKS + b]);
    wave_first_max_f64(bv, br);
    if ((tid & 63) == 0) {
        red_v[tid >> 6] = bv;
        red_r[tid >> 6] = br;
    }
    __syncthreads();
    bv = red_v[0];
    br = red_r[0];
    for (int w = 1; w < DIAR_STATS_WG / 64; w++) take_first_max(bv, br, red_v[w], red_r[w]);
    const double d = -bv;
    const bool go = br != INT_MAX && d != (double)INFINITY && ((k_max > 0 && live > k_max) || (live > k_min && d < threshold));
    if (!go) {
        if (tid == 0) {
            st[ST_STOP] = 1;
            st[ST_I] = -1;
        }
        return;
    }
    const int64_t i = br / n, j = br - i * n;                        // (i < j < n: the rank of a table entry the argmin kernel read)
    if (tid == 0) {
        merge_i[c0 + taken] = (int32_t)i;
        merge_j[c0 + taken] = (int32_t)j;
        merge_d[c0 + taken] = d;
        st[ST_MERGES] = taken + 1;
        st[ST_LIVE] = live - 1;
        st[ST_I] = (int32_t)i;
        st[ST_J] = (int32_t)j;
        alive[c0 + j] = 0;
    }
    if constexpr (DB > 0) {
        const int P = diar_stat_len(D);
        double *si = stats + (c0 + i) * P;
        const double *sj = stats + (c0 + j) * P;
        for (int e = tid; e < P; e += DIAR_STATS_WG) si[e] = si[e] + sj[e];
        __syncthreads();                                             // the merged statistics are visible to wave 0
        if (tid < 64) {
            bool ok;
            const double v = wave_logdet<DB>(si, nullptr, D, ridge, ok);
            if (tid == 0) {
                ld[c0 + i] = v;
                if (!ok) bad[c0 + i] = 1;
            }
        }
    } else {
        if (tid == 0) {
            const int ci = cnt[c0 + i], cj = cnt[c0 + j];
            st[ST_CI] = ci;                                          // the sizes the row update weighs with
            st[ST_CJ] = cj;
            cnt[c0 + i] = ci + cj;
        }
    }
}

template <int DB>
__global__ __launch_bounds__(64 * DIAR_WAVES)
void diar_row_kernel(const int32_t *__restrict__ state, const int64_t *__restrict__ cl_off, const int64_t *__restrict__ tab_off,
                     const int32_t *__restrict__ alive, const int32_t *__restrict__ bad, const double *__restrict__ stats,
                     const double *__restrict__ ld, int D, double ridge, double pen, double *__restrict__ tab) {
    const int g = blockIdx.y;
    const int32_t *st = state + g * ST_LEN;
    if (st[ST_STOP]) return;
    const int64_t i = st[ST_I];
    if (i < 0) return;
    const int64_t c0 = cl_off[g], n = cl_off[g + 1] - c0;
    const int64_t k = (int64_t)blockIdx.x * DIAR_WAVES + (threadIdx.x >> 6);
    if (k >= n || k == i || !alive[c0 + k]) return;                  // (whole wave)
    const int P = diar_stat_len(D);
    const double *sa = stats + (c0 + i) * P, *sb = stats + (c0 + k) * P;
    bool ok;
    const double ld_ab = wave_logdet<DB>(sa, sb, D, ridge, ok);
    if ((threadIdx.x & 63) == 0) {
        const bool good = ok && !bad[c0 + i] && !bad[c0 + k];
        const int64_t lo = min(i, k), hi = max(i, k);
        tab[tab_off[g] + lo * n + hi] = good ? delta_bic(sa[0], sb[0], ld_ab, ld[c0 + i], ld[c0 + k], pen) : (double)INFINITY;
    }
}

// Lance-Williams: d(i u j, k) from d(i, k) and d(j, k); only entries (lo, hi), lo < hi, of the table are used.
__global__ __launch_bounds__(DIAR_STATS_WG)
void ahc_row_matrix_kernel(const int32_t *__restrict__ state, int64_t n, const int32_t *__restrict__ alive, int linkage, double *__restrict__ tab) {
    if (state[ST_STOP]) return;
    const int64_t i = state[ST_I], j = state[ST_J];
    if (i < 0) return;
    const int64_t k = (int64_t)blockIdx.x * DIAR_STATS_WG + threadIdx.x;
    if (k >= n || k == i || k == j || !alive[k]) return;
    const double dik = tab[min(i, k) * n + max(i, k)], djk = tab[min(j, k) * n + max(j, k)];
    double v;
    if (linkage == AHC_AVERAGE) {
        const double ci = (double)state[ST_CI], cj = (double)state[ST_CJ];
        v = (ci * dik + cj * djk) / (ci + cj);
    } else if (linkage == AHC_COMPLETE) {
        v = dik >= djk ? dik : djk;
    } else {
        v = dik <= djk ? dik : djk;
    }
    tab[min(i, k) * n + max(i, k)] = v;
}

__global__ __launch_bounds__(64)
void ahc_all_stopped_kernel(const int32_t *__restrict__ state, int G, int32_t *__restrict__ word) {
    if (threadIdx.x != 0) return;
    int all = 1;
    for (int g = 0; g < G; g++) all = all && state[g * ST_LEN + ST_STOP];
    word[0] = all;
}

// ---- host ----

struct DiarWs {
    DevBuf<double> seg_stats, cl_stats, ld, tab, c, part_v, merge_d;
    DevBuf<int32_t> seg_rec, bnd_rec, cl_rec, kept, alive, bad, cnt, state, part_r, merge_i, merge_j, word;
    DevBuf<int64_t> frame_off, seg_off, bnd_off, cl_off, tab_off, init_off;
    PinnedBuf<int32_t> h_word;
};

std::atomic<long> &diar_scratch_option() {
    static std::atomic<long> v{(long)(DIAR_DEFAULT_SCRATCH >> 20)};
    return v;
}

#define DIAR_BUCKETS(D, CALL)                       \
    do {                                            \
        switch (diar_bucket(D)) {                   \
            case 16: { constexpr int DB = 16; CALL; } break;    \
            case 32: { constexpr int DB = 32; CALL; } break;    \
            case 48: { constexpr int DB = 48; CALL; } break;    \
            default: { constexpr int DB = 64; CALL; } break;    \
        }                                           \
    } while (0)

double bic_penalty(int D, double lambda) { return lambda * 0.5 * (double)(D + diar_tri(D)); }

// the base segments of recordings [u0, u1): tables up, the statistics kernel.  Returns the group's segment offsets.
std::vector<int64_t> launch_stats(DiarWs &w, SRBatch &feat, int u0, int u1, int L) {
    const int G = u1 - u0, D = feat.dim;
    std::vector<int64_t> seg_off((size_t)G + 1, 0), frame_off((size_t)G + 1);
    for (int g = 0; g <= G; g++) frame_off[(size_t)g] = feat.offsets[(size_t)(u0 + g)];
    for (int g = 0; g < G; g++) seg_off[(size_t)g + 1] = seg_off[(size_t)g] + diar_segments(frame_off[(size_t)g + 1] - frame_off[(size_t)g], L);
    const int64_t n_seg = seg_off[(size_t)G];
    if (n_seg > INT32_MAX / 2) fail("diarisation: %lld base segments in one group (at most 2^30: a longer L)", (long long)n_seg);
    std::vector<int32_t> seg_rec((size_t)n_seg);
    for (int g = 0; g < G; g++)
        for (int64_t s = seg_off[(size_t)g]; s < seg_off[(size_t)g + 1]; s++) seg_rec[(size_t)s] = g;
    w.frame_off.upload(frame_off.data(), frame_off.size());
    w.seg_off.upload(seg_off.data(), seg_off.size());
    w.seg_stats.ensure((size_t)std::max<int64_t>(1, n_seg) * diar_stat_len(D));
    if (n_seg > 0) {
        w.seg_rec.upload(seg_rec.data(), seg_rec.size());
        ScopedKernelTimer tm(T_CMVN);
        hipLaunchKernelGGL(diar_stats_kernel, dim3((unsigned)n_seg), dim3(DIAR_STATS_WG), (size_t)DIAR_STATS_CHUNK * D * sizeof(float), ctx().stream,
                           feat.data.p, w.frame_off.p, w.seg_rec.p, w.seg_off.p, D, (int64_t)L, w.seg_stats.p);
        SR_HIP(hipGetLastError());
    }
    sync_stream();                                                   // (the host tables outlive their uploads)
    return seg_off;
}

// The merge loop over the G recordings whose tables, alive flags and state sit in the workspace.  DB_D: the statistics' dimension
// (the matrix mode passes 0).
void run_merge_loop(DiarWs &w, int G, int64_t n_max, int D, int linkage, double ridge, double pen, double threshold, int k_min, int k_max) {
    hipStream_t st = ctx().stream;
    const int nb = diar_argmin_blocks(n_max);
    w.part_v.ensure((size_t)G * DIAR_ARGMIN_BLOCKS);
    w.part_r.ensure((size_t)G * DIAR_ARGMIN_BLOCKS);
    w.word.ensure(1);
    w.h_word.ensure(1);
    const int64_t max_steps = std::max<int64_t>(0, n_max - 1);
    for (int64_t step = 0; step < max_steps; step++) {
        {
            ScopedKernelTimer tm(T_ESTEP);
            hipLaunchKernelGGL(ahc_argmin_kernel, dim3((unsigned)nb, (unsigned)G), dim3(DIAR_STATS_WG), 0, st, w.tab.p, w.tab_off.p, w.cl_off.p,
                               w.alive.p, w.state.p, w.part_v.p, w.part_r.p);
            if (D > 0)
                DIAR_BUCKETS(D, hipLaunchKernelGGL((ahc_merge_kernel<DB>), dim3((unsigned)G), dim3(DIAR_STATS_WG), 0, st, w.part_v.p, w.part_r.p, nb,
                                                   w.cl_off.p, w.alive.p, w.state.p, w.cl_stats.p, w.ld.p, w.bad.p, (int32_t *)nullptr, w.merge_i.p,
                                                   w.merge_j.p, w.merge_d.p, D, ridge, threshold, k_min, k_max));
            else
                hipLaunchKernelGGL((ahc_merge_kernel<0>), dim3((unsigned)G), dim3(DIAR_STATS_WG), 0, st, w.part_v.p, w.part_r.p, nb, w.cl_off.p,
                                   w.alive.p, w.state.p, (double *)nullptr, (double *)nullptr, (int32_t *)nullptr, w.cnt.p, w.merge_i.p, w.merge_j.p,
                                   w.merge_d.p, 0, 0.0, threshold, k_min, k_max);
        }
        {
            ScopedKernelTimer tm(T_SCORE_REF);
            if (D > 0)
                DIAR_BUCKETS(D, hipLaunchKernelGGL((diar_row_kernel<DB>), dim3((unsigned)((n_max + DIAR_WAVES - 1) / DIAR_WAVES), (unsigned)G),
                                                   dim3(64 * DIAR_WAVES), 0, st, w.state.p, w.cl_off.p, w.tab_off.p, w.alive.p, w.bad.p, w.cl_stats.p,
                                                   w.ld.p, D, ridge, pen, w.tab.p));
            else
                hipLaunchKernelGGL(ahc_row_matrix_kernel, dim3((unsigned)((n_max + DIAR_STATS_WG - 1) / DIAR_STATS_WG)), dim3(DIAR_STATS_WG), 0, st,
                                   w.state.p, n_max, w.alive.p, linkage, w.tab.p);
        }
        if ((step + 1) % DIAR_CADENCE == 0 && step + 1 < max_steps) {
            hipLaunchKernelGGL(ahc_all_stopped_kernel, dim3(1), dim3(64), 0, st, w.state.p, G, w.word.p);
            SR_HIP(hipGetLastError());
            SR_HIP(hipMemcpyAsync(w.h_word.p, w.word.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            sync_stream();
            if (w.h_word.p[0]) break;
        }
    }
    SR_HIP(hipGetLastError());
}

void init_loop_state(DiarWs &w, const std::vector<int64_t> &cl_off, int G) {
    const int64_t n_cl = cl_off[(size_t)G];
    std::vector<int32_t> state((size_t)G * ST_LEN, 0), ones((size_t)std::max<int64_t>(1, n_cl), 1);
    for (int g = 0; g < G; g++) {
        state[(size_t)g * ST_LEN + ST_LIVE] = (int32_t)(cl_off[(size_t)g + 1] - cl_off[(size_t)g]);
        state[(size_t)g * ST_LEN + ST_I] = -1;
    }
    w.state.upload(state.data(), state.size());
    w.alive.upload(ones.data(), ones.size());
    w.cnt.upload(ones.data(), ones.size());
    w.merge_i.ensure(ones.size());
    w.merge_j.ensure(ones.size());
    w.merge_d.ensure(ones.size());
    sync_stream();
}

void run_group(DiarWs &w, SRBatch &feat, int u0, int u1, const DiarParams &prm, DiarResult &out) {
    hipStream_t st = ctx().stream;
    const int G = u1 - u0, D = feat.dim, P = diar_stat_len(D);
    const double pen = bic_penalty(D, prm.lambda);
    const std::vector<int64_t> seg_off = launch_stats(w, feat, u0, u1, prm.L);
    // the boundaries between base segments
    std::vector<int64_t> bnd_off((size_t)G + 1, 0);
    for (int g = 0; g < G; g++) bnd_off[(size_t)g + 1] = bnd_off[(size_t)g] + std::max<int64_t>(0, seg_off[(size_t)g + 1] - seg_off[(size_t)g] - 1);
    const int64_t n_bnd = bnd_off[(size_t)G];
    std::vector<int32_t> kept((size_t)n_bnd, 1);                     // uniform: every boundary is kept
    if (prm.change == DIAR_CHANGE_BIC && n_bnd > 0) {
        std::vector<int32_t> bnd_rec((size_t)n_bnd);
        for (int g = 0; g < G; g++)
            for (int64_t b = bnd_off[(size_t)g]; b < bnd_off[(size_t)g + 1]; b++) bnd_rec[(size_t)b] = g;
        w.bnd_rec.upload(bnd_rec.data(), bnd_rec.size());
        w.bnd_off.upload(bnd_off.data(), bnd_off.size());
        w.c.ensure((size_t)n_bnd);
        w.kept.ensure((size_t)n_bnd);
        {
            ScopedKernelTimer tm(T_SCORE_REF);
            DIAR_BUCKETS(D, hipLaunchKernelGGL((diar_change_kernel<DB>), dim3((unsigned)n_bnd), dim3(64), (size_t)2 * P * sizeof(double), st,
                                               w.seg_stats.p, w.bnd_rec.p, w.bnd_off.p, w.seg_off.p, D, (int64_t)prm.m, prm.ridge, pen, w.c.p));
            hipLaunchKernelGGL(diar_peak_kernel, dim3((unsigned)((n_bnd + 63) / 64)), dim3(64), 0, st, w.c.p, w.bnd_rec.p, w.bnd_off.p, n_bnd,
                               (int64_t)prm.m, w.kept.p);
        }
        SR_HIP(hipGetLastError());
        w.kept.download(kept.data(), (size_t)n_bnd);
        sync_stream();
    }
    // the initial clusters: the runs of base segments between kept boundaries
    std::vector<int64_t> cl_off((size_t)G + 1, 0), tab_off((size_t)G + 1, 0), init_off;
    int64_t n_max = 0;
    for (int g = 0; g < G; g++) {
        const int64_t ns = seg_off[(size_t)g + 1] - seg_off[(size_t)g];
        int64_t ni = 0;
        if (ns > 0) {
            init_off.push_back(0);
            for (int64_t b = 1; b < ns; b++)
                if (kept[(size_t)(bnd_off[(size_t)g] + b - 1)]) {
                    init_off.push_back(b);
                    ni++;
                }
            init_off.push_back(ns);
            ni++;
        } else {
            init_off.push_back(0);
        }
        if (ni > DIAR_MAX_INIT)
            fail("diarisation: recording %d has %lld initial clusters, a recording takes at most %d; use longer segments (a larger L)", u0 + g,
                 (long long)ni, DIAR_MAX_INIT);
        cl_off[(size_t)g + 1] = cl_off[(size_t)g] + ni;
        tab_off[(size_t)g + 1] = tab_off[(size_t)g] + ni * ni;
        n_max = std::max(n_max, ni);
    }
    const int64_t n_cl = cl_off[(size_t)G];
    std::vector<int32_t> cl_rec((size_t)n_cl);
    for (int g = 0; g < G; g++)
        for (int64_t c = cl_off[(size_t)g]; c < cl_off[(size_t)g + 1]; c++) cl_rec[(size_t)c] = g;
    std::vector<int32_t> bad0((size_t)n_cl, 0), mi((size_t)n_cl, 0), mj((size_t)n_cl, 0), state((size_t)G * ST_LEN, 0);
    std::vector<double> md((size_t)n_cl, 0.0);
    if (n_cl > 0) {
        w.cl_off.upload(cl_off.data(), cl_off.size());
        w.tab_off.upload(tab_off.data(), tab_off.size());
        w.init_off.upload(init_off.data(), init_off.size());
        w.cl_rec.upload(cl_rec.data(), cl_rec.size());
        w.cl_stats.ensure((size_t)n_cl * P);
        w.ld.ensure((size_t)n_cl);
        w.bad.ensure((size_t)n_cl);
        w.tab.ensure((size_t)tab_off[(size_t)G]);
        init_loop_state(w, cl_off, G);
        {
            ScopedKernelTimer tm(T_CMVN);
            hipLaunchKernelGGL(diar_gather_kernel, dim3((unsigned)n_cl), dim3(DIAR_STATS_WG), 0, st, w.seg_stats.p, w.cl_rec.p, w.cl_off.p, w.seg_off.p,
                               w.init_off.p, D, w.cl_stats.p);
        }
        {
            ScopedKernelTimer tm(T_SCORE_REF);
            DIAR_BUCKETS(D, hipLaunchKernelGGL((diar_ld_kernel<DB>), dim3((unsigned)((n_cl + DIAR_WAVES - 1) / DIAR_WAVES)), dim3(64 * DIAR_WAVES), 0, st,
                                               w.cl_stats.p, n_cl, D, prm.ridge, w.ld.p, w.bad.p));
            if (n_max > 1)
                DIAR_BUCKETS(D, hipLaunchKernelGGL((diar_pairs_kernel<DB>), dim3((unsigned)((n_max * (n_max - 1) / 2 + DIAR_WAVES - 1) / DIAR_WAVES), (unsigned)G),
                                                   dim3(64 * DIAR_WAVES), 0, st, w.cl_stats.p, w.cl_off.p, w.tab_off.p, w.ld.p, w.bad.p, D, prm.ridge,
                                                   pen, w.tab.p));
        }
        SR_HIP(hipGetLastError());
        w.bad.download(bad0.data(), (size_t)n_cl);                   // the clusters that failed on their own, before any merge
        sync_stream();
        run_merge_loop(w, G, n_max, D, 0, prm.ridge, pen, prm.threshold, prm.k_min, prm.k_max);
        w.merge_i.download(mi.data(), (size_t)n_cl);
        w.merge_j.download(mj.data(), (size_t)n_cl);
        w.merge_d.download(md.data(), (size_t)n_cl);
        w.state.download(state.data(), state.size());
        sync_stream();
    }
    // home: the group's part of the batch's results
    for (int g = 0; g < G; g++) {
        const int64_t c0 = cl_off[(size_t)g], ni = cl_off[(size_t)g + 1] - c0;
        const int64_t taken = n_cl > 0 ? state[(size_t)g * ST_LEN + ST_MERGES] : 0;
        for (int64_t t = taken; t < ni; t++) {                       // (behind the log: nothing was written)
            mi[(size_t)(c0 + t)] = mj[(size_t)(c0 + t)] = 0;
            md[(size_t)(c0 + t)] = 0.0;
        }
        const size_t at = out.label.size();
        out.init_cl_off.push_back(out.init_cl_off.back() + ni);
        for (int64_t k = 0; k <= ni; k++) out.init_off.push_back(init_off[(size_t)(c0 + g + k)]);
        out.merge_i.insert(out.merge_i.end(), mi.begin() + c0, mi.begin() + c0 + ni);
        out.merge_j.insert(out.merge_j.end(), mj.begin() + c0, mj.begin() + c0 + ni);
        out.merge_d.insert(out.merge_d.end(), md.begin() + c0, md.begin() + c0 + ni);
        out.label.resize(at + (size_t)ni);
        const int k = diar_labels(ni, mi.data() + c0, mj.data() + c0, taken, out.label.data() + at);
        if (k < 0) fail("diarisation: recording %d came back with a merge log that is not one", u0 + g);
        int64_t nf = 0;
        for (int64_t c = 0; c < ni; c++) nf += bad0[(size_t)(c0 + c)];
        out.n_merges.push_back(taken);
        out.n_clusters.push_back(k);
        out.fail.push_back(nf);
        out.n_seg.push_back(seg_off[(size_t)g + 1] - seg_off[(size_t)g]);
    }
}

DiarPlan checked_plan(SRBatch &feat, const DiarParams &prm) {
    std::vector<int64_t> lengths((size_t)feat.n_utt);
    for (int u = 0; u < feat.n_utt; u++) lengths[(size_t)u] = feat.offsets[(size_t)u + 1] - feat.offsets[(size_t)u];
    DiarPlan pl;
    std::string why;
    if (!plan_diar(feat.dim, prm, lengths.data(), feat.n_utt, (int64_t)diar_scratch_mib() << 20, pl, why)) fail("%s", why.c_str());
    return pl;
}

}  // namespace

void set_diar_scratch_mib(long v) { diar_scratch_option().store(v); }
long diar_scratch_mib() { return diar_scratch_option().load(); }

void diar_stats_batch(SRBatch &feat, int L, int64_t *seg_off_out, double *stats_out) {
    DiarParams prm;
    prm.L = L;
    const DiarPlan pl = checked_plan(feat, prm);
    ensure_device();
    auto &w = per_device<DiarWs>();
    const int P = diar_stat_len(feat.dim);
    int64_t done = 0;
    seg_off_out[0] = 0;
    for (size_t gi = 0; gi + 1 < pl.group_begin.size(); gi++) {
        const int u0 = pl.group_begin[gi], u1 = pl.group_begin[gi + 1];
        const std::vector<int64_t> seg_off = launch_stats(w, feat, u0, u1, L);
        const int64_t ns = seg_off.back();
        if (ns > 0) {
            w.seg_stats.download(stats_out + done * P, (size_t)ns * P);
            sync_stream();
        }
        for (int g = 0; g < u1 - u0; g++) seg_off_out[u0 + g + 1] = done + seg_off[(size_t)g + 1];
        done += ns;
    }
}

void diar_bic_matrix(int D, int64_t n, const double *stats, double lambda, double ridge, double *out, double *ld_out, int64_t *fail_out) {
    ensure_device();
    auto &w = per_device<DiarWs>();
    hipStream_t st = ctx().stream;
    const int P = diar_stat_len(D);
    if (fail_out) *fail_out = 0;
    if (n <= 0) return;
    const std::vector<int64_t> cl_off = {0, n}, tab_off = {0, n * n};
    std::vector<double> tab((size_t)(n * n)), ld((size_t)n);
    std::vector<int32_t> bad((size_t)n);
    w.cl_stats.upload(stats, (size_t)n * P);
    w.cl_off.upload(cl_off.data(), 2);
    w.tab_off.upload(tab_off.data(), 2);
    w.ld.ensure((size_t)n);
    w.bad.ensure((size_t)n);
    w.tab.ensure((size_t)(n * n));
    const double pen = bic_penalty(D, lambda);
    {
        ScopedKernelTimer tm(T_SCORE_REF);
        DIAR_BUCKETS(D, hipLaunchKernelGGL((diar_ld_kernel<DB>), dim3((unsigned)((n + DIAR_WAVES - 1) / DIAR_WAVES)), dim3(64 * DIAR_WAVES), 0, st,
                                           w.cl_stats.p, n, D, ridge, w.ld.p, w.bad.p));
        if (n > 1)
            DIAR_BUCKETS(D, hipLaunchKernelGGL((diar_pairs_kernel<DB>), dim3((unsigned)((n * (n - 1) / 2 + DIAR_WAVES - 1) / DIAR_WAVES), 1u), dim3(64 * DIAR_WAVES),
                                               0, st, w.cl_stats.p, w.cl_off.p, w.tab_off.p, w.ld.p, w.bad.p, D, ridge, pen, w.tab.p));
    }
    SR_HIP(hipGetLastError());
    if (n > 1) w.tab.download(tab.data(), tab.size());
    w.ld.download(ld.data(), ld.size());
    w.bad.download(bad.data(), bad.size());
    sync_stream();
    int64_t nf = 0;
    for (int64_t i = 0; i < n; i++) {
        nf += bad[(size_t)i];
        if (ld_out) ld_out[i] = bad[(size_t)i] ? (double)NAN : ld[(size_t)i];
        for (int64_t j = 0; j < n; j++) out[i * n + j] = i == j ? 0.0 : i < j ? tab[(size_t)(i * n + j)] : tab[(size_t)(j * n + i)];
    }
    if (fail_out) *fail_out = nf;
}

void diar_cluster_batch(SRBatch &feat, const DiarParams &prm, DiarResult &out) {
    const DiarPlan pl = checked_plan(feat, prm);
    ensure_device();
    auto &w = per_device<DiarWs>();
    out = DiarResult();
    out.init_cl_off.push_back(0);
    for (size_t gi = 0; gi + 1 < pl.group_begin.size(); gi++) run_group(w, feat, pl.group_begin[gi], pl.group_begin[gi + 1], prm, out);
}

void ahc_matrix(int64_t n, const double *dist, int linkage, double threshold, int k_min, int k_max, int32_t *merge_i, int32_t *merge_j,
                double *merge_d, int64_t *n_merges_out, int32_t *label_out, int64_t *n_clusters_out) {
    *n_merges_out = 0;
    *n_clusters_out = 0;
    if (n <= 0) return;
    if (ahc_matrix_bytes(n) > ((int64_t)diar_scratch_mib() << 20))
        fail("clustering: the table of %lld items takes %lld bytes, the bound is %lld; raise the option diar_scratch_mib or cluster fewer items",
             (long long)n, (long long)ahc_matrix_bytes(n), (long long)((int64_t)diar_scratch_mib() << 20));
    ensure_device();
    auto &w = per_device<DiarWs>();
    const std::vector<int64_t> cl_off = {0, n}, tab_off = {0, n * n};
    w.tab.upload(dist, (size_t)(n * n));
    w.cl_off.upload(cl_off.data(), 2);
    w.tab_off.upload(tab_off.data(), 2);
    init_loop_state(w, cl_off, 1);
    run_merge_loop(w, 1, n, 0, linkage, 0.0, 0.0, threshold, k_min, k_max);
    std::vector<int32_t> state(ST_LEN, 0);
    w.state.download(state.data(), state.size());
    if (n > 1) {
        w.merge_i.download(merge_i, (size_t)(n - 1));
        w.merge_j.download(merge_j, (size_t)(n - 1));
        w.merge_d.download(merge_d, (size_t)(n - 1));
    }
    sync_stream();
    const int64_t taken = state[ST_MERGES];
    for (int64_t t = taken; t < n - 1; t++) {                        // (behind the log: nothing was written)
        merge_i[t] = merge_j[t] = 0;
        merge_d[t] = 0.0;
    }
    const int k = diar_labels(n, merge_i, merge_j, taken, label_out);
    if (k < 0) fail("clustering: the merge log that came back is not one");
    *n_merges_out = taken;
    *n_clusters_out = k;
}

}  // namespace sr
