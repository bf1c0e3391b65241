// em_f64_dev.hpp -- the per-workgroup bodies of the float64 iteration engine (em_f64.hip: one fit per launch) as __device__
// functions, so that the batched MAP enrolment (map_batch.hip: a set of speakers per launch, the workgroup's speaker and local tile
// read from a table) runs the SAME element arithmetic: two restatements could be contracted into fused multiply-adds differently, and
// the batched fit promises the single fit's bits.  A body takes the fit's (or the speaker's) view `a` and the tile / chunk / mixture
// block / element the workgroup or thread stands for; it never reads blockIdx itself.
#pragma once

#include "map_plan.hpp"
#include "wave_ops.hpp"

#include <hip/hip_runtime.h>

namespace sr {

constexpr double E64_MINLOG = -708.396418532264, E64_BAND = -598.0, E64_LN_1E_15 = -34.538776394910684, E64_SQRT_2_PI = 2.5066282746310002;

struct E64Args {
    const float *X;
    int n, n_pad, dim, K, n_chunks, n_kb, map;
    double *w, *mu, *sg, *h, *c;       // the model on the device: [K], [K][D], [K][D], 1 / (2 sigma^2), ln w - sum ln(sqrt(2 pi) sigma)
    const double *ubm_mu;
    double *L;                         // [n_kb * 64][n_pad]
    double *mb, *sb;                   // [n_kb][n_pad]
    double *llf;                       // [n_pad]  a frame's total; +inf where it carries no responsibility
    double *partial;                   // [n_chunks][K][2 D + 1]
    double *llpart;                    // [n_chunks][2]
    double *head;                      // [2]
    double min_sigma, relevance;
};

__device__ __forceinline__ void e64_derive_body(const E64Args &a, int what /* 1: h, 2: c, 3: both */, int i) {
    const int D = a.dim;
    if ((what & 1) && i < a.K * D) a.h[i] = 0.5 / (a.sg[i] * a.sg[i]);
    if ((what & 2) && i < a.K) {
        double c = a.w[i] > 0.0 ? log(a.w[i]) : -__builtin_inf();
        for (int d = 0; d < D; d++) c -= log(E64_SQRT_2_PI * a.sg[i * D + d]);
        a.c[i] = c;
    }
}

__device__ __forceinline__ void e64_density_body(const E64Args &a, double *e64_lds, int tile, int kb) {
    const int D = a.dim, XS = D + 1;
    double2 *s_p = reinterpret_cast<double2 *>(e64_lds);          // [64][D] {mean, 1 / (2 sigma^2)}: one 16-byte read per pair
    double *s_c = e64_lds + 2 * E64_KB * D;          // [64]
    double *s_pm = s_c + E64_KB;                     // [4][128]
    float *s_x = reinterpret_cast<float *>(s_pm + 4 * E64_DFR);    // [128][D + 1]
    const int tid = threadIdx.x, f = tid & 63, g = tid >> 6;
    const int f0 = tile * E64_DFR, k0 = kb * E64_KB;
    for (int i = tid; i < E64_KB * D; i += E64_THREADS) {
        const int k = k0 + i / D;
        s_p[i] = k < a.K ? make_double2(a.mu[(size_t)k0 * D + i], a.h[(size_t)k0 * D + i]) : make_double2(0.0, 0.0);
    }
    if (tid < E64_KB) s_c[tid] = k0 + tid < a.K ? a.c[k0 + tid] : -__builtin_inf();
    for (int i = tid; i < E64_DFR * D; i += E64_THREADS) {
        const int fr = i / D, d = i - fr * D;
        s_x[fr * XS + d] = f0 + fr < a.n ? a.X[(size_t)(f0 + fr) * D + d] : 0.f;
    }
    __syncthreads();
    // frames f and f + 64 against this wave's 16 mixtures: a parameter pair read from LDS serves two frames (the reads, not the
    // arithmetic, bound this kernel: 2048 x 3000 x 39 takes 100 us with a read per value, 68-75 with a mixture's {mean, h} as ONE
    // 16-byte read; the loop 60 of them, the exponentials 7, the stores of L 6 -- parts switched off, profiles/r06_em_f64.txt)
    double lp0[E64_PER], lp1[E64_PER];
#pragma unroll
    for (int j = 0; j < E64_PER; j++) lp0[j] = lp1[j] = s_c[g * E64_PER + j];
    for (int d = 0; d < D; d++) {
        const double x0 = (double)s_x[f * XS + d], x1 = (double)s_x[(f + 64) * XS + d];
#pragma unroll
        for (int j = 0; j < E64_PER; j++) {
            const double2 ph = s_p[(g * E64_PER + j) * D + d];
            const double mu = ph.x, h = ph.y;
            const double t0 = x0 - mu, t1 = x1 - mu;
            lp0[j] = fma(-(t0 * t0), h, lp0[j]);
            lp1[j] = fma(-(t1 * t1), h, lp1[j]);
        }
    }
    double pm0 = -__builtin_inf(), pm1 = -__builtin_inf();
#pragma unroll
    for (int j = 0; j < E64_PER; j++) {
        double *row = a.L + (size_t)(k0 + g * E64_PER + j) * a.n_pad + f0 + f;
        row[0] = lp0[j];
        row[64] = lp1[j];
        if (lp0[j] >= E64_MINLOG) pm0 = fmax(pm0, lp0[j]);
        if (lp1[j] >= E64_MINLOG) pm1 = fmax(pm1, lp1[j]);
    }
    s_pm[g * E64_DFR + f] = pm0;
    s_pm[g * E64_DFR + f + 64] = pm1;
    __syncthreads();
    double m[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int ff = f + 64 * q;
        m[q] = fmax(fmax(s_pm[ff], s_pm[E64_DFR + ff]), fmax(s_pm[2 * E64_DFR + ff], s_pm[3 * E64_DFR + ff]));
    }
    __syncthreads();
    double ps0 = 0.0, ps1 = 0.0;
    if (m[0] >= E64_MINLOG) {
#pragma unroll
        for (int j = 0; j < E64_PER; j++) ps0 += lp0[j] >= E64_MINLOG ? exp(lp0[j] - m[0]) : 0.0;
    }
    if (m[1] >= E64_MINLOG) {
#pragma unroll
        for (int j = 0; j < E64_PER; j++) ps1 += lp1[j] >= E64_MINLOG ? exp(lp1[j] - m[1]) : 0.0;
    }
    s_pm[g * E64_DFR + f] = ps0;
    s_pm[g * E64_DFR + f + 64] = ps1;
    __syncthreads();
    if (g < 2) {                                     // (wave 0: frames f, wave 1: frames f + 64)
        const int ff = f + 64 * g;
        a.mb[(size_t)kb * a.n_pad + f0 + ff] = m[g];
        a.sb[(size_t)kb * a.n_pad + f0 + ff] = ((s_pm[ff] + s_pm[E64_DFR + ff]) + s_pm[2 * E64_DFR + ff]) + s_pm[3 * E64_DFR + ff];
    }
}

// A frame's total from its blocks' (maximum, sum) pairs -- four groups of threads take every fourth block each, their maxima and then
// their sums meet in LDS in group order (one thread per frame walking up to 32 blocks' exponentials in a row: 20 us per pass at 2048
// mixtures); the chunk's sum of totals (safe_log: ln 1e-15 for a frame without a surviving term) and its flag.  64 frames per workgroup.
__device__ __forceinline__ void e64_lse_body(const E64Args &a, int chunk) {
    __shared__ double s_part[4][E64_FR];
    const int f = threadIdx.x & 63, g = threadIdx.x >> 6, F = chunk * E64_FR + f;
    const bool valid = F < a.n;
    double pm = -__builtin_inf();
    for (int b = g; b < a.n_kb; b += 4) pm = fmax(pm, a.mb[(size_t)b * a.n_pad + F]);
    s_part[g][f] = pm;
    __syncthreads();
    const double m = fmax(fmax(s_part[0][f], s_part[1][f]), fmax(s_part[2][f], s_part[3][f]));
    const bool live = m >= E64_MINLOG;
    __syncthreads();
    double ps = 0.0;
    if (live)
        for (int b = g; b < a.n_kb; b += 4) {
            const double bm = a.mb[(size_t)b * a.n_pad + F];
            if (bm >= E64_MINLOG) ps += a.sb[(size_t)b * a.n_pad + F] * exp(bm - m);
        }
    s_part[g][f] = ps;
    __syncthreads();
    if (g != 0) return;
    const double s = ((s_part[0][f] + s_part[1][f]) + s_part[2][f]) + s_part[3][f];
    const double ll = live ? m + log(s) : 0.0;
    a.llf[F] = valid && live ? ll : __builtin_inf();
    const int bad = valid && ((live && m < E64_BAND) || !(s == s));
    const double t = wave_sum_f64(valid ? (live ? ll : E64_LN_1E_15) : 0.0);
    const unsigned long long any = __builtin_amdgcn_ballot_w64(bad);
    if (f == 0) {
        a.llpart[2 * chunk] = t;
        a.llpart[2 * chunk + 1] = any ? 1.0 : 0.0;
    }
}

__device__ __forceinline__ void e64_stats_body(const E64Args &a, double *e64_lds, int chunk, int kb) {
    const int D = a.dim, XS = D + 1, REC = 2 * D + 1;
    double *s_g = e64_lds;                           // [64][64]   responsibilities of the block's mixtures
    double *s_mu = s_g + E64_KB * E64_FR;            // [64][D]
    float *s_x = reinterpret_cast<float *>(s_mu + E64_KB * D);     // [64][D + 1]
    __shared__ int s_bad;
    const int tid = threadIdx.x, f = tid & 63, g = tid >> 6;
    const int f0 = chunk * E64_FR, k0 = kb * E64_KB;
    if (tid == 0) s_bad = 0;
    for (int i = tid; i < E64_KB * D; i += E64_STHREADS) s_mu[i] = k0 + i / D < a.K ? a.mu[(size_t)k0 * D + i] : 0.0;
    for (int i = tid; i < E64_FR * D; i += E64_STHREADS) {
        const int fr = i / D, d = i - fr * D;
        s_x[fr * XS + d] = f0 + fr < a.n ? a.X[(size_t)(f0 + fr) * D + d] : 0.f;
    }
    const double ll = a.llf[f0 + f];                 // (+inf: no responsibility -- exp(lp - inf) = 0)
    __syncthreads();
#pragma unroll
    for (int j = 0; j < E64_SPER; j++) {
        const int kl = g * E64_SPER + j;
        const double lp = a.L[(size_t)(k0 + kl) * a.n_pad + f0 + f];
        if (f0 + f < a.n && !(lp == lp) && k0 + kl < a.K) atomicOr(&s_bad, 1);
        s_g[kl * E64_FR + f] = lp >= E64_MINLOG ? exp(lp - ll) : 0.0;
    }
    __syncthreads();
    // sums of the block's mixtures over the chunk's frames: a (mixture, dimension) pair per thread and step, four running sums per
    // moment (frames i = q mod 4) added up in a fixed order
    const int R = E64_KB * (D + 1);
    for (int role = tid; role < R; role += E64_STHREADS) {
        const int kl = role / (D + 1), d = role - kl * (D + 1);
        if (k0 + kl >= a.K) continue;
        const double *gam = s_g + kl * E64_FR;
        double p1[4] = {0.0, 0.0, 0.0, 0.0}, p2[4] = {0.0, 0.0, 0.0, 0.0};
        double *dst = a.partial + ((size_t)chunk * a.K + k0 + kl) * REC;
        if (d < D) {
            const double mu = s_mu[kl * D + d];
            for (int i = 0; i < E64_FR; i += 4) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const double dv = (double)s_x[(i + q) * XS + d] - mu;
                    const double gd = gam[i + q] * dv;
                    p1[q] += gd;
                    p2[q] = fma(gd, dv, p2[q]);
                }
            }
            dst[d] = (p1[0] + p1[1]) + (p1[2] + p1[3]);
            dst[D + d] = (p2[0] + p2[1]) + (p2[2] + p2[3]);
        } else {
            for (int i = 0; i < E64_FR; i += 4) {
#pragma unroll
                for (int q = 0; q < 4; q++) p1[q] += gam[i + q];
            }
            dst[2 * D] = (p1[0] + p1[1]) + (p1[2] + p1[3]);
        }
    }
    if (tid == 0 && s_bad) a.llpart[2 * chunk + 1] = 1.0;       // (a NaN density: any block of the chunk raises the chunk's flag)
}

// the pass's total log-likelihood (the chunks' sums: two per lane, then the wave's fixed-order sum) and the number of flagged chunks;
// one wave, the same values in every lane
__device__ __forceinline__ void e64_head_sums(const E64Args &a, double &ll, double &b) {
    const int lane = threadIdx.x;
    double v = 0.0, bad = 0.0;
    for (int c = lane; c < a.n_chunks; c += 64) {
        v += a.llpart[2 * c];
        bad += a.llpart[2 * c + 1];
    }
    ll = wave_sum_f64(v);
    b = wave_sum_f64(bad);
}

// sums over the chunks in order + the M-step of element i = (mixture, dimension)
__device__ __forceinline__ void e64_mstep_body(const E64Args &a, int i) {
    const int D = a.dim, REC = 2 * D + 1;
    if (i >= a.K * D) return;
    const int k = i / D, d = i - k * D;
    double nk = 0.0, sd = 0.0, sdd = 0.0;
    for (int c = 0; c < a.n_chunks; c++) {                       // (the chunks in order)
        const double *p = a.partial + ((size_t)c * a.K + k) * REC;
        nk += p[2 * D];
        sd += p[d];
        sdd += p[D + d];
    }
    const bool empty = nk == 0.0;
    if (empty) nk = 1e-6;                                        // min_n_k, gmm.cc:502-509
    const double mu_old = a.mu[i];
    const double shift = sd / nk;                                // E_k[x] - mu_old
    // no responsibility at all (raw N_k 0): the reference's E_k[x] = sum g x / 1e-6 is 0, not the old mean (gmm.cc:396-412)
    const double ex = empty ? 0.0 : mu_old + shift;
    if (a.map) {                                                 // update_means, gmmubm.cc:53-74
        const double alpha = nk / (nk + a.relevance);
        a.mu[i] = alpha * ex + (1 - alpha) * a.ubm_mu[i];
    } else {                                                     // gmm.cc:396-437
        a.mu[i] = ex;
        double var = sdd / nk - shift * shift;                   // sum g (x - mu_new)^2 = sdd - N shift^2
        if (var < 0) var = 0;
        const double sg = fmax(a.min_sigma, sqrt(var));
        a.sg[i] = sg;
        a.h[i] = 0.5 / (sg * sg);
    }
}

}  // namespace sr
