// gmm_full.hip -- full-covariance GMMs: scikit-learn's GaussianMixture(covariance_type='full'), the model the reference's shipped
// CLI trains and scores (src/gui/skgmm.py:20, GaussianMixture(32) on mix_feature's 28 columns).
//
// Scoring (fp32, the hot path): lp_k(x) = c_k - 1/2 |P_k^T (x - mu_k)|^2 with c_k = ln w_k + sum_i ln P_k[i][i] - D/2 ln 2 pi.
// y = P_k^T (x - mu_k) is a matrix product: v_mfma_f32_32x32x2_f32 with A = P_k^T (rows: the output dims j, a row block of 32)
// and B = x - mu_k (32 frames as columns, two dims per step).  The frames of a wave stay in registers for the whole launch and
// every mixture's mean is subtracted on the way into the MFMA (one v_sub per MFMA: no cancellation of the expanded x P - mu P
// form in fp32).  C then holds y_j(frame) with the frame = lane & 31: |y|^2 is 16 in-lane FMAs plus one exchange between the
// lane halves, and the log-sum-exp over k runs per lane (online, in mixture order).  The model is staged in LDS a chunk of
// mixtures at a time, in the lane image the MFMA reads (one conflict-free ds_read_b32 per step, serving the wave's T frame
// tiles), and shared by the workgroup's 4 waves: 4 T 32 frames per staged copy.  The per-utterance sums are formed by a second
// kernel from the per-frame values in an order fixed by the utterance alone (lane j of a wave adds frames j, j + 64, ... of the
// utterance in float64, then a butterfly), so the bits do not depend on tiling or on the batch around the utterance.
// fullcov_finalize_kernel forms the same sums and, behind them, every utterance's argmax on the device: the serving paths (the
// fused PCM call, the serving stream, the multi-GPU predictor) bring a decision back in one copy, with no host work in between.
//
// Training (float64, the whole fit on the device; em_f64.hip's pattern): one driver, fe_fit_group, fits a group of speakers of one
// K and D in the same launches.  An iteration is eight launches -- log densities, log-sum-exp + responsibilities, the mean (lower
// bound), nk + means, the covariance sums by frame chunks, the per-mixture Cholesky + inverse (one workgroup per mixture), the
// weights, the stop rule per speaker -- and the host reads one 16-byte record per speaker.  The statistics run on the vector ALU
// in float64: at speaker size (K 32, D 28, ~5600 frames) the covariance GEMMs are 8e7 FMAs per iteration, microseconds of
// arithmetic, while a measured iteration takes ~0.4 ms (K-wide per-mixture kernels); the fp64 MFMA (D = 28
// padded to 32, the responsibility applied to an operand first) was therefore not tried.
// The kernels are the bodies below with a speaker axis; inside a speaker every sum is formed by the same threads in the same order
// whatever the group, so a speaker's bits do not depend on the speakers fitted with it.  fullgmm_fit is a group of one,
// fullgmm_fit_batch cuts its speakers into groups by workspace size ("Training").
#include "gmm_full.hpp"

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace sr {

namespace {

typedef float fc_f32x16 __attribute__((ext_vector_type(16)));
constexpr double FC_LN_2PI = 1.8378770664093453;
const char *const FC_ILL_DEFINED =
    "Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance caused by "
    "singleton or collapsed samples). Try to decrease the number of components, increase reg_covar, or scale the input data.";

// ---------------------------------------------------------------- scoring
// NS: steps of two dims the kernel is built for (16: D <= 32, one row block; 32: D <= 64, two row blocks); T: 32-frame tiles per
// wave.  KC mixtures per LDS chunk: KC * RB * NS * 64 floats = 32 KiB (four workgroups per CU).
template <int NS, int T>
__global__ __launch_bounds__(256)
void fullcov_score_kernel(const float *__restrict__ X, long n, int D, int ns, int nrb, const float *__restrict__ P,
                          const float *__restrict__ MU, const float *__restrict__ C, const int *__restrict__ kbeg, float *__restrict__ fll) {
    constexpr int RB = NS / 16, KC = 128 / (NS * RB);
    __shared__ __attribute__((aligned(16))) float sP[KC * RB * NS * 64];
    __shared__ float sMu[KC * 64];
    __shared__ float sC[KC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, col = lane & 31;
    const int m = blockIdx.y;
    const long f0 = (long)blockIdx.x * (4 * T * 32) + (long)wave * T * 32;
    float xr[T][NS];
#pragma unroll
    for (int t = 0; t < T; t++) {
        const long f = f0 + 32 * t + col;
#pragma unroll
        for (int s = 0; s < NS; s++) {
            const int d = 2 * s + half;
            xr[t][s] = (f < n && d < D) ? X[f * D + d] : 0.f;
        }
    }
    float mx[T], sm[T];
#pragma unroll
    for (int t = 0; t < T; t++) {
        mx[t] = -__builtin_inff();
        sm[t] = 0.f;
    }
    const int kb0 = kbeg[m], kb1 = kbeg[m + 1];
    const int per = nrb * ns * 64;                       // floats of one mixture's image
    for (int kc0 = kb0; kc0 < kb1; kc0 += KC) {
        const int nk = min(KC, kb1 - kc0);
        __syncthreads();
        const float4 *src = reinterpret_cast<const float4 *>(P + (size_t)kc0 * per);
        float4 *dst = reinterpret_cast<float4 *>(sP);
        for (int i = threadIdx.x; i < nk * per / 4; i += 256) dst[i] = src[i];
        for (int i = threadIdx.x; i < nk * 64; i += 256) sMu[i] = MU[(size_t)kc0 * 64 + i];
        if (threadIdx.x < nk) sC[threadIdx.x] = C[kc0 + threadIdx.x];
        __syncthreads();
        for (int j = 0; j < nk; j++) {
            float q[T];
#pragma unroll
            for (int t = 0; t < T; t++) q[t] = 0.f;
            for (int rb = 0; rb < nrb; rb++) {
                fc_f32x16 acc[T];
#pragma unroll
                for (int t = 0; t < T; t++)
#pragma unroll
                    for (int r = 0; r < 16; r++) acc[t][r] = 0.f;
                const float *pa = sP + (size_t)(j * nrb + rb) * ns * 64 + lane;
                const float *pm = sMu + j * 64 + half;
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    if (s < ns) {
                        const float a = pa[s * 64], mu = pm[2 * s];
#pragma unroll
                        for (int t = 0; t < T; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xr[t][s] - mu, acc[t], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int t = 0; t < T; t++)
#pragma unroll
                    for (int r = 0; r < 16; r++) q[t] = fmaf(acc[t][r], acc[t][r], q[t]);
            }
            const float c = sC[j];
#pragma unroll
            for (int t = 0; t < T; t++) {
                const float qq = q[t] + __shfl_xor(q[t], 32);
                const float lp = c - 0.5f * qq;
                if (lp > mx[t]) {
                    sm[t] = sm[t] * __expf(mx[t] - lp) + 1.f;
                    mx[t] = lp;
                } else if (lp > -__builtin_inff()) {
                    sm[t] += __expf(lp - mx[t]);
                }
            }
        }
    }
    if (half == 0) {
#pragma unroll
        for (int t = 0; t < T; t++) {
            const long f = f0 + 32 * t + col;
            if (f < n) fll[(size_t)m * n + f] = mx[t] + __logf(sm[t]);
        }
    }
}

// a wave per (utterance, model): lane j adds the utterance's frames j, j + 64, ... in float64, then a butterfly -- an order set by the
// utterance alone
__global__ __launch_bounds__(256)
void fullcov_sum_kernel(const float *__restrict__ fll, long n, const int64_t *__restrict__ off, int U, int S, double *__restrict__ sums) {
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (long)U * S) return;
    const int u = (int)(item / S), m = (int)(item % S);
    const int64_t b = off[u], e = off[u + 1];
    const float *row = fll + (size_t)m * n;
    double s = 0.0;
    for (int64_t i = b + lane; i < e; i += 64) s += (double)row[i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) sums[(size_t)u * S + m] = s;
}

// the first maximum in numpy's sense: (a, ia) beats (b, ib) when it is larger, NaN where b is not, or equal with a lower index
__device__ inline bool fc_better(double a, int ia, double b, int ib) {
    if (a != a) return b == b || ia < ib;
    if (b != b) return false;
    return a > b || (a == b && ia < ib);
}

// The whole decision on the device: a workgroup per utterance, its waves over the models (wave w: models w, w + FC_FIN_WAVES, ...).
// Every (utterance, model) sum is formed exactly as fullcov_sum_kernel forms it -- lane j adds frames j, j + 64, ... in float64,
// then the butterfly 32 ... 1 -- so the bits are the same on every path.  argmax[u] is the first maximum of sums[u][m] / n_u
// (float64 division, what skgmm.GMMSet.predict computes on the host); an utterance without frames gets sums 0 and argmax -1.
// `cnt` (may be null; the serving stream's voice-activity front end): utterance u is the first cnt[u] rows of its range, the rest of
// the range is padding -- the sums are those of an utterance of cnt[u] frames.  `plain` != 0: the argmax compares the sums
// themselves (a diagonal set's decision, gmm_finalize_kernel's) instead of the per-frame means.
constexpr int FC_FIN_WAVES = 8;
__global__ __launch_bounds__(64 * FC_FIN_WAVES)
void fullcov_finalize_kernel(const float *__restrict__ fll, long n, const int64_t *__restrict__ off, int U, int S,
                             double *__restrict__ sums, int *__restrict__ argmax, const int *__restrict__ cnt, int plain) {
    __shared__ double s_val[FC_FIN_WAVES];
    __shared__ int s_idx[FC_FIN_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, u = blockIdx.x;
    const int64_t b = off[u];
    const int64_t e = cnt ? min(b + (int64_t)cnt[u], off[u + 1]) : off[u + 1];
    const double n_u = plain ? 1.0 : (double)(e - b);
    double best = 0.0;
    int best_m = -1;
    for (int m = wave; m < S; m += FC_FIN_WAVES) {
        const float *row = fll + (size_t)m * n;
        double s = 0.0;
        for (int64_t i = b + lane; i < e; i += 64) s += (double)row[i];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) sums[(size_t)u * S + m] = s;
        const double v = s / n_u;
        if (best_m < 0 || fc_better(v, m, best, best_m)) {
            best = v;
            best_m = m;
        }
    }
    if (lane == 0) {
        s_val[wave] = best;
        s_idx[wave] = best_m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double bv = 0.0;
        int bm = -1;
        for (int w = 0; w < FC_FIN_WAVES; w++)
            if (s_idx[w] >= 0 && (bm < 0 || fc_better(s_val[w], s_idx[w], bv, bm))) {
                bv = s_val[w];
                bm = s_idx[w];
            }
        argmax[u] = e > b ? bm : -1;
    }
}

// ---------------------------------------------------------------- training (float64)
constexpr int FE_FB = 32;          // frames of a density workgroup
constexpr int FE_PQ = 9;           // covariance pairs per thread: 9 x 256 >= 64 x 65 / 2
static_assert(FE_PQ * 256 >= FULL_MAX_D * (FULL_MAX_D + 1) / 2, "fe_cov: 256 threads x FE_PQ slots must hold the upper triangle at FULL_MAX_D");
constexpr int FE_CB = 32;          // frames staged per covariance step

struct FeArgs {
    const double *X;                // [n][D]
    long n;
    int D, K, n_chunks, chunk;
    double *w, *logw, *mu, *prec, *logdet, *cov;     // [K], [K], [K][D], [K][D][D], [K], [K][D][D]
    double *lp;                     // [n][K]: log densities, then responsibilities
    double *lpn;                    // [n]
    double *nk;                     // [K]
    double *partial;                // [n_chunks][K][D (D + 1) / 2]
    double *head;                   // [2]: lower bound, failure flag
    double reg;
};

// weighted log densities: -1/2 (D ln 2 pi + |P^T (x - mu)|^2) + log det + ln w  (sklearn _estimate_log_gaussian_prob + _estimate_log_weights)
__device__ __forceinline__ void fe_logprob(const FeArgs &a, const unsigned bx, const int k) {
    extern __shared__ double fe_lds[];
    const int D = a.D, XS = D + 1;
    double *sP = fe_lds, *sMu = sP + D * D, *sDiff = sMu + D, *sQ = sDiff + FE_FB * XS;
    const int tid = threadIdx.x, f = tid & (FE_FB - 1), g = tid / FE_FB;
    const long f0 = (long)bx * FE_FB;
    for (int i = tid; i < D * D; i += 256) sP[i] = a.prec[(size_t)k * D * D + i];
    for (int i = tid; i < D; i += 256) sMu[i] = a.mu[(size_t)k * D + i];
    __syncthreads();
    for (int i = tid; i < FE_FB * D; i += 256) {
        const int fr = i / D, d = i - fr * D;
        sDiff[fr * XS + d] = f0 + fr < a.n ? a.X[(size_t)(f0 + fr) * D + d] - sMu[d] : 0.0;
    }
    __syncthreads();
    double q = 0.0;
    for (int j = g; j < D; j += 256 / FE_FB) {
        double y = 0.0;
        for (int i = 0; i <= j; i++) y = fma(sP[i * D + j], sDiff[f * XS + i], y);      // P upper triangular
        q = fma(y, y, q);
    }
    sQ[g * FE_FB + f] = q;
    __syncthreads();
    if (g == 0 && f0 + f < a.n) {
        double qq = 0.0;
        for (int h = 0; h < 256 / FE_FB; h++) qq += sQ[h * FE_FB + f];
        a.lp[(size_t)(f0 + f) * a.K + k] = -0.5 * (D * FC_LN_2PI + qq) + a.logdet[k] + a.logw[k];
    }
}

// a frame's log-sum-exp (max + log sum exp(a - max)) and its responsibilities exp(lp - lse), in place
__device__ __forceinline__ void fe_lse(const FeArgs &a, const unsigned bx) {
    const long f = (long)bx * 256 + threadIdx.x;
    if (f >= a.n) return;
    double *row = a.lp + (size_t)f * a.K;
    double m = -__builtin_inf();
    for (int k = 0; k < a.K; k++) m = fmax(m, row[k]);
    double s = 0.0;
    for (int k = 0; k < a.K; k++) s += exp(row[k] - m);
    const double l = log(s) + m;
    a.lpn[f] = l;
    for (int k = 0; k < a.K; k++) row[k] = exp(row[k] - l);
}

// fixed-order block sum of 256 threads' values (every thread gets the total)
__device__ double fe_block_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const double t = red[0];
    __syncthreads();
    return t;
}

__device__ __forceinline__ void fe_bound(const FeArgs &a) {
    __shared__ double red[256];
    double s = 0.0;
    for (long f = threadIdx.x; f < a.n; f += 256) s += a.lpn[f];
    s = fe_block_sum(s, red);
    if (threadIdx.x == 0) a.head[0] = s / (double)a.n;
}

// nk = sum resp + 10 eps, means = resp^T X / nk (the new means: the covariance below is formed around them)
__device__ __forceinline__ void fe_means(const FeArgs &a, const int k) {
    __shared__ double red[256];
    const int K = a.K, D = a.D;
    double s = 0.0;
    for (long f = threadIdx.x; f < a.n; f += 256) s += a.lp[(size_t)f * K + k];
    const double nk = fe_block_sum(s, red) + 10.0 * DBL_EPSILON;
    if (threadIdx.x == 0) a.nk[k] = nk;
    for (int d = 0; d < D; d++) {
        double t = 0.0;
        for (long f = threadIdx.x; f < a.n; f += 256) t = fma(a.lp[(size_t)f * K + k], a.X[(size_t)f * D + d], t);
        t = fe_block_sum(t, red);
        if (threadIdx.x == 0) a.mu[(size_t)k * D + d] = t / nk;
    }
}

// sum over a chunk of frames of resp (x - mu)(x - mu)^T, the upper triangle, pair p = (i, j >= i) in row order
__device__ __forceinline__ void fe_cov(const FeArgs &a, const int k, const int c) {
    __shared__ double sDiff[FE_CB * (FULL_MAX_D + 1)];
    __shared__ double sR[FE_CB];
    const int D = a.D, K = a.K, XS = D + 1, npairs = D * (D + 1) / 2;
    int pi[FE_PQ], pj[FE_PQ];
    double acc[FE_PQ];
#pragma unroll
    for (int q = 0; q < FE_PQ; q++) {
        int rem = threadIdx.x + 256 * q, i = 0;
        if (rem >= npairs) rem = 0;
        while (rem >= D - i) {
            rem -= D - i;
            i++;
        }
        pi[q] = i;
        pj[q] = i + rem;
        acc[q] = 0.0;
    }
    const long b = (long)c * a.chunk, e = min(a.n, b + a.chunk);
    for (long t0 = b; t0 < e; t0 += FE_CB) {
        __syncthreads();
        for (int i = threadIdx.x; i < FE_CB * D; i += 256) {
            const int fr = i / D, d = i - fr * D;
            sDiff[fr * XS + d] = t0 + fr < e ? a.X[(size_t)(t0 + fr) * D + d] - a.mu[(size_t)k * D + d] : 0.0;
        }
        if (threadIdx.x < FE_CB) sR[threadIdx.x] = t0 + threadIdx.x < e ? a.lp[(size_t)(t0 + threadIdx.x) * K + k] : 0.0;
        __syncthreads();
        const int nf = (int)min((long)FE_CB, e - t0);
#pragma unroll
        for (int q = 0; q < FE_PQ; q++) {
            if ((int)threadIdx.x + 256 * q < npairs) {
                double s = acc[q];
                for (int fr = 0; fr < nf; fr++) s = fma(sR[fr] * sDiff[fr * XS + pi[q]], sDiff[fr * XS + pj[q]], s);
                acc[q] = s;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < FE_PQ; q++) {
        const int p = threadIdx.x + 256 * q;
        if (p < npairs) a.partial[((size_t)c * K + k) * npairs + p] = acc[q];
    }
}

// covariance = chunk sums in order / nk + reg I; Cholesky L (a pivot <= 0 sets the failure flag); P = (L^-1)^T; log det = sum ln P_ii
__device__ __forceinline__ void fe_chol(const FeArgs &a, const int k) {
    __shared__ double sA[FULL_MAX_D * (FULL_MAX_D + 1)];
    __shared__ int bad;
    const int D = a.D, XS = D + 1, npairs = D * (D + 1) / 2, t = threadIdx.x;
    if (t == 0) bad = 0;
    const double nk = a.nk[k];
    double *cov = a.cov + (size_t)k * D * D, *P = a.prec + (size_t)k * D * D;
    for (int p = t; p < npairs; p += 64) {
        int rem = p, i = 0;
        while (rem >= D - i) {
            rem -= D - i;
            i++;
        }
        const int j = i + rem;
        double s = 0.0;
        for (int c = 0; c < a.n_chunks; c++) s += a.partial[((size_t)c * a.K + k) * npairs + p];
        double v = s / nk;
        if (i == j) v += a.reg;
        sA[i * XS + j] = sA[j * XS + i] = v;
        cov[i * D + j] = cov[j * D + i] = v;
    }
    __syncthreads();
    // column by column, in place (lower triangle)
    for (int j = 0; j < D; j++) {
        if (t == j) {
            double s = sA[j * XS + j];
            for (int m = 0; m < j; m++) s -= sA[j * XS + m] * sA[j * XS + m];
            if (!(s > 0.0)) bad = 1;
            sA[j * XS + j] = sqrt(s);
        }
        __syncthreads();
        if (t > j && t < D) {
            double s = sA[t * XS + j];
            for (int m = 0; m < j; m++) s -= sA[t * XS + m] * sA[j * XS + m];
            sA[t * XS + j] = s / sA[j * XS + j];
        }
        __syncthreads();
    }
    // column c of Z = L^-1 by forward substitution, written as row c of P (P = Z^T: P[c][i] = Z[i][c], upper triangular)
    if (t < D) {
        for (int i = 0; i < t; i++) P[t * D + i] = 0.0;
        for (int i = t; i < D; i++) {
            double s = i == t ? 1.0 : 0.0;
            for (int m = t; m < i; m++) s -= sA[i * XS + m] * P[t * D + m];
            P[t * D + i] = s / sA[i * XS + i];
        }
    }
    if (t == 0) {
        double ld = 0.0;
        for (int i = 0; i < D; i++) ld += log(1.0 / sA[i * XS + i]);     // (P_ii, as the substitution above forms it)
        a.logdet[k] = ld;
        if (bad) a.head[1] = 1.0;
    }
}

// mode 0 (EM): w = nk / sum nk; mode 1 (k-means initialisation): w = nk / n.  Then ln w.
__device__ __forceinline__ void fe_weights(const FeArgs &a, const int mode) {
    if (threadIdx.x != 0) return;
    double tot = 0.0;
    if (mode == 0)
        for (int k = 0; k < a.K; k++) tot += a.nk[k];
    else
        tot = (double)a.n;
    for (int k = 0; k < a.K; k++) {
        a.w[k] = a.nk[k] / tot;
        a.logw[k] = log(a.w[k]);
    }
}

// explicit initialisation: ln w and log det from the given arrays
__device__ __forceinline__ void fe_derive(const FeArgs &a) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.K) return;
    double ld = 0.0;
    for (int i = 0; i < a.D; i++) ld += log(a.prec[((size_t)k * a.D + i) * a.D + i]);
    a.logdet[k] = ld;
    a.logw[k] = log(a.w[k]);
}

// ---- a group of S models of one K and D (fe_fit_group): the bodies above with a speaker axis.  A workgroup looks its speaker
// up, leaves at once when that speaker has stopped (converged, at max_iter, or failed), and otherwise runs the body on the speaker's
// view -- the FeArgs of that speaker alone -- so inside a speaker every sum is formed by the same threads in the same order
// whatever the group.  The frame-parallel kernels (densities, log-sum-exp, covariance chunks) take (speaker, block)
// pairs from a work list built once per group: frame counts are ragged, and a grid sized by the longest speaker would mostly idle.
enum { FE_ACTIVE = 0, FE_CONVERGED = 1, FE_MAX_ITER = 2, FE_FAILED = 3 };

struct FeSpk {                      // the per-speaker table (device memory)
    long row0, n;                   // first row of the speaker in the group's X / lp / lpn, its frames
    int n_chunks, chunk;            // the covariance chunking of a fit of n frames
    long o_partial;                 // its slice of `partial`; the K-sized slices (w, logw, mu, prec, logdet, cov, nk) are s * their size
    double reg, tol, prev;          // prev: the bound of the iteration before
    int max_iter, state;            // state: FE_*
    int given, pad;                 // given: the fit starts from the handle's parameters (else from k-means labels)
};
// a speaker's launch geometry, each formula once: fe_fit_group builds the tables and work lists from them, fe_spk_bytes the group cut
inline long fe_lp_blocks(long n) { return (n + FE_FB - 1) / FE_FB; }                      // density workgroups
inline long fe_lse_blocks(long n) { return (n + 255) / 256; }                             // log-sum-exp / one-hot workgroups
inline int fe_n_chunks(long n) { return (int)std::min<long>(32, (n + 255) / 256); }       // covariance chunks
inline size_t fe_partial_len(long n, int K, int D) { return (size_t)fe_n_chunks(n) * K * (D * (D + 1) / 2); }
struct FeRec {                      // what the host reads after every iteration
    double bound;
    int state, n_iter;
};
struct FeBatch {
    const double *X;
    int D, K, S;
    double *w, *logw, *mu, *prec, *logdet, *cov, *lp, *lpn, *nk, *partial, *head;      // head: [S][2] lower bound, failure flag
    FeSpk *spk;
    FeRec *rec;
    const int2 *wl_lp, *wl_lse, *wl_cov;       // (speaker, block of FE_FB frames / block of 256 frames / covariance chunk)
    int only;                       // 0: every active speaker; the start's launches: 1 the k-means speakers only, 2 the given ones
};

__device__ __forceinline__ bool fe_stopped(const FeBatch &b, const int s) {
    const FeSpk &t = b.spk[s];
    return t.state != FE_ACTIVE || (b.only != 0 && b.only != 1 + t.given);
}

__device__ __forceinline__ FeArgs fe_view(const FeBatch &b, const int s) {
    const FeSpk &t = b.spk[s];
    const size_t K = b.K, D = b.D, row0 = t.row0;
    FeArgs a;
    a.X = b.X + row0 * D;
    a.n = t.n;
    a.D = b.D;
    a.K = b.K;
    a.n_chunks = t.n_chunks;
    a.chunk = t.chunk;
    a.w = b.w + s * K;
    a.logw = b.logw + s * K;
    a.mu = b.mu + s * K * D;
    a.prec = b.prec + s * K * D * D;
    a.logdet = b.logdet + s * K;
    a.cov = b.cov + s * K * D * D;
    a.lp = b.lp + row0 * K;
    a.lpn = b.lpn + row0;
    a.nk = b.nk + s * K;
    a.partial = b.partial + t.o_partial;
    a.head = b.head + 2 * (size_t)s;
    a.reg = t.reg;
    return a;
}

__global__ __launch_bounds__(256) void fe_logprob_batch_kernel(const FeBatch b) {
    const int2 wi = b.wl_lp[blockIdx.x];
    if (fe_stopped(b, wi.x)) return;
    fe_logprob(fe_view(b, wi.x), wi.y, blockIdx.y);
}
__global__ __launch_bounds__(256) void fe_lse_batch_kernel(const FeBatch b) {
    const int2 wi = b.wl_lse[blockIdx.x];
    if (fe_stopped(b, wi.x)) return;
    fe_lse(fe_view(b, wi.x), wi.y);
}
__global__ __launch_bounds__(256) void fe_bound_batch_kernel(const FeBatch b) {
    if (fe_stopped(b, blockIdx.x)) return;
    fe_bound(fe_view(b, blockIdx.x));
}
__global__ __launch_bounds__(256) void fe_means_batch_kernel(const FeBatch b) {
    if (fe_stopped(b, blockIdx.y)) return;
    fe_means(fe_view(b, blockIdx.y), blockIdx.x);
}
__global__ __launch_bounds__(256) void fe_cov_batch_kernel(const FeBatch b) {
    const int2 wi = b.wl_cov[blockIdx.x];
    if (fe_stopped(b, wi.x)) return;
    fe_cov(fe_view(b, wi.x), blockIdx.y, wi.y);
}
__global__ __launch_bounds__(64) void fe_chol_batch_kernel(const FeBatch b) {
    if (fe_stopped(b, blockIdx.y)) return;
    fe_chol(fe_view(b, blockIdx.y), blockIdx.x);
}
__global__ void fe_weights_batch_kernel(const FeBatch b, int mode) {
    if (fe_stopped(b, blockIdx.x)) return;
    fe_weights(fe_view(b, blockIdx.x), mode);
}
__global__ void fe_derive_batch_kernel(const FeBatch b) {
    if (fe_stopped(b, blockIdx.y)) return;
    fe_derive(fe_view(b, blockIdx.y));
}

// the k-means start: one-hot responsibilities from the labels (label: [rows of the group])
__global__ __launch_bounds__(256) void fe_onehot_batch_kernel(const FeBatch b, const int *__restrict__ label) {
    const int2 wi = b.wl_lse[blockIdx.x];
    if (fe_stopped(b, wi.x)) return;            // (launched with b.only = 1: the k-means speakers)
    const FeSpk &t = b.spk[wi.x];
    const long f = (long)wi.y * 256 + threadIdx.x;
    if (f >= t.n) return;
    const int l = label[t.row0 + f];
    double *row = b.lp + (size_t)(t.row0 + f) * b.K;
    for (int k = 0; k < b.K; k++) row[k] = k == l ? 1.0 : 0.0;
}

// The stop rule (scikit-learn's), per speaker, behind the M-step of iteration `it`: a failure flag fails the speaker; else the E-step's
// bound of this iteration against the one before decides (the M-step of the converging iteration has run, as in scikit-learn).
// it == 0: the M-step of the k-means start, which can only fail.
__global__ void fe_stop_batch_kernel(const FeBatch b, int it) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= b.S) return;
    FeSpk &t = b.spk[s];
    if (t.state != FE_ACTIVE) return;
    FeRec &r = b.rec[s];
    const double *head = b.head + 2 * (size_t)s;
    r.n_iter = it;
    if (head[1] != 0.0) {
        t.state = r.state = FE_FAILED;
        return;
    }
    if (it == 0) return;
    const double lower = head[0];
    r.bound = lower;
    if (fabs(lower - t.prev) < t.tol) t.state = r.state = FE_CONVERGED;
    else if (it >= t.max_iter) t.state = r.state = FE_MAX_ITER;
    t.prev = lower;
}

struct FeBatchWorkspace {
    DevBuf<double> X, w, logw, mu, prec, logdet, cov, lp, lpn, nk, partial, head;
    DevBuf<FeSpk> spk;
    DevBuf<FeRec> rec;
    DevBuf<int2> wl_lp, wl_lse, wl_cov;
    DevBuf<int> label;
    PinnedBuf<FeRec> h_rec;
};
// the device memory a speaker of n frames takes in it: X, lp, lpn, partial, the parameters (prec and cov, mu, w logw logdet nk),
// head; the three work lists, the k-means labels, its table entry and record
size_t fe_spk_bytes(long n, int K, int D) {
    const size_t N = (size_t)n, KD = (size_t)K * D;
    return sizeof(double) * (N * D + N * K + N + fe_partial_len(n, K, D) + 2 * KD * D + KD + 4 * K + 2) +
           sizeof(int2) * (size_t)(fe_lp_blocks(n) + fe_lse_blocks(n) + fe_n_chunks(n)) + sizeof(int) * N + sizeof(FeSpk) + sizeof(FeRec);
}

// sr_set_option("full_fit_batch_bytes"): 1 GiB holds 100 speakers of 5600 x 28 at K 32 (5.5 MB each: X, lp, lpn, the chunk sums,
// the parameters and tables) in one group with room to spare.  The workspace only grows and is kept for the next call, like the
// library's other per-device workspaces: after a batch a process holds up to this much device memory.
std::atomic<long> g_fit_batch_bytes{1L << 30};
std::atomic<long> g_fit_batch_calls{0}, g_fit_batch_speakers{0}, g_fit_batch_iterations{0};

// the argument checks of a fit (no device work); `who`: "" or "speaker s: "
void fe_check_args(const SRFullGMM &g, const double *X, long n, int D, const SRFullFitParams &p, const char *who) {
    const int K = g.K;
    if (D != g.D) fail("%sdata has %d columns, the model %d", who, D, g.D);
    if (n < K) fail("%sExpected n_samples >= n_components but got n_components = %d, n_samples = %ld", who, K, n);
    if (p.max_iter < 1) fail("%smax_iter must be >= 1 (got %d)", who, p.max_iter);
    if (p.init_given && !g.trained) fail("%sinit_given: the handle has no parameters", who);
    if (!(p.reg_covar >= 0.0) || !(p.tol >= 0.0)) fail("%stol and reg_covar must be >= 0", who);
    if (p.seed < 0) fail("%sseed must be >= 0", who);
    for (long e = 0; e < n * D; e++)
        if (!std::isfinite(X[e])) fail("%sInput X contains NaN or infinity.", who);
}

// The EM driver.  Speakers [s0, s1) of `models`: one set of launches per EM iteration, one download of the S records behind it.
// status[s]: 0 fitted, -1 failed (messages[s] says why; the handle keeps its parameters).  -> the iterations launched
long fe_fit_group(SRFullGMM *const *models, int s0, int s1, const double *X, const int64_t *row_offsets, int D, const SRFullFitParams *params,
                  SRFullFitStats *out, int *status, std::vector<std::string> &messages) {
    const int S = s1 - s0, K = models[s0]->K;
    const long r0 = (long)row_offsets[s0], rows = (long)row_offsets[s1] - r0;
    auto &ws = per_device<FeBatchWorkspace>();
    std::vector<FeSpk> spk((size_t)S);
    std::vector<FeRec> rec((size_t)S);
    std::vector<int2> wl_lp, wl_lse, wl_cov;
    long o_partial = 0;
    int max_iter = 0;
    bool any_kmeans = false, any_given = false;
    for (int i = 0; i < S; i++) {
        const SRFullFitParams &p = params[s0 + i];
        const long n = (long)(row_offsets[s0 + i + 1] - row_offsets[s0 + i]);
        FeSpk &t = spk[i];
        t.row0 = (long)row_offsets[s0 + i] - r0;
        t.n = n;
        t.n_chunks = fe_n_chunks(n);
        t.chunk = (int)((n + t.n_chunks - 1) / t.n_chunks);
        t.o_partial = o_partial;
        o_partial += (long)fe_partial_len(n, K, D);
        t.reg = p.reg_covar;
        t.tol = p.tol;
        t.prev = -std::numeric_limits<double>::infinity();
        t.max_iter = p.max_iter;
        t.state = FE_ACTIVE;
        t.given = p.init_given ? 1 : 0;
        t.pad = 0;
        rec[i] = FeRec{t.prev, FE_ACTIVE, 0};
        max_iter = std::max(max_iter, p.max_iter);
        (p.init_given ? any_given : any_kmeans) = true;
        for (long b = 0; b < fe_lp_blocks(n); b++) wl_lp.push_back(make_int2(i, (int)b));
        for (long b = 0; b < fe_lse_blocks(n); b++) wl_lse.push_back(make_int2(i, (int)b));
        for (int c = 0; c < t.n_chunks; c++) wl_cov.push_back(make_int2(i, c));
    }
    const size_t SK = (size_t)S * K;
    ws.X.upload(X + (size_t)r0 * D, (size_t)rows * D);
    ws.w.ensure(SK);
    ws.logw.ensure(SK);
    ws.mu.ensure(SK * D);
    ws.prec.ensure(SK * D * D);
    ws.logdet.ensure(SK);
    ws.cov.ensure(SK * D * D);
    ws.lp.ensure((size_t)rows * K);
    ws.lpn.ensure((size_t)rows);
    ws.nk.ensure(SK);
    ws.partial.ensure((size_t)o_partial);
    ws.head.ensure(2 * (size_t)S);
    ws.spk.upload(spk.data(), spk.size());
    ws.rec.upload(rec.data(), rec.size());
    ws.wl_lp.upload(wl_lp.data(), wl_lp.size());
    ws.wl_lse.upload(wl_lse.data(), wl_lse.size());
    ws.wl_cov.upload(wl_cov.data(), wl_cov.size());
    ws.h_rec.ensure((size_t)S);
    FeBatch b{};
    b.X = ws.X.p; b.D = D; b.K = K; b.S = S;
    b.w = ws.w.p; b.logw = ws.logw.p; b.mu = ws.mu.p; b.prec = ws.prec.p; b.logdet = ws.logdet.p; b.cov = ws.cov.p;
    b.lp = ws.lp.p; b.lpn = ws.lpn.p; b.nk = ws.nk.p; b.partial = ws.partial.p; b.head = ws.head.p;
    b.spk = ws.spk.p; b.rec = ws.rec.p; b.wl_lp = ws.wl_lp.p; b.wl_lse = ws.wl_lse.p; b.wl_cov = ws.wl_cov.p;
    hipStream_t st = ctx().stream;
    SR_HIP(hipMemsetAsync(ws.head.p, 0, 2 * (size_t)S * sizeof(double), st));
    const unsigned n_lp = (unsigned)wl_lp.size(), n_lse = (unsigned)wl_lse.size(), n_cov = (unsigned)wl_cov.size(), gs = (unsigned)((S + 63) / 64);
    const size_t lds_lp = sizeof(double) * ((size_t)D * D + D + FE_FB * (D + 1) + 256);
    auto mstep = [&](int weight_mode) {
        hipLaunchKernelGGL(fe_means_batch_kernel, dim3(K, S), dim3(256), 0, st, b);
        hipLaunchKernelGGL(fe_cov_batch_kernel, dim3(n_cov, K), dim3(256), 0, st, b);
        hipLaunchKernelGGL(fe_chol_batch_kernel, dim3(K, S), dim3(64), 0, st, b);
        hipLaunchKernelGGL(fe_weights_batch_kernel, dim3(S), dim3(64), 0, st, b, weight_mode);
    };
    auto read_records = [&]() {
        SR_HIP(hipGetLastError());
        SR_HIP(hipMemcpyAsync(ws.h_rec.p, ws.rec.p, (size_t)S * sizeof(FeRec), hipMemcpyDeviceToHost, st));
        sync_stream();
    };
    // initialisation.  The given parameters go up first (whole arrays: a k-means speaker's slice is written by its M-step
    // behind them); then the k-means speakers take their first M-step and the given ones their derive launch, each launch
    // restricted to its kind by b.only.
    std::vector<double> w0, mu0, prec0;
    std::vector<int> label;
    if (any_given) {
        w0.assign(SK, 0.0);
        mu0.assign(SK * D, 0.0);
        prec0.assign(SK * D * D, 0.0);
        for (int i = 0; i < S; i++) {
            if (!params[s0 + i].init_given) continue;
            const SRFullGMM &g = *models[s0 + i];
            std::copy(g.weights.begin(), g.weights.end(), w0.begin() + (size_t)i * K);
            std::copy(g.means.begin(), g.means.end(), mu0.begin() + (size_t)i * K * D);
            std::copy(g.prec_chol.begin(), g.prec_chol.end(), prec0.begin() + (size_t)i * K * D * D);
        }
        ws.w.upload(w0.data(), w0.size());
        ws.mu.upload(mu0.data(), mu0.size());
        ws.prec.upload(prec0.data(), prec0.size());
    }
    if (any_kmeans) {
        // sklearn's init_params='kmeans', speaker by speaker in batch order (kmeans_labels is host-sequenced)
        label.assign((size_t)rows, 0);
        std::vector<float> Xf;
        for (int i = 0; i < S; i++) {
            if (params[s0 + i].init_given) continue;
            const double *Xs = X + (size_t)row_offsets[s0 + i] * D;
            Xf.resize((size_t)spk[i].n * D);
            for (size_t e = 0; e < Xf.size(); e++) Xf[e] = (float)Xs[e];
            const std::vector<int> l = kmeans_labels(Xf.data(), spk[i].n, D, K, params[s0 + i].seed);
            std::copy(l.begin(), l.end(), label.begin() + spk[i].row0);
        }
        ws.label.upload(label.data(), label.size());
        b.only = 1;
        hipLaunchKernelGGL(fe_onehot_batch_kernel, dim3(n_lse), dim3(256), 0, st, b, ws.label.p);
        mstep(1);
        hipLaunchKernelGGL(fe_stop_batch_kernel, dim3(gs), dim3(64), 0, st, b, 0);       // (a first M-step can only fail)
    }
    if (any_given) {
        b.only = 2;
        hipLaunchKernelGGL(fe_derive_batch_kernel, dim3((K + 63) / 64, S), dim3(64), 0, st, b);
    }
    b.only = 0;
    bool active = true;
    if (any_kmeans) {
        read_records();
        active = false;
        for (int i = 0; i < S; i++) active = active || ws.h_rec.p[i].state == FE_ACTIVE;
    }
    long iterations = 0;
    for (int it = 1; active && it <= max_iter; it++) {
        hipLaunchKernelGGL(fe_logprob_batch_kernel, dim3(n_lp, K), dim3(256), lds_lp, st, b);
        hipLaunchKernelGGL(fe_lse_batch_kernel, dim3(n_lse), dim3(256), 0, st, b);
        hipLaunchKernelGGL(fe_bound_batch_kernel, dim3(S), dim3(256), 0, st, b);
        mstep(0);
        hipLaunchKernelGGL(fe_stop_batch_kernel, dim3(gs), dim3(64), 0, st, b, it);
        read_records();
        iterations++;
        active = false;
        for (int i = 0; i < S; i++) active = active || ws.h_rec.p[i].state == FE_ACTIVE;
    }
    std::vector<double> w(SK), mu(SK * D), prec(SK * D * D), cov(SK * D * D);
    ws.w.download(w.data(), w.size());
    ws.mu.download(mu.data(), mu.size());
    ws.prec.download(prec.data(), prec.size());
    ws.cov.download(cov.data(), cov.size());
    sync_stream();
    for (int i = 0; i < S; i++) {
        const FeRec &r = ws.h_rec.p[i];
        SRFullGMM &g = *models[s0 + i];
        if (r.state == FE_FAILED) {
            status[s0 + i] = -1;
            messages[s0 + i] = FC_ILL_DEFINED;
            continue;
        }
        status[s0 + i] = 0;
        out[s0 + i].converged = r.state == FE_CONVERGED ? 1 : 0;
        out[s0 + i].n_iter = r.n_iter;
        out[s0 + i].lower_bound = r.bound;
        g.weights.assign(w.begin() + (size_t)i * K, w.begin() + (size_t)(i + 1) * K);
        g.means.assign(mu.begin() + (size_t)i * K * D, mu.begin() + (size_t)(i + 1) * K * D);
        g.prec_chol.assign(prec.begin() + (size_t)i * K * D * D, prec.begin() + (size_t)(i + 1) * K * D * D);
        g.covariances.assign(cov.begin() + (size_t)i * K * D * D, cov.begin() + (size_t)(i + 1) * K * D * D);
        g.trained = true;
    }
    return iterations;
}

}  // namespace

// a group of one.  Not a fullgmm_fit_batch of one: no "speaker 0: " in a message, no counter moves, and no option cuts or refuses it
void fullgmm_fit(SRFullGMM &g, const double *X, long n, int D, const SRFullFitParams &p, SRFullFitStats &out) {
    fe_check_args(g, X, n, D, p, "");
    ensure_device();
    SRFullGMM *const model = &g;
    const int64_t row_offsets[2] = {0, n};
    int status = 0;
    std::vector<std::string> message(1);
    fe_fit_group(&model, 0, 1, X, row_offsets, D, &p, &out, &status, message);
    if (status != 0) fail("%s", message[0].c_str());
}

void set_full_fit_batch_bytes(long bytes) { g_fit_batch_bytes.store(bytes); }
long full_fit_batch_bytes() { return g_fit_batch_bytes.load(); }

void full_fit_batch_stats(long *calls, long *speakers, long *iterations) {
    if (calls) *calls = g_fit_batch_calls.load();
    if (speakers) *speakers = g_fit_batch_speakers.load();
    if (iterations) *iterations = g_fit_batch_iterations.load();
}

void fullgmm_fit_batch(SRFullGMM *const *models, int S, const double *X, const int64_t *row_offsets, int D, const SRFullFitParams *params,
                       SRFullFitStats *out, int *status, std::vector<std::string> &messages) {
    if (S < 1) fail("a batch needs at least one speaker (S = %d)", S);
    for (int s = 0; s < S; s++)
        if (!models[s]) fail("speaker %d: null model handle", s);
    if (row_offsets[0] != 0) fail("row_offsets must start at 0 (got %lld)", (long long)row_offsets[0]);
    for (int s = 0; s < S; s++)
        if (row_offsets[s + 1] < row_offsets[s])
            fail("row_offsets must not decrease (speaker %d: %lld after %lld)", s, (long long)row_offsets[s + 1], (long long)row_offsets[s]);
    const int K = models[0]->K;
    for (int s = 1; s < S; s++) {
        if (models[s]->K != K) fail("speaker %d has %d components, speaker 0 has %d: a batch is fitted with one K", s, models[s]->K, K);
        if (models[s]->D != models[0]->D) fail("speaker %d has %d dims, speaker 0 has %d: a batch is fitted with one D", s, models[s]->D, models[0]->D);
    }
    {
        std::vector<const SRFullGMM *> seen(models, models + S);
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) fail("a model handle appears twice in the batch");
    }
    char who[32];
    for (int s = 0; s < S; s++) {
        snprintf(who, sizeof who, "speaker %d: ", s);
        fe_check_args(*models[s], X + (size_t)row_offsets[s] * D, (long)(row_offsets[s + 1] - row_offsets[s]), D, params[s], who);
    }
    messages.assign((size_t)S, std::string());
    ensure_device();
    g_fit_batch_calls++;
    g_fit_batch_speakers += S;
    // groups of speakers, in batch order, whose workspace stays under full_fit_batch_bytes (a speaker larger than that is a group
    // of its own); a speaker's fit does not depend on its group
    const long limit = g_fit_batch_bytes.load();
    int s0 = 0;
    while (s0 < S) {
        size_t bytes = 0;
        int s1 = s0;
        while (s1 < S && s1 - s0 < 65535) {
            const size_t need = fe_spk_bytes((long)(row_offsets[s1 + 1] - row_offsets[s1]), K, D);
            if (s1 > s0 && bytes + need > (size_t)limit) break;
            bytes += need;
            s1++;
        }
        g_fit_batch_iterations += fe_fit_group(models, s0, s1, X, row_offsets, D, params, out, status, messages);
        s0 = s1;
    }
}

void fullset_pack(SRFullSet &set, const SRFullGMM *const *models, int S) {
    if (S < 1) fail("a set needs at least one model");
    const int D = models[0] ? models[0]->D : 0;
    set.S = S;
    set.D = D;
    set.ns = (D + 1) / 2;
    set.nrb = (D + 31) / 32;
    set.kbeg.assign(S + 1, 0);
    for (int m = 0; m < S; m++) {
        const SRFullGMM *g = models[m];
        if (!g) fail("null model %d", m);
        if (!g->trained) fail("model %d has no parameters", m);
        if (g->D != D) fail("model %d has %d dims, model 0 has %d", m, g->D, D);
        set.kbeg[m + 1] = set.kbeg[m] + g->K;
    }
    const int KT = set.kbeg[S], ns = set.ns, nrb = set.nrb, per = nrb * ns * 64;
    std::vector<float> P((size_t)KT * per, 0.f), mu((size_t)KT * 64, 0.f), c(KT);
    for (int m = 0; m < S; m++) {
        const SRFullGMM *g = models[m];
        for (int k = 0; k < g->K; k++) {
            const int kt = set.kbeg[m] + k;
            const double *Pk = g->prec_chol.data() + (size_t)k * D * D;
            // A of v_mfma_f32_32x32x2_f32: lane l holds A[row l & 31][step dim l >> 5] = P^T[j][d] = P[d][j]
            for (int rb = 0; rb < nrb; rb++)
                for (int s = 0; s < ns; s++)
                    for (int l = 0; l < 64; l++) {
                        const int d = 2 * s + (l >> 5), j = 32 * rb + (l & 31);
                        if (d < D && j < D) P[(size_t)kt * per + ((size_t)rb * ns + s) * 64 + l] = (float)Pk[(size_t)d * D + j];
                    }
            double ld = 0.0;
            for (int i = 0; i < D; i++) {
                mu[(size_t)kt * 64 + i] = (float)g->means[(size_t)k * D + i];
                ld += std::log(Pk[(size_t)i * D + i]);
            }
            c[kt] = (float)(std::log(g->weights[k]) + ld - 0.5 * D * FC_LN_2PI);
        }
    }
    ensure_device();
    set.device = current_device();
    set.P.upload(P.data(), P.size());
    set.mu.upload(mu.data(), mu.size());
    set.c.upload(c.data(), c.size());
    set.d_kbeg.upload(set.kbeg.data(), set.kbeg.size());
    sync_stream();
}

namespace {

void fullset_check(SRFullSet &set, SRBatch &b) {
    if (b.kind != SRBatch::FEATURES) fail("full-covariance scoring needs a feature batch");
    if (b.dim != set.D) fail("batch has %d dims, the models %d", b.dim, set.D);
    ensure_device();
    if (set.device != current_device()) fail("model set lives on device %d, the calling thread is on device %d", set.device, current_device());
    b.bind_device();
}

// the scoring kernel into set.fll [S][n] (the caller has sized it)
void fullset_launch_score(SRFullSet &set, const SRBatch &b, hipStream_t st) {
    const long n = b.n_rows;
    const int S = set.S;
    if (set.D <= 32) {
        const unsigned gx = (unsigned)((n + 4 * 4 * 32 - 1) / (4 * 4 * 32));
        hipLaunchKernelGGL((fullcov_score_kernel<16, 4>), dim3(gx, S), dim3(256), 0, st, b.data.p, n, set.D, set.ns, set.nrb, set.P.p,
                           set.mu.p, set.c.p, set.d_kbeg.p, set.fll.p);
    } else {
        const unsigned gx = (unsigned)((n + 4 * 2 * 32 - 1) / (4 * 2 * 32));
        hipLaunchKernelGGL((fullcov_score_kernel<32, 2>), dim3(gx, S), dim3(256), 0, st, b.data.p, n, set.D, set.ns, set.nrb, set.P.p,
                           set.mu.p, set.c.p, set.d_kbeg.p, set.fll.p);
    }
}

}  // namespace

void fullset_reserve(SRFullSet &set, int64_t n_rows, int n_utt) {
    set.fll.ensure((size_t)set.S * std::max<int64_t>(1, n_rows));
    set.res.ensure((size_t)std::max(1, n_utt) * set.S + ((size_t)std::max(1, n_utt) + 1) / 2);
}

const double *fullset_score_device(SRFullSet &set, SRBatch &b) {
    fullset_check(set, b);
    const long n = b.n_rows;
    const int U = b.n_utt, S = set.S;
    fullset_reserve(set, n, U);
    hipStream_t st = ctx().stream;
    ScopedKernelTimer timer(T_SCORE);
    if (n > 0) fullset_launch_score(set, b, st);
    if (U > 0)
        hipLaunchKernelGGL(fullcov_finalize_kernel, dim3((unsigned)U), dim3(64 * FC_FIN_WAVES), 0, st, set.fll.p, n, b.d_offsets.p, U, S,
                           set.res.p, reinterpret_cast<int *>(set.res.p + (size_t)U * S), (const int *)nullptr, 0);
    SR_HIP(hipGetLastError());
    return set.res.p;
}

void masked_finalize(const float *fll, long n, const int64_t *d_off, const int *d_cnt, int U, int S, bool plain, double *d_sums, int *d_argmax) {
    if (U <= 0) return;
    hipLaunchKernelGGL(fullcov_finalize_kernel, dim3((unsigned)U), dim3(64 * FC_FIN_WAVES), 0, ctx().stream, fll, n, d_off, U, S, d_sums,
                       d_argmax, d_cnt, plain ? 1 : 0);
    SR_HIP(hipGetLastError());
}

void fullset_score_device_masked(SRFullSet &set, SRBatch &b, const int *d_cnt, double *d_res) {
    fullset_check(set, b);
    const long n = b.n_rows;
    const int U = b.n_utt, S = set.S;
    set.fll.ensure((size_t)S * std::max(1L, n));
    ScopedKernelTimer timer(T_SCORE);
    if (n > 0) fullset_launch_score(set, b, ctx().stream);
    masked_finalize(set.fll.p, n, b.d_offsets.p, d_cnt, U, S, false, d_res, reinterpret_cast<int *>(d_res + (size_t)U * S));
}

void fullset_predict_pcm(SRMfcc &m, SRFullSet &set, SRBatch &pcm, int nd, double *sums, int *argmax) {
    ensure_device();
    if (set.device != current_device()) fail("model set lives on device %d, the calling thread is on device %d", set.device, current_device());
    if (nd < 0 || nd > 2) fail("delta order must be 0, 1 or 2");
    if (m.n_lpc > 0 && nd != 0) fail("LPC columns (mix_feature) come without deltas: use nd = 0");
    const int dim = m.n_ceps * (nd + 1) + m.n_lpc;
    if (dim != set.D)
        fail("the extractor yields %d columns (%d cepstra x %d + %d LPC), the models have %d dims", dim, m.n_ceps, nd + 1, m.n_lpc, set.D);
    struct Workspace {
        SRBatch feat;            // reused across calls: a serving loop allocates nothing
    };
    SRBatch &feat = per_device<Workspace>().feat;
    mfcc_extract_batch(m, pcm, nd, 1, feat);
    const int U = feat.n_utt, S = set.S;
    const double *res = fullset_score_device(set, feat);
    // sums and the argmax values behind them: one copy
    const size_t n_sums = (size_t)U * S, bytes = n_sums * sizeof(double) + (size_t)U * sizeof(int);
    set.h_res.ensure(n_sums + ((size_t)U + 1) / 2 + 1);
    if (U > 0) SR_HIP(hipMemcpyAsync(set.h_res.p, res, bytes, hipMemcpyDeviceToHost, ctx().stream));
    sync_stream();
    if (sums) std::copy(set.h_res.p, set.h_res.p + n_sums, sums);
    if (argmax) std::memcpy(argmax, set.h_res.p + n_sums, (size_t)U * sizeof(int));
}

void fullset_score(SRFullSet &set, SRBatch &b, double *sums, int *argmax, float *frame_ll) {
    fullset_check(set, b);
    const long n = b.n_rows;
    const int U = b.n_utt, S = set.S;
    set.fll.ensure((size_t)S * std::max(1L, n));
    set.sums.ensure((size_t)std::max(1, U) * S);
    hipStream_t st = ctx().stream;
    if (n > 0) {
        ScopedKernelTimer timer(T_SCORE);
        fullset_launch_score(set, b, st);
        if (U > 0)
            hipLaunchKernelGGL(fullcov_sum_kernel, dim3((unsigned)(((long)U * S + 3) / 4)), dim3(256), 0, st, set.fll.p, n, b.d_offsets.p, U, S,
                               set.sums.p);
        SR_HIP(hipGetLastError());
    }
    std::vector<double> h((size_t)U * S, 0.0);
    if (n > 0 && U > 0) set.sums.download(h.data(), h.size());
    if (frame_ll && n > 0) set.fll.download(frame_ll, (size_t)S * n);
    sync_stream();
    if (sums) std::copy(h.begin(), h.end(), sums);
    if (argmax)
        for (int u = 0; u < U; u++) {
            int best = 0;
            for (int m = 1; m < S; m++)
                if (h[(size_t)u * S + m] > h[(size_t)u * S + best]) best = m;
            argmax[u] = best;
        }
}

}  // namespace sr
