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
// Training (float64, the whole fit on the device): gmm_full_fit.hip, planned by full_plan.cpp.
#include "gmm_full.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace sr {

namespace {

typedef float fc_f32x16 __attribute__((ext_vector_type(16)));

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

}  // namespace

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
