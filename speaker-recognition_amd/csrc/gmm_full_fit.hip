// gmm_full_fit.hip -- training full-covariance GMMs: scikit-learn's GaussianMixture(covariance_type='full').fit, the model the
// reference's shipped CLI trains (src/gui/skgmm.py:20, GaussianMixture(32) on mix_feature's 28 columns).  Scoring: gmm_full.hip.
//
// Float64, the whole fit on the device (em_f64.hip's pattern): one driver, fe_fit_group, fits a group of speakers of one K and D in
// the same launches.  An iteration is eight launches -- log densities, log-sum-exp + responsibilities, the mean (lower
// bound), nk + means, the covariance sums by frame chunks, the per-mixture Cholesky + inverse (one workgroup per mixture), the
// weights, the stop rule per speaker -- and the host reads one 16-byte record per speaker.  The statistics run on the vector ALU
// in float64: at speaker size (K 32, D 28, ~5600 frames) the covariance GEMMs are 8e7 FMAs per iteration, microseconds of
// arithmetic, while a measured iteration takes ~0.4 ms (K-wide per-mixture kernels); the fp64 MFMA (D = 28
// padded to 32, the responsibility applied to an operand first) was therefore not tried.
// The kernels are the bodies below with a speaker axis; inside a speaker every sum is formed by the same threads in the same order
// whatever the group, so a speaker's bits do not depend on the speakers fitted with it.
// What is decided before the device is touched -- the cut of a batch into groups by workspace size, the per-speaker tables, the
// work lists, every buffer's size -- is full_plan.cpp's ("Training"): fullgmm_fit plans a group of one,
// fullgmm_fit_batch its whole call, and fe_fit_group runs one group of a plan as four steps: fill the workspace, start, loop,
// hand back.
#include "gmm_full.hpp"
#include "kmeans_init.hpp"

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

namespace sr {

namespace {

const char *const FC_ILL_DEFINED =
    "Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance caused by "
    "singleton or collapsed samples). Try to decrease the number of components, increase reg_covar, or scale the input data.";

// ---------------------------------------------------------------- the kernels (FE_FB, FE_CB, FE_PQ, FULL_MAX_D: full_plan.hpp)
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
struct FeRec {                      // what the host reads after every iteration
    double bound;
    int state, n_iter;
};
static_assert(sizeof(FeSpk) == FE_SPK_BYTES && sizeof(FeRec) == FE_REC_BYTES, "full_plan.hpp counts the tables' bytes by these sizes");
static_assert(sizeof(int2) == sizeof(FullWork) && alignof(int2) >= alignof(FullWork), "the work lists go up as the plan holds them");
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

// ---------------------------------------------------------------- the driver
// (every buffer's size: FullCounts of full_plan.hpp, which the group cut adds up)
struct FeBatchWorkspace {
    DevBuf<double> X, w, logw, mu, prec, logdet, cov, lp, lpn, nk, partial, head;
    DevBuf<FeSpk> spk;
    DevBuf<FeRec> rec;
    DevBuf<int2> wl_lp, wl_lse, wl_cov;
    DevBuf<int> label;
    PinnedBuf<FeRec> h_rec;
};

// sr_set_option("full_fit_batch_bytes"): 1 GiB holds 100 speakers of 5600 x 28 at K 32 (5.5 MB each: X, lp, lpn, the chunk sums,
// the parameters and tables) in one group with room to spare.  The workspace only grows and is kept for the next call, like the
// library's other per-device workspaces: after a batch a process holds up to this much device memory.
std::atomic<long> g_fit_batch_bytes{(long)FULL_DEFAULT_BYTES};
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

// the plan of a call (no device work): S speakers of one K, lengths from row_offsets
void fe_plan(int K, int D, const int64_t *row_offsets, const SRFullFitParams *params, int S, long bound, FullFitPlan &plan) {
    std::vector<int64_t> n((size_t)S);
    std::vector<int> given((size_t)S), max_iter((size_t)S);
    for (int s = 0; s < S; s++) {
        n[s] = row_offsets[s + 1] - row_offsets[s];
        given[s] = params[s].init_given ? 1 : 0;
        max_iter[s] = params[s].max_iter;
    }
    std::string why;
    if (!plan_full_fit(K, D, n.data(), given.data(), max_iter.data(), S, bound, plan, why)) fail("%s", why.c_str());
}

// One group of a plan on the device.  The arrays of the call (models, X, params) start at the group's first speaker.
struct FeGroup {
    const FullGroupPlan &g;
    const FullSpeakerPlan *spk;     // [g.count]
    SRFullGMM *const *models;
    const double *X;
    const SRFullFitParams *params;
    FeBatchWorkspace &ws;
    FeBatch b;
    size_t lds_lp;
    hipStream_t st;
};

// Step 1: the workspace sized by the plan's counts; X, the two tables built from the plan's rows and the three work lists go up
void fe_fill_workspace(FeGroup &q, const FullFitPlan &plan) {
    const FullGroupPlan &g = q.g;
    const FullCounts &c = g.counts;
    FeBatchWorkspace &ws = q.ws;
    const int S = g.count;
    std::vector<FeSpk> spk((size_t)S);
    std::vector<FeRec> rec((size_t)S);
    for (int i = 0; i < S; i++) {
        const FullSpeakerPlan &sp = q.spk[i];
        const SRFullFitParams &p = q.params[i];
        FeSpk &t = spk[i];
        t.row0 = (long)sp.row0;
        t.n = (long)sp.n;
        t.n_chunks = sp.n_chunks;
        t.chunk = sp.chunk;
        t.o_partial = (long)sp.o_partial;
        t.reg = p.reg_covar;
        t.tol = p.tol;
        t.prev = -std::numeric_limits<double>::infinity();
        t.max_iter = p.max_iter;
        t.state = FE_ACTIVE;
        t.given = p.init_given ? 1 : 0;
        t.pad = 0;
        rec[i] = FeRec{t.prev, FE_ACTIVE, 0};
    }
    ws.X.upload(q.X, (size_t)c.X);
    ws.w.ensure((size_t)c.w);
    ws.logw.ensure((size_t)c.logw);
    ws.mu.ensure((size_t)c.mu);
    ws.prec.ensure((size_t)c.prec);
    ws.logdet.ensure((size_t)c.logdet);
    ws.cov.ensure((size_t)c.cov);
    ws.lp.ensure((size_t)c.lp);
    ws.lpn.ensure((size_t)c.lpn);
    ws.nk.ensure((size_t)c.nk);
    ws.partial.ensure((size_t)c.partial);
    ws.head.ensure((size_t)c.head);
    ws.spk.upload(spk.data(), (size_t)c.spk);
    ws.rec.upload(rec.data(), (size_t)c.rec);
    ws.wl_lp.upload(reinterpret_cast<const int2 *>(plan.wl_lp.data() + g.lp0), (size_t)c.wl_lp);
    ws.wl_lse.upload(reinterpret_cast<const int2 *>(plan.wl_lse.data() + g.lse0), (size_t)c.wl_lse);
    ws.wl_cov.upload(reinterpret_cast<const int2 *>(plan.wl_cov.data() + g.cov0), (size_t)c.wl_cov);
    ws.h_rec.ensure((size_t)c.rec);
    FeBatch &b = q.b;
    b = FeBatch{};
    b.X = ws.X.p; b.D = plan.D; b.K = plan.K; b.S = S;
    b.w = ws.w.p; b.logw = ws.logw.p; b.mu = ws.mu.p; b.prec = ws.prec.p; b.logdet = ws.logdet.p; b.cov = ws.cov.p;
    b.lp = ws.lp.p; b.lpn = ws.lpn.p; b.nk = ws.nk.p; b.partial = ws.partial.p; b.head = ws.head.p;
    b.spk = ws.spk.p; b.rec = ws.rec.p; b.wl_lp = ws.wl_lp.p; b.wl_lse = ws.wl_lse.p; b.wl_cov = ws.wl_cov.p;
    SR_HIP(hipMemsetAsync(ws.head.p, 0, (size_t)c.head * sizeof(double), q.st));
}

// the M-step's four launches and the stop rule behind them
void fe_launch_mstep(const FeGroup &q, int weight_mode, int it) {
    const FeBatch &b = q.b;
    const unsigned K = (unsigned)b.K, S = (unsigned)b.S;
    hipLaunchKernelGGL(fe_means_batch_kernel, dim3(K, S), dim3(256), 0, q.st, b);
    hipLaunchKernelGGL(fe_cov_batch_kernel, dim3((unsigned)q.g.counts.wl_cov, K), dim3(256), 0, q.st, b);
    hipLaunchKernelGGL(fe_chol_batch_kernel, dim3(K, S), dim3(64), 0, q.st, b);
    hipLaunchKernelGGL(fe_weights_batch_kernel, dim3(S), dim3(64), 0, q.st, b, weight_mode);
    hipLaunchKernelGGL(fe_stop_batch_kernel, dim3((S + 63) / 64), dim3(64), 0, q.st, b, it);
}

// Step 2, the start.  The given parameters go up first (whole arrays: a k-means speaker's slice is written by its M-step
// behind them); then the k-means speakers take their first M-step (which can only fail) and the given ones their derive launch,
// each launch restricted to its kind by b.only.
void fe_start(FeGroup &q) {
    const FullGroupPlan &g = q.g;
    FeBatch &b = q.b;
    FeBatchWorkspace &ws = q.ws;
    const int S = g.count, K = b.K, D = b.D;
    if (g.any_given) {
        std::vector<double> w0((size_t)g.counts.w, 0.0), mu0((size_t)g.counts.mu, 0.0), prec0((size_t)g.counts.prec, 0.0);
        for (int i = 0; i < S; i++) {
            if (!q.params[i].init_given) continue;
            const SRFullGMM &m = *q.models[i];
            std::copy(m.weights.begin(), m.weights.end(), w0.begin() + (size_t)i * K);
            std::copy(m.means.begin(), m.means.end(), mu0.begin() + (size_t)i * K * D);
            std::copy(m.prec_chol.begin(), m.prec_chol.end(), prec0.begin() + (size_t)i * K * D * D);
        }
        ws.w.upload(w0.data(), w0.size());
        ws.mu.upload(mu0.data(), mu0.size());
        ws.prec.upload(prec0.data(), prec0.size());
    }
    if (g.any_kmeans) {
        // sklearn's init_params='kmeans', speaker by speaker in batch order (kmeans_labels is host-sequenced)
        std::vector<int> label((size_t)g.rows, 0);
        std::vector<float> Xf;
        for (int i = 0; i < S; i++) {
            if (q.params[i].init_given) continue;
            const double *Xs = q.X + (size_t)q.spk[i].row0 * D;
            Xf.resize((size_t)q.spk[i].n * D);
            for (size_t e = 0; e < Xf.size(); e++) Xf[e] = (float)Xs[e];
            const std::vector<int> l = kmeans_labels(Xf.data(), (long)q.spk[i].n, D, K, q.params[i].seed);
            std::copy(l.begin(), l.end(), label.begin() + q.spk[i].row0);
        }
        ws.label.upload(label.data(), label.size());
        b.only = 1;
        hipLaunchKernelGGL(fe_onehot_batch_kernel, dim3((unsigned)g.counts.wl_lse), dim3(256), 0, q.st, b, ws.label.p);
        fe_launch_mstep(q, 1, 0);
    }
    if (g.any_given) {
        b.only = 2;
        hipLaunchKernelGGL(fe_derive_batch_kernel, dim3((K + 63) / 64, S), dim3(64), 0, q.st, b);
    }
    b.only = 0;
}

// Step 3, the loop: an iteration's eight launches ...
void fe_launch_iteration(const FeGroup &q, int it) {
    const FeBatch &b = q.b;
    const FullCounts &c = q.g.counts;
    hipLaunchKernelGGL(fe_logprob_batch_kernel, dim3((unsigned)c.wl_lp, b.K), dim3(256), q.lds_lp, q.st, b);
    hipLaunchKernelGGL(fe_lse_batch_kernel, dim3((unsigned)c.wl_lse), dim3(256), 0, q.st, b);
    hipLaunchKernelGGL(fe_bound_batch_kernel, dim3(b.S), dim3(256), 0, q.st, b);
    fe_launch_mstep(q, 0, it);
}

// ... and the S records behind them -> is a speaker still active
bool fe_read_records(const FeGroup &q) {
    const int S = q.g.count;
    SR_HIP(hipGetLastError());
    SR_HIP(hipMemcpyAsync(q.ws.h_rec.p, q.ws.rec.p, (size_t)S * sizeof(FeRec), hipMemcpyDeviceToHost, q.st));
    sync_stream();
    bool active = false;
    for (int i = 0; i < S; i++) active = active || q.ws.h_rec.p[i].state == FE_ACTIVE;
    return active;
}

// Step 4: the parameters come down; a fitted speaker's go to its handle.  status[i]: 0 fitted, -1 failed (messages[i] says why;
// the handle keeps its parameters)
void fe_hand_back(const FeGroup &q, SRFullFitStats *out, int *status, std::string *messages) {
    const FullCounts &c = q.g.counts;
    const int S = q.g.count, K = q.b.K, D = q.b.D;
    std::vector<double> w((size_t)c.w), mu((size_t)c.mu), prec((size_t)c.prec), cov((size_t)c.cov);
    q.ws.w.download(w.data(), w.size());
    q.ws.mu.download(mu.data(), mu.size());
    q.ws.prec.download(prec.data(), prec.size());
    q.ws.cov.download(cov.data(), cov.size());
    sync_stream();
    for (int i = 0; i < S; i++) {
        const FeRec &r = q.ws.h_rec.p[i];
        SRFullGMM &m = *q.models[i];
        if (r.state == FE_FAILED) {
            status[i] = -1;
            messages[i] = FC_ILL_DEFINED;
            continue;
        }
        status[i] = 0;
        out[i].converged = r.state == FE_CONVERGED ? 1 : 0;
        out[i].n_iter = r.n_iter;
        out[i].lower_bound = r.bound;
        m.weights.assign(w.begin() + (size_t)i * K, w.begin() + (size_t)(i + 1) * K);
        m.means.assign(mu.begin() + (size_t)i * K * D, mu.begin() + (size_t)(i + 1) * K * D);
        m.prec_chol.assign(prec.begin() + (size_t)i * K * D * D, prec.begin() + (size_t)(i + 1) * K * D * D);
        m.covariances.assign(cov.begin() + (size_t)i * K * D * D, cov.begin() + (size_t)(i + 1) * K * D * D);
        m.trained = true;
    }
}

// The EM driver: group `gi` of a plan, one set of launches per EM iteration, one download of the group's records behind it.
// models, X (first row of the call), row_offsets, params, out, status, messages: the call's arrays.  -> the iterations launched
long fe_fit_group(const FullFitPlan &plan, size_t gi, SRFullGMM *const *models, const double *X, const int64_t *row_offsets,
                  const SRFullFitParams *params, SRFullFitStats *out, int *status, std::string *messages) {
    const FullGroupPlan &g = plan.groups[gi];
    FeGroup q{g, plan.speakers.data() + g.first, models + g.first, X + (size_t)row_offsets[g.first] * plan.D, params + g.first,
              per_device<FeBatchWorkspace>(), FeBatch{}, plan.lds_logprob, ctx().stream};
    fe_fill_workspace(q, plan);
    fe_start(q);
    bool active = g.any_kmeans ? fe_read_records(q) : true;
    long iterations = 0;
    for (int it = 1; active && it <= g.max_iter; it++) {
        fe_launch_iteration(q, it);
        active = fe_read_records(q);
        iterations++;
    }
    fe_hand_back(q, out + g.first, status + g.first, messages + g.first);
    return iterations;
}

}  // namespace

// a group of one.  Not a fullgmm_fit_batch of one: no "speaker 0: " in a message, no counter moves, and no option cuts or refuses it
void fullgmm_fit(SRFullGMM &g, const double *X, long n, int D, const SRFullFitParams &p, SRFullFitStats &out) {
    fe_check_args(g, X, n, D, p, "");
    const int64_t row_offsets[2] = {0, n};
    FullFitPlan plan;
    fe_plan(g.K, D, row_offsets, &p, 1, std::numeric_limits<long>::max(), plan);
    ensure_device();
    SRFullGMM *const model = &g;
    int status = 0;
    std::string message;
    fe_fit_group(plan, 0, &model, X, row_offsets, &p, &out, &status, &message);
    if (status != 0) fail("%s", message.c_str());
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
    // groups of speakers, in batch order, whose workspace stays under full_fit_batch_bytes (a speaker larger than that is a group
    // of its own); a speaker's fit does not depend on its group
    FullFitPlan plan;
    fe_plan(K, D, row_offsets, params, S, g_fit_batch_bytes.load(), plan);
    messages.assign((size_t)S, std::string());
    ensure_device();
    g_fit_batch_calls++;
    g_fit_batch_speakers += S;
    for (size_t gi = 0; gi < plan.groups.size(); gi++)
        g_fit_batch_iterations += fe_fit_group(plan, gi, models, X, row_offsets, params, out, status, messages.data());
}

}  // namespace sr
