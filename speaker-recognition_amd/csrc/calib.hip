// calib.hip -- score calibration and fusion on the device: prior-weighted linear logistic regression (Bruemmer's FoCal / BOSARIS) of
// S <= 8 score rows X [S][n] against labels lab [n] (1 target, 0 non-target, negative: not a trial), float64 throughout.
// With theta = (w_1 .. w_S, b), z_i = sum_s w_s X[s][i] + b, tau = ln(P / (1 - P)), sp(a) = max(a, 0) + log1p(exp(-|a|)):
//   f = (1 / ln 2) [P / n_t sum_tar sp(-(z_i + tau)) + (1 - P) / n_n sum_non sp(z_i + tau)] + lam / 2 sum_s w_s^2
// and g, H its gradient and Hessian (include/pygmm_hip.h states them).  Cllr is f at S = 1, theta = (1, 0), P = 1/2, lam = 0.
// The kernels:
//   calib_pass_kernel<S>    one evaluation of (f, g, H) at the state's trial point.  A workgroup of 256 lanes owns CALIB_BLOCK = 4096
//                           consecutive trials, lane l the trials l, l + 256, ... of the block (coalesced).  f, g and the upper triangle
//                           of H -- 1 + (S + 1) + (S + 1)(S + 2) / 2 float64 accumulators -- stay in registers; one exp per trial:
//                           sp, s and s (1 - s) all come from e = exp(-|z + tau|), so nothing overflows and 1 - s is formed without
//                           cancellation.  A skipped trial's scores are replaced by a select, never multiplied.  The workgroup's sums
//                           go through a fixed tree (wave_sum_f64, then the four waves in order) into partial [n_blocks][A].
//   calib_step_kernel<S>    one workgroup: lane l adds the partials of blocks l, l + 256, ... in that order, then the same tree; the
//                           ridge; then lane 0 alone: the accept / halve decision of the damped Newton loop, the Cholesky
//                           factorisation of H (at most 9 x 9, in LDS), the solve, the Newton decrement and the stop rule.  It writes
//                           the state (calib_plan.hpp) that the next pass reads.
//   calib_apply_kernel<S>   out[i] = z_i, elementwise over all n.
//   calib_counts_kernel     misses and false alarms at up to 16 thresholds in one pass: ballots and population counts, integers
//                           per workgroup that the host adds.  Exact.
// Both kernels of the loop return at once when the state's stop word is set, so the host enqueues pass + step pairs without reading
// anything back but that word, every CALIB_CADENCE-th pair.  No atomics; the block size is fixed, so the bits of a result depend on
// (X, lab, P, lam, theta0, tol, max_pass) only -- not on the number of compute units, an option, or the run.
#include "calib.hpp"
#include "calib_plan.hpp"
#include "common.hpp"
#include "wave_ops.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <vector>

namespace sr {

static_assert(CALIB_WG == 256 && CALIB_BLOCK % CALIB_WG == 0, "four waves; a block is a whole number of strides");
static_assert(calib_acc(CALIB_MAX_S) <= CALIB_WG, "a lane per accumulator writes the workgroup's sums");
constexpr int CALIB_WAVES = CALIB_WG / 64;
constexpr double CALIB_INV_LN2 = 1.4426950408889634074;
// A pivot that is not above the rounding error of its own formation counts as not > 0: two identical systems give a pivot of a few
// ulps of H_jj of either sign, not an exact zero.
constexpr double CALIB_PIVOT_REL = 16.0 * 2.220446049250313e-16;

struct CalibTheta {
    double v[CALIB_MAX_S + 1];
};
struct CalibThr {
    double v[CALIB_MAX_THR];
};

// The workgroup's sum of every accumulator, in a fixed order; lane k < A ends with the total of accumulator k.
template <int A>
static __device__ __forceinline__ double calib_block_sum(double (&acc)[A], double (*red)[A]) {
#pragma unroll
    for (int k = 0; k < A; k++) {
        const double t = wave_sum_f64(acc[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = t;
    }
    __syncthreads();
    double tot = 0.0;
    if (threadIdx.x < A) tot = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    return tot;
}

template <int S>
__global__ __launch_bounds__(CALIB_WG) void calib_pass_kernel(const double *__restrict__ X, const signed char *__restrict__ lab, int64_t n,
                                                               const double *__restrict__ state, double tau, double c_t, double c_n,
                                                               double *__restrict__ partial) {
    constexpr int P = S + 1, A = calib_acc(S);
    __shared__ double red[CALIB_WAVES][A];
    if (state[CALIB_ST_STOP] >= 0.0) return;
    double w[P];
#pragma unroll
    for (int s = 0; s < P; s++) w[s] = state[calib_off_trial(S) + s];
    double acc[A];
#pragma unroll
    for (int k = 0; k < A; k++) acc[k] = 0.0;
    const int64_t base = (int64_t)blockIdx.x * CALIB_BLOCK + threadIdx.x;
#pragma unroll 1
    for (int it = 0; it < CALIB_BLOCK / CALIB_WG; it++) {
        const int64_t i = base + (int64_t)it * CALIB_WG;
        const bool in = i < n;
        const int l = in ? (int)lab[i] : -1;
        const bool valid = l >= 0, target = l > 0;
        double x[P];
#pragma unroll
        for (int s = 0; s < S; s++) {
            const double v = in ? X[(int64_t)s * n + i] : 0.0;
            x[s] = valid ? v : 0.0;
        }
        x[S] = 1.0;
        double z = w[S];
#pragma unroll
        for (int s = 0; s < S; s++) z = fma(w[s], x[s], z);
        const double a = z + tau;
        const double e = exp(-fabs(a));
        const double l1p = log1p(e);
        const double q = 1.0 / (1.0 + e), eq = e * q;
        const bool pos = a >= 0.0;
        const double sg = pos ? q : eq, oms = pos ? eq : q;          // s and 1 - s
        const double c = valid ? (target ? c_t : c_n) : 0.0;
        const double spv = fmax(target ? -a : a, 0.0) + l1p;
        const double r = c * (target ? -oms : sg);
        const double h = c * (eq * q);
        acc[0] = fma(c, spv, acc[0]);
#pragma unroll
        for (int s = 0; s < S; s++) acc[1 + s] = fma(r, x[s], acc[1 + s]);
        acc[1 + S] += r;
        int k = 1 + P;
#pragma unroll
        for (int s = 0; s < P; s++) {
            const double hx = s < S ? h * x[s] : h;
#pragma unroll
            for (int t = s; t < P; t++) {
                acc[k] = t < S ? fma(hx, x[t], acc[k]) : acc[k] + hx;
                k++;
            }
        }
    }
    const double tot = calib_block_sum<A>(acc, red);
    if (threadIdx.x < A) partial[(int64_t)blockIdx.x * A + threadIdx.x] = tot;
}

// mode 0: a step of the fit; 1: evaluation only (f, g, H of the trial point into the state's slots, stop = CONVERGED).
template <int S>
__global__ __launch_bounds__(CALIB_WG) void calib_step_kernel(const double *__restrict__ partial, int64_t n_blocks, double *__restrict__ state,
                                                               double ridge, double tol, int mode) {
    constexpr int P = S + 1, A = calib_acc(S);
    __shared__ double red[CALIB_WAVES][A];
    __shared__ double tot[A];
    __shared__ double L[P][P];
    __shared__ double y[P], d[P];
    if (state[CALIB_ST_STOP] >= 0.0) return;
    double acc[A];
#pragma unroll
    for (int k = 0; k < A; k++) acc[k] = 0.0;
#pragma unroll 1
    for (int64_t b = threadIdx.x; b < n_blocks; b += CALIB_WG) {
#pragma unroll
        for (int k = 0; k < A; k++) acc[k] += partial[b * A + k];
    }
    const double mine = calib_block_sum<A>(acc, red);
    if (threadIdx.x < A) tot[threadIdx.x] = mine * CALIB_INV_LN2;
    __syncthreads();
    if (threadIdx.x != 0) return;

    double *theta = state + calib_off_theta(S), *trial = state + calib_off_trial(S), *sd = state + calib_off_d(S);
    double *sg = state + calib_off_g(S), *sH = state + calib_off_H(S);
    // the ridge, on the S weights only
    double w2 = 0.0;
    {
        int k = 1 + P;
        for (int s = 0; s < P; s++) {
            if (s < S) {
                const double w = trial[s];
                w2 = fma(w, w, w2);
                tot[1 + s] = fma(ridge, w, tot[1 + s]);
                tot[k] += ridge;
            }
            k += P - s;
        }
    }
    const double f_new = fma(0.5 * ridge, w2, tot[0]);
    const double passes = state[CALIB_ST_PASSES] + 1.0;
    state[CALIB_ST_PASSES] = passes;
    if (mode == 1) {
        state[CALIB_ST_F] = f_new;
        for (int k = 0; k < P; k++) sg[k] = tot[1 + k];
        for (int k = 0; k < P * (P + 1) / 2; k++) sH[k] = tot[1 + P + k];
        state[CALIB_ST_STOP] = (double)CALIB_CONVERGED;
        return;
    }
    const bool capped = passes >= state[CALIB_ST_CAP];
    const bool first = state[CALIB_ST_PHASE] == 0.0;
    const double f_old = state[CALIB_ST_F];
    if (!first && !(isfinite(f_new) && f_new <= f_old)) {
        // halve
        const double t = 0.5 * state[CALIB_ST_T];
        state[CALIB_ST_T] = t;
        state[CALIB_ST_HALVINGS] += 1.0;
        if (t < 1.0 / (double)(1 << CALIB_HALVINGS)) {
            state[CALIB_ST_STOP] = (double)CALIB_STALLED;
            return;
        }
        for (int k = 0; k < P; k++) trial[k] = fma(t, sd[k], theta[k]);
        if (capped) state[CALIB_ST_STOP] = (double)CALIB_CAP;
        return;
    }
    // accept
    if (!first) state[CALIB_ST_ACCEPTED] += 1.0;
    state[CALIB_ST_PHASE] = 1.0;
    state[CALIB_ST_F] = f_new;
    for (int k = 0; k < P; k++) theta[k] = trial[k], sg[k] = tot[1 + k];
    for (int k = 0; k < P * (P + 1) / 2; k++) sH[k] = tot[1 + P + k];
    // H = L L^T
    {
        int k = 1 + P;
        for (int s = 0; s < P; s++)
            for (int t = s; t < P; t++) L[t][s] = tot[k++];          // the lower triangle holds H
    }
    for (int j = 0; j < P; j++) {
        const double hjj = L[j][j];
        double piv = hjj;
        for (int k = 0; k < j; k++) piv -= L[j][k] * L[j][k];
        if (!(piv > CALIB_PIVOT_REL * hjj) || !isfinite(piv)) {
            state[CALIB_ST_STOP] = (double)CALIB_SINGULAR;
            return;
        }
        const double ljj = sqrt(piv);
        L[j][j] = ljj;
        for (int i = j + 1; i < P; i++) {
            double v = L[i][j];
            for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k];
            L[i][j] = v / ljj;
        }
    }
    // L y = -g, L^T d = y
    for (int i = 0; i < P; i++) {
        double v = -tot[1 + i];
        for (int k = 0; k < i; k++) v -= L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
    for (int i = P - 1; i >= 0; i--) {
        double v = y[i];
        for (int k = i + 1; k < P; k++) v -= L[k][i] * d[k];
        d[i] = v / L[i][i];
    }
    double lam2 = 0.0;
    bool finite = true;
    for (int k = 0; k < P; k++) {
        lam2 -= tot[1 + k] * d[k];
        sd[k] = d[k];
        finite = finite && isfinite(theta[k] + d[k]);
    }
    state[CALIB_ST_LAM2] = lam2;
    if (!isfinite(lam2) || !finite) {
        state[CALIB_ST_STOP] = (double)CALIB_SINGULAR;
        return;
    }
    if (lam2 <= tol) {
        state[CALIB_ST_STOP] = (double)CALIB_CONVERGED;
        return;
    }
    state[CALIB_ST_T] = 1.0;
    for (int k = 0; k < P; k++) trial[k] = theta[k] + d[k];
    if (capped) state[CALIB_ST_STOP] = (double)CALIB_CAP;
}

template <int S>
__global__ __launch_bounds__(CALIB_WG) void calib_apply_kernel(const double *__restrict__ X, int64_t n, CalibTheta th, double *__restrict__ out) {
    const int64_t base = (int64_t)blockIdx.x * CALIB_BLOCK + threadIdx.x;
#pragma unroll 4
    for (int it = 0; it < CALIB_BLOCK / CALIB_WG; it++) {
        const int64_t i = base + (int64_t)it * CALIB_WG;
        if (i < n) {
            double z = th.v[S];
#pragma unroll
            for (int s = 0; s < S; s++) z = fma(th.v[s], X[(int64_t)s * n + i], z);
            out[i] = z;
        }
    }
}

// counts [n_blocks][2][16]: misses, then false alarms, of the block's trials at each threshold.  Accept iff llr >= thr.
__global__ __launch_bounds__(CALIB_WG) void calib_counts_kernel(const double *__restrict__ llr, const signed char *__restrict__ lab, int64_t n,
                                                                 CalibThr thr, int *__restrict__ counts) {
    __shared__ int red[CALIB_WAVES][2 * CALIB_MAX_THR];
    int miss[CALIB_MAX_THR], fa[CALIB_MAX_THR];
#pragma unroll
    for (int j = 0; j < CALIB_MAX_THR; j++) miss[j] = fa[j] = 0;
    const int64_t base = (int64_t)blockIdx.x * CALIB_BLOCK + threadIdx.x;
#pragma unroll 1
    for (int it = 0; it < CALIB_BLOCK / CALIB_WG; it++) {
        const int64_t i = base + (int64_t)it * CALIB_WG;
        const bool in = i < n;
        const int l = in ? (int)lab[i] : -1;
        const bool valid = l >= 0, target = l > 0;
        const double v = in ? llr[i] : 0.0;
        const double x = valid ? v : 0.0;
#pragma unroll
        for (int j = 0; j < CALIB_MAX_THR; j++) {
            const bool accept = x >= thr.v[j];
            miss[j] += __popcll(__ballot(valid && target && !accept));
            fa[j] += __popcll(__ballot(valid && !target && accept));
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < CALIB_MAX_THR; j++) red[threadIdx.x >> 6][j] = miss[j], red[threadIdx.x >> 6][CALIB_MAX_THR + j] = fa[j];
    }
    __syncthreads();
    if (threadIdx.x < 2 * CALIB_MAX_THR)
        counts[(int64_t)blockIdx.x * 2 * CALIB_MAX_THR + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// ---- host ----

static std::atomic<long> &calib_scratch_option() {
    static std::atomic<long> v{(long)(CALIB_DEFAULT_SCRATCH >> 20)};
    return v;
}
void set_calib_scratch_mib(long v) { calib_scratch_option().store(v); }
long calib_scratch_mib() { return calib_scratch_option().load(); }

namespace {
struct CalibScratch {
    DevBuf<double> X, partial, state, out;
    DevBuf<signed char> lab;
    DevBuf<int> counts;
    PinnedBuf<double> stop;
};
}  // namespace

#define SR_CALIB_BY_S(S, CALL)                                           \
    switch (S) {                                                         \
        case 1: { constexpr int kS = 1; CALL; } break;                   \
        case 2: { constexpr int kS = 2; CALL; } break;                   \
        case 3: { constexpr int kS = 3; CALL; } break;                   \
        case 4: { constexpr int kS = 4; CALL; } break;                   \
        case 5: { constexpr int kS = 5; CALL; } break;                   \
        case 6: { constexpr int kS = 6; CALL; } break;                   \
        case 7: { constexpr int kS = 7; CALL; } break;                   \
        case 8: { constexpr int kS = 8; CALL; } break;                   \
        default: fail("calibration: no kernel for S = %d", S);           \
    }

static void launch_pass(hipStream_t st, int S, const CalibPlan &pl, const CalibScratch &w, double tau, double c_t, double c_n) {
    ScopedKernelTimer tm(T_JFA_GEMM_A);
    SR_CALIB_BY_S(S, hipLaunchKernelGGL(calib_pass_kernel<kS>, dim3((unsigned)pl.pass_grid), dim3(CALIB_WG), 0, st, w.X.p, w.lab.p, pl.n, w.state.p,
                                        tau, c_t, c_n, w.partial.p));
    SR_HIP(hipGetLastError());
}

static void launch_step(hipStream_t st, int S, const CalibPlan &pl, const CalibScratch &w, double ridge, double tol, int mode) {
    ScopedKernelTimer tm(T_JFA_FACTOR);
    SR_CALIB_BY_S(S, hipLaunchKernelGGL(calib_step_kernel<kS>, dim3(1), dim3(CALIB_WG), 0, st, w.partial.p, pl.n_blocks, w.state.p, ridge, tol, mode));
    SR_HIP(hipGetLastError());
}

// The refusals every call that reads labelled trials shares, the plan and the bound; nothing of the device.
static CalibPlan calib_prepare(const char *call, int S, int64_t n, int n_thr, const double *X, const int8_t *lab, CalibCounts &cnt) {
    std::string why;
    CalibPlan pl;
    if (!calib_check_shape(S, n, why)) fail("%s", why.c_str());
    if (!X) fail("calibration: null argument (%s)", S == 1 && n_thr ? "llr, the scores [n]" : "X, the scores [S][n]");
    if (!calib_check_trials(S, n, X, lab, cnt, why)) fail("%s", why.c_str());
    if (!plan_calib(S, n, n_thr, 0, 1, pl, why)) fail("%s", why.c_str());
    if (!calib_check_bound(pl, call, (int64_t)calib_scratch_mib() << 20, why)) fail("%s", why.c_str());
    return pl;
}

static void calib_fill_counts(int64_t *counts, const CalibCounts &c) {
    if (counts) counts[0] = c.n_t, counts[1] = c.n_n, counts[2] = c.n_skip;
}

void calib_train(int S, int64_t n, const double *X, const int8_t *lab, double prior, double ridge, double tol, int max_pass, const double *theta0,
                 int resume, double *state, int64_t *counts) {
    std::string why;
    if (!calib_check_shape(S, n, why)) fail("%s", why.c_str());
    if (!calib_check_params(prior, ridge, tol, max_pass, why)) fail("%s", why.c_str());
    if (!state) fail("calibration: null argument (state, the %d doubles sr_calib_plan reports)", calib_state_len(S));
    if (theta0 && !calib_check_theta(S, theta0, "theta0", why)) fail("%s", why.c_str());
    CalibCounts cnt;
    const CalibPlan pl = calib_prepare("train", S, n, 0, X, lab, cnt);
    std::vector<double> hs((size_t)pl.state_len, 0.0);
    if (resume) {
        std::memcpy(hs.data(), state, sizeof(double) * hs.size());
        if (hs[CALIB_ST_S] != (double)S || hs[CALIB_ST_STOP] != (double)CALIB_CAP || !(hs[CALIB_ST_PASSES] >= 1.0) ||
            !(hs[CALIB_ST_PASSES] <= 1e9))
            fail("calibration: resume needs the state of a call with the same S that ended by CAP (stop code 1); this one holds S = %g, "
                 "stop code %g", hs[CALIB_ST_S], hs[CALIB_ST_STOP]);
        for (double v : hs)
            if (!std::isfinite(v)) fail("calibration: the state to resume from holds a non-finite value");
        hs[CALIB_ST_CAP] = hs[CALIB_ST_PASSES] + (double)max_pass;
    } else {
        hs[CALIB_ST_T] = 1.0;
        hs[CALIB_ST_CAP] = (double)max_pass;
        hs[CALIB_ST_S] = (double)S;
        for (int s = 0; s <= S; s++) hs[(size_t)(calib_off_theta(S) + s)] = hs[(size_t)(calib_off_trial(S) + s)] = theta0 ? theta0[s] : 0.0;
    }
    hs[CALIB_ST_STOP] = -1.0;
    hs[CALIB_ST_NT] = (double)cnt.n_t, hs[CALIB_ST_NN] = (double)cnt.n_n, hs[CALIB_ST_SKIP] = (double)cnt.n_skip;
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_calib_train");
    ensure_device();
    hipStream_t st = ctx().stream;
    auto &w = per_device<CalibScratch>();
    w.X.upload(X, (size_t)((int64_t)S * n));
    w.lab.upload(reinterpret_cast<const signed char *>(lab), (size_t)n);
    w.state.upload(hs.data(), hs.size());
    w.partial.ensure((size_t)(pl.n_blocks * pl.acc));
    w.stop.ensure(1);
    const double tau = std::log(prior / (1.0 - prior));
    const double c_t = prior / (double)cnt.n_t, c_n = (1.0 - prior) / (double)cnt.n_n;
    for (int it = 0; it < max_pass; it++) {
        launch_pass(st, S, pl, w, tau, c_t, c_n);
        launch_step(st, S, pl, w, ridge, tol, 0);
        if ((it + 1) % CALIB_CADENCE == 0 || it + 1 == max_pass) {
            SR_HIP(hipMemcpyAsync(w.stop.p, w.state.p + CALIB_ST_STOP, sizeof(double), hipMemcpyDeviceToHost, st));
            sync_stream();
            if (w.stop.p[0] >= 0.0) break;
        }
    }
    w.state.download(hs.data(), hs.size());
    sync_stream();
    if (!(hs[CALIB_ST_STOP] >= 0.0)) fail("calibration: the loop ended without a stop code (an internal error)");
    std::memcpy(state, hs.data(), sizeof(double) * hs.size());
    calib_fill_counts(counts, cnt);
}

void calib_eval(int S, int64_t n, const double *X, const int8_t *lab, double prior, double ridge, const double *theta, double *f, double *g,
                double *H, int64_t *counts) {
    std::string why;
    if (!calib_check_shape(S, n, why)) fail("%s", why.c_str());
    if (!calib_check_params(prior, ridge, 0.0, 1, why)) fail("%s", why.c_str());
    if (!theta) fail("calibration: null argument (theta, the S weights and the offset)");
    if (!f) fail("calibration: null argument (f, the objective)");
    if (!calib_check_theta(S, theta, "theta", why)) fail("%s", why.c_str());
    CalibCounts cnt;
    const CalibPlan pl = calib_prepare("train", S, n, 0, X, lab, cnt);
    std::vector<double> hs((size_t)pl.state_len, 0.0);
    hs[CALIB_ST_STOP] = -1.0;
    hs[CALIB_ST_CAP] = 1.0;
    hs[CALIB_ST_S] = (double)S;
    for (int s = 0; s <= S; s++) hs[(size_t)(calib_off_theta(S) + s)] = hs[(size_t)(calib_off_trial(S) + s)] = theta[s];
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_calib_eval");
    ensure_device();
    hipStream_t st = ctx().stream;
    auto &w = per_device<CalibScratch>();
    w.X.upload(X, (size_t)((int64_t)S * n));
    w.lab.upload(reinterpret_cast<const signed char *>(lab), (size_t)n);
    w.state.upload(hs.data(), hs.size());
    w.partial.ensure((size_t)(pl.n_blocks * pl.acc));
    const double c_t = prior / (double)cnt.n_t, c_n = (1.0 - prior) / (double)cnt.n_n;
    launch_pass(st, S, pl, w, std::log(prior / (1.0 - prior)), c_t, c_n);
    launch_step(st, S, pl, w, ridge, 0.0, 1);
    w.state.download(hs.data(), hs.size());
    sync_stream();
    const int P = S + 1;
    *f = hs[CALIB_ST_F];
    if (g)
        for (int k = 0; k < P; k++) g[k] = hs[(size_t)(calib_off_g(S) + k)];
    if (H) {
        int k = calib_off_H(S);
        for (int s = 0; s < P; s++)
            for (int t = s; t < P; t++) H[s * P + t] = H[t * P + s] = hs[(size_t)k++];
    }
    calib_fill_counts(counts, cnt);
}

void calib_apply(int S, int64_t n, const double *X, const double *theta, double *out) {
    std::string why;
    CalibPlan pl;
    if (!calib_check_shape(S, n, why)) fail("%s", why.c_str());
    if (!X) fail("calibration: null argument (X, the scores [S][n])");
    if (!theta) fail("calibration: null argument (theta, the S weights and the offset)");
    if (!out) fail("calibration: null argument (out, the calibrated scores [n])");
    if (!calib_check_theta(S, theta, "theta", why)) fail("%s", why.c_str());
    if (!plan_calib(S, n, 0, 0, 1, pl, why)) fail("%s", why.c_str());
    if (!calib_check_bound(pl, "apply", (int64_t)calib_scratch_mib() << 20, why)) fail("%s", why.c_str());
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_calib_apply");
    ensure_device();
    hipStream_t st = ctx().stream;
    auto &w = per_device<CalibScratch>();
    w.X.upload(X, (size_t)((int64_t)S * n));
    w.out.ensure((size_t)n);
    CalibTheta th = {};
    for (int s = 0; s <= S; s++) th.v[s] = theta[s];
    {
        ScopedKernelTimer tm(T_JFA_UPDATE);
        SR_CALIB_BY_S(S, hipLaunchKernelGGL(calib_apply_kernel<kS>, dim3((unsigned)pl.apply_grid), dim3(CALIB_WG), 0, st, w.X.p, n, th, w.out.p));
        SR_HIP(hipGetLastError());
    }
    w.out.download(out, (size_t)n);
    sync_stream();
}

void calib_counts(int64_t n, const double *llr, const int8_t *lab, int m, const double *thr, int64_t *miss, int64_t *fa, int64_t *counts) {
    std::string why;
    if (!calib_check_shape(1, n, why)) fail("%s", why.c_str());
    if (!calib_check_thresholds(m, thr, why)) fail("%s", why.c_str());
    if (!miss || !fa) fail("calibration: null argument (miss and fa, the counts [m])");
    CalibCounts cnt;
    const CalibPlan pl = calib_prepare("counts", 1, n, m, llr, lab, cnt);
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_calib_counts");
    ensure_device();
    hipStream_t st = ctx().stream;
    auto &w = per_device<CalibScratch>();
    w.X.upload(llr, (size_t)n);
    w.lab.upload(reinterpret_cast<const signed char *>(lab), (size_t)n);
    const size_t nc = (size_t)(pl.n_blocks * 2 * CALIB_MAX_THR);
    w.counts.ensure(nc);
    CalibThr t;
    for (int j = 0; j < CALIB_MAX_THR; j++) t.v[j] = j < m ? thr[j] : HUGE_VAL;
    {
        ScopedKernelTimer tm(T_JFA_UPDATE);
        hipLaunchKernelGGL(calib_counts_kernel, dim3((unsigned)pl.counts_grid), dim3(CALIB_WG), 0, st, w.X.p, w.lab.p, n, t, w.counts.p);
        SR_HIP(hipGetLastError());
    }
    std::vector<int> host(nc);
    w.counts.download(host.data(), nc);
    sync_stream();
    for (int j = 0; j < m; j++) miss[j] = fa[j] = 0;
    for (int64_t b = 0; b < pl.n_blocks; b++)
        for (int j = 0; j < m; j++) {
            miss[j] += host[(size_t)(b * 2 * CALIB_MAX_THR + j)];
            fa[j] += host[(size_t)(b * 2 * CALIB_MAX_THR + CALIB_MAX_THR + j)];
        }
    calib_fill_counts(counts, cnt);
}

}  // namespace sr
