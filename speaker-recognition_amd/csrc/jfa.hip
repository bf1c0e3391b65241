// jfa.hip -- JFA factor estimation on the device: the reference's estimate_y_and_v.m / estimate_x_and_u.m (src/jfa/; MATLAB there, one
// speaker at a time in a loop over mixtures), which are ONE computation on different groups of rows.  For every group g (a speaker,
// or a session) with centred first-order statistics Fc_g, occupancies N[g], variances E and a loading matrix W [R][K D]
// (v, u, or the stacked [v; u]; W_c = the D columns of mixture c):
//   P_c = W_c diag(1 / E_c) W_c^T            L_g = I + sum_c N[g][c] P_c           b_g = W (Fc_g ./ E)
//   y_g = L_g^-1 b_g                         Q_g = L_g^-1 + y_g y_g^T
//   A_c = sum_g N[g][c] Q_g                  C   = sum_g y_g Fc_g^T                W_c <- A_c^-1 C_c
// Everything is float64.  The four products  L = I + N P  (reduction over K),  b = Fc (W ./ E)^T  (over K D),  A += N^T Q  and
// C += Y^T Fc  (over the groups of a chunk) are the dense layer's GEMM (dense64.hpp: strides instead of transposes; an accumulating
// launch continues from what A and C hold).  Three kernels here, none touching the pass counters (trial scoring, jfa_score.hip,
// launches the first two through the launchers declared in jfa_dev.hpp; the Cholesky and the two inverse routines inside the third
// are the layer's, dense64_dev.hpp):
//   jfa_scale_kernel    W ./ E, once per call (the B operand of the b product).
//   jfa_gram_kernel     P [K][R][R]: a 16 x 16 tile of one mixture per workgroup, the two row panels of W_c through LDS; the product
//                       W[i][d] W[j][d] is formed first, so P is symmetric to the bit.
//   jfa_factor_kernel   one workgroup per R x R block: right-looking Cholesky in panels of 16 columns (the panel, all its rows, in
//                       LDS; the trailing update reads it from there), then either (groups) y by two triangular solves, the inverse
//                       of the factor in place row by row, L^-T L^-1 in place, + y y^T, mirrored: Q_g over L_g; or (update) the D
//                       columns of C_c solved in place in W_c.  The block is worked on where it lies in global memory, or, for
//                       R <= jfa_lds_rows, copied into LDS first -- the same code on another pointer.
// Degenerate inputs: a block that does not factor (a pivot <= 0 or not finite) -- a group: y = 0, Q = 0 (it adds nothing to A and
// C) and it is counted; a mixture of the update: W_c keeps its old value and it is counted.  Nothing non-finite is spread.
// Deterministic: no atomics; a group's y depends on its own N, Fc and on W only; A and C are summed in group order whatever the
// chunking -- the results do not depend on the scratch bound, bit for bit.
#include "dense64.hpp"
#include "dense64_dev.hpp"
#include "jfa_dev.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <vector>

namespace sr {

__global__ __launch_bounds__(JFA_WG)
void jfa_scale_kernel(const double *__restrict__ W, const double *__restrict__ iE, double *__restrict__ WE, int64_t n, int64_t kd) {
    const int64_t i = (int64_t)blockIdx.x * JFA_WG + threadIdx.x;
    if (i < n) WE[i] = W[i] * iE[i % kd];
}

// ---- P_c = W_c diag(1 / E_c) W_c^T.  grid (K, tiles of 16 x 16) ----
__global__ __launch_bounds__(JFA_WG)
void jfa_gram_kernel(const double *__restrict__ W, const double *__restrict__ iE, double *__restrict__ P, int R, int K, int D) {
    __shared__ double wi[JFA_GRAM_TILE][JFA_GRAM_DSTEP + 1], wj[JFA_GRAM_TILE][JFA_GRAM_DSTEP + 1], ie[JFA_GRAM_DSTEP];
    const int tid = threadIdx.x;
    const int c = blockIdx.x;
    const int gt = (R + JFA_GRAM_TILE - 1) / JFA_GRAM_TILE;
    const int ti = blockIdx.y / gt, tj = blockIdx.y % gt;
    const int li = tid >> 4, lj = tid & 15;
    const int64_t kd = (int64_t)K * D;
    double acc = 0.0;
    for (int d0 = 0; d0 < D; d0 += JFA_GRAM_DSTEP) {
        const int nd = min(JFA_GRAM_DSTEP, D - d0);
        __syncthreads();                       // the previous dimensions have been read by every lane
        for (int e = tid; e < JFA_GRAM_TILE * JFA_GRAM_DSTEP; e += JFA_WG) {
            const int r = e / JFA_GRAM_DSTEP, d = e % JFA_GRAM_DSTEP;
            const int gi = ti * JFA_GRAM_TILE + r, gj = tj * JFA_GRAM_TILE + r;
            const int64_t col = (int64_t)c * D + d0 + d;
            wi[r][d] = (gi < R && d < nd) ? W[(int64_t)gi * kd + col] : 0.0;
            wj[r][d] = (gj < R && d < nd) ? W[(int64_t)gj * kd + col] : 0.0;
        }
        if (tid < JFA_GRAM_DSTEP) ie[tid] = tid < nd ? iE[(int64_t)c * D + d0 + tid] : 0.0;
        __syncthreads();
        for (int d = 0; d < nd; d++) acc = __builtin_fma(wi[li][d] * wj[lj][d], ie[d], acc);
    }
    const int i = ti * JFA_GRAM_TILE + li, j = tj * JFA_GRAM_TILE + lj;
    if (i < R && j < R) P[((int64_t)c * R + i) * R + j] = acc;
}

// T [R][nrhs] (row stride ldt; LDS or global memory) <- (F F^T)^-1 T with the factor F in M's lower triangle: two triangular solves.
static __device__ void jfa_solve(const double *M, int R, double *T, int64_t ldt, int nrhs) {
    const int tid = threadIdx.x;
    for (int j = 0; j < R; j++) {
        const double djj = M[(int64_t)j * R + j];
        for (int r = tid; r < nrhs; r += JFA_WG) T[j * ldt + r] /= djj;
        __syncthreads();
        const int64_t n = (int64_t)(R - j - 1) * nrhs;
        for (int64_t e = tid; e < n; e += JFA_WG) {
            const int i = j + 1 + (int)(e / nrhs), r = (int)(e % nrhs);
            T[i * ldt + r] = __builtin_fma(-M[(int64_t)i * R + j], T[j * ldt + r], T[i * ldt + r]);
        }
        __syncthreads();
    }
    for (int j = R - 1; j >= 0; j--) {
        const double djj = M[(int64_t)j * R + j];
        for (int r = tid; r < nrhs; r += JFA_WG) T[j * ldt + r] /= djj;
        __syncthreads();
        const int64_t n = (int64_t)j * nrhs;
        for (int64_t e = tid; e < n; e += JFA_WG) {
            const int i = (int)(e / nrhs), r = (int)(e % nrhs);
            T[i * ldt + r] = __builtin_fma(-M[(int64_t)j * R + i], T[j * ldt + r], T[i * ldt + r]);
        }
        __syncthreads();
    }
}

// mode 0 (groups): blocks = L [n][R][R] -> Q, rhs = b [n][R], out = y [n][R].
// mode 1 (update): blocks = A [K][R][R] (destroyed), rhs = C [R][K D], out = W [R][K D] (rhs_ld = K D), block c owns columns c D ..
__global__ __launch_bounds__(JFA_WG)
void jfa_factor_kernel(double *__restrict__ blocks, int R, int use_lds, int mode, const double *__restrict__ rhs, int64_t rhs_ld,
                       double *__restrict__ out, int D, int *__restrict__ flags) {
    extern __shared__ double jfa_lds[];
    double *pan = jfa_lds;                     // [R][DENSE_PS]
    double *t = pan + (size_t)R * DENSE_PS;      // [R]
    double *buf = t + R;                       // [R]
    double *mat = buf + R;                     // [R][R], LDS path only
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    const int rr = R * R;
    double *Mg = blocks + g * rr;
    double *M = Mg;
    if (use_lds) {
        for (int e = tid; e < rr; e += JFA_WG) mat[e] = Mg[e];
        M = mat;
        __syncthreads();
    }
    const bool ok = dense_cholesky(M, R, pan);
    __syncthreads();
    if (mode == 0) {
        double *yg = out + g * R;
        if (!ok) {
            for (int e = tid; e < rr; e += JFA_WG) Mg[e] = 0.0;
            for (int i = tid; i < R; i += JFA_WG) yg[i] = 0.0;
            if (tid == 0) flags[g] = 1;
            return;
        }
        for (int i = tid; i < R; i += JFA_WG) t[i] = rhs[g * R + i];
        __syncthreads();
        jfa_solve(M, R, t, 1, 1);
        for (int i = tid; i < R; i += JFA_WG) yg[i] = t[i];
        dense_tri_inverse(M, R, buf);
        dense_inverse_from_tri(M, R, buf, t);
        if (use_lds)
            for (int e = tid; e < rr; e += JFA_WG) Mg[e] = mat[e];
        if (tid == 0) flags[g] = 0;
    } else {
        if (!ok) {
            if (tid == 0) flags[g] = 1;
            return;
        }
        double *Wc = out + g * D;
        const double *Cc = rhs + g * D;
        for (int e = tid; e < R * D; e += JFA_WG) {
            const int i = e / D, d = e % D;
            Wc[i * rhs_ld + d] = Cc[i * rhs_ld + d];
        }
        __syncthreads();
        jfa_solve(M, R, Wc, rhs_ld, D);
        if (tid == 0) flags[g] = 0;
    }
}

// ---- host ----

static std::atomic<long> &jfa_scratch_option() {
    static std::atomic<long> v{(long)(JFA_DEFAULT_SCRATCH >> 20)};
    return v;
}
static std::atomic<long> &jfa_lds_option() {
    static std::atomic<long> v{0};
    return v;
}
void set_jfa_scratch_mib(long v) { jfa_scratch_option().store(v); }
long jfa_scratch_mib() { return jfa_scratch_option().load(); }
void set_jfa_lds_rows(long v) { jfa_lds_option().store(v); }
long jfa_lds_rows() { return jfa_lds_option().load(); }

namespace {
struct JfaUpdateScratch {
    DevBuf<double> A, C, W;
    DevBuf<int> flags;
};
}  // namespace

void launch_scale(hipStream_t st, const double *W, const double *iE, double *WE, int64_t n, int64_t kd) {
    hipLaunchKernelGGL(jfa_scale_kernel, dim3((unsigned)((n + JFA_WG - 1) / JFA_WG)), dim3(JFA_WG), 0, st, W, iE, WE, n, kd);
    SR_HIP(hipGetLastError());
}

void launch_gram(hipStream_t st, const double *W, const double *iE, double *P, int R, int K, int D) {
    const int64_t gt = (R + JFA_GRAM_TILE - 1) / JFA_GRAM_TILE;
    hipLaunchKernelGGL(jfa_gram_kernel, dim3((unsigned)K, (unsigned)(gt * gt)), dim3(JFA_WG), 0, st, W, iE, P, R, K, D);
    SR_HIP(hipGetLastError());
}

static void launch_factor(hipStream_t st, TimerKind kind, int64_t n, double *blocks, int R, int path, int mode, const double *rhs,
                          int64_t rhs_ld, double *out, int D, int *flags) {
    static int attr_set[MAX_DEVICES] = {};
    const int lds = jfa_factor_lds_bytes(R, path);
    if (attr_set[ctx().device] < lds) {
        SR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&jfa_factor_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        attr_set[ctx().device] = lds;
    }
    ScopedKernelTimer t(kind);
    hipLaunchKernelGGL(jfa_factor_kernel, dim3((unsigned)n), dim3(JFA_WG), (size_t)lds, st, blocks, R, path == 0 ? 1 : 0, mode, rhs, rhs_ld,
                       out, D, flags);
    SR_HIP(hipGetLastError());
}

static JfaPlan jfa_plan_or_fail(int64_t G, int K, int D, int R) {
    JfaPlan pl;
    std::string why;
    if (!plan_jfa(G, K, D, R, (int64_t)jfa_scratch_mib() << 20, (int)jfa_lds_rows(), std::max(1, ctx().n_cu), pl, why)) fail("%s", why.c_str());
    return pl;
}

// the device stages of one factors pass on h.W; y -> h.Y, with `accumulate` A -> h.A and C -> h.C, the groups' flags -> h.flags
static void jfa_run_factors(SRJfa &h, int R, bool accumulate, const JfaPlan &pl) {
    const int K = h.K, D = h.D;
    const int64_t G = h.G, kd = (int64_t)K * D, rr = (int64_t)R * R;
    hipStream_t st = ctx().stream;
    h.WE.ensure((size_t)(R * kd));
    h.P.ensure((size_t)(K * rr));
    h.Y.ensure((size_t)(G * R));
    h.B.ensure((size_t)(G * R));
    h.L.ensure((size_t)(pl.chunk * rr));
    h.flags.ensure((size_t)std::max<int64_t>(G, K));
    if (accumulate) {
        h.A.ensure((size_t)(K * rr));
        h.C.ensure((size_t)(R * kd));
    }
    {
        ScopedKernelTimer t(T_JFA_GRAM);
        launch_scale(st, h.W.p, h.iE.p, h.WE.p, R * kd, kd);
        launch_gram(st, h.W.p, h.iE.p, h.P.p, R, K, D);
    }
    for (int64_t ci = 0; ci < pl.n_chunks; ci++) {
        const int64_t g0 = ci * pl.chunk, n = std::min(pl.chunk, G - g0);
        dense_gemm(T_JFA_GEMM_L, st, h.N.p + g0 * K, K, 1, h.P.p, rr, 1, h.L.p, rr, n, rr, K, false, R + 1);                 // L = I + N P
        dense_gemm(T_JFA_GEMM_B, st, h.Fc.p + g0 * kd, kd, 1, h.WE.p, 1, kd, h.B.p + g0 * R, R, n, R, kd, false, 0);         // b = Fc (W ./ E)^T
        launch_factor(st, T_JFA_FACTOR, n, h.L.p, R, pl.path, 0, h.B.p + g0 * R, R, h.Y.p + g0 * R, 0, h.flags.p + g0);
        if (accumulate) {
            dense_gemm(T_JFA_GEMM_A, st, h.N.p + g0 * K, 1, K, h.L.p, rr, 1, h.A.p, rr, K, rr, n, ci > 0, 0);                // A += N^T Q
            dense_gemm(T_JFA_GEMM_C, st, h.Y.p + g0 * R, 1, R, h.Fc.p + g0 * kd, kd, 1, h.C.p, kd, R, kd, n, ci > 0, 0);     // C += Y^T Fc
        }
    }
}

static int64_t jfa_count_flags(DevBuf<int> &flags, std::vector<int> &host, int64_t n) {
    host.resize((size_t)n);
    SR_HIP(hipMemcpyAsync(host.data(), flags.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, ctx().stream));
    sync_stream();
    int64_t c = 0;
    for (int64_t i = 0; i < n; i++) c += host[i] != 0;
    return c;
}

void jfa_check_handle(SRJfa &h, const char *what) {
    if (gpu_runtime_lost()) fail_gpu_runtime_lost(what);
    ensure_device();
    if (h.device != ctx().device) fail("%s: the handle lives on device %d, the calling thread is on device %d", what, h.device, ctx().device);
}

SRJfa *jfa_open(int64_t G, int K, int D, const double *N, const double *Fc, const double *E) {
    std::string why;
    if (!jfa_check_stats(G, K, D, N, Fc, E, why)) fail("%s", why.c_str());
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_jfa_open");
    ensure_device();
    const int64_t kd = (int64_t)K * D;
    std::vector<double> ie((size_t)kd);
    for (int64_t i = 0; i < kd; i++) ie[i] = 1.0 / E[i];
    SRJfa *h = new SRJfa();
    try {
        h->G = G;
        h->K = K;
        h->D = D;
        h->device = ctx().device;
        h->N.upload(N, (size_t)(G * K));
        h->Fc.upload(Fc, (size_t)(G * kd));
        h->E.upload(E, (size_t)kd);
        h->iE.upload(ie.data(), (size_t)kd);
        sync_stream();
    } catch (...) {
        delete h;
        throw;
    }
    return h;
}

void jfa_close(SRJfa *h) { delete h; }

void jfa_factors(SRJfa &h, const double *W, int R, double *y, double *A, double *C, int64_t *bad_groups) {
    std::string why;
    if (!jfa_check_rank(R, why)) fail("%s", why.c_str());
    if (!W || !y) fail("sr_jfa_factors: null argument (W and y are required)");
    if ((A == nullptr) != (C == nullptr)) fail("sr_jfa_factors: the accumulators A and C come together or not at all");
    const int64_t kd = (int64_t)h.K * h.D, rr = (int64_t)R * R;
    if (!jfa_check_finite(W, R * kd, "W", why)) fail("%s", why.c_str());
    JfaPlan pl;
    if (!plan_jfa(h.G, h.K, h.D, R, (int64_t)jfa_scratch_mib() << 20, (int)jfa_lds_rows(), 1, pl, why)) fail("%s", why.c_str());
    jfa_check_handle(h, "sr_jfa_factors");
    pl = jfa_plan_or_fail(h.G, h.K, h.D, R);
    h.W.upload(W, (size_t)(R * kd));
    jfa_run_factors(h, R, A != nullptr, pl);
    h.Y.download(y, (size_t)(h.G * R));
    if (A) {
        h.A.download(A, (size_t)(h.K * rr));
        h.C.download(C, (size_t)(R * kd));
    }
    const int64_t bad = jfa_count_flags(h.flags, h.h_flags, h.G);
    if (bad_groups) *bad_groups = bad;
}

static void jfa_check_update(int K, int D, int R, std::string &why) {
    if (!jfa_check_shape(1, K, D, why) || !jfa_check_rank(R, why)) fail("%s", why.c_str());
}

void jfa_update(int K, int D, int R, const double *A, const double *C, double *W, int64_t *skipped) {
    std::string why;
    jfa_check_update(K, D, R, why);
    if (!A || !C || !W) fail("sr_jfa_update: null argument");
    const int64_t kd = (int64_t)K * D, rr = (int64_t)R * R;
    if (!jfa_check_finite(A, K * rr, "A", why) || !jfa_check_finite(C, R * kd, "C", why) || !jfa_check_finite(W, R * kd, "W", why))
        fail("%s", why.c_str());
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_jfa_update");
    ensure_device();
    const JfaPlan pl = jfa_plan_or_fail(1, K, D, R);
    auto &w = per_device<JfaUpdateScratch>();
    w.A.upload(A, (size_t)(K * rr));
    w.C.upload(C, (size_t)(R * kd));
    w.W.upload(W, (size_t)(R * kd));
    w.flags.ensure((size_t)K);
    launch_factor(ctx().stream, T_JFA_UPDATE, K, w.A.p, R, pl.path, 1, w.C.p, kd, w.W.p, D, w.flags.p);
    w.W.download(W, (size_t)(R * kd));
    std::vector<int> host;
    const int64_t s = jfa_count_flags(w.flags, host, K);
    if (skipped) *skipped = s;
}

void jfa_train(SRJfa &h, double *W, int R, int n_iter, double *y, int64_t *skipped) {
    std::string why;
    if (!jfa_check_rank(R, why)) fail("%s", why.c_str());
    if (!W) fail("sr_jfa_train: null argument");
    if (n_iter < 1) fail("sr_jfa_train: n_iter must be >= 1");
    const int64_t kd = (int64_t)h.K * h.D;
    if (!jfa_check_finite(W, R * kd, "W", why)) fail("%s", why.c_str());
    JfaPlan pl;
    if (!plan_jfa(h.G, h.K, h.D, R, (int64_t)jfa_scratch_mib() << 20, (int)jfa_lds_rows(), 1, pl, why)) fail("%s", why.c_str());
    jfa_check_handle(h, "sr_jfa_train");
    pl = jfa_plan_or_fail(h.G, h.K, h.D, R);
    h.W.upload(W, (size_t)(R * kd));
    for (int it = 0; it < n_iter; it++) {
        jfa_run_factors(h, R, true, pl);
        // (a group that did not factor has added zeros: its flag is not needed again, the update reuses the table for its mixtures)
        launch_factor(ctx().stream, T_JFA_UPDATE, h.K, h.A.p, R, pl.path, 1, h.C.p, kd, h.W.p, h.D, h.flags.p);
    }
    h.W.download(W, (size_t)(R * kd));
    if (y) h.Y.download(y, (size_t)(h.G * R));
    const int64_t s = jfa_count_flags(h.flags, h.h_flags, h.K);
    if (skipped) *skipped = s;
}

}  // namespace sr
