// jfa_score.hip -- the score matrix of a JFA verification run on the device: J models (their factors y, z) against T test segments
// (their raw statistics N, F), by the reference's two scorers (src/jfa/; MATLAB there, a loop over segments and models on the host):
//   integrated (kscore_famous_19.m)  the likelihood with the channel factors integrated out.  M_0 = m, M_j = m + z_j .* d + y_j v:
//       lin[t][j]  = sum_i F[t][i] M_j[i] / E[i]           quad[t][j] = sum_c N[t][c] q[j][c],   q[j][c] = sum_d M_j[c,d]^2 / E[c,d]
//       L_t        = I + sum_c N[t][c] P_c                 a_t        = u (F[t] ./ E)
//       h[t][j]    = sum_c N[t][c] G[c][j],                G[c][j]    = u_c (M_j,c ./ E_c)
//       quad2      = || chol(L_t)^-1 (a_t - h[t][j]) ||^2  s          = (lin - quad / 2 + quad2 / 2) / n_t     out[j-1][t] = s[t][j] - s[t][0]
//     The reference forms u' (N_t ./ E .* M_j) per pair (K D Ru operations); G is formed once per call and h for all pairs of a chunk
//     is ONE product N [n x K] G [K x Ru (J + 1)]: K Ru operations a pair.
//   linear (linear_scoring.m)        out[j][t] = sum_i ((z_j .* d + y_j v)[i] / E[i]) (F[t][i] - N[t][c(i)] (m + x_t u)[i]) / n_t.
// Float64 throughout.  Every product goes through the dense layer's GEMM (dense64.hpp), the scalings and P through jfa.hip's scale
// and gram kernels (jfa_dev.hpp); the kernels here:
//   jfa_synth_kernel       M = [m;] (m +) z .* d + y v over the product y v, elementwise.
//   jfa_cross_kernel       q and G: a 16 x 16 tile (channel factors x models) of one mixture per workgroup, as the gram kernel; G is laid
//                          out [c][r][j], models fastest, so that h [t][r][j] has the models contiguous for the substitution.
//   jfa_kscore_kernel      one workgroup per test segment: the panel Cholesky of L_t (dense64_dev.hpp; in LDS up to jfa_lds_rows rows, in
//                          place above), then ONE forward substitution over all J + 1 right-hand sides a_t - h[t][.][j], a lane per
//                          model walking its column row by row, the column norms, the scores and the subtraction of column 0.
//   jfa_compensate_kernel  linear mode's (F - N (m + x u)) / n_t over the product x u, elementwise.
// Deterministic: no atomics; a pair's score depends on its segment's N, F and its model's y, z only (the GEMM's rows and columns are
// independent, a segment has its own workgroup, a model its own lane): the same bits alone and in any batch, under any scratch bound.
// Degenerate inputs: a segment with n_t = 0 gets a row of zeros (the reference divides by zero); a segment whose L_t does not factor
// gets zeros and is counted.  Nothing non-finite is spread.
#include "dense64.hpp"
#include "dense64_dev.hpp"
#include "jfa_dev.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace sr {

// M [rows][kd] holds y v in its rows ubm_row .. (row 0 untouched by the product when ubm_row = 1).  z, d: null = zeros.
__global__ __launch_bounds__(JFA_WG)
void jfa_synth_kernel(const double *__restrict__ m, const double *__restrict__ z, const double *__restrict__ d, double *__restrict__ M, int64_t n,
                      int64_t kd, int ubm_row) {
    const int64_t i = (int64_t)blockIdx.x * JFA_WG + threadIdx.x;
    if (i >= n) return;
    const int64_t r = i / kd, c = i % kd;
    if (ubm_row && r == 0) {
        M[i] = m[c];
        return;
    }
    double val = M[i];
    if (z && d) val = __builtin_fma(z[(r - ubm_row) * kd + c], d[c], val);
    if (ubm_row) val += m[c];
    M[i] = val;
}

// ---- q [J1][K] and G [K][Ru][J1].  grid (K, tiles of 16 models, tiles of 16 channel factors) ----
__global__ __launch_bounds__(JFA_WG)
void jfa_cross_kernel(const double *__restrict__ u, const double *__restrict__ M, const double *__restrict__ ME, double *__restrict__ q,
                      double *__restrict__ G, int Ru, int64_t J1, int K, int D) {
    __shared__ double wu[JFA_GRAM_TILE][JFA_GRAM_DSTEP + 1], wm[JFA_GRAM_TILE][JFA_GRAM_DSTEP + 1], wme[JFA_GRAM_TILE][JFA_GRAM_DSTEP + 1];
    const int tid = threadIdx.x;
    const int c = blockIdx.x;
    const int64_t tj = blockIdx.y;
    const int ti = blockIdx.z;
    const int li = tid >> 4, lj = tid & 15;
    const int64_t kd = (int64_t)K * D;
    double acc = 0.0, accq = 0.0;
    for (int d0 = 0; d0 < D; d0 += JFA_GRAM_DSTEP) {
        const int nd = min(JFA_GRAM_DSTEP, D - d0);
        __syncthreads();                       // the previous dimensions have been read by every lane
        for (int e = tid; e < JFA_GRAM_TILE * JFA_GRAM_DSTEP; e += JFA_WG) {
            const int r = e / JFA_GRAM_DSTEP, dd = e % JFA_GRAM_DSTEP;
            const int gi = ti * JFA_GRAM_TILE + r;
            const int64_t gj = tj * JFA_GRAM_TILE + r;
            const int64_t col = (int64_t)c * D + d0 + dd;
            wu[r][dd] = (gi < Ru && dd < nd) ? u[(int64_t)gi * kd + col] : 0.0;
            wme[r][dd] = (gj < J1 && dd < nd) ? ME[gj * kd + col] : 0.0;
            if (ti == 0) wm[r][dd] = (gj < J1 && dd < nd) ? M[gj * kd + col] : 0.0;
        }
        __syncthreads();
        for (int dd = 0; dd < nd; dd++) acc = __builtin_fma(wu[li][dd], wme[lj][dd], acc);
        if (ti == 0 && li == 0)
            for (int dd = 0; dd < nd; dd++) accq = __builtin_fma(wm[lj][dd], wme[lj][dd], accq);
    }
    const int i = ti * JFA_GRAM_TILE + li;
    const int64_t j = tj * JFA_GRAM_TILE + lj;
    if (i < Ru && j < J1) G[((int64_t)c * Ru + i) * J1 + j] = acc;
    if (ti == 0 && li == 0 && j < J1) q[j * K + c] = accq;
}

// ---- one workgroup per test segment of a chunk.  L [n][Ru][Ru] and h [n][Ru][J1] are the chunk's; a [T][Ru], lin / quad [T][J1], nt [T],
// flags [T], out [J][T] are the call's, addressed by t = t0 + block.  lin is overwritten by the scores s[t][j]. ----
__global__ __launch_bounds__(JFA_WG)
void jfa_kscore_kernel(double *__restrict__ L, int Ru, int use_lds, const double *__restrict__ a, double *__restrict__ h, double *__restrict__ lin,
                       const double *__restrict__ quad, const double *__restrict__ nt, int64_t J1, int64_t T, int64_t t0,
                       double *__restrict__ out, int *__restrict__ flags) {
    extern __shared__ double jfa_score_lds[];
    double *pan = jfa_score_lds;               // [Ru][DENSE_PS]
    double *s0 = pan + (size_t)Ru * DENSE_PS;    // [2 Ru] spare: the UBM's score in its first element
    double *mat = s0 + 2 * Ru;                 // [Ru][Ru], LDS path only
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x, t = t0 + g;
    const int rr = Ru * Ru;
    const double n = nt[t];
    double *Mg = L + g * rr;
    double *Mf = Mg;
    bool ok = n > 0.0;
    if (ok) {
        if (use_lds) {
            for (int e = tid; e < rr; e += JFA_WG) mat[e] = Mg[e];
            Mf = mat;
            __syncthreads();
        }
        ok = dense_cholesky(Mf, Ru, pan);
        __syncthreads();
        if (tid == 0) flags[t] = ok ? 0 : 1;
    } else if (tid == 0) {
        flags[t] = 0;
    }
    if (!ok) {                                 // (uniform: n and the pivots are the same for every lane)
        for (int64_t j = 1 + tid; j < J1; j += JFA_WG) out[(j - 1) * T + t] = 0.0;
        return;
    }
    double *hb = h + g * Ru * J1;
    const double *ag = a + t * Ru;
    for (int64_t j = tid; j < J1; j += JFA_WG) {
        double nrm = 0.0;
        for (int r = 0; r < Ru; r++) {
            const double *Lr = Mf + (int64_t)r * Ru;
            double s = ag[r] - hb[r * J1 + j];
            for (int k = 0; k < r; k++) s = __builtin_fma(-Lr[k], hb[k * J1 + j], s);
            s /= Lr[r];
            hb[r * J1 + j] = s;
            nrm = __builtin_fma(s, s, nrm);
        }
        const double score = (lin[t * J1 + j] - 0.5 * quad[t * J1 + j] + 0.5 * nrm) / n;
        lin[t * J1 + j] = score;
        if (j == 0) s0[0] = score;
    }
    __syncthreads();
    const double ubm = s0[0];
    for (int64_t j = 1 + tid; j < J1; j += JFA_WG) out[(j - 1) * T + t] = lin[t * J1 + j] - ubm;
}

// xu [T][kd] holds x u; -> (F - N (m + x u)) / n_t, zeros for a segment of no frames.
__global__ __launch_bounds__(JFA_WG)
void jfa_compensate_kernel(const double *__restrict__ F, const double *__restrict__ N, const double *__restrict__ m, double *__restrict__ xu,
                           const double *__restrict__ nt, int64_t n, int K, int D) {
    const int64_t i = (int64_t)blockIdx.x * JFA_WG + threadIdx.x;
    if (i >= n) return;
    const int64_t kd = (int64_t)K * D, t = i / kd, c = i % kd;
    const double nn = nt[t];
    xu[i] = nn > 0.0 ? (F[i] - N[t * K + c / D] * (m[c] + xu[i])) / nn : 0.0;
}

// ---- host ----

namespace {
struct JfaScoreScratch {
    DevBuf<double> N, F, m, iE, d, v, u, z, y, x, nt;
    DevBuf<double> M, ME, uE, P, q, G, lin, quad, a, out, L, h;
    DevBuf<int> flags;
};
}  // namespace

static void launch_kscore(hipStream_t st, const JfaScorePlan &pl, int64_t n, double *L, int Ru, const double *a, double *h, double *lin,
                          const double *quad, const double *nt, int64_t J1, int64_t T, int64_t t0, double *out, int *flags) {
    static int attr_set[MAX_DEVICES] = {};
    if (attr_set[ctx().device] < pl.kscore_lds) {
        SR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&jfa_kscore_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, pl.kscore_lds));
        attr_set[ctx().device] = pl.kscore_lds;
    }
    ScopedKernelTimer tm(T_JFA_FACTOR);
    hipLaunchKernelGGL(jfa_kscore_kernel, dim3((unsigned)n), dim3(JFA_WG), (size_t)pl.kscore_lds, st, L, Ru, pl.path == 0 ? 1 : 0, a, h, lin, quad, nt,
                       J1, T, t0, out, flags);
    SR_HIP(hipGetLastError());
}

void jfa_score(int mode, int64_t T, int64_t J, int K, int D, int Ry, int Ru, const double *N, const double *F, const double *m, const double *E,
               const double *d, const double *v, const double *u, const double *z, const double *y, const double *x, const unsigned char *mask,
               int64_t mask_rows, int64_t mask_cols, double *out, int64_t *empty_segments, int64_t *bad_segments) {
    const char *what = mode == JFA_SCORE_LINEAR ? "sr_jfa_score_linear" : "sr_jfa_score_integrated";
    std::string why;
    if (!jfa_score_check_inputs(T, J, K, D, Ry, Ru, mode, N, F, m, E, d, v, u, z, y, x, mask, mask_rows, mask_cols, why)) fail("%s", why.c_str());
    if (!out) fail("%s: null argument (the score matrix)", what);
    JfaScorePlan pl;
    if (!plan_jfa_score(T, J, K, D, Ry, Ru, mode, (int64_t)jfa_scratch_mib() << 20, (int)jfa_lds_rows(), 1, pl, why)) fail("%s", why.c_str());
    if (gpu_runtime_lost()) fail_gpu_runtime_lost(what);
    ensure_device();
    if (!plan_jfa_score(T, J, K, D, Ry, Ru, mode, (int64_t)jfa_scratch_mib() << 20, (int)jfa_lds_rows(), std::max(1, ctx().n_cu), pl, why))
        fail("%s", why.c_str());
    const int64_t kd = (int64_t)K * D;
    std::vector<double> nt((size_t)T);
    int64_t empty = 0;
    for (int64_t t = 0; t < T; t++) {          // in mixture order: a segment's n_t does not depend on the batch
        double s = 0.0;
        for (int c = 0; c < K; c++) s += N[t * K + c];
        nt[(size_t)t] = s;
        empty += !(s > 0.0);
    }
    auto &w = per_device<JfaScoreScratch>();
    w.N.upload(N, (size_t)(T * K));
    w.F.upload(F, (size_t)(T * kd));
    w.nt.upload(nt.data(), (size_t)T);
    jfa_score_device(pl, T, J, K, D, Ry, Ru, w.N.p, w.F.p, w.nt.p, m, E, d, v, u, z, y, x, mask, out, bad_segments);
    if (empty_segments) *empty_segments = empty;
}

// The launches, on statistics and totals that are on the device already: the host-array entry above has just uploaded them, the
// entries on a statistics handle (jfa_stats.hip) pass the handle's own buffers.  Synchronises before it returns.
void jfa_score_device(const JfaScorePlan &pl, int64_t T, int64_t J, int K, int D, int Ry, int Ru, const double *dN, const double *dF,
                      const double *d_nt, const double *m, const double *E, const double *d, const double *v, const double *u, const double *z,
                      const double *y, const double *x, const unsigned char *mask, double *out, int64_t *bad_segments) {
    const int mode = pl.mode;
    const int64_t kd = (int64_t)K * D, rr = (int64_t)Ru * Ru, J1 = J + 1;
    std::vector<double> ie((size_t)kd);
    for (int64_t i = 0; i < kd; i++) ie[(size_t)i] = 1.0 / E[i];
    hipStream_t st = ctx().stream;
    auto &w = per_device<JfaScoreScratch>();
    const bool integrated = mode == JFA_SCORE_INTEGRATED;
    const int ubm_row = integrated ? 1 : 0;
    const int64_t rows = J + ubm_row;
    w.m.upload(m, (size_t)kd);
    w.iE.upload(ie.data(), (size_t)kd);
    if (d) w.d.upload(d, (size_t)kd);
    w.v.upload(v, (size_t)(Ry * kd));
    w.u.upload(u, (size_t)(Ru * kd));
    if (z) w.z.upload(z, (size_t)(J * kd));
    w.y.upload(y, (size_t)(J * Ry));
    w.M.ensure((size_t)(rows * kd));
    w.ME.ensure((size_t)(rows * kd));
    w.out.ensure((size_t)(J * T));
    // the models: y v, then m + z .* d (row 0 = m in integrated mode), then ./ E
    dense_gemm(T_JFA_GEMM_C, st, w.y.p, Ry, 1, w.v.p, kd, 1, w.M.p + ubm_row * kd, kd, J, kd, Ry, false, 0);
    {
        ScopedKernelTimer tm(T_JFA_GRAM);
        hipLaunchKernelGGL(jfa_synth_kernel, dim3((unsigned)((rows * kd + JFA_WG - 1) / JFA_WG)), dim3(JFA_WG), 0, st, w.m.p,
                           (z && d) ? w.z.p : nullptr, (z && d) ? w.d.p : nullptr, w.M.p, rows * kd, kd, ubm_row);
        SR_HIP(hipGetLastError());
        launch_scale(st, w.M.p, w.iE.p, w.ME.p, rows * kd, kd);
    }
    int64_t bad = 0;
    if (integrated) {
        w.uE.ensure((size_t)(Ru * kd));
        w.P.ensure((size_t)(K * rr));
        w.q.ensure((size_t)(J1 * K));
        w.G.ensure((size_t)(K * Ru * J1));
        w.lin.ensure((size_t)(T * J1));
        w.quad.ensure((size_t)(T * J1));
        w.a.ensure((size_t)(T * Ru));
        w.L.ensure((size_t)(pl.chunk * rr));
        w.h.ensure((size_t)(pl.chunk * Ru * J1));
        w.flags.ensure((size_t)T);
        {
            ScopedKernelTimer tm(T_JFA_GRAM);
            launch_scale(st, w.u.p, w.iE.p, w.uE.p, Ru * kd, kd);
            launch_gram(st, w.u.p, w.iE.p, w.P.p, Ru, K, D);
            hipLaunchKernelGGL(jfa_cross_kernel, dim3((unsigned)pl.cross.x, (unsigned)pl.cross.y, (unsigned)pl.cross_z), dim3(JFA_WG), 0, st, w.u.p,
                               w.M.p, w.ME.p, w.q.p, w.G.p, Ru, J1, K, D);
            SR_HIP(hipGetLastError());
        }
        for (int64_t ci = 0; ci < pl.n_chunks; ci++) {
            const int64_t t0 = ci * pl.chunk, n = std::min(pl.chunk, T - t0);
            const double *Nc = dN + t0 * K, *Fc = dF + t0 * kd;
            dense_gemm(T_JFA_GEMM_L, st, Nc, K, 1, w.P.p, rr, 1, w.L.p, rr, n, rr, K, false, Ru + 1);                        // L = I + N P
            dense_gemm(T_JFA_GEMM_B, st, Fc, kd, 1, w.uE.p, 1, kd, w.a.p + t0 * Ru, Ru, n, Ru, kd, false, 0);                // a = F (u ./ E)^T
            dense_gemm(T_JFA_GEMM_B, st, Fc, kd, 1, w.ME.p, 1, kd, w.lin.p + t0 * J1, J1, n, J1, kd, false, 0);              // lin = F (M ./ E)^T
            dense_gemm(T_JFA_GEMM_A, st, Nc, K, 1, w.q.p, 1, K, w.quad.p + t0 * J1, J1, n, J1, K, false, 0);                 // quad = N q^T
            dense_gemm(T_JFA_GEMM_A, st, Nc, K, 1, w.G.p, Ru * J1, 1, w.h.p, Ru * J1, n, Ru * J1, K, false, 0);              // h = N G
            launch_kscore(st, pl, n, w.L.p, Ru, w.a.p, w.h.p, w.lin.p, w.quad.p, d_nt, J1, T, t0, w.out.p, w.flags.p);
        }
        std::vector<int> host((size_t)T);
        SR_HIP(hipMemcpyAsync(host.data(), w.flags.p, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, st));
        w.out.download(out, (size_t)(J * T));
        sync_stream();
        for (int64_t t = 0; t < T; t++) bad += host[(size_t)t] != 0;
    } else {
        w.x.upload(x, (size_t)(T * Ru));
        w.h.ensure((size_t)(T * kd));          // the compensated statistics
        dense_gemm(T_JFA_GEMM_C, st, w.x.p, Ru, 1, w.u.p, kd, 1, w.h.p, kd, T, kd, Ru, false, 0);                            // x u
        {
            ScopedKernelTimer tm(T_JFA_GRAM);
            hipLaunchKernelGGL(jfa_compensate_kernel, dim3((unsigned)((T * kd + JFA_WG - 1) / JFA_WG)), dim3(JFA_WG), 0, st, dF, dN, w.m.p, w.h.p,
                               d_nt, T * kd, K, D);
            SR_HIP(hipGetLastError());
        }
        dense_gemm(T_JFA_GEMM_B, st, w.ME.p, kd, 1, w.h.p, 1, kd, w.out.p, T, J, T, kd, false, 0);                           // out = (M ./ E) Fc^T
        w.out.download(out, (size_t)(J * T));
        sync_stream();
    }
    if (mask)
        for (int64_t i = 0; i < J * T; i++)
            if (!mask[i]) out[i] = 0.0;
    if (bad_segments) *bad_segments = bad;
}

}  // namespace sr
