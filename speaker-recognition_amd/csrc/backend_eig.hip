// backend_eig.hip -- what the i-vector back end builds on the symmetric eigen-solver (eig.hip), float64 throughout:
//   gen_eig       Sb v = psi Sw v:  L = chol(Sw) (dense_cholesky through plda.hip's block inverse), M = L^-1 Sb L^-T by the triangular
//                 inverse and two products, symmetrised as the mean of its halves, M = Q diag(psi) Q^T by sym_eig_device, V = L^-T Q:
//                 V^T Sw V = I, V^T Sb V = diag(psi), psi descending, the vectors' signs sym_eig's.
//   lda_fit       mu, the within-class covariance Sw about the class means (what kind "wccn" forms) and the between-class covariance
//                 Sb = (1 / n) sum_i n_i (m_i - mu)(m_i - mu)^T = (1 / n) F^T diag(1 / n_i) F of the class sums F of the centred rows, so
//                 that Sb + Sw is the total covariance; A [P][R] the first P columns of V, transposed: A Sw A^T = I_P.
//   backend_project  (X - mu) A^T [n][P], length-normalised as backend_apply does it.
//   plda_score_diag  the two-covariance PLDA score in the basis V of gen_eig(Sb, Sw), where Sw = I and Sb = diag(psi):
//                 u_t = V^T (x_t - mu), G_j = V^T (E_j - c mu), h_cd = psi_d / (c psi_d + 1), s_cd = 1 + h_cd, s_0d = 1 + psi_d,
//                 m_jd = h_cd G_jd (= g_cd ebar_jd), Mt = m / s, q_j = sum_d m_jd Mt_jd, a_ct = sum_d u_td^2 / s_cd:
//                 score = -1/2 sum_d ln s_cd - 1/2 (a_ct - 2 (Mt U^T)[j][t] + q_j) + 1/2 sum_d ln s_0d + 1/2 a_0t.
//                 Two products (U, G), ONE cross product over all models whatever their class, one narrow product U.^2 [T][R] by
//                 [R][classes + 1], an assemble kernel; no factorisation.  The tables of h, 1 / s and the log sums are O(classes R)
//                 and made on the host, d = 0 .. R - 1 in order.
// The kernels here are elementwise; every product is the dense layer's GEMM (dense64.hpp), every centring, class sum, row dot product, row
// norm and block inverse plda.hip's (eig_dev.hpp).  No atomics; fixed orders; a score depends on its model's count and sum and on its
// segment only, so neither the batch nor the chunking under "plda_scratch_mib" shows, bit for bit.
#include "dense64.hpp"
#include "eig_dev.hpp"
#include "jfa.hpp"              // the option jfa_lds_rows, nothing else of JFA's

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace sr {

// M <- (M + M^T) / 2, a lane per element of the lower triangle.
__global__ __launch_bounds__(PLDA_WG)
void beig_symmetrise_kernel(double *__restrict__ M, int R) {
    const int e = blockIdx.x * PLDA_WG + threadIdx.x;
    if (e >= R * R) return;
    const int i = e / R, j = e % R;
    if (j > i) return;
    const double v = 0.5 * (M[e] + M[j * R + i]);
    M[e] = v;
    M[j * R + i] = v;
}

__global__ __launch_bounds__(PLDA_WG)
void beig_scale_rows_kernel(const double *__restrict__ F, const double *__restrict__ w, double *__restrict__ out, int64_t rows, int R) {
    const int64_t e = (int64_t)blockIdx.x * PLDA_WG + threadIdx.x;
    if (e < rows * R) out[e] = w[e / R] * F[e];
}

// m = h[cls[j]] .* G[j],  Mt = m .* inv_s[cls[j]]
__global__ __launch_bounds__(PLDA_WG)
void beig_models_kernel(const double *__restrict__ G, const int *__restrict__ cls, const double *__restrict__ h, const double *__restrict__ inv_s,
                        double *__restrict__ Mm, double *__restrict__ Mt, int64_t J, int R) {
    const int64_t e = (int64_t)blockIdx.x * PLDA_WG + threadIdx.x;
    if (e >= J * R) return;
    const int64_t t = (int64_t)cls[e / R] * R + e % R;
    const double m = h[t] * G[e];
    Mm[e] = m;
    Mt[e] = m * inv_s[t];
}

__global__ __launch_bounds__(PLDA_WG)
void beig_square_kernel(const double *__restrict__ U, double *__restrict__ out, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * PLDA_WG + threadIdx.x;
    if (e < n) out[e] = U[e] * U[e];
}

// out[j][t0 + c], j < J, c < cols, holds the cross term (row stride ld); a [cols][nc + 1], its last column a_0; q [J]; ld_c, ok [nc].
__global__ __launch_bounds__(PLDA_WG)
void beig_assemble_kernel(double *__restrict__ out, int64_t ld, int64_t t0, int64_t J, int64_t cols, const double *__restrict__ q,
                          const int *__restrict__ cls, const double *__restrict__ a, int nc, const double *__restrict__ ld_c, double ld_0,
                          const int *__restrict__ ok) {
    const int64_t e = (int64_t)blockIdx.x * PLDA_WG + threadIdx.x;
    if (e >= J * cols) return;
    const int64_t j = e / cols, c = e % cols;
    const int k = cls[j];
    double *p = out + j * ld + t0 + c;
    double v = 0.0;
    if (ok[k]) {
        const double quad = (a[c * (nc + 1) + k] - 2.0 * *p) + q[j];
        v = 0.5 * ((ld_0 - ld_c[k]) + (a[c * (nc + 1) + nc] - quad));
    }
    *p = v;
}

// ---- host ----

namespace {
struct BeigScratch {
    DevBuf<double> Sb, Sw, T1, M, Q, psi, V;                   // the generalised problem
    DevBuf<double> X, Xc, Xw, F, Fs, mu, coef, A, Y;           // LDA, the projection
    DevBuf<double> inv_n, inv_cnt;                             // LDA: the scalar 1 / n, the classes' 1 / n_i
    DevBuf<double> E, G, Mm, Mt, q, Z, U, a, h, inv_s, ld_c, out;      // the diagonalised scorer
    DevBuf<int64_t> order, start, midx;
    DevBuf<int> flags, cls, ok;
};
}  // namespace

static unsigned flat_blocks(int64_t n) { return (unsigned)((n + PLDA_WG - 1) / PLDA_WG); }

// The plan of plda.hip's block inverse for one R x R block.
static PldaPlan block_plan(int R) {
    PldaPlan pl;
    std::string why;
    const int64_t zero = 0;
    if (!plan_plda_train(1, R, &zero, 1, (int)jfa_lds_rows(), std::max(1, ctx().n_cu), pl, why)) fail("%s", why.c_str());
    return pl;
}

// Sb, Sw [R][R] on the device (Sw's lower triangle is read; both are overwritten) -> psi [R], V [R][R] on the device.
// -> 0, 1 (Sw did not factor: psi and V are exact zeros) or 2 (the sweep cap).  Synchronises.
static int gen_eig_device(hipStream_t st, BeigScratch &s, const PldaPlan &pl, int R, double *Sb, double *Sw, double *psi, double *V, int *sweeps) {
    const int64_t rr = (int64_t)R * R;
    std::vector<int> flags;
    std::vector<double> logdet;
    if (sweeps) *sweeps = 0;
    if (plda_invert_blocks(st, pl, Sw, 1, 1, flags, logdet)) {         // Sw <- L^-1, the upper triangle zeros
        SR_HIP(hipMemsetAsync(psi, 0, (size_t)R * 8, st));
        SR_HIP(hipMemsetAsync(V, 0, (size_t)rr * 8, st));
        sync_stream();
        return 1;
    }
    s.T1.ensure((size_t)rr), s.M.ensure((size_t)rr), s.Q.ensure((size_t)rr);
    dense_gemm(T_JFA_GEMM_C, st, Sw, R, 1, Sb, R, 1, s.T1.p, R, R, R, R, false, 0);              // L^-1 Sb
    dense_gemm(T_JFA_GEMM_C, st, s.T1.p, R, 1, Sw, 1, R, s.M.p, R, R, R, R, false, 0);           // (L^-1 Sb) L^-T
    {
        ScopedKernelTimer tm(T_JFA_UPDATE);
        hipLaunchKernelGGL(beig_symmetrise_kernel, dim3(flat_blocks(rr)), dim3(PLDA_WG), 0, st, s.M.p, R);
        SR_HIP(hipGetLastError());
    }
    EigPlan ep;
    std::string why;
    if (!plan_eig(R, std::max(1, ctx().n_cu), ep, why)) fail("%s", why.c_str());
    int converged = 0;
    sym_eig_device(st, ep, s.M.p, psi, s.Q.p, sweeps, &converged);
    dense_gemm(T_JFA_GEMM_C, st, Sw, 1, R, s.Q.p, R, 1, V, R, R, R, R, false, 0);                // V = L^-T Q
    sync_stream();
    return converged ? 0 : 2;
}

void gen_eig(int R, const double *Sb, const double *Sw, double *psi, double *V, int *sweeps, int *status) {
    std::string why;
    if (!eig_check_matrix(Sb, R, "Sb", why) || !eig_check_matrix(Sw, R, "Sw", why)) fail("%s", why.c_str());
    if (!psi || !V) fail("generalised eigen-problem: null argument (psi [R] and V [R][R], the results)");
    plda_check_device("sr_gen_eig");
    hipStream_t st = ctx().stream;
    auto &s = per_device<BeigScratch>();
    const int64_t rr = (int64_t)R * R;
    const std::vector<double> sb = plda_mirrored(Sb, R), sw = plda_mirrored(Sw, R);
    s.Sb.upload(sb.data(), (size_t)rr), s.Sw.upload(sw.data(), (size_t)rr);
    s.psi.ensure((size_t)R), s.V.ensure((size_t)rr);
    const int code = gen_eig_device(st, s, block_plan(R), R, s.Sb.p, s.Sw.p, s.psi.p, s.V.p, sweeps);
    s.psi.download(psi, (size_t)R);
    s.V.download(V, (size_t)rr);
    sync_stream();
    if (status) *status = code;
}

void lda_fit(int64_t n, int R, const double *X, const int64_t *ids, int64_t S, int P, double *mu_out, double *A, double *psi_out) {
    std::string why;
    plda_check_matrix(X, n, R, "X, the training vectors [n][R]", "n, the number of training vectors");
    if (!mu_out || !A || !psi_out) fail("LDA: null argument (mu [R], A [P][R] and psi [P], the results)");
    PldaPlan pl;
    if (!plan_plda_train(n, R, ids, S, (int)jfa_lds_rows(), 1, pl, why)) fail("%s", why.c_str());
    if (!lda_check_dims(P, R, S, why)) fail("%s", why.c_str());
    plda_check_device("sr_lda_fit");
    if (!plan_plda_train(n, R, ids, S, (int)jfa_lds_rows(), std::max(1, ctx().n_cu), pl, why)) fail("%s", why.c_str());
    hipStream_t st = ctx().stream;
    auto &s = per_device<BeigScratch>();
    const int64_t rr = (int64_t)R * R;
    const std::vector<double> mu = plda_row_mean(X, n, R);
    // the rows centred in the plan's sorted order, the class sums, the rows about their class means
    std::vector<int64_t> midx((size_t)n);
    std::vector<double> coef((size_t)n), inv_cnt((size_t)S);
    const std::vector<double> inv_n(1, 1.0 / (double)n);
    for (int64_t g = 0; g < S; g++) {
        const int64_t cnt = pl.row_start[(size_t)g + 1] - pl.row_start[(size_t)g];
        inv_cnt[(size_t)g] = 1.0 / (double)cnt;
        for (int64_t r = pl.row_start[(size_t)g]; r < pl.row_start[(size_t)g + 1]; r++) midx[(size_t)r] = g, coef[(size_t)r] = inv_cnt[(size_t)g];
    }
    s.X.upload(X, (size_t)(n * R));
    s.mu.upload(mu.data(), (size_t)R);
    s.order.upload(pl.row_order.data(), (size_t)n);
    s.start.upload(pl.row_start.data(), (size_t)S + 1);
    s.midx.upload(midx.data(), (size_t)n);
    s.coef.upload(coef.data(), (size_t)n);
    s.Xc.ensure((size_t)(n * R)), s.Xw.ensure((size_t)(n * R)), s.F.ensure((size_t)(S * R)), s.Fs.ensure((size_t)(S * R));
    s.Sb.ensure((size_t)rr), s.Sw.ensure((size_t)rr), s.T1.ensure((size_t)rr), s.psi.ensure((size_t)R), s.V.ensure((size_t)rr);
    plda_launch_centre(st, s.X.p, s.order.p, s.mu.p, nullptr, nullptr, s.Xc.p, n, R);
    plda_launch_class_sums(st, s.Xc.p, s.start.p, s.F.p, S, R);
    plda_launch_centre(st, s.Xc.p, nullptr, s.F.p, s.midx.p, s.coef.p, s.Xw.p, n, R);
    plda_accumulate_gram(st, s.Xw.p, s.Xw.p, s.T1.p, n, pl.sum_chunk, R);
    s.inv_n.upload(inv_n.data(), 1);
    s.inv_cnt.upload(inv_cnt.data(), (size_t)S);
    plda_launch_combine(st, nullptr, 0, s.T1.p, s.inv_n.p, s.Sw.p, 1, R);                         // Sw = Xw^T Xw / n
    {
        ScopedKernelTimer tm(T_JFA_UPDATE);
        hipLaunchKernelGGL(beig_scale_rows_kernel, dim3(flat_blocks(S * R)), dim3(PLDA_WG), 0, st, s.F.p, s.inv_cnt.p, s.Fs.p, S, R);
        SR_HIP(hipGetLastError());
    }
    plda_accumulate_gram(st, s.F.p, s.Fs.p, s.T1.p, S, pl.grp_chunk, R);
    plda_launch_combine(st, nullptr, 0, s.T1.p, s.inv_n.p, s.Sb.p, 1, R);                             // Sb = F^T diag(1 / n_i) F / n
    sync_stream();                             // (the tables above are host memory of this frame)
    int sweeps = 0;
    const int code = gen_eig_device(st, s, pl, R, s.Sb.p, s.Sw.p, s.psi.p, s.V.p, &sweeps);
    if (code == 1)
        fail("LDA: the within-class covariance of these %lld vectors of %d dimensions does not factor (dependent columns, or too few vectors); "
             "pass more vectors or reduce the dimension", (long long)n, R);
    if (code == 2) fail("LDA: the eigen-solver reached its cap of %d sweeps without converging; check the vectors' scale", sweeps);
    std::vector<double> V((size_t)rr), psi((size_t)R);
    s.V.download(V.data(), (size_t)rr);
    s.psi.download(psi.data(), (size_t)R);
    sync_stream();
    for (int p = 0; p < P; p++) {
        psi_out[p] = psi[(size_t)p];
        for (int k = 0; k < R; k++) A[(int64_t)p * R + k] = V[(size_t)k * R + p];
    }
    std::memcpy(mu_out, mu.data(), (size_t)R * 8);
}

void backend_project(int64_t n, int R, int P, const double *X, const double *mu, const double *A, int length_norm, double *Y, int64_t *zero_rows) {
    std::string why;
    plda_check_matrix(X, n, R, "X, the vectors [n][R]", "n, the number of vectors");
    if (P < 1 || P > R) fail("projection: P, the rows of A, is %d; a projection of vectors of %d dimensions keeps 1 <= P <= R", P, R);
    if (!mu || !A || !Y) fail("projection: null argument (mu [R], A [P][R] and Y [n][P] are all required)");
    if (!plda_check_finite(mu, R, "mu", why) || !plda_check_finite(A, (int64_t)P * R, "A", why)) fail("%s", why.c_str());
    plda_check_device("sr_backend_project");
    hipStream_t st = ctx().stream;
    auto &s = per_device<BeigScratch>();
    s.X.upload(X, (size_t)(n * R));
    s.mu.upload(mu, (size_t)R);
    s.A.upload(A, (size_t)P * R);
    s.Xc.ensure((size_t)(n * R)), s.Y.ensure((size_t)(n * P));
    plda_launch_centre(st, s.X.p, nullptr, s.mu.p, nullptr, nullptr, s.Xc.p, n, R);
    dense_gemm(T_JFA_GEMM_C, st, s.Xc.p, R, 1, s.A.p, 1, R, s.Y.p, P, n, P, R, false, 0);        // (X - mu) A^T
    int64_t zeros = 0;
    if (length_norm) {
        s.flags.ensure((size_t)n);
        plda_launch_rownorm(st, s.Y.p, n, P, s.flags.p);
        std::vector<int> flags((size_t)n);
        s.flags.download(flags.data(), (size_t)n);
        sync_stream();
        for (int f : flags) zeros += f != 0;
    }
    s.Y.download(Y, (size_t)(n * P));
    sync_stream();
    if (zero_rows) *zero_rows = zeros;
}

void plda_score_diag(int64_t J, int64_t T, int R, const double *mu, const double *V, const double *psi, const double *E, const int64_t *enrol_n,
                     const double *X, double *out, int64_t *bad_classes) {
    std::string why;
    plda_check_matrix(E, J, R, "E, the models' enrolment sums [J][R]", "J, the number of models");
    plda_check_matrix(X, T, R, "X, the test vectors [T][R]", "T, the number of test segments");
    if (!mu || !V || !psi || !out) fail("diagonalised PLDA scoring: null argument (mu [R], V [R][R], psi [R] and out [J][T] are all required)");
    if (!plda_check_finite(mu, R, "mu", why) || !plda_check_finite(V, (int64_t)R * R, "V", why)) fail("%s", why.c_str());
    PldaPlan pl;
    if (!plan_plda_score(J, T, R, enrol_n, (int64_t)1 << 40, (int)jfa_lds_rows(), 1, pl, why)) fail("%s", why.c_str());
    const int nc = (int)pl.classes.size();
    DiagChunks ch;
    if (!plan_diag_chunks(T, R, nc, (int64_t)plda_scratch_mib() << 20, ch, why)) fail("%s", why.c_str());
    plda_check_device("sr_plda_score_diag");
    hipStream_t st = ctx().stream;
    auto &s = per_device<BeigScratch>();
    // the tables, on the host: h_cd = psi_d / (c psi_d + 1), 1 / s_cd, the log sums; the last row of inv_s is 1 / s_0d
    const bool usable = diag_psi_usable(psi, R);
    std::vector<double> h((size_t)nc * R, 0.0), inv_s((size_t)(nc + 1) * R, 1.0), ld_c((size_t)nc, 0.0), cnt((size_t)J);
    std::vector<int> ok((size_t)nc, usable ? 1 : 0), cls((size_t)J);
    double ld_0 = 0.0;
    int64_t bad = 0;
    for (int k = 0; k < nc; k++) {
        const double c = (double)pl.classes[(size_t)k].count;
        // s_cd = ((c + 1) psi_d + 1) / (c psi_d + 1) must be positive: with (c + 1) psi_d + 1 > 0 so are c psi_d + 1 and s_0d.  A backstop:
        // a usable psi_d is above -1e-9 max|psi|, so this is only met where max|psi| > 1e9 / (c + 1) -- and there 1 / s_cd is no number to score with.
        for (int d = 0; d < R && ok[(size_t)k]; d++)
            if (!((c + 1.0) * psi[d] + 1.0 > 0.0)) ok[(size_t)k] = 0;
        if (ok[(size_t)k])
            for (int d = 0; d < R; d++) {
                const double hd = psi[d] / (c * psi[d] + 1.0), sd = 1.0 + hd;
                h[(size_t)k * R + d] = hd;
                inv_s[(size_t)k * R + d] = 1.0 / sd;
                ld_c[(size_t)k] += std::log(sd);
            }
        bad += ok[(size_t)k] ? 0 : 1;
        for (int64_t p = 0; p < pl.classes[(size_t)k].size; p++) cls[(size_t)pl.perm[(size_t)(pl.classes[(size_t)k].start + p)]] = k;
    }
    if (bad_classes) *bad_classes = bad;
    if (bad == nc) {                           // nothing to compute: exact zeros
        std::memset(out, 0, (size_t)(J * T) * 8);
        return;
    }
    for (int d = 0; d < R; d++) {
        inv_s[(size_t)nc * R + d] = 1.0 / (1.0 + psi[d]);
        ld_0 += std::log(1.0 + psi[d]);
    }
    for (int64_t j = 0; j < J; j++) cnt[(size_t)j] = (double)enrol_n[j];
    const int64_t chunk = ch.chunk;
    s.E.upload(E, (size_t)(J * R));
    s.mu.upload(mu, (size_t)R);
    s.V.upload(V, (size_t)R * R);
    s.coef.upload(cnt.data(), (size_t)J);
    s.h.upload(h.data(), h.size()), s.inv_s.upload(inv_s.data(), inv_s.size()), s.ld_c.upload(ld_c.data(), (size_t)nc);
    s.cls.upload(cls.data(), (size_t)J), s.ok.upload(ok.data(), (size_t)nc);
    s.F.ensure((size_t)(J * R)), s.G.ensure((size_t)(J * R)), s.Mm.ensure((size_t)(J * R)), s.Mt.ensure((size_t)(J * R)), s.q.ensure((size_t)J);
    s.Z.ensure((size_t)(chunk * R)), s.U.ensure((size_t)(chunk * R)), s.a.ensure((size_t)(chunk * (nc + 1)));
    s.out.ensure((size_t)(J * T));
    plda_launch_centre(st, s.E.p, nullptr, s.mu.p, nullptr, s.coef.p, s.F.p, J, R);               // f_j = e_j - n_j mu
    dense_gemm(T_JFA_GEMM_C, st, s.F.p, R, 1, s.V.p, R, 1, s.G.p, R, J, R, R, false, 0);         // G = F V
    {
        ScopedKernelTimer tm(T_JFA_UPDATE);
        hipLaunchKernelGGL(beig_models_kernel, dim3(flat_blocks(J * R)), dim3(PLDA_WG), 0, st, s.G.p, s.cls.p, s.h.p, s.inv_s.p, s.Mm.p, s.Mt.p, J, R);
        SR_HIP(hipGetLastError());
    }
    plda_launch_rowdot(st, s.Mm.p, s.Mt.p, s.q.p, J, R);
    for (int64_t ci = 0; ci < ch.n_chunks; ci++) {
        const int64_t t0 = ci * chunk, nt = std::min(chunk, T - t0);
        s.Z.upload(X + t0 * R, (size_t)(nt * R));
        plda_launch_centre(st, s.Z.p, nullptr, s.mu.p, nullptr, nullptr, s.U.p, nt, R);
        dense_gemm(T_JFA_GEMM_C, st, s.U.p, R, 1, s.V.p, R, 1, s.Z.p, R, nt, R, R, false, 0);    // U = (X - mu) V, in Z
        dense_gemm(T_JFA_GEMM_C, st, s.Mt.p, R, 1, s.Z.p, 1, R, s.out.p + t0, T, J, nt, R, false, 0);         // Mt U^T: every model at once
        {
            ScopedKernelTimer tm(T_JFA_UPDATE);
            hipLaunchKernelGGL(beig_square_kernel, dim3(flat_blocks(nt * R)), dim3(PLDA_WG), 0, st, s.Z.p, s.U.p, nt * R);
            SR_HIP(hipGetLastError());
        }
        dense_gemm(T_JFA_GEMM_C, st, s.U.p, R, 1, s.inv_s.p, 1, R, s.a.p, nc + 1, nt, nc + 1, R, false, 0);   // a = U.^2 [nt][R] by [R][nc + 1]
        {
            ScopedKernelTimer tm(T_JFA_UPDATE);
            hipLaunchKernelGGL(beig_assemble_kernel, dim3(flat_blocks(J * nt)), dim3(PLDA_WG), 0, st, s.out.p, T, t0, J, nt, s.q.p, s.cls.p, s.a.p, nc,
                               s.ld_c.p, ld_0, s.ok.p);
            SR_HIP(hipGetLastError());
        }
        sync_stream();                         // (the next chunk's upload reuses Z)
    }
    s.out.download(out, (size_t)(J * T));
    sync_stream();
}

}  // namespace sr
