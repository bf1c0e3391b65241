// abi_backend.cpp -- what works on scores and i-vectors: score normalisation, calibration, the PLDA back end, the eigen-solver.
#include "abi_internal.hpp"

#include "calib.hpp"
#include "calib_plan.hpp"
#include "eig_plan.hpp"
#include "norm_plan.hpp"
#include "plda.hpp"
#include "plda_plan.hpp"
#include "score_norm.hpp"

#include <cstring>
#include <string>

using namespace sr;

extern "C" {

// ---- score normalisation (score_norm.hip).  Every refusal comes before the device is touched. ----

int sr_score_norm(int mode, int64_t J, int64_t T, int64_t Cz, int64_t Ct, int top_n, const double *S, const double *Ez, const double *Tt,
                  const double *Zt, double *out, int64_t *degenerate) {
    SR_TRY
    score_norm(mode, J, T, Cz, Ct, top_n, S, Ez, Tt, Zt, out, degenerate);
    return 0;
    SR_CATCH(-1)
}

int sr_score_norm_select(int64_t rows, int64_t C, int top_n, const double *X, int64_t *idx, double *mu, double *sigma) {
    SR_TRY
    score_norm_select(rows, C, top_n, X, idx, mu, sigma);
    return 0;
    SR_CATCH(-1)
}

int sr_score_norm_plan(int mode, int64_t J, int64_t T, int64_t Cz, int64_t Ct, int top_n, int64_t scratch_bytes, int n_cu, int64_t *out,
                       int n_out) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 40) fail("sr_score_norm_plan writes 40 fields");
    std::string why;
    NormPlan p;
    if (n_cu > 0) {
        if (!plan_score_norm(mode, J, T, Cz, Ct, top_n, scratch_bytes, n_cu, p, why)) fail("%s", why.c_str());
    } else {
        if (!plan_score_norm(mode, J, T, Cz, Ct, top_n, scratch_bytes, 1, p, why)) fail("%s", why.c_str());      // the refusals first
        ensure_device();
        if (!plan_score_norm(mode, J, T, Cz, Ct, top_n, scratch_bytes, ctx().n_cu, p, why)) fail("%s", why.c_str());
    }
    const int64_t v[40] = {p.mode, p.n_sel, p.n_sel_test, p.chunk, p.n_chunks, p.fixed_bytes, p.seg_bytes, p.bytes_scratch, p.bytes_S, p.bytes_Ez,
                           p.bytes_Tt, p.bytes_Zt, p.bytes_out, p.bytes_moments, p.bytes_tnorm, p.bytes_counts, p.select_enrol.x, p.select_test.x,
                           p.select_zt.x, p.select_lds_enrol, p.select_lds_test, p.shift_enrol.x, p.shift_test.x, p.gemm_enrol.x, p.gemm_enrol.y,
                           p.gemm_test.x, p.gemm_test.y, p.gemm_lds, p.apply.x, p.apply.y, p.select_rounds, NORM_MAX_C, NORM_MAX_ROWS, NORM_WG,
                           0, 0, 0, 0, 0, 0};
    std::memcpy(out, v, sizeof v);
    return 40;
    SR_CATCH(-1)
}

// ---- score calibration and fusion (calib.hip).  Every refusal comes before the device is touched. ----

int sr_calib_train(int S, int64_t n, const double *X, const int8_t *lab, double prior, double ridge, double tol, int max_pass, const double *theta0,
                   int resume, double *state, int64_t *counts) {
    SR_TRY
    calib_train(S, n, X, lab, prior, ridge, tol, max_pass, theta0, resume, state, counts);
    return 0;
    SR_CATCH(-1)
}

int sr_calib_eval(int S, int64_t n, const double *X, const int8_t *lab, double prior, double ridge, const double *theta, double *f, double *g,
                  double *H, int64_t *counts) {
    SR_TRY
    calib_eval(S, n, X, lab, prior, ridge, theta, f, g, H, counts);
    return 0;
    SR_CATCH(-1)
}

int sr_calib_apply(int S, int64_t n, const double *X, const double *theta, double *out) {
    SR_TRY
    calib_apply(S, n, X, theta, out);
    return 0;
    SR_CATCH(-1)
}

int sr_calib_counts(int64_t n, const double *llr, const int8_t *lab, int m, const double *thr, int64_t *miss, int64_t *fa, int64_t *counts) {
    SR_TRY
    calib_counts(n, llr, lab, m, thr, miss, fa, counts);
    return 0;
    SR_CATCH(-1)
}

int sr_calib_plan(int S, int64_t n, int n_thr, int call, int64_t scratch_bytes, int n_cu, int64_t *out, int n_out) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 28) fail("sr_calib_plan writes 28 fields");
    if (call < 0 || call > 2) fail("sr_calib_plan: call is 0 (train / eval), 1 (apply) or 2 (counts)");
    std::string why;
    CalibPlan p;
    if (!plan_calib(S, n, n_thr, scratch_bytes, n_cu > 0 ? n_cu : 1, p, why)) fail("%s", why.c_str());          // the refusals first
    if (scratch_bytes > 0 && !calib_check_bound(p, call == 1 ? "apply" : call == 2 ? "counts" : "train", scratch_bytes, why)) fail("%s", why.c_str());
    if (n_cu <= 0) {
        ensure_device();
        if (!plan_calib(S, n, n_thr, scratch_bytes, ctx().n_cu, p, why)) fail("%s", why.c_str());
    }
    const int64_t v[28] = {p.S, p.n, p.n_blocks, p.acc, p.state_len, p.bytes_X, p.bytes_lab, p.bytes_partial, p.bytes_state, p.bytes_out,
                           p.bytes_thr, p.bytes_counts, p.resident_train, p.resident_apply, p.resident_counts, p.pass_grid, p.step_grid,
                           p.apply_grid, p.counts_grid, p.pass_rounds, CALIB_MAX_S, CALIB_MAX_THR, CALIB_BLOCK, CALIB_WG,
                           CALIB_CADENCE, CALIB_MAX_PASS, CALIB_MAX_N, 0};
    std::memcpy(out, v, sizeof v);
    return 28;
    SR_CATCH(-1)
}

// ---- the i-vector back end (plda.hip).  Every refusal comes before the device is touched. ----

int sr_backend_fit(int kind, int64_t n, int R, const double *X, const int64_t *ids, int64_t n_labels, double *mu, double *A) {
    SR_TRY
    backend_fit(kind, n, R, X, ids, n_labels, mu, A);
    return 0;
    SR_CATCH(-1)
}

int sr_backend_apply(int64_t n, int R, const double *X, const double *mu, const double *A, int length_norm, double *Y, int64_t *zero_rows) {
    SR_TRY
    backend_apply(n, R, X, mu, A, length_norm, Y, zero_rows);
    return 0;
    SR_CATCH(-1)
}

int sr_cosine_score(int64_t J, int64_t T, int R, const double *E, const double *X, double *out) {
    SR_TRY
    cosine_score(J, T, R, E, X, out);
    return 0;
    SR_CATCH(-1)
}

int sr_plda_train(int64_t n, int R, const double *X, const int64_t *ids, int64_t n_labels, int n_iter, int default_start, double *mu, double *Sb,
                  double *Sw, int *iterations, int *n_classes, int *stop) {
    SR_TRY
    plda_train(n, R, X, ids, n_labels, n_iter, default_start, mu, Sb, Sw, iterations, n_classes, stop);
    return 0;
    SR_CATCH(-1)
}

int sr_plda_score(int64_t J, int64_t T, int R, const double *mu, const double *Sb, const double *Sw, const double *E, const int64_t *enrol_n,
                  const double *X, double *out, int64_t *bad_classes) {
    SR_TRY
    plda_score(J, T, R, mu, Sb, Sw, E, enrol_n, X, out, bad_classes);
    return 0;
    SR_CATCH(-1)
}

int sr_plda_plan(int kind, int R, int64_t rows, int64_t groups, int64_t T, const int64_t *counts, int64_t scratch_bytes, int lds_rows, int n_cu,
                 int64_t *out, int n_out, int64_t *perm, int64_t *classes) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 36) fail("sr_plda_plan writes 36 fields");
    if (kind != PLDA_TRAIN && kind != PLDA_SCORE) fail("sr_plda_plan: the kind is 0 (training) or 1 (scoring)");
    std::string why;
    PldaPlan p;
    auto plan = [&](int cu) {
        const bool ok = kind == PLDA_TRAIN ? plan_plda_train(rows, R, counts, groups, lds_rows, cu, p, why)
                                           : plan_plda_score(rows, T, R, counts, scratch_bytes, lds_rows, cu, p, why);
        if (!ok) fail("%s", why.c_str());
    };
    if (n_cu > 0) {
        plan(n_cu);
    } else {
        plan(1);                               // the refusals first
        ensure_device();
        plan(ctx().n_cu);
    }
    const int64_t v[36] = {p.kind, p.R, p.rows, p.groups, p.T, (int64_t)p.classes.size(), p.sum_chunk, p.sum_chunks, p.grp_chunk, p.grp_chunks,
                           p.chunk, p.n_chunks, p.seg_bytes, p.bytes_scratch, p.bytes_blocks, p.bytes_rows, p.path, p.lds_rows, p.factor_lds,
                           p.gemm_lds, p.centre.x, p.class_sums.x, p.class_sums.y, p.invert.x, p.gemm_rows.x, p.gemm_rows.y, p.gemm_acc.x,
                           p.gemm_acc.y, p.rowdot.x, p.gemm_cross.x, p.gemm_cross.y, p.assemble.x, p.invert_rounds,
                           PLDA_MAX_R, PLDA_MAX_ROWS, p.tri.y};
    std::memcpy(out, v, sizeof v);
    if (perm) std::memcpy(perm, p.perm.data(), p.perm.size() * sizeof(int64_t));
    if (classes)
        for (size_t c = 0; c < p.classes.size(); c++)
            classes[3 * c] = p.classes[c].count, classes[3 * c + 1] = p.classes[c].start, classes[3 * c + 2] = p.classes[c].size;
    return 36;
    SR_CATCH(-1)
}

// ---- the symmetric eigen-solver and what the back end builds on it (eig.hip, backend_eig.hip).  Every refusal comes first. ----

int sr_sym_eig(int R, const double *A, double *w, double *V, int *sweeps, int *converged) {
    SR_TRY
    sym_eig(R, A, w, V, sweeps, converged);
    return 0;
    SR_CATCH(-1)
}

int sr_gen_eig(int R, const double *Sb, const double *Sw, double *psi, double *V, int *sweeps, int *status) {
    SR_TRY
    gen_eig(R, Sb, Sw, psi, V, sweeps, status);
    return 0;
    SR_CATCH(-1)
}

int sr_lda_fit(int64_t n, int R, const double *X, const int64_t *ids, int64_t n_labels, int P, double *mu, double *A, double *psi) {
    SR_TRY
    lda_fit(n, R, X, ids, n_labels, P, mu, A, psi);
    return 0;
    SR_CATCH(-1)
}

int sr_backend_project(int64_t n, int R, int P, const double *X, const double *mu, const double *A, int length_norm, double *Y, int64_t *zero_rows) {
    SR_TRY
    backend_project(n, R, P, X, mu, A, length_norm, Y, zero_rows);
    return 0;
    SR_CATCH(-1)
}

int sr_plda_score_diag(int64_t J, int64_t T, int R, const double *mu, const double *V, const double *psi, const double *E, const int64_t *enrol_n,
                       const double *X, double *out, int64_t *bad_classes) {
    SR_TRY
    plda_score_diag(J, T, R, mu, V, psi, E, enrol_n, X, out, bad_classes);
    return 0;
    SR_CATCH(-1)
}

int sr_eig_plan(int R, int n_cu, int64_t *out, int n_out, int *schedule) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 24) fail("sr_eig_plan writes 24 fields");
    std::string why;
    EigPlan p;
    if (n_cu > 0) {
        if (!plan_eig(R, n_cu, p, why)) fail("%s", why.c_str());
    } else {
        if (!plan_eig(R, 1, p, why)) fail("%s", why.c_str());      // the refusals first
        ensure_device();
        if (!plan_eig(R, ctx().n_cu, p, why)) fail("%s", why.c_str());
    }
    const int64_t v[24] = {p.R, p.b, p.blocks, p.phantom, p.rounds, p.pairs, p.single, p.max_sweeps, p.inner_sweeps, p.solve_lds, p.update_lds,
                           p.solve_grid, p.cols_x, p.cols_y, p.cols_z, p.rows_x, p.rows_y, p.launches_per_sweep, p.bytes_work, p.pair_rounds,
                           PLDA_MAX_R, EIG_TILE_ROWS, EIG_N, EIG_WG};
    std::memcpy(out, v, sizeof v);
    if (schedule)
        for (size_t i = 0; i < p.schedule.size(); i++) schedule[2 * i] = p.schedule[i].p, schedule[2 * i + 1] = p.schedule[i].q;
    return 24;
    SR_CATCH(-1)
}

}  // extern "C"
