// plda.hpp -- the i-vector back end on the device, host memory in and out: whitening / WCCN, cosine scoring and the two-covariance
// PLDA (plda.hip), the symmetric eigen-solver (eig.hip) and what the back end builds on it (backend_eig.hip).
#pragma once

#include <cstdint>

namespace sr {

// plda.hip
void plda_train(int64_t n, int R, const double *X, const int64_t *ids, int64_t S, int n_iter, int default_start, double *mu_out, double *Sb,
                double *Sw, int *iterations, int *n_classes, int *stop);
void plda_score(int64_t J, int64_t T, int R, const double *mu, const double *Sb, const double *Sw, const double *E, const int64_t *enrol_n,
                const double *X, double *out, int64_t *bad_classes);
void backend_fit(int kind, int64_t n, int R, const double *X, const int64_t *ids, int64_t S, double *mu_out, double *A);
void backend_apply(int64_t n, int R, const double *X, const double *mu, const double *A, int length_norm, double *Y, int64_t *zero_rows);
void cosine_score(int64_t J, int64_t T, int R, const double *E, const double *X, double *out);
void set_plda_scratch_mib(long v);
long plda_scratch_mib();
// eig.hip, the host entry behind sr_sym_eig (A, w, V host memory).
void sym_eig(int R, const double *A, double *w, double *V, int *sweeps, int *converged);
// backend_eig.hip
void gen_eig(int R, const double *Sb, const double *Sw, double *psi, double *V, int *sweeps, int *status);
void lda_fit(int64_t n, int R, const double *X, const int64_t *ids, int64_t S, int P, double *mu_out, double *A, double *psi_out);
void backend_project(int64_t n, int R, int P, const double *X, const double *mu, const double *A, int length_norm, double *Y, int64_t *zero_rows);
void plda_score_diag(int64_t J, int64_t T, int R, const double *mu, const double *V, const double *psi, const double *E, const int64_t *enrol_n,
                     const double *X, double *out, int64_t *bad_classes);

}  // namespace sr
