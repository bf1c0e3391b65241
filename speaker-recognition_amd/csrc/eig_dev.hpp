// eig_dev.hpp -- what eig.hip (the symmetric eigen-solver), backend_eig.hip (the generalised problem, LDA, the diagonalised PLDA
// scorer) and plda.hip (whose launchers the second reuses) hand each other.  Everything here runs on the calling thread's device
// and stream; the pointers are device memory unless a comment says host.  Nothing of JFA's and nothing of the dense layer's: a file
// that forms a product includes dense64.hpp itself.
#pragma once

#include "common.hpp"
#include "eig_plan.hpp"
#include "plda.hpp"

#include <vector>

namespace sr {

// eig.hip: w [R] descending and V [R][R] (column k the unit eigenvector of w[k], its component of largest magnitude positive, the
// lowest index winning a tie) of the symmetric A [R][R], whose lower triangle is read and which is overwritten.  Synchronises.
void sym_eig_device(hipStream_t st, const EigPlan &pl, double *A, double *w, double *V, int *sweeps, int *converged);

// plda.hip's launchers and host helpers, defined there under these names and used by backend_eig.hip as well (the kernels stay
// where they are).
void plda_launch_centre(hipStream_t st, const double *X, const int64_t *src, const double *M, const int64_t *midx, const double *coef, double *out,
                        int64_t rows, int R);
void plda_launch_class_sums(hipStream_t st, const double *Xs, const int64_t *row_start, double *F, int64_t S, int R);
void plda_launch_combine(hipStream_t st, const double *A, int64_t stride_a, const double *B, const double *coef, double *out, int64_t nb, int R);
void plda_launch_rowdot(hipStream_t st, const double *A, const double *B, double *out, int64_t rows, int R);
void plda_launch_rownorm(hipStream_t st, double *Y, int64_t rows, int R, int *flags);
void plda_accumulate_gram(hipStream_t st, const double *A, const double *B, double *C, int64_t rows, int64_t chunk, int R);
// Inverts n blocks in place (mode 0 the inverse, 1 the inverse of the Cholesky factor, 2 the factor); -> the blocks that failed.  Synchronises.
int64_t plda_invert_blocks(hipStream_t st, const PldaPlan &pl, double *blocks, int64_t n, int mode, std::vector<int> &flags, std::vector<double> &logdet);
std::vector<double> plda_row_mean(const double *X /*host*/, int64_t n, int R);
std::vector<double> plda_mirrored(const double *M /*host*/, int R);
void plda_check_device(const char *what);
void plda_check_matrix(const double *X /*host*/, int64_t n, int R, const char *name, const char *rows_name);

}  // namespace sr
