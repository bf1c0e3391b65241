// dense64.hpp -- the float64 dense layer's one host entry: the strided GEMM of dense64.hip on v_mfma_f64_16x16x4_f64.  What JFA
// estimation, scoring and centring (jfa.hip, jfa_score.hip, jfa_stats.hip), the i-vector back end (plda.hip, backend_eig.hip) and
// score normalisation (score_norm.hip) form every product with.  The geometry is dense64_plan.hpp's; the factorisation of one block
// inside a consumer's own kernel is dense64_dev.hpp's.
#pragma once

#include "common.hpp"
#include "dense64_plan.hpp"

namespace sr {

// C [M][N] (row stride ldc) (+)= A [M][Kred] B [Kred][N] on the stream, booked to `kind`.  A[m][k] is at A + m sam + k sak and
// B[k][n] at B + k sbk + n sbn: a transposed operand is a pair of strides, never a copy.  accumulate: the launch starts from what C
// holds, so a sum cut into launches of whole reduction tiles (multiples of DENSE_KSTEP) is the same sequence of matrix instructions
// as the uncut one.  diag_step > 0: 1 is added to every column that is a multiple of it (I + ... over rows of flattened blocks).
// M <= 65535 x DENSE_TILE (the row tiles are the grid's y).
void dense_gemm(TimerKind kind, hipStream_t st, const double *A, int64_t sam, int64_t sak, const double *B, int64_t sbk, int64_t sbn, double *C,
                int64_t ldc, int64_t M, int64_t N, int64_t Kred, bool accumulate, int diag_step);

}  // namespace sr
