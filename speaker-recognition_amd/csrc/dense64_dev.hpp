// dense64_dev.hpp -- the float64 dense layer's device routines: the panel Cholesky of one R x R block by one workgroup of DENSE_WG
// lanes and the two routines that turn its factor into the inverse.  Header-only: device code is not linked across files in this
// build, so each consumer's own kernel inlines them -- jfa_factor_kernel (jfa.hip), jfa_kscore_kernel (jfa_score.hip),
// plda_invert_kernel (plda.hip).  The block M has row stride R and is worked on where it lies: in LDS (path 0 of the plans: the
// kernel copied it there) or in place in global memory (path 1), the same code on another pointer; the panel is in LDS on both.
// A kernel sizes its dynamic LDS with dense_factor_lds_bytes (dense64_plan.hpp).  For .hip files only.
#pragma once

#include "dense64_plan.hpp"

#include <hip/hip_runtime.h>

namespace sr {

// Lower Cholesky factor over the lower triangle of M (the upper triangle is not read).  false: a pivot <= 0 or not finite (every
// lane returns the same: the pivot is read from LDS behind a barrier).
[[maybe_unused]] static __device__ bool dense_cholesky(double *M, int R, double *pan /* [R][DENSE_PS] */) {
    const int tid = threadIdx.x;
    for (int j0 = 0; j0 < R; j0 += DENSE_NB) {
        const int nb = min(DENSE_NB, R - j0), rows = R - j0;
        for (int e = tid; e < rows * nb; e += DENSE_WG) {
            const int r = e / nb, c = e % nb;
            pan[r * DENSE_PS + c] = M[(int64_t)(j0 + r) * R + j0 + c];
        }
        __syncthreads();
        for (int c = 0; c < nb; c++) {
            const double p = pan[c * DENSE_PS + c];
            if (!(p > 0.0) || !__builtin_isfinite(p)) return false;
            const double d = sqrt(p);
            __syncthreads();                   // every lane has read the pivot
            for (int r = c + tid; r < rows; r += DENSE_WG) pan[r * DENSE_PS + c] = r == c ? d : pan[r * DENSE_PS + c] / d;
            __syncthreads();
            const int w = nb - c - 1;
            for (int e = tid; e < (rows - c - 1) * w; e += DENSE_WG) {
                const int r = c + 1 + e / w, c2 = c + 1 + e % w;
                if (r >= c2) pan[r * DENSE_PS + c2] = __builtin_fma(-pan[r * DENSE_PS + c], pan[c2 * DENSE_PS + c], pan[r * DENSE_PS + c2]);
            }
            __syncthreads();
        }
        for (int e = tid; e < rows * nb; e += DENSE_WG) {
            const int r = e / nb, c = e % nb;
            if (r >= c) M[(int64_t)(j0 + r) * R + j0 + c] = pan[r * DENSE_PS + c];
        }
        const int t = rows - nb;               // the trailing block, lower triangle: M[i][k] -= sum_c pan[i][c] pan[k][c]
        for (int e = tid; e < t * t; e += DENSE_WG) {
            const int i = e / t, k = e % t;
            if (k <= i) {
                double *dst = M + (int64_t)(j0 + nb + i) * R + j0 + nb + k;
                const double *pi = pan + (nb + i) * DENSE_PS, *pk = pan + (nb + k) * DENSE_PS;
                double s = *dst;
                for (int c = 0; c < nb; c++) s = __builtin_fma(-pi[c], pk[c], s);
                *dst = s;
            }
        }
        __syncthreads();                       // the panel is consumed, the trailing block written
    }
    return true;
}

// The factor's inverse X = F^-1 over F, row by row: X[i][j] = -(sum_{j <= k < i} F[i][k] X[k][j]) / F[i][i], X[i][i] = 1 / F[i][i].
// Row i of F is needed by row i of X only, so it goes through `row` and is overwritten.
[[maybe_unused]] static __device__ void dense_tri_inverse(double *M, int R, double *row /* [R] */) {
    const int tid = threadIdx.x;
    for (int i = 0; i < R; i++) {
        for (int k = tid; k <= i; k += DENSE_WG) row[k] = M[(int64_t)i * R + k];
        __syncthreads();
        const double dii = row[i];
        for (int j = tid; j < i; j += DENSE_WG) {
            double s = 0.0;
            for (int k = j; k < i; k++) s = __builtin_fma(row[k], M[(int64_t)k * R + j], s);
            M[(int64_t)i * R + j] = -s / dii;
        }
        if (tid == 0) M[(int64_t)i * R + i] = 1.0 / dii;
        __syncthreads();
    }
}

// X^T X (+ y y^T) over X, row by row, mirrored into the upper triangle: row i of the result needs rows >= i of X, which later rows
// do not touch.  Column i of X goes through `col`.
[[maybe_unused]] static __device__ void dense_inverse_from_tri(double *M, int R, double *col /* [R] */, const double *y /* [R] or null */) {
    const int tid = threadIdx.x;
    for (int i = 0; i < R; i++) {
        for (int k = i + tid; k < R; k += DENSE_WG) col[k] = M[(int64_t)k * R + i];
        __syncthreads();
        for (int j = tid; j <= i; j += DENSE_WG) {
            double s = 0.0;
            for (int k = i; k < R; k++) s = __builtin_fma(col[k], M[(int64_t)k * R + j], s);
            if (y) s += y[i] * y[j];
            M[(int64_t)i * R + j] = s;
            M[(int64_t)j * R + i] = s;
        }
        __syncthreads();
    }
}

}  // namespace sr
