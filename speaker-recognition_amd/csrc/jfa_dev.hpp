// jfa_dev.hpp -- what jfa.hip (factor estimation), jfa_score.hip (trial scoring), jfa_stats.hip (resident statistics, centring,
// z / d) and plda.hip (the i-vector back end) share: the two handle types, the panel Cholesky of one R x R block by one workgroup
// and the two routines that turn its factor into the inverse, and the host launchers each of the first three defines for the
// others (bw_stats.hip includes it for the statistics handle its resident entry fills).
#pragma once

#include "common.hpp"
#include "jfa.hpp"
#include "jfa_plan.hpp"

#include <vector>

// A factor handle: what sr_jfa_open uploads, or what sr_jfa_open_centred forms on the device (jfa_stats.hip).
struct SRJfa {
    int64_t G = 0;
    int K = 0, D = 0, device = 0;
    sr::DevBuf<double> N, Fc, E, iE;                    // resident for the handle's life
    sr::DevBuf<double> W, WE, P, A, C, Y, B, L;         // per call, grown on demand
    sr::DevBuf<double> zd_d, zd_z, zd_a, zd_b;          // sr_jfa_zd's, grown on demand
    sr::DevBuf<int> flags;
    std::vector<int> h_flags;
};

// Raw statistics of n sessions on one device (jfa_stats.hip): N [n][K], F [n][K D], validated when the handle was made.
struct SRStats {
    int64_t n = 0;
    int K = 0, D = 0, device = 0;
    sr::DevBuf<double> N, F;
};

namespace sr {

constexpr int JFA_PS = JFA_NB + 1;                     // row stride of the Cholesky panel in LDS

// C [M][N] (+)= A B through jfa_gemm_kernel, booked to `kind`; the operands are addressed by (row stride, column stride).
void launch_gemm(TimerKind kind, hipStream_t st, const double *A, int64_t sam, int64_t sak, const double *B, int64_t sbk, int64_t sbn, double *C,
                 int64_t ldc, int64_t M, int64_t N, int64_t Kred, bool accumulate, int diag_step);
// WE = W .* iE over n elements of rows of kd columns (jfa_scale_kernel); P [K][R][R] from W [R][K D] (jfa_gram_kernel).  No timer of their own.
void launch_scale(hipStream_t st, const double *W, const double *iE, double *WE, int64_t n, int64_t kd);
void launch_gram(hipStream_t st, const double *W, const double *iE, double *P, int R, int K, int D);
// jfa.hip: the handle's device and the runtime, as every call on a handle checks them.
void jfa_check_handle(SRJfa &h, const char *what);
// jfa_score.hip: the scoring launches on device-resident statistics dN [T][K], dF [T][K D] and totals d_nt [T] (on the calling thread's
// device; everything else host memory as jfa_score takes it).  `pl`: the plan for this device.
void jfa_score_device(const JfaScorePlan &pl, int64_t T, int64_t J, int K, int D, int Ry, int Ru, const double *dN, const double *dF,
                      const double *d_nt, const double *m, const double *E, const double *d, const double *v, const double *u, const double *z,
                      const double *y, const double *x, const unsigned char *mask, double *out, int64_t *bad_segments);
// jfa_stats.hip: nt [T] = a segment's K counts added in mixture order; returns the segments with nt <= 0 (synchronises).  T_JFA_GRAM.
int64_t launch_segment_totals(hipStream_t st, const double *N, int64_t T, int K, double *nt);
// jfa_stats.hip: the check of a resident pass's result (the texts of jfa_check_raw_stats; synchronises); the live-handle registry.
void stats_check_device(const SRStats &s);
const SRStats &stats_live(const SRStats *s, const char *what);
SRStats *stats_new(int64_t n, int K, int D);      // an empty registered handle on the calling thread's device, buffers allocated

#ifdef __HIPCC__
// jfa.hip's own two triangular solves (its kernels alone call it: device code is not linked across files)
__device__ void jfa_solve(const double *M, int R, double *T, int64_t ldt, int nrhs);

// ---- the factorisation of one R x R block by one workgroup.  M: the block, row stride R, in LDS or in global memory. ----

// Lower Cholesky factor over the lower triangle of M (the upper triangle is not read).  false: a pivot <= 0 or not finite (every
// lane returns the same: the pivot is read from LDS behind a barrier).
[[maybe_unused]] static __device__ bool jfa_cholesky(double *M, int R, double *pan /* [R][JFA_PS] */) {
    const int tid = threadIdx.x;
    for (int j0 = 0; j0 < R; j0 += JFA_NB) {
        const int nb = min(JFA_NB, R - j0), rows = R - j0;
        for (int e = tid; e < rows * nb; e += JFA_WG) {
            const int r = e / nb, c = e % nb;
            pan[r * JFA_PS + c] = M[(int64_t)(j0 + r) * R + j0 + c];
        }
        __syncthreads();
        for (int c = 0; c < nb; c++) {
            const double p = pan[c * JFA_PS + c];
            if (!(p > 0.0) || !__builtin_isfinite(p)) return false;
            const double d = sqrt(p);
            __syncthreads();                   // every lane has read the pivot
            for (int r = c + tid; r < rows; r += JFA_WG) pan[r * JFA_PS + c] = r == c ? d : pan[r * JFA_PS + c] / d;
            __syncthreads();
            const int w = nb - c - 1;
            for (int e = tid; e < (rows - c - 1) * w; e += JFA_WG) {
                const int r = c + 1 + e / w, c2 = c + 1 + e % w;
                if (r >= c2) pan[r * JFA_PS + c2] = __builtin_fma(-pan[r * JFA_PS + c], pan[c2 * JFA_PS + c], pan[r * JFA_PS + c2]);
            }
            __syncthreads();
        }
        for (int e = tid; e < rows * nb; e += JFA_WG) {
            const int r = e / nb, c = e % nb;
            if (r >= c) M[(int64_t)(j0 + r) * R + j0 + c] = pan[r * JFA_PS + c];
        }
        const int t = rows - nb;               // the trailing block, lower triangle: M[i][k] -= sum_c pan[i][c] pan[k][c]
        for (int e = tid; e < t * t; e += JFA_WG) {
            const int i = e / t, k = e % t;
            if (k <= i) {
                double *dst = M + (int64_t)(j0 + nb + i) * R + j0 + nb + k;
                const double *pi = pan + (nb + i) * JFA_PS, *pk = pan + (nb + k) * JFA_PS;
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
[[maybe_unused]] static __device__ void jfa_tri_inverse(double *M, int R, double *row /* [R] */) {
    const int tid = threadIdx.x;
    for (int i = 0; i < R; i++) {
        for (int k = tid; k <= i; k += JFA_WG) row[k] = M[(int64_t)i * R + k];
        __syncthreads();
        const double dii = row[i];
        for (int j = tid; j < i; j += JFA_WG) {
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
[[maybe_unused]] static __device__ void jfa_inverse_from_tri(double *M, int R, double *col /* [R] */, const double *y /* [R] or null */) {
    const int tid = threadIdx.x;
    for (int i = 0; i < R; i++) {
        for (int k = i + tid; k < R; k += JFA_WG) col[k] = M[(int64_t)k * R + i];
        __syncthreads();
        for (int j = tid; j <= i; j += JFA_WG) {
            double s = 0.0;
            for (int k = i; k < R; k++) s = __builtin_fma(col[k], M[(int64_t)k * R + j], s);
            if (y) s += y[i] * y[j];
            M[(int64_t)i * R + j] = s;
            M[(int64_t)j * R + i] = s;
        }
        __syncthreads();
    }
}

#endif

}  // namespace sr
