// dense64.hip -- the float64 dense layer's GEMM (dense64.hpp; the geometry is dense64_plan.hpp's).
//   dense_gemm_kernel   C (+)= A B on v_mfma_f64_16x16x4_f64 with both operands addressed by (row stride, column stride), so one
//                       kernel serves every product of its consumers, transposed or not, without a copy.  A workgroup owns a
//                       64 x 64 tile, a wave 16 rows of it; the operands pass through LDS sixteen reduction steps at a time; rows,
//                       columns and reduction steps beyond the edges are read as zeros.  Accumulating launches start from what C
//                       holds, so a sum that is cut into chunks of whole reduction tiles is the same sequence of matrix
//                       instructions as the uncut one: JFA's A and C over chunks of groups, PLDA's sums over chunks of rows.
// Deterministic: no atomics, one fixed order of the reduction whatever the grid.
#include "dense64.hpp"

namespace sr {

typedef double dense_f64x4 __attribute__((ext_vector_type(4)));

// ---- C [M][N] (+)= A [M][Kred] B [Kred][N], A[m][k] at A + m sam + k sak, B[k][n] at B + k sbk + n sbn.  grid (N / 64, M / 64) ----
// v_mfma_f64_16x16x4_f64: lane l supplies A[row l & 15][k l >> 4] and B[k l >> 4][column l & 15] and receives
// D[row (l >> 4) + 4 r][column l & 15], r = 0..3 (bw_stats.hip).
// diag_step > 0: 1 is added to every column that is a multiple of it (L = I + ...: the diagonal of a flattened R x R row).
__global__ __launch_bounds__(DENSE_WG)
void dense_gemm_kernel(const double *__restrict__ A, int64_t sam, int64_t sak, const double *__restrict__ B, int64_t sbk, int64_t sbn,
                       double *__restrict__ C, int64_t ldc, int M, int64_t N, int64_t Kred, int accumulate, int diag_step) {
    __shared__ double As[DENSE_KSTEP][DENSE_TS], Bs[DENSE_KSTEP][DENSE_TS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, fl = lane >> 4;
    const int64_t m0 = (int64_t)blockIdx.y * DENSE_TILE, n0 = (int64_t)blockIdx.x * DENSE_TILE;
    const bool a_kfast = sak == 1, b_nfast = sbn == 1;
    dense_f64x4 acc[4];
#pragma unroll
    for (int nb = 0; nb < 4; nb++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int64_t row = m0 + wave * 16 + fl + 4 * r, col = n0 + 16 * nb + j;
            acc[nb][r] = (accumulate && row < M && col < N) ? C[row * ldc + col] : 0.0;
        }
    for (int64_t k0 = 0; k0 < Kred; k0 += DENSE_KSTEP) {
        double ra[4], rb[4];
        int am[4], ak[4], bn[4], bk[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int idx = tid + DENSE_WG * e;                    // 0 .. 1023: the 64 x 16 elements of either tile
            am[e] = a_kfast ? idx >> 4 : idx & 63;
            ak[e] = a_kfast ? idx & 15 : idx >> 6;
            bn[e] = b_nfast ? idx & 63 : idx >> 4;
            bk[e] = b_nfast ? idx >> 6 : idx & 15;
            const int64_t gm = m0 + am[e], gka = k0 + ak[e], gn = n0 + bn[e], gkb = k0 + bk[e];
            ra[e] = (gm < M && gka < Kred) ? A[gm * sam + gka * sak] : 0.0;
            rb[e] = (gn < N && gkb < Kred) ? B[gkb * sbk + gn * sbn] : 0.0;
        }
        __syncthreads();                       // the previous tiles have been consumed by every wave
#pragma unroll
        for (int e = 0; e < 4; e++) {
            As[ak[e]][am[e]] = ra[e];
            Bs[bk[e]][bn[e]] = rb[e];
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < DENSE_KSTEP / 4; s++) {
            const double av = As[4 * s + fl][wave * 16 + j];
#pragma unroll
            for (int nb = 0; nb < 4; nb++) acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Bs[4 * s + fl][16 * nb + j], acc[nb], 0, 0, 0);
        }
    }
#pragma unroll
    for (int nb = 0; nb < 4; nb++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int64_t row = m0 + wave * 16 + fl + 4 * r, col = n0 + 16 * nb + j;
            if (row < M && col < N) {
                double v = acc[nb][r];
                if (diag_step > 0 && col % diag_step == 0) v += 1.0;
                C[row * ldc + col] = v;
            }
        }
}

void dense_gemm(TimerKind kind, hipStream_t st, const double *A, int64_t sam, int64_t sak, const double *B, int64_t sbk, int64_t sbn, double *C,
                int64_t ldc, int64_t M, int64_t N, int64_t Kred, bool accumulate, int diag_step) {
    ScopedKernelTimer t(kind);
    const Grid2 g = dense_gemm_grid(M, N);
    hipLaunchKernelGGL(dense_gemm_kernel, dim3((unsigned)g.x, (unsigned)g.y), dim3(DENSE_WG), 0, st, A, sam, sak, B, sbk, sbn, C, ldc, (int)M, N, Kred,
                       accumulate ? 1 : 0, diag_step);
    SR_HIP(hipGetLastError());
}

}  // namespace sr
