// plda.hip -- the i-vector back end on the device, float64 throughout: centring, whitening / WCCN (A = chol(Sigma)^-1), length
// normalisation, cosine scoring, and the two-covariance Gaussian PLDA  x_ij = mu + y_i + e_ij,  y ~ N(0, Sb),  e ~ N(0, Sw).
// With n_i the vectors of speaker i, f_i = sum_j (x_ij - mu), T2 = sum (x - mu)(x - mu)^T, S speakers, n vectors, one EM round is
//   Phi_c = (Sb^-1 + c Sw^-1)^-1  per distinct count c        yhat_i = Phi_{n_i} Sw^-1 f_i
//   Sb <- (sum_i Phi_{n_i} + Yhat^T Yhat) / S
//   Sw <- (T2 - F^T Yhat - Yhat^T F + Yhat^T diag(n_i) Yhat + sum_i n_i Phi_{n_i}) / n
// and the log-likelihood ratio of model j (n_j = c enrolment vectors, f_j = e_j - c mu) against segment t (x = x_t - mu) is
//   -1/2 ln det(Phi_c + Sw) - 1/2 (x - yhat_j)^T P_c (x - yhat_j) + 1/2 ln det(Sb + Sw) + 1/2 x^T P_0 x,
//   P_c = (Phi_c + Sw)^-1,  P_0 = (Sb + Sw)^-1,  the quadratic form taken apart as  a_t - 2 (Yhat P_c X^T)[j][t] + q_j.
// The speakers (models) are sorted by count in the plan (plda_plan.cpp), so a count class is a contiguous row range; every product
// goes through the dense layer's GEMM (dense64.hpp: both operands addressed by strides, so no transposed copies; the sums over rows
// and over speakers are accumulating launches of PLDA_SUM_CHUNK rows, whole reduction tiles).  The kernels here:
//   plda_centre_kernel       out[r] = X[src[r]] - coef[r] M[midx[r]]: centring, the gather into sorted order, the class means of WCCN.
//   plda_class_sums_kernel   F[s] = the sum of the sorted speaker's rows, in row order: a segmented sum, a lane per (speaker, column).
//   plda_combine_kernel      out[b] = A[b] + coef[b] B over a batch of R x R blocks (Sb^-1 + c Sw^-1; Phi_c + Sw; a covariance / n).
//   plda_invert_kernel       one workgroup per R x R SPD block: dense_cholesky (dense64_dev.hpp) and the log-determinant off the factor's
//                            diagonal.  For
//                            R <= jfa_lds_rows the block is in LDS and the same workgroup goes on to the factor's inverse
//                            (whitening) and the inverse over the block (mirrored: symmetric to the bit).  Above, the block is
//                            factored in place in global memory, and
//   plda_tri_inverse_kernel  takes the factor's inverse X a wave per column across the chip; the inverse X^T X is then a product.
//   plda_scale_rows_kernel   n_i yhat_i.
//   plda_update_kernel       the two new covariances from the five sums, the lower triangle computed and mirrored.
//   plda_rowdot_kernel       out[r] = <A[r], B[r]>, a wave per row: lane l adds columns l, l + 64, ... then a fixed tree.
//   plda_rownorm_kernel      a row scaled to unit 2-norm, a wave per row; a norm that is 0 or not finite: exact zeros, flagged.
//   plda_assemble_kernel     streams over the cross term where the GEMM left it in the output and forms the score (or the cosine).
// Degenerate inputs: a block that does not factor is zeroed and flagged.  Training stops there and returns the last pair that
// factored, with the iteration and a stop code; scoring writes exact zeros into the class's rows and counts the class.
// Deterministic: no atomics; every sum has a fixed order; a score depends on its model's count and sum and on its segment only, so
// neither the batch nor the chunking of the segments under "plda_scratch_mib" shows, bit for bit.
// The launchers and host helpers named plda_* are declared in eig_dev.hpp: backend_eig.hip calls the same ones.
#include "dense64.hpp"
#include "dense64_dev.hpp"
#include "eig_dev.hpp"
#include "jfa.hpp"              // the option jfa_lds_rows, nothing else of JFA's
#include "plda_plan.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <vector>

namespace sr {

static_assert(PLDA_WG == DENSE_WG, "the factorisation is written for DENSE_WG lanes");
// Rows of at least this many scores (64 KiB) go from the device straight to their model's place in the result; shorter rows come
// back in one copy and are put in place on the host (a copy per row of 16 KB measured slower than that: 19 against 16 ms at 200 x 2000).
constexpr int64_t PLDA_ROW_COPY_MIN = 8192;

// out [rows][R]; src, midx, coef may each be null: row r itself, row 0 of M, 1.
__global__ __launch_bounds__(PLDA_WG)
void plda_centre_kernel(const double *__restrict__ X, const int64_t *__restrict__ src, const double *__restrict__ M,
                        const int64_t *__restrict__ midx, const double *__restrict__ coef, double *__restrict__ out, int64_t rows, int R) {
    const int64_t e = (int64_t)blockIdx.x * PLDA_WG + threadIdx.x;
    if (e >= rows * R) return;
    const int64_t r = e / R;
    const int k = (int)(e % R);
    const double x = X[(src ? src[r] : r) * R + k], m = M[(midx ? midx[r] : 0) * R + k];
    out[e] = coef ? __builtin_fma(-coef[r], m, x) : x - m;
}

// grid (S, blocks of 256 columns)
__global__ __launch_bounds__(PLDA_WG)
void plda_class_sums_kernel(const double *__restrict__ Xs, const int64_t *__restrict__ row_start, double *__restrict__ F, int R) {
    const int64_t s = blockIdx.x;
    const int k = blockIdx.y * PLDA_WG + threadIdx.x;
    if (k >= R) return;
    double acc = 0.0;
    for (int64_t r = row_start[s]; r < row_start[s + 1]; r++) acc += Xs[r * R + k];
    F[s * R + k] = acc;
}

// out [nb][rr] = A[b * stride_a] (0 without A) + coef[b] B
__global__ __launch_bounds__(PLDA_WG)
void plda_combine_kernel(const double *__restrict__ A, int64_t stride_a, const double *__restrict__ B, const double *__restrict__ coef,
                         double *__restrict__ out, int64_t nb, int64_t rr) {
    const int64_t e = (int64_t)blockIdx.x * PLDA_WG + threadIdx.x;
    if (e >= nb * rr) return;
    const int64_t b = e / rr, i = e % rr;
    out[e] = __builtin_fma(coef[b], B[i], A ? A[b * stride_a + i] : 0.0);
}

// The sum of v over the wave by a fixed tree; lane 0 holds it.
static __device__ inline double plda_wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// mode 0: the block's inverse over the block; mode 1: the inverse of its lower Cholesky factor, the upper triangle zeros; mode 2:
// the factor itself, the upper triangle zeros.  logdet [n]: ln det of the block.  A block that does not factor: zeros, logdet 0, flag 1.
__global__ __launch_bounds__(PLDA_WG)
void plda_invert_kernel(double *__restrict__ blocks, int R, int use_lds, int mode, double *__restrict__ logdet, int *__restrict__ flags) {
    extern __shared__ double plda_lds[];
    double *pan = plda_lds;                    // [R][DENSE_PS]
    double *buf = pan + (size_t)R * DENSE_PS;    // [R]
    double *mat = buf + R;                     // [R][R], LDS path only
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    const int rr = R * R;
    double *Mg = blocks + g * rr;
    double *M = Mg;
    if (use_lds) {
        for (int e = tid; e < rr; e += PLDA_WG) mat[e] = Mg[e];
        M = mat;
        __syncthreads();
    }
    const bool ok = dense_cholesky(M, R, pan);
    __syncthreads();
    if (!ok) {
        for (int e = tid; e < rr; e += PLDA_WG) Mg[e] = 0.0;
        if (tid == 0) logdet[g] = 0.0, flags[g] = 1;
        return;
    }
    if (tid == 0) {                            // (before the inverse overwrites the diagonal: lane 0 writes it there too)
        double s = 0.0;
        for (int i = 0; i < R; i++) s += log(M[(int64_t)i * R + i]);
        logdet[g] = 2.0 * s;
        flags[g] = 0;
    }
    if (mode != 2) dense_tri_inverse(M, R, buf);
    if (mode == 0) {
        dense_inverse_from_tri(M, R, buf, nullptr);
    } else {
        for (int e = tid; e < rr; e += PLDA_WG)
            if (e % R > e / R) M[e] = 0.0;
        __syncthreads();
    }
    if (use_lds)
        for (int e = tid; e < rr; e += PLDA_WG) Mg[e] = mat[e];
}

// X = L^-1 of the factors L [n][R][R] (lower triangles) by forward substitution, column j by one wave: x_j = 1 / L_jj,
// x_i = -(sum_{j <= k < i} L_ik x_k) / L_ii, the sum over 64 lanes (lane l the terms j + l, j + l + 64, ...) and a fixed tree.  The four
// columns of a workgroup step through the rows together.  X's upper triangle is zeros; a block with its flag set gives zeros.
// grid (n, R / 4)
__global__ __launch_bounds__(PLDA_WG)
void plda_tri_inverse_kernel(const double *__restrict__ L, double *__restrict__ X, int R, const int *__restrict__ flags) {
    __shared__ double xs[PLDA_ROWS_PER_WG][PLDA_MAX_R];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t g = blockIdx.x;
    const int j0 = blockIdx.y * PLDA_ROWS_PER_WG, j = j0 + wave;
    const double *Lg = L + g * R * R;
    double *Xg = X + g * R * R;
    if (flags[g] != 0) {                       // (the whole workgroup: no barrier is left behind)
        if (j < R)
            for (int i = lane; i < R; i += 64) Xg[i * R + j] = 0.0;
        return;
    }
    if (j < R && lane == 0) xs[wave][j] = 1.0 / Lg[j * R + j];
    __syncthreads();
    for (int i = j0 + 1; i < R; i++) {
        if (j < i) {                           // (wave-uniform)
            double s = 0.0;
            for (int k = j + lane; k < i; k += 64) s = __builtin_fma(Lg[i * R + k], xs[wave][k], s);
            s = plda_wave_sum(s);
            if (lane == 0) xs[wave][i] = -s / Lg[i * R + i];
        }
        __syncthreads();
    }
    if (j < R)
        for (int i = lane; i < R; i += 64) Xg[i * R + j] = i < j ? 0.0 : xs[wave][i];
}

__global__ __launch_bounds__(PLDA_WG)
void plda_scale_rows_kernel(const double *__restrict__ Y, const double *__restrict__ w, double *__restrict__ out, int64_t rows, int R) {
    const int64_t e = (int64_t)blockIdx.x * PLDA_WG + threadIdx.x;
    if (e < rows * R) out[e] = w[e / R] * Y[e];
}

// Sb' = (sum_c size_c Phi_c + YY) / S,  Sw' = (T2 - FY - FY^T + YnY + sum_c size_c count_c Phi_c) / n, classes added in order.
// YnY = Yhat^T (n .* Yhat) is symmetric but for rounding: the mean of the two halves is taken.  bad[0] = 1: a non-finite value.
__global__ __launch_bounds__(PLDA_WG)
void plda_update_kernel(const double *__restrict__ Phi, const double *__restrict__ cls_size, const double *__restrict__ cls_count, int nc,
                        const double *__restrict__ T2, const double *__restrict__ FY, const double *__restrict__ YY,
                        const double *__restrict__ YnY, double S, double n, int R, double *__restrict__ Sb, double *__restrict__ Sw,
                        int *__restrict__ bad) {
    const int e = blockIdx.x * PLDA_WG + threadIdx.x;
    const int rr = R * R;
    if (e >= rr) return;
    const int i = e / R, j = e % R;
    if (j > i) return;
    const int t = j * R + i;
    double sp = 0.0, snp = 0.0;
    for (int c = 0; c < nc; c++) {
        const double phi = Phi[(int64_t)c * rr + e];
        sp = __builtin_fma(cls_size[c], phi, sp);
        snp = __builtin_fma(cls_size[c] * cls_count[c], phi, snp);
    }
    const double sb = (sp + YY[e]) / S;
    const double sw = (((T2[e] - (FY[e] + FY[t])) + 0.5 * (YnY[e] + YnY[t])) + snp) / n;
    Sb[e] = Sb[t] = sb;
    Sw[e] = Sw[t] = sw;
    if (!__builtin_isfinite(sb) || !__builtin_isfinite(sw)) bad[0] = 1;
}

__global__ __launch_bounds__(PLDA_WG)
void plda_rowdot_kernel(const double *__restrict__ A, const double *__restrict__ B, double *__restrict__ out, int64_t rows, int R) {
    const int64_t row = (int64_t)blockIdx.x * PLDA_ROWS_PER_WG + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    double s = 0.0;
    for (int k = lane; k < R; k += 64) s = __builtin_fma(A[row * R + k], B[row * R + k], s);
    s = plda_wave_sum(s);
    if (lane == 0) out[row] = s;
}

__global__ __launch_bounds__(PLDA_WG)
void plda_rownorm_kernel(double *__restrict__ Y, int64_t rows, int R, int *__restrict__ flags) {
    const int64_t row = (int64_t)blockIdx.x * PLDA_ROWS_PER_WG + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    double s = 0.0;
    for (int k = lane; k < R; k += 64) s = __builtin_fma(Y[row * R + k], Y[row * R + k], s);
    const double nrm = sqrt(__shfl(plda_wave_sum(s), 0));
    const bool ok = nrm > 0.0 && __builtin_isfinite(nrm);
    for (int k = lane; k < R; k += 64) Y[row * R + k] = ok ? Y[row * R + k] / nrm : 0.0;
    if (lane == 0) flags[row] = ok ? 0 : 1;
}

// out[row0 + r][t0 + c], r < rows, c < cols, holds the cross term (row stride ld).  q [rows] from row0; a, a0 [cols].
// mode 0: the PLDA score (`ok` 0: exact zeros);  mode 1: the cosine, q and a the squared norms (a norm that is 0 or not finite: 0).
__global__ __launch_bounds__(PLDA_WG)
void plda_assemble_kernel(int mode, double *__restrict__ out, int64_t ld, int64_t row0, int64_t t0, int64_t rows, int64_t cols,
                          const double *__restrict__ q, const double *__restrict__ a, const double *__restrict__ a0, double ld_c, double ld_0,
                          int ok) {
    const int64_t e = (int64_t)blockIdx.x * PLDA_WG + threadIdx.x;
    if (e >= rows * cols) return;
    const int64_t r = e / cols, c = e % cols;
    double *p = out + (row0 + r) * ld + t0 + c;
    const double cross = *p;
    double v = 0.0;
    if (mode == 0) {
        if (ok) {
            const double quad = (a[c] - 2.0 * cross) + q[row0 + r];
            v = 0.5 * ((ld_0 - ld_c) + (a0[c] - quad));
        }
    } else {
        const double d = sqrt(q[row0 + r]) * sqrt(a[c]);
        if (d > 0.0 && __builtin_isfinite(d)) v = cross / d;
    }
    *p = v;
}

// ---- host ----

static std::atomic<long> &plda_scratch_option() {
    static std::atomic<long> v{(long)(PLDA_DEFAULT_SCRATCH >> 20)};
    return v;
}
void set_plda_scratch_mib(long v) { plda_scratch_option().store(v); }
long plda_scratch_mib() { return plda_scratch_option().load(); }

namespace {
struct PldaScratch {
    DevBuf<double> X, Xc, Xw, F, G, Y, Yn, M, Z, mu, coef, w, q, a, a0, out;
    DevBuf<double> pairs, work, phi, pc, tri, T2, FY, YY, YnY, logdet, cls_size, cls_count;
    DevBuf<int64_t> order, start, midx;
    DevBuf<int> flags, bad;
};
}  // namespace

static unsigned flat_blocks(int64_t n) { return (unsigned)((n + PLDA_WG - 1) / PLDA_WG); }

void plda_launch_centre(hipStream_t st, const double *X, const int64_t *src, const double *M, const int64_t *midx, const double *coef, double *out,
                          int64_t rows, int R) {
    ScopedKernelTimer tm(T_JFA_GRAM);
    hipLaunchKernelGGL(plda_centre_kernel, dim3(flat_blocks(rows * R)), dim3(PLDA_WG), 0, st, X, src, M, midx, coef, out, rows, R);
    SR_HIP(hipGetLastError());
}

void plda_launch_class_sums(hipStream_t st, const double *Xs, const int64_t *row_start, double *F, int64_t S, int R) {
    ScopedKernelTimer tm(T_JFA_GRAM);
    hipLaunchKernelGGL(plda_class_sums_kernel, dim3((unsigned)S, (unsigned)((R + PLDA_WG - 1) / PLDA_WG)), dim3(PLDA_WG), 0, st, Xs, row_start, F, R);
    SR_HIP(hipGetLastError());
}

void plda_launch_combine(hipStream_t st, const double *A, int64_t stride_a, const double *B, const double *coef, double *out, int64_t nb, int R) {
    ScopedKernelTimer tm(T_JFA_GRAM);
    const int64_t rr = (int64_t)R * R;
    hipLaunchKernelGGL(plda_combine_kernel, dim3(flat_blocks(nb * rr)), dim3(PLDA_WG), 0, st, A, stride_a, B, coef, out, nb, rr);
    SR_HIP(hipGetLastError());
}

// Inverts n blocks in place; the flags and the log-determinants come back to the host (synchronises).  Returns the blocks that failed.
int64_t plda_invert_blocks(hipStream_t st, const PldaPlan &pl, double *blocks, int64_t n, int mode, std::vector<int> &flags, std::vector<double> &logdet) {
    auto &w = per_device<PldaScratch>();
    static int attr_set[MAX_DEVICES] = {};
    if (attr_set[ctx().device] < pl.factor_lds) {
        SR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&plda_invert_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, pl.factor_lds));
        attr_set[ctx().device] = pl.factor_lds;
    }
    w.flags.ensure((size_t)n);
    w.logdet.ensure((size_t)n);
    const int R = pl.R;
    const int64_t rr = (int64_t)R * R;
    {
        ScopedKernelTimer tm(T_JFA_FACTOR);
        hipLaunchKernelGGL(plda_invert_kernel, dim3((unsigned)n), dim3(PLDA_WG), (size_t)pl.factor_lds, st, blocks, R, pl.path == 0 ? 1 : 0,
                           pl.path == 0 ? mode : 2, w.logdet.p, w.flags.p);
        SR_HIP(hipGetLastError());
    }
    if (pl.path != 0) {
        // In global memory one workgroup's row-by-row inverse waits on a chain of R^2 / 2 loads; here the factor's inverse X is taken
        // a wave per column across the chip, and the inverse X^T X is a product (symmetric to the bit: the same terms in the same order).
        w.tri.ensure((size_t)(n * rr));
        {
            ScopedKernelTimer tm(T_JFA_FACTOR);
            hipLaunchKernelGGL(plda_tri_inverse_kernel, dim3((unsigned)n, (unsigned)pl.tri.y), dim3(PLDA_WG), 0,
                               st, blocks, w.tri.p, R, w.flags.p);
            SR_HIP(hipGetLastError());
        }
        if (mode == 0)
            for (int64_t g = 0; g < n; g++) dense_gemm(T_JFA_FACTOR, st, w.tri.p + g * rr, 1, R, w.tri.p + g * rr, R, 1, blocks + g * rr, R, R, R, R, false, 0);
        else
            SR_HIP(hipMemcpyAsync(blocks, w.tri.p, (size_t)(n * rr) * 8, hipMemcpyDeviceToDevice, st));
    }
    flags.resize((size_t)n);
    logdet.resize((size_t)n);
    w.flags.download(flags.data(), (size_t)n);
    w.logdet.download(logdet.data(), (size_t)n);
    sync_stream();
    int64_t bad = 0;
    for (int f : flags) bad += f != 0;
    return bad;
}

void plda_launch_rowdot(hipStream_t st, const double *A, const double *B, double *out, int64_t rows, int R) {
    ScopedKernelTimer tm(T_JFA_GRAM);
    hipLaunchKernelGGL(plda_rowdot_kernel, dim3((unsigned)((rows + PLDA_ROWS_PER_WG - 1) / PLDA_ROWS_PER_WG)), dim3(PLDA_WG), 0, st, A, B, out, rows, R);
    SR_HIP(hipGetLastError());
}

static void launch_assemble(hipStream_t st, int mode, double *out, int64_t ld, int64_t row0, int64_t t0, int64_t rows, int64_t cols, const double *q,
                            const double *a, const double *a0, double ld_c, double ld_0, bool ok) {
    ScopedKernelTimer tm(T_JFA_UPDATE);
    hipLaunchKernelGGL(plda_assemble_kernel, dim3(flat_blocks(rows * cols)), dim3(PLDA_WG), 0, st, mode, out, ld, row0, t0, rows, cols, q, a, a0, ld_c,
                       ld_0, ok ? 1 : 0);
    SR_HIP(hipGetLastError());
}

// C [R][R] (+)= A^T B over the rows r0 .. of A, B [rows][R], `chunk` rows a launch, in order.
void plda_accumulate_gram(hipStream_t st, const double *A, const double *B, double *C, int64_t rows, int64_t chunk, int R) {
    for (int64_t r0 = 0; r0 < rows; r0 += chunk) {
        const int64_t n = std::min(chunk, rows - r0);
        dense_gemm(T_JFA_GEMM_A, st, A + r0 * R, 1, R, B + r0 * R, R, 1, C, R, R, R, n, r0 > 0, 0);
    }
}

// The mean of the rows, column by column in row order.
std::vector<double> plda_row_mean(const double *X, int64_t n, int R) {
    std::vector<double> mu((size_t)R, 0.0);
    for (int64_t i = 0; i < n; i++)
        for (int k = 0; k < R; k++) mu[(size_t)k] += X[i * R + k];
    for (int k = 0; k < R; k++) mu[(size_t)k] /= (double)n;
    return mu;
}

// The lower triangle mirrored: what the device reads of a covariance that is symmetric but for rounding.
std::vector<double> plda_mirrored(const double *M, int R) {
    std::vector<double> out((size_t)R * R);
    for (int i = 0; i < R; i++)
        for (int j = 0; j <= i; j++) out[(size_t)i * R + j] = out[(size_t)j * R + i] = M[(int64_t)i * R + j];
    return out;
}

void plda_launch_rownorm(hipStream_t st, double *Y, int64_t rows, int R, int *flags) {
    ScopedKernelTimer tm(T_JFA_UPDATE);
    hipLaunchKernelGGL(plda_rownorm_kernel, dim3((unsigned)((rows + PLDA_ROWS_PER_WG - 1) / PLDA_ROWS_PER_WG)), dim3(PLDA_WG), 0, st, Y, rows, R, flags);
    SR_HIP(hipGetLastError());
}

void plda_check_device(const char *what) {
    if (gpu_runtime_lost()) fail_gpu_runtime_lost(what);
    ensure_device();
}

void plda_check_matrix(const double *X, int64_t n, int R, const char *name, const char *rows_name) {
    std::string why;
    if (!plda_check_rank(R, why) || !plda_check_rows(n, rows_name, why)) fail("%s", why.c_str());
    if (!X) fail("PLDA back end: null argument (%s)", name);
    if (!plda_check_finite(X, n * R, name, why)) fail("%s", why.c_str());
}

// Uploads X, centres it by its mean in the plan's sorted row order (w.Xc) and, with `sums`, adds up the speakers' rows (w.F).  -> mu
static std::vector<double> centre_and_sum(hipStream_t st, PldaScratch &w, const PldaPlan &pl, const double *X, bool sums) {
    const int64_t n = pl.rows, S = pl.groups;
    const int R = pl.R;
    std::vector<double> mu = plda_row_mean(X, n, R);
    w.X.upload(X, (size_t)(n * R));
    w.mu.upload(mu.data(), (size_t)R);
    w.order.upload(pl.row_order.data(), (size_t)n);
    w.start.upload(pl.row_start.data(), (size_t)S + 1);
    w.Xc.ensure((size_t)(n * R));
    w.F.ensure((size_t)(S * R));
    plda_launch_centre(st, w.X.p, w.order.p, w.mu.p, nullptr, nullptr, w.Xc.p, n, R);
    if (sums) plda_launch_class_sums(st, w.Xc.p, w.start.p, w.F.p, S, R);
    sync_stream();                             // (mu and the plan's tables are host memory of this frame)
    return mu;
}

void plda_train(int64_t n, int R, const double *X, const int64_t *ids, int64_t S, int n_iter, int default_start, double *mu_out, double *Sb,
                double *Sw, int *iterations, int *n_classes, int *stop) {
    std::string why;
    plda_check_matrix(X, n, R, "X, the training vectors [n][R]", "n, the number of training vectors");
    if (!Sb || !Sw) fail("PLDA training: null argument (Sb and Sw [R][R], the start and the result)");
    if (n_iter < 1) fail("PLDA training: n_iter is %d; run at least one iteration (n_iter >= 1)", n_iter);
    if (default_start != 0 && default_start != 1) fail("PLDA training: default_start is 0 (Sb and Sw hold the start) or 1 (both start from half the total covariance)");
    if (!default_start && (!plda_check_symmetric(Sb, R, "Sb", why) || !plda_check_symmetric(Sw, R, "Sw", why))) fail("%s", why.c_str());
    PldaPlan pl;
    if (!plan_plda_train(n, R, ids, S, (int)jfa_lds_rows(), 1, pl, why)) fail("%s", why.c_str());
    plda_check_device("sr_plda_train");
    if (!plan_plda_train(n, R, ids, S, (int)jfa_lds_rows(), std::max(1, ctx().n_cu), pl, why)) fail("%s", why.c_str());
    hipStream_t st = ctx().stream;
    auto &w = per_device<PldaScratch>();
    const int64_t rr = (int64_t)R * R, nc = (int64_t)pl.classes.size();
    const std::vector<double> mu = centre_and_sum(st, w, pl, X, true);
    w.T2.ensure((size_t)rr), w.FY.ensure((size_t)rr), w.YY.ensure((size_t)rr), w.YnY.ensure((size_t)rr);
    plda_accumulate_gram(st, w.Xc.p, w.Xc.p, w.T2.p, n, pl.sum_chunk, R);
    // the tables: a speaker's count (sorted order), the classes' counts and sizes
    std::vector<double> wn((size_t)S), csize((size_t)nc), ccount((size_t)nc);
    for (int64_t c = 0; c < nc; c++) {
        csize[(size_t)c] = (double)pl.classes[(size_t)c].size, ccount[(size_t)c] = (double)pl.classes[(size_t)c].count;
        for (int64_t s = 0; s < pl.classes[(size_t)c].size; s++) wn[(size_t)(pl.classes[(size_t)c].start + s)] = ccount[(size_t)c];
    }
    w.w.upload(wn.data(), (size_t)S);
    w.cls_size.upload(csize.data(), (size_t)nc);
    w.cls_count.upload(ccount.data(), (size_t)nc);
    std::vector<double> start, start_w;
    const double half[2] = {0.5 / (double)n, 0.5 / (double)n};
    w.pairs.ensure((size_t)(6 * rr));          // three pairs (Sb, Sw): the last that factored, the current, the next
    w.work.ensure((size_t)(2 * rr));
    w.phi.ensure((size_t)(nc * rr));
    w.G.ensure((size_t)(S * R)), w.Y.ensure((size_t)(S * R)), w.Yn.ensure((size_t)(S * R));
    w.bad.ensure(1);
    if (default_start) {                       // Sb = Sw = T2 / (2 n): half the total covariance each (T2 is symmetric to the bit)
        w.coef.upload(half, 2);
        plda_launch_combine(st, nullptr, 0, w.T2.p, w.coef.p, w.pairs.p, 2, R);
    } else {
        start = plda_mirrored(Sb, R), start_w = plda_mirrored(Sw, R);
        SR_HIP(hipMemcpyAsync(w.pairs.p, start.data(), (size_t)rr * 8, hipMemcpyHostToDevice, st));
        SR_HIP(hipMemcpyAsync(w.pairs.p + rr, start_w.data(), (size_t)rr * 8, hipMemcpyHostToDevice, st));
    }
    int good = 0, cur = 0, done = 0, code = PLDA_STOP_NONE;
    std::vector<int> flags;
    std::vector<double> logdet;
    for (int it = 0; it < n_iter; it++) {
        double *pair = w.pairs.p + (int64_t)cur * 2 * rr;
        SR_HIP(hipMemcpyAsync(w.work.p, pair, (size_t)(2 * rr) * 8, hipMemcpyDeviceToDevice, st));
        if (plda_invert_blocks(st, pl, w.work.p, 2, 0, flags, logdet)) {
            code = flags[0] ? PLDA_STOP_SB : PLDA_STOP_SW;
            break;
        }
        const double *iSb = w.work.p, *iSw = w.work.p + rr;
        plda_launch_combine(st, iSb, 0, iSw, w.cls_count.p, w.phi.p, nc, R);               // Sb^-1 + c Sw^-1
        if (plda_invert_blocks(st, pl, w.phi.p, nc, 0, flags, logdet)) {
            code = PLDA_STOP_PHI;
            break;
        }
        good = cur;
        dense_gemm(T_JFA_GEMM_B, st, w.F.p, R, 1, iSw, R, 1, w.G.p, R, S, R, R, false, 0);                                   // G = F Sw^-1
        for (int64_t c = 0; c < nc; c++) {
            const PldaClass &k = pl.classes[(size_t)c];
            dense_gemm(T_JFA_GEMM_L, st, w.G.p + k.start * R, R, 1, w.phi.p + c * rr, R, 1, w.Y.p + k.start * R, R, k.size, R, R, false, 0);      // Yhat_c = G_c Phi_c
        }
        {
            ScopedKernelTimer tm(T_JFA_GRAM);
            hipLaunchKernelGGL(plda_scale_rows_kernel, dim3(flat_blocks(S * R)), dim3(PLDA_WG), 0, st, w.Y.p, w.w.p, w.Yn.p, S, R);
            SR_HIP(hipGetLastError());
        }
        plda_accumulate_gram(st, w.Y.p, w.Y.p, w.YY.p, S, pl.grp_chunk, R);
        plda_accumulate_gram(st, w.F.p, w.Y.p, w.FY.p, S, pl.grp_chunk, R);
        plda_accumulate_gram(st, w.Y.p, w.Yn.p, w.YnY.p, S, pl.grp_chunk, R);
        int next = 0;
        while (next == good || next == cur) next++;
        double *np = w.pairs.p + (int64_t)next * 2 * rr;
        SR_HIP(hipMemsetAsync(w.bad.p, 0, sizeof(int), st));
        {
            ScopedKernelTimer tm(T_JFA_UPDATE);
            hipLaunchKernelGGL(plda_update_kernel, dim3(flat_blocks(rr)), dim3(PLDA_WG), 0, st, w.phi.p, w.cls_size.p, w.cls_count.p, (int)nc, w.T2.p,
                               w.FY.p, w.YY.p, w.YnY.p, (double)S, (double)n, R, np, np + rr, w.bad.p);
            SR_HIP(hipGetLastError());
        }
        int bad = 0;
        w.bad.download(&bad, 1);
        sync_stream();
        if (bad) {
            code = PLDA_STOP_NON_FINITE;
            break;
        }
        cur = next;
        done++;
    }
    const int ret = code == PLDA_STOP_NONE ? cur : good;
    if (code != PLDA_STOP_NONE && code != PLDA_STOP_NON_FINITE && good != cur) done--;      // (the pair that did not factor is dropped)
    SR_HIP(hipMemcpyAsync(Sb, w.pairs.p + (int64_t)ret * 2 * rr, (size_t)rr * 8, hipMemcpyDeviceToHost, st));
    SR_HIP(hipMemcpyAsync(Sw, w.pairs.p + (int64_t)ret * 2 * rr + rr, (size_t)rr * 8, hipMemcpyDeviceToHost, st));
    sync_stream();
    if (mu_out) std::memcpy(mu_out, mu.data(), (size_t)R * 8);
    if (iterations) *iterations = done;
    if (n_classes) *n_classes = (int)nc;
    if (stop) *stop = code;
}

void plda_score(int64_t J, int64_t T, int R, const double *mu, const double *Sb, const double *Sw, const double *E, const int64_t *enrol_n,
                const double *X, double *out, int64_t *bad_classes) {
    std::string why;
    plda_check_matrix(E, J, R, "E, the models' enrolment sums [J][R]", "J, the number of models");
    plda_check_matrix(X, T, R, "X, the test vectors [T][R]", "T, the number of test segments");
    if (!mu || !Sb || !Sw || !out) fail("PLDA scoring: null argument (mu [R], Sb and Sw [R][R] and out [J][T] are all required)");
    if (!plda_check_finite(mu, R, "mu", why) || !plda_check_symmetric(Sb, R, "Sb", why) || !plda_check_symmetric(Sw, R, "Sw", why))
        fail("%s", why.c_str());
    PldaPlan pl;
    const int64_t bound = (int64_t)plda_scratch_mib() << 20;
    if (!plan_plda_score(J, T, R, enrol_n, bound, (int)jfa_lds_rows(), 1, pl, why)) fail("%s", why.c_str());
    plda_check_device("sr_plda_score");
    if (!plan_plda_score(J, T, R, enrol_n, bound, (int)jfa_lds_rows(), std::max(1, ctx().n_cu), pl, why)) fail("%s", why.c_str());
    hipStream_t st = ctx().stream;
    auto &w = per_device<PldaScratch>();
    const int64_t rr = (int64_t)R * R, nc = (int64_t)pl.classes.size(), chunk = pl.chunk;
    // the models in sorted order, their counts
    std::vector<double> Es((size_t)(J * R)), cnt((size_t)J), ccount((size_t)nc), ones((size_t)nc + 1, 1.0);
    bool identity = true;
    for (int64_t s = 0; s < J; s++) {
        const int64_t j = pl.perm[(size_t)s];
        identity = identity && j == s;
        std::memcpy(&Es[(size_t)(s * R)], E + j * R, (size_t)R * 8);
        cnt[(size_t)s] = (double)enrol_n[j];
    }
    for (int64_t c = 0; c < nc; c++) ccount[(size_t)c] = (double)pl.classes[(size_t)c].count;
    const std::vector<double> sb = plda_mirrored(Sb, R), sw = plda_mirrored(Sw, R);
    w.X.upload(Es.data(), (size_t)(J * R));
    w.mu.upload(mu, (size_t)R);
    w.coef.upload(cnt.data(), (size_t)J);
    w.cls_count.upload(ccount.data(), (size_t)nc);
    w.cls_size.upload(ones.data(), (size_t)nc + 1);
    w.pairs.ensure((size_t)(2 * rr)), w.work.ensure((size_t)(2 * rr));
    w.phi.ensure((size_t)(nc * rr)), w.pc.ensure((size_t)((nc + 1) * rr));
    w.F.ensure((size_t)(J * R)), w.G.ensure((size_t)(J * R)), w.Y.ensure((size_t)(J * R)), w.M.ensure((size_t)(J * R)), w.q.ensure((size_t)J);
    w.Xc.ensure((size_t)(chunk * R)), w.Z.ensure((size_t)(chunk * R)), w.a.ensure((size_t)chunk), w.a0.ensure((size_t)chunk);
    w.out.ensure((size_t)(J * T));
    SR_HIP(hipMemcpyAsync(w.pairs.p, sb.data(), (size_t)rr * 8, hipMemcpyHostToDevice, st));
    SR_HIP(hipMemcpyAsync(w.pairs.p + rr, sw.data(), (size_t)rr * 8, hipMemcpyHostToDevice, st));
    SR_HIP(hipMemcpyAsync(w.work.p, w.pairs.p, (size_t)(2 * rr) * 8, hipMemcpyDeviceToDevice, st));
    const double *dSb = w.pairs.p, *dSw = w.pairs.p + rr, *iSb = w.work.p, *iSw = w.work.p + rr;
    std::vector<int> flags, phi_flags;
    std::vector<double> logdet;
    std::vector<char> ok((size_t)nc, 1);
    bool all_bad = plda_invert_blocks(st, pl, w.work.p, 2, 0, flags, logdet) != 0;
    double ld_0 = 0.0;
    if (!all_bad) {
        plda_launch_combine(st, iSb, 0, iSw, w.cls_count.p, w.phi.p, nc, R);                // Sb^-1 + c Sw^-1
        plda_invert_blocks(st, pl, w.phi.p, nc, 0, phi_flags, logdet);
        plda_launch_combine(st, w.phi.p, rr, dSw, w.cls_size.p, w.pc.p, nc, R);             // Phi_c + Sw
        plda_launch_combine(st, dSb, 0, dSw, w.cls_size.p, w.pc.p + nc * rr, 1, R);         // Sb + Sw
        plda_invert_blocks(st, pl, w.pc.p, nc + 1, 0, flags, logdet);
        all_bad = flags[(size_t)nc] != 0;
        ld_0 = logdet[(size_t)nc];
        for (int64_t c = 0; c < nc; c++) ok[(size_t)c] = !phi_flags[(size_t)c] && !flags[(size_t)c];
    }
    if (all_bad) std::fill(ok.begin(), ok.end(), 0);
    int64_t bad = 0;
    for (char o : ok) bad += !o;
    if (!all_bad) {
        plda_launch_centre(st, w.X.p, nullptr, w.mu.p, nullptr, w.coef.p, w.F.p, J, R);      // f_j = e_j - n_j mu
        dense_gemm(T_JFA_GEMM_B, st, w.F.p, R, 1, iSw, R, 1, w.G.p, R, J, R, R, false, 0);                                  // G = F Sw^-1
        for (int64_t c = 0; c < nc; c++) {
            const PldaClass &k = pl.classes[(size_t)c];
            if (!ok[(size_t)c]) continue;
            dense_gemm(T_JFA_GEMM_L, st, w.G.p + k.start * R, R, 1, w.phi.p + c * rr, R, 1, w.Y.p + k.start * R, R, k.size, R, R, false, 0);      // Yhat_c = G_c Phi_c
            dense_gemm(T_JFA_GEMM_L, st, w.Y.p + k.start * R, R, 1, w.pc.p + c * rr, R, 1, w.M.p + k.start * R, R, k.size, R, R, false, 0);      // M = Yhat_c P_c
            plda_launch_rowdot(st, w.M.p + k.start * R, w.Y.p + k.start * R, w.q.p + k.start, k.size, R);
        }
    }
    for (int64_t ci = 0; ci < pl.n_chunks; ci++) {
        const int64_t t0 = ci * chunk, nt = std::min(chunk, T - t0);
        if (!all_bad) {
            w.Z.upload(X + t0 * R, (size_t)(nt * R));
            plda_launch_centre(st, w.Z.p, nullptr, w.mu.p, nullptr, nullptr, w.Xc.p, nt, R);
            dense_gemm(T_JFA_GEMM_B, st, w.Xc.p, R, 1, w.pc.p + nc * rr, R, 1, w.Z.p, R, nt, R, R, false, 0);              // Z = X P_0
            plda_launch_rowdot(st, w.Z.p, w.Xc.p, w.a0.p, nt, R);
        }
        for (int64_t c = 0; c < nc; c++) {
            const PldaClass &k = pl.classes[(size_t)c];
            if (ok[(size_t)c]) {
                dense_gemm(T_JFA_GEMM_B, st, w.Xc.p, R, 1, w.pc.p + c * rr, R, 1, w.Z.p, R, nt, R, R, false, 0);           // Z = X P_c
                plda_launch_rowdot(st, w.Z.p, w.Xc.p, w.a.p, nt, R);
                dense_gemm(T_JFA_GEMM_C, st, w.M.p + k.start * R, R, 1, w.Xc.p, 1, R, w.out.p + k.start * T + t0, T, k.size, nt, R, false, 0);      // M X^T
            }
            launch_assemble(st, 0, w.out.p, T, k.start, t0, k.size, nt, w.q.p, w.a.p, w.a0.p, ok[(size_t)c] ? logdet[(size_t)c] : 0.0, ld_0,
                            ok[(size_t)c] != 0);
        }
        sync_stream();                         // (the next chunk's upload reuses Z)
    }
    if (identity) {
        w.out.download(out, (size_t)(J * T));
        sync_stream();
    } else if (T >= PLDA_ROW_COPY_MIN) {       // every sorted row straight to its model's place
        for (int64_t s = 0; s < J; s++)
            SR_HIP(hipMemcpyAsync(out + pl.perm[(size_t)s] * T, w.out.p + s * T, (size_t)T * 8, hipMemcpyDeviceToHost, st));
        sync_stream();
    } else {                                   // short rows: one copy, the rows put in place on the host
        std::vector<double> sorted((size_t)(J * T));
        w.out.download(sorted.data(), (size_t)(J * T));
        sync_stream();
        for (int64_t s = 0; s < J; s++) std::memcpy(out + pl.perm[(size_t)s] * T, &sorted[(size_t)(s * T)], (size_t)T * 8);
    }
    if (bad_classes) *bad_classes = bad;
}

void backend_fit(int kind, int64_t n, int R, const double *X, const int64_t *ids, int64_t S, double *mu_out, double *A) {
    std::string why;
    if (kind != PLDA_WHITEN && kind != PLDA_WCCN) fail("PLDA back end: the kind is 0 (whiten) or 1 (wccn)");
    plda_check_matrix(X, n, R, "X, the training vectors [n][R]", "n, the number of training vectors");
    if (!mu_out || !A) fail("PLDA back end: null argument (mu [R] and A [R][R], the results)");
    // whitening has one class: everything
    std::vector<int64_t> zeros;
    if (kind == PLDA_WHITEN) {
        zeros.assign((size_t)n, 0);
        ids = zeros.data();
        S = 1;
    }
    PldaPlan pl;
    if (!plan_plda_train(n, R, ids, S, (int)jfa_lds_rows(), 1, pl, why)) fail("%s", why.c_str());
    plda_check_device("sr_backend_fit");
    if (!plan_plda_train(n, R, ids, S, (int)jfa_lds_rows(), std::max(1, ctx().n_cu), pl, why)) fail("%s", why.c_str());
    hipStream_t st = ctx().stream;
    auto &w = per_device<PldaScratch>();
    const int64_t rr = (int64_t)R * R;
    const std::vector<double> mu = centre_and_sum(st, w, pl, X, kind == PLDA_WCCN);
    const double *rows = w.Xc.p;
    std::vector<int64_t> midx;
    std::vector<double> coef;
    if (kind == PLDA_WCCN) {                   // the class means are subtracted first
        midx.resize((size_t)n), coef.resize((size_t)n);
        for (int64_t s = 0; s < S; s++)
            for (int64_t r = pl.row_start[(size_t)s]; r < pl.row_start[(size_t)s + 1]; r++)
                midx[(size_t)r] = s, coef[(size_t)r] = 1.0 / (double)(pl.row_start[(size_t)s + 1] - pl.row_start[(size_t)s]);
        w.midx.upload(midx.data(), (size_t)n);
        w.coef.upload(coef.data(), (size_t)n);
        w.Xw.ensure((size_t)(n * R));
        plda_launch_centre(st, w.Xc.p, nullptr, w.F.p, w.midx.p, w.coef.p, w.Xw.p, n, R);
        rows = w.Xw.p;
    }
    w.T2.ensure((size_t)rr), w.work.ensure((size_t)rr);
    plda_accumulate_gram(st, rows, rows, w.T2.p, n, pl.sum_chunk, R);
    const double inv_n = 1.0 / (double)n;
    w.cls_size.upload(&inv_n, 1);
    plda_launch_combine(st, nullptr, 0, w.T2.p, w.cls_size.p, w.work.p, 1, R);               // the covariance
    std::vector<int> flags;
    std::vector<double> logdet;
    if (plda_invert_blocks(st, pl, w.work.p, 1, 1, flags, logdet))
        fail("PLDA back end: the %s covariance of these %lld vectors of %d dimensions does not factor (dependent columns, or too few vectors); "
             "pass more vectors or reduce the dimension", kind == PLDA_WCCN ? "within-class" : "total", (long long)n, R);
    w.work.download(A, (size_t)rr);
    sync_stream();
    std::memcpy(mu_out, mu.data(), (size_t)R * 8);
}

void backend_apply(int64_t n, int R, const double *X, const double *mu, const double *A, int length_norm, double *Y, int64_t *zero_rows) {
    std::string why;
    plda_check_matrix(X, n, R, "X, the vectors [n][R]", "n, the number of vectors");
    if (!mu || !A || !Y) fail("PLDA back end: null argument (mu [R], A [R][R] and Y [n][R] are all required)");
    if (!plda_check_finite(mu, R, "mu", why) || !plda_check_finite(A, (int64_t)R * R, "A", why)) fail("%s", why.c_str());
    plda_check_device("sr_backend_apply");
    hipStream_t st = ctx().stream;
    auto &w = per_device<PldaScratch>();
    w.X.upload(X, (size_t)(n * R));
    w.mu.upload(mu, (size_t)R);
    w.work.upload(A, (size_t)R * R);
    w.Xc.ensure((size_t)(n * R)), w.Y.ensure((size_t)(n * R));
    plda_launch_centre(st, w.X.p, nullptr, w.mu.p, nullptr, nullptr, w.Xc.p, n, R);
    dense_gemm(T_JFA_GEMM_B, st, w.Xc.p, R, 1, w.work.p, 1, R, w.Y.p, R, n, R, R, false, 0);      // (X - mu) A^T
    int64_t zeros = 0;
    if (length_norm) {
        w.flags.ensure((size_t)n);
        plda_launch_rownorm(st, w.Y.p, n, R, w.flags.p);
        std::vector<int> flags((size_t)n);
        w.flags.download(flags.data(), (size_t)n);
        sync_stream();
        for (int f : flags) zeros += f != 0;
    }
    w.Y.download(Y, (size_t)(n * R));
    sync_stream();
    if (zero_rows) *zero_rows = zeros;
}

void cosine_score(int64_t J, int64_t T, int R, const double *E, const double *X, double *out) {
    plda_check_matrix(E, J, R, "E, the models' vectors [J][R]", "J, the number of models");
    plda_check_matrix(X, T, R, "X, the test vectors [T][R]", "T, the number of test segments");
    if (!out) fail("cosine scoring: null argument (out, the score matrix [J][T])");
    if (J > (((int64_t)1 << 36) / T)) fail("cosine scoring: a score matrix of more than 2^36 values; split the trial list");
    plda_check_device("sr_cosine_score");
    hipStream_t st = ctx().stream;
    auto &w = per_device<PldaScratch>();
    w.X.upload(E, (size_t)(J * R));
    w.Xc.upload(X, (size_t)(T * R));
    w.q.ensure((size_t)J), w.a.ensure((size_t)T), w.out.ensure((size_t)(J * T));
    plda_launch_rowdot(st, w.X.p, w.X.p, w.q.p, J, R);
    plda_launch_rowdot(st, w.Xc.p, w.Xc.p, w.a.p, T, R);
    dense_gemm(T_JFA_GEMM_C, st, w.X.p, R, 1, w.Xc.p, 1, R, w.out.p, T, J, T, R, false, 0);       // E X^T
    launch_assemble(st, 1, w.out.p, T, 0, 0, J, T, w.q.p, w.a.p, nullptr, 0.0, 0.0, true);
    w.out.download(out, (size_t)(J * T));
    sync_stream();
}

}  // namespace sr
