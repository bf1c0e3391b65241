// eig.hip -- the float64 symmetric eigen-solver on the device: two-sided block Jacobi.  A [R][R] symmetric (not assumed definite),
// 1 <= R <= 512  ->  w [R] descending, V [R][R] with column k the unit eigenvector of w[k], its component of largest magnitude
// positive (the lowest index winning a tie), the sweeps taken and a `converged` flag.
// The R columns are cut into blocks of EIG_B = 32 (the last may be narrower), an odd number of blocks padded with an empty phantom
// block; a sweep is the blocks - 1 rounds of the round-robin tournament (eig_plan.cpp holds it as a table), a round has blocks / 2
// disjoint pairs and three stages, each one launch:
//   eig_pair_solve_kernel  a workgroup per pair: the pair's 2b x 2b sub-problem A[idx, idx] in LDS, up to EIG_INNER_SWEEPS sweeps of
//                          cyclic Jacobi rotations in the parallel (round-robin) ordering (fewer once nothing is left to rotate;
//                          the sub-problem need not be solved to the end for the outer iteration to converge as fast: eig_plan.hpp),
//                          the inner angle |theta| <= pi / 4, Q accumulated from the
//                          identity -- so Q is the eigenvector matrix nearest the identity by construction, which is what makes the
//                          outer iteration converge (an inner solver that sorts does not).  A rotation whose |a_pq| is at or below
//                          eps max|A_input| is skipped: a sub-problem that is diagonal already costs one look.  The solved block
//                          goes back into A (mirrored), Q into the pair's slot.
//   eig_update_kernel      columns: A[:, idx] <- A[:, idx] Q (the rows outside idx) and V[:, idx] <- V[:, idx] Q; a workgroup per
//                          (pair, tile of 64 rows, matrix): Q and the tile in LDS, plain float64 FMAs, k = 0 .. 2b - 1 in order.
//   eig_update_kernel      rows: A[idx, :] <- Q^T A[idx, :] (the columns outside idx): the same kernel, the strides exchanged.
// For R <= 2b the first stage alone is the solver (eig_single_kernel: one launch, the sweeps counted inside).  After every sweep the
// largest off-diagonal magnitude is reduced on the device (a wave per row, then one workgroup) and read back; the iteration stops
// at  off <= R 2^-52 max|A_input|  or at the cap of EIG_MAX_SWEEPS = 40 (converged = 0, what there is comes back).  The sort is
// made once at the end (eig_rank_kernel: a rank by counting, ties by index; eig_gather_kernel: the columns permuted and signed).
// No grid-wide barrier, no cooperative launch, no atomics; every sum has a fixed order and max is exact, so the same bits from run
// to run.  All of it is booked to T_JFA_FACTOR.
#include "eig_dev.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace sr {

static_assert(EIG_WG == 256 && EIG_N == 64, "the kernels are written for 256 lanes and sub-problems of up to 64");
constexpr double EIG_EPS = 2.220446049250313e-16;      // 2^-52

// The maximum over the workgroup; every lane gets it.  red [EIG_WG].
static __device__ double eig_wg_max(double v, double *red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int off = EIG_WG / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] = fmax(red[tid], red[tid + off]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

static __device__ double eig_off_max_lds(const double *S, int n, double *red) {
    double m = 0.0;
    for (int e = threadIdx.x; e < n * n; e += EIG_WG) {
        const int i = e / n, j = e % n;
        if (i != j) m = fmax(m, fabs(S[i * EIG_LD + j]));
    }
    return eig_wg_max(m, red);
}

// Cyclic Jacobi on S [n][EIG_LD] in LDS (symmetric, n <= EIG_N), Q [n][EIG_LD] accumulating the rotations: sweeps of n - 1 steps (n
// made even by a dummy index), a step's n / 2 disjoint rotations computed by n / 2 lanes and applied by all: the columns of S, then
// the rows of S and the columns of Q.  Until the largest off-diagonal magnitude is <= stop, or `cap` sweeps.  -> the sweeps taken.
static __device__ int eig_jacobi_lds(double *S, double *Q, double *rot /*[EIG_B][4]*/, int *pq /*[EIG_B][2]*/, double *red, int n, double skip,
                                     double stop, int cap, int *converged) {
    const int tid = threadIdx.x;
    const int ne = n + (n & 1), half = ne / 2, m = ne - 1;
    int sweeps = 0;
    double off = eig_off_max_lds(S, n, red);
    while (off > stop && sweeps < cap) {
        for (int r = 0; r < m; r++) {
            if (tid < half) {
                int p = tid == 0 ? r : (r + tid) % m, q = tid == 0 ? m : (r + m - tid) % m;
                if (p > q) {
                    const int t = p;
                    p = q, q = t;
                }
                double c = 1.0, s = 0.0, dpp = 0.0, dqq = 0.0;
                if (q < n) {
                    const double apq = S[p * EIG_LD + q];
                    if (fabs(apq) > skip) {
                        const double app = S[p * EIG_LD + p], aqq = S[q * EIG_LD + q];
                        const double theta = (aqq - app) / (2.0 * apq);
                        const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(__builtin_fma(theta, theta, 1.0)));
                        c = 1.0 / sqrt(__builtin_fma(t, t, 1.0));
                        s = t * c;
                        dpp = app - t * apq;
                        dqq = aqq + t * apq;
                    }
                }
                rot[tid * 4] = c, rot[tid * 4 + 1] = s, rot[tid * 4 + 2] = dpp, rot[tid * 4 + 3] = dqq;
                pq[tid * 2] = p, pq[tid * 2 + 1] = q;
            }
            __syncthreads();
            for (int e = tid; e < half * n; e += EIG_WG) {             // S <- S J: the columns p, q of every row
                const int k = e / n, i = e % n;
                const double c = rot[k * 4], s = rot[k * 4 + 1];
                if (s == 0.0) continue;
                const int p = pq[k * 2], q = pq[k * 2 + 1];
                const double x = S[i * EIG_LD + p], y = S[i * EIG_LD + q];
                S[i * EIG_LD + p] = c * x - s * y;
                S[i * EIG_LD + q] = s * x + c * y;
            }
            __syncthreads();
            for (int e = tid; e < half * n; e += EIG_WG) {             // S <- J^T S: the rows p, q; Q <- Q J
                const int k = e / n, j = e % n;
                const double c = rot[k * 4], s = rot[k * 4 + 1];
                if (s == 0.0) continue;
                const int p = pq[k * 2], q = pq[k * 2 + 1];
                const double x = S[p * EIG_LD + j], y = S[q * EIG_LD + j];
                double np = c * x - s * y, nq = s * x + c * y;
                if (j == p) np = rot[k * 4 + 2], nq = 0.0;             // (the 2 x 2 itself by its formulas: the zero is exact)
                if (j == q) np = 0.0, nq = rot[k * 4 + 3];
                S[p * EIG_LD + j] = np;
                S[q * EIG_LD + j] = nq;
                const double u = Q[j * EIG_LD + p], v = Q[j * EIG_LD + q];
                Q[j * EIG_LD + p] = c * u - s * v;
                Q[j * EIG_LD + q] = s * u + c * v;
            }
            __syncthreads();
        }
        sweeps++;
        off = eig_off_max_lds(S, n, red);
    }
    *converged = off <= stop ? 1 : 0;
    return sweeps;
}

struct EigLds {
    double *S, *Q, *rot, *red;
    int *pq;
};
static __device__ EigLds eig_carve(double *lds) {
    EigLds l;
    l.S = lds;
    l.Q = l.S + EIG_N * EIG_LD;
    l.rot = l.Q + EIG_N * EIG_LD;
    l.red = l.rot + 4 * EIG_B;
    l.pq = reinterpret_cast<int *>(l.red + EIG_WG);
    return l;
}

// The global column of the pair's local index k: block p's n1 columns, then block q's.
static __device__ inline int eig_col(int k, int p, int q, int n1) { return k < n1 ? p * EIG_B + k : q * EIG_B + (k - n1); }

// R <= EIG_N: the whole solver.  A: the lower triangle is read.  wraw [R] the diagonal reached, V [R][R] the rotations; info: sweeps, converged.
__global__ __launch_bounds__(EIG_WG)
void eig_single_kernel(const double *__restrict__ A, int R, double *__restrict__ wraw, double *__restrict__ V, int *__restrict__ info) {
    extern __shared__ double eig_lds[];
    const EigLds l = eig_carve(eig_lds);
    const int tid = threadIdx.x;
    double top = 0.0;
    for (int e = tid; e < R * R; e += EIG_WG) {
        const int i = e / R, j = e % R;
        const double a = i >= j ? A[i * R + j] : A[j * R + i];
        l.S[i * EIG_LD + j] = a;
        l.Q[i * EIG_LD + j] = i == j ? 1.0 : 0.0;
        top = fmax(top, fabs(a));
    }
    top = eig_wg_max(top, l.red);
    int converged = 0;
    const int sweeps = eig_jacobi_lds(l.S, l.Q, l.rot, l.pq, l.red, R, EIG_EPS * top, (double)R * EIG_EPS * top, EIG_MAX_SWEEPS, &converged);
    for (int e = tid; e < R * R; e += EIG_WG) V[e] = l.Q[(e / R) * EIG_LD + e % R];
    for (int i = tid; i < R; i += EIG_WG) wraw[i] = l.S[i * EIG_LD + i];
    if (tid == 0) info[0] = sweeps, info[1] = converged;
}

// A workgroup per working pair of the round (pairs [grid][2]).  Qg [grid][EIG_N][EIG_N].
__global__ __launch_bounds__(EIG_WG)
void eig_pair_solve_kernel(double *__restrict__ A, int R, const int *__restrict__ pairs, double *__restrict__ Qg, double skip) {
    extern __shared__ double eig_lds[];
    const EigLds l = eig_carve(eig_lds);
    const int tid = threadIdx.x;
    const int p = pairs[2 * blockIdx.x], q = pairs[2 * blockIdx.x + 1];
    const int n1 = min(EIG_B, R - p * EIG_B), n = n1 + min(EIG_B, R - q * EIG_B);
    for (int e = tid; e < n * n; e += EIG_WG) {
        const int i = e / n, j = e % n;
        const int gi = eig_col(max(i, j), p, q, n1), gj = eig_col(min(i, j), p, q, n1);
        l.S[i * EIG_LD + j] = A[(int64_t)gi * R + gj];
        l.Q[i * EIG_LD + j] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    int converged = 0;
    eig_jacobi_lds(l.S, l.Q, l.rot, l.pq, l.red, n, skip, skip, EIG_INNER_SWEEPS, &converged);
    double *Qp = Qg + (int64_t)blockIdx.x * EIG_N * EIG_N;
    for (int e = tid; e < n * n; e += EIG_WG) {
        const int i = e / n, j = e % n;
        A[(int64_t)eig_col(i, p, q, n1) * R + eig_col(j, p, q, n1)] = l.S[max(i, j) * EIG_LD + min(i, j)];
        Qp[i * EIG_N + j] = l.Q[i * EIG_LD + j];
    }
}

// Element (i, k) of the pair's slab is X[i * si + col(k) * sk], i < R: out (i, m) = sum_k X (i, k) Q[k][m], in place, the i inside the
// pair's own blocks left alone when skip_own (A's diagonal block is the solver's).  transposed 0: si = R, sk = 1 (columns; blockIdx.z
// 0: A, 1: V, every row); 1: si = 1, sk = R (rows of A).  grid (working pairs, tiles of EIG_TILE_ROWS, matrices).
__global__ __launch_bounds__(EIG_WG)
void eig_update_kernel(double *__restrict__ A, double *__restrict__ V, int R, const int *__restrict__ pairs, const double *__restrict__ Qg,
                       int transposed) {
    extern __shared__ double eig_lds[];
    double *Qs = eig_lds, *Xs = eig_lds + EIG_N * EIG_LD;              // [n][EIG_LD], [rows][EIG_LD]
    const int tid = threadIdx.x;
    const int p = pairs[2 * blockIdx.x], q = pairs[2 * blockIdx.x + 1];
    const int n1 = min(EIG_B, R - p * EIG_B), n = n1 + min(EIG_B, R - q * EIG_B);
    const bool own = blockIdx.z == 0;
    double *X = own ? A : V;
    const int64_t si = transposed ? 1 : R, sk = transposed ? R : 1;
    const int i0 = blockIdx.y * EIG_TILE_ROWS, rows = min(EIG_TILE_ROWS, R - i0);
    const double *Qp = Qg + (int64_t)blockIdx.x * EIG_N * EIG_N;
    for (int e = tid; e < n * n; e += EIG_WG) Qs[(e / n) * EIG_LD + e % n] = Qp[(e / n) * EIG_N + e % n];
    for (int e = tid; e < rows * n; e += EIG_WG) {
        const int r = transposed ? e % rows : e / n, k = transposed ? e / rows : e % n;
        Xs[r * EIG_LD + k] = X[(int64_t)(i0 + r) * si + (int64_t)eig_col(k, p, q, n1) * sk];
    }
    __syncthreads();
    for (int e = tid; e < rows * n; e += EIG_WG) {
        const int r = transposed ? e % rows : e / n, mcol = transposed ? e / rows : e % n;
        const int blk = (i0 + r) / EIG_B;
        if (own && (blk == p || blk == q)) continue;
        double acc = 0.0;
        for (int k = 0; k < n; k++) acc = __builtin_fma(Xs[r * EIG_LD + k], Qs[k * EIG_LD + mcol], acc);
        X[(int64_t)(i0 + r) * si + (int64_t)eig_col(mcol, p, q, n1) * sk] = acc;
    }
}

// rowmax[i] = max_j |A[i][j]|, j != i unless with_diag: a wave per row.
__global__ __launch_bounds__(EIG_WG)
void eig_rowmax_kernel(const double *__restrict__ A, int R, int with_diag, double *__restrict__ rowmax) {
    const int row = blockIdx.x * (EIG_WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= R) return;
    double m = 0.0;
    for (int j = lane; j < R; j += 64)
        if (with_diag || j != row) m = fmax(m, fabs(A[(int64_t)row * R + j]));
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off));
    if (lane == 0) rowmax[row] = m;
}

// out[0] = max of v [n]: one workgroup.
__global__ __launch_bounds__(EIG_WG)
void eig_max_kernel(const double *__restrict__ v, int n, double *__restrict__ out) {
    __shared__ double red[EIG_WG];
    double m = 0.0;
    for (int i = threadIdx.x; i < n; i += EIG_WG) m = fmax(m, v[i]);
    m = eig_wg_max(m, red);
    if (threadIdx.x == 0) out[0] = m;
}

// V = I; with A: wraw is not touched (it is read off A's diagonal at the end).
__global__ __launch_bounds__(EIG_WG)
void eig_identity_kernel(double *__restrict__ V, int R) {
    const int e = blockIdx.x * EIG_WG + threadIdx.x;
    if (e < R * R) V[e] = e / R == e % R ? 1.0 : 0.0;
}

// The sort, once: rank by counting (descending, equal values by index, a NaN last), perm[rank] = the column, w[rank] its value.  d: the values at
// stride ld (A's diagonal: ld = R + 1; wraw: ld = 1).  One workgroup.
__global__ __launch_bounds__(EIG_WG)
void eig_rank_kernel(const double *__restrict__ d, int64_t ld, int R, double *__restrict__ w, int *__restrict__ perm) {
    __shared__ double vals[PLDA_MAX_R];
    for (int i = threadIdx.x; i < R; i += EIG_WG) vals[i] = d[i * ld];
    __syncthreads();
    for (int j = threadIdx.x; j < R; j += EIG_WG) {
        const double v = vals[j];
        int rank = 0;
        const bool vn = v != v;
        for (int i = 0; i < R; i++) {                                  // (a NaN sorts last, NaNs among themselves by index: the ranks are a permutation whatever the values)
            const double u = vals[i];
            const bool un = u != u;
            const bool before = vn ? !un : (!un && u > v);
            const bool same = vn ? un : (!un && u == v);
            rank += (before || (same && i < j)) ? 1 : 0;
        }
        perm[rank] = j;
        w[rank] = v;
    }
}

// out[:, k] = +- Vw[:, perm[k]], the sign making the component of largest magnitude positive, the lowest index winning a tie.
// A workgroup per column k.
__global__ __launch_bounds__(EIG_WG)
void eig_gather_kernel(const double *__restrict__ Vw, const int *__restrict__ perm, int R, double *__restrict__ out) {
    __shared__ double mag[EIG_WG];
    __shared__ int idx[EIG_WG];
    const int k = blockIdx.x, src = perm[k], tid = threadIdx.x;
    double best = -1.0;
    int at = 0;
    for (int i = tid; i < R; i += EIG_WG) {                            // (ascending i: a later equal magnitude does not replace)
        const double a = fabs(Vw[(int64_t)i * R + src]);
        if (a > best) best = a, at = i;
    }
    mag[tid] = best, idx[tid] = at;
    __syncthreads();
    for (int off = EIG_WG / 2; off > 0; off >>= 1) {
        if (tid < off && (mag[tid + off] > mag[tid] || (mag[tid + off] == mag[tid] && idx[tid + off] < idx[tid])))
            mag[tid] = mag[tid + off], idx[tid] = idx[tid + off];
        __syncthreads();
    }
    const double sign = Vw[(int64_t)idx[0] * R + src] < 0.0 ? -1.0 : 1.0;
    for (int i = tid; i < R; i += EIG_WG) out[(int64_t)i * R + k] = sign * Vw[(int64_t)i * R + src];
}

// ---- host ----

namespace {
struct EigScratch {
    DevBuf<double> A, V, Vw, w, Q, rowmax, top, wraw;
    DevBuf<int> sched, info, perm;
};
}  // namespace

static void eig_lds_attr(const void *fn, int bytes, int *done) {
    if (done[ctx().device] < bytes) {
        SR_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        done[ctx().device] = bytes;
    }
}

// The largest |A[i][j]| (off the diagonal unless with_diag), reduced on the device; synchronises.
static double eig_matrix_max(hipStream_t st, EigScratch &s, const double *A, int R, bool with_diag) {
    s.rowmax.ensure((size_t)R), s.top.ensure(1);
    {
        ScopedKernelTimer tm(T_JFA_FACTOR);
        hipLaunchKernelGGL(eig_rowmax_kernel, dim3((unsigned)((R + 3) / 4)), dim3(EIG_WG), 0, st, A, R, with_diag ? 1 : 0, s.rowmax.p);
        SR_HIP(hipGetLastError());
        hipLaunchKernelGGL(eig_max_kernel, dim3(1), dim3(EIG_WG), 0, st, s.rowmax.p, R, s.top.p);
        SR_HIP(hipGetLastError());
    }
    double v = 0.0;
    s.top.download(&v, 1);
    sync_stream();
    return v;
}

void sym_eig_device(hipStream_t st, const EigPlan &pl, double *A, double *w, double *V, int *sweeps, int *converged) {
    static int solve_attr[MAX_DEVICES] = {}, single_attr[MAX_DEVICES] = {}, update_attr[MAX_DEVICES] = {};
    auto &s = per_device<EigScratch>();
    const int R = pl.R;
    const int64_t rr = (int64_t)R * R;
    s.Vw.ensure((size_t)rr), s.perm.ensure((size_t)R), s.info.ensure(2);
    int taken = 0, ok = 0;
    const double *diag = A;
    int64_t diag_ld = (int64_t)R + 1;
    if (pl.single) {
        eig_lds_attr(reinterpret_cast<const void *>(&eig_single_kernel), pl.solve_lds, single_attr);
        s.wraw.ensure((size_t)R);
        {
            ScopedKernelTimer tm(T_JFA_FACTOR);
            hipLaunchKernelGGL(eig_single_kernel, dim3(1), dim3(EIG_WG), (size_t)pl.solve_lds, st, A, R, s.wraw.p, s.Vw.p, s.info.p);
            SR_HIP(hipGetLastError());
        }
        int info[2] = {0, 0};
        s.info.download(info, 2);
        sync_stream();
        taken = info[0], ok = info[1];
        diag = s.wraw.p, diag_ld = 1;
    } else {
        eig_lds_attr(reinterpret_cast<const void *>(&eig_pair_solve_kernel), pl.solve_lds, solve_attr);
        eig_lds_attr(reinterpret_cast<const void *>(&eig_update_kernel), pl.update_lds, update_attr);
        // the working pairs of every round: the phantom's pair is not launched
        const int working = (int)pl.solve_grid;
        std::vector<int> table;
        table.reserve((size_t)pl.rounds * working * 2);
        for (int r = 0; r < pl.rounds; r++)
            for (int k = 0; k < pl.pairs; k++) {
                const EigPair &e = pl.schedule[(size_t)r * pl.pairs + k];
                if (e.q >= pl.blocks) continue;
                table.push_back(e.p), table.push_back(e.q);
            }
        if ((int64_t)table.size() != (int64_t)pl.rounds * working * 2) fail("eigen-solver: the schedule does not hold %d working pairs a round", working);
        s.sched.upload(table.data(), table.size());
        s.Q.ensure((size_t)working * EIG_N * EIG_N);
        const double top = eig_matrix_max(st, s, A, R, true);
        const double skip = EIG_EPS * top, stop = (double)R * EIG_EPS * top;
        {
            ScopedKernelTimer tm(T_JFA_FACTOR);
            hipLaunchKernelGGL(eig_identity_kernel, dim3((unsigned)((rr + EIG_WG - 1) / EIG_WG)), dim3(EIG_WG), 0, st, s.Vw.p, R);
            SR_HIP(hipGetLastError());
        }
        double off = eig_matrix_max(st, s, A, R, false);
        while (off > stop && taken < pl.max_sweeps) {
            for (int r = 0; r < pl.rounds; r++) {
                ScopedKernelTimer tm(T_JFA_FACTOR);
                const int *pairs = s.sched.p + (int64_t)r * working * 2;
                hipLaunchKernelGGL(eig_pair_solve_kernel, dim3((unsigned)working), dim3(EIG_WG), (size_t)pl.solve_lds, st, A, R, pairs, s.Q.p, skip);
                SR_HIP(hipGetLastError());
                hipLaunchKernelGGL(eig_update_kernel, dim3((unsigned)pl.cols_x, (unsigned)pl.cols_y, (unsigned)pl.cols_z), dim3(EIG_WG),
                                   (size_t)pl.update_lds, st, A, s.Vw.p, R, pairs, s.Q.p, 0);
                SR_HIP(hipGetLastError());
                hipLaunchKernelGGL(eig_update_kernel, dim3((unsigned)pl.rows_x, (unsigned)pl.rows_y, 1), dim3(EIG_WG), (size_t)pl.update_lds, st, A,
                                   s.Vw.p, R, pairs, s.Q.p, 1);
                SR_HIP(hipGetLastError());
            }
            taken++;
            off = eig_matrix_max(st, s, A, R, false);
        }
        ok = off <= stop ? 1 : 0;
    }
    {
        ScopedKernelTimer tm(T_JFA_FACTOR);
        hipLaunchKernelGGL(eig_rank_kernel, dim3(1), dim3(EIG_WG), 0, st, diag, diag_ld, R, w, s.perm.p);
        SR_HIP(hipGetLastError());
        hipLaunchKernelGGL(eig_gather_kernel, dim3((unsigned)R), dim3(EIG_WG), 0, st, s.Vw.p, s.perm.p, R, V);
        SR_HIP(hipGetLastError());
    }
    sync_stream();
    if (sweeps) *sweeps = taken;
    if (converged) *converged = ok;
}

void sym_eig(int R, const double *A, double *w, double *V, int *sweeps, int *converged) {
    std::string why;
    if (!eig_check_matrix(A, R, "A", why)) fail("%s", why.c_str());
    if (!w || !V) fail("eigen-solver: null argument (w [R] and V [R][R], the results)");
    EigPlan pl;
    if (!plan_eig(R, 1, pl, why)) fail("%s", why.c_str());
    plda_check_device("sr_sym_eig");
    if (!plan_eig(R, std::max(1, ctx().n_cu), pl, why)) fail("%s", why.c_str());
    hipStream_t st = ctx().stream;
    auto &s = per_device<EigScratch>();
    const int64_t rr = (int64_t)R * R;
    const std::vector<double> lower = plda_mirrored(A, R);        // (the device reads the lower triangle)
    s.A.upload(lower.data(), (size_t)rr);
    s.w.ensure((size_t)R), s.V.ensure((size_t)rr);
    sym_eig_device(st, pl, s.A.p, s.w.p, s.V.p, sweeps, converged);
    s.w.download(w, (size_t)R);
    s.V.download(V, (size_t)rr);
    sync_stream();
}

}  // namespace sr
