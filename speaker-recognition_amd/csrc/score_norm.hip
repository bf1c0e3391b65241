// score_norm.hip -- score normalisation on the device: a score matrix S [J][T] (models x test segments) against impostor cohorts,
// float64 throughout.  With Ez [J][Cz] the models against the Z-cohort, Tt [Ct][T] the T-cohort models against the test segments,
// Zt [Ct][Cz] the T-cohort models against the Z-cohort, mu / sigma the mean and the population standard deviation (ddof = 0):
//   z    (S - mu(Ez[j,:])) / sigma(Ez[j,:])                     t    (S - mu(Tt[:,t])) / sigma(Tt[:,t])
//   zt   S' = z-norm of S by Ez, Tt' = z-norm of Tt by Zt (row c of Tt by row c of Zt), out = t-norm of S' by Tt'
//   s    (z + t) / 2                                            as1  as s, the moments over the top-N of Ez[j,:] and of Tt[:,t]
//   as2  (Cz = Ct) I_t = the top-N of Tt[:,t], I_j = the top-N of Ez[j,:]:
//        ((S - mu(Ez[j,I_t])) / sigma(Ez[j,I_t]) + (S - mu(Tt[I_j,t])) / sigma(Tt[I_j,t])) / 2
// "top-N": the N largest values, ties to the lower index, -0.0 taken as +0.0.  The kernels:
//   norm_select_moments_kernel   one workgroup per cohort row (a column of Tt is a row read with stride T: strided loads, no transposed
//                                copy).  The row goes into LDS as order-preserving 64-bit keys; the N-th largest key is found by radix
//                                select, eight passes of one byte each over a 256-bin LDS histogram (no sort); the row is walked once
//                                more in index order, 256 elements a step, and the selected keys are compacted to the front of the row:
//                                ties at the threshold are taken by their prefix count in index order.  Indices come out ascending.
//                                The moments are summed over the compacted values: relative to the first of them (a constant set has
//                                variance 0 exactly), lane l adding the values l, l + 256, ... in that order, then a fixed tree -- the
//                                order depends on the selected set only.  With everything selected (the plain modes, top_n >= C) the
//                                select and the compaction are skipped.
//   norm_shift_kernel            as2's operands: X - (the full row's or column's mean) and its square, elementwise.
//   norm_apply_kernel            elementwise over J x T: the normalisation from per-row / per-column moments, or (as2) from the four
//                                products  Es SelT^T, (Es .* Es) SelT^T, SelE Ts, SelE (Ts .* Ts)  that the dense layer's GEMM forms
//                                (Sel*: 0/1 rows of the selection; Es = Ez - mu(Ez[j,:]), Ts = Tt - mu(Tt[:,t]): the shift keeps the
//                                cancellation in q / N - (s / N)^2 down; a pair whose products cannot tell its variance from 0 -- a
//                                selected set that is constant in a row that is not -- takes its moments from the values
//                                themselves, as the selection kernel does).  A moment pair whose variance is not > 0 or not finite is
//                                degenerate: every trial that needs it gets 0.0 exactly.  as2 counts its degenerate pairs by a
//                                reduction per workgroup into integers the host adds; the other modes count flagged rows and columns.
// Deterministic: no atomics on global memory, no float atomics anywhere (the histogram's are integer, in LDS).  A row's selection and
// moments are the same bits alone, in any batch, from run to run; an as2 score depends on its model's row of Ez and its segment's
// column of Tt only, so the chunking of the test segments under "norm_scratch_mib" does not show, bit for bit.
#include "dense64.hpp"
#include "norm_plan.hpp"
#include "score_norm.hpp"

#include <algorithm>
#include <atomic>
#include <vector>

namespace sr {

constexpr int NORM_APPLY_Z = 0, NORM_APPLY_T = 1, NORM_APPLY_ZT = 2, NORM_APPLY_S = 3, NORM_APPLY_PAIR = 4;
static_assert(NORM_WG == NORM_BINS && NORM_WG == 256, "a lane per histogram bin, four waves");

// Larger double <-> larger key; -0.0 and +0.0 share a key.
static __device__ inline unsigned long long norm_key(double x) {
    if (x == 0.0) x = 0.0;
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

static __device__ inline double norm_value(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// The sum of v over the workgroup: a fixed tree inside each wave, then ((w0 + w1) + (w2 + w3)).  Every lane returns it.
static __device__ inline double norm_block_sum(double v, double *wsum /* [4] */) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    __syncthreads();                           // the previous sum has been read by every lane
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    return (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// ---- one workgroup per row: X[row][i] at X + row * row_stride + i * elem_stride, i < C.  n_sel = min(top_n, C).
// idx [rows][n_sel] (or null): the selected indices, ascending; sel [rows][C] (or null): 1.0 where selected, else 0.0;
// mu, sigma, flags [rows]: of the selected values; sigma 0.0 and flag 1 where the variance is not > 0 or not finite. ----
__global__ __launch_bounds__(NORM_WG)
void norm_select_moments_kernel(const double *__restrict__ X, int64_t row_stride, int64_t elem_stride, int C, int n_sel, int64_t *__restrict__ idx,
                                double *__restrict__ sel, double *__restrict__ mu, double *__restrict__ sigma, int *__restrict__ flags) {
    extern __shared__ unsigned long long norm_lds[];
    unsigned long long *keys = norm_lds;                       // [C]
    unsigned int *hist = (unsigned int *)(keys + C);           // [NORM_BINS]
    unsigned int *ws = hist + NORM_BINS;                       // [0..3] / [4..7] the scans' wave totals, [8] the bin chosen, [9] what is left of k
    double *wsum = (double *)(ws + 12);                        // [4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = blockIdx.x;
    const double *x = X + row * row_stride;
    for (int i = tid; i < C; i += NORM_WG) keys[i] = norm_key(x[(int64_t)i * elem_stride]);
    __syncthreads();
    if (n_sel < C) {
        // the n_sel-th largest key, a byte a pass from the top: `thr` holds the bytes decided, k what is still to take below them
        unsigned long long thr = 0;
        unsigned int k = (unsigned int)n_sel;
        for (int pass = 0; pass < 8; pass++) {
            const int shift = 56 - 8 * pass;
            hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < C; i += NORM_WG) {
                const unsigned long long key = keys[i];
                if (pass == 0 || (key >> (shift + 8)) == (thr >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255], 1u);
            }
            __syncthreads();
            if (wave == 0) {                   // lane l owns the bins 255 - 4 l .. 252 - 4 l: the first bin from the top where the count reaches k
                const int b0 = 255 - 4 * lane;
                const unsigned int c0 = hist[b0], c1 = hist[b0 - 1], c2 = hist[b0 - 2], c3 = hist[b0 - 3];
                const unsigned int own = c0 + c1 + c2 + c3;
                unsigned int incl = own;
                for (int off = 1; off < 64; off <<= 1) {
                    const unsigned int v = __shfl_up(incl, off);
                    if (lane >= off) incl += v;
                }
                const unsigned int excl = incl - own;
                if (excl < k && k <= incl) {
                    unsigned int above = excl;
                    int bin = b0;
                    if (above + c0 < k) {
                        above += c0, bin = b0 - 1;
                        if (above + c1 < k) {
                            above += c1, bin = b0 - 2;
                            if (above + c2 < k) above += c2, bin = b0 - 3;
                        }
                    }
                    ws[8] = (unsigned int)bin;
                    ws[9] = k - above;
                }
            }
            __syncthreads();
            thr |= (unsigned long long)ws[8] << shift;
            k = ws[9];
        }
        // thr: the n_sel-th largest key; k of the keys equal to it are taken, the first in index order.  256 elements a step.
        unsigned int run_eq = 0, run_sel = 0;
        for (int base = 0; base < C; base += NORM_WG) {
            const int i = base + tid;
            const bool in = i < C;
            const unsigned long long key = in ? keys[i] : 0ull;
            const bool gt = in && key > thr, eq = in && key == thr;
            const unsigned long long below = (1ull << lane) - 1ull;
            const unsigned long long beq = __ballot(eq);
            if (lane == 0) ws[wave] = (unsigned int)__popcll(beq);
            __syncthreads();
            unsigned int eq_before = run_eq + (unsigned int)__popcll(beq & below), eq_all = 0;
            for (int w = 0; w < 4; w++) {
                const unsigned int t = ws[w];
                if (w < wave) eq_before += t;
                eq_all += t;
            }
            const bool take = gt || (eq && eq_before < k);
            const unsigned long long bs = __ballot(take);
            if (lane == 0) ws[4 + wave] = (unsigned int)__popcll(bs);
            __syncthreads();                   // (every lane holds its key: the compacted ones may land on this step's elements)
            unsigned int pos = run_sel + (unsigned int)__popcll(bs & below), sel_all = 0;
            for (int w = 0; w < 4; w++) {
                const unsigned int t = ws[4 + w];
                if (w < wave) pos += t;
                sel_all += t;
            }
            if (take && pos < (unsigned int)n_sel) {
                keys[pos] = key;
                if (idx) idx[row * n_sel + pos] = i;
            }
            if (sel && in) sel[row * C + i] = take ? 1.0 : 0.0;
            run_eq += eq_all;
            run_sel += sel_all;
        }
        __syncthreads();
    } else {
        for (int i = tid; i < C; i += NORM_WG) {
            if (idx) idx[row * n_sel + i] = i;
            if (sel) sel[row * C + i] = 1.0;
        }
    }
    // the moments of keys[0 .. n_sel), relative to the first
    const double pivot = norm_value(keys[0]);
    double s = 0.0;
    for (int m = tid; m < n_sel; m += NORM_WG) s += norm_value(keys[m]) - pivot;
    const double mean = norm_block_sum(s, wsum) / (double)n_sel;
    double q = 0.0;
    for (int m = tid; m < n_sel; m += NORM_WG) {
        const double d = (norm_value(keys[m]) - pivot) - mean;
        q = __builtin_fma(d, d, q);
    }
    const double var = norm_block_sum(q, wsum) / (double)n_sel;
    if (tid == 0) {
        const bool ok = var > 0.0 && __builtin_isfinite(var);
        mu[row] = pivot + mean;
        sigma[row] = ok ? sqrt(var) : 0.0;
        flags[row] = ok ? 0 : 1;
    }
}

// out [rows][cols] = X[r][c0 + c] - (by_row ? m[r] : m[c0 + c]), out2 = its square.  X's row stride: ld.
__global__ __launch_bounds__(NORM_WG)
void norm_shift_kernel(const double *__restrict__ X, int64_t ld, int64_t c0, int64_t rows, int64_t cols, const double *__restrict__ m, int by_row,
                       double *__restrict__ out, double *__restrict__ out2) {
    const int64_t e = (int64_t)blockIdx.x * NORM_WG + threadIdx.x;
    if (e >= rows * cols) return;
    const int64_t r = e / cols, c = e % cols;
    const double v = X[r * ld + c0 + c] - (by_row ? m[r] : m[c0 + c]);
    out[e] = v;
    out2[e] = v * v;
}

// as2's operands, for the pairs whose products cannot decide (below).  Ez [J][C], Tt [C][T], SelT [n][C] (row i = column t0 + i), SelE [J][C].
struct NormPairSrc {
    const double *Ez, *Tt, *SelT, *SelE;
    int64_t T;
    int C;
};

// The moments of the values x[c * stride] with sel[c] != 0, c < C, taken from the values themselves as the selection kernel takes
// them: relative to the first selected value, in index order.  A constant set has variance 0 exactly.
static __device__ void norm_pair_moments(const double *__restrict__ x, int64_t stride, const double *__restrict__ sel, int C, double n, double &mu,
                                         double &var) {
    double pivot = 0.0, s = 0.0, q = 0.0;
    bool first = true;
    for (int c = 0; c < C; c++)
        if (sel[c] != 0.0) {
            const double v = x[(int64_t)c * stride];
            if (first) pivot = v, first = false;
            s += v - pivot;
        }
    const double mean = s / n;
    for (int c = 0; c < C; c++)
        if (sel[c] != 0.0) {
            const double d = (x[(int64_t)c * stride] - pivot) - mean;
            q = __builtin_fma(d, d, q);
        }
    mu = pivot + mean;
    var = q / n;
}

// The products give a pair's variance as q / N - (s / N)^2 about the row's (column's) mean, with an error of at most about
// 3 (N + 2) eps q / N (N-term sums, the square).  Where that variance is not above 2^-30 q / N -- the selected values lie within
// 2^-15 of their own distance from the shift, a constant set among them, for which the products leave the rounding error of one
// multiplication, of either sign -- the products cannot decide, and the pair's moments are taken from the values themselves.
// Above it the products' variance is good to 3 (N + 2) / N 2^-22 relative.
constexpr double NORM_PAIR_RECHECK = 0x1p-30;

// ---- grid (rows, blocks of 256 columns).  S [rows][ld] and out [rows][ld], columns t0 .. t0 + n.  mr / sr [rows], mc / sc [ld]: the
// moments by row and by column (a degenerate pair has sigma 0).  PAIR: P1 .. P4 [rows][ldp] the sums and the sums of squares over the
// selections, column i of them = column t0 + i; mr / mc the shifts; src the operands; counts [rows][gridDim.y][2] the degenerate
// pairs by side. ----
__global__ __launch_bounds__(NORM_WG)
void norm_apply_kernel(int mode, const double *__restrict__ S, double *__restrict__ out, int64_t ld, int64_t t0, int64_t n,
                       const double *__restrict__ mr, const double *__restrict__ sr, const double *__restrict__ mc, const double *__restrict__ sc,
                       const double *__restrict__ P1, const double *__restrict__ P2, const double *__restrict__ P3, const double *__restrict__ P4,
                       int64_t ldp, double n_sel, NormPairSrc src, int *__restrict__ counts) {
    __shared__ unsigned int wcount[2][4];
    const int64_t j = blockIdx.x, i = (int64_t)blockIdx.y * NORM_WG + threadIdx.x, t = t0 + i;
    const bool in = i < n;
    bool bad_e = false, bad_t = false;
    if (in) {
        const double s = S[j * ld + t];
        double v = 0.0;
        if (mode == NORM_APPLY_PAIR) {
            const double qe = P2[j * ldp + i] / n_sel, qt = P4[j * ldp + i] / n_sel;
            double me = P1[j * ldp + i] / n_sel, mt = P3[j * ldp + i] / n_sel;
            double ve = __builtin_fma(-me, me, qe), vt = __builtin_fma(-mt, mt, qt);
            me += mr[j];
            mt += mc[t];
            if (!(ve > NORM_PAIR_RECHECK * qe)) norm_pair_moments(src.Ez + j * src.C, 1, src.SelT + i * src.C, src.C, n_sel, me, ve);
            if (!(vt > NORM_PAIR_RECHECK * qt)) norm_pair_moments(src.Tt + t, src.T, src.SelE + j * src.C, src.C, n_sel, mt, vt);
            bad_e = !(ve > 0.0) || !__builtin_isfinite(ve);
            bad_t = !(vt > 0.0) || !__builtin_isfinite(vt);
            if (!bad_e && !bad_t) v = 0.5 * ((s - me) / sqrt(ve) + (s - mt) / sqrt(vt));
        } else {
            const bool rows = mode != NORM_APPLY_T, cols = mode != NORM_APPLY_Z;
            const double se = rows ? sr[j] : 1.0, st = cols ? sc[t] : 1.0;
            bad_e = rows && !(se > 0.0);
            bad_t = cols && !(st > 0.0);
            if (!bad_e && !bad_t) {
                if (mode == NORM_APPLY_Z) v = (s - mr[j]) / se;
                else if (mode == NORM_APPLY_T) v = (s - mc[t]) / st;
                else if (mode == NORM_APPLY_ZT) v = ((s - mr[j]) / se - mc[t]) / st;
                else v = 0.5 * ((s - mr[j]) / se + (s - mc[t]) / st);
            }
        }
        out[j * ld + t] = v;
    }
    if (counts) {
        const unsigned long long be = __ballot(bad_e), bt = __ballot(bad_t);
        if ((threadIdx.x & 63) == 0) {
            wcount[0][threadIdx.x >> 6] = (unsigned int)__popcll(be);
            wcount[1][threadIdx.x >> 6] = (unsigned int)__popcll(bt);
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            const unsigned int *w = wcount[threadIdx.x];
            counts[(j * gridDim.y + blockIdx.y) * 2 + threadIdx.x] = (int)(w[0] + w[1] + w[2] + w[3]);
        }
    }
}

// ---- host ----

static std::atomic<long> &norm_scratch_option() {
    static std::atomic<long> v{(long)(NORM_DEFAULT_SCRATCH >> 20)};
    return v;
}
void set_norm_scratch_mib(long v) { norm_scratch_option().store(v); }
long norm_scratch_mib() { return norm_scratch_option().load(); }

namespace {
struct NormScratch {
    DevBuf<double> S, Ez, Tt, Zt, out, tn;
    DevBuf<double> mr, sr, mc, sc, mz, sz, mfull, sfull, mt, st;
    DevBuf<double> SelE, Es, Es2, SelT, Ts, Ts2, P1, P2, P3, P4;
    DevBuf<int> fr, fc, fz, ffull, ft, counts;
    DevBuf<double> X, mu, sigma;               // the selection stage alone
    DevBuf<int64_t> idx;
};
}  // namespace

static void launch_select(hipStream_t st, const double *X, int64_t row_stride, int64_t elem_stride, int64_t rows, int64_t C, int64_t n_sel,
                          int64_t *idx, double *sel, double *mu, double *sigma, int *flags) {
    static int attr_set[MAX_DEVICES] = {};
    const int lds = norm_select_lds_bytes(C);
    if (attr_set[ctx().device] < lds) {
        SR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&norm_select_moments_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        attr_set[ctx().device] = lds;
    }
    ScopedKernelTimer tm(T_JFA_FACTOR);
    hipLaunchKernelGGL(norm_select_moments_kernel, dim3((unsigned)rows), dim3(NORM_WG), (size_t)lds, st, X, row_stride, elem_stride, (int)C,
                       (int)n_sel, idx, sel, mu, sigma, flags);
    SR_HIP(hipGetLastError());
}

static void launch_shift(hipStream_t st, const double *X, int64_t ld, int64_t c0, int64_t rows, int64_t cols, const double *m, bool by_row,
                         double *out, double *out2) {
    ScopedKernelTimer tm(T_JFA_GRAM);
    hipLaunchKernelGGL(norm_shift_kernel, dim3((unsigned)((rows * cols + NORM_WG - 1) / NORM_WG)), dim3(NORM_WG), 0, st, X, ld, c0, rows, cols, m,
                       by_row ? 1 : 0, out, out2);
    SR_HIP(hipGetLastError());
}

static void launch_apply(hipStream_t st, int mode, const double *S, double *out, int64_t rows, int64_t ld, int64_t t0, int64_t n, const double *mr,
                         const double *sr, const double *mc, const double *sc, const double *P1, const double *P2, const double *P3,
                         const double *P4, int64_t ldp, int64_t n_sel, const NormPairSrc &src, int *counts) {
    ScopedKernelTimer tm(T_JFA_UPDATE);
    hipLaunchKernelGGL(norm_apply_kernel, dim3((unsigned)rows, (unsigned)((n + NORM_WG - 1) / NORM_WG)), dim3(NORM_WG), 0, st, mode, S, out, ld, t0,
                       n, mr, sr, mc, sc, P1, P2, P3, P4, ldp, (double)n_sel, src, counts);
    SR_HIP(hipGetLastError());
}

static int64_t count_flags(hipStream_t st, const DevBuf<int> &f, int64_t n) {
    std::vector<int> host((size_t)n);
    SR_HIP(hipMemcpyAsync(host.data(), f.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    sync_stream();
    int64_t bad = 0;
    for (int v : host) bad += v;
    return bad;
}

void score_norm(int mode, int64_t J, int64_t T, int64_t Cz, int64_t Ct, int top_n, const double *S, const double *Ez, const double *Tt,
                const double *Zt, double *out, int64_t *degenerate) {
    std::string why;
    if (!norm_check_inputs(mode, J, T, Cz, Ct, top_n, S, Ez, Tt, Zt, why)) fail("%s", why.c_str());
    if (!out) fail("sr_score_norm: null argument (out, the normalised matrix [J][T])");
    NormPlan pl;
    const int64_t bound = (int64_t)norm_scratch_mib() << 20;
    if (!plan_score_norm(mode, J, T, Cz, Ct, top_n, bound, 1, pl, why)) fail("%s", why.c_str());
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_score_norm");
    ensure_device();
    if (!plan_score_norm(mode, J, T, Cz, Ct, top_n, bound, std::max(1, ctx().n_cu), pl, why)) fail("%s", why.c_str());
    hipStream_t st = ctx().stream;
    auto &w = per_device<NormScratch>();
    const bool enrol = norm_needs_enrol(mode), test = norm_needs_test(mode);
    w.S.upload(S, (size_t)(J * T));
    w.out.ensure((size_t)(J * T));
    if (enrol) {
        w.Ez.upload(Ez, (size_t)(J * Cz));
        w.mr.ensure((size_t)J), w.sr.ensure((size_t)J), w.fr.ensure((size_t)J);
    }
    if (test) {
        w.Tt.upload(Tt, (size_t)(Ct * T));
        w.mc.ensure((size_t)T), w.sc.ensure((size_t)T), w.fc.ensure((size_t)T);
    }
    int64_t bad_e = 0, bad_t = 0;
    if (mode == NORM_AS2) {
        const int64_t C = Cz, N = pl.n_sel, chunk = pl.chunk;
        w.mfull.ensure((size_t)J), w.sfull.ensure((size_t)J), w.ffull.ensure((size_t)J);
        w.mt.ensure((size_t)chunk), w.st.ensure((size_t)chunk), w.ft.ensure((size_t)chunk);
        w.SelE.ensure((size_t)(J * C)), w.Es.ensure((size_t)(J * C)), w.Es2.ensure((size_t)(J * C));
        w.SelT.ensure((size_t)(chunk * C)), w.Ts.ensure((size_t)(chunk * C)), w.Ts2.ensure((size_t)(chunk * C));
        w.P1.ensure((size_t)(J * chunk)), w.P2.ensure((size_t)(J * chunk)), w.P3.ensure((size_t)(J * chunk)), w.P4.ensure((size_t)(J * chunk));
        const int64_t gy = (chunk + NORM_WG - 1) / NORM_WG;
        w.counts.ensure((size_t)(J * gy * 2));
        // the shifts: the full rows' and columns' means; the enrolment side's selection and shifted copies, once per call
        launch_select(st, w.Ez.p, C, 1, J, C, C, nullptr, nullptr, w.mfull.p, w.sfull.p, w.ffull.p);
        launch_select(st, w.Tt.p, 1, T, T, C, C, nullptr, nullptr, w.mc.p, w.sc.p, w.fc.p);
        launch_select(st, w.Ez.p, C, 1, J, C, N, nullptr, w.SelE.p, w.mr.p, w.sr.p, w.fr.p);
        launch_shift(st, w.Ez.p, C, 0, J, C, w.mfull.p, true, w.Es.p, w.Es2.p);
        std::vector<int> host;
        for (int64_t ci = 0; ci < pl.n_chunks; ci++) {
            const int64_t t0 = ci * chunk, n = std::min(chunk, T - t0);
            // SelT [n][C]: the selections of the columns t0 .. (their own moments, as1's, are not used)
            launch_select(st, w.Tt.p + t0, 1, T, n, C, N, nullptr, w.SelT.p, w.mt.p, w.st.p, w.ft.p);
            launch_shift(st, w.Tt.p, T, t0, C, n, w.mc.p, false, w.Ts.p, w.Ts2.p);                                       // Ts [C][n]
            dense_gemm(T_JFA_GEMM_A, st, w.Es.p, C, 1, w.SelT.p, 1, C, w.P1.p, n, J, n, C, false, 0);                 // Es SelT^T
            dense_gemm(T_JFA_GEMM_A, st, w.Es2.p, C, 1, w.SelT.p, 1, C, w.P2.p, n, J, n, C, false, 0);                // (Es .* Es) SelT^T
            dense_gemm(T_JFA_GEMM_B, st, w.SelE.p, C, 1, w.Ts.p, n, 1, w.P3.p, n, J, n, C, false, 0);                 // SelE Ts
            dense_gemm(T_JFA_GEMM_B, st, w.SelE.p, C, 1, w.Ts2.p, n, 1, w.P4.p, n, J, n, C, false, 0);                // SelE (Ts .* Ts)
            launch_apply(st, NORM_APPLY_PAIR, w.S.p, w.out.p, J, T, t0, n, w.mfull.p, nullptr, w.mc.p, nullptr, w.P1.p, w.P2.p, w.P3.p, w.P4.p, n,
                         N, NormPairSrc{w.Ez.p, w.Tt.p, w.SelT.p, w.SelE.p, T, (int)C}, w.counts.p);
            const int64_t nc = J * ((n + NORM_WG - 1) / NORM_WG) * 2;
            host.resize((size_t)nc);
            SR_HIP(hipMemcpyAsync(host.data(), w.counts.p, (size_t)nc * sizeof(int), hipMemcpyDeviceToHost, st));
            sync_stream();
            for (int64_t e = 0; e < nc; e += 2) bad_e += host[(size_t)e], bad_t += host[(size_t)e + 1];
        }
    } else {
        if (enrol) launch_select(st, w.Ez.p, Cz, 1, J, Cz, pl.n_sel, nullptr, nullptr, w.mr.p, w.sr.p, w.fr.p);
        const double *test_src = w.Tt.p;
        if (mode == NORM_ZT) {                 // Tt' = Tt z-normalised by Zt's rows
            w.Zt.upload(Zt, (size_t)(Ct * Cz));
            w.mz.ensure((size_t)Ct), w.sz.ensure((size_t)Ct), w.fz.ensure((size_t)Ct), w.tn.ensure((size_t)(Ct * T));
            launch_select(st, w.Zt.p, Cz, 1, Ct, Cz, Cz, nullptr, nullptr, w.mz.p, w.sz.p, w.fz.p);
            launch_apply(st, NORM_APPLY_Z, w.Tt.p, w.tn.p, Ct, T, 0, T, w.mz.p, w.sz.p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0,
                         NormPairSrc{}, nullptr);
            test_src = w.tn.p;
        }
        if (test) launch_select(st, test_src, 1, T, T, Ct, pl.n_sel_test, nullptr, nullptr, w.mc.p, w.sc.p, w.fc.p);
        const int apply = mode == NORM_Z ? NORM_APPLY_Z : mode == NORM_T ? NORM_APPLY_T : mode == NORM_ZT ? NORM_APPLY_ZT : NORM_APPLY_S;
        launch_apply(st, apply, w.S.p, w.out.p, J, T, 0, T, w.mr.p, w.sr.p, w.mc.p, w.sc.p, nullptr, nullptr, nullptr, nullptr, 0, 0, NormPairSrc{}, nullptr);
        if (enrol) bad_e = count_flags(st, w.fr, J);
        if (test) bad_t = count_flags(st, w.fc, T);
        if (mode == NORM_ZT) bad_t += count_flags(st, w.fz, Ct);
    }
    w.out.download(out, (size_t)(J * T));
    sync_stream();
    if (degenerate) degenerate[0] = bad_e, degenerate[1] = bad_t;
}

void score_norm_select(int64_t rows, int64_t C, int top_n, const double *X, int64_t *idx, double *mu, double *sigma) {
    std::string why;
    if (!norm_check_select(rows, C, top_n, X, why)) fail("%s", why.c_str());
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_score_norm_select");
    ensure_device();
    hipStream_t st = ctx().stream;
    auto &w = per_device<NormScratch>();
    const int64_t n_sel = std::min<int64_t>(top_n, C);
    w.X.upload(X, (size_t)(rows * C));
    w.mu.ensure((size_t)rows), w.sigma.ensure((size_t)rows), w.ffull.ensure((size_t)rows);
    if (idx) w.idx.ensure((size_t)(rows * n_sel));
    launch_select(st, w.X.p, C, 1, rows, C, n_sel, idx ? w.idx.p : nullptr, nullptr, w.mu.p, w.sigma.p, w.ffull.p);
    if (idx) w.idx.download(idx, (size_t)(rows * n_sel));
    if (mu) w.mu.download(mu, (size_t)rows);
    if (sigma) w.sigma.download(sigma, (size_t)rows);
    sync_stream();
}

}  // namespace sr
