// jfa_stats.hip -- the layer between the three kernels of the JFA leg (bw_stats.hip -> jfa.hip -> jfa_score.hip): statistics that
// stay on the device from the Baum-Welch pass to the score matrix.
//   SRStats               raw N [n][K], F [n][K D] of n sessions, float64, on one device: filled by the reduce of the Baum-Welch pass
//                         (sr_bw_stats_resident) or uploaded once (sr_stats_from_host); validated when made -- on the host before
//                         the upload, or by jfa_stats_check_kernel on the pass's result -- so that no consumer meets a NaN later.
//   sr_jfa_open_centred   the grouping and centring jfa.py does in numpy, on the device, into an ordinary factor handle
//                         (jfa_plan.hpp has the formulas): y v and a chunk of x u through the dense layer's GEMM (dense64.hpp),      
//                         then one streaming kernel.  jfa_centre_kernel: a workgroup owns 256 (or 512: two per lane, 16-byte
//                         accesses, where K D is even) columns of one group's row and walks that group's sessions of the chunk in
//                         ascending order from a host-built index; it reads F once, N once, the product once and writes Fc once.
//                         A later chunk continues from what the row holds; the shift N_g (m + z d + y v) is taken off with the
//                         group's last session.  The lane's mixture index is one division before the loop.
//   sr_jfa_zd             estimate_z_and_d.m on a handle's resident N_g, Fc_g, E: a lane owns a supervector column over all groups
//                         and all rounds (columns do not interact), sums a and b in group order; z is written when asked for.
//   jfa_segment_totals    the scorers' n_t = a segment's K counts added in mixture order, as the host-array entry adds them.
// No atomics anywhere: a group's row is the same bits alone, inside any batch, under any bound and from run to run -- row r of a
// matrix-core product depends on row r of its first operand only, and every sum has one fixed order.
#include "dense64.hpp"
#include "jfa_dev.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <mutex>
#include <set>
#include <vector>

namespace sr {

constexpr int JFA_ZD_WG = 64;                          // a column a lane, one wave a workgroup: K D / 64 workgroups over the chip
constexpr int JFA_CHECK_BLOCKS = 1024;

// ---- first offending elements of N (non-finite; negative) and F (non-finite): per workgroup, the host takes the minima ----
__global__ __launch_bounds__(JFA_WG)
void jfa_stats_check_kernel(const double *__restrict__ N, int64_t nN, const double *__restrict__ F, int64_t nF, long long *__restrict__ out) {
    __shared__ long long s[3][JFA_WG];
    const int tid = threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * JFA_WG;
    long long a = LLONG_MAX, b = LLONG_MAX, c = LLONG_MAX;
    for (int64_t i = (int64_t)blockIdx.x * JFA_WG + tid; i < nN; i += stride) {
        const double v = N[i];
        if (!__builtin_isfinite(v)) a = min(a, (long long)i);
        else if (v < 0.0) b = min(b, (long long)i);
    }
    for (int64_t i = (int64_t)blockIdx.x * JFA_WG + tid; i < nF; i += stride)
        if (!__builtin_isfinite(F[i])) c = min(c, (long long)i);
    s[0][tid] = a;
    s[1][tid] = b;
    s[2][tid] = c;
    __syncthreads();
    for (int w = JFA_WG / 2; w > 0; w >>= 1) {
        if (tid < w)
            for (int q = 0; q < 3; q++) s[q][tid] = min(s[q][tid], s[q][tid + w]);
        __syncthreads();
    }
    if (tid < 3) out[3 * blockIdx.x + tid] = s[tid][0];
}

// ---- dst[r] = src[rows[r]], rows of `width` doubles.  grid (rows, column blocks) ----
__global__ __launch_bounds__(JFA_WG)
void jfa_take_kernel(const double *__restrict__ src, const int64_t *__restrict__ rows, double *__restrict__ dst, int64_t width) {
    const int64_t r = blockIdx.x, from = rows[r];
    for (int64_t c = (int64_t)blockIdx.y * JFA_WG + threadIdx.x; c < width; c += (int64_t)gridDim.y * JFA_WG)
        dst[r * width + c] = src[from * width + c];
}

// ---- N_g = sum of a group's sessions' rows in the index's (ascending session) order.  grid (groups, blocks of K) ----
__global__ __launch_bounds__(JFA_WG)
void jfa_group_counts_kernel(const double *__restrict__ N, const int *__restrict__ order, const int *__restrict__ gstart, double *__restrict__ Ng, int K) {
    const int g = blockIdx.x, k = blockIdx.y * JFA_WG + threadIdx.x;
    if (k >= K) return;
    double acc = 0.0;
    for (int i = gstart[g]; i < gstart[g + 1]; i++) acc += N[(int64_t)order[i] * K + k];
    Ng[(int64_t)g * K + k] = acc;
}

template <int VEC>
struct JfaVec;
template <>
struct JfaVec<1> {
    double v[1];
    __device__ __forceinline__ void load(const double *p) { v[0] = *p; }
    __device__ __forceinline__ void store(double *p) const { *p = v[0]; }
};
template <>
struct JfaVec<2> {
    double v[2];
    __device__ __forceinline__ void load(const double *p) {
        const double2 t = *reinterpret_cast<const double2 *>(p);
        v[0] = t.x;
        v[1] = t.y;
    }
    __device__ __forceinline__ void store(double *p) const { *reinterpret_cast<double2 *>(p) = make_double2(v[0], v[1]); }
};

// ---- the centring stream.  grid (entries of this chunk, column blocks); a lane owns VEC adjacent columns of one group's row.
// entries {row g, first position in `order`, sessions, bit 0: the group's first chunk | bit 1: its last}: groups are speakers, the
// shift row is g.  entries == null: groups are sessions, block x is session j0 + x, its shift row lab[j].
// xu (or null): the chunk's product, row j - j0.  z, d (or null, together), yv (or null): the shift's optional terms. ----
template <int VEC>
__global__ __launch_bounds__(JFA_WG)
void jfa_centre_kernel(const double *__restrict__ F, const double *__restrict__ N, const double *__restrict__ xu, int64_t j0,
                       const int *__restrict__ order, const int4 *__restrict__ entries, const int *__restrict__ lab, const double *__restrict__ Ng,
                       const double *__restrict__ m, const double *__restrict__ z, const double *__restrict__ d, const double *__restrict__ yv,
                       double *__restrict__ Fc, int K, int D, int64_t kd) {
    const int64_t col = ((int64_t)blockIdx.y * JFA_WG + threadIdx.x) * VEC;
    if (col >= kd) return;
    int64_t g, srow;
    int begin, count, flags;
    if (entries) {
        const int4 e = entries[blockIdx.x];
        g = srow = e.x;
        begin = e.y;
        count = e.z;
        flags = e.w;
    } else {
        g = j0 + blockIdx.x;
        srow = lab[g];
        begin = (int)g;
        count = 1;
        flags = 3;
    }
    int k[VEC];
#pragma unroll
    for (int q = 0; q < VEC; q++) k[q] = (int)((col + q) / D);
    double *dst = Fc + g * kd + col;
    JfaVec<VEC> acc;
    if (flags & 1) {
#pragma unroll
        for (int q = 0; q < VEC; q++) acc.v[q] = 0.0;
    } else {
        acc.load(dst);
    }
    for (int i = 0; i < count; i++) {
        const int64_t j = order ? order[begin + i] : begin + i;
        JfaVec<VEC> f;
        f.load(F + j * kd + col);
        if (xu) {
            JfaVec<VEC> p;
            p.load(xu + (j - j0) * kd + col);
#pragma unroll
            for (int q = 0; q < VEC; q++) acc.v[q] += f.v[q] - N[j * K + k[q]] * p.v[q];
        } else {
#pragma unroll
            for (int q = 0; q < VEC; q++) acc.v[q] += f.v[q];
        }
    }
    if (flags & 2) {
        JfaVec<VEC> sh;
        sh.load(m + col);
        if (z) {
            JfaVec<VEC> zz, dd;
            zz.load(z + srow * kd + col);
            dd.load(d + col);
#pragma unroll
            for (int q = 0; q < VEC; q++) sh.v[q] += zz.v[q] * dd.v[q];
        }
        if (yv) {
            JfaVec<VEC> p;
            p.load(yv + srow * kd + col);
#pragma unroll
            for (int q = 0; q < VEC; q++) sh.v[q] += p.v[q];
        }
#pragma unroll
        for (int q = 0; q < VEC; q++) acc.v[q] -= Ng[g * K + k[q]] * sh.v[q];
    }
    acc.store(dst);
}

// ---- estimate_z_and_d.m.  A lane owns column c over every group and every round:  L = 1 + N_g d^2 / E,  z = Fc_g d / (E L),
// a = sum_g (1 / L + z^2) N_g,  b = sum_g z Fc_g,  d <- b / a  (operation order as jfa.estimate_z_and_d writes it).
// n_iter == 0: one evaluation, d untouched.  z (or null), a, b: of the last round, i.e. for the d that round started from. ----
__global__ __launch_bounds__(JFA_ZD_WG)
void jfa_zd_kernel(const double *__restrict__ Ng, const double *__restrict__ Fc, const double *__restrict__ E, double *__restrict__ d, int n_iter,
                   double *__restrict__ z, double *__restrict__ a_out, double *__restrict__ b_out, int64_t G, int K, int D, int64_t kd) {
    const int64_t c = (int64_t)blockIdx.x * JFA_ZD_WG + threadIdx.x;
    if (c >= kd) return;
    const int k = (int)(c / D);
    const double e = E[c];
    double dd = d[c], a = 0.0, b = 0.0;
    const int rounds = n_iter > 0 ? n_iter : 1;
    for (int r = 0; r < rounds; r++) {
        const bool last = r == rounds - 1;
        const double d2 = dd * dd;
        a = 0.0;
        b = 0.0;
        for (int64_t g = 0; g < G; g++) {
            const double n = Ng[g * K + k], f = Fc[g * kd + c];
            const double L = 1.0 + n / e * d2;
            const double zz = f / e * dd / L;
            a += (1.0 / L + zz * zz) * n;
            b += zz * f;
            if (last && z) z[g * kd + c] = zz;
        }
        if (n_iter > 0) dd = b / a;
    }
    if (n_iter > 0) d[c] = dd;
    a_out[c] = a;
    b_out[c] = b;
}

// ---- n_t = sum_c N[t][c] in mixture order, plain adds (what jfa_score adds on the host); segments with n_t <= 0 per workgroup ----
__global__ __launch_bounds__(JFA_WG)
void jfa_segment_totals_kernel(const double *__restrict__ N, int64_t T, int K, double *__restrict__ nt, int *__restrict__ empty) {
    __shared__ int s[JFA_WG];
    const int tid = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * JFA_WG + tid;
    int e = 0;
    if (t < T) {
        double acc = 0.0;
        for (int c = 0; c < K; c++) acc += N[t * K + c];
        nt[t] = acc;
        e = !(acc > 0.0);
    }
    s[tid] = e;
    __syncthreads();
    for (int w = JFA_WG / 2; w > 0; w >>= 1) {
        if (tid < w) s[tid] += s[tid + w];
        __syncthreads();
    }
    if (tid == 0) empty[blockIdx.x] = s[0];
}

// ---- host ----

namespace {
struct JfaStatsScratch {
    DevBuf<long long> check;
    DevBuf<int64_t> rows;
    DevBuf<int> empty;
    DevBuf<double> xu, yv, z, d, m, y, x, u, v, nt;
    DevBuf<int> order, gstart, lab;
    DevBuf<int4> entries;
};

std::mutex g_stats_mu;
std::set<const SRStats *> &live_stats() {
    static std::set<const SRStats *> s;
    return s;
}
}  // namespace

const SRStats &stats_live(const SRStats *s, const char *what) {
    if (!s) fail("%s: null statistics handle; make one with sr_bw_stats_resident or sr_stats_from_host", what);
    std::lock_guard<std::mutex> lk(g_stats_mu);
    if (!live_stats().count(s)) fail("%s: the statistics handle is closed (or was never opened); make a new one", what);
    return *s;
}

SRStats *stats_new(int64_t n, int K, int D) {
    SRStats *h = new SRStats();
    try {
        h->n = n;
        h->K = K;
        h->D = D;
        h->device = ctx().device;
        h->N.alloc((size_t)(n * K));
        h->F.alloc((size_t)(n * K) * (size_t)D);
    } catch (...) {
        delete h;
        throw;
    }
    std::lock_guard<std::mutex> lk(g_stats_mu);
    live_stats().insert(h);
    return h;
}

void stats_close(SRStats *s) {
    if (!s) return;
    {
        std::lock_guard<std::mutex> lk(g_stats_mu);
        if (!live_stats().erase(s)) return;            // closed before: harmless
    }
    delete s;
}

static void stats_on_device(const SRStats &s, const char *what) {
    if (gpu_runtime_lost()) fail_gpu_runtime_lost(what);
    if (s.device != current_device())
        fail("%s: the statistics handle lives on device %d, the calling thread is on device %d; call from a thread bound to that device", what,
             s.device, current_device());
    ensure_device();
}

void stats_check_device(const SRStats &s) {
    auto &w = per_device<JfaStatsScratch>();
    const int64_t nN = s.n * s.K, nF = nN * s.D;
    const int blocks = (int)std::min<int64_t>(JFA_CHECK_BLOCKS, (nF + JFA_WG - 1) / JFA_WG);
    w.check.ensure((size_t)3 * blocks);
    {
        ScopedKernelTimer t(T_JFA_GRAM);
        hipLaunchKernelGGL(jfa_stats_check_kernel, dim3((unsigned)blocks), dim3(JFA_WG), 0, ctx().stream, s.N.p, nN, s.F.p, nF, w.check.p);
        SR_HIP(hipGetLastError());
    }
    std::vector<long long> host((size_t)3 * blocks);
    w.check.download(host.data(), host.size());
    sync_stream();
    long long first[3] = {LLONG_MAX, LLONG_MAX, LLONG_MAX};
    for (int b = 0; b < blocks; b++)
        for (int q = 0; q < 3; q++) first[q] = std::min(first[q], host[(size_t)3 * b + q]);
    if (first[0] != LLONG_MAX) fail("%s", jfa_text_non_finite("N", first[0]).c_str());
    if (first[2] != LLONG_MAX) fail("%s", jfa_text_non_finite("F", first[2]).c_str());
    if (first[1] != LLONG_MAX) fail("%s", jfa_text_negative(first[1], s.K).c_str());
}

SRStats *stats_from_host(int64_t n, int K, int D, const double *N, const double *F) {
    std::string why;
    if (!jfa_check_raw_stats(n, K, D, N, F, why)) fail("%s", why.c_str());
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_stats_from_host");
    ensure_device();
    SRStats *h = stats_new(n, K, D);
    try {
        h->N.upload(N, (size_t)(n * K));
        h->F.upload(F, (size_t)(n * K) * (size_t)D);
        sync_stream();
    } catch (...) {
        stats_close(h);
        throw;
    }
    return h;
}

void stats_info(const SRStats *sp, int64_t *out, int n_out) {
    const SRStats &s = stats_live(sp, "sr_stats_info");
    if (!out) fail("sr_stats_info: null argument");
    if (n_out < 4) fail("sr_stats_info writes 4 fields");
    out[0] = s.n;
    out[1] = s.K;
    out[2] = s.D;
    out[3] = s.device;
}

void stats_get(const SRStats *sp, double *N, double *F) {
    const SRStats &s = stats_live(sp, "sr_stats_get");
    stats_on_device(s, "sr_stats_get");
    if (N) s.N.download(N, (size_t)(s.n * s.K));
    if (F) s.F.download(F, (size_t)(s.n * s.K) * (size_t)s.D);
    sync_stream();
}

SRStats *stats_take(const SRStats *sp, const int64_t *rows, int64_t n_rows) {
    const SRStats &s = stats_live(sp, "sr_stats_take");
    if (!rows) fail("sr_stats_take: null argument (rows)");
    if (n_rows < 1 || n_rows > ((int64_t)1 << 31) - 1) fail("sr_stats_take: n_rows is %lld; take 1 .. 2^31 - 1 rows", (long long)n_rows);
    for (int64_t i = 0; i < n_rows; i++)
        if (rows[i] < 0 || rows[i] >= s.n)
            fail("sr_stats_take: rows[%lld] is %lld, the handle holds sessions 0 .. %lld; pass 0-based row indices", (long long)i, (long long)rows[i],
                 (long long)(s.n - 1));
    const int64_t kd = (int64_t)s.K * s.D;
    if (n_rows > ((int64_t)1 << 36) / kd) fail("sr_stats_take: statistics of more than 2^36 values; take fewer rows at a time");
    stats_on_device(s, "sr_stats_take");
    auto &w = per_device<JfaStatsScratch>();
    SRStats *h = stats_new(n_rows, s.K, s.D);
    try {
        w.rows.upload(rows, (size_t)n_rows);
        hipStream_t st = ctx().stream;
        ScopedKernelTimer t(T_JFA_GRAM);
        hipLaunchKernelGGL(jfa_take_kernel, dim3((unsigned)n_rows, (unsigned)std::min<int64_t>(65535, (s.K + JFA_WG - 1) / JFA_WG)), dim3(JFA_WG), 0, st,
                           s.N.p, w.rows.p, h->N.p, (int64_t)s.K);
        SR_HIP(hipGetLastError());
        hipLaunchKernelGGL(jfa_take_kernel, dim3((unsigned)n_rows, (unsigned)std::min<int64_t>(65535, (kd + JFA_WG - 1) / JFA_WG)), dim3(JFA_WG), 0, st,
                           s.F.p, w.rows.p, h->F.p, kd);
        SR_HIP(hipGetLastError());
    } catch (...) {
        stats_close(h);
        throw;
    }
    try {
        sync_stream();
    } catch (...) {
        stats_close(h);
        throw;
    }
    return h;
}

// ---- grouping and centring ----

namespace {
struct CentreIndex {
    int64_t G = 0, P = 0;                  // rows of the result; labels that occur
    std::vector<int> order, gstart, lab;   // mode 0: sessions by (label, session), group starts; mode 1: a session's compact label
    std::vector<int64_t> present;          // the labels that occur, ascending
    std::vector<int4> entries;             // mode 0: all chunks' entries
    std::vector<size_t> chunk_begin;       // mode 0: [n_chunks + 1]
};
}  // namespace

static void centre_index(int mode, const int64_t *ids, int64_t n, const JfaCentrePlan &pl, CentreIndex &ix) {
    ix.order.resize((size_t)n);
    for (int64_t j = 0; j < n; j++) ix.order[(size_t)j] = (int)j;
    std::stable_sort(ix.order.begin(), ix.order.end(), [ids](int a, int b) { return ids[a] < ids[b]; });
    ix.gstart.clear();
    ix.present.clear();
    for (int64_t i = 0; i < n; i++)
        if (i == 0 || ids[ix.order[(size_t)i]] != ids[ix.order[(size_t)i - 1]]) {
            ix.gstart.push_back((int)i);
            ix.present.push_back(ids[ix.order[(size_t)i]]);
        }
    ix.gstart.push_back((int)n);
    ix.P = (int64_t)ix.present.size();
    if (mode == JFA_CENTRE_SESSIONS) {
        ix.G = n;
        ix.lab.resize((size_t)n);
        for (int64_t p = 0; p < ix.P; p++)
            for (int i = ix.gstart[(size_t)p]; i < ix.gstart[(size_t)p + 1]; i++) ix.lab[(size_t)ix.order[(size_t)i]] = (int)p;
        return;
    }
    ix.G = ix.P;
    std::vector<int> pos(ix.gstart.begin(), ix.gstart.end() - 1);
    ix.chunk_begin.assign((size_t)pl.n_chunks + 1, 0);
    for (int64_t ci = 0; ci < pl.n_chunks; ci++) {
        const int64_t j1 = std::min(n, (ci + 1) * pl.chunk);
        ix.chunk_begin[(size_t)ci] = ix.entries.size();
        for (int64_t g = 0; g < ix.G; g++) {
            const int b = pos[(size_t)g], end = ix.gstart[(size_t)g + 1];
            int e = b;
            while (e < end && ix.order[(size_t)e] < j1) e++;
            if (e == b) continue;
            ix.entries.push_back(make_int4((int)g, b, e - b, (b == ix.gstart[(size_t)g] ? 1 : 0) | (e == end ? 2 : 0)));
            pos[(size_t)g] = e;
        }
    }
    ix.chunk_begin[(size_t)pl.n_chunks] = ix.entries.size();
}

template <int VEC>
static void launch_centre(hipStream_t st, int64_t n_entries, int64_t col_blocks, const double *F, const double *N, const double *xu, int64_t j0,
                          const int *order, const int4 *entries, const int *lab, const double *Ng, const double *m, const double *z, const double *d,
                          const double *yv, double *Fc, int K, int D) {
    hipLaunchKernelGGL((jfa_centre_kernel<VEC>), dim3((unsigned)n_entries, (unsigned)col_blocks), dim3(JFA_WG), 0, st, F, N, xu, j0, order, entries, lab,
                       Ng, m, z, d, yv, Fc, K, D, (int64_t)K * D);
    SR_HIP(hipGetLastError());
}

SRJfa *jfa_open_centred(const SRStats *sp, const double *E, const double *m, int mode, const int64_t *ids, int64_t n_labels, const double *d,
                        const double *z, const double *v, int Ry, const double *y, const double *u, int Ru, const double *x) {
    const char *what = "sr_jfa_open_centred";
    const SRStats &s = stats_live(sp, what);
    std::string why;
    if (!E || !m) fail("%s: null argument (E and m [K D] are both required)", what);
    if ((d == nullptr) != (z == nullptr)) fail("%s: d [K D] and z [n_labels][K D] come together or not at all", what);
    if ((v == nullptr) != (y == nullptr)) fail("%s: v [Ry][K D] and y [n_labels][Ry] come together or not at all", what);
    if ((u == nullptr) != (x == nullptr)) fail("%s: u [Ru][K D] and x [n][Ru] come together or not at all", what);
    if (!v) Ry = 0;
    if (!u) Ru = 0;
    if (!jfa_centre_check_shape(s.n, s.K, s.D, mode, n_labels, Ry, Ru, v != nullptr, u != nullptr, why)) fail("%s", why.c_str());
    if (!jfa_centre_check_labels(ids, s.n, n_labels, why)) fail("%s", why.c_str());
    const int K = s.K, D = s.D;
    const int64_t n = s.n, kd = (int64_t)K * D;
    if (!jfa_check_finite(E, kd, "E", why) || !jfa_check_finite(m, kd, "m", why) || (d && !jfa_check_finite(d, kd, "d", why)) ||
        (z && !jfa_check_finite(z, n_labels * kd, "z", why)) || (v && !jfa_check_finite(v, Ry * kd, "v", why)) ||
        (y && !jfa_check_finite(y, n_labels * Ry, "y", why)) || (u && !jfa_check_finite(u, Ru * kd, "u", why)) ||
        (x && !jfa_check_finite(x, n * Ru, "x", why)))
        fail("%s", why.c_str());
    for (int64_t i = 0; i < kd; i++)
        if (!(E[i] > 0.0)) fail("JFA factors: E must be positive, element %lld is not; pass the UBM's variances", (long long)i);
    JfaCentrePlan pl;
    if (!plan_jfa_centre(n, n_labels, K, D, Ry, Ru, mode, (int64_t)jfa_scratch_mib() << 20, pl, why)) fail("%s", why.c_str());
    stats_on_device(s, what);

    CentreIndex ix;
    centre_index(mode, ids, n, pl, ix);
    const int64_t G = ix.G, P = ix.P;
    hipStream_t st = ctx().stream;
    auto &w = per_device<JfaStatsScratch>();
    std::vector<double> ie((size_t)kd), rows_buf;
    for (int64_t i = 0; i < kd; i++) ie[(size_t)i] = 1.0 / E[i];
    SRJfa *h = new SRJfa();
    try {
        h->G = G;
        h->K = K;
        h->D = D;
        h->device = ctx().device;
        h->N.alloc((size_t)(G * K));
        h->Fc.alloc((size_t)(G * kd));
        h->E.upload(E, (size_t)kd);
        h->iE.upload(ie.data(), (size_t)kd);
        w.m.upload(m, (size_t)kd);
        // the optional terms' rows, one per label that occurs (a label without sessions has no row anywhere)
        const double *dz = nullptr, *dd = nullptr, *dyv = nullptr;
        if (z) {
            rows_buf.resize((size_t)(P * kd));
            for (int64_t p = 0; p < P; p++) std::copy(z + ix.present[(size_t)p] * kd, z + (ix.present[(size_t)p] + 1) * kd, rows_buf.begin() + p * kd);
            w.z.upload(rows_buf.data(), rows_buf.size());
            w.d.upload(d, (size_t)kd);
            sync_stream();                     // (rows_buf is reused below)
            dz = w.z.p;
            dd = w.d.p;
        }
        if (v) {
            rows_buf.resize((size_t)(P * Ry));
            for (int64_t p = 0; p < P; p++) std::copy(y + ix.present[(size_t)p] * Ry, y + (ix.present[(size_t)p] + 1) * Ry, rows_buf.begin() + p * Ry);
            w.y.upload(rows_buf.data(), rows_buf.size());
            w.v.upload(v, (size_t)(Ry * kd));
            w.yv.ensure((size_t)(P * kd));
            dense_gemm(T_JFA_GEMM_C, st, w.y.p, Ry, 1, w.v.p, kd, 1, w.yv.p, kd, P, kd, Ry, false, 0);          // y v
            dyv = w.yv.p;
        }
        if (u) {
            w.x.upload(x, (size_t)(n * Ru));
            w.u.upload(u, (size_t)(Ru * kd));
            w.xu.ensure((size_t)(pl.chunk * kd));
        }
        if (mode == JFA_CENTRE_SESSIONS) {
            w.lab.upload(ix.lab.data(), ix.lab.size());
            SR_HIP(hipMemcpyAsync(h->N.p, s.N.p, (size_t)(n * K) * sizeof(double), hipMemcpyDeviceToDevice, st));
        } else {
            w.order.upload(ix.order.data(), ix.order.size());
            w.gstart.upload(ix.gstart.data(), ix.gstart.size());
            w.entries.upload(ix.entries.data(), ix.entries.size());
            ScopedKernelTimer t(T_JFA_GRAM);
            hipLaunchKernelGGL(jfa_group_counts_kernel, dim3((unsigned)G, (unsigned)((K + JFA_WG - 1) / JFA_WG)), dim3(JFA_WG), 0, st, s.N.p, w.order.p,
                               w.gstart.p, h->N.p, K);
            SR_HIP(hipGetLastError());
        }
        for (int64_t ci = 0; ci < pl.n_chunks; ci++) {
            const int64_t j0 = ci * pl.chunk, nc = std::min(pl.chunk, n - j0);
            if (u) dense_gemm(T_JFA_GEMM_C, st, w.x.p + j0 * Ru, Ru, 1, w.u.p, kd, 1, w.xu.p, kd, nc, kd, Ru, false, 0);      // x u of the chunk
            int64_t n_entries = nc;
            const int4 *entries = nullptr;
            if (mode == JFA_CENTRE_GROUPS) {
                n_entries = (int64_t)(ix.chunk_begin[(size_t)ci + 1] - ix.chunk_begin[(size_t)ci]);
                entries = w.entries.p + ix.chunk_begin[(size_t)ci];
            }
            if (n_entries == 0) continue;
            ScopedKernelTimer t(T_JFA_GRAM);
            const double *xu = u ? w.xu.p : nullptr;
            const int *order = mode == JFA_CENTRE_GROUPS ? w.order.p : nullptr, *lab = mode == JFA_CENTRE_SESSIONS ? w.lab.p : nullptr;
            if (pl.vec == 2)
                launch_centre<2>(st, n_entries, pl.centre.y, s.F.p, s.N.p, xu, j0, order, entries, lab, h->N.p, w.m.p, dz, dd, dyv, h->Fc.p, K, D);
            else
                launch_centre<1>(st, n_entries, pl.centre.y, s.F.p, s.N.p, xu, j0, order, entries, lab, h->N.p, w.m.p, dz, dd, dyv, h->Fc.p, K, D);
        }
        sync_stream();
    } catch (...) {
        delete h;
        throw;
    }
    return h;
}

void jfa_statistics(SRJfa &h, double *N, double *Fc) {
    jfa_check_handle(h, "sr_jfa_statistics");
    if (N) h.N.download(N, (size_t)(h.G * h.K));
    if (Fc) h.Fc.download(Fc, (size_t)(h.G * h.K) * (size_t)h.D);
    sync_stream();
}

void jfa_zd(SRJfa &h, double *d, int n_iter, double *z, double *a, double *b) {
    std::string why;
    const int64_t kd = (int64_t)h.K * h.D;
    if (!d) fail("sr_jfa_zd: null argument (d [K D] is required)");
    if (n_iter < 0) fail("sr_jfa_zd: n_iter must be >= 0 (0: z, a and b for the d given, d untouched)");
    if (!jfa_check_finite(d, kd, "d", why)) fail("%s", why.c_str());
    jfa_check_handle(h, "sr_jfa_zd");
    hipStream_t st = ctx().stream;
    h.zd_d.upload(d, (size_t)kd);
    h.zd_a.ensure((size_t)kd);
    h.zd_b.ensure((size_t)kd);
    if (z) h.zd_z.ensure((size_t)(h.G * kd));
    {
        ScopedKernelTimer t(T_JFA_GRAM);
        hipLaunchKernelGGL(jfa_zd_kernel, dim3((unsigned)((kd + JFA_ZD_WG - 1) / JFA_ZD_WG)), dim3(JFA_ZD_WG), 0, st, h.N.p, h.Fc.p, h.E.p, h.zd_d.p, n_iter,
                           z ? h.zd_z.p : nullptr, h.zd_a.p, h.zd_b.p, h.G, h.K, h.D, kd);
        SR_HIP(hipGetLastError());
    }
    if (n_iter > 0) h.zd_d.download(d, (size_t)kd);
    if (z) h.zd_z.download(z, (size_t)(h.G * kd));
    if (a) h.zd_a.download(a, (size_t)kd);
    if (b) h.zd_b.download(b, (size_t)kd);
    sync_stream();
}

// ---- the scorers on a statistics handle ----

int64_t launch_segment_totals(hipStream_t st, const double *N, int64_t T, int K, double *nt) {
    auto &w = per_device<JfaStatsScratch>();
    const int64_t blocks = (T + JFA_WG - 1) / JFA_WG;
    w.empty.ensure((size_t)blocks);
    {
        ScopedKernelTimer t(T_JFA_GRAM);
        hipLaunchKernelGGL(jfa_segment_totals_kernel, dim3((unsigned)blocks), dim3(JFA_WG), 0, st, N, T, K, nt, w.empty.p);
        SR_HIP(hipGetLastError());
    }
    std::vector<int> host((size_t)blocks);
    w.empty.download(host.data(), host.size());
    sync_stream();
    int64_t empty = 0;
    for (int v : host) empty += v;
    return empty;
}

void jfa_score_stats(int mode, const SRStats *tst, int64_t J, int Ry, int Ru, const double *m, const double *E, const double *d, const double *v,
                     const double *u, const double *z, const double *y, const double *x, const unsigned char *mask, int64_t mask_rows,
                     int64_t mask_cols, double *out, int64_t *empty_segments, int64_t *bad_segments) {
    const char *what = mode == JFA_SCORE_LINEAR ? "sr_jfa_score_linear_stats" : "sr_jfa_score_integrated_stats";
    const SRStats &s = stats_live(tst, what);
    const int64_t T = s.n;
    const int K = s.K, D = s.D;
    std::string why;
    if (!jfa_score_check_inputs_resident(T, J, K, D, Ry, Ru, mode, m, E, d, v, u, z, y, x, mask, mask_rows, mask_cols, why)) fail("%s", why.c_str());
    if (!out) fail("%s: null argument (the score matrix)", what);
    JfaScorePlan pl;
    if (!plan_jfa_score(T, J, K, D, Ry, Ru, mode, (int64_t)jfa_scratch_mib() << 20, (int)jfa_lds_rows(), 1, pl, why)) fail("%s", why.c_str());
    stats_on_device(s, what);
    if (!plan_jfa_score(T, J, K, D, Ry, Ru, mode, (int64_t)jfa_scratch_mib() << 20, (int)jfa_lds_rows(), std::max(1, ctx().n_cu), pl, why))
        fail("%s", why.c_str());
    auto &w = per_device<JfaStatsScratch>();
    w.nt.ensure((size_t)T);
    const int64_t empty = launch_segment_totals(ctx().stream, s.N.p, T, K, w.nt.p);
    jfa_score_device(pl, T, J, K, D, Ry, Ru, s.N.p, s.F.p, w.nt.p, m, E, d, v, u, z, y, x, mask, out, bad_segments);
    if (empty_segments) *empty_segments = empty;
}

}  // namespace sr
