// bw_stats.hip -- batched per-utterance Baum-Welch statistics against one diagonal model of a set (the UBM): the front of a JFA /
// i-vector / supervector leg (the reference's src/jfa/collect_suf_stats.m + sc_compute_suf_stats.m: MATLAB there, one session at
// a time).  For utterance u, mixture k, with gamma_k(t) = w_k N(x_t; mu_k, sigma_k^2) / sum_j w_j N(x_t; mu_j, sigma_j^2):
//   N[u][k]    = sum_t gamma_k(t)
//   F[u][k][d] = sum_t gamma_k(t) x_t[d]          (mixture-major: the reference's supervector order)
//   ll[u]      = sum_t ln sum_j w_j N(x_t; ...)
// Three kernels, none of them shared with the scoring or the training paths (and none touching the pass counters):
//   A. bw_lse_kernel<DP>    lane = frame, the row in registers, the model's records through LDS eight at a time in the 2-FMA log2
//                           form of the vector engine on ITS packed parameters (gmm_model.hpp), centred on the set's centre; an
//                           online maximum / sum gives the frame's log2 total as the pair {max, log2 sum}, both fp32.
//   B. bw_stats_kernel<DP>  the segmented sibling of em_stats_mfma_kernel: a workgroup owns 64 mixtures and one frame RANGE of one
//                           utterance (bw_plan.cpp), walks it in tiles of 128 frames; per tile a wave (lane = two frames)
//                           recomputes its 16 mixtures' log2 densities -- the same fused multiply-adds in the same order as
//                           pass A, so a frame's posteriors sum to 1 to fp32 rounding --, forms exp2((lp - max) - log2 sum) on the
//                           vector ALU, passes the posteriors through LDS into the A layout and lets v_mfma_f64_16x16x4_f64
//                           accumulate the columns [x_0 .. x_{D-1} | 1] from fp32-exact operands.  The accumulators stay in
//                           registers until the range is done; one float64 slab per (range, mixture block).
//   C. bw_reduce_kernel     adds an utterance's slabs in range order, float64, into N[u] and F[u].
// plus bw_ll_kernel (an utterance's ll and its count of dropped frames, float64, fixed order).
// A frame contributes iff its log2 total is finite: a row holding a NaN or an infinity, or values so large that every density
// is -inf, adds nothing to N, F and ll and is counted in dropped[u].  Posteriors are formed in the LOG domain: a frame far from
// every mixture, whose linear-domain densities would all underflow (the reference's gaussian_posteriors.m then divides 0 by 0),
// has a finite total and contributes like any other.
// Deterministic: no atomics; an utterance's cut into ranges depends on its own length and the option bw_range_frames only, its
// slabs are added in range order whatever group they were computed in -- N, F and ll of an utterance are the same bits alone, in
// any batch and under any scratch bound.
// Two entry points share one body (bw_stats_run): sr_bw_stats_batch reduces into the per-device scratch and copies N and F home;
// sr_bw_stats_resident reduces into the buffers of a statistics handle (jfa_dev.hpp, jfa_stats.hip) and leaves them there.
#include "batch.hpp"
#include "bw_plan.hpp"
#include "bw_stats.hpp"
#include "gmm_model.hpp"
#include "jfa_dev.hpp"
#include "score.hpp"
#include "wave_ops.hpp"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

namespace sr {

static_assert(sizeof(BwRange) == sizeof(TileDesc), "the range table is read on the device as tile descriptors");

typedef double bw_f64x4 __attribute__((ext_vector_type(4)));
constexpr int BW_WAVES = BW_WG / 64, BW_MB = BW_WG_MIX / BW_WAVES;      // 4 waves, 16 mixtures each
constexpr int BW_F = BW_TILE / 64;                                       // frames per lane in the posterior phase
// row strides = 2 mod 32: the operand reads of the matrix phase are ds_read_b32, conflict-free at this stride (em.hip, measured)
constexpr int BW_XS = BW_TILE + 2, BW_GS = BW_TILE + 2;
constexpr float BW_M0 = -3.0e38f;              // where the running maximum starts: finite, so that exp2(m - m_new) never sees inf - inf
constexpr double BW_LN2 = 0.693147180559945309417;

// The constants of a record as these kernels use them: a dead mixture -- the padding of the last record, a weight of 0: c = NEG_BIG
// in the packed layout -- is -inf here, not -1e30: its posterior is exactly 0 for every frame, and a frame whose real densities
// are all -inf does not get a finite total from the padding.
__device__ __forceinline__ float4 bw_constants(float4 c) {
    const float ninf = -__builtin_inff();
    return make_float4(c.x <= NEG_BIG ? ninf : c.x, c.y <= NEG_BIG ? ninf : c.y, c.z <= NEG_BIG ? ninf : c.z, c.w <= NEG_BIG ? ninf : c.w);
}

// does the frame contribute?  (the same test in pass B and in the ll kernel)
__device__ __forceinline__ bool bw_live(float2 l) { return __builtin_isfinite(l.x + l.y); }

// ---- A. per-frame log2-sum-exp ----
template <int DP>
__global__ __launch_bounds__(BW_WG)
void bw_lse_kernel(const float *__restrict__ X, int64_t n_frames, int dim, const float4 *__restrict__ params /* the model's records */,
                   const float *__restrict__ center, int n_records, float2 *__restrict__ lse /* [n_frames] {max, log2 sum} */) {
    constexpr int REC = 2 * DP + 1;
    __shared__ float4 rec_s[CB * REC];
    const int tid = threadIdx.x;
    const int64_t frame = (int64_t)blockIdx.x * BW_WG + tid;
    const bool valid = frame < n_frames;
    float x[DP];
    {
        const float *src = X + (valid ? frame : 0) * dim;
#pragma unroll
        for (int d = 0; d < DP; d++) x[d] = (d < dim ? src[d] : 0.f) - center[d];
    }
    float m = BW_M0, s = 0.f;
    for (int r0 = 0; r0 < n_records; r0 += CB) {
        const int nr = min(CB, n_records - r0);
        __syncthreads();                       // the previous records have been read by every lane
        for (int i = tid; i < nr * REC; i += BW_WG) {
            const float4 v = params[(size_t)r0 * REC + i];
            rec_s[i] = i % REC == 2 * DP ? bw_constants(v) : v;
        }
        __syncthreads();
#pragma unroll 1
        for (int r = 0; r < nr; r++) {
            const float4 *rec = rec_s + r * REC;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
            for (int d = 0; d < DP; d++) {
                const float4 p0 = rec[2 * d];
                const float4 p1 = rec[2 * d + 1];
                const float t0 = fmaf(x[d], p0.x, p0.y);
                const float t1 = fmaf(x[d], p0.z, p0.w);
                const float t2 = fmaf(x[d], p1.x, p1.y);
                const float t3 = fmaf(x[d], p1.z, p1.w);
                a0 = fmaf(t0, t0, a0);
                a1 = fmaf(t1, t1, a1);
                a2 = fmaf(t2, t2, a2);
                a3 = fmaf(t3, t3, a3);
            }
            const float4 cc = rec[2 * DP];
            const float l0 = cc.x - a0, l1 = cc.y - a1, l2 = cc.z - a2, l3 = cc.w - a3;
            const float mn = fmaxf(m, fmaxf(fmaxf(l0, l1), fmaxf(l2, l3)));
            s = s * __builtin_amdgcn_exp2f(m - mn) + ((__builtin_amdgcn_exp2f(l0 - mn) + __builtin_amdgcn_exp2f(l1 - mn)) +
                                                      (__builtin_amdgcn_exp2f(l2 - mn) + __builtin_amdgcn_exp2f(l3 - mn)));
            m = mn;
        }
    }
    if (valid) lse[frame] = make_float2(m, __builtin_amdgcn_logf(s));
}

// ---- an utterance's log-likelihood and its dropped frames ----
__global__ __launch_bounds__(BW_WG)
void bw_ll_kernel(const float2 *__restrict__ lse, const int64_t *__restrict__ offsets, double *__restrict__ ll, long long *__restrict__ dropped) {
    __shared__ double sa[BW_WG];
    __shared__ long long sd[BW_WG];
    const int tid = threadIdx.x;
    const int64_t b = offsets[blockIdx.x], e = offsets[blockIdx.x + 1];
    double a = 0.0;
    long long dr = 0;
    for (int64_t t = b + tid; t < e; t += BW_WG) {
        const float2 l = lse[t];
        if (bw_live(l)) a += ((double)l.x + (double)l.y) * BW_LN2;
        else dr++;
    }
    sa[tid] = a;
    sd[tid] = dr;
    __syncthreads();
    for (int w = BW_WG / 2; w > 0; w >>= 1) {
        if (tid < w) {
            sa[tid] += sa[tid + w];
            sd[tid] += sd[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        ll[blockIdx.x] = sa[0];
        dropped[blockIdx.x] = sd[0];
    }
}

// ---- B. the statistics of one (range, block of 64 mixtures) on the fp64 matrix cores ----
// v_mfma_f64_16x16x4_f64: M = 16 mixtures, N = 16 statistic columns, K = 4 frames; lane l supplies A[mixture l & 15][frame l >> 4]
// and B[frame l >> 4][column l & 15] and receives D[mixture (l >> 4) + 4 r][column l & 15], r = 0..3 (em.hip).
template <int DP>
__global__ __launch_bounds__(BW_WG, 2)
void bw_stats_kernel(const float *__restrict__ X, int dim, const float4 *__restrict__ params, const float *__restrict__ center,
                     int n_records, const float2 *__restrict__ lse, const TileDesc *__restrict__ ranges /* of this group */,
                     double *__restrict__ slabs /* [gridDim.x][gridDim.y * 64][NCB * 16] */) {
    constexpr int REC = 2 * DP + 1;
    constexpr int NFULL = DP / 16, NCB = (DP + 1 + 15) / 16;       // NCB - NFULL == 1: the block that holds the count column
    constexpr int RECS_WG = BW_WG_MIX / KB;
    static_assert(NCB - NFULL == 1, "one mixed block");
    extern __shared__ float4 bw_lds[];
    float4 *par = bw_lds;                                          // [RECS_WG * REC]
    float *xt = reinterpret_cast<float *>(par + RECS_WG * REC);    // raw rows of the tile, [d][frame], stride BW_XS
    float *gs_all = xt + DP * BW_XS;                               // posteriors, per wave [mixture][frame], stride BW_GS
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rec0 = blockIdx.y * RECS_WG;
    const TileDesc rg = ranges[blockIdx.x];
    // this workgroup's parameter records -> LDS (dead records beyond the model: c = -inf, everything else 0)
    for (int i = tid; i < RECS_WG * REC; i += BW_WG) {
        const int r = rec0 + i / REC;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < n_records) v = params[(size_t)r * REC + (i % REC)];
        else if (i % REC == 2 * DP) v = make_float4(NEG_BIG, NEG_BIG, NEG_BIG, NEG_BIG);
        par[i] = i % REC == 2 * DP ? bw_constants(v) : v;
    }
    if (DP != dim)                                                 // padded dimensions read as 0
        for (int i = tid; i < DP * BW_XS; i += BW_WG) xt[i] = 0.f;

    // column 16 cb + j of this lane's B operand: x_q for q < DP, the constant 1 at q == DP, 0 beyond -- y = v al + ga
    const int j = lane & 15, fl = lane >> 4;
    int boff[NFULL > 0 ? NFULL : 1];
#pragma unroll
    for (int cb = 0; cb < NFULL; cb++) boff[cb] = (16 * cb + j) * BW_XS + fl;
    const int qm = 16 * NFULL + j;
    const int moff = (qm < DP ? qm : 0) * BW_XS + fl;
    const double al = qm < DP ? 1.0 : 0.0, ga = qm == DP ? 1.0 : 0.0;
    bw_f64x4 acc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) acc[cb] = (bw_f64x4){0.0, 0.0, 0.0, 0.0};
    float *g = gs_all + (size_t)wave * BW_MB * BW_GS;
    const float4 *mypar = par + (size_t)wave * (BW_MB / KB) * REC;

    const int n_tiles = (rg.count + BW_TILE - 1) / BW_TILE;
    for (int tile = 0; tile < n_tiles; tile++) {
        __syncthreads();                       // every wave is done with the previous tile's rows (and `par` is filled)
        // the tile's rows -> xt[d][frame], lane = frame, the four waves every fourth dimension.  A frame that does not
        // contribute (beyond the range, or dropped) goes in as a row of zeros with the "maximum" +1e30: its densities are
        // finite and every posterior below is exp2(-1e30) = 0 -- nothing of a NaN row reaches the matrix cores
        float lm[BW_F], ls[BW_F];
#pragma unroll
        for (int h = 0; h < BW_F; h++) {
            const int fr = tile * BW_TILE + 64 * h + lane;
            bool live = false;
            lm[h] = 1.0e30f;
            ls[h] = 0.f;
            if (fr < rg.count) {
                const float2 l = lse[rg.start + fr];
                live = bw_live(l);
                if (live) {
                    lm[h] = l.x;
                    ls[h] = l.y;
                }
            }
            const float *src = X + (rg.start + (live ? fr : 0)) * dim;
            for (int d = wave; d < dim; d += BW_WAVES) xt[d * BW_XS + 64 * h + lane] = live ? src[d] : 0.f;
        }
        __syncthreads();                       // this tile's rows are in place for every wave
        // ---- posteriors of this wave's 16 mixtures, lane = frames l and l + 64: pass A's arithmetic, operation for operation
        float x[BW_F][DP];
#pragma unroll
        for (int h = 0; h < BW_F; h++)
#pragma unroll
            for (int d = 0; d < DP; d++) x[h][d] = xt[d * BW_XS + 64 * h + lane] - center[d];
        // (the records never change: without an offset the compiler cannot see through, it hoists every parameter read out of
        // the tile loop and spills -- em.hip)
        int roff = 0;
        asm volatile("" : "+s"(roff));
#pragma unroll 1
        for (int r = 0; r < BW_MB / KB; r++) {
            const float4 *rec = mypar + roff + r * REC;
            float a4[BW_F][KB];
#pragma unroll
            for (int h = 0; h < BW_F; h++)
#pragma unroll
                for (int q = 0; q < KB; q++) a4[h][q] = 0.f;
#pragma unroll
            for (int d = 0; d < DP; d++) {
                const float4 p0 = rec[2 * d];
                const float4 p1 = rec[2 * d + 1];
#pragma unroll
                for (int h = 0; h < BW_F; h++) {
                    const float t0 = fmaf(x[h][d], p0.x, p0.y);
                    const float t1 = fmaf(x[h][d], p0.z, p0.w);
                    const float t2 = fmaf(x[h][d], p1.x, p1.y);
                    const float t3 = fmaf(x[h][d], p1.z, p1.w);
                    a4[h][0] = fmaf(t0, t0, a4[h][0]);
                    a4[h][1] = fmaf(t1, t1, a4[h][1]);
                    a4[h][2] = fmaf(t2, t2, a4[h][2]);
                    a4[h][3] = fmaf(t3, t3, a4[h][3]);
                }
            }
            const float4 cc = rec[2 * DP];
#pragma unroll
            for (int h = 0; h < BW_F; h++) {
                g[(r * KB + 0) * BW_GS + 64 * h + lane] = __builtin_amdgcn_exp2f(((cc.x - a4[h][0]) - lm[h]) - ls[h]);
                g[(r * KB + 1) * BW_GS + 64 * h + lane] = __builtin_amdgcn_exp2f(((cc.y - a4[h][1]) - lm[h]) - ls[h]);
                g[(r * KB + 2) * BW_GS + 64 * h + lane] = __builtin_amdgcn_exp2f(((cc.z - a4[h][2]) - lm[h]) - ls[h]);
                g[(r * KB + 3) * BW_GS + 64 * h + lane] = __builtin_amdgcn_exp2f(((cc.w - a4[h][3]) - lm[h]) - ls[h]);
            }
        }
        wave_sync();
        // ---- BW_TILE / 4 frame groups x NCB column blocks on the fp64 matrix cores
#pragma unroll 4
        for (int fg = 0; fg < BW_TILE / 4; fg++) {
            const double av = (double)g[j * BW_GS + 4 * fg + fl];             // A[mixture j][frame 4 fg + fl]
#pragma unroll
            for (int cb = 0; cb < NFULL; cb++) {
                const double v = (double)xt[boff[cb] + 4 * fg];
                acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, v, acc[cb], 0, 0, 0);
            }
            const double v = (double)xt[moff + 4 * fg];
            acc[NFULL] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, __builtin_fma(v, al, ga), acc[NFULL], 0, 0, 0);
        }
        wave_sync();                           // (g is rewritten by this wave's next tile)
    }
    // ---- this workgroup's sums -> its slab: D[mixture (l >> 4) + 4 r][column l & 15]
    double *slab = slabs + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * BW_WG_MIX * (NCB * 16);
#pragma unroll
    for (int cb = 0; cb < NCB; cb++)
#pragma unroll
        for (int r = 0; r < 4; r++)
            slab[(size_t)(wave * BW_MB + fl + 4 * r) * (NCB * 16) + 16 * cb + j] = acc[cb][r];
}

// ---- C. an utterance's slabs of this group, in range order, onto what the groups before it left in N[u] and F[u] ----
__global__ __launch_bounds__(BW_WG)
void bw_reduce_kernel(const double *__restrict__ slabs, const int4 *__restrict__ segs /* {utterance, first range of the group, ranges, 0} */,
                      int blocks_per_seg, int K, int D, int dp, int n_mix_blocks, int nc, double *__restrict__ N, double *__restrict__ F) {
    const int4 sg = segs[blockIdx.x / blocks_per_seg];
    const int e = (blockIdx.x % blocks_per_seg) * BW_WG + threadIdx.x;
    if (e >= K * (D + 1)) return;
    const int k = e / (D + 1), c = e - k * (D + 1);
    const int col = c < D ? c : dp;
    double *dst = c < D ? F + ((size_t)sg.x * K + k) * D + c : N + (size_t)sg.x * K + k;
    const size_t stride = (size_t)n_mix_blocks * BW_WG_MIX * nc;
    const double *src = slabs + (size_t)sg.y * stride + (size_t)k * nc + col;
    double acc = *dst;
    for (int r = 0; r < sg.z; r++) acc += src[(size_t)r * stride];
    *dst = acc;
}

// ---- host ----

static std::atomic<long> &bw_scratch_option() {
    static std::atomic<long> v{(long)(BW_DEFAULT_SCRATCH >> 20)};
    return v;
}
static std::atomic<long> &bw_range_option() {
    static std::atomic<long> v{0};
    return v;
}
void set_bw_scratch_mib(long v) { bw_scratch_option().store(v); }
long bw_scratch_mib() { return bw_scratch_option().load(); }
void set_bw_range_frames(long v) { bw_range_option().store(v); }
long bw_range_frames() { return bw_range_option().load(); }

namespace {
struct BwScratch {
    DevBuf<float2> lse;
    DevBuf<double> slabs, N, F, ll;
    DevBuf<long long> dropped;
    DevBuf<TileDesc> ranges;
    DevBuf<int4> segs;
    PinnedBuf<double> h_ll;
    PinnedBuf<long long> h_dropped;
};
}  // namespace

static size_t bw_lds_bytes(int dp) {
    return (size_t)(BW_WG_MIX / KB) * (2 * dp + 1) * sizeof(float4) + (size_t)dp * BW_XS * sizeof(float) +
           (size_t)BW_WG_MIX * BW_GS * sizeof(float);
}

template <int DP>
static void launch_bw_lse(dim3 grid, hipStream_t st, const float *X, int64_t n, int dim, const float4 *params, const float *center,
                          int n_records, float2 *lse) {
    hipLaunchKernelGGL((bw_lse_kernel<DP>), grid, dim3(BW_WG), 0, st, X, n, dim, params, center, n_records, lse);
}

template <int DP>
static void launch_bw_stats(dim3 grid, hipStream_t st, const float *X, int dim, const float4 *params, const float *center, int n_records,
                            const float2 *lse, const TileDesc *ranges, double *slabs) {
    static bool attr_set[MAX_DEVICES] = {};
    if (!attr_set[ctx().device]) {
        SR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&bw_stats_kernel<DP>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)bw_lds_bytes(DP)));
        attr_set[ctx().device] = true;
    }
    hipLaunchKernelGGL((bw_stats_kernel<DP>), grid, dim3(BW_WG), bw_lds_bytes(DP), st, X, dim, params, center, n_records, lse, ranges, slabs);
}

#define SR_BW_DIMS(CASE) CASE(8) CASE(13) CASE(16) CASE(24) CASE(26) CASE(32) CASE(34) CASE(39) CASE(40)

// The passes of one call, N and F into device memory the caller names: the per-device scratch (sr_bw_stats_batch, which then
// copies them home) or a statistics handle's own buffers (sr_bw_stats_resident).  `out(U, K, D)` is asked for the two pointers
// once every refusal is past and the device is bound; ll and dropped come back through the pinned staging buffers.
struct BwOut {
    double *N = nullptr, *F = nullptr;
};

template <typename OutFn>
static void bw_stats_run(const char *what, SRModelSet &set, int model, SRBatch &feat, OutFn &&out, double *N_out, double *F_out, double *ll_out,
                         int64_t *dropped_out) {
    // every refusal before the device is touched
    const int S = set.host.n_models, D = set.host.dim;
    const int K = (model >= 0 && model < (int)set.host.model_mixtures.size()) ? set.host.model_mixtures[model] : 0;
    std::string why;
    if (!bw_check(feat.kind == SRBatch::FEATURES, S, model, K, D, feat.dim, why)) fail("%s", why.c_str());
    const int U = feat.n_utt;
    const int64_t n = feat.n_rows;
    if (gpu_runtime_lost()) fail_gpu_runtime_lost(what);
    ensure_device();
    feat.bind_device();
    if (set.device != ctx().device) fail("model set lives on device %d, the calling thread is on device %d", set.device, ctx().device);
    std::vector<int64_t> lengths((size_t)U);
    for (int u = 0; u < U; u++) lengths[u] = feat.offsets[u + 1] - feat.offsets[u];
    BwPlan pl;
    if (!plan_bw(K, D, lengths.data(), U, bw_range_frames(), (int64_t)bw_scratch_mib() << 20, ctx().n_cu, pl, why)) fail("%s", why.c_str());
    if (pl.dp != set.host.dp) fail("Baum-Welch statistics: the set is packed at %d padded dimensions, the plan expects %d", set.host.dp, pl.dp);
    const BwOut dst = out(U, K, D);
    if (U == 0) return;
    const int n_records = (K + KB - 1) / KB;
    const float4 *params = reinterpret_cast<const float4 *>(set.d_params.p) + set.host.chunks[set.host.model_chunk_begin[model]].offset_f4;
    const float *center = set.d_center0.p;
    hipStream_t st = ctx().stream;
    auto &w = per_device<BwScratch>();
    const size_t nN = (size_t)U * K, nF = nN * D;
    w.ll.ensure((size_t)U);
    w.dropped.ensure((size_t)U);
    SR_HIP(hipMemsetAsync(dst.N, 0, nN * sizeof(double), st));
    SR_HIP(hipMemsetAsync(dst.F, 0, nF * sizeof(double), st));
    if (n > 0) {
        w.lse.ensure((size_t)n);
        ScopedKernelTimer t(T_BW_LSE);
        const dim3 grid((unsigned)pl.lse_grid);
#define SR_CASE(V) case V: launch_bw_lse<V>(grid, st, feat.data.p, n, D, params, center, n_records, w.lse.p); break;
        switch (pl.dp) {
            SR_BW_DIMS(SR_CASE)
            default: fail("no Baum-Welch kernel for padded dim %d", pl.dp);
        }
#undef SR_CASE
        SR_HIP(hipGetLastError());
    }
    // (an utterance without frames reads nothing of `lse`)
    hipLaunchKernelGGL(bw_ll_kernel, dim3((unsigned)U), dim3(BW_WG), 0, st, w.lse.p, feat.d_offsets.p, w.ll.p, w.dropped.p);
    SR_HIP(hipGetLastError());

    const int64_t n_ranges = (int64_t)pl.ranges.size();
    const int nc = pl.ncb * 16;
    if (n_ranges > 0) {
        w.slabs.ensure((size_t)std::min(n_ranges, pl.group_ranges) * (size_t)(pl.slab_bytes / (int64_t)sizeof(double)));
        w.ranges.upload(reinterpret_cast<const TileDesc *>(pl.ranges.data()), pl.ranges.size());
        // the (utterance, group) segments of the reduce, all groups in one table
        std::vector<int4> segs;
        std::vector<size_t> seg_begin((size_t)pl.n_groups + 1, 0);
        for (int64_t gi = 0; gi < pl.n_groups; gi++) {
            const int64_t r0 = gi * pl.group_ranges, r1 = std::min(n_ranges, r0 + pl.group_ranges);
            seg_begin[gi] = segs.size();
            for (int64_t r = r0; r < r1;) {
                int64_t e = r + 1;
                while (e < r1 && pl.ranges[e].utt == pl.ranges[r].utt) e++;
                segs.push_back(make_int4(pl.ranges[r].utt, (int)(r - r0), (int)(e - r), 0));
                r = e;
            }
        }
        seg_begin[pl.n_groups] = segs.size();
        w.segs.upload(segs.data(), segs.size());
        for (int64_t gi = 0; gi < pl.n_groups; gi++) {
            const int64_t r0 = gi * pl.group_ranges, r1 = std::min(n_ranges, r0 + pl.group_ranges);
            {
                ScopedKernelTimer t(T_BW_STATS);
                const dim3 grid((unsigned)(r1 - r0), (unsigned)pl.n_mix_blocks);
#define SR_CASE(V) case V: launch_bw_stats<V>(grid, st, feat.data.p, D, params, center, n_records, w.lse.p, w.ranges.p + r0, w.slabs.p); break;
                switch (pl.dp) {
                    SR_BW_DIMS(SR_CASE)
                    default: fail("no Baum-Welch kernel for padded dim %d", pl.dp);
                }
#undef SR_CASE
                SR_HIP(hipGetLastError());
            }
            const int64_t n_segs = (int64_t)(seg_begin[gi + 1] - seg_begin[gi]);
            if (n_segs * pl.reduce_blocks > INT32_MAX) fail("Baum-Welch statistics: the reduce of one group needs more than 2^31 - 1 workgroups; lower bw_scratch_mib");
            {
                ScopedKernelTimer t(T_BW_REDUCE);
                hipLaunchKernelGGL(bw_reduce_kernel, dim3((unsigned)(n_segs * pl.reduce_blocks)), dim3(BW_WG), 0, st, w.slabs.p,
                                   w.segs.p + seg_begin[gi], (int)pl.reduce_blocks, K, D, pl.dp, pl.n_mix_blocks, nc, dst.N, dst.F);
                SR_HIP(hipGetLastError());
            }
        }
    }
    if (N_out) SR_HIP(hipMemcpyAsync(N_out, dst.N, nN * sizeof(double), hipMemcpyDeviceToHost, st));
    if (F_out) SR_HIP(hipMemcpyAsync(F_out, dst.F, nF * sizeof(double), hipMemcpyDeviceToHost, st));
    w.h_ll.ensure((size_t)U);
    w.h_dropped.ensure((size_t)U);
    SR_HIP(hipMemcpyAsync(w.h_ll.p, w.ll.p, (size_t)U * sizeof(double), hipMemcpyDeviceToHost, st));
    SR_HIP(hipMemcpyAsync(w.h_dropped.p, w.dropped.p, (size_t)U * sizeof(long long), hipMemcpyDeviceToHost, st));
    sync_stream();
    if (ll_out) std::memcpy(ll_out, w.h_ll.p, (size_t)U * sizeof(double));
    if (dropped_out)
        for (int u = 0; u < U; u++) dropped_out[u] = (int64_t)w.h_dropped.p[u];
}

void bw_stats_batch(SRModelSet &set, int model, SRBatch &feat, double *N_out, double *F_out, double *ll_out, int64_t *dropped_out) {
    if (feat.n_utt > 0 && (!N_out || !F_out)) {
        // (the shape's refusals come first, as they always did)
        std::string why;
        const int K = (model >= 0 && model < (int)set.host.model_mixtures.size()) ? set.host.model_mixtures[model] : 0;
        if (!bw_check(feat.kind == SRBatch::FEATURES, set.host.n_models, model, K, set.host.dim, feat.dim, why)) fail("%s", why.c_str());
        fail("sr_bw_stats_batch: null output (N and F are both required)");
    }
    bw_stats_run("sr_bw_stats_batch", set, model, feat, [](int U, int K, int D) {
        auto &w = per_device<BwScratch>();
        w.N.ensure((size_t)U * K);
        w.F.ensure((size_t)U * K * D);
        return BwOut{w.N.p, w.F.p};
    }, N_out, F_out, ll_out, dropped_out);
}

SRStats *bw_stats_resident(SRModelSet &set, int model, SRBatch &feat, double *ll_out, int64_t *dropped_out) {
    if (feat.n_utt < 1) {
        std::string why;
        const int K = (model >= 0 && model < (int)set.host.model_mixtures.size()) ? set.host.model_mixtures[model] : 0;
        if (!bw_check(feat.kind == SRBatch::FEATURES, set.host.n_models, model, K, set.host.dim, feat.dim, why)) fail("%s", why.c_str());
        fail("sr_bw_stats_resident: the batch holds no utterance; a statistics handle needs at least one session");
    }
    SRStats *h = nullptr;
    try {
        bw_stats_run("sr_bw_stats_resident", set, model, feat, [&h](int U, int K, int D) {
            h = stats_new(U, K, D);
            return BwOut{h->N.p, h->F.p};
        }, nullptr, nullptr, ll_out, dropped_out);
        stats_check_device(*h);
    } catch (...) {
        stats_close(h);
        throw;
    }
    return h;
}

}  // namespace sr
