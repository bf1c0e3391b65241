// gmm_topc.hip -- top-C Gaussian selection (Reynolds, Quatieri & Dunn 2000): fast scoring of a speaker set that was MAP-adapted,
// means only, from one UBM (gmmubm.cc:40-81), so that every model's component k keeps the UBM's sigma_k and w_k.  Per frame x:
//   t_k   = ln w_k - sum_d ln(sqrt(2 pi) sigma_kd) - sum_d (x_d - mu^bg_kd)^2 / (2 sigma_kd^2)          k = 0 .. K - 1
//   top   = the C indices of the largest t_k, descending, equal values to the lower index first
//   LL_bg = logsumexp over all K of t_k                                  (the background column stays exact)
//   LL_s  = logsumexp over k in top of the same expression with mu^s     (every other column: C components instead of K)
// S K D multiply-adds per frame become K D + S C D.  An approximation, so opt-in: nothing of the exact path calls into this file.
//
// Arithmetic: fp32, the direct form of the vector engine on ITS packed parameters (gmm_model.hpp: s = sqrt(log2e / 2) / sigma,
// m = -(mu - centre) s, c = log2e (ln w - sum ln(sqrt(2 pi) sigma)); log2 density = c - sum_d ((x_d - centre_d) s_kd + m_kd)^2),
// so the expanded form's conditioning limits never arise and C = K reproduces the exact path within the parity gate.
//
// A kernel that gathered S C D parameters per frame would read as much as the exact pass computes.  The layout is the
// mixture-of-experts one -- route frames to components, then run every component over ITS frames -- in chunks of frames whose
// scratch stays under the option "topc_scratch_mib" (topc_plan.cpp):
//   1. select   a lane per frame, the row in registers, the background's {s, m} by wave-uniform loads: all K terms through an
//               online log2-sum-exp (LL_bg) and into a running selection of CR >= C register slots (topc_select_kernel<TP, CR>);
//               C > 8: the K keys go to scratch and topc_rank_kernel places component k at its rank (K^2 compares per frame).
//               A non-finite key counts as -inf for the selection and slots start as placeholders that every real component
//               beats: a NaN frame selects 0 .. C - 1, distinct and in range.
//   2. route    histogram of the selected indices, exclusive scan (entries and runs per component), scatter of the (frame, slot)
//               pairs into per-component lists.  Integer atomics only: the ORDER inside a list varies from run to run, the
//               values do not -- every term is computed alone and written to its own place.
//   3. evaluate a workgroup per (component, run of its entries), a lane per model with the model's m_sk in registers; the
//               run's rows, already scaled, staged in LDS 64 at a time and read by broadcast; a coalesced row of S terms per
//               entry to terms[frame][slot][.] (topc_eval_kernel<TP>).
//   4. combine  a workgroup per tile (<= 64 frames of one utterance and one chunk), a lane per model: log2-sum-exp over the C slots,
//               the clamp, the tile's sum in float64 in frame order; gmm_finalize_kernel adds the tiles in its fixed order.
// No floating-point atomics anywhere: results are bit-identical from run to run.
// SR_CLAMP_COMPAT here is the plain threshold -- a per-frame value below ln DBL_MIN = -708.396 becomes ln 1e-15 -- and nothing
// else: the partial-product re-evaluation (gmm_flush.hip) belongs to the exact path.
#include "batch.hpp"
#include "gmm_model.hpp"
#include "lse.hpp"
#include "score.hpp"
#include "topc.hpp"
#include "topc_plan.hpp"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

namespace sr {

constexpr float TOPC_LN_DBL_MIN = -708.396418532264f;

// ---- 1. select ----

__global__ __launch_bounds__(TOPC_WG)
void topc_gather_bg_kernel(const float *__restrict__ scale, const float *__restrict__ mtab, int n, int S, int bg, float2 *__restrict__ out) {
    const int i = blockIdx.x * TOPC_WG + threadIdx.x;
    if (i < n) out[i] = make_float2(scale[i], mtab[(int64_t)i * S + bg]);
}

// (m, ssum) <- (m, ssum) (+) the log2-domain term t: one exponential per term.  m starts at -3e38 (finite: a term of -inf
// adds 0 and never becomes m), a NaN term makes ssum NaN.
__device__ __forceinline__ void topc_lse_add(float t, float &m, float &ssum) {
    const float dlt = t - m;
    const float e = __builtin_amdgcn_exp2f(-fabsf(dlt));
    const bool up = dlt > 0.0f;
    ssum = up ? fmaf(ssum, e, 1.0f) : ssum + e;
    m = up ? t : m;
}

template <int TP, int CR>
__global__ __launch_bounds__(TOPC_WG)
void topc_select_kernel(const float *__restrict__ X, int D, int64_t f0, int nf, const float2 *__restrict__ bg, const float *__restrict__ cst,
                        const float *__restrict__ center, int K, int C, float *__restrict__ ll_bg, int *__restrict__ sel,
                        float *__restrict__ keys) {
    constexpr int CRN = CR > 0 ? CR : 1;
    const int f = blockIdx.x * TOPC_WG + threadIdx.x;
    const bool live = f < nf;
    const float *row = X + (f0 + (live ? f : 0)) * (int64_t)D;
    float x[TP];
#pragma unroll
    for (int d = 0; d < TP; d++) x[d] = d < D ? row[d] - center[d] : 0.0f;
    float m = -3.0e38f, ssum = 0.0f;
    float bv[CRN];
    int bi[CRN];
#pragma unroll
    for (int j = 0; j < CRN; j++) {
        bv[j] = -__builtin_inff();
        bi[j] = K + j;                       // a placeholder: every real component beats it
    }
    for (int k = 0; k < K; k++) {
        const float2 *__restrict__ p = bg + (int64_t)k * TP;       // wave-uniform
        float q0 = 0.0f, q1 = 0.0f;
#pragma unroll
        for (int d = 0; d < TP; d += 2) {
            const float z0 = fmaf(x[d], p[d].x, p[d].y), z1 = fmaf(x[d + 1], p[d + 1].x, p[d + 1].y);
            q0 = fmaf(z0, z0, q0);
            q1 = fmaf(z1, z1, q1);
        }
        const float t = cst[k] - (q0 + q1);
        topc_lse_add(t, m, ssum);
        const float key = t == t ? t : -__builtin_inff();
        if (CR > 0) {
            // sorted insertion, from the last slot up: the new component (the highest index so far) goes in front of slot j when
            // its key is larger, or equal and the slot a placeholder; what it passes moves down one slot
            bool beat[CRN];
#pragma unroll
            for (int j = 0; j < CRN; j++) beat[j] = key > bv[j] || (key == bv[j] && bi[j] >= K);
#pragma unroll
            for (int j = CRN - 1; j >= 0; j--) {
                const bool above = j > 0 && beat[j > 0 ? j - 1 : 0];
                const float nv = above ? bv[j > 0 ? j - 1 : 0] : key;
                const int ni = above ? bi[j > 0 ? j - 1 : 0] : k;
                bv[j] = beat[j] ? nv : bv[j];
                bi[j] = beat[j] ? ni : bi[j];
            }
        } else if (live) {
            keys[(int64_t)k * nf + f] = key;
        }
    }
    if (!live) return;
    ll_bg[f] = LSE_LN2 * (m + log2f(ssum));
    if (CR > 0) {
#pragma unroll
        for (int j = 0; j < CRN; j++)
            if (j < C) sel[(int64_t)f * C + j] = bi[j];
    }
}

// C above the register slots: component k of frame f goes to slot rank(k) = the number of components in front of it
// (larger key, or equal key and lower index) when that is below C.  A workgroup per frame, the K keys in LDS.
__global__ __launch_bounds__(TOPC_WG)
void topc_rank_kernel(const float *__restrict__ keys, int nf, int K, int C, int *__restrict__ sel) {
    extern __shared__ float sk[];
    const int f = blockIdx.x;
    for (int k = threadIdx.x; k < K; k += TOPC_WG) sk[k] = keys[(int64_t)k * nf + f];
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += TOPC_WG) {
        const float a = sk[k];
        int rank = 0;
        for (int j = 0; j < K; j++) {
            const float b = sk[j];
            rank += (b > a || (b == a && j < k)) ? 1 : 0;
        }
        if (rank < C) sel[(int64_t)f * C + rank] = k;
    }
}

// ---- 2. route ----

__global__ __launch_bounds__(TOPC_WG)
void topc_hist_kernel(const int *__restrict__ sel, int n_pairs, int K, int *__restrict__ count) {
    const int i = blockIdx.x * TOPC_WG + threadIdx.x;
    if (i >= n_pairs) return;
    const int k = sel[i];
    if ((unsigned)k < (unsigned)K) atomicAdd(&count[k], 1);
}

// exclusive sums over the K components of their entries (start, and cursor = start for the scatter) and of their runs of `run`
// entries (run_start); one workgroup, a contiguous stretch of components per lane
__global__ __launch_bounds__(TOPC_WG)
void topc_scan_kernel(const int *__restrict__ count, int K, int run, int *__restrict__ start, int *__restrict__ run_start,
                      int *__restrict__ cursor) {
    __shared__ int se[TOPC_WG], sr_[TOPC_WG];
    const int tid = threadIdx.x;
    const int per = (K + TOPC_WG - 1) / TOPC_WG;
    const int b = min(tid * per, K), e = min(b + per, K);
    int ne = 0, nr = 0;
    for (int k = b; k < e; k++) {
        ne += count[k];
        nr += (count[k] + run - 1) / run;
    }
    se[tid] = ne;
    sr_[tid] = nr;
    __syncthreads();
    for (int d = 1; d < TOPC_WG; d <<= 1) {
        const int a = tid >= d ? se[tid - d] : 0, c = tid >= d ? sr_[tid - d] : 0;
        __syncthreads();
        se[tid] += a;
        sr_[tid] += c;
        __syncthreads();
    }
    int pe = se[tid] - ne, pr = sr_[tid] - nr;
    for (int k = b; k < e; k++) {
        start[k] = pe;
        cursor[k] = pe;
        run_start[k] = pr;
        pe += count[k];
        pr += (count[k] + run - 1) / run;
    }
    if (tid == TOPC_WG - 1) {
        start[K] = se[tid];
        run_start[K] = sr_[tid];
    }
}

__global__ __launch_bounds__(TOPC_WG)
void topc_scatter_kernel(const int *__restrict__ sel, int n_pairs, int K, int *__restrict__ cursor, int *__restrict__ list) {
    const int i = blockIdx.x * TOPC_WG + threadIdx.x;
    if (i >= n_pairs) return;
    const int k = sel[i];
    if ((unsigned)k >= (unsigned)K) return;
    const int pos = atomicAdd(&cursor[k], 1);
    if (pos < n_pairs) list[pos] = i;           // the pair IS its index: frame of the chunk * C + slot
}

// ---- 3. evaluate ----

template <int TP>
__global__ __launch_bounds__(256)
void topc_eval_kernel(const float *__restrict__ X, int D, int64_t f0, const float *__restrict__ scale, const float *__restrict__ center,
                      const float *__restrict__ mtab, const float *__restrict__ cst, int K, int S, int C, int run,
                      const int *__restrict__ start, const int *__restrict__ run_start, const int *__restrict__ list,
                      float *__restrict__ terms) {
    __shared__ __attribute__((aligned(16))) float xs[TOPC_STAGE * TP];
    __shared__ int pr[TOPC_STAGE];
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int unit = blockIdx.x;
    if (unit >= run_start[K]) return;            // the grid is an upper bound of the runs
    int lo = 0, hi = K;                          // run_start[lo] <= unit < run_start[hi]; components without entries have no run
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (run_start[mid] <= unit) lo = mid; else hi = mid;
    }
    const int k = lo;
    const int e0 = start[k] + (unit - run_start[k]) * run;
    const int e1 = min(start[k + 1], e0 + run);
    const int s = blockIdx.y * nthreads + tid;
    const bool live = s < S;
    float m[TP];
#pragma unroll
    for (int d = 0; d < TP; d++) m[d] = live ? mtab[((int64_t)k * TP + d) * S + s] : 0.0f;
    const float c = cst[k];
    const float *__restrict__ sc = scale + (int64_t)k * TP;
    for (int st = e0; st < e1; st += TOPC_STAGE) {
        const int ne = min(TOPC_STAGE, e1 - st);
        __syncthreads();                         // the last stage's readers are done
        if (tid < ne) pr[tid] = list[st + tid];
        __syncthreads();
        for (int i = tid; i < ne * TP; i += nthreads) {
            const int e = i / TP, d = i - e * TP;
            const int64_t frame = f0 + pr[e] / C;
            xs[i] = d < D ? (X[frame * D + d] - center[d]) * sc[d] : 0.0f;
        }
        __syncthreads();
        for (int e = 0; e < ne; e++) {
            const float4 *xv = reinterpret_cast<const float4 *>(xs + e * TP);     // the same address in every lane: a broadcast
            float q0 = 0.0f, q1 = 0.0f;
#pragma unroll
            for (int d4 = 0; d4 < TP / 4; d4++) {
                const float4 v = xv[d4];
                const float z0 = v.x + m[4 * d4], z1 = v.y + m[4 * d4 + 1], z2 = v.z + m[4 * d4 + 2], z3 = v.w + m[4 * d4 + 3];
                q0 = fmaf(z0, z0, q0);
                q1 = fmaf(z1, z1, q1);
                q0 = fmaf(z2, z2, q0);
                q1 = fmaf(z3, z3, q1);
            }
            if (live) terms[(int64_t)pr[e] * S + s] = c - (q0 + q1);
        }
    }
}

// ---- 4. combine ----

__global__ __launch_bounds__(256)
void topc_combine_kernel(const float *__restrict__ terms, const float *__restrict__ ll_bg, const TileDesc *__restrict__ tiles, int tile0,
                         int64_t f0, int S, int C, int bg, int clamp, int64_t n_frames, double *__restrict__ partial,
                         float *__restrict__ frame_ll) {
    const int tile = tile0 + blockIdx.x;
    const TileDesc td = tiles[tile];
    for (int s = threadIdx.x; s < S; s += blockDim.x) {
        double acc = 0.0;
        for (int i = 0; i < td.count; i++) {
            const int64_t fl = td.start + i - f0;            // frame of the chunk
            float ll;
            if (s == bg) {
                ll = ll_bg[fl];
            } else {
                const float *__restrict__ t = terms + fl * C * S + s;
                float m = -3.0e38f, ssum = 0.0f;
                for (int j = 0; j < C; j++) topc_lse_add(t[(int64_t)j * S], m, ssum);
                ll = LSE_LN2 * (m + log2f(ssum));
            }
            if (clamp && ll < TOPC_LN_DBL_MIN) ll = LSE_LN_1E_15;
            acc += (double)ll;
            if (frame_ll) frame_ll[(int64_t)s * n_frames + td.start + i] = ll;
        }
        partial[(int64_t)tile * S + s] = acc;
    }
}

// ---- host ----

static std::atomic<long> &scratch_option() {
    static std::atomic<long> v{(long)(TOPC_DEFAULT_SCRATCH >> 20)};
    return v;
}
void set_topc_scratch_mib(long v) { scratch_option().store(v); }
long topc_scratch_mib() { return scratch_option().load(); }

namespace {
struct TopcScratch {
    DevBuf<float> terms, ll_bg, keys, frame_ll;
    DevBuf<int> sel, list, tables;          // tables: count [K], cursor [K], start [K + 1], run_start [K + 1]
    DevBuf<double> partial, results;
    TileTable tt;                           // tiles of <= TOPC_TILE frames that cross neither an utterance nor a chunk
    PinnedBuf<double> h_results;
};

// {s, m, c} of mixture k of model s in the vector layout (gmm_model.hpp: records of KB mixtures)
struct VecLayout {
    const PackedModels &pm;
    size_t rec_f4;
    explicit VecLayout(const PackedModels &p) : pm(p), rec_f4((size_t)2 * p.dp + 1) {}
    const float *rec(int s, int k) const {
        return pm.params.data() + ((size_t)pm.chunks[pm.model_chunk_begin[s]].offset_f4 + (size_t)(k / KB) * rec_f4) * 4;
    }
    float scale(int s, int k, int d) const { return rec(s, k)[(size_t)d * 8 + (size_t)(k % KB) * 2]; }
    float m(int s, int k, int d) const { return rec(s, k)[(size_t)d * 8 + (size_t)(k % KB) * 2 + 1]; }
    float c(int s, int k) const { return rec(s, k)[(size_t)2 * pm.dp * 4 + (k % KB)]; }
};
}  // namespace

// Do the set's models share sigma and weights with one another (or is there one model)?  Read off the packed vector layout:
// s and c are functions of sigma and the weights alone.
static bool topc_tied(const PackedModels &pm) {
    const int S = pm.n_models;
    if ((int)pm.model_mixtures.size() != S) return false;
    const int K = pm.model_mixtures[0];
    for (int s = 1; s < S; s++)
        if (pm.model_mixtures[s] != K) return false;
    const VecLayout v(pm);
    for (int s = 1; s < S; s++)
        for (int k = 0; k < K; k++) {
            const float a = v.c(0, k), b = v.c(s, k);
            if (std::memcmp(&a, &b, sizeof a) != 0) return false;
            for (int d = 0; d < pm.dim; d++) {
                const float x = v.scale(0, k, d), y = v.scale(s, k, d);
                if (std::memcmp(&x, &y, sizeof x) != 0) return false;
            }
        }
    return true;
}

// whether the set qualifies, without touching the device (the answer is kept)
bool topc_set_tied(SRModelSet &set) {
    if (set.topc_state == 0) set.topc_state = topc_tied(set.host) ? 2 : -1;
    return set.topc_state > 0;
}

static void ensure_topc_tables(SRModelSet &set, int tp) {
    if (set.topc_state == 1 && set.topc_tp == tp) return;
    const PackedModels &pm = set.host;
    const int S = pm.n_models, K = pm.model_mixtures[0], D = pm.dim;
    const VecLayout v(pm);
    std::vector<float> scale((size_t)K * tp + tp, 0.0f), mt((size_t)K * tp * S, 0.0f), cst((size_t)K);
    for (int k = 0; k < K; k++) {
        cst[k] = v.c(0, k);
        for (int d = 0; d < D; d++) {
            scale[(size_t)k * tp + d] = v.scale(0, k, d);
            float *dst = mt.data() + ((size_t)k * tp + d) * S;
            for (int s = 0; s < S; s++) dst[s] = v.m(s, k, d);
        }
    }
    for (int d = 0; d < D; d++) scale[(size_t)K * tp + d] = pm.center[d];      // the centre rides behind the scales
    set.d_topc_scale.upload(scale.data(), scale.size());
    set.d_topc_m.upload(mt.data(), mt.size());
    set.d_topc_c.upload(cst.data(), cst.size());
    set.d_topc_bg.ensure((size_t)K * tp * 2);
    sync_stream();
    set.topc_state = 1;
    set.topc_tp = tp;
    set.topc_k = K;
    set.topc_bg = -1;
}

template <int TP>
static void launch_select(int cr, dim3 grid, hipStream_t st, const float *X, int D, int64_t f0, int nf, const float2 *bg, const float *cst,
                          const float *center, int K, int C, float *ll_bg, int *sel, float *keys) {
    switch (cr) {
    case 1: hipLaunchKernelGGL((topc_select_kernel<TP, 1>), grid, dim3(TOPC_WG), 0, st, X, D, f0, nf, bg, cst, center, K, C, ll_bg, sel, keys); break;
    case 5: hipLaunchKernelGGL((topc_select_kernel<TP, 5>), grid, dim3(TOPC_WG), 0, st, X, D, f0, nf, bg, cst, center, K, C, ll_bg, sel, keys); break;
    case 8: hipLaunchKernelGGL((topc_select_kernel<TP, 8>), grid, dim3(TOPC_WG), 0, st, X, D, f0, nf, bg, cst, center, K, C, ll_bg, sel, keys); break;
    default: hipLaunchKernelGGL((topc_select_kernel<TP, 0>), grid, dim3(TOPC_WG), 0, st, X, D, f0, nf, bg, cst, center, K, C, ll_bg, sel, keys); break;
    }
}

void score_batch_set_topc(SRModelSet &set, SRBatch &feat, int bg, int top_c, double *sums_out, int *argmax_out, int *topc_out,
                          float *frame_ll_out, int flags) {
    // every refusal before the device is touched
    const int S = set.host.n_models, D = set.host.dim;
    const int K = set.host.model_mixtures.empty() ? 0 : set.host.model_mixtures[0];
    std::string why;
    if (!topc_check(feat.kind != SRBatch::FEATURES || topc_set_tied(set), S, K, D, bg, top_c, feat.kind == SRBatch::FEATURES, why))
        fail("%s", why.c_str());
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_score_batch_set_topc");
    ensure_device();
    feat.bind_device();
    if (set.device != ctx().device) fail("model set lives on device %d, the calling thread is on device %d", set.device, ctx().device);
    if (feat.dim != D) fail("feature dim %d != model dim %d", feat.dim, D);
    const int64_t n = feat.n_rows;
    const int U = feat.n_utt, C = top_c;
    TopcPlan pl;
    if (!plan_topc(K, D, S, C, n, (int64_t)topc_scratch_mib() << 20, ctx().n_cu, pl, why)) fail("%s", why.c_str());
    ensure_topc_tables(set, pl.tp);
    hipStream_t st = ctx().stream;
    const float *center = set.d_topc_scale.p + (size_t)K * pl.tp;
    if (set.topc_bg != bg) {
        const int nb = K * pl.tp;
        hipLaunchKernelGGL(topc_gather_bg_kernel, dim3((nb + TOPC_WG - 1) / TOPC_WG), dim3(TOPC_WG), 0, st, set.d_topc_scale.p, set.d_topc_m.p,
                           nb, S, bg, reinterpret_cast<float2 *>(set.d_topc_bg.p));
        SR_HIP(hipGetLastError());
        set.topc_bg = bg;
    }

    // tiles: every utterance cut at TOPC_TILE frames and at the chunk boundaries (multiples of pl.chunk from frame 0)
    auto &w = per_device<TopcScratch>();
    std::vector<TileDesc> tiles;
    std::vector<int> begin((size_t)U + 1, 0);
    for (int u = 0; u < U; u++) {
        begin[u] = (int)tiles.size();
        for (int64_t s0 = feat.offsets[u]; s0 < feat.offsets[u + 1];) {
            const int64_t chunk_end = (s0 / pl.chunk + 1) * pl.chunk;
            const int64_t e = std::min(std::min(s0 + TOPC_TILE, feat.offsets[u + 1]), chunk_end);
            tiles.push_back(TileDesc{s0, (int32_t)(e - s0), u});
            s0 = e;
        }
    }
    begin[U] = (int)tiles.size();
    const int n_tiles = (int)tiles.size();
    w.tt.frames_per_tile = TOPC_TILE;
    w.tt.n_tiles = n_tiles;
    w.tt.d_tiles.upload(tiles.data(), tiles.size());
    w.tt.d_utt_tile_begin.upload(begin.data(), begin.size());

    const int64_t cf = pl.chunk;                // frames of a full chunk
    w.terms.ensure((size_t)std::max<int64_t>(1, cf * C * S));
    w.ll_bg.ensure((size_t)std::max<int64_t>(1, cf));
    w.sel.ensure((size_t)std::max<int64_t>(1, cf * C));
    w.list.ensure((size_t)std::max<int64_t>(1, cf * C));
    if (pl.cr == 0) w.keys.ensure((size_t)std::max<int64_t>(1, cf * K));
    w.tables.ensure((size_t)4 * K + 2);
    w.partial.ensure((size_t)std::max(1, n_tiles) * S);
    w.results.ensure((size_t)U * S + ((size_t)U + 1) / 2 + 1);
    float *fll = nullptr;
    if (frame_ll_out && n > 0) {
        w.frame_ll.ensure((size_t)S * n);
        fll = w.frame_ll.p;
    }
    int *count = w.tables.p, *cursor = count + K, *start = cursor + K, *run_start = start + K + 1;

    size_t tile_at = 0;
    for (int64_t ch = 0; ch < pl.n_chunks; ch++) {
        const int64_t f0 = ch * cf;
        const int nf = (int)std::min<int64_t>(cf, n - f0);
        const int n_pairs = nf * C;
        const dim3 g_frames((unsigned)((nf + TOPC_WG - 1) / TOPC_WG)), g_pairs((unsigned)((n_pairs + TOPC_WG - 1) / TOPC_WG));
        SR_HIP(hipMemsetAsync(count, 0, (size_t)K * sizeof(int), st));
        {
            ScopedKernelTimer t(T_TOPC_SELECT);
            const float2 *bgp = reinterpret_cast<const float2 *>(set.d_topc_bg.p);
            if (pl.tp == 16) launch_select<16>(pl.cr, g_frames, st, feat.data.p, D, f0, nf, bgp, set.d_topc_c.p, center, K, C, w.ll_bg.p, w.sel.p, w.keys.p);
            else if (pl.tp == 40) launch_select<40>(pl.cr, g_frames, st, feat.data.p, D, f0, nf, bgp, set.d_topc_c.p, center, K, C, w.ll_bg.p, w.sel.p, w.keys.p);
            else launch_select<64>(pl.cr, g_frames, st, feat.data.p, D, f0, nf, bgp, set.d_topc_c.p, center, K, C, w.ll_bg.p, w.sel.p, w.keys.p);
            if (pl.cr == 0)
                hipLaunchKernelGGL(topc_rank_kernel, dim3((unsigned)nf), dim3(TOPC_WG), (size_t)pl.rank_lds, st, w.keys.p, nf, K, C, w.sel.p);
            SR_HIP(hipGetLastError());
        }
        if (topc_out) SR_HIP(hipMemcpyAsync(topc_out + f0 * C, w.sel.p, (size_t)n_pairs * sizeof(int), hipMemcpyDeviceToHost, st));
        {
            ScopedKernelTimer t(T_TOPC_ROUTE);
            hipLaunchKernelGGL(topc_hist_kernel, g_pairs, dim3(TOPC_WG), 0, st, w.sel.p, n_pairs, K, count);
            hipLaunchKernelGGL(topc_scan_kernel, dim3(1), dim3(TOPC_WG), 0, st, count, K, pl.run, start, run_start, cursor);
            hipLaunchKernelGGL(topc_scatter_kernel, g_pairs, dim3(TOPC_WG), 0, st, w.sel.p, n_pairs, K, cursor, w.list.p);
            SR_HIP(hipGetLastError());
        }
        {
            ScopedKernelTimer t(T_TOPC_EVAL);
            const dim3 grid((unsigned)((n_pairs + pl.run - 1) / pl.run + K), (unsigned)pl.eval_grid_y), wg((unsigned)(64 * pl.eval_waves));
            if (pl.tp == 16)
                hipLaunchKernelGGL(topc_eval_kernel<16>, grid, wg, 0, st, feat.data.p, D, f0, set.d_topc_scale.p, center, set.d_topc_m.p,
                                   set.d_topc_c.p, K, S, C, pl.run, start, run_start, w.list.p, w.terms.p);
            else if (pl.tp == 40)
                hipLaunchKernelGGL(topc_eval_kernel<40>, grid, wg, 0, st, feat.data.p, D, f0, set.d_topc_scale.p, center, set.d_topc_m.p,
                                   set.d_topc_c.p, K, S, C, pl.run, start, run_start, w.list.p, w.terms.p);
            else
                hipLaunchKernelGGL(topc_eval_kernel<64>, grid, wg, 0, st, feat.data.p, D, f0, set.d_topc_scale.p, center, set.d_topc_m.p,
                                   set.d_topc_c.p, K, S, C, pl.run, start, run_start, w.list.p, w.terms.p);
            SR_HIP(hipGetLastError());
        }
        size_t tile_end = tile_at;
        while (tile_end < tiles.size() && tiles[tile_end].start < f0 + nf) tile_end++;
        if (tile_end > tile_at) {
            ScopedKernelTimer t(T_TOPC_COMBINE);
            hipLaunchKernelGGL(topc_combine_kernel, dim3((unsigned)(tile_end - tile_at)), dim3((unsigned)pl.combine_wg), 0, st, w.terms.p,
                               w.ll_bg.p, w.tt.d_tiles.p, (int)tile_at, f0, S, C, bg, flags & 1, n, w.partial.p, fll);
            SR_HIP(hipGetLastError());
        }
        tile_at = tile_end;
    }
    double *d_sums = w.results.p;
    int *d_argmax = reinterpret_cast<int *>(w.results.p + (size_t)U * S);
    if (U > 0) {
        ScopedKernelTimer t(T_FINALIZE);
        launch_finalize(w.partial.p, w.tt, U, S, 1, d_sums, d_argmax, nullptr, nullptr, 0, FinalizeDelivery{nullptr, nullptr, 0, 0u});
        SR_HIP(hipGetLastError());
        const size_t nd = (size_t)U * S + ((size_t)U + 1) / 2;
        w.h_results.ensure(nd);
        SR_HIP(hipMemcpyAsync(w.h_results.p, w.results.p, results_bytes((size_t)U, (size_t)S), hipMemcpyDeviceToHost, st));
    }
    if (fll) SR_HIP(hipMemcpyAsync(frame_ll_out, fll, (size_t)S * n * sizeof(float), hipMemcpyDeviceToHost, st));
    sync_stream();
    if (U > 0) {
        if (sums_out) std::memcpy(sums_out, w.h_results.p, (size_t)U * S * sizeof(double));
        if (argmax_out) std::memcpy(argmax_out, w.h_results.p + (size_t)U * S, (size_t)U * sizeof(int));
    }
}

}  // namespace sr
