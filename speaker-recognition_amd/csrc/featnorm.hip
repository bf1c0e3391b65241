// featnorm.hip -- short-time feature normalisation of every utterance of an fp32 feature batch, the result a new feature batch on
// the same device: feature warping (Pelecanos & Sridharan 2001) and sliding-window mean / mean-and-variance normalisation (what
// Kaldi's apply-cmvn-sliding does with a centred window).  Each utterance on its own, each column on its own.
//
// An utterance of T frames, W the window: frame t looks at the N = min(W, T) rows from s0(t) = min(max(t - W / 2, 0), T - N).
//   warp:  less = values of the window < x_t, eq = values == x_t (fp32 comparisons, the frame itself among them);
//          r2 = 2 less + eq - 1, out = (float) quantile((r2 + 1) / (2 N))  (norm_quantile.hpp: AS241, float64, taken through the
//          lower half so that mirrored ranks give negated values to the bit).  A NaN cell: rank -1, NaN out, counted.
//   cmn:   mean = (sum x) / N in float64, summed in window order; out = (float)(x_t - mean).
//   cmvn:  var = (sum (x - mean)^2) / N, the second pass in window order too; out = (float)((x_t - mean) / sqrt(var)).  A window
//          whose values all compare equal gives exactly 0 and is counted (decided by comparisons, not from the variance).
//
// One kernel.  A workgroup takes a tile: F consecutive frames of one utterance.  It stages the rows its frames' windows cover --
// [s0(first), s0(last) + N), at most F + N - 1 -- transposed into LDS, [column][row], `cols` columns per pass (coalesced row-major
// reads; the column stride is 4 x an odd number of floats, so a column starts on 16 bytes and the transposed writes spread over the
// banks).  A wave then takes 64 consecutive frames of one column, a lane per frame.  The 64 windows overlap in all but their
// fringes, so the wave walks their union once: every lane reads the same four values (one 16-byte broadcast read), the stretch
// common to all 64 windows needs no test, and only the two fringes are masked by index.  Sums are formed lane by lane in window
// order (a masked term adds +0.0, which changes no partial sum that started at +0.0), so a frame's result does not depend on the
// tile it falls into, the batch around it or the run.  No atomics: a wave leaves its count of degenerate cells beside its tile,
// featnorm_count_kernel adds an utterance's up in order.  The decisions -- F, the rows and columns staged, the table -- are
// plan_feature_norm's (featnorm_plan.cpp).

// the sums, the polynomial chains and the float64 passes are stated operation by operation: nothing is fused
#pragma clang fp contract(off)

#include "batch.hpp"
#include "featnorm.hpp"
#include "featnorm_plan.hpp"
#include "norm_quantile.hpp"

#include <algorithm>
#include <atomic>
#include <vector>

namespace sr {

constexpr int FEATNORM_WAVES = FEATNORM_WG / FEATNORM_WAVE;

struct FeatNormArgs {
    const float *x;             // [rows][dim]
    float *y;                   // [rows][dim]
    int32_t *ranks;             // [rows][dim] or null (warp)
    const int64_t *off;         // [U + 1] row offsets of the batch
    const int32_t *tile_utt;    // [n_tiles]
    const int32_t *tile_k;      // [n_tiles] the tile's index inside its utterance
    int32_t *wave_count;        // [n_tiles][FEATNORM_WAVES]
    const float *table;         // [2 W - 1] warped values of a full window, or null
    int64_t n_tiles;
    int W, dim, F, stride, cols;
};

__device__ __forceinline__ int64_t window_start(int64_t t, int64_t T, int W, int N) {
    return min(max(t - W / 2, (int64_t)0), T - (int64_t)N);
}

// The union of a wave's windows, in chunks of four values: chunks [k0, k1) and [k2, k3) hold values outside some lane's window
// (`m` gets the index), chunks [k1, k2) lie inside every lane's (`u` needs none).
template <typename FM, typename FU>
__device__ __forceinline__ void walk(const float *__restrict__ col, int k0, int k1, int k2, int k3, FM &&m, FU &&u) {
    for (int k = k0; k < k1; k++) {
        const float4 v = *reinterpret_cast<const float4 *>(col + 4 * k);
        m(4 * k, v.x); m(4 * k + 1, v.y); m(4 * k + 2, v.z); m(4 * k + 3, v.w);
    }
#pragma unroll 2
    for (int k = k1; k < k2; k++) {
        const float4 v = *reinterpret_cast<const float4 *>(col + 4 * k);
        u(v.x); u(v.y); u(v.z); u(v.w);
    }
    for (int k = k2; k < k3; k++) {
        const float4 v = *reinterpret_cast<const float4 *>(col + 4 * k);
        m(4 * k, v.x); m(4 * k + 1, v.y); m(4 * k + 2, v.z); m(4 * k + 3, v.w);
    }
}

template <int MODE>
__global__ __launch_bounds__(FEATNORM_WG)
void featnorm_kernel(FeatNormArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x % FEATNORM_WAVE, wave = threadIdx.x / FEATNORM_WAVE;
    for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int u = a.tile_utt[tile];
        const int64_t row0 = a.off[u], T = a.off[u + 1] - row0;
        const int64_t f0 = (int64_t)a.tile_k[tile] * a.F;
        const int N = (int)min((int64_t)a.W, T);
        const int Fc = (int)min((int64_t)a.F, T - f0);
        int count = 0;
        const int64_t b = Fc > 0 ? window_start(f0, T, a.W, N) : 0;
        const int span = Fc > 0 ? (int)(window_start(f0 + Fc - 1, T, a.W, N) + N - b) : 0;
        // (the plan sized the columns for the longest utterance's tiles: a tile that would not fit them is left alone)
        const bool fits = Fc > 0 && span <= a.stride && b + span <= T;
        const int n_groups = fits ? (Fc + FEATNORM_WAVE - 1) / FEATNORM_WAVE : 0;
        for (int c0 = 0; c0 < a.dim && fits; c0 += a.cols) {
            const int Cc = min(a.cols, a.dim - c0);
            __syncthreads();                        // the pass before is read out
            const float *__restrict__ src = a.x + (row0 + b) * a.dim + c0;
            // element i = r Cc + c of the staged block, i = lane, lane + 256, ..: one division per pass, then steps
            const int dr = FEATNORM_WG / Cc, dc = FEATNORM_WG - dr * Cc;
            for (int r = (int)threadIdx.x / Cc, c = (int)threadIdx.x - r * Cc; r < span;) {
                lds[c * a.stride + r] = src[(int64_t)r * a.dim + c];
                r += dr;
                c += dc;
                if (c >= Cc) {
                    c -= Cc;
                    r++;
                }
            }
            __syncthreads();
            for (int item = wave; item < Cc * n_groups; item += FEATNORM_WAVES) {
                const int c = item / n_groups, g = item - c * n_groups;
                const bool valid = g * FEATNORM_WAVE + lane < Fc;
                const int64_t t = f0 + min(g * FEATNORM_WAVE + lane, Fc - 1);       // (lanes past the tile repeat its last frame)
                const int at = (int)(window_start(t, T, a.W, N) - b);
                const float *__restrict__ col = lds + c * a.stride;
                const float x = col[(int)(t - b)];
                // the union [lo, hi) of the wave's windows and the stretch [cl, ch) common to all of them
                const int lo = __builtin_amdgcn_readfirstlane(at), a_last = __builtin_amdgcn_readlane(at, FEATNORM_WAVE - 1);
                const int hi = a_last + N, cl = a_last, ch = lo + N;
                const int k0 = lo / 4, k3 = (hi + 3) / 4;
                int k1 = (cl + 3) / 4, k2 = ch / 4;
                if (k1 >= k2) k1 = k2 = k3;
                const unsigned un = (unsigned)N;
                float out;
                bool flagged = false;
                if (MODE == FEATNORM_WARP) {
                    int less = 0, eq = 0;
                    walk(col, k0, k1, k2, k3,
                         [&](int j, float v) {
                             const bool in = (unsigned)(j - at) < un;
                             less += (in && v < x) ? 1 : 0;
                             eq += (in && v == x) ? 1 : 0;
                         },
                         [&](float v) {
                             less += v < x ? 1 : 0;
                             eq += v == x ? 1 : 0;
                         });
                    const int r2 = 2 * less + eq - 1;
                    flagged = r2 < 0;                   // a NaN cell: nothing is below it, nothing equals it
                    if (flagged)
                        out = __builtin_nanf("");
                    else if (a.table && N == a.W)
                        out = a.table[r2];
                    else
                        out = (float)warp_value(r2, N);
                    if (a.ranks && valid) a.ranks[(row0 + t) * a.dim + c0 + c] = r2;
                } else {
                    const float first = col[at];
                    double sum = 0.0;
                    bool alleq = true;
                    walk(col, k0, k1, k2, k3,
                         [&](int j, float v) {
                             const bool in = (unsigned)(j - at) < un;
                             sum += in ? (double)v : 0.0;
                             alleq = alleq && (!in || v == first);
                         },
                         [&](float v) {
                             sum += (double)v;
                             alleq = alleq && v == first;
                         });
                    const double mean = sum / (double)N;
                    if (MODE == FEATNORM_CMN) {
                        out = (float)((double)x - mean);
                    } else {
                        flagged = alleq;
                        double acc = 0.0;
                        if (!__all(alleq)) {
                            walk(col, k0, k1, k2, k3,
                                 [&](int j, float v) {
                                     const bool in = (unsigned)(j - at) < un;
                                     const double d = (double)v - mean;
                                     acc += in ? d * d : 0.0;
                                 },
                                 [&](float v) {
                                     const double d = (double)v - mean;
                                     acc += d * d;
                                 });
                        }
                        const double var = acc / (double)N;
                        out = alleq ? 0.0f : (float)(((double)x - mean) / sqrt(var));
                    }
                }
                if (valid) a.y[(row0 + t) * a.dim + c0 + c] = out;
                count += __popcll(__ballot(valid && flagged));
            }
        }
        if (lane == 0) a.wave_count[tile * FEATNORM_WAVES + wave] = count;
    }
}

// table[r2] = the warped value of the doubled mid-rank r2 in a full window: the function the kernel evaluates, evaluated once
__global__ __launch_bounds__(FEATNORM_WG)
void featnorm_table_kernel(int W, float *__restrict__ table) {
    const int r2 = blockIdx.x * FEATNORM_WG + threadIdx.x;
    if (r2 < 2 * W - 1) table[r2] = (float)warp_value(r2, W);
}

// an utterance's count: its tiles' waves, in order
__global__ __launch_bounds__(FEATNORM_WG)
void featnorm_count_kernel(int U, const int64_t *__restrict__ utt_tile, const int32_t *__restrict__ wave_count, int64_t *__restrict__ out) {
    const int u = blockIdx.x * FEATNORM_WG + threadIdx.x;
    if (u >= U) return;
    int64_t s = 0;
    for (int64_t i = utt_tile[u] * FEATNORM_WAVES; i < utt_tile[u + 1] * FEATNORM_WAVES; i++) s += wave_count[i];
    out[u] = s;
}

// ---- host ----

static std::atomic<long> &tile_option() {
    static std::atomic<long> v{0};
    return v;
}
void set_feature_norm_tile(long v) { tile_option().store(v); }
long feature_norm_tile() { return tile_option().load(); }

namespace {
struct FeatNormScratch {
    DevBuf<int32_t> tiles;          // tile_utt [n_tiles], tile_k [n_tiles]
    DevBuf<int64_t> utt_tile;       // [U + 1]
    DevBuf<int32_t> wave_count, ranks;
    DevBuf<int64_t> counts;
    DevBuf<float> table;
    int table_W = 0;                // the window the table holds
    PinnedBuf<int64_t> h_counts;
};
}  // namespace

void feature_norm_batch(SRBatch &in, int mode, int window, SRBatch &out, int64_t *degenerate_out, int32_t *ranks_out) {
    // every refusal first: nothing of the device is touched for a call that cannot run
    const int U = in.n_utt;
    int64_t max_frames = 0;
    if (in.kind == SRBatch::FEATURES)
        for (int u = 0; u < U; u++) max_frames = std::max(max_frames, in.offsets[u + 1] - in.offsets[u]);
    FeatNormPlan pl;
    std::string why;
    if (!plan_feature_norm(mode, window, in.kind == SRBatch::FEATURES, in.dim, max_frames, feature_norm_tile(), 1, pl, why))
        fail("sr_feature_norm_batch: %s", why.c_str());
    if (ranks_out && mode != FEATNORM_WARP) fail("sr_feature_norm_batch: ranks are what feature warping computes (mode 0)");
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_feature_norm_batch");
    ensure_device();
    in.bind_device();
    out.bind_device();
    if (!plan_feature_norm(mode, window, true, in.dim, max_frames, feature_norm_tile(), ctx().n_cu, pl, why))
        fail("sr_feature_norm_batch: %s", why.c_str());

    const int dim = in.dim;
    std::vector<int64_t> utt_tile((size_t)U + 1, 0);
    for (int u = 0; u < U; u++) utt_tile[u + 1] = utt_tile[u] + featnorm_tiles(in.offsets[u + 1] - in.offsets[u], pl.F);
    const int64_t n_tiles = utt_tile[U];
    if (n_tiles > INT32_MAX / FEATNORM_WAVES) fail("sr_feature_norm_batch: %lld tiles", (long long)n_tiles);
    std::vector<int32_t> tiles(2 * (size_t)n_tiles);
    for (int u = 0; u < U; u++)
        for (int64_t k = 0; k < utt_tile[u + 1] - utt_tile[u]; k++) {
            tiles[(size_t)(utt_tile[u] + k)] = u;
            tiles[(size_t)(n_tiles + utt_tile[u] + k)] = (int32_t)k;
        }

    out.kind = SRBatch::FEATURES;
    out.n_utt = U;
    out.dim = dim;
    out.n_rows = in.n_rows;
    out.offsets = in.offsets;
    out.d_offsets.upload(out.offsets.data(), out.offsets.size());
    out.data.ensure((size_t)std::max<int64_t>(1, in.n_rows * dim));
    out.invalidate_tiles();

    auto &w = per_device<FeatNormScratch>();
    hipStream_t st = ctx().stream;
    w.h_counts.ensure((size_t)std::max(1, U));
    if (n_tiles > 0) {
        w.tiles.upload(tiles.data(), tiles.size());
        w.utt_tile.upload(utt_tile.data(), utt_tile.size());
        w.wave_count.ensure((size_t)n_tiles * FEATNORM_WAVES);
        w.counts.ensure((size_t)U);
        if (ranks_out) w.ranks.ensure((size_t)(in.n_rows * dim));

        FeatNormArgs a;
        a.x = in.data.p;
        a.y = out.data.p;
        a.ranks = ranks_out ? w.ranks.p : nullptr;
        a.off = in.d_offsets.p;
        a.tile_utt = w.tiles.p;
        a.tile_k = w.tiles.p + n_tiles;
        a.wave_count = w.wave_count.p;
        a.table = nullptr;
        a.n_tiles = n_tiles;
        a.W = window; a.dim = dim; a.F = pl.F; a.stride = pl.stride; a.cols = pl.cols;

        ScopedKernelTimer tm(T_CMVN);
        if (pl.table) {
            if (w.table_W != window) {
                w.table.ensure((size_t)pl.table_len);
                hipLaunchKernelGGL(featnorm_table_kernel, dim3((pl.table_len + FEATNORM_WG - 1) / FEATNORM_WG), dim3(FEATNORM_WG), 0, st, window,
                                   w.table.p);
                w.table_W = window;
            }
            a.table = w.table.p;
        }
        const dim3 grid(featnorm_grid(n_tiles, ctx().n_cu)), wg(FEATNORM_WG);
        if (mode == FEATNORM_WARP)
            hipLaunchKernelGGL(featnorm_kernel<FEATNORM_WARP>, grid, wg, pl.lds_bytes, st, a);
        else if (mode == FEATNORM_CMN)
            hipLaunchKernelGGL(featnorm_kernel<FEATNORM_CMN>, grid, wg, pl.lds_bytes, st, a);
        else
            hipLaunchKernelGGL(featnorm_kernel<FEATNORM_CMVN>, grid, wg, pl.lds_bytes, st, a);
        hipLaunchKernelGGL(featnorm_count_kernel, dim3((U + FEATNORM_WG - 1) / FEATNORM_WG), dim3(FEATNORM_WG), 0, st, U, w.utt_tile.p,
                           w.wave_count.p, w.counts.p);
        SR_HIP(hipGetLastError());
        SR_HIP(hipMemcpyAsync(w.h_counts.p, w.counts.p, (size_t)U * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        if (ranks_out) w.ranks.download(ranks_out, (size_t)(in.n_rows * dim));
    }
    sync_stream();
    if (degenerate_out)
        for (int u = 0; u < U; u++) degenerate_out[u] = n_tiles > 0 ? w.h_counts.p[u] : 0;
}

}  // namespace sr
