// silence.hip -- the reference's energy-threshold silence removal (src/filters/silence.py:11-50: what its corpus preparation
// applies to every recording) on every utterance of an int16 PCM batch, the result a new PCM batch on the same device.
//
// One signal of n samples, L = int(frame_duration * fs), S = int(frame_shift * fs):
//   A = (sum x^2) / float(n);  walk i from 0 while i < n:  the frame is x[i : i + L] clipped at n, len samples,
//   e = (sum frame^2) / float(len);  e < A * perc (strict, float64): silent, i += L;  else the frame's first min(S, len) samples
//   go to the output and i += S.
// The sums are exact integers (int16^2 in int64); a decision is three float64 operations on them -- int64 -> double, one IEEE
// division, one multiply for the threshold -- and the kernels below perform exactly those (no fast-math, nothing to contract).
//
// Every i the walk visits is a multiple of g = gcd(L, S): "position" p stands for the sample p g.  The stages:
//   1. silence_chunk_kernel: the sum of squares of every position's g samples (the last position of an utterance holds fewer),
//      then an inclusive scan over ALL positions of the batch (silence_scan_*: tiles of 2048, the tile totals, the add) -- a
//      frame's energy is pre[min(p + L/g, P)] - pre[p], an utterance's the difference over its positions; differences never
//      cross an utterance, so the scan needs no segments.
//   2. The walk next(p) = p + (silent(p) ? L/g : S/g) is serial, but a jump is at most E = max(L, S) / g positions: the
//      positions are cut into blocks of B, and silence_maps_kernel computes for every block and each of the E offsets the walk
//      can enter it at the offset at which it enters the next block (a lane per (block, entry); an entry at or beyond B passes
//      through).  silence_chain_kernel then follows the maps: one table look-up per block and utterance, not one step per frame.
//   3. silence_mark_kernel walks every block again from its true entry and lists the kept frames and their samples; a scan over
//      the blocks' sample counts gives every block's place in the output and (silence_offsets_kernel) the U + 1 offsets of the
//      new batch; silence_copy_kernel moves the kept frames (32-bit copies where source, destination and lengths are even).
// The decisions -- g, E, B, the shape of the maps launch -- are plan_silence's (silence_plan.cpp).
#include "batch.hpp"
#include "silence.hpp"
#include "silence_plan.hpp"

#include <algorithm>
#include <atomic>
#include <vector>

namespace sr {

constexpr int SCAN_TILE = SILENCE_WG * SILENCE_SCAN_ITEMS;

struct SilenceArgs {
    const int64_t *off;       // [U + 1] sample offsets of the PCM batch
    const int64_t *pos_off;   // [U + 1] first position of every utterance
    const int64_t *blk_off;   // [U + 1] first block of every utterance
    const int64_t *pre;       // [positions + 1] sum of squares of all positions before
    int U;
    int64_t L, g, Lg, Sg, K, E, B, cap;
    double perc;
};

// tab[r] <= v < tab[r + 1], tab strictly increasing with tab[0] = 0 and v < tab[n]
__device__ __forceinline__ int find_segment(const int64_t *__restrict__ tab, int n, int64_t v) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

struct SilenceUtt {
    int64_t c0, P, s0, n;
    double thr;
};

__device__ __forceinline__ SilenceUtt load_utt(const SilenceArgs &a, int u) {
    SilenceUtt t;
    t.c0 = a.pos_off[u];
    t.P = a.pos_off[u + 1] - t.c0;
    t.s0 = a.off[u];
    t.n = a.off[u + 1] - t.s0;
    const int64_t total = a.pre[t.c0 + t.P] - a.pre[t.c0];
    const double A = (double)total / (double)t.n;      // silence.py:34
    t.thr = A * a.perc;                                // :40, the right-hand side
    return t;
}

__device__ __forceinline__ bool frame_silent(const SilenceArgs &a, const SilenceUtt &t, int64_t p) {
    const int64_t hi = min(p + a.Lg, t.P);
    const int64_t sum = a.pre[t.c0 + hi] - a.pre[t.c0 + p];
    const int64_t len = min(a.L, t.n - p * a.g);
    return (double)sum / (double)len < t.thr;          // silence.py:39-40
}

// ---- 1. energies ----

template <int LANES>
__global__ __launch_bounds__(SILENCE_WG)
void silence_chunk_kernel(const int16_t *__restrict__ pcm, SilenceArgs a, int64_t n_pos, int64_t *__restrict__ pre) {
    constexpr int PER_WG = SILENCE_WG / LANES;
    const int lane = threadIdx.x % LANES;
    for (int64_t w = blockIdx.x; w * PER_WG < n_pos; w += gridDim.x) {
        const int64_t c = w * PER_WG + threadIdx.x / LANES;
        int64_t acc = 0;
        if (c < n_pos) {
            const int u = find_segment(a.pos_off, a.U, c);
            const int64_t s = a.off[u] + (c - a.pos_off[u]) * a.g;
            const int64_t e = min(s + a.g, a.off[u + 1]);          // the ragged last position of an utterance
            for (int64_t i = s + lane; i < e; i += LANES) {
                const int v = pcm[i];
                acc += v * v;                                      // <= 2^30
            }
        }
        if (LANES == 64) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
        }
        if (c < n_pos && lane == 0) pre[c + 1] = acc;
        if (c == 0 && lane == 0) pre[0] = 0;
    }
}

// inclusive sums of s[0 .. 255] in place (Hillis-Steele over the workgroup)
__device__ __forceinline__ void block_scan_256(int64_t *s) {
    const int tid = threadIdx.x;
    __syncthreads();
    for (int d = 1; d < SILENCE_WG; d <<= 1) {
        const int64_t t = tid >= d ? s[tid - d] : 0;
        __syncthreads();
        s[tid] += t;
        __syncthreads();
    }
}

__global__ __launch_bounds__(SILENCE_WG)
void silence_scan_tiles_kernel(int64_t *__restrict__ v, int64_t n, int64_t *__restrict__ tile_tot) {
    __shared__ int64_t s[SILENCE_WG];
    const int tid = threadIdx.x;
    for (int64_t tile = blockIdx.x; tile * SCAN_TILE < n; tile += gridDim.x) {
        const int64_t base = tile * SCAN_TILE + (int64_t)tid * SILENCE_SCAN_ITEMS;
        int64_t x[SILENCE_SCAN_ITEMS], run = 0;
#pragma unroll
        for (int k = 0; k < SILENCE_SCAN_ITEMS; k++) {
            run += base + k < n ? v[base + k] : 0;
            x[k] = run;
        }
        s[tid] = run;
        block_scan_256(s);
        const int64_t before = s[tid] - run;
#pragma unroll
        for (int k = 0; k < SILENCE_SCAN_ITEMS; k++)
            if (base + k < n) v[base + k] = x[k] + before;
        if (tid == SILENCE_WG - 1) tile_tot[tile] = s[tid];
        __syncthreads();
    }
}

// exclusive sums of the tile totals in place: one workgroup, a contiguous stretch per lane
__global__ __launch_bounds__(SILENCE_WG)
void silence_scan_totals_kernel(int64_t *__restrict__ tot, int64_t n_tiles) {
    __shared__ int64_t s[SILENCE_WG];
    const int tid = threadIdx.x;
    const int64_t per = (n_tiles + SILENCE_WG - 1) / SILENCE_WG;
    const int64_t b = min(tid * per, n_tiles), e = min(b + per, n_tiles);
    int64_t sum = 0;
    for (int64_t i = b; i < e; i++) sum += tot[i];
    s[tid] = sum;
    block_scan_256(s);
    int64_t run = s[tid] - sum;
    for (int64_t i = b; i < e; i++) {
        const int64_t t = tot[i];
        tot[i] = run;
        run += t;
    }
}

__global__ __launch_bounds__(SILENCE_WG)
void silence_scan_add_kernel(int64_t *__restrict__ v, int64_t n, const int64_t *__restrict__ tile_before) {
    for (int64_t tile = blockIdx.x; tile * SCAN_TILE < n; tile += gridDim.x) {
        const int64_t add = tile_before[tile];
#pragma unroll
        for (int k = 0; k < SILENCE_SCAN_ITEMS; k++) {
            const int64_t i = tile * SCAN_TILE + k * SILENCE_WG + threadIdx.x;
            if (i < n) v[i] += add;
        }
    }
}

// ---- 2. the walk, block by block ----

// maps[blk][e]: the walk that enters block blk at offset e enters the next block at this offset; -1: never (it would be an
// offset no live walk holds).  The last block of an utterance has no next one: its row is never read.
__global__ __launch_bounds__(SILENCE_WG)
void silence_maps_kernel(SilenceArgs a, int64_t n_blocks, int bpw, int32_t *__restrict__ maps) {
    const int64_t items = (int64_t)bpw * a.E;
    for (int64_t w = blockIdx.x; w * bpw < n_blocks; w += gridDim.x) {
        for (int64_t item = threadIdx.x; item < items; item += SILENCE_WG) {
            const int64_t blk = w * bpw + item / a.E, e = item % a.E;
            if (blk >= n_blocks) continue;
            const int u = find_segment(a.blk_off, a.U, blk);
            const int64_t k = blk - a.blk_off[u];
            const SilenceUtt t = load_utt(a, u);
            int64_t p = k * a.B + e;
            const int64_t end = min((k + 1) * a.B, t.P);
            while (p < end) p += frame_silent(a, t, p) ? a.Lg : a.Sg;
            const int64_t x = p - (k + 1) * a.B;
            maps[blk * a.E + e] = (x >= 0 && x < a.E) ? (int32_t)x : -1;
        }
    }
}

// entry[blk]: the offset at which an utterance's walk enters the block, -1 once the walk is over
__global__ __launch_bounds__(64)
void silence_chain_kernel(SilenceArgs a, const int32_t *__restrict__ maps, int32_t *__restrict__ entry) {
    const int u = blockIdx.x * 64 + threadIdx.x;
    if (u >= a.U) return;
    const int64_t b0 = a.blk_off[u], nb = a.blk_off[u + 1] - b0, P = a.pos_off[u + 1] - a.pos_off[u];
    int64_t e = 0;
    for (int64_t k = 0; k < nb; k++) {
        entry[b0 + k] = (int32_t)e;
        if (e >= 0) e = k * a.B + e >= P ? -1 : maps[(b0 + k) * a.E + e];
    }
}

// ---- 3. kept frames, their places, the copy ----

__global__ __launch_bounds__(SILENCE_WG)
void silence_mark_kernel(SilenceArgs a, int64_t n_blocks, const int32_t *__restrict__ entry, int32_t *__restrict__ list,
                         int32_t *__restrict__ n_kept, int64_t *__restrict__ cnt) {
    for (int64_t blk = (int64_t)blockIdx.x * SILENCE_WG + threadIdx.x; blk < n_blocks; blk += (int64_t)gridDim.x * SILENCE_WG) {
        if (blk == 0) cnt[0] = 0;
        const int32_t e = entry[blk];
        int64_t j = 0, samples = 0;
        if (e >= 0) {
            const int u = find_segment(a.blk_off, a.U, blk);
            const int64_t k = blk - a.blk_off[u];
            const SilenceUtt t = load_utt(a, u);
            int64_t p = k * a.B + e;
            const int64_t end = min((k + 1) * a.B, t.P);
            while (p < end) {
                if (frame_silent(a, t, p)) {
                    p += a.Lg;
                } else {
                    // (kept frames lie at least Sg apart inside B positions: j stays below cap = ceil(B / Sg))
                    if (j < a.cap) list[blk * a.cap + j] = (int32_t)(p - k * a.B);
                    j++;
                    samples += min(a.K, t.n - p * a.g);            // silence.py:43: min(S, len), len = min(L, n - i)
                    p += a.Sg;
                }
            }
        }
        n_kept[blk] = (int32_t)min(j, a.cap);
        cnt[blk + 1] = samples;
    }
}

__global__ __launch_bounds__(SILENCE_WG)
void silence_offsets_kernel(SilenceArgs a, const int64_t *__restrict__ cnt, int64_t *__restrict__ out_off) {
    const int u = blockIdx.x * SILENCE_WG + threadIdx.x;
    if (u <= a.U) out_off[u] = cnt[a.blk_off[u]];
}

// a block's kept frames to their place: `total` samples, frame j's at j K (only an utterance's last frame is shorter)
template <typename I>
__device__ __forceinline__ void copy_block(const int16_t *__restrict__ src, const int32_t *__restrict__ l, int64_t g, I K, I total,
                                           bool pairs, int16_t *__restrict__ dst) {
    if (pairs) {
        // every frame starts on an even sample on both sides and K is even: two samples per load and store
        const I np = total / 2;
        for (I t = threadIdx.x; t < np; t += SILENCE_WG) {
            const I s = 2 * t, j = s / K, r = s - j * K;
            *reinterpret_cast<uint32_t *>(dst + s) = *reinterpret_cast<const uint32_t *>(src + (int64_t)l[j] * g + r);
        }
        if ((total & 1) && threadIdx.x == 0) {
            const I s = total - 1, j = s / K, r = s - j * K;
            dst[s] = src[(int64_t)l[j] * g + r];
        }
    } else {
        for (I s = threadIdx.x; s < total; s += SILENCE_WG) {
            const I j = s / K, r = s - j * K;
            dst[s] = src[(int64_t)l[j] * g + r];
        }
    }
}

__global__ __launch_bounds__(SILENCE_WG)
void silence_copy_kernel(const int16_t *__restrict__ pcm, SilenceArgs a, int64_t n_blocks, const int32_t *__restrict__ list,
                         const int32_t *__restrict__ n_kept, const int64_t *__restrict__ cnt, int16_t *__restrict__ out) {
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        if (n_kept[blk] == 0) continue;
        const int64_t d0 = cnt[blk], total = cnt[blk + 1] - d0;
        const int u = find_segment(a.blk_off, a.U, blk);
        const int64_t src0 = a.off[u] + (blk - a.blk_off[u]) * a.B * a.g;
        const bool pairs = ((a.K | a.g | src0 | d0) & 1) == 0;
        const int32_t *l = list + blk * a.cap;
        if (total < ((int64_t)1 << 31) && a.K < ((int64_t)1 << 31))
            copy_block<uint32_t>(pcm + src0, l, a.g, (uint32_t)a.K, (uint32_t)total, pairs, out + d0);
        else
            copy_block<int64_t>(pcm + src0, l, a.g, a.K, total, pairs, out + d0);
    }
}

// ---- host ----

static std::atomic<long> &block_option() {
    static std::atomic<long> v{0};
    return v;
}
void set_silence_block(long v) { block_option().store(v); }
long silence_block() { return block_option().load(); }

namespace {
struct SilenceScratch {
    DevBuf<int64_t> tables;         // pos_off [U + 1], blk_off [U + 1]
    DevBuf<int64_t> pre, tile_tot, cnt;
    DevBuf<int32_t> maps, entry, list, n_kept;
    PinnedBuf<int64_t> h_off;       // the new batch's offsets on their way back
};

// v[0 .. n) -> its inclusive sums, in place
void scan_inclusive(int64_t *v, int64_t n, DevBuf<int64_t> &tile_tot) {
    if (n <= 0) return;
    const int64_t n_tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    tile_tot.ensure((size_t)n_tiles);
    const int grid = silence_grid(n_tiles, 1);
    hipLaunchKernelGGL(silence_scan_tiles_kernel, dim3(grid), dim3(SILENCE_WG), 0, ctx().stream, v, n, tile_tot.p);
    if (n_tiles > 1) {
        hipLaunchKernelGGL(silence_scan_totals_kernel, dim3(1), dim3(SILENCE_WG), 0, ctx().stream, tile_tot.p, n_tiles);
        hipLaunchKernelGGL(silence_scan_add_kernel, dim3(grid), dim3(SILENCE_WG), 0, ctx().stream, v, n, tile_tot.p);
    }
    SR_HIP(hipGetLastError());
}
}  // namespace

void silence_remove_batch(SRBatch &pcm, double fs, double frame_duration, double frame_shift, double perc, SRBatch &out,
                          int64_t *kept_out) {
    ensure_device();
    if (pcm.kind != SRBatch::PCM16) fail("silence removal takes an int16 PCM batch (float PCM and feature batches are refused)");
    pcm.bind_device();
    out.bind_device();
    const int U = pcm.n_utt;
    if (U < 1) fail("silence removal needs at least one utterance");
    int64_t max_samples = 0;
    for (int u = 0; u < U; u++) {
        const int64_t n = pcm.offsets[u + 1] - pcm.offsets[u];
        if (n < 1) fail("utterance %d has no samples (the reference's remove_silence raises there)", u);
        max_samples = std::max(max_samples, n);
    }
    SilencePlan pl;
    std::string why;
    if (!plan_silence(fs, frame_duration, frame_shift, max_samples, silence_block(), pl, why)) fail("remove_silence: %s", why.c_str());

    std::vector<int64_t> tab(2 * ((size_t)U + 1), 0);
    int64_t *pos_off = tab.data(), *blk_off = tab.data() + U + 1;
    for (int u = 0; u < U; u++) {
        const int64_t n = pcm.offsets[u + 1] - pcm.offsets[u];
        const int64_t P = n / pl.g + (n % pl.g != 0);
        pos_off[u + 1] = pos_off[u] + P;
        blk_off[u + 1] = blk_off[u] + P / pl.B + (P % pl.B != 0);
    }
    const int64_t n_pos = pos_off[U], n_blocks = blk_off[U];

    auto &w = per_device<SilenceScratch>();
    w.tables.upload(tab.data(), tab.size());
    w.pre.ensure((size_t)n_pos + 1);
    w.cnt.ensure((size_t)n_blocks + 1);
    w.maps.ensure((size_t)n_blocks * (size_t)pl.E);
    w.entry.ensure((size_t)n_blocks);
    w.list.ensure((size_t)n_blocks * (size_t)pl.list_cap);
    w.n_kept.ensure((size_t)n_blocks);
    w.h_off.ensure((size_t)U + 1);

    SilenceArgs a;
    a.off = pcm.d_offsets.p;
    a.pos_off = w.tables.p;
    a.blk_off = w.tables.p + U + 1;
    a.pre = w.pre.p;
    a.U = U;
    a.L = pl.L; a.g = pl.g; a.Lg = pl.Lg; a.Sg = pl.Sg; a.K = pl.K; a.E = pl.E; a.B = pl.B; a.cap = pl.list_cap;
    a.perc = perc;
    hipStream_t st = ctx().stream;

    if (pl.chunk_lanes == 64)
        hipLaunchKernelGGL(silence_chunk_kernel<64>, dim3(silence_grid(n_pos, SILENCE_WG / 64)), dim3(SILENCE_WG), 0, st, pcm.pcm16.p, a,
                           n_pos, w.pre.p);
    else
        hipLaunchKernelGGL(silence_chunk_kernel<1>, dim3(silence_grid(n_pos, SILENCE_WG)), dim3(SILENCE_WG), 0, st, pcm.pcm16.p, a, n_pos,
                           w.pre.p);
    SR_HIP(hipGetLastError());
    scan_inclusive(w.pre.p + 1, n_pos, w.tile_tot);

    hipLaunchKernelGGL(silence_maps_kernel, dim3(silence_grid(n_blocks, pl.blocks_per_wg)), dim3(SILENCE_WG), 0, st, a, n_blocks,
                       pl.blocks_per_wg, w.maps.p);
    hipLaunchKernelGGL(silence_chain_kernel, dim3((U + 63) / 64), dim3(64), 0, st, a, w.maps.p, w.entry.p);
    hipLaunchKernelGGL(silence_mark_kernel, dim3(silence_grid(n_blocks, SILENCE_WG)), dim3(SILENCE_WG), 0, st, a, n_blocks, w.entry.p,
                       w.list.p, w.n_kept.p, w.cnt.p);
    SR_HIP(hipGetLastError());
    scan_inclusive(w.cnt.p + 1, n_blocks, w.tile_tot);

    out.kind = SRBatch::PCM16;
    out.n_utt = U;
    out.dim = 0;
    out.d_offsets.ensure((size_t)U + 1);
    hipLaunchKernelGGL(silence_offsets_kernel, dim3((U + 1 + SILENCE_WG - 1) / SILENCE_WG), dim3(SILENCE_WG), 0, st, a, w.cnt.p,
                       out.d_offsets.p);
    SR_HIP(hipGetLastError());
    // the U + 1 offsets come back once, through page-locked memory: the host copy is what tile tables are built from
    SR_HIP(hipMemcpyAsync(w.h_off.p, out.d_offsets.p, ((size_t)U + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    sync_stream();
    out.offsets.assign(w.h_off.p, w.h_off.p + U + 1);
    out.n_rows = out.offsets[U];
    out.invalidate_tiles();
    if (out.offsets[0] != 0 || out.n_rows < 0 || out.n_rows > pcm.n_rows) fail("silence removal: inconsistent output offsets");
    for (int u = 0; u < U; u++) {
        const int64_t kept = out.offsets[u + 1] - out.offsets[u];
        if (kept < 0 || kept > pcm.offsets[u + 1] - pcm.offsets[u]) fail("silence removal: inconsistent output offsets");
        if (kept_out) kept_out[u] = kept;
    }
    out.pcm16.ensure((size_t)std::max<int64_t>(1, out.n_rows));
    if (out.n_rows > 0) {
        hipLaunchKernelGGL(silence_copy_kernel, dim3(silence_grid(n_blocks, 1)), dim3(SILENCE_WG), 0, st, pcm.pcm16.p, a, n_blocks,
                           w.list.p, w.n_kept.p, w.cnt.p, out.pcm16.p);
        SR_HIP(hipGetLastError());
    }
}

}  // namespace sr
