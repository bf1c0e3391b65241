// gmm_score.hip -- diagonal-GMM log-likelihood scoring on gfx950 (CDNA4), the hot loop of
// the path.  Replaces Gaussian::probability_of_fast_exp (src/gmm/src/gmm.cc:176-202),
// GMM::log_probability_of_fast_exp (:237-244) and threaded_log_probability_of (:533-569), and
// -- by looping all S speaker models over a resident frame tile -- the per-speaker ABI loop
// of GMMSet.predict_one (src/testbench/gmmset.py:59-64, 95-99).
//
// Formulation:  LL(x) = ln2 * log2sum_k 2^(c_k - sum_d (x_d s_kd + m_kd)^2)
// with the tables of gmm_model.hpp; fp32, online max; optional reference-compat clamp.
//
// Mapping: a workgroup (256 threads = 4 wave64) owns one tile of 256*F frames of one
// utterance; every lane keeps F frames (F*D floats) in VGPRs for the whole kernel, so X is
// read from HBM exactly once.  Mixture parameters stream through LDS in chunks (double
// buffered by LDS-DMA); all lanes read the same LDS address (broadcast),
// two ds_read_b128 feed 8*F FMAs.  The log-sum-exp is online per lane, in the log2 domain
// (v_exp_f32 / v_log_f32 are base-2).  No MFMA: the 2-FMA distance form is not a contraction.
#include "lse.hpp"
#include "score.hpp"
#include "wave_ops.hpp"

#include <cmath>

namespace sr {

__host__ __device__ constexpr int score_waves_per_eu(int dp, int f) {
    return dp > 64 ? 2 : (dp * f + 44 <= 128) ? 4 : (dp * f + 44 <= 168) ? 3 : 2;     // wide rows: LDS chunks of 20-33 KB
}

typedef float v2f __attribute__((ext_vector_type(2)));

// Lane-private arithmetic on either one frame (float) or a packed pair of frames (v2f ->
// v_pk_fma_f32, the mixture constants broadcast to both halves through op_sel).
template <bool PK> struct Lanes;
template <> struct Lanes<false> {
    using T = float;
    static constexpr int W = 1;
    static __device__ __forceinline__ T zero() { return 0.0f; }
    static __device__ __forceinline__ T fma_bcast(T x, float s, float m) { return fmaf(x, s, m); }
    static __device__ __forceinline__ T fma_sq(T t, T acc) { return fmaf(t, t, acc); }
    static __device__ __forceinline__ float get(T v, int) { return v; }
    static __device__ __forceinline__ void set(T &v, int, float s) { v = s; }
};
template <> struct Lanes<true> {
    using T = v2f;
    static constexpr int W = 2;
    static __device__ __forceinline__ T zero() { return (v2f){0.0f, 0.0f}; }
    static __device__ __forceinline__ T fma_bcast(T x, float s, float m) {
        return __builtin_elementwise_fma(x, (v2f){s, s}, (v2f){m, m});
    }
    static __device__ __forceinline__ T fma_sq(T t, T acc) { return __builtin_elementwise_fma(t, t, acc); }
    static __device__ __forceinline__ float get(T v, int e) { return e ? v.y : v.x; }
    static __device__ __forceinline__ void set(T &v, int e, float s) { if (e) v.y = s; else v.x = s; }
};

template <int DP, int F, bool PK>
__global__ __launch_bounds__(256, score_waves_per_eu(DP, F))
void gmm_score_kernel(const float *__restrict__ X, const TileDesc *__restrict__ tiles,
                      const float4 *__restrict__ params, const float *__restrict__ center,
                      const ChunkDesc *__restrict__ chunks,
                      const int *__restrict__ group_chunk_begin, double *__restrict__ partial,
                      float *__restrict__ frame_ll, int64_t n_frames, int dim, int n_models,
                      int clamp, int n_groups, int n_tiles, float band_hi) {
    using L = Lanes<PK>;
    using XT = typename L::T;
    constexpr int W = L::W;
    constexpr int NV = F / W;                // lane-private vectors per dim
    static_assert(F % W == 0, "packed variant needs an even number of frames per lane");
    constexpr int REC = 2 * DP + 1;          // float4 per record
    constexpr int CHUNK_F4 = CB * REC;       // float4 per LDS buffer
    constexpr int PF = (CHUNK_F4 + 255) / 256;
    // Two separately named LDS objects (not one [2][..] array): the buffer a ds_read touches
    // is then statically distinct from the one an in-flight LDS-DMA writes, which lets hipcc
    // keep the DMA outstanding across the compute instead of draining vmcnt(0) first.
    __shared__ float4 lds_a[CHUNK_F4];
    __shared__ float4 lds_b[CHUNK_F4];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // XCD-aware 1-D grid: workgroup b runs on XCD b % 8 (observed dispatch order, speed only), so
    // the G workgroups that share a frame tile are given ids 8 apart: same XCD, same L2, adjacent
    // in dispatch order -> the tile's rows leave HBM / the fabric once instead of G times.
    const int tile_lo = blockIdx.x & 7;
    const int q = blockIdx.x >> 3;
    const int g = q % n_groups;
    const int tile_id = (q / n_groups) * 8 + tile_lo;
    if (tile_id >= n_tiles) return;              // padding workgroups (whole workgroup, before any barrier)
    const TileDesc tile = tiles[tile_id];
    const int chunk_begin = group_chunk_begin[g];
    const int chunk_end = group_chunk_begin[g + 1];

    // LDS-DMA (global_load_lds_dwordx4): LDS destination = wave-uniform base + lane*16, so a
    // chunk (a linear run of float4) lands as a linear image; no VGPR round trip.
    auto stage = [&](float4 *dst, const ChunkDesc cd) {
        const float4 *src = params + cd.offset_f4;
        const int n4 = cd.n_records * REC;
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const int base = (i * 4 + wave) * 64;
            if (base + lane < n4)
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void *)(src + base + lane),
                    (__attribute__((address_space(3))) void *)(dst + base), 16, 0, 0);
        }
    };
    stage(lds_a, chunks[chunk_begin]);   // in flight while the frames are fetched

    // ---- resident frames: frame f of this lane = tile.start + f*256 + tid ----
    XT x[NV][DP];
    bool valid[F];
    int64_t row[F];
#pragma unroll
    for (int f = 0; f < F; f++) {
        const int local = f * 256 + tid;
        valid[f] = local < tile.count;
        row[f] = tile.start + (valid[f] ? local : 0);
        const float *src = X + row[f] * dim;
        if (dim == DP) {
#pragma unroll
            for (int d = 0; d < DP; d++) L::set(x[f / W][d], f % W, src[d] - center[d]);
        } else {
#pragma unroll
            for (int d = 0; d < DP; d++) L::set(x[f / W][d], f % W, (d < dim) ? src[d] - center[d] : 0.0f);
        }
    }

    float m[F], ssum[F];
#pragma unroll
    for (int f = 0; f < F; f++) {
        m[f] = NEG_BIG;
        ssum[f] = 0.0f;
    }
    const float drop_thr = clamp ? LSE_MINLOG2 : -3.0e38f;      // wave-uniform
    dma_publish_barrier();   // drains the LDS-DMA of chunk 0 (hipcc emits vmcnt(0) before the barrier)

    // One chunk: stage the next one into `other`, run all records of `cur`, close the model
    // if the chunk is its last, then barrier (next chunk landed; everyone is done with `cur`).
    auto do_chunk = [&](const float4 *cur, float4 *other, int c) {
        const ChunkDesc cd = chunks[c];
        if (c + 1 < chunk_end) stage(other, chunks[c + 1]);

        for (int r = 0; r < cd.n_records; r++) {
            const float4 *rec = cur + r * REC;
            XT acc[NV][KB];
#pragma unroll
            for (int h = 0; h < NV; h++)
#pragma unroll
                for (int j = 0; j < KB; j++) acc[h][j] = L::zero();
#pragma unroll
            for (int d = 0; d < DP; d++) {
                const float4 p0 = rec[2 * d];
                const float4 p1 = rec[2 * d + 1];
#pragma unroll
                for (int h = 0; h < NV; h++) {
                    const XT xv = x[h][d];
                    const XT t0 = L::fma_bcast(xv, p0.x, p0.y);
                    const XT t1 = L::fma_bcast(xv, p0.z, p0.w);
                    const XT t2 = L::fma_bcast(xv, p1.x, p1.y);
                    const XT t3 = L::fma_bcast(xv, p1.z, p1.w);
                    acc[h][0] = L::fma_sq(t0, acc[h][0]);
                    acc[h][1] = L::fma_sq(t1, acc[h][1]);
                    acc[h][2] = L::fma_sq(t2, acc[h][2]);
                    acc[h][3] = L::fma_sq(t3, acc[h][3]);
                }
            }
            const float4 cc = rec[2 * DP];
#pragma unroll
            for (int f = 0; f < F; f++) {
                const float v0 = cc.x - L::get(acc[f / W][0], f % W);
                const float v1 = cc.y - L::get(acc[f / W][1], f % W);
                const float v2 = cc.z - L::get(acc[f / W][2], f % W);
                const float v3 = cc.w - L::get(acc[f / W][3], f % W);
                const float mx = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
                const float mn = fmaxf(m[f], mx);
                // the reference's sub-DBL_MIN terms are exactly 0 (lse.hpp).  Branch-free on purpose: a wave-uniform "only
                // next to the boundary" branch here, inside the unrolled frame loop, cost this kernel 300-800 dwords of
                // scratch per lane (1240 B at D = 39, F = 4: 10x slower); four selects per frame and record are ~4 %.
                // (a running maximum below the boundary means every earlier term was dropped: ssum is already 0)
                // (the select sits on exp2's ARGUMENT -- 2^-1e30 = 0 -- so that the compiler has nothing expensive to branch around)
                const float e0 = __builtin_amdgcn_exp2f(v0 >= drop_thr ? v0 - mn : LSE_NEG_BIG);
                const float e1 = __builtin_amdgcn_exp2f(v1 >= drop_thr ? v1 - mn : LSE_NEG_BIG);
                const float e2 = __builtin_amdgcn_exp2f(v2 >= drop_thr ? v2 - mn : LSE_NEG_BIG);
                const float e3 = __builtin_amdgcn_exp2f(v3 >= drop_thr ? v3 - mn : LSE_NEG_BIG);
                ssum[f] = fmaf(ssum[f], __builtin_amdgcn_exp2f(m[f] - mn), (e0 + e1) + (e2 + e3));
                m[f] = mn;
            }
        }

        if (cd.model_done >= 0) {   // wave-uniform: close the model, start the next one
            const int s = cd.model_done;
            double mine = 0.0;
            bool hot = false;              // a frame in the band of the reference's partial-product flushes (lse.hpp)
#pragma unroll
            for (int f = 0; f < F; f++) {
                // the reference's underflow behaviour (safe_log -> ln 1e-15, gmm.cc:34-38, :237-244): lse.hpp
                const float ll = lse_close1(m[f], ssum[f], clamp);
                if (valid[f]) {
                    mine += (double)ll;
                    if (frame_ll) frame_ll[(int64_t)s * n_frames + row[f]] = ll;
                    hot |= ll < band_hi;
                }
                m[f] = NEG_BIG;
                ssum[f] = 0.0f;
            }
            mine = wave_sum_f64(mine);     // DPP + readlane: no LDS round trips in the per-model close
            if (__builtin_amdgcn_ballot_w64(hot) != 0) mine = SR_FLUSH_POISON;
            if (lane == 0) partial[((int64_t)tile_id * n_models + s) * 4 + wave] = mine;
        }
        dma_publish_barrier();
    };

    for (int c = chunk_begin; c < chunk_end; c += 2) {
        do_chunk(lds_a, lds_b, c);
        if (c + 1 < chunk_end) do_chunk(lds_b, lds_a, c + 1);
    }
}

// Rows wider than MAX_REG_DIM (the reference has no limit, gmm.cc:40-51): the same direct form, same records, same lane = frame,
// with the D loop cut into slices of WIDE_DC dimensions.  A step = (chunk of <= CB records of one model, slice): the slice's
// parameters -- n_records runs of 2 WIDE_DC float4 inside the record-major layout -- land in LDS by LDS-DMA one step ahead, the
// lane fetches its row's slice (256 B of its own row; the tile's rows stay in L2 between steps), and the CB x KB running
// distances stay in registers across the chunk's slices; constants, log-sum-exp update and the model close follow the last
// slice exactly as above.  Any dim: the slice count is a run-time value.
__global__ __launch_bounds__(256, 3)
void gmm_score_wide_kernel(const float *__restrict__ X, const TileDesc *__restrict__ tiles,
                           const float4 *__restrict__ params, const float *__restrict__ center,
                           const ChunkDesc *__restrict__ chunks, const int *__restrict__ group_chunk_begin,
                           double *__restrict__ partial, float *__restrict__ frame_ll, int64_t n_frames, int dim, int dp,
                           int n_models, int clamp, int n_groups, int n_tiles, float band_hi) {
    constexpr int DC = WIDE_DC;
    constexpr int RUN = 2 * DC;              // float4 per record and slice
    constexpr int SLICE_F4 = CB * RUN;
    constexpr int PF = SLICE_F4 / 256;
    static_assert(RUN % 64 == 0 && SLICE_F4 % 256 == 0, "an LDS-DMA instruction stays inside one record's run");
    __shared__ float4 lds_a[SLICE_F4];
    __shared__ float4 lds_b[SLICE_F4];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile_lo = blockIdx.x & 7;      // XCD-aware order, as gmm_score_kernel
    const int q = blockIdx.x >> 3;
    const int g = q % n_groups;
    const int tile_id = (q / n_groups) * 8 + tile_lo;
    if (tile_id >= n_tiles) return;
    const TileDesc tile = tiles[tile_id];
    const int chunk_begin = group_chunk_begin[g];
    const int chunk_end = group_chunk_begin[g + 1];
    const int rec_f4 = 2 * dp + 1;
    const int n_dc = dp / DC;

    auto stage = [&](float4 *dst, const ChunkDesc cd, int dc) {
        const float4 *src = params + cd.offset_f4 + dc * RUN;
        const int n4 = cd.n_records * RUN;
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const int base = (i * 4 + wave) * 64;      // wave-uniform; record base / RUN, offset base % RUN + lane inside its run
            if (base < n4)
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void *)(src + (size_t)(base / RUN) * rec_f4 + (base % RUN) + lane),
                    (__attribute__((address_space(3))) void *)(dst + base), 16, 0, 0);
        }
    };
    stage(lds_a, chunks[chunk_begin], 0);

    const bool valid = tid < tile.count;
    const int64_t row = tile.start + (valid ? tid : 0);
    const float *xrow = X + row * dim;
    float m = NEG_BIG, ssum = 0.0f;
    const float drop_thr = clamp ? LSE_MINLOG2 : -3.0e38f;
    float acc[CB][KB];
    dma_publish_barrier();

    auto do_step = [&](const float4 *cur, float4 *other, int c, int dc) __attribute__((always_inline)) {
        const ChunkDesc cd = chunks[c];
        {
            const int dcn = dc + 1 < n_dc ? dc + 1 : 0;
            const int cn = dcn ? c : c + 1;
            if (cn < chunk_end) stage(other, chunks[cn], dcn);
        }
        float x[DC];
        const int d0 = dc * DC;
        if (d0 + DC <= dim) {                // wave-uniform
#pragma unroll
            for (int d = 0; d < DC; d++) x[d] = xrow[d0 + d] - center[d0 + d];
        } else {
#pragma unroll
            for (int d = 0; d < DC; d++) x[d] = (d0 + d < dim) ? xrow[d0 + d] - center[d0 + d] : 0.0f;
        }
        if (dc == 0) {
#pragma unroll
            for (int r = 0; r < CB; r++)
#pragma unroll
                for (int j = 0; j < KB; j++) acc[r][j] = 0.0f;
        }
#pragma unroll
        for (int r = 0; r < CB; r++) {
            if (r < cd.n_records) {          // wave-uniform
                const float4 *rec = cur + r * RUN;
#pragma unroll
                for (int d = 0; d < DC; d++) {
                    const float4 p0 = rec[2 * d];
                    const float4 p1 = rec[2 * d + 1];
                    const float t0 = fmaf(x[d], p0.x, p0.y);
                    const float t1 = fmaf(x[d], p0.z, p0.w);
                    const float t2 = fmaf(x[d], p1.x, p1.y);
                    const float t3 = fmaf(x[d], p1.z, p1.w);
                    acc[r][0] = fmaf(t0, t0, acc[r][0]);
                    acc[r][1] = fmaf(t1, t1, acc[r][1]);
                    acc[r][2] = fmaf(t2, t2, acc[r][2]);
                    acc[r][3] = fmaf(t3, t3, acc[r][3]);
                }
            }
        }
        if (dc == n_dc - 1) {
#pragma unroll
            for (int r = 0; r < CB; r++) {
                if (r < cd.n_records) {
                    const float4 cc = params[cd.offset_f4 + (size_t)r * rec_f4 + 2 * dp];      // wave-uniform address
                    const float v0 = cc.x - acc[r][0], v1 = cc.y - acc[r][1], v2 = cc.z - acc[r][2], v3 = cc.w - acc[r][3];
                    const float mx = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
                    const float mn = fmaxf(m, mx);
                    // (the reference's sub-DBL_MIN terms are exactly 0: lse.hpp; select on exp2's argument as gmm_score_kernel)
                    const float e0 = __builtin_amdgcn_exp2f(v0 >= drop_thr ? v0 - mn : LSE_NEG_BIG);
                    const float e1 = __builtin_amdgcn_exp2f(v1 >= drop_thr ? v1 - mn : LSE_NEG_BIG);
                    const float e2 = __builtin_amdgcn_exp2f(v2 >= drop_thr ? v2 - mn : LSE_NEG_BIG);
                    const float e3 = __builtin_amdgcn_exp2f(v3 >= drop_thr ? v3 - mn : LSE_NEG_BIG);
                    ssum = fmaf(ssum, __builtin_amdgcn_exp2f(m - mn), (e0 + e1) + (e2 + e3));
                    m = mn;
                }
            }
            if (cd.model_done >= 0) {
                const int s = cd.model_done;
                const float ll = lse_close1(m, ssum, clamp);
                double mine = 0.0;
                bool hot = false;
                if (valid) {
                    mine = (double)ll;
                    if (frame_ll) frame_ll[(int64_t)s * n_frames + row] = ll;
                    hot = ll < band_hi;
                }
                m = NEG_BIG;
                ssum = 0.0f;
                mine = wave_sum_f64(mine);
                if (__builtin_amdgcn_ballot_w64(hot) != 0) mine = SR_FLUSH_POISON;
                if (lane == 0) partial[((int64_t)tile_id * n_models + s) * 4 + wave] = mine;
            }
        }
        dma_publish_barrier();
    };

    int c = chunk_begin, dc = 0;
    while (c < chunk_end) {
        do_step(lds_a, lds_b, c, dc);
        if (++dc == n_dc) { dc = 0; c++; }
        if (c >= chunk_end) break;
        do_step(lds_b, lds_a, c, dc);
        if (++dc == n_dc) { dc = 0; c++; }
    }
}

// Per utterance: add the tile/wave partials in a fixed order (deterministic), then the
// reference's argmax -- first maximum wins (gmmset.py:62-64, `max(enumerate(scores), key=...)`).
// A (tile, model) whose partial is SR_FLUSH_POISON holds a frame in the band where the reference's flushes of partial
// products decide (lse.hpp): it is left out of the sum and noted for gmm_flush.hip, which adds the tile's sum later.
//
// The order (round 4): the utterance's tiles in segments of `seg` consecutive tiles -- 32, or more for utterances of more
// than 32 k tiles, so that there are at most 1024 segments -- each summed front to back, then the segment sums front to back.
// It depends on the utterance's own tile count only, never on the batch around it.  One thread per (segment, model): until
// round 4 one thread per model walked ALL the tiles, which for the one long utterance of an E-step (400 k frames = 12 500
// tiles, one model) was 1.7 ms of dependent loads behind a 0.6 ms scoring kernel.
constexpr int FIN_LDS_DOUBLES = 4096;
__global__ __launch_bounds__(256)
void gmm_finalize_kernel(const double *partial, const int *utt_tile_begin, int n_models,
                         int per_tile, double *sums, int *argmax, int2 *flush_list, int *flush_count, int flush_cap,
                         FinalizeDelivery dl) {
    __shared__ double seg_sum[FIN_LDS_DOUBLES];
    const int u = blockIdx.x;
    const int tb = utt_tile_begin[u], te = utt_tile_begin[u + 1];
    const int n_t = te - tb;
    const int seg = max(32, (n_t + 1023) / 1024);
    const int n_seg = (n_t + seg - 1) / seg;                   // <= 1024
    const int mb = max(1, min(n_models, FIN_LDS_DOUBLES / max(1, n_seg)));      // models per pass
    double best = -INFINITY;
    int best_i = 0x7fffffff;
    for (int s0 = 0; s0 < n_models; s0 += mb) {
        const int m = min(mb, n_models - s0);
        for (int item = threadIdx.x; item < n_seg * m; item += 256) {
            const int sg = item / m, s = s0 + item - sg * m;   // (consecutive threads: consecutive models of one segment)
            const int t0 = tb + sg * seg, t1 = min(te, t0 + seg);
            double acc = 0.0;
            for (int t = t0; t < t1; t++) {
                // per_tile = 4: one double per wave of the tile's workgroup; 1: already combined
                const double *p = partial + ((int64_t)t * n_models + s) * per_tile;
                double tile_sum = 0.0;
                bool poisoned = false;
                for (int i = 0; i < per_tile; i++) {
                    poisoned |= flush_poisoned(p[i]);
                    tile_sum += p[i];
                }
                if (__builtin_expect(poisoned && flush_count != nullptr, 0)) {
                    const int idx = atomicAdd(flush_count, 1);
                    if (idx < flush_cap) flush_list[idx] = make_int2(t, s);
                    continue;
                }
                acc += tile_sum;
            }
            seg_sum[item] = acc;
        }
        __syncthreads();
        for (int sl = threadIdx.x; sl < m; sl += 256) {
            double acc = 0.0;
            for (int sg = 0; sg < n_seg; sg++) acc += seg_sum[sg * m + sl];
            const int s = s0 + sl;
            sums[(int64_t)u * n_models + s] = acc;
            if (acc > best) {                                  // (a thread meets its models in increasing order)
                best = acc;
                best_i = s;
            }
        }
        __syncthreads();
    }
    __shared__ double sv[256];
    __shared__ int si[256];
    sv[threadIdx.x] = best;
    si[threadIdx.x] = best_i;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            const double ov = sv[threadIdx.x + w];
            const int oi = si[threadIdx.x + w];
            if (ov > sv[threadIdx.x] || (ov == sv[threadIdx.x] && oi < si[threadIdx.x])) {
                sv[threadIdx.x] = ov;
                si[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) argmax[u] = (te > tb && si[0] != 0x7fffffff) ? si[0] : -1;
    if (dl.host == nullptr) return;
    // ---- the last workgroup to get here delivers the pass: results and counters to host memory, counters cleared ----
    __shared__ int s_last;
    __threadfence();                                       // this workgroup's sums / argmax / list entries before its ticket
    __syncthreads();
    if (threadIdx.x == 0) s_last = atomicAdd(&dl.counters[2], 1) == (int)gridDim.x - 1;
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    const int U = (int)gridDim.x;
    double *h_sums = reinterpret_cast<double *>(dl.host + 1);
    int *h_arg = reinterpret_cast<int *>(h_sums + (size_t)U * n_models);
    for (int i = threadIdx.x; i < U * n_models; i += 256)
        h_sums[i] = __hip_atomic_load(&sums[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int i = threadIdx.x; i < U; i += 256) h_arg[i] = __hip_atomic_load(&argmax[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x == 0) {
        dl.host->oor = __hip_atomic_load(&dl.counters[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        dl.host->n_flush = __hip_atomic_load(&dl.counters[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();                                       // (the counters are read: clear them for the next pass)
    for (int i = threadIdx.x; i < dl.n_counters; i += 256) dl.counters[i] = 0;
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(&dl.host->seq, dl.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Hybrid sets: LL = ln(exp(LL_a) + exp(LL_b)) per frame and model, the per-tile float64 sums for gmm_finalize_kernel, and
// (optionally) the merged per-frame values.  With the reference's clamp on, a part whose mixtures all fell below
// DBL_MIN reports ln(1e-15) (lse.hpp): both -> ln(1e-15); one -> the other part alone, as the reference's linear-domain
// sum of the surviving terms.
__global__ __launch_bounds__(256)
void gmm_merge_kernel(const float *__restrict__ A, const float *__restrict__ B, const TileDesc *__restrict__ tiles,
                      int n_models, int64_t n_frames, int clamp, double *__restrict__ partial, float *__restrict__ out,
                      float band_hi) {
    __shared__ double part[4];
    const TileDesc tile = tiles[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool valid = tid < tile.count;
    const int64_t row = tile.start + (valid ? tid : 0);
    for (int s = 0; s < n_models; s++) {
        double mine = 0.0;
        bool hot = false;                             // a frame in the band of the reference's partial-product flushes (lse.hpp)
        if (valid) {
            const float a = A[(int64_t)s * n_frames + row], b = B[(int64_t)s * n_frames + row];
            float ll;
            // with the clamp on, a half whose terms all underflowed reports -inf (lse.hpp, clamp 2): out of band
            const bool sa = clamp && a == -INFINITY, sb = clamp && b == -INFINITY;
            if (sa || sb) {
                ll = sa ? (sb ? LSE_LN_1E_15 : b) : a;        // (both: the reference's ln 1e-15)
            } else {
                const float hi = fmaxf(a, b), lo = fminf(a, b);
                ll = hi + LSE_LN2 * log2f(1.0f + __builtin_amdgcn_exp2f((lo - hi) * 1.4426950408889634f));
            }
            if (out) out[(int64_t)s * n_frames + row] = ll;
            mine = (double)ll;
            hot = ll < band_hi;
        }
        mine = wave_sum_f64(mine);
        if (__builtin_amdgcn_ballot_w64(hot) != 0) mine = SR_FLUSH_POISON;     // (inf + anything finite stays inf below)
        __syncthreads();                              // the previous model's reader is done with part[]
        if (lane == 0) part[wave] = mine;
        __syncthreads();
        if (tid == 0) partial[(int64_t)blockIdx.x * n_models + s] = ((part[0] + part[1]) + part[2]) + part[3];
    }
}

// ---------------- launch code (the passes themselves: gmm_score_host.cpp) ----------------

template <int DP, int F, bool PK>
static void launch_score(const ScoreArgs &a) {
    dim3 grid((unsigned)((int64_t)a.n_groups * ((a.n_tiles + 7) / 8) * 8));   // 1-D, XCD-aware order
    hipLaunchKernelGGL((gmm_score_kernel<DP, F, PK>), grid, dim3(256), 0, ctx().stream, a.X, a.tiles,
                       a.params, a.center, a.chunks, a.group_chunk_begin, a.partial, a.frame_ll, a.n_frames,
                       a.dim, a.n_models, a.clamp, a.n_groups, a.n_tiles, a.band_hi);
}

template <int DP>
static void dispatch_f(const ScoreArgs &a, int F, bool pk) {
    if constexpr (DP > 64) {
        return launch_score<DP, 1, false>(a);     // wide rows: one frame per lane
    } else {
        if (F == 1) return launch_score<DP, 1, false>(a);
        if (F == 2) return pk ? launch_score<DP, 2, true>(a)
                              : launch_score<DP, 2, false>(a);
        if constexpr (DP <= 40) {
            if (F == 4) return pk ? launch_score<DP, 4, true>(a)
                                  : launch_score<DP, 4, false>(a);
        }
        fail("frames_per_lane=%d not instantiated for dim %d", F, DP);
    }
}

void launch_score_vector(const ScoreArgs &a, int DP, int F, bool pk) {
    switch (DP) {
        case 8: dispatch_f<8>(a, F, pk); break;
        case 13: dispatch_f<13>(a, F, pk); break;
        case 16: dispatch_f<16>(a, F, pk); break;
        case 24: dispatch_f<24>(a, F, pk); break;
        case 26: dispatch_f<26>(a, F, pk); break;
        case 32: dispatch_f<32>(a, F, pk); break;
        case 34: dispatch_f<34>(a, F, pk); break;
        case 39: dispatch_f<39>(a, F, pk); break;
        case 40: dispatch_f<40>(a, F, pk); break;
        case 48: dispatch_f<48>(a, F, pk); break;
        case 56: dispatch_f<56>(a, F, pk); break;
        case 64: dispatch_f<64>(a, F, pk); break;
        case 80: dispatch_f<80>(a, F, pk); break;
        case 96: dispatch_f<96>(a, F, pk); break;
        default: fail("no scoring kernel for padded dim %d", DP);
    }
}

void launch_score_wide(const ScoreArgs &a, int DP) {
    dim3 grid((unsigned)((int64_t)a.n_groups * ((a.n_tiles + 7) / 8) * 8));
    hipLaunchKernelGGL(gmm_score_wide_kernel, grid, dim3(256), 0, ctx().stream, a.X, a.tiles, a.params, a.center, a.chunks,
                       a.group_chunk_begin, a.partial, a.frame_ll, a.n_frames, a.dim, DP, a.n_models, a.clamp, a.n_groups, a.n_tiles,
                       a.band_hi);
}

void launch_finalize(const double *partial, const TileTable &tt, int n_utt, int n_models, int per_tile, double *sums, int *argmax,
                     int2 *flush_list, int *flush_count, int flush_cap, const FinalizeDelivery &dl) {
    hipLaunchKernelGGL(gmm_finalize_kernel, dim3((unsigned)n_utt), dim3(256), 0, ctx().stream, partial, tt.d_utt_tile_begin.p,
                       n_models, per_tile, sums, argmax, flush_list, flush_count, flush_cap, dl);
}

void launch_merge(const float *a, const float *b, const TileTable &tt, int n_models, int64_t n_frames, int clamp, double *partial,
                  float *out, float band_hi) {
    hipLaunchKernelGGL(gmm_merge_kernel, dim3((unsigned)tt.n_tiles), dim3(256), 0, ctx().stream, a, b, tt.d_tiles.p, n_models,
                       n_frames, clamp, partial, out, band_hi);
}

}  // namespace sr
