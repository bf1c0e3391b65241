// timeline.hip -- who spoke when: a scoring pass's per-frame matrix [S][n_frames] (fp32, on the device) -> a label per window of
// every recording of the batch.  The definitions (include/pygmm_hip.h states them in full; tests/timeline_oracle.py restates them):
//   windows    recording of n frames, window W, hop H: Nw = 0 if n = 0 else 1 + ceil(max(0, n - W) / H); window j covers frames
//              [j H, min(j H + W, n)), c_j of them (W < H: no window that would start at or behind frame n, timeline_plan.hpp).
//   sums       sum[j][s]: float64, the fp32 values of column s added in frame order.  q = sum / c_j; a NaN q becomes -inf (the
//              recording's count of such windows goes up).
//   states     a state per column; column bg (if >= 0) is "nobody": emission q + threshold, label -1, LAST in every tie; the
//              speakers come in column order.  The first maximum in that order wins everywhere.
//   raw        the first maximum of a window's emissions; -1 when that maximum is -inf.
//   hold       shown[j] = raw[k], k the last window <= j where NOT (raw[k] != -1 and raw[k-1] != -1 and raw[k-1] != raw[k]).
//   viterbi    max over paths of sum_j e_j(l_j) - beta (#changes), every run but the last at least m windows; float64, states
//              (s, k), k = 1 .. m, the recurrence of the header; one add or one compare per operation, nothing fused.
//
// Four kernels and two small ones:
//   timeline_sum_kernel      a workgroup = 4 consecutive windows of one recording x 64 columns.  It walks the frames those windows
//                            span in chunks of 64, each chunk staged transposed into LDS ([frame][column], coalesced reads along
//                            the frames of a column; stride 65 floats so that neither side meets a bank twice); wave w adds the
//                            chunk's part of window w, a lane per column, in frame order.  Output [window][column]: the lanes of
//                            a wave write one row.  No atomics: a sum has one owner.
//   timeline_raw_kernel      a wave per window: emissions, first maximum (wave_first_max_f64 over (value, priority rank)), the
//                            NaN flag.
//   timeline_hold_kernel     a workgroup per recording: the hold rule as a maximum-scan of "last window whose change test is
//                            false" over 256 windows at a time with a carry -- an alternating stretch of any length costs the
//                            same as a quiet one; also the recording's count of NaN windows.
//   timeline_forward_kernel  a workgroup per recording, lanes over states; a lane holds the emissions of the next `tile` windows
//                            in registers (the loads of a tile are issued before the steps of the tile before it, the divisions
//                            done behind them: a step is the maximum, the adds and the compares).  S <= 64: one
//                            wave, the entering maximum by DPP / readlane, no barrier; S <= 1024: a lane per state, the waves'
//                            maxima meet in LDS behind ONE barrier a step (two slots, by the step's parity); S <= 4096: four
//                            states a lane.  d(s, m) lives in a register; d(s, 1 .. m - 1) is a ring of m - 1 slots per state
//                            (LDS when it fits, else global; m = 2: a register).  Back-pointers: a stay bit per (window, state)
//                            -- a wave's ballot is one 64-bit word -- and the entering state per window.
//   timeline_trace_kernel    a lane per recording walks back from the end state and writes the labels.
// The decisions are plan_timeline's (timeline_plan.cpp).
#pragma clang fp contract(off)

#include "timeline.hpp"
#include "timeline_plan.hpp"

#include "batch.hpp"
#include "wave_ops.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

namespace sr {

namespace {

// ---- window sums ----

__global__ __launch_bounds__(TIMELINE_SUM_WG)
void timeline_sum_kernel(const float *__restrict__ fll, int64_t n_total, const int64_t *__restrict__ off,
                         const int64_t *__restrict__ win_off, const int32_t *__restrict__ tile_utt, const int32_t *__restrict__ tile_j0,
                         int S, int64_t W, int64_t H, double *__restrict__ sums, int32_t *__restrict__ counts) {
    __shared__ float lds[TIMELINE_SUM_CHUNK * TIMELINE_SUM_STRIDE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int u = tile_utt[blockIdx.x];
    const int64_t j0 = tile_j0[blockIdx.x];
    const int s0 = blockIdx.y * TIMELINE_SUM_COLS;
    const int64_t row0 = off[u], n = off[u + 1] - row0;
    const int64_t wbase = win_off[u], nw = win_off[u + 1] - wbase;
    const int64_t jw = j0 + wave;
    const bool active = jw < nw;
    const int64_t wb = jw * H, we = min(wb + W, n);                  // this wave's window
    const int64_t jl = min(j0 + TIMELINE_SUM_WINDOWS - 1, nw - 1);   // the tile's last window
    const int64_t fb = j0 * H, fe = min(jl * H + W, n);              // the frames the tile spans: inside [0, n)
    double acc = 0.0;
    for (int64_t c0 = fb; c0 < fe; c0 += TIMELINE_SUM_CHUNK) {
        const int cn = (int)min((int64_t)TIMELINE_SUM_CHUNK, fe - c0);
        // a hop longer than the window leaves gaps: a chunk no window of the tile touches is not read (the same answer in every lane)
        bool used = false;
        for (int w = 0; w < TIMELINE_SUM_WINDOWS; w++) {
            const int64_t b = (j0 + w) * H, e = min(b + W, n);
            used = used || (j0 + w < nw && b < c0 + cn && e > c0);
        }
        if (!used) continue;
        __syncthreads();                                             // the chunk before is read out
        for (int c = wave; c < TIMELINE_SUM_COLS; c += TIMELINE_SUM_WG / 64)
            if (lane < cn && s0 + c < S) lds[lane * TIMELINE_SUM_STRIDE + c] = fll[(int64_t)(s0 + c) * n_total + row0 + c0 + lane];
        __syncthreads();
        if (active) {
            const int lo = (int)(max(wb, c0) - c0), hi = (int)(min(we, c0 + cn) - c0);
            for (int f = lo; f < hi; f++) acc += (double)lds[f * TIMELINE_SUM_STRIDE + lane];
        }
    }
    if (active && s0 + lane < S) sums[(wbase + jw) * S + s0 + lane] = acc;
    if (active && blockIdx.y == 0 && lane == 0) counts[wbase + jw] = (int32_t)(we - wb);
}

// ---- emissions ----

__device__ __forceinline__ double emission(double sum, double dc, bool nobody, double threshold, bool &bad) {
    double q = sum / dc;
    bad = q != q;
    if (bad) q = -INFINITY;
    if (nobody) {
        q = q + threshold;
        if (q != q) q = -INFINITY;                                   // (-inf + an infinite threshold)
    }
    return q;
}

__device__ __forceinline__ void take_first_max(double &v, int &r, double ov, int orank) {
    if (ov > v || (ov == v && orank < r)) {
        v = ov;
        r = orank;
    }
}

constexpr int TIMELINE_RAW_WAVES = 4;

__global__ __launch_bounds__(64 * TIMELINE_RAW_WAVES)
void timeline_raw_kernel(const double *__restrict__ sums, const int32_t *__restrict__ counts, int64_t nw_total, int S, int bg,
                         double threshold, int32_t *__restrict__ raw, int32_t *__restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * TIMELINE_RAW_WAVES + (threadIdx.x >> 6);
    if (j >= nw_total) return;                                       // (whole wave)
    const double dc = (double)counts[j];
    const double *row = sums + j * S;
    double best = -INFINITY;
    int rank = INT_MAX;
    bool any_bad = false;
    for (int s = lane; s < S; s += 64) {
        bool b;
        const double e = emission(row[s], dc, s == bg, threshold, b);
        any_bad = any_bad || b;
        take_first_max(best, rank, e, s == bg ? S : s);
    }
    wave_first_max_f64(best, rank);
    const bool wave_bad = __ballot(any_bad) != 0;
    if (lane == 0) {
        raw[j] = (best == -INFINITY || rank >= S) ? -1 : rank;
        bad[j] = wave_bad ? 1 : 0;
    }
}

// ---- the hold rule, the copy of the raw labels, the NaN count ----

constexpr int TIMELINE_HOLD_WG = 256;

__global__ __launch_bounds__(TIMELINE_HOLD_WG)
void timeline_hold_kernel(const int32_t *__restrict__ raw, const int32_t *__restrict__ bad, const int64_t *__restrict__ win_off, int mode,
                          int32_t *__restrict__ label, int64_t *__restrict__ bad_out) {
    __shared__ int sc[TIMELINE_HOLD_WG];
    const int tid = threadIdx.x;
    const int u = blockIdx.x;
    const int64_t w0 = win_off[u], nw = win_off[u + 1] - w0;
    int64_t carry = -1;                                              // the last anchor of the chunks before
    int cnt = 0;
    for (int64_t base = 0; base < nw; base += TIMELINE_HOLD_WG) {
        const int64_t j = base + tid;
        const bool valid = j < nw;
        const int r = valid ? raw[w0 + j] : -1;
        cnt += valid ? bad[w0 + j] : 0;
        if (mode == TIMELINE_RAW) {
            if (valid) label[w0 + j] = r;
        } else if (mode == TIMELINE_HOLD) {
            const int rp = (valid && j > 0) ? raw[w0 + j - 1] : -1;
            const bool change = valid && j > 0 && r != -1 && rp != -1 && rp != r;
            int a = (valid && !change) ? tid : -1;                   // the anchor inside this chunk: an inclusive maximum-scan
            sc[tid] = a;
            __syncthreads();
            for (int d = 1; d < TIMELINE_HOLD_WG; d <<= 1) {
                const int v = tid >= d ? sc[tid - d] : -1;
                __syncthreads();
                a = max(a, v);
                sc[tid] = a;
                __syncthreads();
            }
            const int last = sc[TIMELINE_HOLD_WG - 1];
            const int64_t anchor = a >= 0 ? base + a : carry;        // (window 0 is always an anchor: never -1 for a valid j)
            if (valid) label[w0 + j] = raw[w0 + anchor];
            if (last >= 0) carry = base + last;
            __syncthreads();                                         // sc is rewritten by the next chunk
        }
    }
    // the count: a fixed tree over the workgroup (integers)
    __syncthreads();
    sc[tid] = cnt;
    __syncthreads();
    for (int d = TIMELINE_HOLD_WG / 2; d > 0; d >>= 1) {
        if (tid < d) sc[tid] += sc[tid + d];
        __syncthreads();
    }
    if (tid == 0) bad_out[u] = sc[0];
}

// ---- Viterbi forward ----

struct ForwardArgs {
    const double *sums;         // [Nw_total][S]
    const int32_t *counts;      // [Nw_total]
    const int64_t *win_off;     // [U + 1]
    uint64_t *stay;             // [Nw_total][words]
    int32_t *enter_arg;         // [Nw_total]
    double *chain_g;            // [U][m - 1][s_pad] when the ring does not fit LDS
    int32_t *end_state;         // [U][2]: state, k
    double *path;               // [U]
    double threshold, beta;
    int S, bg, m, words, s_pad, chain_lds;
};

// the workgroup's first maximum of (v, r): every lane gets it.  MULTI: through LDS, slot `par`; one barrier.
template <bool MULTI>
__device__ __forceinline__ void wg_first_max(double &v, int &r, double *red_v, int *red_r, int par, int wave, int lane, int n_waves) {
    wave_first_max_f64(v, r);
    if (MULTI) {
        if (lane == 0) {
            red_v[par * 16 + wave] = v;
            red_r[par * 16 + wave] = r;
        }
        __syncthreads();
        v = red_v[par * 16];
        r = red_r[par * 16];
        for (int w = 1; w < n_waves; w++) take_first_max(v, r, red_v[par * 16 + w], red_r[par * 16 + w]);
    }
}

template <int NS, int TILE, bool MULTI>
__global__ __launch_bounds__(MULTI ? 1024 : 64)
void timeline_forward_kernel(ForwardArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds_d[];
    double *red_v = lds_d;                                           // [2][16]
    int *red_r = reinterpret_cast<int *>(lds_d + 32);                // [2][16]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
    const int u = blockIdx.x;
    const int64_t w0 = a.win_off[u];
    const int64_t nw = a.win_off[u + 1] - w0;
    const int m = a.m, S = a.S, slots = m - 1;
    if (nw <= 0) {                                                   // (the whole workgroup)
        if (tid == 0) {
            a.path[u] = 0.0;
            a.end_state[2 * u] = 0;
            a.end_state[2 * u + 1] = 0;
        }
        return;
    }
    double *chain = a.chain_lds ? lds_d + TIMELINE_RED_DOUBLES : a.chain_g + (int64_t)u * (slots > 0 ? slots : 0) * a.s_pad;

    int st[NS], rank[NS];
    bool valid[NS];
    double dm[NS], c1[NS];
#pragma unroll
    for (int i = 0; i < NS; i++) {
        st[i] = i * (int)blockDim.x + tid;
        valid[i] = st[i] < S;
        rank[i] = !valid[i] ? INT_MAX : st[i] == a.bg ? S : st[i];
        dm[i] = -INFINITY;
        c1[i] = -INFINITY;
    }
    // A tile of windows ahead of the step: the sums and counts are loaded a tile early and turned into emissions (the division,
    // the NaN and nobody rules) when the tile before is done -- neither a load nor the division sits in the chain of steps.
    double cur[NS][TILE], nxt[NS][TILE];
    int nxt_cnt[TILE];
    auto load = [&](double (&dst)[NS][TILE], int (&cnt)[TILE], int64_t j0) {
#pragma unroll
        for (int t = 0; t < TILE; t++) {
            cnt[t] = j0 + t < nw ? a.counts[w0 + j0 + t] : 1;
#pragma unroll
            for (int i = 0; i < NS; i++) dst[i][t] = (j0 + t < nw && valid[i]) ? a.sums[(w0 + j0 + t) * S + st[i]] : 0.0;
        }
    };
    auto to_emissions = [&](double (&v)[NS][TILE], const int (&cnt)[TILE]) {
#pragma unroll
        for (int t = 0; t < TILE; t++)
#pragma unroll
            for (int i = 0; i < NS; i++) {
                bool b;
                v[i][t] = valid[i] ? emission(v[i][t], (double)cnt[t], st[i] == a.bg, a.threshold, b) : -INFINITY;
            }
    };
    load(cur, nxt_cnt, 0);
    to_emissions(cur, nxt_cnt);
    int h = 0;                                                       // the ring: d(s, k) sits in slot (h + k - 1) mod (m - 1)
    int red = 0;                                                     // reductions so far: the LDS slot alternates
    for (int64_t j0 = 0; j0 < nw; j0 += TILE) {
        load(nxt, nxt_cnt, j0 + TILE);
#pragma unroll
        for (int t = 0; t < TILE; t++) {
            const int64_t j = j0 + t;
            if (j >= nw) break;
            if (j == 0) {
#pragma unroll
                for (int i = 0; i < NS; i++) {
                    const double e = cur[i][t];
                    if (m == 1) dm[i] = e;
                    else if (m == 2) c1[i] = e;
                    else if (valid[i]) {
                        chain[st[i]] = e;
                        for (int k = 1; k < slots; k++) chain[k * a.s_pad + st[i]] = -INFINITY;
                    }
                }
                continue;
            }
            double bv = -INFINITY;
            int br = INT_MAX;
#pragma unroll
            for (int i = 0; i < NS; i++) take_first_max(bv, br, dm[i], rank[i]);
            wg_first_max<MULTI>(bv, br, red_v, red_r, red & 1, wave, lane, n_waves);
            red++;
            const double enter = bv - a.beta;
            // (br is a state's rank unless a NaN -- emissions of +inf, outside the contract -- kept every state out: then state 0)
            if (tid == 0) a.enter_arg[w0 + j] = br < S ? br : br == S ? a.bg : 0;
            const int slot_last = m > 2 ? (h + m - 2) % slots : 0;
#pragma unroll
            for (int i = 0; i < NS; i++) {
                bool stay = false;
                const double e = cur[i][t];
                if (m == 1) {
                    stay = dm[i] >= enter;
                    dm[i] = e + (stay ? dm[i] : enter);
                } else if (m == 2) {
                    stay = dm[i] >= c1[i];
                    dm[i] = e + (stay ? dm[i] : c1[i]);
                    c1[i] = e + enter;
                } else if (valid[i]) {
                    const double cl = chain[slot_last * a.s_pad + st[i]];
                    stay = dm[i] >= cl;
                    dm[i] = e + (stay ? dm[i] : cl);
                    for (int k = 0; k < slots; k++)
                        if (k != slot_last) chain[k * a.s_pad + st[i]] = e + chain[k * a.s_pad + st[i]];
                    chain[slot_last * a.s_pad + st[i]] = e + enter;
                }
                const uint64_t word = __ballot(stay && valid[i]);
                const int wi = i * n_waves + wave;
                if (lane == 0 && wi < a.words) a.stay[(w0 + j) * a.words + wi] = word;
            }
            if (m > 2) h = slot_last;
        }
        to_emissions(nxt, nxt_cnt);
#pragma unroll
        for (int t = 0; t < TILE; t++)
#pragma unroll
            for (int i = 0; i < NS; i++) cur[i][t] = nxt[i][t];
    }
    // the end state: the first maximum over (s, k), k from m down to 1, the priority order inside a k; a later k wins only when above
    double best = 0.0;
    int best_r = 0, best_k = 0;
    for (int k = m; k >= 1; k--) {
        double bv = -INFINITY;
        int br = INT_MAX;
#pragma unroll
        for (int i = 0; i < NS; i++) {
            double v = -INFINITY;
            if (valid[i]) v = k == m ? dm[i] : m == 2 ? c1[i] : chain[((h + k - 1) % slots) * a.s_pad + st[i]];
            take_first_max(bv, br, v, rank[i]);
        }
        wg_first_max<MULTI>(bv, br, red_v, red_r, red & 1, wave, lane, n_waves);
        red++;
        if (k == m || bv > best) {
            best = bv;
            best_r = br;
            best_k = k;
        }
    }
    if (tid == 0) {
        a.path[u] = best;
        a.end_state[2 * u] = best_r < S ? best_r : best_r == S ? a.bg : 0;
        a.end_state[2 * u + 1] = best_k;
    }
}

// ---- traceback ----

__global__ __launch_bounds__(64)
void timeline_trace_kernel(int U, const int64_t *__restrict__ win_off, const uint64_t *__restrict__ stay, const int32_t *__restrict__ enter_arg,
                           const int32_t *__restrict__ end_state, int m, int bg, int words, int32_t *__restrict__ label) {
    const int u = blockIdx.x * 64 + threadIdx.x;
    if (u >= U) return;
    const int64_t w0 = win_off[u], nw = win_off[u + 1] - w0;
    if (nw <= 0) return;
    int s = end_state[2 * u], k = end_state[2 * u + 1];
    for (int64_t j = nw - 1; j >= 0; j--) {
        label[w0 + j] = s == bg ? -1 : s;
        if (j == 0) break;
        if (k == m) {
            const bool stayed = (stay[(w0 + j) * words + (s >> 6)] >> (s & 63)) & 1;
            if (!stayed) {
                if (m == 1) s = enter_arg[w0 + j];
                else k = m - 1;
            }
        } else if (k > 1) {
            k--;
        } else {
            s = enter_arg[w0 + j];
            k = m;
        }
    }
}

struct TimelineWs {
    DevBuf<double> sums, path, chain;
    DevBuf<int32_t> counts, raw, bad, label, enter_arg, end_state, tiles;
    DevBuf<int64_t> win_off, bad_count;
    DevBuf<uint64_t> stay;
    PinnedBuf<int32_t> h_label;
    PinnedBuf<double> h_path;
    PinnedBuf<int64_t> h_bad;
};

// The decision kernels over sums, counts and window offsets that sit in the workspace; results to the host in one wait.
void decide_device(TimelineWs &w, int U, int S, int64_t nw_total, const TimelineRule &rule, int *label_out, double *path_out, int64_t *bad_out,
                   double *sums_out) {
    hipStream_t st = ctx().stream;
    TimelinePlan pl;
    std::string why;
    if (!plan_timeline(S, rule.min_dur, 0, 1, 1, pl, why)) fail("timeline: %s", why.c_str());
    const size_t nwt = (size_t)std::max<int64_t>(1, nw_total);
    w.raw.ensure(nwt);
    w.bad.ensure(nwt);
    w.label.ensure(nwt);
    w.bad_count.ensure((size_t)std::max(1, U));
    w.path.ensure((size_t)std::max(1, U));
    w.h_label.ensure(nwt);
    w.h_path.ensure((size_t)std::max(1, U));
    w.h_bad.ensure((size_t)std::max(1, U));
    if (U > 0) {
        {
            ScopedKernelTimer tm(T_SCORE_REF);
            if (nw_total > 0)
                hipLaunchKernelGGL(timeline_raw_kernel, dim3((unsigned)((nw_total + TIMELINE_RAW_WAVES - 1) / TIMELINE_RAW_WAVES)),
                                   dim3(64 * TIMELINE_RAW_WAVES), 0, st, w.sums.p, w.counts.p, nw_total, S, rule.bg, rule.threshold, w.raw.p, w.bad.p);
            hipLaunchKernelGGL(timeline_hold_kernel, dim3((unsigned)U), dim3(TIMELINE_HOLD_WG), 0, st, w.raw.p, w.bad.p, w.win_off.p, rule.mode,
                               w.label.p, w.bad_count.p);
            if (rule.mode == TIMELINE_VITERBI) {
                w.stay.ensure(nwt * pl.words);
                w.enter_arg.ensure(nwt);
                w.end_state.ensure(2 * (size_t)U);
                if (pl.chain_slots > 0 && !pl.chain_lds) w.chain.ensure((size_t)U * pl.chain_slots * pl.s_pad);
                ForwardArgs a;
                a.sums = w.sums.p;
                a.counts = w.counts.p;
                a.win_off = w.win_off.p;
                a.stay = w.stay.p;
                a.enter_arg = w.enter_arg.p;
                a.chain_g = w.chain.p;
                a.end_state = w.end_state.p;
                a.path = w.path.p;
                a.threshold = rule.threshold;
                a.beta = rule.beta;
                a.S = S; a.bg = rule.bg; a.m = rule.min_dur; a.words = pl.words; a.s_pad = pl.s_pad; a.chain_lds = pl.chain_lds ? 1 : 0;
                const dim3 grid((unsigned)U), wg((unsigned)pl.lanes);
                if (pl.variant == 0)
                    hipLaunchKernelGGL((timeline_forward_kernel<1, TIMELINE_TILE, false>), grid, wg, pl.fwd_lds_bytes, st, a);
                else if (pl.variant == 1)
                    hipLaunchKernelGGL((timeline_forward_kernel<1, TIMELINE_TILE, true>), grid, wg, pl.fwd_lds_bytes, st, a);
                else
                    hipLaunchKernelGGL((timeline_forward_kernel<TIMELINE_LOOP_STATES, TIMELINE_TILE_LOOP, true>), grid, wg, pl.fwd_lds_bytes, st, a);
            }
        }
        if (rule.mode == TIMELINE_VITERBI) {
            ScopedKernelTimer tm(T_ESTEP);
            hipLaunchKernelGGL(timeline_trace_kernel, dim3((unsigned)((U + 63) / 64)), dim3(64), 0, st, U, w.win_off.p, w.stay.p, w.enter_arg.p,
                               w.end_state.p, rule.min_dur, rule.bg, pl.words, w.label.p);
        }
        SR_HIP(hipGetLastError());
        if (nw_total > 0) SR_HIP(hipMemcpyAsync(w.h_label.p, w.label.p, (size_t)nw_total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        SR_HIP(hipMemcpyAsync(w.h_bad.p, w.bad_count.p, (size_t)U * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        if (rule.mode == TIMELINE_VITERBI) SR_HIP(hipMemcpyAsync(w.h_path.p, w.path.p, (size_t)U * sizeof(double), hipMemcpyDeviceToHost, st));
        if (sums_out && nw_total > 0) w.sums.download(sums_out, (size_t)nw_total * S);
    }
    sync_stream();
    if (nw_total > 0) std::memcpy(label_out, w.h_label.p, (size_t)nw_total * sizeof(int32_t));
    for (int u = 0; u < U; u++) {
        if (bad_out) bad_out[u] = w.h_bad.p[u];
        if (path_out) path_out[u] = rule.mode == TIMELINE_VITERBI ? w.h_path.p[u] : (double)NAN;
    }
}

}  // namespace

void timeline_decide_host(const double *sums, const int32_t *counts, const int64_t *win_off, int U, int S, const TimelineRule &rule,
                          int *label_out, double *path_out, int64_t *bad_out) {
    ensure_device();
    auto &w = per_device<TimelineWs>();
    const int64_t nw_total = win_off[U];
    w.sums.upload(sums, (size_t)nw_total * S);
    w.counts.upload(counts, (size_t)nw_total);
    w.win_off.upload(win_off, (size_t)U + 1);
    decide_device(w, U, S, nw_total, rule, label_out, path_out, bad_out, nullptr);
}

void timeline_from_frames(const float *d_fll, SRBatch &feat, int S, int window, int hop, const TimelineRule &rule, int64_t *win_off_out,
                          int *label_out, double *sums_out, double *path_out, int64_t *bad_out) {
    const int U = feat.n_utt;
    std::vector<int64_t> win_off((size_t)U + 1, 0), utt_tile((size_t)U + 1, 0);
    for (int u = 0; u < U; u++) {
        const int64_t nw = timeline_windows(feat.offsets[u + 1] - feat.offsets[u], window, hop);
        win_off[u + 1] = win_off[u] + nw;
        utt_tile[u + 1] = utt_tile[u] + (nw + TIMELINE_SUM_WINDOWS - 1) / TIMELINE_SUM_WINDOWS;
    }
    const int64_t nw_total = win_off[U], n_tiles = utt_tile[U];
    if (nw_total > INT32_MAX / 2) fail("timeline: %lld windows in one call (at most 2^30: split the batch)", (long long)nw_total);
    std::vector<int32_t> tiles(2 * (size_t)n_tiles);
    for (int u = 0; u < U; u++)
        for (int64_t k = 0; k < utt_tile[u + 1] - utt_tile[u]; k++) {
            tiles[(size_t)(utt_tile[u] + k)] = u;
            tiles[(size_t)(n_tiles + utt_tile[u] + k)] = (int32_t)(k * TIMELINE_SUM_WINDOWS);
        }
    auto &w = per_device<TimelineWs>();
    w.win_off.upload(win_off.data(), win_off.size());
    w.sums.ensure((size_t)std::max<int64_t>(1, nw_total) * S);
    w.counts.ensure((size_t)std::max<int64_t>(1, nw_total));
    if (n_tiles > 0) {
        if (!d_fll) fail("timeline: the scoring pass left no per-frame matrix");
        w.tiles.upload(tiles.data(), tiles.size());
        ScopedKernelTimer tm(T_CMVN);
        hipLaunchKernelGGL(timeline_sum_kernel, dim3((unsigned)n_tiles, (unsigned)((S + TIMELINE_SUM_COLS - 1) / TIMELINE_SUM_COLS)),
                           dim3(TIMELINE_SUM_WG), 0, ctx().stream, d_fll, feat.n_rows, feat.d_offsets.p, w.win_off.p, w.tiles.p,
                           w.tiles.p + n_tiles, S, (int64_t)window, (int64_t)hop, w.sums.p, w.counts.p);
        SR_HIP(hipGetLastError());
    }
    if (win_off_out) std::copy(win_off.begin(), win_off.end(), win_off_out);
    // (decide_device waits for the stream before it returns: `tiles` and `win_off` outlive their uploads)
    decide_device(w, U, S, nw_total, rule, label_out, path_out, bad_out, sums_out);
}

}  // namespace sr
