// map_batch.hip -- a set of speakers MAP-adapted from ONE UBM in one batched device fit (sr_map_fit_batch): every speaker the model
// bits and the iteration count of its single fit (train_em -> train_em_f64, em_f64.hip), whatever the batch around it.
//
// Why: enrolment was a loop of single fits -- per speaker an upload and four to six launches per iteration whose grids are far below
// the chip (3000 frames against 512 mixtures: 24 x 8 density workgroups on 256 compute units), the host waiting for 16 bytes every
// second pass.  Here a launch carries a whole group of speakers: its grid's x walks a table of {speaker, first row, local tile} rows
// (map_plan.cpp), the workgroup's speaker and tile come from its row, and the element arithmetic is em_f64.hip's own -- the same
// __device__ bodies (em_f64_dev.hpp), tiles and chunks counted from the speaker's own first frame, so every sum has the single fit's
// order.  sigma, the weights, 1 / (2 sigma^2), the mixtures' constants and the UBM's means are ONE copy for the call; per speaker
// there are its means and its scratch slices.
//
//   mapb_density / mapb_lse / mapb_stats   e64_density / _lse / _stats for the row's speaker
//   mapb_head    per speaker: the pass's total and flag, then the stop rule of gmm.cc:622-650 as train_em_f64 applies it on the
//                host -- the total under the model of iteration it - 1 read on pass it at odd it - 1 -- applied on the device: a
//                speaker that meets it clears `active` BEFORE that pass's M-step (its model stays as iteration it - 1 left it);
//                the speakers still active are counted into one word per pass
//   mapb_mstep   e64_mstep for every active speaker
// Workgroups of an inactive speaker return after reading its state.  The host reads the pass's count where the rule is taken (every
// second pass) and stops launching at 0.  A speaker whose flag rose (a live frame within E64_BAND of the underflow boundary, a NaN
// density) freezes and is refitted alone by train_em afterwards: the iteration-at-a-time path, as its single fit takes it.
#include "score.hpp"
#include "em.hpp"
#include "em_f64_dev.hpp"
#include "map_batch.hpp"
#include "map_plan.hpp"
#include "ref_rand.hpp"

#include "../../include/pygmm_hip.h"

#include <atomic>
#include <cfloat>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

namespace sr {

namespace {

// a speaker of the group on the device: where its frames and its slices of the group's scratch are (offsets in doubles)
struct MapbSpk {
    int64_t first;
    int32_t n, n_pad, n_chunks, pad;
    int64_t off_mu, off_L, off_mb, off_sb, off_llf, off_partial, off_llpart;
};

struct MapbArgs {
    const float *X;                    // the call's frames
    int dim, K, n_kb, n_spk;
    double *w, *sg, *h, *c;            // the call's one copy: [K], [K][D], 1 / (2 sigma^2), ln w - sum ln(sqrt(2 pi) sigma)
    const double *ubm_mu;              // [K][D]
    double *scratch;                   // the group's: means [n_spk][K][D], states [n_spk][MAP_STATE], then the speakers' slices
    double *state;                     // = scratch + n_spk K D: {last_ll, active, done_it, flag} per speaker
    const MapbSpk *spk;                // [n_spk]
    const MapTileRow *tiles, *chunks;  // the group's rows
    int *active;                       // [nit + 1] speakers still active after pass it
    double relevance, threshold;
    int it, nit;
};

__device__ __forceinline__ bool mapb_active(const MapbArgs &b, int slot) { return b.state[(size_t)slot * MAP_STATE + 1] != 0.0; }

// the speaker's fit as em_f64.hip's bodies see one
__device__ __forceinline__ E64Args mapb_view(const MapbArgs &b, int slot) {
    const MapbSpk s = b.spk[slot];
    E64Args a;
    a.X = b.X + (size_t)s.first * b.dim;
    a.n = s.n;
    a.n_pad = s.n_pad;
    a.dim = b.dim;
    a.K = b.K;
    a.n_chunks = s.n_chunks;
    a.n_kb = b.n_kb;
    a.map = 1;
    a.w = b.w;
    a.mu = b.scratch + s.off_mu;
    a.sg = b.sg;
    a.h = b.h;
    a.c = b.c;
    a.ubm_mu = b.ubm_mu;
    a.L = b.scratch + s.off_L;
    a.mb = b.scratch + s.off_mb;
    a.sb = b.scratch + s.off_sb;
    a.llf = b.scratch + s.off_llf;
    a.partial = b.scratch + s.off_partial;
    a.llpart = b.scratch + s.off_llpart;
    a.head = nullptr;
    a.min_sigma = 0.0;
    a.relevance = b.relevance;
    return a;
}

// the call's constants from the UBM's weights and sigmas (e64_derive_kernel's arithmetic)
__global__ __launch_bounds__(256)
void mapb_derive_kernel(const MapbArgs b) {
    E64Args a = {};
    a.dim = b.dim;
    a.K = b.K;
    a.w = b.w;
    a.sg = b.sg;
    a.h = b.h;
    a.c = b.c;
    e64_derive_body(a, 3, blockIdx.x * 256 + threadIdx.x);
}

// every speaker of the group starts from the UBM's means (gmm_replace_with, gmmubm.cc:29-38), active, nothing read yet
__global__ __launch_bounds__(256)
void mapb_init_kernel(const MapbArgs b) {
    const int i = blockIdx.x * 256 + threadIdx.x, slot = blockIdx.y;
    if (i < b.K * b.dim) b.scratch[b.spk[slot].off_mu + i] = b.ubm_mu[i];
    if (i == 0) {
        double *st = b.state + (size_t)slot * MAP_STATE;
        st[0] = -DBL_MAX;
        st[1] = 1.0;
        st[2] = (double)b.nit;
        st[3] = 0.0;
    }
}

__global__ __launch_bounds__(E64_THREADS)
void mapb_density_kernel(const MapbArgs b) {
    extern __shared__ __attribute__((aligned(16))) double e64_lds[];
    const MapTileRow t = b.tiles[blockIdx.x];
    if (!mapb_active(b, t.slot)) return;
    const E64Args a = mapb_view(b, t.slot);
    e64_density_body(a, e64_lds, t.local, blockIdx.y);
}

__global__ __launch_bounds__(256)
void mapb_lse_kernel(const MapbArgs b) {
    const MapTileRow t = b.chunks[blockIdx.x];
    if (!mapb_active(b, t.slot)) return;
    const E64Args a = mapb_view(b, t.slot);
    e64_lse_body(a, t.local);
}

__global__ __launch_bounds__(E64_STHREADS)
void mapb_stats_kernel(const MapbArgs b) {
    extern __shared__ __attribute__((aligned(16))) double e64_lds[];
    const MapTileRow t = b.chunks[blockIdx.x];
    if (!mapb_active(b, t.slot)) return;
    const E64Args a = mapb_view(b, t.slot);
    e64_stats_body(a, e64_lds, t.local, blockIdx.y);
}

// One wave per speaker: the pass's total and flag (e64_head_kernel's sums), then train_em_f64's host logic for this pass.
__global__ __launch_bounds__(64)
void mapb_head_kernel(const MapbArgs b) {
    const int slot = blockIdx.x;
    if (!mapb_active(b, slot)) return;
    const E64Args a = mapb_view(b, slot);
    double ll, bad;
    e64_head_sums(a, ll, bad);
    if (threadIdx.x != 0) return;
    double *st = b.state + (size_t)slot * MAP_STATE;
    const double flag = st[3] + bad;
    st[3] = flag;
    bool active = true;
    if (flag > 0.0) {
        active = false;                                          // frozen: the iteration-at-a-time path refits it
    } else {
        // the total under the model as iteration it - 1 left it: the reference takes it after odd iterations (gmm.cc:622-650)
        if (b.it >= 1 && ((b.it - 1) & 1)) {
            const double ll_diff = ll - st[0];
            if (fabs(ll_diff) / fabs(ll) < b.threshold && ll_diff < b.threshold) {
                st[2] = (double)b.it;
                active = false;
            } else {
                st[0] = ll;
            }
        }
        if (b.it == b.nit) active = false;                       // (the total-only pass after an odd last iteration)
    }
    if (active) atomicAdd(b.active + b.it, 1);
    else st[1] = 0.0;
}

__global__ __launch_bounds__(256)
void mapb_mstep_kernel(const MapbArgs b) {
    const int slot = blockIdx.y;
    if (!mapb_active(b, slot)) return;
    const E64Args a = mapb_view(b, slot);
    e64_mstep_body(a, blockIdx.x * 256 + threadIdx.x);
}

struct MapbWorkspace {
    DevBuf<float> X;
    DevBuf<double> model, scratch;
    DevBuf<MapbSpk> spk;
    DevBuf<MapTileRow> tiles, chunks;
    DevBuf<int> active;
    PinnedBuf<double> h_out;
    PinnedBuf<int> h_active;
};

std::atomic<long> g_calls{0}, g_batched{0}, g_single{0}, g_handed{0}, g_passes{0};
std::atomic<long> g_scratch_bytes{(long)MAP_DEFAULT_SCRATCH};

}  // namespace

void set_map_fit_batch_bytes(long v) { g_scratch_bytes.store(v); }
long map_fit_batch_bytes() { return g_scratch_bytes.load(); }

void map_fit_batch_stats(long *calls, long *speakers_batched, long *speakers_single, long *speakers_handed_over, long *passes) {
    if (calls) *calls = g_calls.load();
    if (speakers_batched) *speakers_batched = g_batched.load();
    if (speakers_single) *speakers_single = g_single.load();
    if (speakers_handed_over) *speakers_handed_over = g_handed.load();
    if (passes) *passes = g_passes.load();
}

// The arguments have been checked (abi_stats.cpp).  status / iterations_out / messages: [S]; -> the number of speakers fitted.
int map_fit_batch(GMM *const *models, int S, const GMM *ubm, const float *X, const int64_t *row_offsets, int dim, const Parameter &param,
                  long seed, int *iterations_out, int *status, std::vector<std::string> &messages) {
    ensure_device();
    const int K = ubm->nr_mixtures, KD = K * dim;
    std::vector<int64_t> lengths((size_t)S);
    for (int s = 0; s < S; s++) lengths[(size_t)s] = row_offsets[s + 1] - row_offsets[s];
    MapPlan plan;
    std::string why;
    if (!plan_map_batch(K, dim, lengths.data(), S, param, map_fit_batch_bytes(), ctx().n_cu, plan, why)) fail("%s", why.c_str());
    // the whole call through single fits: the progress lines, the reference's side effects and a forced engine are the single path's
    const bool all_single = param.verbosity >= 1 || reference_side_effects() || em_stats_engine() != 0;
    if (all_single) {
        for (int s : plan.batched) plan.speakers[(size_t)s].route = MAP_ROUTE_SINGLE;
        plan.batched.clear();
        plan.groups.clear();
    }
    g_calls++;
    messages.assign((size_t)S, std::string());
    for (int s = 0; s < S; s++) {
        status[s] = -1;
        iterations_out[s] = 0;
    }
    int fitted = 0;
    std::vector<int> later;                     // the speakers the single fit serves: routed there, or handed over
    for (int s = 0; s < S; s++)
        if (plan.speakers[(size_t)s].route == MAP_ROUTE_SINGLE) later.push_back(s);

    if (!plan.batched.empty()) {
        auto &w = per_device<MapbWorkspace>();
        hipStream_t st = ctx().stream;
        const double relevance = 16.0;          // gmm.hh:118-120
        const int nit = param.nr_iteration;
        MapbArgs b;
        b.dim = dim;
        b.K = K;
        b.n_kb = plan.n_kb;
        b.relevance = relevance;
        b.threshold = param.threshold;
        b.nit = nit;
        // the frames of all speakers: ONE upload
        w.X.upload(X, (size_t)row_offsets[S] * dim);
        b.X = w.X.p;
        // the call's model block: w [K], sg [KD], ubm mu [KD], h [KD], c [K]
        std::vector<double> init((size_t)K + 2 * (size_t)KD);
        for (int k = 0; k < K; k++) init[(size_t)k] = ubm->weights[(size_t)k];
        for (int i = 0; i < KD; i++) {
            init[(size_t)K + i] = ubm->sigma[(size_t)i];
            init[(size_t)K + KD + i] = ubm->mean[(size_t)i];
        }
        w.model.ensure((size_t)2 * K + 3 * (size_t)KD);
        b.w = w.model.p;
        b.sg = b.w + K;
        double *ubm_mu = b.sg + KD;
        b.ubm_mu = ubm_mu;
        b.h = ubm_mu + KD;
        b.c = b.h + KD;
        SR_HIP(hipMemcpyAsync(b.w, init.data(), init.size() * sizeof(double), hipMemcpyHostToDevice, st));
        const unsigned g_kd = (unsigned)((KD + 255) / 256);
        b.n_spk = 0;
        b.scratch = b.state = nullptr;
        b.spk = nullptr;
        b.tiles = b.chunks = nullptr;
        b.active = nullptr;
        b.it = 0;
        hipLaunchKernelGGL(mapb_derive_kernel, dim3(g_kd), dim3(256), 0, st, b);
        const size_t lds_a = plan.lds_density, lds_b = plan.lds_stats;
        if (lds_a > 64 * 1024)
            SR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&mapb_density_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_a));
        if (lds_b > 64 * 1024)
            SR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&mapb_stats_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
        w.active.ensure((size_t)nit + 1);
        w.h_active.ensure(1);
        b.active = w.active.p;
        std::vector<MapbSpk> spk;
        for (const MapGroupPlan &g : plan.groups) {
            spk.resize((size_t)g.count);
            for (int i = 0; i < g.count; i++) {
                const MapSpeakerPlan &sp = plan.speakers[(size_t)plan.batched[(size_t)g.first + i]];
                spk[(size_t)i] = MapbSpk{sp.first, (int32_t)sp.n, sp.n_pad, sp.n_chunks, 0, sp.off_mu, sp.off_L, sp.off_mb, sp.off_sb,
                                         sp.off_llf, sp.off_partial, sp.off_llpart};
            }
            w.scratch.ensure((size_t)(g.scratch_bytes / (int64_t)sizeof(double)));
            w.spk.upload(spk.data(), spk.size());
            w.tiles.upload(plan.tiles.data() + g.tile0, (size_t)g.n_tiles);
            w.chunks.upload(plan.chunks.data() + g.chunk0, (size_t)g.n_chunks);
            SR_HIP(hipMemsetAsync(w.active.p, 0, ((size_t)nit + 1) * sizeof(int), st));
            b.n_spk = g.count;
            b.scratch = w.scratch.p;
            b.state = b.scratch + (size_t)g.count * KD;
            b.spk = w.spk.p;
            b.tiles = w.tiles.p;
            b.chunks = w.chunks.p;
            b.it = 0;
            hipLaunchKernelGGL(mapb_init_kernel, dim3(g_kd, (unsigned)g.count), dim3(256), 0, st, b);
            const dim3 grid_a((unsigned)g.n_tiles, (unsigned)plan.n_kb), grid_b((unsigned)g.n_chunks, (unsigned)plan.n_kb);
            for (int it = 0;; it++) {
                const bool ll_only = it == nit;            // the total after the LAST iteration, when that one is an odd one (gmm.cc:622)
                if (ll_only && ((nit - 1) & 1) == 0) break;
                b.it = it;
                {
                    ScopedKernelTimer t(T_ESTEP);
                    hipLaunchKernelGGL(mapb_density_kernel, grid_a, dim3(E64_THREADS), lds_a, st, b);
                    hipLaunchKernelGGL(mapb_lse_kernel, dim3((unsigned)g.n_chunks), dim3(256), 0, st, b);
                    hipLaunchKernelGGL(mapb_stats_kernel, grid_b, dim3(E64_STHREADS), lds_b, st, b);
                    hipLaunchKernelGGL(mapb_head_kernel, dim3((unsigned)g.count), dim3(64), 0, st, b);
                }
                SR_HIP(hipGetLastError());
                g_passes++;
                if (ll_only) break;
                // one word, where the rule is taken: the speakers still active after this pass
                if (it >= 1 && ((it - 1) & 1)) {
                    SR_HIP(hipMemcpyAsync(w.h_active.p, w.active.p + it, sizeof(int), hipMemcpyDeviceToHost, st));
                    sync_stream();
                    if (w.h_active.p[0] == 0) break;
                }
                ScopedKernelTimer t(T_ESTEP);
                hipLaunchKernelGGL(mapb_mstep_kernel, dim3(g_kd, (unsigned)g.count), dim3(256), 0, st, b);
            }
            // the group's means and states: ONE download
            const size_t n_out = (size_t)g.count * ((size_t)KD + MAP_STATE);
            w.h_out.ensure(n_out);
            SR_HIP(hipMemcpyAsync(w.h_out.p, w.scratch.p, n_out * sizeof(double), hipMemcpyDeviceToHost, st));
            sync_stream();
            for (int i = 0; i < g.count; i++) {
                const int s = plan.batched[(size_t)g.first + i];
                const double *state = w.h_out.p + (size_t)g.count * KD + (size_t)i * MAP_STATE;
                if (state[3] > 0.0) {
                    later.push_back(s);
                    continue;
                }
                GMM &gmm = *models[s];
                gmm.nr_mixtures = K;                         // gmm_replace_with, gmmubm.cc:29-38
                gmm.dim = dim;
                gmm.weights = ubm->weights;
                gmm.sigma = ubm->sigma;
                gmm.mean.assign(w.h_out.p + (size_t)i * KD, w.h_out.p + (size_t)(i + 1) * KD);
                gmm.drop_single();
                if (seed < 0) burn_reference_rand(1 + K);   // the legacy symbol: keep libc's stream in step with the reference
                iterations_out[s] = (int)state[2];
                status[s] = 0;
                fitted++;
                g_batched++;
            }
        }
    }

    // the single fit's speakers, each alone: one that fails fails alone
    for (int s : later) {
        const MapSpeakerPlan &sp = plan.speakers[(size_t)s];
        const bool handed = sp.route == MAP_ROUTE_BATCHED;
        try {
            iterations_out[s] = train_em(*models[s], ubm, X + (size_t)sp.first * dim, (long)sp.n, dim, param, seed);
            status[s] = handed ? 2 : 1;
            fitted++;
            (handed ? g_handed : g_single)++;
        } catch (const std::exception &e) {
            status[s] = -1;
            messages[(size_t)s] = e.what();
        }
    }
    for (int s = 0; s < S; s++)
        if (plan.speakers[(size_t)s].route == MAP_ROUTE_ERROR) messages[(size_t)s] = "X.size() == 0";        // gmm.cc:582-586, train_em's
    return fitted;
}

}  // namespace sr
