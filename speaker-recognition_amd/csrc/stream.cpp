// stream.cpp -- fixed-shape serving session (BASELINE configs[4]: 1 s windows of 8 kHz audio):
// `n_windows` windows of `window_samples` samples per tick -> MFCC -> CMVN(/deltas) -> speaker set ->
// decision per window.  Two slots of pinned host + device buffers and a second HIP stream: the H2D
// copy of tick i+1 runs while the kernels of tick i do (hipStream double buffering); results come
// back through pinned memory; the host only waits in sr_stream_collect.
// With SR_STREAM_GRAPH the per-tick device work (4 kernels + 2 result copies) is captured once per
// slot into a hipGraph and replayed with one hipGraphLaunch: the tick is launch-bound at small
// n_windows.  The graph holds raw pointers into the library's cached workspaces, so it is
// re-captured whenever any of them was reallocated or rewritten since (g_devbuf_epoch).
// sr_stream_create_full serves a full-covariance set (SRFullSet) instead: the tick is MFCC (+ LPC columns or deltas) -> scoring
// -> fullcov_finalize_kernel -> one copy of the sums with the argmax values behind them.  Its log-sum-exp is exact (no saturation,
// no partial-product band): nothing of such a tick is ever scored again at collect, and it touches none of the diagonal pass
// counters.
// sr_stream_create_vad puts the reference's voice-activity front end in front of either tick (its conversation loop --
// gui.py:179-214 -- is ModelInterface.filter, then predict, per polled window): ltsd_amp_kernel -> ltsd_reduce_kernel ->
// vad_compact_kernel (ltsd.hip: Schmitt rule, one-third rule, voiced samples to the front of the window's slot in a second PCM
// buffer, voiced length L and frame count T to device tables) -> the feature kernels over the fixed slots -> CMVN over each slot's
// first T rows (zeros behind them) -> scoring of every row -> fullcov_finalize_kernel over each slot's first T rows -> one copy of
// sums, argmax and voiced counts.  Launches only: no sample comes back, no offset is rebuilt on the host, so the tick replays from a
// graph like the others.  A full-covariance VAD tick is final as it arrives.  A diagonal one runs the scoring pass for its
// per-frame values and sums them with that same kernel (the engines' own per-utterance sums cover the padding rows too and are
// not used); when the pass's flags come back set, collect re-scores the slot's features synchronously as below, resolves the
// partial-product band on the per-frame values (flush_resolve overwrites them) and sums again.
// sr_stream_set_open (diagonal sessions, before the first submit) adds the open-set decision to every tick: open_set_decision_kernel
// (open_set.hip) behind the tick's finalize -- over the windows' row offsets, or over the VAD session's device-side frame counts --
// and one more small copy (margins, labels) into the slot's pinned block; a captured tick holds both.  Rule and threshold are part
// of the capture and fixed for the session's life.  A tick that collect re-scores is decided again on its final sums.
#include "../../include/pygmm_hip.h"

#include "abi_internal.hpp"
#include "batch.hpp"
#include "gmm_full.hpp"
#include "mfcc.hpp"
#include "score.hpp"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <deque>

struct SRStream {
    SRMfcc *mfcc = nullptr;
    SRModelSet *set = nullptr;           // a diagonal session ...
    SRFullSet *fset = nullptr;           // ... or a full-covariance one: exactly one of the two is set
    sr::LtsdSession *vad = nullptr;      // the voice-activity front end (sr_stream_create_vad), or null
    int n_windows = 0, nd = 0, n_models = 0, flags = 0;
    int64_t window_samples = 0;
    hipStream_t copy_stream = nullptr;
    struct Slot {
        int16_t *h_pcm = nullptr;        // pinned
        double *h_sums = nullptr;        // pinned [n_windows][S]
        int *h_argmax = nullptr;         // pinned [n_windows]
        int *h_oor = nullptr;            // pinned: the fp16 engines' saturation flag of this tick
        SRBatch pcm, feat;
        // a VAD session: the compacted windows, and the tick's results as one block -- sums [n_windows][S], argmax [n_windows],
        // voiced samples [n_windows] (copied back together), then the frame counts [n_windows] the reductions read
        SRBatch vpcm;
        sr::DevBuf<double> d_res;
        int *h_voiced = nullptr;         // pinned, behind h_argmax in the same allocation
        sr::DevBuf<double> d_open;       // sr_stream_set_open: the tick's margins [n_windows], then labels [n_windows] ...
        double *h_open = nullptr;        // ... and where they land (pinned)
        hipEvent_t h2d_done = nullptr, done = nullptr, t_submit = nullptr;
        hipGraphExec_t exec = nullptr;   // SR_STREAM_GRAPH: the captured tick
        long exec_epoch = -1;
        bool busy = false;
    } slot[2];
    std::deque<int> in_flight;           // slot indices, oldest first
    long submitted = 0;
    int device = 0;                      // the GPU the session lives on
    bool open = false;                   // sr_stream_set_open: every tick carries the open-set decision
    sr::OpenSetRule open_rule{0, 0.0};
};

using namespace sr;

// test hook, off unless sr_set_option("debug_capture_delay_ms", n) turns it on (it used to be an environment variable read on
// every capture: a stray variable could stall serving, and getenv races with a concurrent setenv)
std::atomic<int> &stream_debug_capture_delay_ms() {
    static std::atomic<int> v{0};
    return v;
}

namespace {

void stream_destroy(SRStream *s) {
    if (!s) return;
    if (gpu_runtime_lost()) return;      // a forked child: the parent's session is not ours to tear down (common.hpp); leaked
    for (auto &sl : s->slot) {
        if (sl.h_pcm) (void)hipHostFree(sl.h_pcm);
        if (sl.h_sums) (void)hipHostFree(sl.h_sums);        // (h_argmax lives behind the sums in the same allocation)
        if (sl.h_oor) (void)hipHostFree(sl.h_oor);
        if (sl.h_open) (void)hipHostFree(sl.h_open);
        if (sl.h2d_done) (void)hipEventDestroy(sl.h2d_done);
        if (sl.done) (void)hipEventDestroy(sl.done);
        if (sl.t_submit) (void)hipEventDestroy(sl.t_submit);
        if (sl.exec) (void)hipGraphExecDestroy(sl.exec);
    }
    if (s->copy_stream) (void)hipStreamDestroy(s->copy_stream);
    ltsd_session_delete(s->vad);
    delete s;
}

// The device side of one tick on the library's stream: kernels + result copies into the slot's
// pinned buffers.  Launches only (every table is cached after the first pass over this shape).
int *vad_argmax(SRStream *s, SRStream::Slot &sl) { return reinterpret_cast<int *>(sl.d_res.p + (size_t)s->n_windows * s->n_models); }
int *vad_frames(SRStream *s, SRStream::Slot &sl) { return vad_argmax(s, sl) + 2 * (size_t)s->n_windows; }

// a diagonal VAD tick's decision from the per-frame values of a pass over the slot's features: each window's first T rows
void vad_sum_frames(SRStream *s, SRStream::Slot &sl, const ScoreResult &r) {
    if (!r.d_frame_ll) fail("serving stream: the scoring pass left no per-frame values");
    masked_finalize(r.d_frame_ll, (long)sl.feat.n_rows, sl.feat.d_offsets.p, vad_frames(s, sl), s->n_windows, s->n_models, true, sl.d_res.p,
                    vad_argmax(s, sl));
}

// the open-set decision of a tick behind its final sums (`d_counts`: the VAD session's frame counts, else the windows' row offsets)
// and the copy of the block into the slot's pinned memory, left in flight
void enqueue_open(SRStream *s, SRStream::Slot &sl, const double *d_sums, const int *d_counts) {
    const size_t U = (size_t)s->n_windows;
    launch_open_set(d_sums, s->n_models, s->open_rule, sl.feat.d_offsets.p, d_counts, nullptr, s->n_windows, sl.d_open.p,
                    open_set_labels(sl.d_open.p, U));
    SR_HIP(hipMemcpyAsync(sl.h_open, sl.d_open.p, open_set_bytes(U), hipMemcpyDeviceToHost, ctx().stream));
}

// the diagonal pass of a tick, plain or VAD: the scoring launches and the copies of its two flags, left in flight
ScoreResult score_tick(SRStream *s, SRStream::Slot &sl, bool want_frame_ll) {
    const ScoreResult r = score_device(*s->set, sl.feat, want_frame_ll, s->flags & 0xff);
    // (sl.h_oor is cleared by sr_stream_submit BEFORE anything of the tick is enqueued, not here: this function also runs under
    // stream capture right behind a plain pass of the same slot, and a host-side clear at that point races with the plain pass's
    // copies below -- when the device won, the tick's "frames in the partial-product band" flag was lost and the tick came back
    // unresolved: one failure in ~10 runs of the full GPU suite, round 3)
    // [1]: (tile, model) pairs in the band where the reference's partial-product flushes decide (lse.hpp): resolved at collect.
    // (Round 4: the workspace keeps the two counters, and the argmax values behind the sums, side by side -- one copy each; a
    // copy is ~4.5 us on the stream, a tenth of a single window's decision.)
    copy_pass_flags(r, sl.h_oor, ctx().stream);
    return r;
}

void enqueue_vad_tick(SRStream *s, SRStream::Slot &sl) {
    int *const d_voiced = vad_argmax(s, sl) + s->n_windows, *const d_frames = vad_frames(s, sl);
    ltsd_session_enqueue(*s->vad, sl.pcm, s->mfcc->frame_len, s->mfcc->frame_shift, sl.vpcm.pcm16.p, d_voiced, d_frames);
    mfcc_extract_batch(*s->mfcc, sl.vpcm, 0, 1, sl.feat, d_frames);
    if (s->fset) {
        fullset_score_device_masked(*s->fset, sl.feat, d_frames, sl.d_res.p);
    } else {
        vad_sum_frames(s, sl, score_tick(s, sl, true));
        if (s->open) enqueue_open(s, sl, sl.d_res.p, d_frames);
    }
    SR_HIP(hipMemcpyAsync(sl.h_sums, sl.d_res.p, results_bytes(s->n_windows, s->n_models, 2), hipMemcpyDeviceToHost, ctx().stream));
}

void enqueue_tick(SRStream *s, SRStream::Slot &sl) {
    if (s->vad) return enqueue_vad_tick(s, sl);
    mfcc_extract_batch(*s->mfcc, sl.pcm, s->nd, 1, sl.feat);
    if (s->fset) {
        // sums [n_windows][S] and the argmax values right behind them, as the slot's pinned buffer holds them: one copy
        const double *res = fullset_score_device(*s->fset, sl.feat);
        SR_HIP(hipMemcpyAsync(sl.h_sums, res, results_bytes(s->n_windows, s->n_models), hipMemcpyDeviceToHost, ctx().stream));
        return;
    }
    const ScoreResult r = score_tick(s, sl, false);
    if (s->open) enqueue_open(s, sl, r.d_sums, nullptr);
    const size_t n_sums = (size_t)s->n_windows * s->n_models;
    if ((const void *)r.d_argmax == (const void *)(r.d_sums + n_sums)) {
        SR_HIP(hipMemcpyAsync(sl.h_sums, r.d_sums, results_bytes(s->n_windows, s->n_models), hipMemcpyDeviceToHost, ctx().stream));
    } else {
        SR_HIP(hipMemcpyAsync(sl.h_sums, r.d_sums, n_sums * sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
        SR_HIP(hipMemcpyAsync(sl.h_argmax, r.d_argmax, (size_t)s->n_windows * sizeof(int), hipMemcpyDeviceToHost, ctx().stream));
    }
}

void capture_tick(SRStream *s, SRStream::Slot &sl) {
    if (sl.exec) {
        (void)hipGraphExecDestroy(sl.exec);
        sl.exec = nullptr;
    }
    const bool prof = ctx().profiling;
    ctx().profiling = false;             // no event records inside the capture
    hipGraph_t g = nullptr;
    const long epoch = g_devbuf_epoch.load();
    // test hook (tests/test_gpu_pipeline.py): hold the host back until the plain pass in front of the capture has finished on the
    // device -- the ordering in which a host-side write during capture used to clobber that pass's result flags
    if (const int d = stream_debug_capture_delay_ms().load()) std::this_thread::sleep_for(std::chrono::milliseconds(d));
    SR_HIP(hipStreamBeginCapture(ctx().stream, hipStreamCaptureModeThreadLocal));
    try {
        std::lock_guard<std::recursive_mutex> _api_lock(api_mutex());
        enqueue_tick(s, sl);
    } catch (...) {
        (void)hipStreamEndCapture(ctx().stream, &g);
        if (g) (void)hipGraphDestroy(g);
        ctx().profiling = prof;
        throw;
    }
    ctx().profiling = prof;
    SR_HIP(hipStreamEndCapture(ctx().stream, &g));
    if (g_devbuf_epoch.load() != epoch) {     // the pass itself touched a workspace: not steady state yet
        (void)hipGraphDestroy(g);
        fail("serving graph: the captured pass modified a cached workspace");
    }
    const hipError_t e = hipGraphInstantiate(&sl.exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) fail("hipGraphInstantiate failed: %s", hipGetErrorString(e));
    sl.exec_epoch = epoch;
}

}  // namespace

namespace {

struct VadParams {
    int ltsd_window, order;
    const float *noise_amp;
    double lambda0, lambda1;
};

SRStream *stream_create(SRMfcc *m, SRModelSet *set, SRFullSet *fset, int n_windows, int64_t window_samples, int nd, int flags,
                        const VadParams *vp = nullptr) {
    try {
        std::lock_guard<std::recursive_mutex> _api_lock(api_mutex());
        ensure_device();
        if (!m || !(set || fset) || n_windows <= 0 || window_samples <= 0) fail("bad arguments to sr_stream_create");
        if (mfcc_num_frames(*m, window_samples) - nd <= 0) fail("window of %lld samples yields no frames", (long long)window_samples);
        if (fset) {
            if (fset->device != current_device())
                fail("model set lives on device %d, the calling thread is on device %d", fset->device, current_device());
            if (nd < 0 || nd > 2) fail("delta order must be 0, 1 or 2");
            if (m->n_lpc > 0 && nd != 0) fail("LPC columns (mix_feature) come without deltas: use nd = 0");
            const int dim = m->n_ceps * (nd + 1) + m->n_lpc;
            if (dim != fset->D) fail("the extractor yields %d columns, the models have %d dims", dim, fset->D);
        }
        // owned by a guard until every step below has succeeded (pinned buffers, events and the
        // copy stream are released by stream_destroy on any failure)
        std::unique_ptr<SRStream, void (*)(SRStream *)> guard(new SRStream(), stream_destroy);
        SRStream *s = guard.get();
        s->device = current_device();
        s->mfcc = m;
        s->set = set;
        s->fset = fset;
        s->n_windows = n_windows;
        s->window_samples = window_samples;
        s->nd = nd;
        s->flags = flags;
        s->n_models = fset ? fset->S : set->host.n_models;
        SR_HIP(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
        const size_t n_samp = (size_t)n_windows * window_samples;
        if (vp) s->vad = ltsd_session_new(n_windows, window_samples, vp->ltsd_window, vp->order, vp->noise_amp, vp->lambda0, vp->lambda1);
        for (auto &sl : s->slot) {
            SR_HIP(hipHostMalloc(reinterpret_cast<void **>(&sl.h_pcm), n_samp * sizeof(int16_t), hipHostMallocDefault));
            // sums and, right behind them, the argmax values: as the device keeps them (score_device), one copy per tick
            const size_t n_sums = (size_t)n_windows * s->n_models;
            SR_HIP(hipHostMalloc(reinterpret_cast<void **>(&sl.h_sums), results_bytes(n_windows, s->n_models, vp ? 2 : 1), hipHostMallocDefault));
            sl.h_argmax = reinterpret_cast<int *>(sl.h_sums + n_sums);
            if (vp) sl.h_voiced = sl.h_argmax + n_windows;
            SR_HIP(hipHostMalloc(reinterpret_cast<void **>(&sl.h_oor), 2 * sizeof(int), hipHostMallocDefault));
            sl.h_oor[0] = sl.h_oor[1] = 0;
            SR_HIP(hipEventCreate(&sl.h2d_done));
            SR_HIP(hipEventCreate(&sl.done));
            SR_HIP(hipEventCreate(&sl.t_submit));
            sl.pcm.bind_device();
            sl.pcm.kind = SRBatch::PCM16;
            sl.pcm.n_utt = n_windows;
            sl.pcm.n_rows = (int64_t)n_samp;
            sl.pcm.offsets.resize(n_windows + 1);
            for (int u = 0; u <= n_windows; u++) sl.pcm.offsets[u] = (int64_t)u * window_samples;
            sl.pcm.pcm16.alloc(n_samp);
            SR_HIP(hipMemsetAsync(sl.pcm.pcm16.p, 0, n_samp * sizeof(int16_t), ctx().stream));
            sl.pcm.d_offsets.upload(sl.pcm.offsets.data(), sl.pcm.offsets.size());
            sync_stream();
            if (vp) {
                sl.vpcm.bind_device();
                sl.vpcm.kind = SRBatch::PCM16;
                sl.vpcm.n_utt = n_windows;
                sl.vpcm.n_rows = (int64_t)n_samp;
                sl.vpcm.offsets = sl.pcm.offsets;
                sl.vpcm.pcm16.alloc(n_samp);
                sl.vpcm.d_offsets.upload(sl.vpcm.offsets.data(), sl.vpcm.offsets.size());
                sl.d_res.alloc(n_sums + (3 * (size_t)n_windows + 1) / 2);
                SR_HIP(hipMemsetAsync(sl.d_res.p, 0, sl.d_res.n * sizeof(double), ctx().stream));
                sync_stream();
                enqueue_vad_tick(s, sl);      // (the same synchronous pass, through the front end)
                sync_stream();
                sl.h_oor[0] = sl.h_oor[1] = 0;
                continue;
            }
            // one synchronous pass per slot builds every table / workspace for this shape, so the
            // steady state launches kernels only
            mfcc_extract_batch(*m, sl.pcm, nd, 1, sl.feat);
            if (fset) (void)fullset_score_device(*fset, sl.feat);
            else (void)score_device(*set, sl.feat, false, flags & 0xff);
            sync_stream();
        }
        return guard.release();
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return nullptr;
    }
}

}  // namespace

extern "C" {

SRStream *sr_stream_create(SRMfcc *m, SRModelSet *set, int n_windows, int64_t window_samples, int nd,
                           int flags) {
    return stream_create(m, set, nullptr, n_windows, window_samples, nd, flags);
}

SRStream *sr_stream_create_full(SRMfcc *m, SRFullSet *set, int n_windows, int64_t window_samples, int nd, int flags) {
    try {
        if (flags & ~SR_STREAM_GRAPH) fail("sr_stream_create_full accepts SR_STREAM_GRAPH only (flags 0x%x)", flags);
        if (!m || !set) fail("bad arguments to sr_stream_create_full");
        if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_stream_create_full");
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return nullptr;
    }
    return stream_create(m, nullptr, set, n_windows, window_samples, nd, flags);
}

SRStream *sr_stream_create_vad(SRMfcc *m, SRModelSet *set, SRFullSet *fullset, int n_windows, int64_t window_samples, int nd, int flags,
                               int ltsd_window, int order, const float *noise_amp, double lambda0, double lambda1) {
    try {
        if (!m || !noise_amp || (set == nullptr) == (fullset == nullptr))
            fail("bad arguments to sr_stream_create_vad (an extractor, a noise spectrum and exactly one of the two model sets)");
        if (n_windows <= 0 || window_samples <= 0) fail("bad arguments to sr_stream_create_vad (%d windows of %lld samples)", n_windows, (long long)window_samples);
        if (nd != 0) fail("a voice-activity session serves nd = 0 only (deltas over a device-side length are not built): got nd = %d", nd);
        if (fullset && (flags & ~SR_STREAM_GRAPH)) fail("sr_stream_create_vad accepts SR_STREAM_GRAPH only with a full-covariance set (flags 0x%x)", flags);
        if (set && (flags & ~(SR_STREAM_GRAPH | SR_CLAMP_COMPAT))) fail("sr_stream_create_vad accepts SR_CLAMP_COMPAT and SR_STREAM_GRAPH (flags 0x%x)", flags);
        if (!std::isfinite(lambda0) || !std::isfinite(lambda1)) fail("LTSD thresholds must be finite (lambda0 %g, lambda1 %g)", lambda0, lambda1);
        ltsd_session_check(window_samples, ltsd_window, order);
        if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_stream_create_vad");
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return nullptr;
    }
    const VadParams vp{ltsd_window, order, noise_amp, lambda0, lambda1};
    return stream_create(m, set, fullset, n_windows, window_samples, 0, flags, &vp);
}

void sr_stream_free(SRStream *s) {
    if (!s || gpu_runtime_lost()) return;
    const int prev = current_device();
    try {
        set_thread_device(s->device);
        std::lock_guard<std::recursive_mutex> _api_lock(api_mutex());   // no submit / collect of another thread in between
        (void)hipSetDevice(s->device);
        (void)hipDeviceSynchronize();
        stream_destroy(s);
        set_thread_device(prev);
    } catch (...) {
    }
}

int sr_stream_submit(SRStream *s, const int16_t *pcm) {
    try {
        std::lock_guard<std::recursive_mutex> _api_lock(api_mutex());
        if (!s || !pcm) fail("null argument");
        if (s->device != current_device()) fail("stream lives on device %d, the calling thread is on device %d", s->device, current_device());
        ensure_device();
        if (s->in_flight.size() >= 2) fail("two ticks already in flight: collect one first");
        const int k = (int)(s->submitted & 1);
        auto &sl = s->slot[k];
        const size_t bytes = (size_t)s->n_windows * s->window_samples * sizeof(int16_t);
        std::memcpy(sl.h_pcm, pcm, bytes);                      // caller's buffer is free again on return
        sl.h_oor[0] = sl.h_oor[1] = 0;                          // this tick's flags: written by its device-to-host copies only
        SR_HIP(hipEventRecord(sl.t_submit, s->copy_stream));
        SR_HIP(hipMemcpyAsync(sl.pcm.pcm16.p, sl.h_pcm, bytes, hipMemcpyHostToDevice, s->copy_stream));
        SR_HIP(hipEventRecord(sl.h2d_done, s->copy_stream));
        SR_HIP(hipStreamWaitEvent(ctx().stream, sl.h2d_done, 0));
        if (s->flags & SR_STREAM_GRAPH) {
            if (!sl.exec || sl.exec_epoch != g_devbuf_epoch.load()) {
                // (re)build: one plain pass first so that every cache reflects this shape, then capture
                enqueue_tick(s, sl);
                capture_tick(s, sl);
            } else if (s->fset) {
                // (a full-covariance tick writes none of the diagonal pass counters)
                SR_HIP(hipGraphLaunch(sl.exec, ctx().stream));
            } else {
                // the replayed tick writes the pass counters without score_device seeing it: a delivering pass behind it must
                // clear them first (a delivering ModelSet.score between submit and collect read this tick's exception counts)
                counters_written_elsewhere();
                SR_HIP(hipGraphLaunch(sl.exec, ctx().stream));
            }
        } else {
            enqueue_tick(s, sl);
        }
        SR_HIP(hipEventRecord(sl.done, ctx().stream));
        sl.busy = true;
        s->in_flight.push_back(k);
        s->submitted++;
        return 0;
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return -1;
    }
}

static int stream_collect(SRStream *s, double *sums_out, int *argmax_out, int *voiced_out, double *device_ms, int *label_out = nullptr,
                          double *margin_out = nullptr, bool want_open = false) {
    try {
        std::lock_guard<std::recursive_mutex> _api_lock(api_mutex());
        if (!s) fail("null stream");
        if (want_open && !s->open) fail("sr_stream_collect_open: the session carries no open-set decision (sr_stream_set_open before the first submit)");
        if (want_open && (!label_out || !margin_out)) fail("sr_stream_collect_open: null output (labels and margins are both required)");
        if (s->device != current_device()) fail("stream lives on device %d, the calling thread is on device %d", s->device, current_device());
        ensure_device();
        if (voiced_out && !s->vad) fail("not a voice-activity session: no voiced counts (sr_stream_create_vad)");
        if (s->in_flight.empty()) fail("nothing in flight");
        const int k = s->in_flight.front();
        s->in_flight.pop_front();
        auto &sl = s->slot[k];
        SR_HIP(hipEventSynchronize(sl.done));
        if (!s->fset && (sl.h_oor[0] != 0 || sl.h_oor[1] != 0)) {
            // a frame of this tick left the fp16 engine's range (-> the fp32-grade engines), or sits in the band where the
            // reference's partial-product flushes decide (-> resolved by fetch_results): its features are still in the
            // slot -- score them again, synchronously
            const int fl = (s->flags & 0xff) | (sl.h_oor[0] != 0 ? SCORE_PRECISE : 0);
            if (s->vad) {
                // per-frame values again; fetch_results without host destinations resolves the band ON THE DEVICE (flush_resolve
                // overwrites the per-frame values of the noted pairs), then the same sum over each window's first T rows
                vad_sum_frames(s, sl, score_resolved(*s->set, sl.feat, true, fl, 0, nullptr, nullptr, nullptr));
                if (s->open) enqueue_open(s, sl, sl.d_res.p, vad_frames(s, sl));       // the decision again, on the final sums
                SR_HIP(hipMemcpyAsync(sl.h_sums, sl.d_res.p, results_bytes(s->n_windows, s->n_models), hipMemcpyDeviceToHost, ctx().stream));
                sync_stream();
            } else if (s->open) {
                // (the decision with the re-scored sums: taken on the device behind finalize and, for the utterances
                // gmm_flush.hip patches, behind the patch)
                const OpenSetFetch open{s->open_rule, open_set_labels(sl.h_open, (size_t)s->n_windows), sl.h_open};
                score_resolved(*s->set, sl.feat, false, fl, 0, sl.h_sums, sl.h_argmax, nullptr, &open);
            } else {
                score_resolved(*s->set, sl.feat, false, fl, 0, sl.h_sums, sl.h_argmax, nullptr);
            }
            sl.h_oor[0] = sl.h_oor[1] = 0;
        }
        if (sums_out) std::memcpy(sums_out, sl.h_sums, (size_t)s->n_windows * s->n_models * sizeof(double));
        if (argmax_out) std::memcpy(argmax_out, sl.h_argmax, (size_t)s->n_windows * sizeof(int));
        if (voiced_out) std::memcpy(voiced_out, sl.h_voiced, (size_t)s->n_windows * sizeof(int));
        if (want_open) {
            std::memcpy(margin_out, sl.h_open, (size_t)s->n_windows * sizeof(double));
            std::memcpy(label_out, open_set_labels(sl.h_open, (size_t)s->n_windows), (size_t)s->n_windows * sizeof(int));
        }
        if (device_ms) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, sl.t_submit, sl.done);
            *device_ms = ms;
        }
        sl.busy = false;
        return 0;
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return -1;
    }
}

int sr_stream_collect(SRStream *s, double *sums_out, int *argmax_out, double *device_ms) {
    return stream_collect(s, sums_out, argmax_out, nullptr, device_ms);
}

int sr_stream_collect_vad(SRStream *s, double *sums_out, int *argmax_out, int *voiced_out, double *device_ms) {
    return stream_collect(s, sums_out, argmax_out, voiced_out, device_ms);
}

int sr_stream_set_open(SRStream *s, int bg, double threshold) {
    try {
        if (!s) fail("sr_stream_set_open: null stream");
        if (s->fset) fail("sr_stream_set_open: a full-covariance session has no open-set decision (no UBM column: diagonal sets only)");
        const OpenSetRule rule{bg, threshold};
        open_set_check(rule, s->n_models);
        if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_stream_set_open");
        std::lock_guard<std::recursive_mutex> _api_lock(api_mutex());
        if (s->submitted > 0) fail("sr_stream_set_open: ticks were submitted already (rule and threshold belong to the captured tick: set them before the first submit)");
        if (s->device != current_device()) fail("stream lives on device %d, the calling thread is on device %d", s->device, current_device());
        ensure_device();
        const size_t U = (size_t)s->n_windows;
        for (auto &sl : s->slot) {
            if (!sl.d_open.p) sl.d_open.alloc(open_set_doubles(U));
            if (!sl.h_open) SR_HIP(hipHostMalloc(reinterpret_cast<void **>(&sl.h_open), open_set_doubles(U) * sizeof(double), hipHostMallocDefault));
        }
        s->open_rule = rule;
        s->open = true;
        return 0;
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return -1;
    }
}

int sr_stream_collect_open(SRStream *s, double *sums_out, int *label_out, double *margin_out, int *voiced_out, double *device_ms) {
    return stream_collect(s, sums_out, nullptr, voiced_out, device_ms, label_out, margin_out, true);
}

}  // extern "C"
