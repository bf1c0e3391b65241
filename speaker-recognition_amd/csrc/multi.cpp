// multi.cpp -- one host process, every GPU of the node: utterance-sharded prediction without torch,
// MPI or any collective ("one host thread + one hipStream pair per device").
//
// The reference's parallelism on this path is a thread pool inside the scoring call
// (Threadpool pool(concurrency), src/gmm/src/gmm.cc:533-560) and a process pool over utterances
// (multiprocessing.Pool, src/test/test-gmm.py:128-133).  Here the unit of sharding is the
// utterance (CMVN, deltas and the per-utterance sums need whole utterances and nothing else):
// utterances are dealt to the slots greedily by length, every slot owns a replica of the models
// and of the extractor tables on its GPU, a host thread per slot runs PCM upload -> MFCC -> CMVN /
// deltas -> all models -> sums + argmax on that GPU's stream, and the host concatenates the
// per-utterance rows.  Bytes that cross between GPUs: none.
//
// A slot is bound to device `slot % visible devices`, so asking for more slots than GPUs is legal:
// the surplus slots share a GPU (serialised by that device's lock) -- how the threading is tested
// on a single-GPU box.
//
// sr_multi_create_full builds the same predictor over full-covariance models (SRFullGMM): every slot holds an SRFullSet replica,
// and a piece runs features (MFCC + LPC columns or deltas) -> full scoring -> fullcov_finalize_kernel -> one copy of its sums
// with the argmax values behind them.  That log-sum-exp is exact: nothing of a full piece is resolved or scored again afterwards.
#include "../../include/pygmm_hip.h"

#include "abi_internal.hpp"
#include "batch.hpp"
#include "common.hpp"
#include "gmm_full.hpp"
#include "gmm_model.hpp"
#include "mfcc.hpp"
#include "multi_plan.hpp"
#include "score.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <deque>
#include <system_error>
#include <thread>
#include <utility>

using namespace sr;

std::atomic<int> &multi_merge_option() {     // sr_set_option("multi_merge_same_device", 0 | 1)
    static std::atomic<int> v{1};
    return v;
}

struct SRMulti {
    // One piece of a slot's utterances: its PCM on the device, the feature stage's workspace and output, page-locked result
    // buffers.  Everything a piece needs is its own, so that pieces of different shapes -- and of different slots on one device --
    // never re-upload a cached table (that would synchronise the stream in the middle of the pipeline).
    struct Chunk {
        std::unique_ptr<SRBatch> pcm;
        PinnedBuf<int16_t> staging;         // only used when the caller's PCM is not page-locked
        hipEvent_t uploaded = nullptr, done = nullptr;
        int u0 = 0, u1 = 0;                 // range of the slot's utterances
        SRBatch feat;
        MfccScratch *scratch = nullptr;
        PinnedBuf<double> h_sums;           // (+ room for the argmax values right behind the sums: they come in one copy, as they lie in the workspace)
        int *h_arg = nullptr;               // where this pass's argmax values landed (behind the sums, or h_argmax)
        PinnedBuf<int> h_argmax, h_flags;   // h_flags: {a frame saturated the fp16 engine, (tile, model) pairs in the partial-product band}
        // the piece's list of (tile, model) pairs in the band, set aside on the device (the scoring workspace it was produced in
        // belongs to the next piece by then): what gmm_flush.hip re-evaluates when it is not empty
        DevBuf<int2> d_list;
        const TileTable *tiles = nullptr;
        int flush_cap = 0;
        // sr_multi_predict_pcm_open: the piece's open-set decision -- margins, then labels (open_set.hip) -- on the device and where
        // it lands
        DevBuf<double> d_open;
        PinnedBuf<double> h_open;
    };
    struct Slot {
        int device = 0;
        std::unique_ptr<SRModelSet> set;    // diagonal models ...
        std::unique_ptr<SRFullSet> fset;    // ... or full-covariance ones (sr_multi_create_full)
        Chunk chunk[MULTI_CHUNKS];
        std::vector<int64_t> offsets;
        std::vector<int> utts;              // global utterance indices, in slot order
        std::vector<double> sums;
        std::vector<int> argmax;
        std::string error;
        double seconds = 0.0;               // wall time of the slot's last pass
        int numa_node = -1;                 // where the slot's host thread was pinned (-1: nowhere)
        MultiSchedule sched;                // what the last passes told about this slot's work: the shape of the next pass's pieces
        int n_pieces = 0;                   // pieces the slot cut in the last call (0: it took no work)
    };
    std::unique_ptr<SRMfcc> mfcc;           // host tables shared; device tables per GPU inside
    std::deque<Slot> slots;                // (a slot owns page-locked buffers and events: not movable)
    int n_models = 0;
    bool full = false;
};

namespace {

// Pageable caller memory -> the page-locked staging buffer.  One thread's memcpy (~25 GB/s) is slower than the link it feeds
// (55 GB/s): copies of more than a few MB are cut over MULTI_STAGING_THREADS short-lived threads (they inherit the slot
// thread's placement next to its GPU).
constexpr int MULTI_STAGING_THREADS = 4;
void staging_copy(void *dst, const void *src, size_t bytes) {
    constexpr size_t PART_MIN = (size_t)4 << 20;
    const int parts = (int)std::min<size_t>(MULTI_STAGING_THREADS, bytes / PART_MIN);
    if (parts <= 1) {
        std::memcpy(dst, src, bytes);
        return;
    }
    const size_t per = ((bytes / parts) + 4095) & ~(size_t)4095;
    struct Joiner {                          // (a thread that could not be started leaves its part to this one)
        std::vector<std::thread> th;
        ~Joiner() {
            for (auto &t : th) t.join();
        }
    } helpers;
    size_t mine_hi = std::min(bytes, per);   // this thread copies [0, mine_hi) and whatever nobody else took
    std::vector<std::pair<size_t, size_t>> left;
    for (int p = 1; p < parts; p++) {
        const size_t lo = std::min(bytes, per * p), hi = p + 1 == parts ? bytes : std::min(bytes, per * (p + 1));
        try {
            helpers.th.emplace_back([=] { std::memcpy((char *)dst + lo, (const char *)src + lo, hi - lo); });
        } catch (const std::system_error &) {
            left.emplace_back(lo, hi);
        }
    }
    std::memcpy(dst, src, mine_hi);
    for (const auto &r : left) std::memcpy((char *)dst + r.first, (const char *)src + r.first, r.second - r.first);
}

// true when [p, p + bytes) is page-locked host memory the copy engines can read directly (hipHostMalloc / hipHostRegister
// / sr_host_register): then the slots DMA straight out of the caller's buffer
bool host_pinned(const void *p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();           // (an ordinary malloc pointer is "invalid value" to the runtime: not an error here)
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

// What a call hands every slot's thread: the caller's PCM and offsets, where the rows go, and (sr_multi_predict_pcm_open) the rule.
struct Call {
    const int16_t *pcm;
    const int64_t *off;
    int nd, flags;
    bool pinned;                            // the caller's PCM is page-locked: the copy engines read it in place
    double *sums_out;
    int *argmax_out;
    const OpenSetRule *open;
    int *label_out;
    double *margin_out;
};

// {device seconds per frame, link seconds per frame} of a slot, for the first pass's estimate (multi_first_schedule): the set's
// arithmetic at the rate its engine class sustains plus the MFCC's 2.7 ns, against a frame shift of int16 samples at 55 GB/s.
std::pair<double, double> frame_seconds(const SRMulti &m, const SRMulti::Slot &s) {
    double flops = 0.0, rate = 0.0;
    if (m.full) {
        // K (2 D^2 + 3 D + 6) per frame-model, at what gmm_full.hip sustains (profiles/r07_full_cov.json: 99 TFLOP/s with one
        // row block, D <= 32; 42 with two)
        const SRFullSet &fs = *s.fset;
        const double D = fs.D;
        flops = (double)fs.kbeg[fs.S] * (2.0 * D * D + 3.0 * D + 6.0);
        rate = fs.D <= 32 ? 99e12 : 42e12;
    } else {
        const SRModelSet &set = *s.set;
        double mixtures = 0.0;                         // of all models together (padded to whole records of KB)
        for (const ChunkDesc &cd : set.host.chunks) mixtures += (double)cd.n_records * KB;
        flops = mixtures * (4.0 * set.host.dim + 6.0);          // per frame
        rate = !set.h2s.params.empty() ? 700e12 : (!set.h2.params.empty() || !set.bx3.params.empty() || !set.shared.params.empty()) ? 350e12 : 60e12;
    }
    const double dev_s = flops / rate + 2.7e-9;
    const double link_s = (double)m.mfcc->frame_shift * sizeof(int16_t) / 55e9;
    return {dev_s, link_s};
}

// Full-covariance sets: the replica's workspaces sized for the largest piece before anything is queued: no piece reallocates (a
// hipFree, which waits for the device) under the kernels of the one before.
void reserve_full(const SRMulti &m, SRMulti::Slot &s, int n_chunks, int nd) {
    int64_t rows = 0;
    int utts = 0;
    for (int c = 0; c < n_chunks; c++) {
        int64_t r = 0;
        for (int i = s.chunk[c].u0; i < s.chunk[c].u1; i++)
            r += std::max<int64_t>(0, mfcc_num_frames(*m.mfcc, s.offsets[i + 1] - s.offsets[i]) - nd);
        rows = std::max(rows, r);
        utts = std::max(utts, s.chunk[c].u1 - s.chunk[c].u0);
    }
    std::lock_guard<std::recursive_mutex> lock(api_mutex());
    fullset_reserve(*s.fset, rows, utts);
}

// A piece's PCM, host -> device on the device's copy stream (queued in order, an event behind it): from the caller's own memory
// when that is page-locked, else through a page-locked staging buffer this thread fills one piece ahead of the copy engine.
void upload_piece(SRMulti::Slot &s, SRMulti::Chunk &ch, const Call &c, int S) {
    if (!ch.pcm) ch.pcm = std::make_unique<SRBatch>();
    if (!ch.uploaded) SR_HIP(hipEventCreateWithFlags(&ch.uploaded, hipEventDisableTiming));
    if (!ch.done) SR_HIP(hipEventCreateWithFlags(&ch.done, hipEventDisableTiming));
    if (!ch.scratch) ch.scratch = mfcc_scratch_new();
    SRBatch &b = *ch.pcm;
    const int nu = ch.u1 - ch.u0;
    const int64_t base = s.offsets[ch.u0], n_samp = s.offsets[ch.u1] - base;
    {
        std::lock_guard<std::recursive_mutex> lock(api_mutex());   // (the batch's buffers may be reallocated: not under a kernel)
        b.bind_device();
        std::vector<int64_t> po((size_t)nu + 1, 0);
        for (int i = 0; i <= nu; i++) po[i] = s.offsets[ch.u0 + i] - base;
        if (b.kind != SRBatch::PCM16 || b.offsets != po || !b.d_offsets.p) {   // a serving loop repeats its shape: nothing to redo
            b.kind = SRBatch::PCM16;
            b.n_utt = nu;
            b.offsets = po;
            b.n_rows = n_samp;
            b.invalidate_tiles();
            b.pcm16.ensure((size_t)std::max<int64_t>(1, n_samp));
            b.d_offsets.upload(b.offsets.data(), b.offsets.size());
            sync_stream();
        }
        ch.h_sums.ensure((size_t)std::max(1, nu) * S + ((size_t)std::max(1, nu) + 1) / 2);
        ch.h_argmax.ensure((size_t)std::max(1, nu));
        ch.h_flags.ensure(2);
        if (c.open) {
            ch.d_open.ensure(open_set_doubles((size_t)std::max(1, nu)));
            ch.h_open.ensure(open_set_doubles((size_t)std::max(1, nu)));
        }
        ch.h_flags.p[0] = ch.h_flags.p[1] = 0;         // (nothing of this piece is in flight: the previous call waited for it)
    }
    if (!c.pinned) ch.staging.ensure((size_t)std::max<int64_t>(1, n_samp));
    for_each_run(s.utts.data(), ch.u0, ch.u1, [&](int i, int j) {
        const int64_t src0 = c.off[s.utts[i]], n = c.off[s.utts[j] + 1] - src0, dst0 = s.offsets[i] - base;
        if (n <= 0) return;
        const int16_t *src = c.pcm + src0;
        if (!c.pinned) {
            staging_copy(ch.staging.p + dst0, src, sizeof(int16_t) * (size_t)n);
            src = ch.staging.p + dst0;
        }
        SR_HIP(hipMemcpyAsync(b.pcm16.p + dst0, src, sizeof(int16_t) * (size_t)n, hipMemcpyHostToDevice, ctx().copy));
    });
    SR_HIP(hipEventRecord(ch.uploaded, ctx().copy));
}

// A piece's kernels (MFCC, CMVN / deltas, all models, finalize; with `open` the decision against the background column behind
// them) and the copies of its results into page-locked buffers, behind its upload's event on the main stream: launches only.
void enqueue_piece(SRMulti &m, SRMulti::Slot &s, SRMulti::Chunk &ch, const Call &c) {
    const int nu = ch.u1 - ch.u0, S = m.n_models;
    if (nu == 0) return;
    std::lock_guard<std::recursive_mutex> lock(api_mutex());
    SR_HIP(hipStreamWaitEvent(ctx().stream, ch.uploaded, 0));
    mfcc_extract_with(*m.mfcc, *ch.pcm, c.nd, 1, ch.feat, ch.scratch);
    if (m.full) {
        // sums and the argmax values right behind them, in one copy; no flags, no list (the log-sum-exp is exact)
        const double *res = fullset_score_device(*s.fset, ch.feat);
        SR_HIP(hipMemcpyAsync(ch.h_sums.p, res, results_bytes(nu, S), hipMemcpyDeviceToHost, ctx().stream));
        ch.h_arg = reinterpret_cast<int *>(ch.h_sums.p + (size_t)nu * S);
        ch.tiles = nullptr;
        ch.flush_cap = 0;
        SR_HIP(hipEventRecord(ch.done, ctx().stream));
        return;
    }
    const ScoreResult r = score_device(*s.set, ch.feat, false, c.flags);
    // (the pass's two counters and its sums + argmax lie side by side in the workspace: one copy each instead of two -- a copy
    // is ~8 us on the stream, and eight pieces' small operations are what keeps the call above max(copy, kernels))
    copy_pass_flags(r, ch.h_flags.p, ctx().stream);
    if (c.open) {
        launch_open_set(r.d_sums, S, *c.open, ch.feat.d_offsets.p, nullptr, nullptr, nu, ch.d_open.p, open_set_labels(ch.d_open.p, (size_t)nu));
        SR_HIP(hipMemcpyAsync(ch.h_open.p, ch.d_open.p, open_set_bytes((size_t)nu), hipMemcpyDeviceToHost, ctx().stream));
    }
    ch.tiles = r.tiles;
    ch.flush_cap = 0;
    if (r.d_flush_count) {
        // frames in the band of the reference's partial-product flushes are the NORMAL case on some workloads (synthetic
        // speech against random models: ~2 k pairs per 10 M frames): keep what resolving them needs, a few MB device to device
        ch.d_list.ensure((size_t)std::max(1, r.flush_cap));
        ch.flush_cap = r.flush_cap;
        SR_HIP(hipMemcpyAsync(ch.d_list.p, r.d_flush_list, (size_t)r.flush_cap * sizeof(int2), hipMemcpyDeviceToDevice, ctx().stream));
    }
    if ((const void *)r.d_argmax == (const void *)(r.d_sums + (size_t)nu * S)) {
        SR_HIP(hipMemcpyAsync(ch.h_sums.p, r.d_sums, results_bytes(nu, S), hipMemcpyDeviceToHost, ctx().stream));
        ch.h_arg = reinterpret_cast<int *>(ch.h_sums.p + (size_t)nu * S);
    } else {
        SR_HIP(hipMemcpyAsync(ch.h_sums.p, r.d_sums, (size_t)nu * S * sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
        SR_HIP(hipMemcpyAsync(ch.h_argmax.p, r.d_argmax, (size_t)nu * sizeof(int), hipMemcpyDeviceToHost, ctx().stream));
        ch.h_arg = ch.h_argmax.p;
    }
    SR_HIP(hipEventRecord(ch.done, ctx().stream));
}

// The one wait of a piece, and what needs the host afterwards -- noticed in the piece's flags {a frame saturated the fp16 engine,
// (tile, model) pairs in the band of the reference's partial-product flushes (lse.hpp)} -- from its features, which are still on
// the device (as csrc/stream.cpp does for a serving tick); then its rows go straight to the caller's arrays.
void collect_piece(SRMulti::Slot &s, SRMulti::Chunk &ch, const Call &c, int S) {
    const int nu = ch.u1 - ch.u0;
    if (nu == 0) return;
    SR_HIP(hipEventSynchronize(ch.done));
    const int saturated = ch.h_flags.p[0], band = ch.h_flags.p[1];
    if (saturated != 0 || band != 0) {
        std::lock_guard<std::recursive_mutex> lock(api_mutex());
        if (!c.open && saturated == 0 && band > 0 && band <= ch.flush_cap) {
            // pairs in the band, nothing else: re-evaluate exactly those with the reference's arithmetic and complete the
            // piece's results where they are, in host memory -- on the device's SECOND stream (what it reads -- the piece's
            // features, the models, the list -- is nobody else's), so that its one host wait does not wait for the later
            // pieces' kernels
            StreamScope side(ctx().aux);
            flush_resolve_host(*s.set, ch.feat, *ch.tiles, ch.d_list.p, band, ch.h_sums.p, ch.h_arg);
        } else {
            // a frame saturated the fp16 engine, or the list overflowed: this piece again, synchronously, from its features.  With
            // `open` also for pairs in the band, which the closed-set call completes in host memory: scored again, the piece is
            // decided on the device behind gmm_flush.hip's patch.
            const int fl = c.flags | (saturated != 0 ? SCORE_PRECISE : 0);
            ch.h_arg = ch.h_argmax.p;
            OpenSetFetch of{};
            if (c.open) of = OpenSetFetch{*c.open, open_set_labels(ch.h_open.p, (size_t)nu), ch.h_open.p};
            score_resolved(*s.set, ch.feat, false, fl, 0, ch.h_sums.p, ch.h_argmax.p, nullptr, c.open ? &of : nullptr);
        }
    }
    for_each_run(s.utts.data(), ch.u0, ch.u1, [&](int i, int j) {
        const size_t n = (size_t)(j + 1 - i), at = (size_t)(i - ch.u0);
        if (c.sums_out) std::memcpy(c.sums_out + (size_t)s.utts[i] * S, ch.h_sums.p + at * S, n * S * sizeof(double));
        else std::memcpy(s.sums.data() + (size_t)i * S, ch.h_sums.p + at * S, n * S * sizeof(double));
        if (c.argmax_out) std::memcpy(c.argmax_out + s.utts[i], ch.h_arg + at, n * sizeof(int));
        else std::memcpy(s.argmax.data() + i, ch.h_arg + at, n * sizeof(int));
        if (c.open) {
            std::memcpy(c.margin_out + s.utts[i], ch.h_open.p + at, n * sizeof(double));
            std::memcpy(c.label_out + s.utts[i], open_set_labels(ch.h_open.p, (size_t)nu) + at, n * sizeof(int));
        }
    });
}

// One slot: its utterances cut into up to MULTI_CHUNKS pieces of whole utterances (multi_plan.cpp).  Every piece is uploaded on
// the copy stream and its kernels and result copies are ENQUEUED on the main stream behind the upload's event, piece after piece,
// without a host synchronisation in between: the copy of piece i + 1 runs under the kernels of piece i, and the host waits once,
// at the end.  (Round 3 scored the pieces one synchronous call each: four waits per slot and a quarter of the PCM uploaded before
// the first kernel -- 8.8 ms on configs[1] where copy and kernels are 5.8 and 5.7 ms.)
// The device's lock is taken piece by piece, so slots that share a GPU interleave on its stream.
void run_slot(SRMulti *m, SRMulti::Slot &s, const Call &c) {
    auto drain = [&]() {                   // nothing of this call may still be reading the caller's buffer when it returns
        try {
            (void)hipStreamSynchronize(ctx().copy);
            (void)hipStreamSynchronize(ctx().main);
        } catch (...) {
        }
    };
    try {
        set_thread_device(s.device);
        ensure_device();
        // this thread fills staging buffers and waits on this GPU's events: next to its PCIe root unless told not to
        s.numa_node = numa_bind_option().load() ? bind_thread_near_device(s.device) : device_numa_node(s.device);
        const auto t0 = std::chrono::steady_clock::now();
        const int U = (int)s.utts.size();
        const int S = m->n_models;
        s.offsets = multi_slot_offsets(c.off, s.utts);
        if (!c.sums_out) s.sums.assign((size_t)U * S, 0.0);
        if (!c.argmax_out) s.argmax.assign((size_t)U, -1);
        const int64_t total = s.offsets[U];
        const std::pair<double, double> per_frame = frame_seconds(*m, s);
        multi_first_schedule(s.sched, total, per_frame.first, per_frame.second);
        const MultiPieces p = plan_slot_pieces(s.offsets.data(), U, s.sched.schedule);
        for (int k = 0; k < MULTI_CHUNKS; k++) {
            s.chunk[k].u0 = k < p.n ? p.u0[k] : 0;
            s.chunk[k].u1 = k < p.n ? p.u1[k] : 0;
        }
        s.n_pieces = p.n;
        if (m->full) reserve_full(*m, s, p.n, c.nd);
        for (int k = 0; k < p.n; k++) {
            upload_piece(s, s.chunk[k], c, S);
            enqueue_piece(*m, s, s.chunk[k], c);
        }
        // one wait per piece, in order; the rare piece that needs the host is redone from its features
        for (int k = 0; k < p.n; k++) collect_piece(s, s.chunk[k], c, S);
        SR_HIP(hipStreamSynchronize(ctx().copy));              // (pieces without utterances still queued their empty copies)
        s.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        multi_vote(s.sched, total, p.n, s.seconds, s.offsets[s.chunk[0].u1]);
    } catch (const std::exception &e) {
        s.error = e.what();
        drain();
    } catch (...) {
        s.error = "unknown C++ exception";
        drain();
    }
}

// The slot count of a new predictor: `n_slots` as asked for, or one per visible device when it is <= 0.
int checked_slots(int n_slots, int &visible) {
    visible = visible_devices();
    if (visible <= 0) fail("no HIP device available; lib/pygmm.so has no CPU path");
    if (n_slots <= 0) n_slots = visible;
    if (n_slots > 64) fail("at most 64 slots");
    return n_slots;
}

// Replicates the models: pack(slot) once per slot on that slot's GPU, under the lock (threads: packing a 1000-speaker set takes
// seconds).  The caller's device is restored; the first slot that failed is reported.
template <class Pack>
void replicate_slots(SRMulti &m, int n_slots, int visible, Pack pack) {
    m.slots.resize((size_t)n_slots);
    const int prev = current_device();
    std::vector<std::thread> th;
    for (int i = 0; i < n_slots; i++) {
        m.slots[i].device = i % visible;
        th.emplace_back([&, i]() {
            auto &s = m.slots[i];
            try {
                set_thread_device(s.device);
                std::lock_guard<std::recursive_mutex> lock(api_mutex());
                pack(s);
            } catch (const std::exception &e) {
                s.error = e.what();
            }
        });
    }
    for (auto &t : th) t.join();
    set_thread_device(prev);
    for (auto &s : m.slots)
        if (!s.error.empty()) fail("device %d: %s", s.device, s.error.c_str());
}

}  // namespace

extern "C" {

SRMulti *sr_multi_create(GMM *const *models, int n_models, double fs, double win_length_ms,
                         double win_shift_ms, int fft_size, int n_filters, int n_ceps,
                         double pre_emphasis, int n_slots) {
    try {
        if (!models || n_models <= 0) fail("empty model list");
        int visible = 0;
        n_slots = checked_slots(n_slots, visible);
        std::vector<const GMM *> v(models, models + n_models);
        for (auto *g : v)
            if (!g) fail("null GMM handle in model list");
        auto m = std::make_unique<SRMulti>();
        m->mfcc = std::make_unique<SRMfcc>(fs, win_length_ms, win_shift_ms, fft_size, n_filters, n_ceps, pre_emphasis);
        m->n_models = n_models;
        replicate_slots(*m, n_slots, visible, [&](SRMulti::Slot &s) {
            s.set = std::make_unique<SRModelSet>();
            pack_model_set(*s.set, v);
            upload_model_set(*s.set);
        });
        return m.release();
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return nullptr;
    }
}

SRMulti *sr_multi_create_full(SRFullGMM *const *models, int n_models, double fs, double win_length_ms, double win_shift_ms, int fft_size,
                              int n_filters, int n_ceps, double pre_emphasis, int n_lpc, int n_slots) {
    try {
        if (!models || n_models <= 0) fail("empty model list");
        if (n_lpc != 0 && n_lpc != 10 && n_lpc != 12 && n_lpc != 15 && n_lpc != 16 && n_lpc != 20)
            fail("LPC order %d is not instantiated (10, 12, 15, 16, 20; 0 = off)", n_lpc);
        for (int i = 0; i < n_models; i++)
            if (!models[i]) fail("null model handle in model list");
        if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_multi_create_full");
        int visible = 0;
        n_slots = checked_slots(n_slots, visible);
        auto m = std::make_unique<SRMulti>();
        m->mfcc = std::make_unique<SRMfcc>(fs, win_length_ms, win_shift_ms, fft_size, n_filters, n_ceps, pre_emphasis);
        m->mfcc->n_lpc = n_lpc;
        m->n_models = n_models;
        m->full = true;
        replicate_slots(*m, n_slots, visible, [&](SRMulti::Slot &s) {
            s.fset = std::make_unique<SRFullSet>();
            fullset_pack(*s.fset, models, n_models);
        });
        return m.release();
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return nullptr;
    }
}

void sr_multi_free(SRMulti *m) {
    if (!m || gpu_runtime_lost()) return;     // (a forked child leaves its parent's device state alone: common.hpp)
    const int prev = current_device();
    for (auto &s : m->slots) {
        try {
            set_thread_device(s.device);
            std::lock_guard<std::recursive_mutex> lock(api_mutex());
            (void)hipSetDevice(s.device);
            s.set.reset();
            s.fset.reset();
            for (auto &ch : s.chunk) {
                ch.pcm.reset();
                if (ch.uploaded) (void)hipEventDestroy(ch.uploaded);
                if (ch.done) (void)hipEventDestroy(ch.done);
                ch.uploaded = ch.done = nullptr;
                if (ch.scratch) mfcc_scratch_delete(ch.scratch);
                ch.scratch = nullptr;
                ch.feat = SRBatch();
                ch.d_list.release();
                ch.d_open.release();
            }
        } catch (...) {
        }
    }
    try { set_thread_device(prev); } catch (...) {}
    delete m;
}

// Page-locks caller memory (a serving loop's PCM ring, say) so that sr_multi_predict_pcm's copy engines read it in place.
int sr_host_register(void *p, size_t bytes) {
    try {
        ensure_device();
        if (!p || bytes == 0) fail("bad arguments to sr_host_register");
        SR_HIP(hipHostRegister(p, bytes, hipHostRegisterDefault));
        return 0;
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return -1;
    }
}
int sr_host_unregister(void *p) {
    try {
        ensure_device();
        SR_HIP(hipHostUnregister(p));
        return 0;
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return -1;
    }
}

int sr_multi_slots(SRMulti *m) { return m ? (int)m->slots.size() : 0; }
int sr_multi_slot_numa_node(SRMulti *m, int slot) {
    return (m && slot >= 0 && slot < (int)m->slots.size()) ? m->slots[slot].numa_node : -1;
}
int sr_multi_slot_device(SRMulti *m, int slot) {
    return (m && slot >= 0 && slot < (int)m->slots.size()) ? m->slots[slot].device : -1;
}
int sr_multi_slot_pieces(SRMulti *m, int slot) {
    return (m && slot >= 0 && slot < (int)m->slots.size()) ? m->slots[slot].n_pieces : -1;
}

// What a call with these offsets, over slots on these devices, decides (multi_plan.cpp): host only, for tests.
int sr_multi_plan(const int64_t *sample_offsets, int n_utt, const int *devices, int n_slots, int merge, const int *schedules,
                  int *active_out, int *counts_out, int *utts_out, int *pieces_out) {
    try {
        if (!sample_offsets || n_utt < 0 || !devices || !active_out || !counts_out || !utts_out || !pieces_out)
            fail("bad arguments to sr_multi_plan");
        if (n_slots < 1 || n_slots > 64) fail("sr_multi_plan: 1 .. 64 slots");
        if (sample_offsets[0] != 0) fail("sample_offsets[0] must be 0");
        for (int u = 0; u < n_utt; u++)
            if (sample_offsets[u + 1] < sample_offsets[u]) fail("sample_offsets must be non-decreasing");
        const std::vector<int> active = multi_active_slots(devices, n_slots, merge != 0);
        const std::vector<std::vector<int>> utts = multi_partition(sample_offsets, n_utt, (int)active.size());
        for (size_t a = 0; a < active.size(); a++) {
            const std::vector<int64_t> so = multi_slot_offsets(sample_offsets, utts[a]);
            const MultiPieces p = plan_slot_pieces(so.data(), (int)utts[a].size(), schedules ? schedules[active[a]] : 0);
            active_out[a] = active[a];
            counts_out[a] = (int)utts[a].size();
            utts_out = std::copy(utts[a].begin(), utts[a].end(), utts_out);
            int *row = pieces_out + a * (1 + 2 * MULTI_CHUNKS);
            row[0] = p.n;
            for (int c = 0; c < MULTI_CHUNKS; c++) row[1 + 2 * c] = p.u0[c], row[2 + 2 * c] = p.u1[c];
        }
        return (int)active.size();
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return -1;
    }
}

static int multi_predict(SRMulti *m, const int16_t *pcm, const int64_t *sample_offsets, int n_utt, int nd, double *sums_out,
                         int *argmax_out, double *slot_seconds_out, int flags, const OpenSetRule *open, int *label_out,
                         double *margin_out) {
    try {
        if (!m || !sample_offsets || n_utt < 0) fail("bad arguments to sr_multi_predict_pcm");
        if (open) {
            if (!label_out || !margin_out) fail("sr_multi_predict_pcm_open: null output (labels and margins are both required)");
            if (m->full) fail("sr_multi_predict_pcm_open: a full-covariance predictor has no open-set decision (no UBM column: diagonal sets only)");
            open_set_check(*open, m->n_models);
        }
        if (sample_offsets[0] != 0) fail("sample_offsets[0] must be 0");
        for (int u = 0; u < n_utt; u++)
            if (sample_offsets[u + 1] < sample_offsets[u]) fail("sample_offsets must be non-decreasing");
        if (sample_offsets[n_utt] > 0 && !pcm) fail("null PCM pointer");
        if (gpu_runtime_lost()) fail_gpu_runtime_lost(open ? "sr_multi_predict_pcm_open" : "sr_multi_predict_pcm");
        if (m->full) {
            if (nd < 0 || nd > 2) fail("delta order must be 0, 1 or 2");
            if (m->mfcc->n_lpc > 0 && nd != 0) fail("LPC columns (mix_feature) come without deltas: use nd = 0");
            const int dim = m->mfcc->n_ceps * (nd + 1) + m->mfcc->n_lpc, D = m->slots.front().fset->D;
            if (dim != D) fail("the extractor yields %d columns, the models have %d dims", dim, D);
        }
        // the slots that take work and their utterances (multi_plan.cpp)
        std::vector<int> devices;
        for (auto &s : m->slots) {
            s.utts.clear();
            s.seconds = 0.0;
            s.n_pieces = 0;
            devices.push_back(s.device);
        }
        const std::vector<int> active = multi_active_slots(devices.data(), (int)devices.size(), multi_merge_option().load() != 0);
        std::vector<std::vector<int>> utts = multi_partition(sample_offsets, n_utt, (int)active.size());
        for (size_t a = 0; a < active.size(); a++) m->slots[active[a]].utts = std::move(utts[a]);
        const bool pinned = sample_offsets[n_utt] > 0 && host_pinned(pcm) &&
                            host_pinned(pcm + sample_offsets[n_utt] - 1);
        std::vector<std::thread> th;
        for (auto &s : m->slots) s.error.clear();
        // (every slot writes its utterances' rows into the caller's arrays itself: disjoint rows)
        const Call call{pcm, sample_offsets, nd, flags, pinned, sums_out, argmax_out, open, label_out, margin_out};
        for (int a : active) th.emplace_back(run_slot, m, std::ref(m->slots[a]), std::cref(call));
        for (auto &t : th) t.join();
        for (auto &s : m->slots)
            if (!s.error.empty()) fail("device %d: %s", s.device, s.error.c_str());
        for (size_t k = 0; k < m->slots.size(); k++)
            if (slot_seconds_out) slot_seconds_out[k] = m->slots[k].seconds;
        return 0;
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return -1;
    }
}

int sr_multi_predict_pcm(SRMulti *m, const int16_t *pcm, const int64_t *sample_offsets, int n_utt,
                         int nd, double *sums_out, int *argmax_out, double *slot_seconds_out, int flags) {
    return multi_predict(m, pcm, sample_offsets, n_utt, nd, sums_out, argmax_out, slot_seconds_out, flags, nullptr, nullptr, nullptr);
}

int sr_multi_predict_pcm_open(SRMulti *m, const int16_t *pcm, const int64_t *sample_offsets, int n_utt, int nd, int bg, double threshold,
                              double *sums_out, int *label_out, double *margin_out, double *slot_seconds_out, int flags) {
    const OpenSetRule rule{bg, threshold};
    return multi_predict(m, pcm, sample_offsets, n_utt, nd, sums_out, nullptr, slot_seconds_out, flags, &rule, label_out, margin_out);
}

}  // extern "C"
