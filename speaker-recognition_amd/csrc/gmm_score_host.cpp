// gmm_score_host.cpp -- a diagonal-GMM scoring pass from the host's side: the per-device workspace and its pass counters, the lazy
// uploads of a set's layouts, score_device (plan -> counters -> delivery -> group table -> one launcher per engine -> finalize),
// the hybrid sets' two passes and merge, and the way results reach host memory.  The decisions are score_plan.cpp's, the
// kernels gmm_score*.hip's.
#include "score.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace sr {

struct LastKernel {
    char name[256] = "";
};
#define g_last_kernel (per_device<LastKernel>().name)      // threads on different devices launch concurrently
const char *last_score_kernel() { return g_last_kernel; }

// The counters of a pass: [0] saturation flag of the fp16 engines, [1] pairs in the partial-product band, [2] the delivering
// finalize's ticket, [4 ...] the shared-sigma engine's exception tiles per model block -- side by side: one clear, one copy.
// Invariant: `clean_p` is set only by a delivering pass (SCORE_HOST_DELIVER: its finalize left `clean_n` counters at `clean_p`
// cleared behind itself), and reset by every pass and by whatever else writes the counters -- a replayed serving graph
// (counters_written_elsewhere, stream.cpp), whose tick does not go through score_device.  A stale `clean_p` left a tick's
// exception counts in place for the next delivering pass: the shared-sigma engine indexed its exception lists with them, past
// their end.  (Every other writer goes through score_device: multi.cpp's pieces, the hybrid halves, the re-runs of
// fetch_results, EM.)
struct PassCounters {
    int *oor_p() { return buf.p; }
    int *flush_count_p() { return buf.p + 1; }
    int *exc_count_p() { return buf.p + 4; }
    int *base() { return buf.p; }
    // before a pass that uses `n` counters: clears them, unless the pass delivers and the last one delivered (only a delivering
    // pass -- never one being captured into a graph -- relies on that)
    void begin(size_t n, bool delivering) {
        buf.ensure(n);
        if (!(delivering && clean_p == buf.p && clean_n >= n)) {
            SR_HIP(hipMemsetAsync(buf.p, 0, n * sizeof(int), ctx().stream));     // the pass's counters, all at once
        } else if (score_options().verify_clean_counters) {
            // test hook: what the skip assumes, read back before anything of this pass is launched (a delivering pass is never
            // captured, so it may wait here); a stale exception count would index the shared-sigma engine's lists out of bounds
            std::vector<int> h(n);
            SR_HIP(hipMemcpyAsync(h.data(), buf.p, n * sizeof(int), hipMemcpyDeviceToHost, ctx().stream));
            sync_stream();
            for (size_t i = 0; i < n; i++)
                if (h[i] != 0) fail("pass counters not clear before a delivering pass: counter %zu of %zu is %d", i, n, h[i]);
        }
        clean_p = nullptr;
    }
    void delivered(size_t n) { clean_p = buf.p; clean_n = n; }
    void invalidate() { clean_p = nullptr; }

private:
    DevBuf<int> buf;
    const int *clean_p = nullptr;
    size_t clean_n = 0;
};

struct ScoreWorkspace {
    DevBuf<double> partial;
    // Results of a pass: [U x S] sums with the U argmax values right behind them, and the pass's counters side by side --
    // one host-bound copy and one clear each instead of two and three (a copy or a fill is ~4.5 us on the stream: 18 us of a
    // 240 us single-utterance decision, round 4).
    DevBuf<double> results;
    PassCounters counters;
    double *sums_p() { return results.p; }
    int *argmax_p(size_t n_sums) { return reinterpret_cast<int *>(results.p + n_sums); }
    void ensure_results(size_t n_utt, size_t n_models) { results.ensure(n_utt * n_models + (n_utt + 1) / 2 + 1); }
    DevBuf<float> frame_ll;
    DevBuf<float> ref_ll;                // split-fp16 shared-sigma engine: the reference model's per-frame LL
    DevBuf<double> ref_partial;
    DevBuf<int> exc_list;                // ... and its exception lists ({tile, listed frames} per block) + the exception pass's plan
    DevBuf<float> hy_a, hy_b;            // hybrid sets: per-frame LL of the two sub-sets
    DevBuf<double> open;                 // the open-set decision of a fetch that asks for it: margin [U], then label [U] (open_set.hip)
    DevBuf<int2> flush_list;             // (tile, model) pairs in the partial-product band (lse.hpp, gmm_flush.hip)
    size_t flush_min_cap = 0;            // set after an overflow: the next pass gets a list of that length
    // SCORE_HOST_DELIVER: the page-locked landing area and the last sequence number handed out
    PinnedBuf<char> deliver;
    void *deliver_dev = nullptr;         // the device's view of it
    unsigned deliver_seq = 0;
};
static ScoreWorkspace &ws() { return per_device<ScoreWorkspace>(); }   // one per device, leaked on purpose

void counters_written_elsewhere() { ws().counters.invalidate(); }

// What a scoring pass needs for the partial-product band (lse.hpp): the threshold its engine compares per-frame values
// with, and the list gmm_finalize_kernel notes poisoned (tile, model) pairs in.  Nothing when the reference's clamp is off.
struct FlushPass {
    float band_hi = -INFINITY;
    int2 *list = nullptr;
    int *count = nullptr;
    int cap = 0;
};
static FlushPass prepare_flush(const SRModelSet &set, int n_tiles, int flags) {
    FlushPass fp;
    if (!(flags & 1) || (flags & SCORE_NO_FLUSH)) return fp;
    auto &w = ws();
    const size_t pairs = (size_t)std::max(1, n_tiles) * (size_t)set.host.n_models;
    size_t cap = std::min<size_t>(pairs, (size_t)1 << 20);
    if (score_options().flush_list_cap > 0) cap = (size_t)score_options().flush_list_cap;     // (testing the overflow path)
    cap = std::min<size_t>(std::max(cap, w.flush_min_cap), 0x7fffffff);
    w.flush_list.ensure(cap);
    fp.list = w.flush_list.p;
    fp.count = w.counters.flush_count_p();          // (cleared with the pass's other counters by score_device)
    // (the capacity the pass is told is a function of ITS size, not of what the workspace happens to hold: a caller that sets a
    // piece's list aside -- multi.cpp -- then sizes its copy once; told the workspace's size, the small pieces of sr_multi's SECOND
    // call found a list grown by the first call's large piece, reallocated theirs under the pipeline and cost configs[2]'s second
    // from-host call 60 ms, round 6)
    fp.cap = (int)std::min<size_t>(cap, 0x7fffffff);
    fp.band_hi = (float)(-708.396418532264 + set.host.flush_band);
    return fp;
}

void upload_model_set(SRModelSet &s) {
    ensure_device();
    s.d_params.upload(s.host.params.data(), s.host.params.size());
    s.d_center0.upload(s.host.center.data(), s.host.center.size());
    s.d_chunks.upload(s.host.chunks.data(), s.host.chunks.size());
    sync_stream();
    s.device = ctx().device;
    if (s.hy_good) upload_model_set(*s.hy_good);
    if (s.hy_bad) upload_model_set(*s.hy_bad);
}

static void ensure_shared_layout(SRModelSet &s) {
    if (s.d_shared_params.p) return;
    s.d_shared_params.upload(s.shared.params.data(), s.shared.params.size());
    s.d_shared_blocks.upload(s.shared.blocks.data(), s.shared.blocks.size());
    s.d_shared_center.upload(s.shared.center.data(), s.shared.center.size());
    sync_stream();
}

static void ensure_h2s_layout(SRModelSet &s) {
    if (s.d_h2s_params.p) return;
    const PackedH2Shared &h = s.h2s;
    s.d_h2s_params.upload(h.params.data(), h.params.size());
    s.d_h2s_blocks.upload(h.blocks.data(), h.blocks.size());
    s.d_h2s_center.upload(h.center.data(), h.center.size());
    s.d_h2s_scale.upload(h.scale.data(), h.scale.size());
    s.d_h2s_qdesc.upload(h.q_desc.data(), h.q_desc.size());
    s.d_h2s_ldesc.upload(h.l_desc.data(), h.l_desc.size());
    s.d_h2s_ref_params.upload(h.ref.params.data(), h.ref.params.size());
    s.d_h2s_ref_chunks.upload(h.ref.chunks.data(), h.ref.chunks.size());
    // the reference pre-pass: one model, one group; its center and scale follow the set's (appended)
    const int gcb[2] = {0, (int)h.ref.chunks.size()};
    s.d_h2s_ref_gcb.upload(gcb, 2);
    s.d_h2s_ref_center.upload(h.ref.center.data(), h.ref.center.size());
    s.d_h2s_ref_scale.upload(h.ref.scale.data(), h.ref.scale.size());
    sync_stream();
}

// The compact order of the same set (PackedH2Compact), for the pipelined kernel: a rearrangement of the flat image, made and
// uploaded by the first pass that takes that kernel -- a set that only ever serves small batches never pays for it.
static bool ensure_h2c_layout(SRModelSet &s) {
    if (s.h2c_state != 0) return s.h2c_state > 0;
    const PackedH2Shared &h = s.h2s;
    if (!h2c_built(s.host.dim, h.klf)) {
        s.h2c_state = -1;
        return false;
    }
    const PackedH2Compact c = pack_h2_compact(h, s.host.dim);
    // (one image of padding on the DEVICE only: the paired form's last stage of a block loads -- never executes -- the image behind
    // the block's last one, score_shapes.hpp: h2q_stage_image)
    const size_t pad_u16 = (size_t)c.nf * 64 * 8;
    s.d_h2c_params.ensure(c.params.size() + pad_u16);
    s.d_h2c_params.upload(c.params.data(), c.params.size());
    SR_HIP(hipMemsetAsync(s.d_h2c_params.p + c.params.size(), 0, pad_u16 * sizeof(uint16_t), ctx().stream));
    s.d_h2c_blocks.upload(c.blocks.data(), c.blocks.size());
    s.d_h2c_qdesc.upload(c.q_desc.data(), c.q_desc.size());
    s.d_h2c_ldesc.upload(c.l_desc.data(), c.l_desc.size());
    sync_stream();
    s.h2c_nk = c.nk;
    s.h2c_state = 1;
    return true;
}

static void ensure_h2_layout(SRModelSet &s) {
    if (s.d_h2_params.p) return;
    s.d_h2_params.upload(s.h2.params.data(), s.h2.params.size());
    s.d_h2_chunks.upload(s.h2.chunks.data(), s.h2.chunks.size());
    s.d_h2_center.upload(s.h2.center.data(), s.h2.center.size());
    s.d_h2_scale.upload(s.h2.scale.data(), s.h2.scale.size());
    sync_stream();
}

void ensure_bx3_layout(SRModelSet &s) {
    if (s.d_bx3_params.p && !s.bx3_stale) return;
    s.bx3_stale = false;
    s.d_bx3_params.upload(s.bx3.params.data(), s.bx3.params.size());
    s.d_bx3_chunks.upload(s.bx3.chunks.data(), s.bx3.chunks.size());
    s.d_bx3_center.upload(s.bx3.center.data(), s.bx3.center.size());
    sync_stream();
}

// The group table lives with the SET (a hybrid set's two halves, or sets scored in turn, each keep theirs: no re-upload -- and
// no stream synchronisation, which a captured serving tick could not take -- in steady state).  `uploaded`: the caller
// synchronises the stream once its launches are out (first call with this grouping only; the copy source is the table's own vector).
static const int *group_table(SRModelSet &set, std::vector<int> &&gcb, bool &uploaded) {
    for (auto &gt : set.group_tables)
        if (gt->host == gcb) return gt->dev.p;
    constexpr size_t MAX_GROUP_TABLES = 8;
    if (set.group_tables.size() < MAX_GROUP_TABLES) {
        set.group_tables.push_back(std::make_unique<SRModelSet::GroupTable>());
        set.group_table_next = set.group_tables.size() - 1;
    }
    auto &gt = *set.group_tables[set.group_table_next];
    set.group_table_next = (set.group_table_next + 1) % MAX_GROUP_TABLES;
    sync_stream();                        // (a replaced table may still be read by a launch in flight)
    gt.host = std::move(gcb);
    gt.dev.upload(gt.host.data(), gt.host.size());
    uploaded = true;
    return gt.dev.p;
}

// ---- one launcher per engine: fills its launch struct, formats last_score_kernel(), launches ----

struct PassArgs {              // what every engine's launch struct carries
    const float *X;
    const TileDesc *tiles;
    const int *d_gcb;
    double *partial;
    float *frame_ll;
    int64_t n_frames;
    int dim, n_models, clamp, n_groups, n_tiles;
    float band_hi;
};
template <class A>
static A common_args(const PassArgs &c) {
    A a;
    a.X = c.X;
    a.tiles = c.tiles;
    a.partial = c.partial;
    a.frame_ll = c.frame_ll;
    a.n_frames = c.n_frames;
    a.dim = c.dim;
    a.n_models = c.n_models;
    a.clamp = c.clamp;
    a.n_groups = c.n_groups;
    a.n_tiles = c.n_tiles;
    a.band_hi = c.band_hi;
    return a;
}

static void launch_shared_f16(SRModelSet &set, SRBatch &feat, TileTable &tt, const ScorePlan &plan, const PassArgs &c) {
    auto &w = ws();
    const ScoreOptions &opt = score_options();
    const int h2s_shape = plan.h2s_shape;
    ensure_h2s_layout(set);
    const PackedH2Shared &h = set.h2s;
    // pre-pass: the reference model's per-frame LL (natural log, no clamp) = the offset
    w.ref_ll.ensure((size_t)std::max<int64_t>(1, feat.n_rows));
    w.ref_partial.ensure((size_t)tt.n_tiles);         // (the generic split kernel's unit: a 32-frame tile per wave, as this engine's)
    {
        PassArgs rc = c;
        rc.partial = w.ref_partial.p;
        rc.frame_ll = w.ref_ll.p;
        rc.n_models = 1;
        rc.clamp = 0;
        rc.n_groups = 1;
        rc.band_hi = -INFINITY;
        MfmaLaunch r = common_args<MfmaLaunch>(rc);
        r.params = reinterpret_cast<const float4 *>(set.d_h2s_ref_params.p);
        r.chunks = set.d_h2s_ref_chunks.p;
        r.group_chunk_begin = set.d_h2s_ref_gcb.p;
        r.center = set.d_h2s_ref_center.p;
        r.scale = set.d_h2s_ref_scale.p;
        r.oor_flag = w.counters.oor_p();
        ScopedKernelTimer t(T_SCORE_REF);
        // (high parts only: a third of the MFMAs; an offset a few nats off is as good as an exact one, gmm_score_split.hip)
        launch_score_split(r, SPLIT_F16X1, h.ref.ks, 1);
    }
    const int n_blocks = (int)h.blocks.size();
    w.exc_list.ensure((size_t)std::max(1, tt.n_tiles) * n_blocks * 2 + (size_t)(std::max(1, tt.n_tiles) + 1) * n_blocks);
    H2sLaunch a = common_args<H2sLaunch>(c);
    a.params = set.d_h2s_params.p;
    a.blocks = set.d_h2s_blocks.p;
    a.group_block_begin = c.d_gcb;
    a.center = set.d_h2s_center.p;
    a.scale = set.d_h2s_scale.p;
    a.q_desc = set.d_h2s_qdesc.p;
    a.l_desc = set.d_h2s_ldesc.p;
    a.ref_ll = w.ref_ll.p;
    a.oor_flag = w.counters.oor_p();
    a.exc_list = w.exc_list.p;
    a.exc_count = w.counters.exc_count_p();
    a.n_blocks = n_blocks;
    a.n_mix_tiles = h.n_tiles;
    a.log2_k = (float)std::log2((double)h.n_tiles * MT);
    a.force_exc = opt.h2s_force_exc;
    a.shape = h2s_shape;
    bool compact = false;
    if (h2s_shape == 2) {      // the pipelined kernel walks work items: ragged tail tiles share a wave
        ensure_work_table(tt, opt.h2s_pack_tails != 0);
        a.tiles = tt.d_tiles_work.p;
        a.n_work = tt.n_work;
        // ... on the compact image where the form applies (score_h2s_shape = 5: on the flat one, for A/B), two blocks behind one
        // quadratic-half image (score_h2s_shape = 6: one per block, for A/B)
        compact = opt.h2s_shape != 5 && ensure_h2c_layout(set);
        if (compact) {
            a.pair = opt.h2s_shape != 6;
            a.c_params = set.d_h2c_params.p;
            a.c_blocks = set.d_h2c_blocks.p;
            a.c_q_desc = set.d_h2c_qdesc.p;
            a.c_l_desc = set.d_h2c_ldesc.p;
        }
    }
    snprintf(g_last_kernel, sizeof(LastKernel::name),
             "%s<%d,%d,%s>%s (shared sigma: quadratic half once per %d models; split-fp16 MFMA, "
             "3 products as one contraction; reference-offset log-sum-exp)", h2s_shape == 2 ? "gmm_score_h2p_kernel" : (h2s_shape == 3 && h2s_msplit_direct(h.klf)) ? "gmm_score_h2m_kernel" : "gmm_score_h2s_kernel",
             compact ? set.h2c_nk : h.kqf, compact ? set.h2c_nk : h.klf,
             h2s_shape == 2 ? "waves=12, pipelined in the wave" : h2s_shape == 1 ? "waves=12" : h2s_shape == 3 ? "waves=4 on one tile, models split" : "waves=4",
             compact ? "/compact" : "", a.pair ? 2 * SHARED_SB : SHARED_SB);
    ScopedKernelTimer t(T_SCORE);
    const int n_launches = launch_score_h2_shared(a, h.kqf, h.klf);
    const size_t len = strlen(g_last_kernel);
    snprintf(g_last_kernel + len, sizeof(LastKernel::name) - len, " [%d launches per pass]", n_launches);
}

static void launch_shared_bf16(SRModelSet &set, const PassArgs &c) {
    ensure_shared_layout(set);
    SharedLaunch a = common_args<SharedLaunch>(c);
    a.params = set.d_shared_params.p;
    a.blocks = set.d_shared_blocks.p;
    a.group_block_begin = c.d_gcb;
    a.center = set.d_shared_center.p;
    a.n_mix_tiles = set.shared.n_tiles;
    snprintf(g_last_kernel, sizeof(LastKernel::name),
             "gmm_score_bx3_shared_kernel<%d,%d> (shared sigma: quadratic half once per %d models; split-bf16 MFMA)",
             set.shared.kq, set.shared.kl, SHARED_SB);
    ScopedKernelTimer t(T_SCORE);
    launch_score_bx3_shared(a, set.shared.kq, set.shared.kl);
}

static void launch_split(SRModelSet &set, const ScorePlan &plan, const PassArgs &c) {
    const bool use_h2 = plan.engine == Engine::SPLIT_F16;
    if (use_h2) ensure_h2_layout(set); else ensure_bx3_layout(set);
    const PackedSplit &split = use_h2 ? set.h2 : set.bx3;
    MfmaLaunch a = common_args<MfmaLaunch>(c);
    a.params = use_h2 ? reinterpret_cast<const float4 *>(set.d_h2_params.p) : reinterpret_cast<const float4 *>(set.d_bx3_params.p);
    a.chunks = use_h2 ? set.d_h2_chunks.p : set.d_bx3_chunks.p;
    a.group_chunk_begin = c.d_gcb;
    a.center = use_h2 ? set.d_h2_center.p : set.d_bx3_center.p;
    if (use_h2) {
        a.scale = set.d_h2_scale.p;
        a.oor_flag = ws().counters.oor_p();
    }
    ScopedKernelTimer t(T_SCORE);
    if (use_h2 && plan.splitp_w) {
        snprintf(g_last_kernel, sizeof(LastKernel::name),
                 "gmm_score_splitp_kernel<f16x2,%d,waves=%d> (3 x v_mfma_f32_32x32x16_f16 per fp32 product; log-sum-exp pipelined "
                 "under the next chunk's MFMAs)", split.ks, plan.splitp_w);
        if (!launch_score_splitp(a, SPLIT_F16X2, split.ks, plan.splitp_w, plan.split_cpm))
            fail("no wide split-fp16 kernel for %d contraction steps and %d waves", split.ks, plan.splitp_w);
    } else if (use_h2) {
        snprintf(g_last_kernel, sizeof(LastKernel::name),
                 "gmm_score_split_kernel<f16x2,%d,%d> (3 x v_mfma_f32_32x32x16_f16 per fp32 product)", split.ks, plan.FT);
        launch_score_split(a, SPLIT_F16X2, split.ks, plan.FT);
    } else {
        snprintf(g_last_kernel, sizeof(LastKernel::name),
                 "gmm_score_split_kernel<bf16x3,%d,%d> (6 x v_mfma_f32_32x32x16_bf16 per fp32 product)", split.ks, plan.FT);
        launch_score_split(a, SPLIT_BF16X3, split.ks, plan.FT);
    }
}

static void launch_vector(SRModelSet &set, const ScorePlan &plan, const PassArgs &c) {
    const int DP = set.host.dp;
    ScoreArgs a = common_args<ScoreArgs>(c);
    a.params = reinterpret_cast<const float4 *>(set.d_params.p);
    a.center = set.d_center0.p;
    a.chunks = set.d_chunks.p;
    a.group_chunk_begin = c.d_gcb;
    ScopedKernelTimer t(T_SCORE);
    if (DP > MAX_REG_DIM) {
        snprintf(g_last_kernel, sizeof(LastKernel::name), "gmm_score_wide_kernel (vector ALU, %d slices of %d dims)", DP / WIDE_DC, WIDE_DC);
        launch_score_wide(a, DP);
    } else {
        const bool packed = score_options().packed >= 0 && plan.F >= 2;
        snprintf(g_last_kernel, sizeof(LastKernel::name), "gmm_score_kernel<%d,%d,%s> (vector ALU)", DP, plan.F, packed ? "packed" : "scalar");
        launch_score_vector(a, DP, plan.F, packed);
    }
}

// SCORE_HOST_DELIVER honoured: the landing area (allocated once) and the pass's sequence number
static FinalizeDelivery prepare_delivery(size_t n_counters) {
    auto &w = ws();
    if (!w.deliver.p) {
        w.deliver.ensure(sizeof(DeliverHeader) + HOST_DELIVER_MAX_BYTES + 64, hipHostMallocCoherent | hipHostMallocMapped);
        std::memset(w.deliver.p, 0, w.deliver.n);
        SR_HIP(hipHostGetDevicePointer(&w.deliver_dev, w.deliver.p, 0));
    }
    FinalizeDelivery dl;
    dl.host = reinterpret_cast<DeliverHeader *>(w.deliver_dev);
    dl.counters = w.counters.base();
    dl.n_counters = (int)n_counters;
    dl.seq = ++w.deliver_seq ? w.deliver_seq : ++w.deliver_seq;      // (0 is "nothing yet")
    return dl;
}

// finalize over the workspace's partial sums, and the result every pass hands back
static ScoreResult finalize_pass(SRBatch &feat, int S, TileTable &tt, int per_tile, const FlushPass &fp, const FinalizeDelivery &dl,
                                 const float *frame_ll, const int *d_oor) {
    auto &w = ws();
    const int U = feat.n_utt;
    w.ensure_results((size_t)std::max(1, U), (size_t)S);
    const size_t n_sums = (size_t)std::max(1, U) * S;
    if (U > 0) {
        ScopedKernelTimer t(T_FINALIZE);
        launch_finalize(w.partial.p, tt, U, S, per_tile, w.sums_p(), w.argmax_p(n_sums), fp.list, fp.count, fp.cap, dl);
    }
    SR_HIP(hipGetLastError());
    ScoreResult r;
    r.d_sums = w.sums_p();
    r.d_argmax = w.argmax_p(n_sums);
    r.d_frame_ll = tt.n_tiles > 0 ? frame_ll : nullptr;
    r.d_oor = d_oor;
    r.d_flush_count = fp.count;
    r.d_flush_list = fp.list;
    r.flush_cap = fp.cap;
    r.tiles = &tt;
    return r;
}

static ScoreResult score_hybrid(SRModelSet &set, SRBatch &feat, bool want_frame_ll, int flags, float *frame_ll_dst);

ScoreResult score_device(SRModelSet &set, SRBatch &feat, bool want_frame_ll, int flags, float *frame_ll_dst) {
    ensure_device();
    if (feat.kind != SRBatch::FEATURES) fail("scoring needs a feature batch");
    feat.bind_device();
    if (set.device != ctx().device)
        fail("model set lives on device %d, the calling thread is on device %d", set.device, ctx().device);
    if (feat.dim != set.host.dim)
        fail("feature dim %d != model dim %d", feat.dim, set.host.dim);
    const ScoreOptions &opt = score_options();
    if (set.hy_good && opt.engine == 0) return score_hybrid(set, feat, want_frame_ll, flags, frame_ll_dst);
    const int S = set.host.n_models;
    const ScorePlan plan = plan_score(set, feat.n_rows, feat.n_utt, opt, flags, ctx().n_cu);
    TileTable &tt = feat.tiles_for(plan.tile_frames);

    auto &w = ws();
    const size_t n_counters = 4 + 2 * set.h2s.blocks.size();      // (shared-sigma engine: exception entries and items per block)
    w.counters.begin(n_counters, (flags & SCORE_HOST_DELIVER) != 0);
    FinalizeDelivery dl{nullptr, nullptr, 0, 0u};
    if ((flags & SCORE_HOST_DELIVER) && !want_frame_ll && !frame_ll_dst && host_deliverable((size_t)feat.n_utt, (size_t)S))
        dl = prepare_delivery(n_counters);
    const FlushPass fp = prepare_flush(set, tt.n_tiles, flags);
    if (frame_ll_dst) want_frame_ll = true;
    if (want_frame_ll && !frame_ll_dst && tt.n_tiles > 0) w.frame_ll.ensure((size_t)S * feat.n_rows);
    float *const fll = !want_frame_ll ? nullptr : frame_ll_dst ? frame_ll_dst : w.frame_ll.p;
    if (tt.n_tiles > 0) {
        std::vector<int> gcb = plan_groups(set, plan, tt.n_tiles, opt, ctx().n_cu);
        PassArgs c;
        c.n_groups = (int)gcb.size() - 1;
        bool uploaded = false;
        c.d_gcb = group_table(set, std::move(gcb), uploaded);
        w.partial.ensure((size_t)tt.n_tiles * S * plan.per_tile);
        c.X = feat.data.p;
        c.tiles = tt.d_tiles.p;
        c.partial = w.partial.p;
        c.frame_ll = fll;
        c.n_frames = feat.n_rows;
        c.dim = feat.dim;
        c.n_models = S;
        // 0 off, 1 the reference's clamp, 2 the same with "all terms underflowed" reported as -inf (a half of a hybrid set)
        c.clamp = (flags & 1) ? ((flags & SCORE_NO_FLUSH) ? 2 : 1) : 0;
        c.n_tiles = tt.n_tiles;
        c.band_hi = fp.band_hi;
        switch (plan.engine) {
            case Engine::SHARED_F16: launch_shared_f16(set, feat, tt, plan, c); break;
            case Engine::SHARED_BF16: launch_shared_bf16(set, c); break;
            case Engine::SPLIT_F16:
            case Engine::SPLIT_BF16: launch_split(set, plan, c); break;
            case Engine::VECTOR: launch_vector(set, plan, c); break;
        }
        SR_HIP(hipGetLastError());
        if (uploaded) sync_stream();
    }
    ScoreResult r = finalize_pass(feat, S, tt, plan.per_tile, fp, dl, fll, plan.writes_oor && tt.n_tiles > 0 ? w.counters.oor_p() : nullptr);
    if (dl.host && feat.n_utt > 0) {
        r.h_deliver = reinterpret_cast<const volatile DeliverHeader *>(w.deliver.p);
        r.deliver_seq = dl.seq;
        w.counters.delivered(n_counters);
    }
    return r;
}

// The two sub-sets of a hybrid set, then the merge (gmm_merge_kernel) and the usual finalize.
static ScoreResult score_hybrid(SRModelSet &set, SRBatch &feat, bool want_frame_ll, int flags, float *frame_ll_dst) {
    auto &w = ws();
    const int S = set.host.n_models;
    const size_t n = (size_t)S * (size_t)std::max<int64_t>(1, feat.n_rows);
    w.hy_a.ensure(n);
    w.hy_b.ensure(n);
    // the ill-conditioned mixtures first (vector engine: the only layout that sub-set carries), then the rest -- so
    // that the fp16 engines' saturation flag of the second call is the one left in the workspace
    // (the partial-product band is the merge's business: the merged value, against the WHOLE model's parameters)
    score_device(*set.hy_bad, feat, true, flags | SCORE_NO_FLUSH, w.hy_b.p);
    const ScoreResult good = score_device(*set.hy_good, feat, true, flags | SCORE_NO_FLUSH, w.hy_a.p);
    char good_name[sizeof(LastKernel::name)];
    snprintf(good_name, sizeof(good_name), "%s", g_last_kernel);
    TileTable &tt = feat.tiles_for(256);
    const FlushPass fp = prepare_flush(set, tt.n_tiles, flags);
    float *out = nullptr;
    if (want_frame_ll || frame_ll_dst) {
        if (!frame_ll_dst) w.frame_ll.ensure(n);
        out = frame_ll_dst ? frame_ll_dst : w.frame_ll.p;
    }
    if (tt.n_tiles > 0) {
        w.partial.ensure((size_t)tt.n_tiles * S);
        ScopedKernelTimer t(T_SCORE);
        launch_merge(w.hy_a.p, w.hy_b.p, tt, S, feat.n_rows, (flags & 1) ? 1 : 0, w.partial.p, out, fp.band_hi);
        SR_HIP(hipGetLastError());
    }
    snprintf(g_last_kernel, sizeof(LastKernel::name), "hybrid: %d ill-conditioned mixtures on the vector ALU + %.150s", set.hy_bad_mixtures, good_name);
    return finalize_pass(feat, S, tt, 1, fp, FinalizeDelivery{nullptr, nullptr, 0, 0u}, out, good.d_oor);
}

struct ResultStaging {
    PinnedBuf<double> sums;
    PinnedBuf<int> argmax;
    PinnedBuf<float> frame_ll;
    PinnedBuf<int> oor;
    PinnedBuf<double> open;
};
static ResultStaging &staging() { return per_device<ResultStaging>(); }   // leaked on purpose (no hipHostFree at exit)

// SCORE_HOST_DELIVER: the pass's last workgroup wrote everything into page-locked host memory and released `seq`.
// Poll for it (a wake-up from hipStreamSynchronize costs more than the kernels' tail); now and then ask the stream --
// a faulted queue must not leave this thread spinning.
static void wait_delivery(const ScoreResult &r) {
    const volatile DeliverHeader *h = r.h_deliver;
    for (unsigned spins = 1;; spins++) {
        if (__atomic_load_n(&h->seq, __ATOMIC_ACQUIRE) == r.deliver_seq) return;
        if ((spins & 0xfff) == 0) {
            const hipError_t e = hipStreamQuery(ctx().stream);
            if (e == hipSuccess) {
                if (__atomic_load_n(&h->seq, __ATOMIC_ACQUIRE) == r.deliver_seq) return;
                fail("scoring pass finished without delivering its results (sequence %u, found %u)", r.deliver_seq, h->seq);
            }
            if (e != hipErrorNotReady) SR_HIP(e);
        }
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
        __builtin_ia32_pause();
#endif
    }
}

// The results a delivering pass left in host memory -> the caller's arrays.  DELIVERED_SATURATED: a frame left the fp16 engine's
// range (nothing copied); DELIVERED_OVERFLOW: more band pairs (`n_flush`) than the list holds (nothing copied).
enum { DELIVERED_OK, DELIVERED_SATURATED, DELIVERED_OVERFLOW };
static int fetch_delivered(SRModelSet &set, SRBatch &feat, const ScoreResult &r, double *sums_out, int *argmax_out, int &n_flush) {
    const size_t U = (size_t)feat.n_utt, S = (size_t)set.host.n_models;
    wait_delivery(r);
    const volatile DeliverHeader *h = r.h_deliver;
    if (r.d_oor && h->oor != 0) return DELIVERED_SATURATED;
    n_flush = r.d_flush_count ? h->n_flush : 0;
    if (n_flush > r.flush_cap) return DELIVERED_OVERFLOW;
    double *h_sums = const_cast<double *>(reinterpret_cast<const volatile double *>(h + 1));
    int *h_arg = reinterpret_cast<int *>(h_sums + U * S);
    if (n_flush) flush_resolve_host(set, feat, *r.tiles, r.d_flush_list, n_flush, h_sums, h_arg);
    if (sums_out) std::memcpy(sums_out, h_sums, U * S * sizeof(double));
    if (argmax_out) std::memcpy(argmax_out, h_arg, U * sizeof(int));
    return DELIVERED_OK;
}

// The pass's two counters, and what the caller asked for, into the pinned staging buffers (large per-frame arrays straight into
// `frame_ll_out`); waits for them.  Returns where the staged argmax values are (behind the sums when they came in one copy).
// `open`: the open-set decision comes with them -- the kernel first, over every utterance, unless `open_decided` says the device's
// block already holds the decision of these sums (gmm_flush.hip redid the patched utterances' itself).
static const int *stage_results(const ScoreResult &r, SRBatch &feat, size_t U, size_t S, bool want_sums, bool want_argmax, size_t fll_n,
                                bool stage_fll, float *frame_ll_out, const OpenSetFetch *open, bool &open_decided) {
    auto &st = staging();
    if (open && U) {
        auto &w = ws();
        w.open.ensure(open_set_doubles(U));
        st.open.ensure(open_set_doubles(U));
        if (!open_decided)
            launch_open_set(r.d_sums, (int)S, open->rule, feat.d_offsets.p, nullptr, nullptr, (int)U, w.open.p, open_set_labels(w.open.p, U));
        open_decided = true;
        SR_HIP(hipMemcpyAsync(st.open.p, w.open.p, open_set_bytes(U), hipMemcpyDeviceToHost, ctx().stream));
    }
    st.oor.p[0] = st.oor.p[1] = 0;
    // (the workspace keeps the two counters, and the argmax values behind the sums, side by side: one copy each)
    copy_pass_flags(r, st.oor.p, ctx().stream);
    const bool together = want_sums && want_argmax && U && (const void *)r.d_argmax == (const void *)(r.d_sums + U * S);
    const int *h_argmax = nullptr;
    if (together) {
        st.sums.ensure(U * S + (U + 1) / 2);
        SR_HIP(hipMemcpyAsync(st.sums.p, r.d_sums, results_bytes(U, S), hipMemcpyDeviceToHost, ctx().stream));
        h_argmax = reinterpret_cast<const int *>(st.sums.p + U * S);
    } else {
        if (want_sums && U) {
            st.sums.ensure(U * S);
            SR_HIP(hipMemcpyAsync(st.sums.p, r.d_sums, U * S * sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
        }
        if (want_argmax && U) {
            st.argmax.ensure(U);
            SR_HIP(hipMemcpyAsync(st.argmax.p, r.d_argmax, U * sizeof(int), hipMemcpyDeviceToHost, ctx().stream));
            h_argmax = st.argmax.p;
        }
    }
    if (fll_n) {
        if (stage_fll) {
            st.frame_ll.ensure(fll_n);
            SR_HIP(hipMemcpyAsync(st.frame_ll.p, r.d_frame_ll, fll_n * sizeof(float), hipMemcpyDeviceToHost, ctx().stream));
        } else {
            SR_HIP(hipMemcpyAsync(frame_ll_out, r.d_frame_ll, fll_n * sizeof(float), hipMemcpyDeviceToHost, ctx().stream));
        }
    }
    sync_stream();
    return h_argmax;
}

// Copies the last scoring call's results to host memory through pinned staging.  With the reference's clamp on, the
// (tile, model) pairs gmm_finalize_kernel left out because a frame of theirs sits in the partial-product band (lse.hpp)
// are resolved first (gmm_flush.hip patches the device results; nothing to do, and nothing extra copied but one int,
// when there are none -- the case of real data).
bool fetch_results(SRModelSet &set, SRBatch &feat, int flags, const ScoreResult &r_in, double *sums_out, int *argmax_out,
                   float *frame_ll_out, const OpenSetFetch *open) {
    auto &st = staging();
    ScoreResult r = r_in;
    const size_t U = (size_t)feat.n_utt, S = (size_t)set.host.n_models, n_frames = (size_t)feat.n_rows;
    struct ResetCap {                       // an enlarged band list is for this batch only
        bool armed = false;
        ~ResetCap() { if (armed) ws().flush_min_cap = 0; }
    } reset_cap;
    if (r.h_deliver && open) fail("open-set decision: the pass delivered its results to the host by itself");
    if (r.h_deliver) {
        int n_flush = 0;
        const int how = fetch_delivered(set, feat, r, sums_out, argmax_out, n_flush);
        if (how != DELIVERED_OVERFLOW) return how == DELIVERED_OK;
        // more pairs than the list holds: the pass again with a list of that length, through the general path below
        ws().flush_min_cap = (size_t)n_flush;
        reset_cap.armed = true;
        r = score_device(set, feat, false, flags & ~SCORE_HOST_DELIVER);
    }
    st.oor.ensure(2);
    const size_t fll_n = (frame_ll_out && r.d_frame_ll) ? S * n_frames : 0;
    const bool stage_fll = fll_n > 0 && fll_n * sizeof(float) <= ((size_t)64 << 20);
    const int *h_argmax = nullptr;
    bool rescored = false;
    bool open_decided = false;              // the device's decision block belongs to the sums of `r` as they stand
    for (;;) {
        h_argmax = stage_results(r, feat, U, S, sums_out != nullptr, argmax_out != nullptr, fll_n, stage_fll, frame_ll_out, open, open_decided);
        if (r.d_oor && st.oor.p[0] != 0) return false;
        int n_flush = st.oor.p[1];
        if (n_flush == 0) break;
        if (n_flush > r.flush_cap) {
            // more pairs than the list holds (the counter kept counting): the pass again with a list of that length -- and ITS
            // sums, argmax and count staged afresh (the loop's top), so that nothing below depends on the two passes having
            // left the same bits in the same places
            if (rescored) fail("partial-product band: %d (tile, model) pairs noted, list of %d", n_flush, r.flush_cap);
            rescored = true;
            ws().flush_min_cap = (size_t)n_flush;
            reset_cap.armed = true;
            const bool own = r.d_frame_ll && r.d_frame_ll != ws().frame_ll.p;
            r = score_device(set, feat, r.d_frame_ll != nullptr, flags, own ? const_cast<float *>(r.d_frame_ll) : nullptr);
            open_decided = false;
            continue;
        }
        if (!fll_n && sums_out && argmax_out && U && !open) {
            // Sums and argmax are already here: complete the HOST copies (one more wait for the tiles' exact sums; what sr_multi's
            // pieces do) instead of patching the device's and copying everything a second time -- two waits, two uploads, two
            // kernels and a copy of all U x S sums less per call.
            // Invariant: the staged sums, the staged argmax and the list all come from the SAME pass `r` (an overflow re-score
            // restarts the loop and stages its own).  The device-resident d_sums / d_argmax stay UNPATCHED on this branch --
            // they are the workspace's, valid until the next scoring call, and nothing reads them after this one returns.
            flush_resolve_host(set, feat, *r.tiles, r.d_flush_list, n_flush, st.sums.p, const_cast<int *>(h_argmax));
            break;
        }
        // (an open-set fetch: the decision staged above was taken on sums without the noted pairs and goes nowhere -- the
        // patched utterances are decided again behind the patch, and the next turn of the loop stages the block afresh)
        flush_resolve(set, feat, *r.tiles, r.d_flush_list, n_flush, const_cast<double *>(r.d_sums),
                      const_cast<int *>(r.d_argmax), const_cast<float *>(r.d_frame_ll), open ? &open->rule : nullptr,
                      open ? ws().open.p : nullptr, open ? open_set_labels(ws().open.p, U) : nullptr);
        r.d_flush_count = nullptr;          // resolved: copy the patched results out
    }
    if (open && U) {
        std::memcpy(open->margin_out, st.open.p, U * sizeof(double));
        std::memcpy(open->label_out, open_set_labels(st.open.p, U), U * sizeof(int));
    }
    if (sums_out && U) std::memcpy(sums_out, st.sums.p, U * S * sizeof(double));
    if (argmax_out && U) std::memcpy(argmax_out, h_argmax, U * sizeof(int));
    if (stage_fll) std::memcpy(frame_ll_out, st.frame_ll.p, fll_n * sizeof(float));
    return true;
}

void score_batch_set(SRModelSet &set, SRBatch &feat, double *sums_out, int *argmax_out,
                     float *frame_ll_out, int flags) {
    // (small result sets land in host memory by themselves: SCORE_HOST_DELIVER, score.hpp)
    // (either result alone too: the legacy ABI's score_all wants one sum, pygmm.cc:98-104, and so does every second EM iteration)
    const int deliver = (!frame_ll_out && (sums_out || argmax_out) && host_deliverable((size_t)feat.n_utt, (size_t)set.host.n_models)) ? SCORE_HOST_DELIVER : 0;
    score_resolved(set, feat, frame_ll_out != nullptr, flags, deliver, sums_out, argmax_out, frame_ll_out);
}

// The sibling of score_batch_set with the open-set decision: the same pass, the decision kernel behind finalize (and behind the
// patch of gmm_flush.hip), labels and margins back with the sums in the fetch's one wait.  No SCORE_HOST_DELIVER: the decision
// reads the device's sums.
void score_batch_set_open(SRModelSet &set, SRBatch &feat, double *sums_out, const OpenSetFetch &open, int flags) {
    score_resolved(set, feat, false, flags, 0, sums_out, nullptr, nullptr, &open);
}

}  // namespace sr

// Work items of the pipelined shared-sigma kernel over a 32-frame tile table: tiles in order, every full one an item of its own, the
// ragged tails (1000-frame utterances leave 8 of 32 columns: 2.3 % of the pass's MFMAs on dead frames) packed greedily, in order,
// up to four and up to 32 columns to an item, all packed items together at the END of the list (pack_tail_tiles, score_plan.hpp).
// The table is padded with empty items to whole rounds of H2P_ROUND_ITEMS = 8 workgroups x 12 waves: the kernel reads
// (tiles + n_tiles)[unit] for every unit of a launched round without a bound of its own.
namespace sr {
void ensure_work_table(TileTable &tt, bool pack_tails) {
    if ((tt.n_work > 0 && tt.work_packed == pack_tails) || tt.n_tiles == 0) return;
    static_assert(sizeof(TileDesc) == sizeof(int4), "work items travel in the tile table's buffer");
    // (pack_tail_tiles, score_plan.cpp: full tiles in order, the packed items together at the end of the list)
    std::vector<int> counts(tt.h_tiles.size());
    for (size_t t = 0; t < counts.size(); t++) counts[t] = tt.h_tiles[t].count;
    const std::vector<WorkItem> items = pack_tail_tiles(counts, tt.frames_per_tile, pack_tails);
    std::vector<int4> work(items.size());
    for (size_t i = 0; i < items.size(); i++) work[i] = make_int4(items[i].t[0], items[i].t[1], items[i].t[2], items[i].t[3]);
    tt.n_work = (int)work.size();
    tt.work_packed = pack_tails;
    work.resize(((work.size() + H2P_ROUND_ITEMS - 1) / H2P_ROUND_ITEMS) * H2P_ROUND_ITEMS, make_int4(-1, -1, -1, -1));
    std::vector<TileDesc> both(tt.h_tiles);
    both.resize(tt.h_tiles.size() + work.size());
    std::memcpy(both.data() + tt.h_tiles.size(), work.data(), work.size() * sizeof(int4));
    if (tt.stage_tiles.h.p && both.size() * sizeof(TileDesc) <= STAGED_TABLE_MAX_BYTES) {      // a rebuilt table of a reused batch
        tt.stage_work.send(tt.d_tiles_work, both.data(), both.size());
        return;
    }
    tt.d_tiles_work.upload(both.data(), both.size());
    sync_stream();
}
}  // namespace sr

sr::TileTable &SRBatch::tiles_for(int frames_per_tile) {
    sr::TileTable *found = nullptr;
    for (auto &t : tile_tables)
        if (t->frames_per_tile == frames_per_tile) {
            if (!t->stale) return *t;
            found = t.get();
        }
    // (a stale table is rebuilt where it stands: the uploads below are on the stream the kernels that read the old contents
    // were launched on, so they run behind them)
    std::unique_ptr<sr::TileTable> fresh;
    if (!found) {
        fresh = std::make_unique<sr::TileTable>();
        fresh->frames_per_tile = frames_per_tile;
    }
    sr::TileTable *const tt = found ? found : fresh.get();
    tt->stale = false;
    tt->n_work = 0;
    tt->work_packed = false;
    std::vector<sr::TileDesc> tiles;
    std::vector<int> begin(n_utt + 1, 0);
    for (int u = 0; u < n_utt; u++) {
        begin[u] = (int)tiles.size();
        for (int64_t s = offsets[u]; s < offsets[u + 1]; s += frames_per_tile) {
            sr::TileDesc td;
            td.start = s;
            td.count = (int32_t)std::min<int64_t>(frames_per_tile, offsets[u + 1] - s);
            td.utt = u;
            tiles.push_back(td);
        }
    }
    begin[n_utt] = (int)tiles.size();
    tt->n_tiles = (int)tiles.size();
    tt->h_tiles = tiles;
    if (found && tiles.size() * sizeof(sr::TileDesc) <= sr::STAGED_TABLE_MAX_BYTES && begin.size() * sizeof(int) <= sr::STAGED_TABLE_MAX_BYTES) {
        // the table of a batch that is being reused: no host wait (common.hpp: StagedUpload)
        tt->stage_tiles.send(tt->d_tiles, tiles.data(), tiles.size());
        tt->stage_begin.send(tt->d_utt_tile_begin, begin.data(), begin.size());
        return *tt;
    }
    tt->d_tiles.upload(tiles.data(), tiles.size());
    tt->d_utt_tile_begin.upload(begin.data(), begin.size());
    sr::sync_stream();
    if (fresh) tile_tables.push_back(std::move(fresh));
    return *tt;
}
