// score.hpp -- host entry points of the scoring path shared between translation units.
#pragma once

#include "batch.hpp"
#include "gmm_model.hpp"
#include "score_plan.hpp"

namespace sr {

// internal: leave the partial-product band alone (the two halves of a hybrid set: their merge looks at the merged value)
constexpr int SCORE_NO_FLUSH = 0x400;
// Small result sets of callers that fetch them right away (fetch_results): gmm_finalize_kernel's last workgroup writes sums, argmax
// and the pass's two counters into page-locked host memory and releases a sequence number the host polls for -- no device-to-host
// copies, no stream synchronisation -- and clears the pass's counters for the next pass (no memset in front of it).
constexpr int SCORE_HOST_DELIVER = 0x800;
constexpr size_t HOST_DELIVER_MAX_BYTES = (size_t)64 << 10;
constexpr size_t HOST_DELIVER_MAX_UTTS = 256;      // every utterance's workgroup takes a ticket from ONE counter: 2000 utterances x 1 model
                                                   // (16 KiB of results) lost 80 us per pass to that queue, more than the copies cost
inline bool host_deliverable(size_t n_utt, size_t n_models) {
    return n_utt > 0 && n_utt <= HOST_DELIVER_MAX_UTTS && n_utt * n_models * sizeof(double) + n_utt * sizeof(int) <= HOST_DELIVER_MAX_BYTES;
}
// what the last workgroup leaves in host memory: this header, then double sums[U][S], then int argmax[U]
struct DeliverHeader {
    int oor, n_flush;
    unsigned seq;
    int pad;
};

// The vector-ALU engine, the hybrid sets' merge and the finalize: kernels and launch code in gmm_score.hip.
struct ScoreArgs {
    const float *X;            // [n_frames][dim] row-major fp32
    const TileDesc *tiles;
    const float4 *params;
    const float *center;       // [DP] subtracted from every frame (PackedModels::center)
    const ChunkDesc *chunks;
    const int *group_chunk_begin;  // [G+1]
    double *partial;           // [n_tiles][S][4]  per-wave partial sums
    float *frame_ll;           // [S][n_frames] or nullptr
    int64_t n_frames;
    int dim;
    int n_models;
    int clamp;
    int n_groups, n_tiles;
    float band_hi;             // below it a frame goes to the partial-product path (lse.hpp); -inf: never
};
void launch_score_vector(const ScoreArgs &a, int DP, int F, bool packed);      // DP <= MAX_REG_DIM: gmm_score_kernel<DP, F, packed>
void launch_score_wide(const ScoreArgs &a, int DP);                            // wider rows: gmm_score_wide_kernel
struct FinalizeDelivery {      // SCORE_HOST_DELIVER; host == nullptr: off
    DeliverHeader *host;
    int *counters;             // the pass's counters: [0] saturation flag, [1] flush count, [2] this kernel's ticket, [4 ...]
    int n_counters;
    unsigned seq;
};
void launch_finalize(const double *partial, const TileTable &tt, int n_utt, int n_models, int per_tile, double *sums, int *argmax,
                     int2 *flush_list, int *flush_count, int flush_cap, const FinalizeDelivery &dl);
void launch_merge(const float *a, const float *b, const TileTable &tt, int n_models, int64_t n_frames, int clamp, double *partial,
                  float *out, float band_hi);
struct MfmaLaunch {
    const float *X;
    const TileDesc *tiles;
    const float4 *params;
    const ChunkDesc *chunks;
    const int *group_chunk_begin;
    const float *center;
    const float *scale = nullptr;   // fp16 scheme: per-dimension power-of-two scale of x - center
    double *partial;
    float *frame_ll;
    int *oor_flag = nullptr;        // fp16 scheme: set when a frame saturated (|scaled x'| >= 255)
    int64_t n_frames;
    int dim, n_models, clamp, n_groups, n_tiles;
    float band_hi = -__builtin_inff();   // below it a frame goes to the partial-product path (lse.hpp); -inf: never
};
struct SharedLaunch {
    const float *X;
    const TileDesc *tiles;
    const uint16_t *params;
    const SharedBlock *blocks;
    const int *group_block_begin;
    const float *center;
    double *partial;
    float *frame_ll;
    int64_t n_frames;
    int dim, n_models, n_mix_tiles, clamp, n_groups, n_tiles;
    float band_hi = -__builtin_inff();
};
void launch_score_bx3_shared(const SharedLaunch &a, int KQ, int KL);
constexpr int H2P_ROUND_ITEMS = 96;     // the pipelined kernel's work table is padded to whole rounds of 8 workgroups x 12 waves
struct H2sLaunch {
    const float *X;
    const TileDesc *tiles;
    const uint16_t *params;
    const SharedBlock *blocks;
    const int *group_block_begin;
    const float *center, *scale;
    const uint16_t *q_desc, *l_desc;
    const float *ref_ll;
    double *partial;
    float *frame_ll;
    int *oor_flag;
    int n_work = 0;     // pipelined shape: `tiles` is TileTable::d_tiles_work -- the tiles, then this many work items (+ padding)
    int *exc_list;      // int2 [n_blocks][n_tiles] {tile, listed columns}, then int [n_blocks][n_tiles + 1] (the exception pass's plan)
    int *exc_count;     // [n_blocks] entries, then [n_blocks] items
    int n_blocks;
    int64_t n_frames;
    int dim, n_models, n_mix_tiles, clamp, n_groups, n_tiles;
    float log2_k;
    int force_exc;
    int shape = 0;          // 0: 4-wave workgroups; 1: 12-wave workgroups (`tiles` = 32-frame tiles); 2: 12 waves, pipelined (gmm_score_h2p_kernel)
    // pipelined shape on the COMPACT image (PackedH2Compact; null: on the flat one): what its main kernel reads instead of `params`,
    // `blocks`, `q_desc`, `l_desc` -- the exception pass behind it keeps the flat ones
    const uint16_t *c_params = nullptr;
    const SharedBlock *c_blocks = nullptr;
    const uint16_t *c_q_desc = nullptr, *c_l_desc = nullptr;
    bool pair = false;      // ... two blocks of a group behind one quadratic-half image (score_shapes.hpp: h2q_*); `c_params` is then
                            // readable one image past its end
    float band_hi = -__builtin_inff();
};
int launch_score_h2_shared(const H2sLaunch &a, int KQF, int KLF);
void launch_score_split(const MfmaLaunch &a, int scheme, int KS, int FT);   // a.params = the split image
// gmm_score_splitp.hip: the same engines as ONE wide workgroup per CU (12 or 16 waves, a 32-frame tile each, the chunk's log-sum-exp
// pipelined under the next chunk's MFMAs); `a.tiles` = 32-frame tiles; `waves` from splitp_waves_f16x2 (score_shapes.hpp).
bool launch_score_splitp(const MfmaLaunch &a, int scheme, int KS, int waves, int chunks_per_model);
const char *last_score_kernel();   // name of the kernel variant the last scoring call launched

// Device-resident results of the last scoring call (valid until the next one).
struct ScoreResult {
    const double *d_sums = nullptr;    // [U][S]
    const int *d_argmax = nullptr;     // [U]
    const float *d_frame_ll = nullptr; // [S][n_frames] when requested
    const int *d_oor = nullptr;        // fp16 engines: nonzero when a frame saturated -> results must be redone
    // reference clamp on: (tile, model) pairs with a frame whose value the reference's flushes of partial products may
    // change (lse.hpp), left out of `d_sums` by gmm_finalize_kernel -- `*d_flush_count` of them (it counts past
    // `flush_cap`), to be resolved by flush_resolve before the results are used (fetch_results does)
    const int *d_flush_count = nullptr;
    const int2 *d_flush_list = nullptr;
    int flush_cap = 0;
    const TileTable *tiles = nullptr;  // the tile table the pass ran on
    // SCORE_HOST_DELIVER honoured: where the results arrive (page-locked host memory) and the sequence number that says they have
    const volatile DeliverHeader *h_deliver = nullptr;
    unsigned deliver_seq = 0;
};

// ---- the open-set decision (open_set.hip): best speaker's per-frame margin over the background column against a threshold ----
struct OpenSetRule {
    int bg;                // the background (UBM) column of the sums
    double threshold;      // margin < threshold: rejected (label -1)
};
// the decision of U utterances as one block: double margin[U], then int label[U] -- one copy
inline size_t open_set_bytes(size_t n_utt) { return n_utt * (sizeof(double) + sizeof(int)); }
inline size_t open_set_doubles(size_t n_utt) { return n_utt + (n_utt + 1) / 2; }
inline int *open_set_labels(double *block, size_t n_utt) { return reinterpret_cast<int *>(block + n_utt); }
// bg inside [0, n_models), threshold not a NaN: checked by every entry point before it touches the device
inline void open_set_check(const OpenSetRule &rule, int n_models) {
    if (rule.bg < 0 || rule.bg >= n_models) fail("open-set decision: background column %d outside [0, %d)", rule.bg, n_models);
    if (rule.threshold != rule.threshold) fail("open-set decision: the threshold is a NaN");
}
// The kernel, enqueued on the current stream, over final sums [U][n_models] on the device.  Frame counts: `d_counts` (ints, per
// utterance) when given, else the row offsets `d_off` [U + 1].  `d_utts` (or null: 0 .. n_items - 1) lists the utterances decided.
void launch_open_set(const double *d_sums, int n_models, const OpenSetRule &rule, const int64_t *d_off, const int *d_counts,
                     const int *d_utts, int n_items, double *d_margin, int *d_label);
// sums in host memory: upload, kernel, one copy back
void open_set_decide_host(const double *sums, int U, int S, const OpenSetRule &rule, const int64_t *n_frames, int *label_out,
                          double *margin_out);
// What a fetch carries when the caller wants the decision with the sums: the kernel runs behind finalize over every utterance, and
// again -- over the patched utterances only, as gmm_flush_argmax_kernel does -- behind gmm_flush.hip's patch; labels and margins
// reach the host with the sums of the pass whose results stand.  Such a fetch never takes the host-side patch.
struct OpenSetFetch {
    OpenSetRule rule;
    int *label_out;        // [U], host
    double *margin_out;    // [U], host
};

// Scores every utterance of `feat` against every model of `set`; leaves results on the device.
// `frame_ll_dst`: device buffer [S][n_frames] the per-frame values go to instead of the workspace's own.
ScoreResult score_device(SRModelSet &set, SRBatch &feat, bool want_frame_ll, int flags, float *frame_ll_dst = nullptr);
// The current device's pass counters may be dirty: the next pass clears them itself.  Whatever writes them without going
// through score_device -- a replayed serving graph (stream.cpp) -- calls this before it is enqueued.
void counters_written_elsewhere();
// Same, then copies what the caller asked for to host memory.
void score_batch_set(SRModelSet &set, SRBatch &feat, double *sums_out, int *argmax_out,
                     float *frame_ll_out, int flags);
// Results of the last scoring call -> host memory, through pinned staging buffers.
// Returns false when the fp16 engine reported saturated frames (nothing was copied out: score again
// with SCORE_PRECISE).
bool fetch_results(SRModelSet &set, SRBatch &feat, int flags, const ScoreResult &r, double *sums_out,
                   int *argmax_out, float *frame_ll_out, const OpenSetFetch *open = nullptr);
// score_device + fetch_results; when the fp16 engine reported saturated frames, the whole batch again on the fp32-grade engines.
// `flags`: what the first pass and both fetches run with; `deliver`: SCORE_HOST_DELIVER or 0, for the first pass only.
// Returns the pass whose results stand.
// `open`: the open-set decision of the utterances with it (then `deliver` must be 0: the decision is taken on the device's sums).
inline ScoreResult score_resolved(SRModelSet &set, SRBatch &feat, bool want_frame_ll, int flags, int deliver, double *sums_out, int *argmax_out,
                           float *frame_ll_out, const OpenSetFetch *open = nullptr) {
    const ScoreResult r = score_device(set, feat, want_frame_ll, flags | deliver);
    if (fetch_results(set, feat, flags, r, sums_out, argmax_out, frame_ll_out, open)) return r;
    const ScoreResult r2 = score_device(set, feat, want_frame_ll, flags | SCORE_PRECISE);
    fetch_results(set, feat, flags | SCORE_PRECISE, r2, sums_out, argmax_out, frame_ll_out, open);
    return r2;
}
// The pass's saturation flag and partial-product count -> h_flags[0], [1] (page-locked), left in flight on `stream`: one copy when
// the two counters are adjacent (the workspace keeps them side by side), else one each.
inline void copy_pass_flags(const ScoreResult &r, int h_flags[2], hipStream_t stream) {
    if (r.d_oor && r.d_flush_count == r.d_oor + 1) {
        SR_HIP(hipMemcpyAsync(h_flags, r.d_oor, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
    } else {
        if (r.d_oor) SR_HIP(hipMemcpyAsync(h_flags, r.d_oor, sizeof(int), hipMemcpyDeviceToHost, stream));
        if (r.d_flush_count) SR_HIP(hipMemcpyAsync(h_flags + 1, r.d_flush_count, sizeof(int), hipMemcpyDeviceToHost, stream));
    }
}
// bytes of U x S sums with `ints_per_utt` ints per utterance (the argmax; the VAD tick's second value) right behind them: one copy
inline size_t results_bytes(size_t n_utt, size_t n_models, size_t ints_per_utt = 1) {
    return n_utt * n_models * sizeof(double) + ints_per_utt * n_utt * sizeof(int);
}
// gmm_flush.hip: the frames of the noted (tile, model) pairs again with the reference's own linear-domain arithmetic;
// adds the tiles' sums to `d_sums`, redoes the argmax of the utterances touched, overwrites the per-frame values
// (`open`: the open-set decision of the utterances touched is redone too, into `d_open_margin` / `d_open_label`)
void flush_resolve(SRModelSet &set, SRBatch &feat, const TileTable &tt, const int2 *d_list, int count, double *d_sums,
                   int *d_argmax, float *d_frame_ll, const OpenSetRule *open = nullptr, double *d_open_margin = nullptr,
                   int *d_open_label = nullptr);
// the same for results that already sit in host memory (sums[U][S], argmax[U] of the batch `feat`): patched on the host, one wait
void flush_resolve_host(SRModelSet &set, SRBatch &feat, const TileTable &tt, const int2 *d_list, int count, double *h_sums,
                        int *h_argmax);
int &flush_order_option();     // 2 = partial products as the reference DSO's compiler forms them (default), 1 = source order
void flush_stats(long *calls, long *pairs, long *frames);
// PCM batch -> MFCC -> CMVN/deltas -> all models -> sums + argmax on the host (abi_score.cpp).
}  // namespace sr
struct SRMfcc;
namespace sr {
void predict_pcm(SRMfcc *m, SRModelSet *set, SRBatch *pcm, int nd, double *sums_out, int *argmax_out, int flags,
                 const OpenSetFetch *open = nullptr);
// score_device + fetch with the open-set decision (gmm_score_host.cpp)
void score_batch_set_open(SRModelSet &set, SRBatch &feat, double *sums_out, const OpenSetFetch &open, int flags);
// Packs + uploads a model set on the current device.
void upload_model_set(SRModelSet &s);
// a GMM handle's own one-model set on the current device, packed and uploaded once (abi_model.cpp; invalidated by GMM::drop_single)
std::shared_ptr<SRModelSet> single_model_set(const GMM *g);
// the split-bf16 layout of a set that carries one (s.bx3), on the device: lazily, as every matrix-core layout (em.hip reads it too)
void ensure_bx3_layout(SRModelSet &s);
inline bool split_bf16_in_range(const SRModelSet &s) { return mfma_ok(s.bx3); }      // what the dispatcher asks before it takes that engine (em.hip)

}  // namespace sr
