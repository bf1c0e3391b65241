// abi_batch.cpp -- PCM and feature batches, and what maps a batch to a batch: silence removal, feature normalisation.
#include "abi_internal.hpp"

#include "featnorm.hpp"
#include "featnorm_plan.hpp"
#include "norm_quantile.hpp"
#include "silence.hpp"
#include "silence_plan.hpp"

#include <algorithm>
#include <cstring>
#include <string>

using namespace sr;

std::unique_ptr<SRBatch> sr::feature_batch(const float *X, int64_t n, int dim,
                                           const int64_t *offsets, int n_utt) {
    ensure_device();
    if (n < 0 || dim <= 0 || n_utt < 0) fail("bad batch shape");
    auto b = std::make_unique<SRBatch>();
    b->bind_device();
    b->kind = SRBatch::FEATURES;
    b->n_utt = n_utt;
    b->dim = dim;
    b->n_rows = n;
    b->offsets.assign(offsets, offsets + n_utt + 1);
    if (b->offsets.front() != 0 || b->offsets.back() != n) fail("offsets must run from 0 to n");
    for (int u = 0; u < n_utt; u++)
        if (b->offsets[u + 1] < b->offsets[u]) fail("offsets must be non-decreasing");
    b->data.upload(X, (size_t)n * dim);
    b->d_offsets.upload(b->offsets.data(), b->offsets.size());
    sync_stream();
    return b;
}

extern "C" {

static SRBatch *pcm_batch(const void *pcm, bool is_f32, const int64_t *sample_offsets, int n_utt) {
    ensure_device();
    if (n_utt < 0 || !sample_offsets) fail("bad PCM batch arguments");
    auto b = std::make_unique<SRBatch>();
    b->bind_device();
    b->kind = is_f32 ? SRBatch::PCMF32 : SRBatch::PCM16;
    b->n_utt = n_utt;
    b->offsets.assign(sample_offsets, sample_offsets + n_utt + 1);
    if (b->offsets.front() != 0) fail("sample_offsets[0] must be 0");
    for (int u = 0; u < n_utt; u++)
        if (b->offsets[u + 1] < b->offsets[u]) fail("sample_offsets must be non-decreasing");
    b->n_rows = b->offsets.back();
    if (b->n_rows > 0 && !pcm) fail("null PCM pointer");
    if (is_f32)
        b->data.upload(static_cast<const float *>(pcm), (size_t)b->n_rows);
    else
        b->pcm16.upload(static_cast<const int16_t *>(pcm), (size_t)b->n_rows);
    b->d_offsets.upload(b->offsets.data(), b->offsets.size());
    sync_stream();
    return b.release();
}

SRBatch *sr_batch_from_pcm(const int16_t *pcm, const int64_t *sample_offsets, int n_utt) {
    SR_TRY
    return pcm_batch(pcm, false, sample_offsets, n_utt);
    SR_CATCH(nullptr)
}

SRBatch *sr_batch_from_pcm_f32(const float *pcm, const int64_t *sample_offsets, int n_utt) {
    SR_TRY
    return pcm_batch(pcm, true, sample_offsets, n_utt);
    SR_CATCH(nullptr)
}

SRBatch *sr_batch_from_features(const float *X, int64_t n_frames, int dim,
                                const int64_t *frame_offsets, int n_utt) {
    SR_TRY
    if (!frame_offsets) fail("null frame_offsets");
    if (n_frames > 0 && !X) fail("null X");
    return feature_batch(X, n_frames, dim, frame_offsets, n_utt).release();
    SR_CATCH(nullptr)
}

int sr_batch_reset_features(SRBatch *b, const float *X, int64_t n_frames, int dim, const int64_t *frame_offsets, int n_utt) {
    SR_TRY
    if (!b || !frame_offsets) fail("null argument");
    if (b->kind != SRBatch::FEATURES) fail("sr_batch_reset_features needs a feature batch");
    if (n_frames < 0 || dim <= 0 || n_utt < 0) fail("bad batch shape");
    if (frame_offsets[0] != 0 || frame_offsets[n_utt] != n_frames) fail("offsets must run from 0 to n");
    for (int u = 0; u < n_utt; u++)
        if (frame_offsets[u + 1] < frame_offsets[u]) fail("offsets must be non-decreasing");
    if (n_frames > 0 && !X) fail("null X");
    b->bind_device();
    const bool same_layout = b->n_utt == n_utt && b->offsets.size() == (size_t)n_utt + 1 && std::equal(b->offsets.begin(), b->offsets.end(), frame_offsets);
    b->n_utt = n_utt;
    b->dim = dim;
    b->n_rows = n_frames;
    // (device buffers only ever grow.)  A serving-sized refill goes through the batch's page-locked copies and is left in flight: the
    // caller's matrix is its own again when the call returns, whatever is queued next on the stream runs behind the transfer
    const size_t n_val = (size_t)n_frames * dim;
    const bool staged = n_val * sizeof(float) <= ((size_t)4 << 20) && ((size_t)n_utt + 1) * sizeof(int64_t) <= STAGED_TABLE_MAX_BYTES;
    if (!same_layout) {
        b->offsets.assign(frame_offsets, frame_offsets + n_utt + 1);
        b->invalidate_tiles();
        if (staged) b->stage_offsets.send(b->d_offsets, b->offsets.data(), b->offsets.size());
        else b->d_offsets.upload(b->offsets.data(), b->offsets.size());
    }
    if (staged) {
        b->stage_rows.send(b->data, X, n_val);
        return 0;
    }
    b->data.upload(X, n_val);
    sync_stream();
    return 0;
    SR_CATCH(-1)
}

// A serving decision's worth of PCM (<= 4 MB): through the batch's page-locked copy, transfer left in flight (batch.hpp) -- the stream
// synchronisation sr_batch_update_pcm used to end with was a sixth of a single-utterance decision (round 6).  false: too large, the
// caller uploads and waits.
static bool stage_small_pcm(SRBatch *b, const int16_t *pcm, int64_t n_samples) {
    if ((size_t)n_samples * sizeof(int16_t) > ((size_t)4 << 20) || n_samples <= 0) return false;
    if (!b->stage_done.e) SR_HIP(hipEventCreateWithFlags(&b->stage_done.e, hipEventDisableTiming));
    else if (hipEventQuery(b->stage_done.e) != hipSuccess) SR_HIP(hipEventSynchronize(b->stage_done.e));
    if ((size_t)n_samples > b->h_stage.n) b->h_stage.ensure((size_t)n_samples + (size_t)n_samples / 4);   // (headroom: as StagedUpload)
    if ((size_t)n_samples > b->pcm16.n) b->pcm16.ensure((size_t)n_samples + (size_t)n_samples / 4);
    g_devbuf_epoch++;                       // (contents changed: a captured graph that depends on them is re-captured, as upload())
    // more than 1 MB: in pieces of 256 K samples, a piece's DMA under the host's copy of the next one (64 utterances x 3 s:
    // 0.936 -> 0.905 ms per call; a second piece costs a small batch its 5 us)
    const int64_t PIECE = n_samples <= ((int64_t)512 << 10) ? n_samples : ((int64_t)256 << 10);
    for (int64_t at = 0; at < n_samples; at += PIECE) {
        const size_t n = (size_t)std::min<int64_t>(PIECE, n_samples - at);
        std::memcpy(b->h_stage.p + at, pcm + at, n * sizeof(int16_t));
        SR_HIP(hipMemcpyAsync(b->pcm16.p + at, b->h_stage.p + at, n * sizeof(int16_t), hipMemcpyHostToDevice, ctx().stream));
    }
    SR_HIP(hipEventRecord(b->stage_done.e, ctx().stream));
    return true;
}

int sr_batch_update_pcm(SRBatch *b, const int16_t *pcm, int64_t n_samples) {
    SR_TRY
    if (!b || !pcm) fail("null argument");
    if (b->kind != SRBatch::PCM16) fail("sr_batch_update_pcm needs an int16 PCM batch");
    if (n_samples != b->n_rows) fail("sample count %lld does not match the batch (%lld)", (long long)n_samples, (long long)b->n_rows);
    b->bind_device();
    if (stage_small_pcm(b, pcm, n_samples)) return 0;
    b->pcm16.upload(pcm, (size_t)n_samples);
    sync_stream();
    return 0;
    SR_CATCH(-1)
}

int sr_batch_reset_pcm(SRBatch *b, const int16_t *pcm, const int64_t *sample_offsets, int n_utt) {
    SR_TRY
    if (!b || !sample_offsets) fail("null argument");
    if (b->kind != SRBatch::PCM16) fail("sr_batch_reset_pcm needs an int16 PCM batch");
    if (n_utt < 0 || sample_offsets[0] != 0) fail("bad PCM batch arguments");
    for (int u = 0; u < n_utt; u++)
        if (sample_offsets[u + 1] < sample_offsets[u]) fail("sample_offsets must be non-decreasing");
    const int64_t n = sample_offsets[n_utt];
    if (n > 0 && !pcm) fail("null PCM pointer");
    b->bind_device();
    b->n_utt = n_utt;
    b->offsets.assign(sample_offsets, sample_offsets + n_utt + 1);
    b->n_rows = n;
    b->invalidate_tiles();
    // (device buffers only ever grow.)  A decision's worth of samples and their offsets: page-locked copies, left in flight
    if (((size_t)n_utt + 1) * sizeof(int64_t) <= STAGED_TABLE_MAX_BYTES && stage_small_pcm(b, pcm, n)) {
        b->stage_offsets.send(b->d_offsets, b->offsets.data(), b->offsets.size());
        return 0;
    }
    b->pcm16.upload(pcm, (size_t)n);
    b->d_offsets.upload(b->offsets.data(), b->offsets.size());
    sync_stream();
    return 0;
    SR_CATCH(-1)
}

void sr_batch_free(SRBatch *b) { delete b; }
int sr_batch_num_utterances(SRBatch *b) { return b ? b->n_utt : 0; }
int64_t sr_batch_num_rows(SRBatch *b) { return b ? b->n_rows : 0; }
int sr_batch_dim(SRBatch *b) { return (b && b->kind == SRBatch::FEATURES) ? b->dim : 0; }

int sr_batch_offsets(SRBatch *b, int64_t *offsets_out) {
    SR_TRY
    if (!b || !offsets_out) fail("null argument");
    std::memcpy(offsets_out, b->offsets.data(), sizeof(int64_t) * b->offsets.size());
    return 0;
    SR_CATCH(-1)
}

int sr_batch_download(SRBatch *b, float *out) {
    SR_TRY
    if (!b || !out) fail("null argument");
    if (b->kind != SRBatch::FEATURES) fail("only feature batches can be downloaded");
    b->bind_device();
    b->data.download(out, (size_t)b->n_rows * b->dim);
    sync_stream();
    return 0;
    SR_CATCH(-1)
}

int sr_batch_download_pcm16(SRBatch *b, int16_t *out) {
    SR_TRY
    if (!b || (!out && b->n_rows > 0)) fail("null argument");
    if (b->kind != SRBatch::PCM16) fail("only int16 PCM batches can be downloaded as PCM16");
    b->bind_device();
    b->pcm16.download(out, (size_t)b->n_rows);
    sync_stream();
    return 0;
    SR_CATCH(-1)
}

SRBatch *sr_silence_remove_batch(SRBatch *pcm, double fs, double frame_duration, double frame_shift, double perc, int64_t *kept_out) {
    SR_TRY
    if (!pcm) fail("null argument");
    auto out = std::make_unique<SRBatch>();
    silence_remove_batch(*pcm, fs, frame_duration, frame_shift, perc, *out, kept_out);
    return out.release();
    SR_CATCH(nullptr)
}

int sr_silence_plan(double fs, double frame_duration, double frame_shift, int64_t max_samples, int32_t *out, int n_out) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 12) fail("sr_silence_plan writes 12 fields");
    SilencePlan p;
    std::string why;
    if (!plan_silence(fs, frame_duration, frame_shift, max_samples, silence_block(), p, why)) fail("remove_silence: %s", why.c_str());
    const int64_t v[12] = {p.L, p.S, p.g, p.E, p.B, p.blocks_max, p.variant, p.blocks_per_wg, p.list_cap,
                           silence_grid(p.blocks_max, p.blocks_per_wg), p.chunk_lanes, p.max_pos};
    for (int i = 0; i < 12; i++) out[i] = (int32_t)std::min<int64_t>(v[i], INT32_MAX);
    return 12;
    SR_CATCH(-1)
}

// ---- short-time feature normalisation (featnorm.hip).  Every refusal comes before the device is touched. ----

SRBatch *sr_feature_norm_batch(SRBatch *feats, int mode, int window, int64_t *degenerate_out, int32_t *ranks_out) {
    SR_TRY
    if (!feats) fail("null argument");
    auto out = std::make_unique<SRBatch>();
    feature_norm_batch(*feats, mode, window, *out, degenerate_out, ranks_out);
    return out.release();
    SR_CATCH(nullptr)
}

int sr_feature_norm_plan(int mode, int window, int dim, int64_t max_frames, int n_cu, int32_t *out, int n_out) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 12) fail("sr_feature_norm_plan writes 12 fields");
    FeatNormPlan p;
    std::string why;
    if (n_cu > 0) {
        if (!plan_feature_norm(mode, window, true, dim, max_frames, feature_norm_tile(), n_cu, p, why)) fail("sr_feature_norm_plan: %s", why.c_str());
    } else {
        if (!plan_feature_norm(mode, window, true, dim, max_frames, feature_norm_tile(), 1, p, why)) fail("sr_feature_norm_plan: %s", why.c_str());
        ensure_device();
        if (!plan_feature_norm(mode, window, true, dim, max_frames, feature_norm_tile(), ctx().n_cu, p, why)) fail("sr_feature_norm_plan: %s", why.c_str());
    }
    const int64_t v[12] = {p.F, p.span_max, p.stride, p.cols, p.passes, p.lds_bytes, p.tiles_max, featnorm_grid(p.tiles_max, n_cu > 0 ? n_cu : ctx().n_cu),
                           p.table ? 1 : 0, p.table_len, FEATNORM_WG, FEATNORM_MAX_W};
    for (int i = 0; i < 12; i++) out[i] = (int32_t)std::min<int64_t>(v[i], INT32_MAX);
    return 12;
    SR_CATCH(-1)
}

double sr_norm_quantile(double p) { return norm_quantile(p); }

}  // extern "C"
