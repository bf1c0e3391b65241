// abi_timeline.cpp -- who spoke when (timeline.hip): the decision on given window sums, the whole pass on a feature batch against a
// diagonal or a full-covariance set, and from resident PCM.  Every argument is checked before the device is touched.
#include "abi_internal.hpp"

#include "gmm_full.hpp"
#include "mfcc.hpp"
#include "score.hpp"
#include "timeline.hpp"
#include "timeline_plan.hpp"

#include <algorithm>
#include <string>

using namespace sr;

namespace {

TimelineRule checked_rule(const char *what, int S, int bg, double threshold, int mode, double beta, int min_dur) {
    std::string why;
    if (!timeline_check(S, bg, threshold, mode, beta, min_dur, why)) fail("%s: %s", what, why.c_str());
    return TimelineRule{bg, threshold, mode, beta, min_dur};
}

void check_windowing(const char *what, int window, int hop) {
    if (window < 1) fail("%s: the window must hold at least 1 frame, got %d", what, window);
    if (hop < 1) fail("%s: the hop must be at least 1 frame, got %d", what, hop);
}

// The call keeps the matrix sr_score_batch_set(frame_ll_out) would return on the device: S x n_frames floats.  A recording that
// cannot fit is refused with the byte count (chunking it is the caller's: the windows of two chunks overlap by W - H frames).
void check_frame_matrix_fits(const char *what, int S, int64_t n_rows) {
    size_t free_b = 0, total_b = 0;
    SR_HIP(hipMemGetInfo(&free_b, &total_b));
    const double need = (double)S * (double)n_rows * sizeof(float);
    if (need > (double)total_b)
        fail("%s: the per-frame matrix needs %.0f bytes (%d columns x %lld frames x 4), the device has %zu: split the recording", what, need, S,
             (long long)n_rows, total_b);
}

}  // namespace

extern "C" {

int64_t sr_timeline_windows(int64_t n_frames, int64_t window, int64_t hop) { return timeline_windows(n_frames, window, hop); }

int sr_timeline_plan(int S, int min_dur, int64_t n_frames, int window, int hop, int32_t *out, int n_out) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 16) fail("sr_timeline_plan writes 16 fields");
    TimelinePlan p;
    std::string why;
    if (!plan_timeline(S, min_dur, n_frames, window, hop, p, why)) fail("sr_timeline_plan: %s", why.c_str());
    const int64_t v[16] = {p.windows, p.variant, p.lanes, p.states_per_lane, p.tile, p.chain_slots, p.chain_lds ? 1 : 0, p.fwd_lds_bytes,
                           p.sum_span, TIMELINE_SUM_CHUNK, p.sum_lds_bytes, p.sum_grid_x, p.sum_grid_y, p.bp_bytes_per_window,
                           TIMELINE_MAX_S, TIMELINE_MAX_M};
    for (int i = 0; i < 16; i++) out[i] = (int32_t)std::min<int64_t>(v[i], INT32_MAX);
    return 16;
    SR_CATCH(-1)
}

int sr_timeline_decide(const double *sums, const int32_t *counts, const int64_t *win_off, int U, int S, int bg, double threshold, int mode,
                       double beta, int min_dur, int *label_out, double *path_score_out, int64_t *bad_windows_out) {
    SR_TRY
    if (U < 0) fail("sr_timeline_decide: %d recordings", U);
    const TimelineRule rule = checked_rule("sr_timeline_decide", S, bg, threshold, mode, beta, min_dur);
    if (!win_off) fail("sr_timeline_decide: null argument (the window offsets)");
    if (win_off[0] != 0) fail("sr_timeline_decide: the window offsets start at %lld, not 0", (long long)win_off[0]);
    for (int u = 0; u < U; u++)
        if (win_off[u + 1] < win_off[u]) fail("sr_timeline_decide: recording %d has a negative window count", u);
    const int64_t nw_total = win_off[U];
    if (nw_total > INT32_MAX / 2) fail("sr_timeline_decide: %lld windows in one call (at most 2^30: split the batch)", (long long)nw_total);
    if (nw_total > 0 && (!sums || !counts || !label_out)) fail("sr_timeline_decide: null argument");
    for (int64_t j = 0; j < nw_total; j++)
        if (counts[j] < 1) fail("sr_timeline_decide: window %lld holds %d frames (a window holds at least one)", (long long)j, counts[j]);
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_timeline_decide");
    timeline_decide_host(sums, counts, win_off, U, S, rule, label_out, path_score_out, bad_windows_out);
    return 0;
    SR_CATCH(-1)
}

int sr_timeline_batch(SRModelSet *set, SRBatch *features, int window, int hop, int bg, double threshold, int mode, double beta, int min_dur,
                      int flags, int64_t *win_off_out, int *label_out, double *sums_out, double *path_score_out, int64_t *bad_windows_out) {
    SR_TRY
    if (!set || !features) fail("sr_timeline_batch: null argument");
    if (!win_off_out) fail("sr_timeline_batch: null output (the window offsets are required)");
    if (features->kind != SRBatch::FEATURES) fail("sr_timeline_batch takes a feature batch; sr_timeline_pcm_batch takes PCM");
    check_windowing("sr_timeline_batch", window, hop);
    const int S = set->host.n_models;
    const TimelineRule rule = checked_rule("sr_timeline_batch", S, bg, threshold, mode, beta, min_dur);
    if (!label_out && features->n_rows > 0) fail("sr_timeline_batch: null output (the labels are required)");
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_timeline_batch");
    // the matrix sr_score_batch_set(frame_ll_out) returns: a saturated pass redone on the precise engines, the partial-product
    // pairs patched on the device (a fetch that asks for no host results takes gmm_flush.hip's device patch)
    ensure_device();
    check_frame_matrix_fits("sr_timeline_batch", S, features->n_rows);
    const ScoreResult r = score_resolved(*set, *features, true, flags, 0, nullptr, nullptr, nullptr);
    timeline_from_frames(r.d_frame_ll, *features, S, window, hop, rule, win_off_out, label_out, sums_out, path_score_out, bad_windows_out);
    return 0;
    SR_CATCH(-1)
}

int sr_fullset_timeline_batch(SRFullSet *set, SRBatch *features, int window, int hop, double threshold, int mode, double beta, int min_dur,
                              int64_t *win_off_out, int *label_out, double *sums_out, double *path_score_out, int64_t *bad_windows_out) {
    SR_TRY
    if (!set || !features) fail("sr_fullset_timeline_batch: null argument");
    if (!win_off_out) fail("sr_fullset_timeline_batch: null output (the window offsets are required)");
    if (features->kind != SRBatch::FEATURES) fail("sr_fullset_timeline_batch takes a feature batch");
    check_windowing("sr_fullset_timeline_batch", window, hop);
    const TimelineRule rule = checked_rule("sr_fullset_timeline_batch", set->S, -1, threshold, mode, beta, min_dur);
    if (!label_out && features->n_rows > 0) fail("sr_fullset_timeline_batch: null output (the labels are required)");
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_fullset_timeline_batch");
    ensure_device();
    check_frame_matrix_fits("sr_fullset_timeline_batch", set->S, features->n_rows);
    fullset_score_device(*set, *features);
    timeline_from_frames(set->fll.p, *features, set->S, window, hop, rule, win_off_out, label_out, sums_out, path_score_out, bad_windows_out);
    return 0;
    SR_CATCH(-1)
}

int sr_timeline_pcm_batch(SRMfcc *m, SRModelSet *set, SRBatch *pcm, int nd, int window, int hop, int bg, double threshold, int mode,
                          double beta, int min_dur, int flags, int64_t *win_off_out, int *label_out, double *sums_out, double *path_score_out,
                          int64_t *bad_windows_out) {
    SR_TRY
    if (!m || !set || !pcm) fail("sr_timeline_pcm_batch: null argument");
    if (!win_off_out || !label_out) fail("sr_timeline_pcm_batch: null output (the window offsets and the labels are required)");
    if (pcm->kind == SRBatch::FEATURES) fail("sr_timeline_pcm_batch takes a PCM batch; sr_timeline_batch takes features");
    check_windowing("sr_timeline_pcm_batch", window, hop);
    const int S = set->host.n_models;
    const TimelineRule rule = checked_rule("sr_timeline_pcm_batch", S, bg, threshold, mode, beta, min_dur);
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_timeline_pcm_batch");
    ensure_device();
    SRBatch *feat_ws = &per_device<SRBatch>();   // the fused calls' feature workspace: nothing leaves the device
    mfcc_extract_batch(*m, *pcm, nd, 1, *feat_ws);
    check_frame_matrix_fits("sr_timeline_pcm_batch", S, feat_ws->n_rows);
    const ScoreResult r = score_resolved(*set, *feat_ws, true, flags, 0, nullptr, nullptr, nullptr);
    timeline_from_frames(r.d_frame_ll, *feat_ws, S, window, hop, rule, win_off_out, label_out, sums_out, path_score_out, bad_windows_out);
    return 0;
    SR_CATCH(-1)
}

}  // extern "C"
