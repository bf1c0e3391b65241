// timeline.hpp -- who spoke when, on the device (timeline.hip): sliding-window sums of a per-frame matrix, the per-window
// decision, the hold rule, the Viterbi decode.
#pragma once

#include <cstdint>

struct SRBatch;

namespace sr {

struct TimelineRule {
    int bg;                // the column that plays "nobody" (label -1), or -1: every column is a speaker
    double threshold;      // added to the nobody state's emission
    int mode;              // 0 raw, 1 hold, 2 viterbi
    double beta;           // viterbi: the price of a label change
    int min_dur;           // viterbi: windows a run holds at least (all but the last)
};

// Sums in host memory [Nw_total][S] with their frame counts and the recordings' window offsets [U + 1]: upload, the decision
// kernels, one copy back.  label_out [Nw_total]; path_out [U] and bad_out [U] may be null.
void timeline_decide_host(const double *sums, const int32_t *counts, const int64_t *win_off, int U, int S, const TimelineRule &rule,
                          int *label_out, double *path_out, int64_t *bad_out);

// The per-frame matrix d_fll [S][feat.n_rows] on the device (a scoring pass's, of the batch `feat`): window sums, then the
// decision.  win_off_out [U + 1]; label_out [Nw_total]; sums_out [Nw_total][S], path_out [U], bad_out [U] may be null.
void timeline_from_frames(const float *d_fll, SRBatch &feat, int S, int window, int hop, const TimelineRule &rule, int64_t *win_off_out,
                          int *label_out, double *sums_out, double *path_out, int64_t *bad_out);

}  // namespace sr
