// bw_stats.hpp -- batched per-session Baum-Welch statistics against a UBM (bw_stats.hip).
#pragma once

#include "batch.hpp"
#include "gmm_model.hpp"

struct SRStats;

namespace sr {

// bw_stats.hip: per-utterance Baum-Welch statistics N [U][K], F [U][K * D] (host memory) of the feature batch against model `model`
// of the set; ll [U] / dropped [U]: host memory or null.  Refusals (bw_plan.cpp: bw_check) come before any device work.
void bw_stats_batch(SRModelSet &set, int model, SRBatch &feat, double *N_out, double *F_out, double *ll_out, int64_t *dropped_out);
// the same passes with N and F left on the device in a statistics handle (jfa.hpp, jfa_dev.hpp)
SRStats *bw_stats_resident(SRModelSet &set, int model, SRBatch &feat, double *ll_out, int64_t *dropped_out);
void set_bw_scratch_mib(long v);
long bw_scratch_mib();
void set_bw_range_frames(long v);
long bw_range_frames();

}  // namespace sr
