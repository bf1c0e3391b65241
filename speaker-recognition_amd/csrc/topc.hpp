// topc.hpp -- top-C Gaussian selection (gmm_topc.hip).
#pragma once

#include "batch.hpp"
#include "gmm_model.hpp"

namespace sr {

// gmm_topc.hip: top-C Gaussian selection against the background column `bg` (opt-in; the exact path never calls it).  Refusals --
// a set that does not share sigma and weights, bg or top_c out of range, a PCM batch -- come before any device work.
// topc_out [n_frames][top_c] / frame_ll_out [S][n_frames]: host memory or null.
void score_batch_set_topc(SRModelSet &set, SRBatch &feat, int bg, int top_c, double *sums_out, int *argmax_out, int *topc_out,
                          float *frame_ll_out, int flags);
bool topc_set_tied(SRModelSet &set);       // does the set qualify?  (host only; the answer is kept)
void set_topc_scratch_mib(long v);
long topc_scratch_mib();

}  // namespace sr
