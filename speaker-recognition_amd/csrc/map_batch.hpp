// map_batch.hpp -- a set of speakers MAP-adapted from one UBM in one batched device fit (map_batch.hip).
#pragma once

#include "gmm_model.hpp"

#include <cstdint>
#include <string>
#include <vector>

struct Parameter;

namespace sr {

int map_fit_batch(GMM *const *models, int S, const GMM *ubm, const float *X, const int64_t *row_offsets, int dim, const Parameter &param,
                  long seed, int *iterations_out, int *status, std::vector<std::string> &messages);
void map_fit_batch_stats(long *calls, long *speakers_batched, long *speakers_single, long *speakers_handed_over, long *passes);
void set_map_fit_batch_bytes(long v);
long map_fit_batch_bytes();

}  // namespace sr
