// featnorm.hpp -- short-time feature normalisation on the device (featnorm.hip).
#pragma once

#include <cstdint>

struct SRBatch;

namespace sr {

void feature_norm_batch(SRBatch &in, int mode, int window, SRBatch &out, int64_t *degenerate_out, int32_t *ranks_out);
void set_feature_norm_tile(long v);
long feature_norm_tile();

}  // namespace sr
