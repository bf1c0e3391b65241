// silence.hpp -- energy-threshold silence removal on the device (silence.hip).
#pragma once

#include <cstdint>

struct SRBatch;

namespace sr {

void silence_remove_batch(SRBatch &pcm, double fs, double frame_duration, double frame_shift, double perc, SRBatch &out, int64_t *kept_out);
void set_silence_block(long v);
long silence_block();

}  // namespace sr
