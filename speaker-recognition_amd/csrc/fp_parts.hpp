// fp_parts.hpp -- fp32 <-> fp16 / bf16 on the host and the part splits of the matrix-core layouts (model_pack.hpp): the packers must
// produce exactly what the device conversions would.  Plain C++17: no HIP header.
#pragma once

#include <cstdint>

namespace sr {

void split_bf16x3(float v, uint16_t out[3]);   // round-to-nearest-even hi/mid/lo parts
void split_f16x2(float v, uint16_t out[2]);    // round-to-nearest-even hi/lo fp16 parts (gradual underflow)
uint16_t f32_to_f16_rne(float v);
float f16_to_f32(uint16_t h);

}  // namespace sr
