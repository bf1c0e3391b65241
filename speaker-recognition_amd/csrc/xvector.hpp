// xvector.hpp -- the x-vector network (C ABI handle `SRXvector *`) and its forward pass (xvector.hip).
#pragma once

#include "batch.hpp"
#include "common.hpp"
#include "xvector_plan.hpp"

#include <vector>

struct SRXvector {
    std::vector<sr::XvLayer> layers;
    sr::XvModelInfo info;
    // host images, made once when the network is created: weights rounded to bf16 (round to nearest even) in the padded
    // [n_pad][k_pad] layout the layer kernel reads, bias / scale / shift padded to n_pad (scale 1, shift 0 where none was given;
    // all three 0 in the padding)
    std::vector<std::vector<uint16_t>> h_w;
    std::vector<std::vector<float>> h_b, h_scale, h_shift;
    // resident copies, uploaded by the first forward pass on the device that runs it
    int device = -1;
    std::vector<sr::DevBuf<uint16_t>> d_w;
    std::vector<sr::DevBuf<float>> d_b, d_scale, d_shift;
};

namespace sr {

long xvector_scratch_mib();
void set_xvector_scratch_mib(long mib);
// 0: v_mfma_f32_32x32x16_bf16 (the default), 1: v_mfma_f32_16x16x32_bf16 -- the timing hook debug_xvector_mfma_shape, kept for timing one against the other
int xvector_mfma_shape();
void set_xvector_mfma_shape(int shape);

// bf16 bits of an fp32 value, round to nearest even (NaN stays a quiet NaN); the device's stores round the same way
uint16_t xv_bf16_rne(float v);

// Builds the host images; refuses non-finite weights.  W[l]: [c_out][n_off * c_in] offset-major; b / scale / shift: [c_out];
// scale and shift null together or given together; every pointer of a pooling layer is ignored.
SRXvector *xvector_create(const XvLayer *layers, int n_layers, const float *const *W, const float *const *b, const float *const *scale,
                          const float *const *shift);

// The forward pass over segments (utterance, first frame, frames) of a resident feature batch, as `plan` (plan_xvector over those
// segments' frame counts, made and checked by the caller before the device is touched) lays it out.  `out`: host fp32
// [plan.out_rows][plan.out_cols] (the embeddings, or the tapped layer's output); `times_ms`: null or [n_layers + 1], the device time
// of the converts [0] and of every layer [1 + l], summed over the chunks.
void xvector_forward(SRXvector &net, SRBatch &feat, const int32_t *segs, const XvPlan &plan, bool tap_bf16, float *out, double *times_ms);

}  // namespace sr
