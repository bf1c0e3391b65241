// score_shapes.hpp -- what the scoring kernels' workgroup shapes can hold, as constexpr functions of integers: the kernel
// files use them in __launch_bounds__ / `if constexpr`, the dispatcher (score_plan.cpp) calls them on the host.  Plain
// C++17: no HIP header, so that the plan builds with any host compiler (tests/host/host_checks.cpp).
#pragma once

#include <initializer_list>

#if defined(__HIPCC__)
#define SR_HD __host__ __device__
#else
#define SR_HD
#endif

namespace sr {

// ---- gmm_score_h2_shared.hip ----
// Workgroup shapes: waves per workgroup x 32-frame column tiles per wave x images per LDS stage.
//   <4,1>   three workgroups per CU, each with its own copy of the stream (small batches)
//   <12,1>  one workgroup per CU, three waves per SIMD sharing one copy
// Tried and measured slower than <4,1> (profiles/r02_h2s_stalls.txt; the code is in commits 401bc2d and f5a34fe):
// two column tiles per wave (COLS = 2: half the LDS fragment reads, 2 waves per SIMD) -4 %; 8 waves x 2 column
// tiles -5 %; 8 waves with the two waves of a SIMD held in anti-phase by a workgroup barrier per phase (one
// chains while the other runs its epilogue) -3 % with one image per phase, -5 % with two.
SR_HD constexpr int h2s_waves_per_eu(int kqf, int klf, int cols, int waves, bool ms = false) {
    // The 4-wave shape at three workgroups per CU (168 registers) kept its quadratic-half frame fragments in scratch from
    // kqf + klf = 10 up (156 .. 364 bytes per lane, one reload inside the image loop = an s_waitcnt vmcnt(0) on the LDS-DMA
    // stream).  Since round 4 it only serves batches below ~2000 frames (plan_score: everything larger takes a 12-wave
    // shape) -- a handful of workgroups, latency-bound, where a third workgroup per CU buys nothing: two per CU, 256 registers,
    // nothing in scratch.
    // (the model-split shape carries a few registers more: at three workgroups per CU its 3 + 3 and 4 + 4 forms spilled 24 / 52 bytes)
    // (since the 4-wave shapes stream four images per stage their LDS admits two workgroups per CU at most, and their batches --
    // below ~2000 frames -- never need more: two per CU for every chain length; the third one's 168-register budget was
    // what spilled, last in <4,4> once the exception lists became per block)
    (void)kqf; (void)klf; (void)cols; (void)ms;
    return waves > 4 ? waves / 4 : 2;
}
constexpr int H2M_MAX_KLF = 9;        // two register sets of fragments fit up to here (D <= 45); the longest chains keep the LDS form
// LDS the pipelined kernel takes: its ring of two stages of four images plus the 12 waves' quadratic-half fragments
SR_HD constexpr bool h2p_fits(int kqf, int klf) { return klf >= 2 && kqf <= klf && (2 * 4 * klf + 12 * kqf) * 1024 <= 160 * 1024; }
// workgroups resident per CU, and 32-frame tiles per workgroup, of shape `shape` (0: 4 waves; 1: 12 waves; 2: 12 waves, pipelined;
// 3: 4 waves on one tile, the block's models split between them)
constexpr int h2s_resident_per_cu(int kqf, int klf, int shape) { return (shape == 0 || shape == 3) ? h2s_waves_per_eu(kqf, klf, 1, 4, shape == 3) : 1; }
constexpr int h2s_tiles_per_wg(int shape) { return shape == 0 ? 4 : shape == 3 ? 1 : 12; }
// shape 3 runs as gmm_score_h2m_kernel (images straight into registers) for these chain lengths
constexpr bool h2s_msplit_direct(int klf) { return klf <= H2M_MAX_KLF; }

// ---- gmm_score_split.hip ----
constexpr int split_max_ft(int ks) { return ks <= 6 ? 2 : 1; }

// ---- gmm_score_splitp.hip ----
// Workgroup shapes: 16 or 12 waves = one workgroup per CU (one copy of the stream for all of them); 8 waves = two per CU: twice the
// stream, but one workgroup's frame prologue (~500 vector instructions per wave, no MFMA) runs under the other's chains -- what short
// streams want (one 256-mixture model: 8 chunks per prologue).
// chunks per LDS stage: an even count (the two accumulators alternate statically), three stages within the workgroup's share of LDS
SR_HD constexpr int splitp_stage_chunks(int ks, int parts, int waves) { return waves > 8 && ks * parts <= 10 ? 4 : 2; }
SR_HD constexpr int splitp_lds_bytes(int ks, int parts, int waves) {
    return 3 * splitp_stage_chunks(ks, parts, waves) * ks * parts * 1024 + waves * 16 * 33 * 4;
}
SR_HD constexpr bool splitp_fits(int ks, int parts, int waves) {
    // 4 waves per SIMD (16 waves, or two workgroups of 8) leave 128 registers: resident frame fragments of up to 10 x 4 beside the
    // two accumulators (ks * parts = 12: 12 bytes of scratch, 14: 64, 16: 116 -- build/gmm_score_splitp.resources); 12 waves have 168
    if (waves != 12 && ks * parts > 10) return false;
    return splitp_lds_bytes(ks, parts, waves) <= (160 * 1024 - 512) / (waves > 8 ? 1 : 2);
}
// workgroups of that shape a CU holds
constexpr int splitp_resident_per_cu(int waves) { return waves > 8 ? 1 : 2; }
// 32-frame tiles a workgroup of the wide shape takes (= its waves): the variant that exists for this layout of the two-part fp16
// scheme (`want` = 0, 8, 12 or 16), 0 = none
inline int splitp_waves_f16x2(int ks, int want) {
    // (instantiated for the two-part fp16 scheme: what the dispatcher takes for every well-conditioned set; the bf16x3 fallback
    // keeps the 4-wave kernel -- 28 more variants of this file cost a minute and a half of build time)
    const int parts = 2;
    if (ks < 2 || ks > 8) return 0;
    for (int w : {want, 16, 12, 8})
        if ((w == 16 || w == 12 || w == 8) && splitp_fits(ks, parts, w)) return w;
    return 0;
}

}  // namespace sr
