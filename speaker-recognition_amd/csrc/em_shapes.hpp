// em_shapes.hpp -- what the statistics kernels of the iteration-at-a-time trainer (em.hip) are built for, as constants and
// constexpr functions of integers: the kernels use them in __launch_bounds__ and for their LDS, the plan (em_plan.cpp) calls them
// on the host.  The three lists of built instantiations stand here ONCE: em.hip's dispatch switches and the *_available predicates
// are both generated from them.  Plain C++17: no HIP header, so that the plan builds with any host compiler (tests/host/em_checks.cpp).
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define SR_HD __host__ __device__
#else
#define SR_HD
#endif

namespace sr {

// (gmm_model.hpp's KB, CB and MAX_REG_DIM again -- that header needs HIP; em.hip asserts them equal)
constexpr int EM_KB = 4, EM_CB = 8, EM_MAX_REG_DIM = 96;
constexpr int EM_LDS_BOUND = 160 * 1024;        // what a workgroup may take of a CU's LDS

// ---- em_stats_kernel<DP> / em_stats_wide_kernel: a workgroup = 256 frames (lane = frame), records cut along gridDim.y ----
constexpr int EMV_FT = 256;
constexpr int EMW_JB = 8;                      // mixtures a thread of the wide kernel's phase B sweeps at a time

// ---- em_stats_mfma_kernel<DP>: 4 waves on one tile at a time and 64 mixtures (16 per wave) ----
constexpr int EMM_WAVES = 4, EMM_MB = 16, EMM_WG_MIX = EMM_WAVES * EMM_MB;
constexpr int EMM_F = 2;                       // frames per lane in the responsibility phase: a parameter read serves both
constexpr int EMM_FT = 64 * EMM_F;             // frames per tile
// Row strides = 2 mod 32.  The operand reads are ds_read_b32: two 32-lane groups, bank = dword address mod 32; a group holds
// (mixture or column j = 0..15) x (frame fl = 0..1 or 2..3) at j * stride + fl + const, i.e. banks 2 j + fl: all different.
// (Stride 4 mod 64 -- the ds_read_b64 / b128 bank map -- made j and j + 8 collide: SQ_LDS_BANK_CONFLICT 55 % of the LDS cycles.)
constexpr int EMM_XS = EMM_FT + 2, EMM_GS = EMM_FT + 2;
// 16-column blocks of a mixture's 2 DP + 1 sums: [x, 16 per block][x^2, 16 per block][the rest of x, of x^2, the count]
SR_HD constexpr int emm_ncb(int dp) { return 2 * (dp / 16) + (2 * (dp % 16) + 1 + 15) / 16; }
// dynamic LDS of em_stats_mfma_kernel<DP>: 16 parameter records (of 2 DP + 1 float4), one transposed tile of rows, four waves'
// responsibilities
SR_HD constexpr size_t emm_lds_bytes(int DP) {
    return (size_t)(EMM_WG_MIX / EM_KB) * (2 * DP + 1) * 16 + (size_t)DP * EMM_XS * sizeof(float) +
           (size_t)EMM_WAVES * EMM_MB * EMM_GS * sizeof(float);
}

// ---- em_stats_split_kernel<DP, KS>: 8 waves, 128 mixtures = 4 tiles of the split-bf16 layout, KS contraction steps ----
constexpr int EMS_WAVES = 8, EMS_WG_MIX = EMS_WAVES * EMM_MB;
constexpr int EMS_TILES = 4;                   // 32-mixture tiles of that layout per workgroup
SR_HD constexpr int ems_lds_bytes(int ks) {
    return 4 * ks * 3 * 64 * 16 + 8 * ks * EMM_XS * 4 + EMS_WG_MIX * EMM_GS * 4;
}
// contraction steps of the split-bf16 layout at `dim` dimensions (8 slots a step, one of them the constant's)
SR_HD constexpr int ems_steps(int dim) { return (dim + 8) / 8; }

// ---- the built instantiations ----
// the vector-ALU form: every padded dim pick_padded_dim hands out up to MAX_REG_DIM (wider rows: em_stats_wide_kernel, any width)
#define SR_EM_VECTOR_DPS(X) X(8) X(13) X(16) X(24) X(26) X(32) X(34) X(39) X(40) X(48) X(56) X(64) X(80) X(96)
// the fp64 matrix-core form: padded dims <= 40 (its LDS -- 16 parameter records, a transposed 128-frame tile, the
// responsibilities: 75 KiB at DP = 39 -- lets two workgroups share a CU); wider rows keep em_stats_kernel
#define SR_EM_MFMA_DPS(X) X(8) X(13) X(16) X(24) X(26) X(32) X(34) X(39) X(40)
// the split-responsibility form: the (padded dim, contraction steps) pairs whose LDS fits a CU (DP = 40 is dim = 40: six steps,
// 164 KB -- not available)
#define SR_EM_SPLIT_SHAPES(X) X(8, 1) X(8, 2) X(13, 2) X(16, 2) X(16, 3) X(24, 3) X(24, 4) X(26, 4) X(32, 4) X(32, 5) X(34, 5) X(39, 5)

#define SR_EM_IS1(V) if (DP == V) return true;
#define SR_EM_IS2(V, W) if (DP == V && KS == W) return true;
SR_HD constexpr bool stats_vector_available(int DP) { SR_EM_VECTOR_DPS(SR_EM_IS1) return false; }
SR_HD constexpr bool stats_mfma_available(int DP) { SR_EM_MFMA_DPS(SR_EM_IS1) return false; }
SR_HD constexpr bool stats_split_available(int DP, int KS) { SR_EM_SPLIT_SHAPES(SR_EM_IS2) return false; }
#undef SR_EM_IS1
#undef SR_EM_IS2

#define SR_EM_FITS1(V) static_assert(emm_lds_bytes(V) <= (size_t)EM_LDS_BOUND, "em_stats_mfma_kernel's LDS fits a CU");
#define SR_EM_FITS2(V, W) \
    static_assert(8 * W >= V && ems_lds_bytes(W) <= EM_LDS_BOUND && stats_mfma_available(V), "the transposed tile has a row per slot feature and fits a CU");
SR_EM_MFMA_DPS(SR_EM_FITS1)
SR_EM_SPLIT_SHAPES(SR_EM_FITS2)
#undef SR_EM_FITS1
#undef SR_EM_FITS2

// float64 slab elements of the matrix-core forms: per (frame chunk, mixture range) wg_mix mixtures x the blocked columns
SR_HD constexpr size_t stats_mfma_slab_doubles(int DP, int n_ranges, int n_chunks, int wg_mix = EMM_WG_MIX) {
    return (size_t)n_chunks * n_ranges * wg_mix * (size_t)(emm_ncb(DP) * 16);
}

}  // namespace sr
