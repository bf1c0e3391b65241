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

// The COMPACT image and contraction order of the pipelined kernel.  The flat order [lo(A) hi(z) | hi(A) lo(z) | hi(A) hi(z)] stores
// hi(A) twice and keeps hi(z) twice in every wave's resident fragments.  A part (D dimensions + the constant) is h = ceil((D + 1) / 8)
// half-steps of 8 slots -- the 8 slots one half-wave holds of a 16-slot MFMA step -- so the duplicates can be lined up with whole
// fragments and dropped: H_p / L_p = half-step p of hi(A) / lo(A) (the constant's parts in the last slot of the last half-step of the
// linear half), zh_p / zl_p the same of the frame side (the constant 1 in zh; a 0 in zl where it would meet hi(C)).
//   even h:  A fragments (H0,H1) .. | (L0,L1) ..;  B registers (zl0,zl1) .. | (zh0,zh1) ..
//            chain  H x zl | H x zh (the H fragments again) | L x zh (the zh registers again)
//   odd h:   A fragments (H0,H1) .. (H_{h-1},H_{h-1}) | (L0,L1) .. (L_{h-1},0);  B registers (zl pairs) | (zh pairs) | (zl_{h-1},zh_{h-1}) | (zh_{h-1},0)
//            chain  H pairs x zl pairs | H pairs x zh pairs | (H,H)_{h-1} x (zl,zh)_{h-1} | L pairs x zh pairs | (L_{h-1},0) x (zh_{h-1},0)
// The same multiset of products in ceil(3h / 2) steps -- never fewer than the flat order's KLF = ceil((3D + 2) / 16), so the form
// applies where the two are equal (3h <= 2 KLF: D = 37 .. 39 of the <8,8> chains, not D = 40 .. 42) -- with h or h + 1 stored
// fragments and as many B registers instead of KLF of each.  A half is part * 16 + p (A: part 0 = hi, 1 = lo; B: 0 = low part of z,
// 1 = high part), -1 = zeros.
constexpr int H2C_MAX_STEPS = 16;
struct H2cMap {
    int h = 0, nk = 0, nf = 0, nb = 0;                     // half-steps per part, chain steps, stored fragments, B registers
    int a_of[H2C_MAX_STEPS] = {}, b_of[H2C_MAX_STEPS] = {};         // step -> stored fragment / B register
    int a_last[H2C_MAX_STEPS] = {}, b_last[H2C_MAX_STEPS] = {};     // stored fragment / B register -> the step that uses it last
    int a_half[H2C_MAX_STEPS][2] = {}, b_half[H2C_MAX_STEPS][2] = {};
};
SR_HD constexpr int h2c_half_steps(int dim) { return (dim + 1 + 7) / 8; }
SR_HD constexpr int h2c_steps(int h) { return (3 * h + 1) / 2; }
SR_HD constexpr bool h2c_applies(int dim, int klf) { return dim >= 1 && h2c_steps(h2c_half_steps(dim)) == klf && klf <= H2C_MAX_STEPS; }
SR_HD constexpr H2cMap h2c_map(int h) {
    H2cMap m;
    m.h = h;
    m.nk = h2c_steps(h);
    const int np = h / 2, odd = h & 1;                     // whole pairs of half-steps; a single one left over
    const int nh = np + odd;                               // fragments of hi(A), and of lo(A)
    m.nf = 2 * nh;
    m.nb = 2 * nh;
    for (int i = 0; i < np; i++) {
        m.a_half[i][0] = 2 * i;                 m.a_half[i][1] = 2 * i + 1;                 // (H_2i, H_2i+1)
        m.a_half[nh + i][0] = 16 + 2 * i;       m.a_half[nh + i][1] = 16 + 2 * i + 1;       // (L_2i, L_2i+1)
        m.b_half[i][0] = 2 * i;                 m.b_half[i][1] = 2 * i + 1;                 // (zl_2i, zl_2i+1)
        m.b_half[np + i][0] = 16 + 2 * i;       m.b_half[np + i][1] = 16 + 2 * i + 1;       // (zh_2i, zh_2i+1)
    }
    if (odd) {
        m.a_half[np][0] = h - 1;                m.a_half[np][1] = h - 1;                    // (H_{h-1}, H_{h-1})
        m.a_half[nh + np][0] = 16 + h - 1;      m.a_half[nh + np][1] = -1;                  // (L_{h-1}, 0)
        m.b_half[2 * np][0] = h - 1;            m.b_half[2 * np][1] = 16 + h - 1;           // (zl_{h-1}, zh_{h-1})
        m.b_half[2 * np + 1][0] = 16 + h - 1;   m.b_half[2 * np + 1][1] = -1;               // (zh_{h-1}, 0)
    }
    int k = 0;
    for (int i = 0; i < np; i++, k++) { m.a_of[k] = i;      m.b_of[k] = i; }                // H pairs x zl pairs
    for (int i = 0; i < np; i++, k++) { m.a_of[k] = i;      m.b_of[k] = np + i; }           // H pairs x zh pairs
    if (odd) { m.a_of[k] = np; m.b_of[k] = 2 * np; k++; }                                  // (H,H) x (zl,zh)
    for (int i = 0; i < np; i++, k++) { m.a_of[k] = nh + i; m.b_of[k] = np + i; }           // L pairs x zh pairs
    if (odd) { m.a_of[k] = nh + np; m.b_of[k] = 2 * np + 1; k++; }                         // (L,0) x (zh,0)
    for (int s = 0; s < m.nk; s++) {
        m.a_last[m.a_of[s]] = s;
        m.b_last[m.b_of[s]] = s;
    }
    return m;
}
// The pipelined kernel reads fragment f of the NEXT image into its register in the step that uses f of this image last; LDS returns
// in order, so the wait in front of step u's MFMA names how many of the wave's own fragment reads were issued after the one that
// filled a_of[u]: the rest of the previous image's, then this image's so far.
SR_HD constexpr int h2c_younger(const H2cMap &m, int u) {
    const int lu = m.a_last[m.a_of[u]];
    int n = 0;
    for (int f = 0; f < m.nf; f++) n += (m.a_last[f] > lu) + (m.a_last[f] < u);
    return n;
}
// What the kernel relies on: every step's operands exist, every stored fragment and B register is used, the fragments' last uses
// come in fragment order (the block's first image is read F0, F1, .. in front of the loop: the same order), and no wait count
// leaves lgkmcnt's four bits.
SR_HD constexpr bool h2c_map_ok(const H2cMap &m) {
    if (m.nk > H2C_MAX_STEPS || m.nf > m.nk || m.nb > m.nk || m.nk != h2c_steps(m.h)) return false;
    for (int f = 0; f < m.nf; f++) {
        bool used = false;
        for (int s = 0; s < m.nk; s++) used = used || m.a_of[s] == f;
        if (!used || (f > 0 && m.a_last[f] <= m.a_last[f - 1])) return false;
    }
    for (int r = 0; r < m.nb; r++) {
        bool used = false;
        for (int s = 0; s < m.nk; s++) used = used || m.b_of[s] == r;
        if (!used) return false;
    }
    for (int s = 0; s < m.nk; s++)
        if (m.a_of[s] < 0 || m.a_of[s] >= m.nf || m.b_of[s] < 0 || m.b_of[s] >= m.nb || h2c_younger(m, s) > 15) return false;
    return true;
}
// the one chain length the compact kernel is built for (KQF = KLF = 8 steps, h = 5: D = 37 .. 39 -- BASELINE configs[2] / [3])
constexpr int H2C_KLF = 8, H2C_H = 5;
constexpr H2cMap H2C_MAP = h2c_map(H2C_H);
static_assert(h2c_map_ok(h2c_map(H2C_H)) && h2c_map(H2C_H).nk == H2C_KLF && h2c_map(H2C_H).nf == 6 && h2c_map(H2C_H).nb == 6, "the compact order of the <8,8> chains");
static_assert(h2c_map_ok(h2c_map(4)) && h2c_map_ok(h2c_map(3)) && h2c_map_ok(h2c_map(6)) && h2c_map_ok(h2c_map(1)), "even and odd part lengths");
SR_HD constexpr bool h2c_built(int dim, int klf) { return klf == H2C_KLF && h2c_applies(dim, klf) && h2c_half_steps(dim) == H2C_H; }
// LDS of the compact form: a ring of two stages of four images of nf fragments plus the 12 waves' nb quadratic-half fragments
SR_HD constexpr int h2c_lds_bytes(int h) { return (2 * 4 * h2c_map(h).nf + 12 * h2c_map(h).nb) * 1024; }
static_assert(h2c_lds_bytes(H2C_H) <= 160 * 1024 && (4 * h2c_map(H2C_H).nf) % 12 == 0, "the compact ring fits a CU; a stage is a whole number of pieces per wave");

// PAIRS of blocks in the compact pipelined kernel: the quadratic half Q is the same for every model of the set, so a workgroup runs
// two consecutive blocks of its group behind ONE Q image -- per mixture tile [Q][L_0 .. L_(sb-1)][L'_0 .. L'_(m2-1)], the second
// block's images taken from ITS stream from image 1 on (its own Q image is never read) -- in stages of g images.  `m1` / `m2` =
// models of the first / second block; m2 = 0 is a lone block (the odd one at a group's end), which runs as it always did.  A pair
// needs a full first block (m1 == sb): every block but a set's last one is.
constexpr int H2Q_SB = 15, H2Q_G = 4;                        // SHARED_SB and the pipelined kernel's images per stage
SR_HD constexpr bool h2q_pairs(int sb, int m1, int m2) { return m2 > 0 && m1 == sb; }
// stages per mixture tile that hold a model (stages of phantom models only are skipped, counted over the pair)
SR_HD constexpr int h2q_stages(int g, int m1, int m2) { return (1 + m1 + m2 + g - 1) / g; }
// images executed per mixture tile: whole stages, but never the slot behind a full pair's last image (1 + 2 sb is one short of a stage)
SR_HD constexpr int h2q_images(int sb, int g, int m1, int m2) {
    return h2q_stages(g, m1, m2) * g < 1 + 2 * sb ? h2q_stages(g, m1, m2) * g : 1 + 2 * sb;
}
// the last executed image of a mixture tile (its epilogue rides on the next tile's Q image) and the accumulator it lies in
SR_HD constexpr int h2q_last_image(int sb, int g, int m1, int m2) { return h2q_images(sb, g, m1, m2) - 1; }
SR_HD constexpr int h2q_last_parity(int sb, int g, int m1, int m2) { return h2q_last_image(sb, g, m1, m2) & 1; }
// ... as a model of the pair: 0 .. sb - 1 the first block's, sb .. 2 sb - 1 the second's (image i holds model i - 1)
SR_HD constexpr int h2q_last_model(int sb, int g, int m1, int m2) { return h2q_last_image(sb, g, m1, m2) - 1; }
// where stage s of a pair comes from: which block's stream (0 / 1), and the first of its g images within that block's mixture tile.
// The second block's last stage ends one image behind its tile -- image 0 of the next tile, or, at the last tile of a set's last
// block, one image past the end: the DEVICE buffer carries one image of padding (the image is loaded, never executed).
SR_HD constexpr int h2q_stage_block(int sb, int g, int s) { return s * g < 1 + sb ? 0 : 1; }
SR_HD constexpr int h2q_stage_image(int sb, int g, int s) { return s * g < 1 + sb ? s * g : s * g - sb; }
static_assert((1 + H2Q_SB) % H2Q_G == 0 && h2q_stages(H2Q_G, H2Q_SB, H2Q_SB) == 8 && h2q_images(H2Q_SB, H2Q_G, H2Q_SB, H2Q_SB) == 31 &&
              h2q_last_parity(H2Q_SB, H2Q_G, H2Q_SB, H2Q_SB) == 0 && h2q_last_parity(H2Q_SB, H2Q_G, H2Q_SB, 6) == 1 &&
              h2q_stage_image(H2Q_SB, H2Q_G, 4) == 1 && h2q_stage_image(H2Q_SB, H2Q_G, 7) == 13, "a full pair: 31 images, the last an even one");
// images executed per mixture tile over a group of `n_models` models in blocks of sb, paired (or block by block)
SR_HD constexpr int h2q_group_images(int sb, int g, int n_models, bool paired) {
    int n = 0, left = n_models;
    while (left > 0) {
        const int m1 = left < sb ? left : sb;
        left -= m1;
        int m2 = 0;
        if (paired && left > 0 && m1 == sb) {
            m2 = left < sb ? left : sb;
            left -= m2;
        }
        n += h2q_images(sb, g, m1, m2);
    }
    return n;
}
static_assert(h2q_group_images(H2Q_SB, H2Q_G, 201, false) == 216 && h2q_group_images(H2Q_SB, H2Q_G, 201, true) == 210, "BASELINE configs[2]: 201 models");

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
