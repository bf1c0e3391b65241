// model_pack_shared.cpp -- the layouts of sets that share sigma and weights (model_pack.hpp): split-bf16, two fp16 parts, and the
// compact order of the latter.
#include "model_pack_parts.hpp"
#include "score_shapes.hpp"

#include <cstring>

namespace sr {

using namespace pack;

PackedBx3Shared pack_models_bx3_shared(const std::vector<const GMM *> &models) {
    PackedBx3Shared pm;
    const GMM &g0 = *models[0];
    const int dim = g0.dim, K = g0.nr_mixtures;
    const int S = (int)models.size();
    pm.kq = (dim + 15) / 16;
    pm.kl = (dim + 1 + 15) / 16;
    pm.n_tiles = (K + MT - 1) / MT;
    const size_t q_u16 = (size_t)pm.kq * 3 * 64 * 8, l_u16 = (size_t)pm.kl * 3 * 64 * 8;
    pm.center.assign(dim, 0.0f);
    set_center(models, dim, pm.center.data());
    ExpandedForm ef{dim, false, pm.center.data(), nullptr};
    SigmaTerms st;
    st.of(g0);                                               // sigma is common to the set
    const size_t block_u16 = (size_t)pm.n_tiles * (q_u16 + (size_t)SHARED_SB * l_u16);
    pm.blocks = shared_blocks(S, block_u16);
    pm.params.assign(pm.blocks.size() * block_u16, 0);
    // the quadratic tiles are the same in every block
    std::vector<uint16_t> qimg((size_t)pm.n_tiles * q_u16, 0);
    std::vector<float> coef((size_t)std::max(pm.kq, pm.kl) * 16);
    for (int t = 0; t < pm.n_tiles; t++)
        for (int i = 0; i < MT; i++) {
            std::fill(coef.begin(), coef.end(), 0.0f);
            ef.expand<A2Form::DIVIDE>(g0, st, t * MT + i, coef.data(), nullptr);
            put_split_row(qimg.data() + (size_t)t * q_u16, pm.kq, i, coef.data(), SPLIT_BF16X3);
        }
    for (size_t b = 0; b < pm.blocks.size(); b++) {
        uint16_t *bp = pm.params.data() + b * block_u16;
        for (int t = 0; t < pm.n_tiles; t++) {
            uint16_t *tp = bp + (size_t)t * (q_u16 + (size_t)SHARED_SB * l_u16);
            std::memcpy(tp, qimg.data() + (size_t)t * q_u16, q_u16 * sizeof(uint16_t));
            for (int si = 0; si < SHARED_SB; si++) {
                uint16_t *lt = tp + q_u16 + (size_t)si * l_u16;
                for (int i = 0; i < MT; i++) {
                    std::fill(coef.begin(), coef.end(), 0.0f);
                    // (a phantom model of the last block: zeros and C = -1e30)
                    coef[(size_t)pm.kl * 16 - 1] =
                        si < pm.blocks[b].n_models ? ef.expand<A2Form::DIVIDE>(*models[b * SHARED_SB + si], st, t * MT + i, nullptr, coef.data()) : NEG_BIG;
                    put_split_row(lt, pm.kl, i, coef.data(), SPLIT_BF16X3);
                }
            }
        }
    }
    pm.amp = ef.amp;
    pm.pad_waste = 1.0 - ((double)K * S) / ((double)pm.n_tiles * MT * pm.blocks.size() * SHARED_SB);
    return pm;
}

PackedH2Shared pack_models_h2_shared(const std::vector<const GMM *> &models) {
    PackedH2Shared pm;
    const GMM &g0 = *models[0];
    const int dim = g0.dim, K = g0.nr_mixtures;
    const int S = (int)models.size();
    pm.kqf = (3 * dim + 15) / 16;
    pm.klf = (3 * dim + 2 + 15) / 16;
    pm.n_tiles = (K + MT - 1) / MT;
    const int kimg = std::max(pm.kqf, pm.klf);
    const size_t img_u16 = (size_t)kimg * 64 * 8;
    // centre and scale for the whole set from the SET's statistics: sigma is common (the first model's will do), the centre
    // takes the means of all models
    pm.center.assign(dim, 0.0f);
    pm.scale.assign(dim, 1.0f);
    set_center(models, dim, pm.center.data());
    pm.sigma_ratio = sigma_range(models, 1, dim, pm.scale.data());
    // slot tables (frame side)
    pm.q_desc.assign((size_t)pm.kqf * 16, 0);
    pm.l_desc.assign((size_t)pm.klf * 16, 0);
    // slot of part product `part` (0 lo x hi, 1 hi x lo, 2 hi x hi) of dimension d; the constant's two slots
    // (three runs; interleaving the parts per dimension instead changes nothing: profiles/r05_slot_order_ab.txt)
    auto qpos = [&](int part, int d) { return part * dim + d; };
    auto lpos = [&](int part, int d) { return part == 0 ? d : part == 1 ? (dim + 1) + d : (2 * dim + 1) + d; };
    const int c_lo = dim, c_hi = 3 * dim + 1;
    for (int d = 0; d < dim; d++) {
        pm.q_desc[qpos(0, d)] = (uint16_t)(d | (1 << 8));           // lo(A2) x hi(z^2)
        pm.q_desc[qpos(1, d)] = (uint16_t)(d | (2 << 8));           // hi(A2) x lo(z^2)
        pm.q_desc[qpos(2, d)] = (uint16_t)(d | (1 << 8));           // hi(A2) x hi(z^2)
        pm.l_desc[lpos(0, d)] = (uint16_t)(d | (1 << 8));           // lo(A1) x hi(z)
        pm.l_desc[lpos(1, d)] = (uint16_t)(d | (2 << 8));           // hi(A1) x lo(z)
        pm.l_desc[lpos(2, d)] = (uint16_t)(d | (1 << 8));           // hi(A1) x hi(z)
    }
    pm.l_desc[c_lo] = (uint16_t)(3 << 8);                           // lo(C) x 1
    pm.l_desc[c_hi] = (uint16_t)(3 << 8);                           // hi(C) x 1
    const size_t block_u16 = (size_t)pm.n_tiles * (1 + SHARED_SB) * img_u16;
    pm.blocks = shared_blocks(S, block_u16);
    const int n_blocks = (int)pm.blocks.size();
    pm.params.assign((size_t)n_blocks * block_u16, 0);
    const ExpandedForm ef0{dim, true, pm.center.data(), pm.scale.data()};
    SigmaTerms st;
    st.of(g0);                                               // sigma is common to the set: its logarithms and reciprocals once, not once per model
    // a coefficient row as slots: the low part against hi(z), the high part against lo(z) and against hi(z)
    auto put_parts = [&](const float *a, std::vector<uint16_t> &slots, auto pos) {
        for (int d = 0; d < dim; d++) {
            uint16_t parts[2];
            split_f16x2(a[d], parts);
            slots[pos(0, d)] = parts[1];
            slots[pos(1, d)] = parts[0];
            slots[pos(2, d)] = parts[0];
        }
    };
    // the quadratic images are the same in every block; padding mixtures copy the last real one (see the linear images)
    std::vector<uint16_t> qimg((size_t)pm.n_tiles * img_u16, 0);
    {
        ExpandedForm ef = ef0;
        std::vector<uint16_t> slots((size_t)pm.kqf * 16);
        std::vector<float> a2(dim);
        for (int t = 0; t < pm.n_tiles; t++)
            for (int i = 0; i < MT; i++) {
                std::fill(slots.begin(), slots.end(), 0);
                ef.expand<A2Form::DIVIDE>(g0, st, t * MT + i, a2.data(), nullptr);
                put_parts(a2.data(), slots, qpos);
                put_flat_row(qimg.data() + (size_t)t * img_u16, pm.kqf, i, slots.data());
            }
        pm.coef_max = ef.coef_max;
    }
    double amp_t[MAX_THREADS] = {0}, coef_t[MAX_THREADS] = {0};
    host_parallel_for(n_blocks, (size_t)SHARED_SB * K * dim, [&](int b, int thr) {
        ExpandedForm ef = ef0;
        std::vector<uint16_t> slots((size_t)pm.klf * 16);
        std::vector<float> a1(dim);
        uint16_t *bp = pm.params.data() + (size_t)b * block_u16;
        for (int t = 0; t < pm.n_tiles; t++) {
            uint16_t *tp = bp + (size_t)t * (1 + SHARED_SB) * img_u16;
            std::memcpy(tp, qimg.data() + (size_t)t * img_u16, img_u16 * sizeof(uint16_t));
            for (int si = 0; si < SHARED_SB; si++) {
                uint16_t *lt = tp + (size_t)(1 + si) * img_u16;
                for (int i = 0; i < MT; i++) {
                    std::fill(slots.begin(), slots.end(), 0);
                    float cst_f = F16_NEG_BIG;               // (a phantom model of the last block: zeros and C = -60000)
                    if (si < pm.blocks[b].n_models) {
                        cst_f = ef.expand<A2Form::DIVIDE>(*models[b * SHARED_SB + si], st, t * MT + i, nullptr, a1.data());
                        put_parts(a1.data(), slots, lpos);
                    }
                    uint16_t parts[2];
                    split_f16x2(cst_f, parts);
                    slots[c_lo] = parts[1];
                    slots[c_hi] = parts[0];
                    put_flat_row(lt, pm.klf, i, slots.data());
                }
            }
        }
        amp_t[thr] = std::max(amp_t[thr], ef.amp);
        coef_t[thr] = std::max(coef_t[thr], ef.coef_max);
    });
    for (int t = 0; t < MAX_THREADS; t++) {
        pm.amp = std::max(pm.amp, amp_t[t]);
        pm.coef_max = std::max(pm.coef_max, coef_t[t]);
    }
    pm.pad_waste = 1.0 - ((double)K * S) / ((double)pm.n_tiles * MT * n_blocks * SHARED_SB);
    pm.ref = pack_models_split({models[0]}, SPLIT_F16X2);
    return pm;
}

PackedH2Compact pack_h2_compact(const PackedH2Shared &pm, int dim) {
    PackedH2Compact pc;
    if (pm.params.empty() || !h2c_applies(dim, pm.klf)) return pc;
    const int h = h2c_half_steps(dim);
    const H2cMap m = h2c_map(h);
    pc.nk = m.nk;
    pc.nf = m.nf;
    pc.nb = m.nb;
    const int c_slot = 8 * h - 1;                        // the constant's place in a part: the last slot of the last half-step
    // where the flat order keeps part `part` (0 hi, 1 lo) of slot s of a part, as a slot of the flat contraction (-1: nowhere, zero)
    auto flat_slot = [&](bool linear, int part, int s) {
        if (s < dim) return part == 1 ? s : linear ? 2 * dim + 1 + s : 2 * dim + s;
        if (linear && s == c_slot) return part == 1 ? dim : 3 * dim + 1;
        return -1;
    };
    // frame side: descriptor of slot s of part `part` (0 low part of z, 1 high part)
    auto b_desc = [&](bool linear, int part, int s) -> uint16_t {
        if (s < dim) return (uint16_t)(s | ((part == 1 ? 1 : 2) << 8));
        if (linear && s == c_slot && part == 1) return (uint16_t)(3 << 8);
        return 0;
    };
    pc.q_desc.assign((size_t)m.nb * 16, 0);
    pc.l_desc.assign((size_t)m.nb * 16, 0);
    for (int r = 0; r < m.nb; r++)
        for (int hh = 0; hh < 2; hh++)
            for (int j = 0; j < 8; j++) {
                const int half = m.b_half[r][hh];
                if (half < 0) continue;
                pc.q_desc[16 * r + 8 * hh + j] = b_desc(false, half >> 4, 8 * (half & 15) + j);
                pc.l_desc[16 * r + 8 * hh + j] = b_desc(true, half >> 4, 8 * (half & 15) + j);
            }
    // u16 of a compact image -> u16 of the flat image it copies (-1: zero), for the two kinds of image
    const size_t flat_u16 = (size_t)std::max(pm.kqf, pm.klf) * 64 * 8, img_u16 = (size_t)m.nf * 64 * 8;
    std::vector<int> src[2];
    for (int linear = 0; linear < 2; linear++) {
        src[linear].assign(img_u16, -1);
        for (int f = 0; f < m.nf; f++)
            for (int hh = 0; hh < 2; hh++) {
                const int half = m.a_half[f][hh];
                if (half < 0) continue;
                for (int j = 0; j < 8; j++) {
                    const int c = flat_slot(linear != 0, half >> 4, 8 * (half & 15) + j);
                    if (c < 0) continue;
                    for (int i = 0; i < MT; i++) src[linear][slot_u16(16 * f + 8 * hh + j, i)] = (int)slot_u16(c, i);
                }
            }
    }
    const size_t n_img = pm.params.size() / flat_u16;
    const size_t per_block = (size_t)pm.n_tiles * (1 + SHARED_SB);
    pc.params.assign(n_img * img_u16, 0);
    for (size_t im = 0; im < n_img; im++) {
        const uint16_t *from = pm.params.data() + im * flat_u16;
        uint16_t *to = pc.params.data() + im * img_u16;
        const int j_img = (int)(im % (1 + SHARED_SB));
        if (j_img > pm.blocks[im / per_block].n_models) continue;           // a phantom model's image: zeros (its sums are never read)
        const std::vector<int> &sv = src[j_img != 0];
        for (size_t e = 0; e < img_u16; e++)
            if (sv[e] >= 0) to[e] = from[sv[e]];
    }
    pc.blocks = pm.blocks;
    for (size_t b = 0; b < pc.blocks.size(); b++) pc.blocks[b].offset_u4 = (uint32_t)((b * per_block * img_u16) / 8);
    return pc;
}

}  // namespace sr
