// model_pack_parts.hpp -- what the packers of model_pack.hpp share, each stated once: the constants, the set's centre, the fp16
// scale, a mixture's expanded form, the slot map of an image, the block table, the host threads.  Internal to model_pack.cpp and
// model_pack_shared.cpp; inline, because the loops that call these run ~10^8 times for a large enrolment.
// The packed bytes are the contract (tests/host/pack_table.inc): where two layouts round an expression differently, both orders
// of operations are kept here side by side.
#pragma once

#include "gmm_model.hpp"

#include <algorithm>
#include <cmath>
#include <thread>

namespace sr {
namespace pack {

constexpr double LOG2E = 1.4426950408889634073599;
constexpr double SQRT_2_PI = 2.5066282746310002;  // gmm.cc:22

// Packing a configs[3]-sized set (1001 models x 2048 mixtures) is ~10^8 log/divide/split steps: the independent pieces
// (models, blocks of 15 models) are shared by a few host threads.  `work(i, thread)` must only write what belongs to piece i
// (and to its thread: at most MAX_THREADS of them).
constexpr int MAX_THREADS = 32;
template <class F>
void host_parallel_for(int n, size_t cost_per_piece, F work) {
    const size_t total = (size_t)n * cost_per_piece;
    const int n_threads = total < ((size_t)1 << 22) ? 1 : std::max(1, std::min({n, (int)std::thread::hardware_concurrency(), MAX_THREADS}));
    auto run = [&](int t) { for (int i = t; i < n; i += n_threads) work(i, t); };
    if (n_threads == 1) return run(0);
    std::vector<std::thread> th;
    for (int t = 1; t < n_threads; t++) th.emplace_back(run, t);
    run(0);
    for (auto &x : th) x.join();
}

// The set's centre, the mean of all mixture means, into center[0 .. dim).  (pack_models asks before it has reported an untrained
// model or one of another dimension: such a model is left out here.)
inline void set_center(const std::vector<const GMM *> &models, int dim, float *center) {
    std::vector<double> acc(dim, 0.0);
    size_t cnt = 0;
    for (const GMM *g : models) {
        if (!g->trained() || g->dim != dim) continue;
        for (int k = 0; k < g->nr_mixtures; k++)
            for (int d = 0; d < dim; d++) acc[d] += g->mean[(size_t)k * dim + d];
        cnt += (size_t)g->nr_mixtures;
    }
    for (int d = 0; d < dim && cnt; d++) center[d] = (float)(acc[d] / (double)cnt);
}

// The sigmas of models [0, n_models): returns max over dims of (max sigma / min sigma), at least 1; with `scale` (the fp16 layouts)
// also the per-dimension power of two 1 / 2^round(log2 of the geometric-mean sigma), the exponent kept within +-40.
inline double sigma_range(const std::vector<const GMM *> &models, size_t n_models, int dim, float *scale) {
    std::vector<double> lsum(dim, 0.0), smin(dim, INFINITY), smax(dim, 0.0);
    size_t cnt = 0;
    for (size_t s = 0; s < n_models; s++) {
        const GMM &g = *models[s];
        for (int k = 0; k < g.nr_mixtures; k++)
            for (int d = 0; d < dim; d++) {
                const double sg = g.sigma[(size_t)k * dim + d];
                if (scale) lsum[d] += std::log2(sg);
                smin[d] = std::min(smin[d], sg);
                smax[d] = std::max(smax[d], sg);
            }
        cnt += (size_t)g.nr_mixtures;
    }
    double ratio = 1.0;
    for (int d = 0; d < dim; d++) {
        ratio = std::max(ratio, smax[d] / smin[d]);
        if (!scale) continue;
        int e = (int)std::lround(lsum[d] / (double)cnt);
        e = std::max(-40, std::min(40, e));
        scale[d] = (float)std::ldexp(1.0, -e);
    }
    return ratio;
}

// What the expanded form takes of a model's sigmas, [K x dim] each: per model in the generic layouts, once for the whole set in
// the shared-sigma ones.
struct SigmaTerms {
    std::vector<double> ln_norm, inv_var;      // ln(sqrt(2 pi) sigma), 1 / sigma^2
    void of(const GMM &g) {
        const size_t n = g.sigma.size();
        ln_norm.resize(n);
        inv_var.resize(n);
        for (size_t e = 0; e < n; e++) {
            const double sg = g.sigma[e];
            ln_norm[e] = std::log(SQRT_2_PI * sg);
            inv_var[e] = 1.0 / (sg * sg);
        }
    }
};

// ---- a mixture in the expanded form (model_pack.hpp):  A2 = -log2e / (2 sigma^2),  A1 = log2e mu' / sigma^2,
// C = log2e (ln w - sum ln(sqrt(2 pi) sigma) - sum mu'^2 / (2 sigma^2)),  mu' = mean - center, on x' = (x - center) * scale ----
// The generic layouts round A2 as (-log2e / 2) * (1 / sigma^2), the shared-sigma ones as (-log2e / 2) / sigma^2: different in the
// last place of the double now and then, and so in a packed bit.  A1, C and amp are the same expression everywhere.
enum class A2Form { TIMES_INVERSE, DIVIDE };
struct ExpandedForm {
    int dim;
    bool f16;               // the fp16 range: constants end at F16_NEG_BIG, dead mixtures are copies (below)
    const float *center;
    const float *scale;     // [dim] powers of two, or nullptr: all 1
    double amp = 0.0;       // max over the mixtures expanded so far of sum_d (mu'_d / sigma_d)^2
    double coef_max = 0.0;  // ... of |coefficient|

    // Row k of model g's images: a2 and a1 receive `dim` coefficients each (nullptr: not wanted; without a1 no constant is formed
    // and 0 is returned), the caller zeroed them; returns C.  `st` holds g's sigma terms.
    // A row past the model's last mixture and, in the fp16 range, a mixture of weight <= 0:
    //   fp32 range: all zeros and C = NEG_BIG (a mixture of weight <= 0 keeps its coefficients);
    //   fp16 range: fp16 cannot say "minus infinity" (-60000 is as low as a constant goes, and a frame far from every mixture
    //   scores BELOW that, so a bare constant would OUTSCORE the real mixtures there): the row is a copy of a real mixture -- itself,
    //   or the model's last -- pushed 60000 log2 units down: always 2^-60000 of something that is in the sum already.
    template <A2Form FORM>
    float expand(const GMM &g, const SigmaTerms &st, int k, float *a2, float *a1) {
        const int K = g.nr_mixtures;
        const float dead = f16 ? F16_NEG_BIG : NEG_BIG;
        const bool pushed_down = f16 && (k >= K || !(g.weights[std::min(k, K - 1)] > 0));
        if (k >= K && !pushed_down) return dead;
        k = std::min(k, K - 1);
        const size_t row = (size_t)k * dim;
        if (a2)
            for (int d = 0; d < dim; d++) {
                const double us = scale ? 1.0 / (double)scale[d] : 1.0;      // x' = z / scale: powers of two, exact
                const double sg = g.sigma[row + d];
                a2[d] = FORM == A2Form::TIMES_INVERSE ? (float)(-0.5 * LOG2E * st.inv_var[row + d] * us * us) : (float)(-0.5 * LOG2E / (sg * sg) * us * us);
                coef_max = std::max(coef_max, (double)std::fabs(a2[d]));
            }
        if (!a1) return 0.0f;
        // ln of a non-positive weight is treated as -inf (the reference's linear-domain sum just adds 0)
        double cst = pushed_down ? 0.0 : g.weights[k] > 0 ? std::log(g.weights[k]) : -INFINITY;
        double a = 0.0;
        for (int d = 0; d < dim; d++) {
            const double us = scale ? 1.0 / (double)scale[d] : 1.0;
            const double mu = g.mean[row + d] - (double)center[d];
            const double iv = st.inv_var[row + d];
            a1[d] = (float)(LOG2E * mu * iv * us);
            coef_max = std::max(coef_max, (double)std::fabs(a1[d]));
            cst -= st.ln_norm[row + d] + 0.5 * mu * mu * iv;
            a += mu * mu * iv;
        }
        amp = std::max(amp, a);
        cst *= LOG2E;
        if (pushed_down) return (float)std::max(cst + (double)F16_NEG_BIG, -65000.0);
        if (!(std::isfinite(cst) && cst > (double)dead)) return dead;
        const float c = (float)cst;
        // (a constant that ROUNDS to `dead`: the generic layouts leave it out of coef_max, the shared-sigma ones count it -- as found)
        if (FORM == A2Form::DIVIDE || c != dead) coef_max = std::max(coef_max, (double)std::fabs(c));
        return c;
    }
};

// ---- images ----
// Slot c of a contraction of 16-slot steps, mixture row i of a 32-mixture tile -> 16-bit element of the image [step][part][lane][8]:
// step c / 16, lane = i + 32 * half with half = (c / 8) % 2, element c % 8.  (One part: the flat image [step][lane][8].)
inline size_t slot_u16(int c, int i, int parts = 1, int part = 0) {
    return ((((size_t)(c >> 4)) * parts + part) * 64 + i + 32 * ((c >> 3) & 1)) * 8 + (c & 7);
}
// row i of a tile image in parts: every coefficient split into the scheme's parts (SPLIT_BF16X3: three, SPLIT_F16X2: two)
inline void put_split_row(uint16_t *tile, int ksteps, int i, const float *coef, int scheme) {
    const int P = scheme == SPLIT_F16X2 ? 2 : 3;
    for (int c = 0; c < ksteps * 16; c++) {
        uint16_t parts[3];
        if (scheme == SPLIT_F16X2)
            split_f16x2(coef[c], parts);
        else
            split_bf16x3(coef[c], parts);
        for (int p = 0; p < P; p++) tile[slot_u16(c, i, P, p)] = parts[p];
    }
}
// row i of a flat image whose slots are 16-bit values already
inline void put_flat_row(uint16_t *img, int ksteps, int i, const uint16_t *slots) {
    for (int c = 0; c < ksteps * 16; c++) img[slot_u16(c, i)] = slots[c];
}

// blocks of SHARED_SB models, each a stream of block_u16 16-bit values
inline std::vector<SharedBlock> shared_blocks(int n_models, size_t block_u16) {
    std::vector<SharedBlock> blocks;
    for (int b = 0; b * SHARED_SB < n_models; b++) {
        SharedBlock sb;
        sb.offset_u4 = (uint32_t)(((size_t)b * block_u16) / 8);
        sb.first_model = b * SHARED_SB;
        sb.n_models = std::min(SHARED_SB, n_models - b * SHARED_SB);
        sb.pad = 0;
        blocks.push_back(sb);
    }
    return blocks;
}

}  // namespace pack
}  // namespace sr
