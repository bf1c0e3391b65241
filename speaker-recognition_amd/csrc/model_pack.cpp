// model_pack.cpp -- parameter packing (host, float64 -> fp32 tables and 16-bit parts): the vector layout and the generic
// matrix-core layouts of model_pack.hpp.  The shared-sigma layouts: model_pack_shared.cpp.
#include "model_pack_parts.hpp"

#include <cstring>
#include <limits>

namespace sr {

using namespace pack;

// 8..64: every engine; 80, 96: the vector-ALU engine with one frame per lane (the matrix-core layouts stop at 64);
// wider rows: whole slices of WIDE_DC dimensions for the D-chunked kernels (gmm_score_wide_kernel, em_stats_wide_kernel) --
// the reference has no limit (gmm.cc:40-51), MAX_DIM only keeps a corrupt model file from asking for terabytes
static const int kDims[] = {8, 13, 16, 24, 26, 32, 34, 39, 40, 48, 56, 64, 80, 96};

int pick_padded_dim(int dim) {
    for (int d : kDims)
        if (d >= dim) return d;
    if (dim <= MAX_DIM) return (dim + WIDE_DC - 1) / WIDE_DC * WIDE_DC;
    fail("feature dim %d > %d", dim, MAX_DIM);
}

PackedModels pack_models(const std::vector<const GMM *> &models) {
    if (models.empty()) fail("empty model set");
    PackedModels pm;
    pm.n_models = (int)models.size();
    pm.dim = models[0]->dim;
    pm.dp = pick_padded_dim(pm.dim);
    const int DP = pm.dp;
    const size_t rec_f4 = (size_t)2 * DP + 1;
    pm.center.assign(DP, 0.0f);
    set_center(models, pm.dim, pm.center.data());
    pm.model_chunk_begin.push_back(0);
    std::vector<size_t> base(pm.n_models);
    size_t total_f4 = 0;
    for (int s = 0; s < pm.n_models; s++) {
        const GMM &g = *models[s];
        if (!g.trained()) fail("model %d of the set is untrained/empty", s);
        if (g.dim != pm.dim) fail("model %d has dim %d, set has %d", s, g.dim, pm.dim);
        const int n_rec = (g.nr_mixtures + KB - 1) / KB;
        base[s] = total_f4;
        for (int r0 = 0; r0 < n_rec; r0 += CB) {
            ChunkDesc cd;
            cd.offset_f4 = (uint32_t)(total_f4 + (size_t)r0 * rec_f4);
            cd.n_records = std::min(CB, n_rec - r0);
            cd.model_done = (r0 + CB >= n_rec) ? s : -1;
            cd.pad = 0;
            pm.chunks.push_back(cd);
        }
        pm.model_chunk_begin.push_back((int)pm.chunks.size());
        pm.model_mixtures.push_back(g.nr_mixtures);
        total_f4 += (size_t)n_rec * rec_f4;
    }
    if (total_f4 >= ((size_t)1 << 32)) fail("model set of %zu parameter records of 16 bytes: chunk offsets are 32-bit", total_f4);
    pm.params.assign(total_f4 * 4, 0.0f);
    std::vector<double> lift(pm.n_models, 0.0);             // per model: max_k sum_d max(0, -ln sigma_kd)
    host_parallel_for(pm.n_models, (size_t)models[0]->nr_mixtures * pm.dim, [&](int s, int) {
        const GMM &g = *models[s];
        const int K = g.nr_mixtures;
        const int n_rec = (K + KB - 1) / KB;
        for (int r = 0; r < n_rec; r++) {
            float *rec = pm.params.data() + (base[s] + (size_t)r * rec_f4) * 4;
            for (int j = 0; j < KB; j++) {
                const int k = r * KB + j;
                float *cslot = rec + (size_t)2 * DP * 4 + j;
                if (k >= K) {
                    *cslot = NEG_BIG;
                    continue;
                }
                // c = log2e * (ln w - sum ln(sqrt(2pi) sigma)); ln of a non-positive weight is
                // treated as -inf -> NEG_BIG (the reference's linear-domain sum just adds 0).
                double c = g.weights[k] > 0 ? std::log(g.weights[k]) : -INFINITY;
                double up = 0.0;
                for (int d = 0; d < pm.dim; d++) {
                    const double sg = g.sigma[(size_t)k * pm.dim + d];
                    up += std::max(0.0, -std::log(sg));
                    const double mu = g.mean[(size_t)k * pm.dim + d] - (double)pm.center[d];
                    const double sc = std::sqrt(LOG2E * 0.5) / sg;
                    // record layout: dim d -> two float4: {s0,m0,s1,m1} {s2,m2,s3,m3}
                    float *pair = rec + (size_t)d * 8 + (size_t)j * 2;
                    pair[0] = (float)sc;
                    pair[1] = (float)(-mu * sc);
                    c -= std::log(SQRT_2_PI * sg);
                }
                c *= LOG2E;
                *cslot = (std::isfinite(c) && c > (double)NEG_BIG) ? (float)c : NEG_BIG;
                // (a degenerate mixture -- sigma 0 or negative: -ln sigma is inf or NaN -- must not lower the band: with an infinite
                // band every frame of the set goes through the exact partial-product path instead of being silently skipped)
                lift[s] = std::isfinite(up) ? std::max(lift[s], up) : std::numeric_limits<double>::infinity();
            }
        }
    });
    int kmax = 1;
    for (const GMM *g : models) kmax = std::max(kmax, g->nr_mixtures);
    pm.flush_band = *std::max_element(lift.begin(), lift.end()) + std::log((double)kmax) + 17.5;
    return pm;
}

// Slot of a step's 16 that holds A2 (pw = 0, against x'^2) or A1 (pw = 1, against x') of feature d: the features of half hh of step
// ks are f0..f3 = 8 ks + 4 hh + 0..3, in the order  A2 f0, A2 f1, A1 f0, A1 f1, A2 f2, A2 f3, A1 f2, A1 f3 -- a lane of the frame
// side owns BOTH powers of four features, in the pairs its packed instructions produce (split_prologue.hpp).  The last slot (A1 of
// d = 8 KS - 1 >= dim) carries C (pairs with the constant 1).
static inline int split_slot(int d, int pw) { return 16 * (d >> 3) + 8 * ((d >> 2) & 1) + 4 * ((d >> 1) & 1) + 2 * pw + (d & 1); }

PackedSplit pack_models_split(const std::vector<const GMM *> &models, int scheme) {
    PackedSplit pm;
    const bool f16 = scheme == SPLIT_F16X2;
    pm.scheme = scheme;
    pm.parts = f16 ? 2 : 3;
    const int dim = models[0]->dim;
    pm.ks = (dim + 1 + 7) / 8;
    const int KS = pm.ks;
    const size_t tile_u16 = (size_t)KS * pm.parts * 64 * 8;
    pm.center.assign(dim, 0.0f);
    pm.scale.assign(dim, 1.0f);
    set_center(models, dim, pm.center.data());
    pm.sigma_ratio = sigma_range(models, models.size(), dim, f16 ? pm.scale.data() : nullptr);
    ExpandedForm ef{dim, f16, pm.center.data(), pm.scale.data()};
    SigmaTerms st;
    size_t live = 0, padded = 0;
    pm.model_chunk_begin.push_back(0);
    std::vector<float> sq((size_t)KS * 8), lin((size_t)KS * 8), coef((size_t)KS * 16);
    for (size_t s = 0; s < models.size(); s++) {
        const GMM &g = *models[s];
        const int K = g.nr_mixtures;
        const int n_tiles = (K + MT - 1) / MT;
        const size_t base = pm.params.size();
        pm.params.resize(base + (size_t)n_tiles * tile_u16, 0);
        live += (size_t)K;
        padded += (size_t)n_tiles * MT;
        st.of(g);
        for (int t = 0; t < n_tiles; t++) {
            uint16_t *tile = pm.params.data() + base + (size_t)t * tile_u16;
            for (int i = 0; i < MT; i++) {
                std::fill(sq.begin(), sq.end(), 0.0f);
                std::fill(lin.begin(), lin.end(), 0.0f);
                lin[(size_t)KS * 8 - 1] = ef.expand<A2Form::TIMES_INVERSE>(g, st, t * MT + i, sq.data(), lin.data());
                for (int d = 0; d < KS * 8; d++) {
                    coef[split_slot(d, 0)] = sq[d];
                    coef[split_slot(d, 1)] = lin[d];
                }
                put_split_row(tile, KS, i, coef.data(), scheme);
            }
            ChunkDesc cd;
            cd.offset_f4 = (uint32_t)((base + (size_t)t * tile_u16) / 8);
            cd.n_records = 1;
            cd.model_done = (t + 1 == n_tiles) ? (int)s : -1;
            cd.pad = 0;
            pm.chunks.push_back(cd);
        }
        pm.model_chunk_begin.push_back((int)pm.chunks.size());
    }
    pm.amp = ef.amp;
    pm.coef_max = ef.coef_max;
    pm.pad_waste = 1.0 - (double)live / (double)padded;
    // the kernels index both tables with compile-time slot numbers 0 .. 8 KS - 1 (split_prologue.hpp): slots past dim are padded
    pm.center.resize((size_t)8 * KS, 0.0f);
    pm.scale.resize((size_t)8 * KS, 0.0f);
    return pm;
}

bool models_share_sigma_and_weights(const std::vector<const GMM *> &models) {
    if (models.size() < 2) return false;
    const GMM &a = *models[0];
    for (size_t s = 1; s < models.size(); s++) {
        const GMM &b = *models[s];
        if (b.nr_mixtures != a.nr_mixtures || b.dim != a.dim) return false;
        if (std::memcmp(a.weights.data(), b.weights.data(), sizeof(double) * a.weights.size()) != 0) return false;
        if (std::memcmp(a.sigma.data(), b.sigma.data(), sizeof(double) * a.sigma.size()) != 0) return false;
    }
    return true;
}

}  // namespace sr
