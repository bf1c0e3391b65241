// abi_model.cpp -- diagonal GMM handles, their text form, and packed model sets.
#include "abi_internal.hpp"

#include "gmm_model.hpp"
#include "score.hpp"

#include <cstring>

using namespace sr;

namespace sr {
// The handle's one-model set on the current device: packed (every layout a small set carries) and uploaded once, until training
// changes the parameters.  The caller holds this device's lock.
std::shared_ptr<SRModelSet> single_model_set(const GMM *g) {
    if (!g) fail("null GMM handle");
    if (!g->trained()) fail("GMM has no parameters yet (train or load it first)");
    auto &slot = g->single[current_device()];          // one per device
    if (!slot || slot->device != ctx().device) {
        auto s = std::make_shared<SRModelSet>();
        pack_model_set(*s, {g});
        upload_model_set(*s);
        slot = s;
    }
    return slot;
}
}  // namespace sr

extern "C" {

void sr_free_gmm(GMM *gmm) { delete gmm; }

GMM *sr_gmm_from_arrays(int K, int D, const double *weights, const double *mean, const double *sigma) {
    SR_TRY
    if (K <= 0 || D <= 0 || !weights || !mean || !sigma) fail("bad arguments to sr_gmm_from_arrays");
    auto g = std::make_unique<GMM>();
    g->nr_mixtures = K;
    g->dim = D;
    g->weights.assign(weights, weights + K);
    g->mean.assign(mean, mean + (size_t)K * D);
    g->sigma.assign(sigma, sigma + (size_t)K * D);
    for (double s : g->sigma)
        if (!(s > 0)) fail("sigma must be positive");
    return g.release();
    SR_CATCH(nullptr)
}

int sr_gmm_get_params(GMM *g, double *weights, double *mean, double *sigma) {
    SR_TRY
    if (!g || !g->trained()) fail("GMM has no parameters");
    if (weights) std::memcpy(weights, g->weights.data(), sizeof(double) * g->weights.size());
    if (mean) std::memcpy(mean, g->mean.data(), sizeof(double) * g->mean.size());
    if (sigma) std::memcpy(sigma, g->sigma.data(), sizeof(double) * g->sigma.size());
    return 0;
    SR_CATCH(-1)
}

int sr_gmm_dumps(GMM *g, char *buf, long buflen, long *needed) {
    SR_TRY
    if (!g) fail("null GMM handle");
    const std::string s = gmm_format_text(*g);
    if (needed) *needed = (long)s.size() + 1;
    if (buf && buflen > (long)s.size()) {
        std::memcpy(buf, s.c_str(), s.size() + 1);
        return 0;
    }
    return buf ? -2 : 0;
    SR_CATCH(-1)
}

GMM *sr_gmm_loads(const char *text) {
    SR_TRY
    if (!text) fail("null text");
    auto g = std::make_unique<GMM>();
    gmm_parse_text(text, *g);
    return g.release();
    SR_CATCH(nullptr)
}

SRModelSet *sr_modelset_create(GMM *const *models, int n_models) {
    SR_TRY
    if (!models || n_models <= 0) fail("empty model list");
    std::vector<const GMM *> v(models, models + n_models);
    for (auto *m : v)
        if (!m) fail("null GMM handle in model list");
    auto s = std::make_unique<SRModelSet>();
    pack_model_set(*s, v);
    upload_model_set(*s);
    return s.release();
    SR_CATCH(nullptr)
}

void sr_modelset_free(SRModelSet *set) { delete set; }

// Conditioning of a packed set, as the engine dispatcher sees it (score.hpp): out[0] = amp (max_k
// sum_d (mu'_kd / sigma_kd)^2 of the expanded form), out[1] = padding waste of the 32-mixture tiles,
// out[2] = largest per-dimension sigma ratio, out[3] = largest scaled coefficient (fp16 schemes),
// out[4] = 1 when the set shares sigma and weights, out[5] = models, out[6] = device.
int sr_modelset_info(SRModelSet *set, double *out8) {
    SR_TRY
    if (!set || !out8) fail("null argument");
    for (int i = 0; i < 8; i++) out8[i] = 0.0;
    const bool shared = !set->h2s.params.empty() || !set->shared.params.empty();
    if (!set->h2s.params.empty()) {
        out8[0] = set->h2s.amp; out8[1] = set->h2s.pad_waste; out8[2] = set->h2s.sigma_ratio; out8[3] = set->h2s.coef_max;
    } else if (!set->h2.params.empty()) {
        out8[0] = set->h2.amp; out8[1] = set->h2.pad_waste; out8[2] = set->h2.sigma_ratio; out8[3] = set->h2.coef_max;
    } else if (!set->shared.params.empty()) {
        out8[0] = set->shared.amp; out8[1] = set->shared.pad_waste;
    } else if (!set->bx3.params.empty()) {
        out8[0] = set->bx3.amp; out8[1] = set->bx3.pad_waste; out8[2] = set->bx3.sigma_ratio;
    }
    out8[4] = shared ? 1.0 : 0.0;
    out8[5] = set->host.n_models;
    out8[6] = set->device;
    out8[7] = set->hy_good ? set->hy_bad_mixtures : 0;      // hybrid form: mixtures (of the largest model) on the vector engine
    return 0;
    SR_CATCH(-1)
}
int sr_modelset_size(SRModelSet *set) { return set ? set->host.n_models : 0; }
int sr_modelset_dim(SRModelSet *set) { return set ? set->host.dim : 0; }

}  // extern "C"
