// abi_legacy.cpp -- the reference's ten symbols (src/gmm/src/pygmm.hh:28-41) on top of the HIP path, and their contiguous forms
// (sr_score_frames_f32, sr_train_f32, sr_score_models_f32): the entry points a process that lost its GPU runtime to fork() hands to
// its helper (fork_proxy.cpp).  Nothing throws across this file.
#include "abi_internal.hpp"

#include "em.hpp"
#include "fork_proxy.hpp"
#include "gmm_model.hpp"
#include "ref_rand.hpp"
#include "score.hpp"

#include <cstring>
#include <fstream>
#include <limits>
#include <sstream>
#include <vector>

using namespace sr;

static SRModelSet &single_set(GMM *g) { return *sr::single_model_set(g); }

// double** rows -> contiguous fp32 (the reference deep-copies too: pygmm.cc:16-23)
static std::vector<float> rows_to_f32(double **X, long n, int dim) {
    if (n > 0 && !X) fail("null X_in");
    std::vector<float> out((size_t)n * dim);
    for (long i = 0; i < n; i++) {
        const double *r = X[i];
        for (int j = 0; j < dim; j++) out[(size_t)i * dim + j] = (float)r[j];
    }
    return out;
}

// The legacy ABI scores ONE model per call, and its callers loop over the speakers with the same
// utterance (gmmset.py:59-64, :95-99: S calls of score_all(x)): re-uploading x S times would make
// the drop-in path pay S H2D copies and S tile-table builds.  The last uploaded matrix stays on the
// device, keyed by shape and CONTENTS: a call's matrix is compared with the host copy kept beside the device one (memcmp: 5 us
// for 1000 x 39 frames on a hit, a few bytes on a miss).  (Through round 5 a 64-bit FNV-1a hash went first: a dependent
// multiply per 8 bytes, 20 us of a 60 us call, for a comparison that decides by itself.)  Matrices above LEGACY_CACHE_MAX_BYTES
// are not kept (neither copy outlives the call).
constexpr size_t LEGACY_CACHE_MAX_BYTES = (size_t)256 << 20;
struct LegacyFeatureCache {
    long n = -1;
    int dim = -1;
    std::vector<float> host;
    std::unique_ptr<SRBatch> batch;
};

// One model against a contiguous fp32 matrix: here, or -- in a process that lost its GPU runtime to fork() -- in its helper.
static void score_one(GMM *g, const float *X, long n, int dim, float *ll_out, double *sum_out, int flags) {
    if (gpu_runtime_lost()) return fork_proxy_score(g, X, n, dim, ll_out, sum_out, flags);
    score_one_local(g, X, n, dim, ll_out, sum_out, flags);
}
static int train_one(GMM &gmm, const GMM *ubm, const float *X, long n, int dim, const Parameter &param, long seed) {
    if (gpu_runtime_lost()) return fork_proxy_train(gmm, ubm, X, n, dim, param, seed);
    return train_em(gmm, ubm, X, n, dim, param, seed);
}

void sr::score_one_local(GMM *g, const float *X, long n, int dim, float *ll_out, double *sum_out, int flags) {
    SRModelSet &set = single_set(g);
    if (dim != g->dim) fail("nr_dim %d does not match the model's dim %d", dim, g->dim);
    auto &cache = per_device<LegacyFeatureCache>();
    const size_t bytes = (size_t)n * dim * sizeof(float);
    const bool hit = cache.batch && cache.n == n && cache.dim == dim &&
                     cache.host.size() * sizeof(float) == bytes && std::memcmp(cache.host.data(), X, bytes) == 0;
    if (!hit) {
        const int64_t off[2] = {0, n};
        cache.batch.reset();                               // (frees the previous matrix before the new one is allocated)
        cache.batch = feature_batch(X, n, dim, off, 1);
        cache.n = n;
        cache.dim = dim;
        if (bytes <= LEGACY_CACHE_MAX_BYTES) cache.host.assign(X, X + (size_t)n * dim);
        else std::vector<float>().swap(cache.host);
    }
    double sum = 0.0;
    score_batch_set(set, *cache.batch, &sum, nullptr, ll_out, flags);
    if (sum_out) *sum_out = sum;
    if (bytes > LEGACY_CACHE_MAX_BYTES) {                  // too large to pin in HBM between calls
        cache.batch.reset();
        cache.n = -1;
    }
}

// Several models on ONE utterance in one fused pass (sr_score_models_f32): what gmmset.py:95-99's loop of score_all calls computes.
// The packed set of the last model list stays on the device, keyed by every model's identity and parameter generation.
namespace {
struct ModelsSetCache {
    std::vector<std::pair<uint64_t, uint64_t>> key;      // (uid, generation) per model
    std::unique_ptr<SRModelSet> set;
    std::unique_ptr<SRBatch> batch;                      // refilled per call (device buffers only grow)
};
}  // namespace
void sr::score_models_local(GMM *const *models, int n_models, const float *X, long n, int dim, double *sums_out, int flags) {
    if (!models || n_models <= 0) fail("empty model list");
    if (!sums_out) fail("null sums_out");
    if (n < 0 || dim <= 0) fail("bad frame matrix shape");
    if (n > 0 && !X) fail("null X");
    std::vector<std::pair<uint64_t, uint64_t>> key((size_t)n_models);
    for (int i = 0; i < n_models; i++) {
        const GMM *g = models[i];
        if (!g) fail("null GMM handle in model list");
        if (!g->trained()) fail("GMM has no parameters yet (train or load it first)");
        if (g->dim != dim) fail("nr_dim %d does not match model %d's dim %d", dim, i, g->dim);
        key[(size_t)i] = {g->uid, g->generation};
    }
    ensure_device();
    auto &cache = per_device<ModelsSetCache>();
    if (!cache.set || cache.key != key || cache.set->device != ctx().device) {
        cache.set.reset();
        auto s = std::make_unique<SRModelSet>();
        pack_model_set(*s, std::vector<const GMM *>(models, models + n_models));
        upload_model_set(*s);
        cache.set = std::move(s);
        cache.key = key;
    }
    const int64_t off[2] = {0, n};
    if (!cache.batch) {
        cache.batch = feature_batch(X, n, dim, off, 1);
    } else if (sr_batch_reset_features(cache.batch.get(), X, n, dim, off, 1) != 0) {
        fail("%s", last_error().c_str());
    }
    score_batch_set(*cache.set, *cache.batch, sums_out, nullptr, nullptr, flags);
}

extern "C" {

// ======================= Part 1: legacy symbols =======================

GMM *new_gmm(int nr_mixture, int covariance_type) {
    SR_TRY
    if (covariance_type != 1) fail("only diagonal matrix supported.");  // gmm.cc:211-215
    if (nr_mixture <= 0) fail("nr_mixture must be positive");
    GMM *g = new GMM();
    g->nr_mixtures = nr_mixture;
    g->covariance_type = covariance_type;
    return g;
    SR_CATCH(nullptr)
}

GMM *load(const char *model_file) {
    SR_TRY
    if (!model_file) fail("null model_file");
    std::ifstream fin(model_file, std::ios::binary);
    if (!fin) fail("cannot open model file '%s'", model_file);
    std::stringstream ss;
    ss << fin.rdbuf();
    auto g = std::make_unique<GMM>();
    gmm_parse_text(ss.str(), *g);
    burn_reference_rand(g->nr_mixtures);    // GMM::load seeds one Random per Gaussian from libc rand() (gmm.cc:671-676, gmm.hh:44)
    return g.release();
    SR_CATCH(nullptr)
}

void dump(GMM *gmm, const char *model_file) {
    SR_TRY
    if (!gmm || !model_file) fail("null argument to dump");
    std::ofstream fout(model_file, std::ios::binary);
    if (!fout) fail("cannot write model file '%s'", model_file);
    fout << gmm_format_text(*gmm);
    SR_CATCH_VOID
}

// pygmm.cc:31-41
static void print_param_block(const struct Parameter *param) {
    printf("nr_instance   :   %d\n", param->nr_instance);
    printf("nr_dim        :   %d\n", param->nr_dim);
    printf("nr_mixture    :   %d\n", param->nr_mixture);
    printf("min_covar     :   %f\n", param->min_covar);
    printf("threshold     :   %f\n", param->threshold);
    printf("nr_iteration  :   %d\n", param->nr_iteration);
    printf("init_with_kmeans: %d\n", param->init_with_kmeans);
    printf("concurrency   :   %d\n", param->concurrency);
    printf("verbosity     :   %d\n", param->verbosity);
}

void train_model(GMM *gmm, double **X_in, struct Parameter *param) {
    SR_TRY
    if (!gmm || !param) fail("null argument to train_model");
    if (reference_side_effects()) print_param_block(param);
    std::vector<float> X = rows_to_f32(X_in, param->nr_instance, param->nr_dim);
    if (train_one(*gmm, nullptr, X.data(), param->nr_instance, param->nr_dim, *param, -1) < 0)
        fail("%s", last_error().c_str());
    SR_CATCH_VOID
}

void train_model_from_ubm(GMM *gmm, GMM *ubm, double **X_in, struct Parameter *param) {
    SR_TRY
    if (!gmm || !ubm || !param) fail("null argument to train_model_from_ubm");
    if (reference_side_effects()) print_param_block(param);
    std::vector<float> X = rows_to_f32(X_in, param->nr_instance, param->nr_dim);
    if (train_one(*gmm, ubm, X.data(), param->nr_instance, param->nr_dim, *param, -1) < 0)
        fail("%s", last_error().c_str());
    SR_CATCH_VOID
}

double score_all(GMM *gmm, double **X_in, int nr_instance, int nr_dim, int /*concurrency*/) {
    SR_TRY
    std::vector<float> X = rows_to_f32(X_in, nr_instance, nr_dim);
    double sum = 0.0;
    score_one(gmm, X.data(), nr_instance, nr_dim, nullptr, &sum, SR_CLAMP_COMPAT);
    return sum;
    SR_CATCH(std::numeric_limits<double>::quiet_NaN())
}

void score_batch(GMM *gmm, double **X_in, double *prob_out, int nr_instance, int nr_dim,
                 int /*concurrency*/) {
    SR_TRY
    if (nr_instance > 0 && !prob_out) fail("null prob_out");
    std::vector<float> X = rows_to_f32(X_in, nr_instance, nr_dim);
    std::vector<float> ll((size_t)nr_instance);
    score_one(gmm, X.data(), nr_instance, nr_dim, ll.data(), nullptr, SR_CLAMP_COMPAT);
    for (int i = 0; i < nr_instance; i++) prob_out[i] = ll[i];
    SR_CATCH_VOID
}

double score_instance(GMM *gmm, double *x_in, int nr_dim) {
    SR_TRY
    if (!x_in) fail("null x_in");
    double *rows[1] = {x_in};
    std::vector<float> X = rows_to_f32(rows, 1, nr_dim);
    double sum = 0.0;
    score_one(gmm, X.data(), 1, nr_dim, nullptr, &sum, SR_CLAMP_COMPAT);
    return sum;
    SR_CATCH(std::numeric_limits<double>::quiet_NaN())
}

int get_dim(GMM *gmm) { return gmm ? gmm->dim : 0; }
int get_nr_mixtures(GMM *gmm) { return gmm ? gmm->nr_mixtures : 0; }

int sr_score_frames_f32(GMM *gmm, const float *X, long n, int dim, float *ll_out, double *sum_out,
                        int flags) {
    SR_TRY
    if (n > 0 && !X) fail("null X");
    score_one(gmm, X, n, dim, ll_out, sum_out, flags);
    return 0;
    SR_CATCH(-1)
}

int sr_train_f32(GMM *gmm, GMM *ubm_or_null, const float *X, long n, int dim,
                 const struct Parameter *param, long seed) {
    SR_TRY
    if (!gmm || !X || !param) fail("null argument to sr_train_f32");
    return train_one(*gmm, ubm_or_null, X, n, dim, *param, seed);
    SR_CATCH(-1)
}

int sr_score_models_f32(GMM *const *models, int n_models, const float *X, long n_frames, int dim, double *sums_out, int flags) {
    SR_TRY
    if (gpu_runtime_lost()) fork_proxy_score_models(models, n_models, X, n_frames, dim, sums_out, flags);
    else score_models_local(models, n_models, X, n_frames, dim, sums_out, flags);
    return 0;
    SR_CATCH(-1)
}

int sr_reference_rand_sample(int *out, int count) {
    SR_TRY
    if (!out || count < 0) fail("bad arguments");
    reference_rand_sample(out, count);
    return 0;
    SR_CATCH(-1)
}

}  // extern "C"
