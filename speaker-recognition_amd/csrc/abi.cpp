// abi.cpp -- extern "C" surface of lib/pygmm.so (declared in include/pygmm_hip.h).
// Part 1 reproduces the reference's ten symbols (src/gmm/src/pygmm.hh:28-41) on top of the
// HIP path; part 2 is the contiguous / batched interface.  Nothing throws across this file.
#include "../../include/pygmm_hip.h"

#include "batch.hpp"
#include "common.hpp"
#include "fork_proxy.hpp"
#include "gmm_full.hpp"
#include "gmm_model.hpp"
#include "kmeans_init.hpp"
#include "mfcc.hpp"
#include "mfcc_plan.hpp"
#include "score.hpp"
#include "silence_plan.hpp"
#include "featnorm_plan.hpp"
#include "norm_quantile.hpp"
#include "topc_plan.hpp"
#include "bw_plan.hpp"
#include "jfa_plan.hpp"
#include "norm_plan.hpp"
#include "calib_plan.hpp"
#include "plda_plan.hpp"
#include "eig_plan.hpp"
#include "map_plan.hpp"
#include "ref_rand.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <limits>
#include <sstream>

namespace sr {
int train_em(GMM &gmm, const GMM *ubm, const float *X, long n, int dim, const Parameter &param,
             long seed);
void set_em_stats_engine(int v);
void set_em_small_test_absent(int v);   // em_small.hip
int last_em_stats_engine();
void set_reference_side_effects(int v);
// map_batch.hip
int map_fit_batch(GMM *const *models, int S, const GMM *ubm, const float *X, const int64_t *row_offsets, int dim, const Parameter &param,
                  long seed, int *iterations_out, int *status, std::vector<std::string> &messages);
void map_fit_batch_stats(long *calls, long *speakers_batched, long *speakers_single, long *speakers_handed_over, long *passes);
void set_map_fit_batch_bytes(long v);
long map_fit_batch_bytes();
// score_norm.hip
void score_norm(int mode, int64_t J, int64_t T, int64_t Cz, int64_t Ct, int top_n, const double *S, const double *Ez, const double *Tt,
                const double *Zt, double *out, int64_t *degenerate);
void score_norm_select(int64_t rows, int64_t C, int top_n, const double *X, int64_t *idx, double *mu, double *sigma);
void set_norm_scratch_mib(long v);
long norm_scratch_mib();
// calib.hip
void calib_train(int S, int64_t n, const double *X, const int8_t *lab, double prior, double ridge, double tol, int max_pass, const double *theta0,
                 int resume, double *state, int64_t *counts);
void calib_eval(int S, int64_t n, const double *X, const int8_t *lab, double prior, double ridge, const double *theta, double *f, double *g,
                double *H, int64_t *counts);
void calib_apply(int S, int64_t n, const double *X, const double *theta, double *out);
void calib_counts(int64_t n, const double *llr, const int8_t *lab, int m, const double *thr, int64_t *miss, int64_t *fa, int64_t *counts);
void set_calib_scratch_mib(long v);
// plda.hip
void plda_train(int64_t n, int R, const double *X, const int64_t *ids, int64_t S, int n_iter, int default_start, double *mu_out, double *Sb,
                double *Sw, int *iterations, int *n_classes, int *stop);
void plda_score(int64_t J, int64_t T, int R, const double *mu, const double *Sb, const double *Sw, const double *E, const int64_t *enrol_n,
                const double *X, double *out, int64_t *bad_classes);
void backend_fit(int kind, int64_t n, int R, const double *X, const int64_t *ids, int64_t S, double *mu_out, double *A);
void backend_apply(int64_t n, int R, const double *X, const double *mu, const double *A, int length_norm, double *Y, int64_t *zero_rows);
void cosine_score(int64_t J, int64_t T, int R, const double *E, const double *X, double *out);
void set_plda_scratch_mib(long v);
// eig.hip, backend_eig.hip
void sym_eig(int R, const double *A, double *w, double *V, int *sweeps, int *converged);
void gen_eig(int R, const double *Sb, const double *Sw, double *psi, double *V, int *sweeps, int *status);
void lda_fit(int64_t n, int R, const double *X, const int64_t *ids, int64_t S, int P, double *mu_out, double *A, double *psi_out);
void backend_project(int64_t n, int R, int P, const double *X, const double *mu, const double *A, int length_norm, double *Y, int64_t *zero_rows);
void plda_score_diag(int64_t J, int64_t T, int R, const double *mu, const double *V, const double *psi, const double *E, const int64_t *enrol_n,
                     const double *X, double *out, int64_t *bad_classes);
// silence.hip
void silence_remove_batch(SRBatch &pcm, double fs, double frame_duration, double frame_shift, double perc, SRBatch &out, int64_t *kept_out);
void set_silence_block(long v);
long silence_block();
// featnorm.hip
void feature_norm_batch(SRBatch &in, int mode, int window, SRBatch &out, int64_t *degenerate_out, int32_t *ranks_out);
void set_feature_norm_tile(long v);
long feature_norm_tile();
}
std::atomic<int> &stream_debug_capture_delay_ms();      // stream.cpp
std::atomic<int> &multi_merge_option();
namespace sr {
int reference_side_effects();
}  // namespace sr

using namespace sr;

// ---- guards: park the message, never unwind into C ----
#define SR_TRY try {                                                     \
    std::lock_guard<std::recursive_mutex> _api_lock(api_mutex());
#define SR_CATCH(ret)                          \
    }                                          \
    catch (const std::exception &e) {          \
        set_error("%s", e.what());             \
        return ret;                            \
    }                                          \
    catch (...) {                              \
        set_error("unknown C++ exception");    \
        return ret;                            \
    }
#define SR_CATCH_VOID                                          \
    }                                                          \
    catch (const std::exception &e) {                          \
        set_error("%s", e.what());                             \
        fprintf(stderr, "pygmm.so: %s\n", e.what());           \
        return;                                                \
    }                                                          \
    catch (...) {                                              \
        set_error("unknown C++ exception");                    \
        return;                                                \
    }

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
static SRModelSet &single_set(GMM *g) { return *sr::single_model_set(g); }

static std::unique_ptr<SRBatch> feature_batch(const float *X, int64_t n, int dim,
                                              const int64_t *offsets, int n_utt) {
    ensure_device();
    if (n < 0 || dim <= 0 || n_utt < 0) fail("bad batch shape");
    auto b = std::make_unique<SRBatch>();
    b->bind_device();
    b->kind = SRBatch::FEATURES;
    b->n_utt = n_utt;
    b->dim = dim;
    b->n_rows = n;
    b->offsets.assign(offsets, offsets + n_utt + 1);
    if (b->offsets.front() != 0 || b->offsets.back() != n) fail("offsets must run from 0 to n");
    for (int u = 0; u < n_utt; u++)
        if (b->offsets[u + 1] < b->offsets[u]) fail("offsets must be non-decreasing");
    b->data.upload(X, (size_t)n * dim);
    b->d_offsets.upload(b->offsets.data(), b->offsets.size());
    sync_stream();
    return b;
}

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

namespace sr {
void score_one_local(GMM *g, const float *X, long n, int dim, float *ll_out, double *sum_out, int flags);
void score_models_local(GMM *const *models, int n_models, const float *X, long n, int dim, double *sums_out, int flags);
}
static std::unique_ptr<SRBatch> feature_batch(const float *X, int64_t n, int dim, const int64_t *offsets, int n_utt);
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

// ======================= Part 2: extensions =======================

const char *sr_last_error(void) { return last_error().c_str(); }

int sr_gpu_runtime_lost(void) { return gpu_runtime_lost() ? 1 : 0; }

int sr_device_count(void) { return visible_devices(); }

// No api lock here: these only move the calling thread between devices.
int sr_set_device(int device) {
    try {
        set_default_device(device);
        return 0;
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return -1;
    }
}

int sr_set_thread_device(int device) {
    try {
        set_thread_device(device);
        return 0;
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return -1;
    }
}

int sr_get_device(void) { return current_device(); }

int sr_device_synchronize(void) {
    SR_TRY
    ensure_device();
    SR_HIP(hipDeviceSynchronize());
    return 0;
    SR_CATCH(-1)
}

int sr_device_name(char *buf, int buflen) {
    SR_TRY
    ensure_device();
    hipDeviceProp_t prop;
    SR_HIP(hipGetDeviceProperties(&prop, ctx().device));
    snprintf(buf, (size_t)buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return 0;
    SR_CATCH(-1)
}

int sr_device_numa_node(int device) {
    try {
        return device_numa_node(device);
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return -1;
    }
}

int sr_bind_thread_near_device(int device) {
    try {
        return bind_thread_near_device(device);
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return -1;
    }
}

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

int sr_score_frames_f32(GMM *gmm, const float *X, long n, int dim, float *ll_out, double *sum_out,
                        int flags) {
    SR_TRY
    if (n > 0 && !X) fail("null X");
    score_one(gmm, X, n, dim, ll_out, sum_out, flags);
    return 0;
    SR_CATCH(-1)
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

static SRBatch *pcm_batch(const void *pcm, bool is_f32, const int64_t *sample_offsets, int n_utt) {
    ensure_device();
    if (n_utt < 0 || !sample_offsets) fail("bad PCM batch arguments");
    auto b = std::make_unique<SRBatch>();
    b->bind_device();
    b->kind = is_f32 ? SRBatch::PCMF32 : SRBatch::PCM16;
    b->n_utt = n_utt;
    b->offsets.assign(sample_offsets, sample_offsets + n_utt + 1);
    if (b->offsets.front() != 0) fail("sample_offsets[0] must be 0");
    for (int u = 0; u < n_utt; u++)
        if (b->offsets[u + 1] < b->offsets[u]) fail("sample_offsets must be non-decreasing");
    b->n_rows = b->offsets.back();
    if (b->n_rows > 0 && !pcm) fail("null PCM pointer");
    if (is_f32)
        b->data.upload(static_cast<const float *>(pcm), (size_t)b->n_rows);
    else
        b->pcm16.upload(static_cast<const int16_t *>(pcm), (size_t)b->n_rows);
    b->d_offsets.upload(b->offsets.data(), b->offsets.size());
    sync_stream();
    return b.release();
}

SRBatch *sr_batch_from_pcm(const int16_t *pcm, const int64_t *sample_offsets, int n_utt) {
    SR_TRY
    return pcm_batch(pcm, false, sample_offsets, n_utt);
    SR_CATCH(nullptr)
}

SRBatch *sr_batch_from_pcm_f32(const float *pcm, const int64_t *sample_offsets, int n_utt) {
    SR_TRY
    return pcm_batch(pcm, true, sample_offsets, n_utt);
    SR_CATCH(nullptr)
}

SRBatch *sr_batch_from_features(const float *X, int64_t n_frames, int dim,
                                const int64_t *frame_offsets, int n_utt) {
    SR_TRY
    if (!frame_offsets) fail("null frame_offsets");
    if (n_frames > 0 && !X) fail("null X");
    return feature_batch(X, n_frames, dim, frame_offsets, n_utt).release();
    SR_CATCH(nullptr)
}

int sr_batch_reset_features(SRBatch *b, const float *X, int64_t n_frames, int dim, const int64_t *frame_offsets, int n_utt) {
    SR_TRY
    if (!b || !frame_offsets) fail("null argument");
    if (b->kind != SRBatch::FEATURES) fail("sr_batch_reset_features needs a feature batch");
    if (n_frames < 0 || dim <= 0 || n_utt < 0) fail("bad batch shape");
    if (frame_offsets[0] != 0 || frame_offsets[n_utt] != n_frames) fail("offsets must run from 0 to n");
    for (int u = 0; u < n_utt; u++)
        if (frame_offsets[u + 1] < frame_offsets[u]) fail("offsets must be non-decreasing");
    if (n_frames > 0 && !X) fail("null X");
    b->bind_device();
    const bool same_layout = b->n_utt == n_utt && b->offsets.size() == (size_t)n_utt + 1 && std::equal(b->offsets.begin(), b->offsets.end(), frame_offsets);
    b->n_utt = n_utt;
    b->dim = dim;
    b->n_rows = n_frames;
    // (device buffers only ever grow.)  A serving-sized refill goes through the batch's page-locked copies and is left in flight: the
    // caller's matrix is its own again when the call returns, whatever is queued next on the stream runs behind the transfer
    const size_t n_val = (size_t)n_frames * dim;
    const bool staged = n_val * sizeof(float) <= ((size_t)4 << 20) && ((size_t)n_utt + 1) * sizeof(int64_t) <= STAGED_TABLE_MAX_BYTES;
    if (!same_layout) {
        b->offsets.assign(frame_offsets, frame_offsets + n_utt + 1);
        b->invalidate_tiles();
        if (staged) b->stage_offsets.send(b->d_offsets, b->offsets.data(), b->offsets.size());
        else b->d_offsets.upload(b->offsets.data(), b->offsets.size());
    }
    if (staged) {
        b->stage_rows.send(b->data, X, n_val);
        return 0;
    }
    b->data.upload(X, n_val);
    sync_stream();
    return 0;
    SR_CATCH(-1)
}

// A serving decision's worth of PCM (<= 4 MB): through the batch's page-locked copy, transfer left in flight (batch.hpp) -- the stream
// synchronisation sr_batch_update_pcm used to end with was a sixth of a single-utterance decision (round 6).  false: too large, the
// caller uploads and waits.
static bool stage_small_pcm(SRBatch *b, const int16_t *pcm, int64_t n_samples) {
    if ((size_t)n_samples * sizeof(int16_t) > ((size_t)4 << 20) || n_samples <= 0) return false;
    if (!b->stage_done.e) SR_HIP(hipEventCreateWithFlags(&b->stage_done.e, hipEventDisableTiming));
    else if (hipEventQuery(b->stage_done.e) != hipSuccess) SR_HIP(hipEventSynchronize(b->stage_done.e));
    if ((size_t)n_samples > b->h_stage.n) b->h_stage.ensure((size_t)n_samples + (size_t)n_samples / 4);   // (headroom: as StagedUpload)
    if ((size_t)n_samples > b->pcm16.n) b->pcm16.ensure((size_t)n_samples + (size_t)n_samples / 4);
    g_devbuf_epoch++;                       // (contents changed: a captured graph that depends on them is re-captured, as upload())
    // more than 1 MB: in pieces of 256 K samples, a piece's DMA under the host's copy of the next one (64 utterances x 3 s:
    // 0.936 -> 0.905 ms per call; a second piece costs a small batch its 5 us)
    const int64_t PIECE = n_samples <= ((int64_t)512 << 10) ? n_samples : ((int64_t)256 << 10);
    for (int64_t at = 0; at < n_samples; at += PIECE) {
        const size_t n = (size_t)std::min<int64_t>(PIECE, n_samples - at);
        std::memcpy(b->h_stage.p + at, pcm + at, n * sizeof(int16_t));
        SR_HIP(hipMemcpyAsync(b->pcm16.p + at, b->h_stage.p + at, n * sizeof(int16_t), hipMemcpyHostToDevice, ctx().stream));
    }
    SR_HIP(hipEventRecord(b->stage_done.e, ctx().stream));
    return true;
}

int sr_batch_update_pcm(SRBatch *b, const int16_t *pcm, int64_t n_samples) {
    SR_TRY
    if (!b || !pcm) fail("null argument");
    if (b->kind != SRBatch::PCM16) fail("sr_batch_update_pcm needs an int16 PCM batch");
    if (n_samples != b->n_rows) fail("sample count %lld does not match the batch (%lld)", (long long)n_samples, (long long)b->n_rows);
    b->bind_device();
    if (stage_small_pcm(b, pcm, n_samples)) return 0;
    b->pcm16.upload(pcm, (size_t)n_samples);
    sync_stream();
    return 0;
    SR_CATCH(-1)
}

int sr_batch_reset_pcm(SRBatch *b, const int16_t *pcm, const int64_t *sample_offsets, int n_utt) {
    SR_TRY
    if (!b || !sample_offsets) fail("null argument");
    if (b->kind != SRBatch::PCM16) fail("sr_batch_reset_pcm needs an int16 PCM batch");
    if (n_utt < 0 || sample_offsets[0] != 0) fail("bad PCM batch arguments");
    for (int u = 0; u < n_utt; u++)
        if (sample_offsets[u + 1] < sample_offsets[u]) fail("sample_offsets must be non-decreasing");
    const int64_t n = sample_offsets[n_utt];
    if (n > 0 && !pcm) fail("null PCM pointer");
    b->bind_device();
    b->n_utt = n_utt;
    b->offsets.assign(sample_offsets, sample_offsets + n_utt + 1);
    b->n_rows = n;
    b->invalidate_tiles();
    // (device buffers only ever grow.)  A decision's worth of samples and their offsets: page-locked copies, left in flight
    if (((size_t)n_utt + 1) * sizeof(int64_t) <= STAGED_TABLE_MAX_BYTES && stage_small_pcm(b, pcm, n)) {
        b->stage_offsets.send(b->d_offsets, b->offsets.data(), b->offsets.size());
        return 0;
    }
    b->pcm16.upload(pcm, (size_t)n);
    b->d_offsets.upload(b->offsets.data(), b->offsets.size());
    sync_stream();
    return 0;
    SR_CATCH(-1)
}

void sr_batch_free(SRBatch *b) { delete b; }
int sr_batch_num_utterances(SRBatch *b) { return b ? b->n_utt : 0; }
int64_t sr_batch_num_rows(SRBatch *b) { return b ? b->n_rows : 0; }
int sr_batch_dim(SRBatch *b) { return (b && b->kind == SRBatch::FEATURES) ? b->dim : 0; }

int sr_batch_offsets(SRBatch *b, int64_t *offsets_out) {
    SR_TRY
    if (!b || !offsets_out) fail("null argument");
    std::memcpy(offsets_out, b->offsets.data(), sizeof(int64_t) * b->offsets.size());
    return 0;
    SR_CATCH(-1)
}

int sr_batch_download(SRBatch *b, float *out) {
    SR_TRY
    if (!b || !out) fail("null argument");
    if (b->kind != SRBatch::FEATURES) fail("only feature batches can be downloaded");
    b->bind_device();
    b->data.download(out, (size_t)b->n_rows * b->dim);
    sync_stream();
    return 0;
    SR_CATCH(-1)
}

int sr_batch_download_pcm16(SRBatch *b, int16_t *out) {
    SR_TRY
    if (!b || (!out && b->n_rows > 0)) fail("null argument");
    if (b->kind != SRBatch::PCM16) fail("only int16 PCM batches can be downloaded as PCM16");
    b->bind_device();
    b->pcm16.download(out, (size_t)b->n_rows);
    sync_stream();
    return 0;
    SR_CATCH(-1)
}

SRBatch *sr_silence_remove_batch(SRBatch *pcm, double fs, double frame_duration, double frame_shift, double perc, int64_t *kept_out) {
    SR_TRY
    if (!pcm) fail("null argument");
    auto out = std::make_unique<SRBatch>();
    silence_remove_batch(*pcm, fs, frame_duration, frame_shift, perc, *out, kept_out);
    return out.release();
    SR_CATCH(nullptr)
}

int sr_silence_plan(double fs, double frame_duration, double frame_shift, int64_t max_samples, int32_t *out, int n_out) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 12) fail("sr_silence_plan writes 12 fields");
    SilencePlan p;
    std::string why;
    if (!plan_silence(fs, frame_duration, frame_shift, max_samples, silence_block(), p, why)) fail("remove_silence: %s", why.c_str());
    const int64_t v[12] = {p.L, p.S, p.g, p.E, p.B, p.blocks_max, p.variant, p.blocks_per_wg, p.list_cap,
                           silence_grid(p.blocks_max, p.blocks_per_wg), p.chunk_lanes, p.max_pos};
    for (int i = 0; i < 12; i++) out[i] = (int32_t)std::min<int64_t>(v[i], INT32_MAX);
    return 12;
    SR_CATCH(-1)
}

// ---- short-time feature normalisation (featnorm.hip).  Every refusal comes before the device is touched. ----

SRBatch *sr_feature_norm_batch(SRBatch *feats, int mode, int window, int64_t *degenerate_out, int32_t *ranks_out) {
    SR_TRY
    if (!feats) fail("null argument");
    auto out = std::make_unique<SRBatch>();
    feature_norm_batch(*feats, mode, window, *out, degenerate_out, ranks_out);
    return out.release();
    SR_CATCH(nullptr)
}

int sr_feature_norm_plan(int mode, int window, int dim, int64_t max_frames, int n_cu, int32_t *out, int n_out) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 12) fail("sr_feature_norm_plan writes 12 fields");
    FeatNormPlan p;
    std::string why;
    if (n_cu > 0) {
        if (!plan_feature_norm(mode, window, true, dim, max_frames, feature_norm_tile(), n_cu, p, why)) fail("sr_feature_norm_plan: %s", why.c_str());
    } else {
        if (!plan_feature_norm(mode, window, true, dim, max_frames, feature_norm_tile(), 1, p, why)) fail("sr_feature_norm_plan: %s", why.c_str());
        ensure_device();
        if (!plan_feature_norm(mode, window, true, dim, max_frames, feature_norm_tile(), ctx().n_cu, p, why)) fail("sr_feature_norm_plan: %s", why.c_str());
    }
    const int64_t v[12] = {p.F, p.span_max, p.stride, p.cols, p.passes, p.lds_bytes, p.tiles_max, featnorm_grid(p.tiles_max, n_cu > 0 ? n_cu : ctx().n_cu),
                           p.table ? 1 : 0, p.table_len, FEATNORM_WG, FEATNORM_MAX_W};
    for (int i = 0; i < 12; i++) out[i] = (int32_t)std::min<int64_t>(v[i], INT32_MAX);
    return 12;
    SR_CATCH(-1)
}

double sr_norm_quantile(double p) { return norm_quantile(p); }

int sr_score_batch_set(SRModelSet *set, SRBatch *features, double *sums_out, int *argmax_out,
                       float *frame_ll_out, int flags) {
    SR_TRY
    if (!set || !features) fail("null argument");
    score_batch_set(*set, *features, sums_out, argmax_out, frame_ll_out, flags);
    return 0;
    SR_CATCH(-1)
}

SRMfcc *sr_mfcc_create(double fs, double win_length_ms, double win_shift_ms, int fft_size,
                       int n_filters, int n_ceps, double pre_emphasis) {
    SR_TRY
    return new SRMfcc(fs, win_length_ms, win_shift_ms, fft_size, n_filters, n_ceps, pre_emphasis);
    SR_CATCH(nullptr)
}

int sr_mfcc_set_lpc(SRMfcc *m, int n_lpc) {
    SR_TRY
    if (!m) fail("null extractor");
    if (n_lpc != 0 && n_lpc != 10 && n_lpc != 12 && n_lpc != 15 && n_lpc != 16 && n_lpc != 20)
        fail("LPC order %d is not instantiated (10, 12, 15, 16, 20; 0 = off)", n_lpc);
    m->n_lpc = n_lpc;
    return 0;
    SR_CATCH(-1)
}

void sr_mfcc_free(SRMfcc *m) { delete m; }
int sr_mfcc_frame_len(SRMfcc *m) { return m ? m->frame_len : 0; }
int sr_mfcc_frame_shift(SRMfcc *m) { return m ? m->frame_shift : 0; }
int64_t sr_mfcc_num_frames(SRMfcc *m, int64_t n_samples) { return m ? mfcc_num_frames(*m, n_samples) : 0; }

int sr_mfcc_tables(SRMfcc *m, double *window, double *melbank, double *dct) {
    SR_TRY
    if (!m) fail("null extractor");
    if (window) std::memcpy(window, m->window.data(), sizeof(double) * m->window.size());
    if (melbank) std::memcpy(melbank, m->melbank.data(), sizeof(double) * m->melbank.size());
    if (dct) std::memcpy(dct, m->dct.data(), sizeof(double) * m->dct.size());
    return 0;
    SR_CATCH(-1)
}

int sr_mfcc_plan(SRMfcc *m, int precision, int generic, int pcm_kind, int64_t n_frames, int n_cu, int32_t *out, int n_out) {
    SR_TRY
    if (!m || !out) fail("null argument");
    if (precision != 0 && precision != 2) fail("mfcc_precision must be 0 or 2");
    if (pcm_kind != 0 && pcm_kind != 1) fail("PCM kind: 0 = int16, 1 = float32");      // (selects the PcmT instance only: no decision hangs on it)
    if (n_out < 16) fail("sr_mfcc_plan writes 16 fields");
    if (n_cu <= 0) {
        ensure_device();
        n_cu = ctx().n_cu;
    }
    const MelLayout mel = mel_layout(*m);
    const MfccPlan p = plan_mfcc(*m, mel, precision, generic != 0, n_frames, n_cu);
    const int32_t v[16] = {p.kernel, p.n1, p.nz1, p.preset, p.wpb, (int32_t)p.lds, (int32_t)std::min<int64_t>(p.frames_per_wave, INT32_MAX), p.grid, p.cp,
                           mel.pad_floats, mel.pass_len[0], mel.pass_len[1], mel.pass_len[2], mel.pass_len[3], mel.max_read, mel.n_empty};
    std::memcpy(out, v, sizeof v);
    return 16;
    SR_CATCH(-1)
}

SRBatch *sr_mfcc_extract_batch(SRMfcc *m, SRBatch *pcm, int nd, int cmvn) {
    SR_TRY
    if (!m || !pcm) fail("null argument");
    auto out = std::make_unique<SRBatch>();
    mfcc_extract_batch(*m, *pcm, nd, cmvn, *out);
    return out.release();
    SR_CATCH(nullptr)
}

// The fused serving step: PCM batch -> MFCC -> CMVN / deltas -> all models -> sums + argmax on the host, one pass.
// (Rounds 1-3 carried an option that cut the batch into chunks and ran the feature kernels of chunk i + 1 on a second stream under the
// scoring of chunk i.  It measured slower on every workload -- configs[1] 5.12 ms in one pass against 5.17 / 5.43 / 5.87 ms with 2 / 4 /
// 8 chunks, configs[2] 337 against 350 ms and later 267 against 538: next to the power-capped scoring kernel the feature launches stretch
// from 20 to 271 ms and the scoring chunks pay their tails, profiles/r02_overlap.txt -- and its second stream did not wait for the
// uploads of sr_multi_predict_pcm's pieces.  Removed in round 4.)
static void predict_unpipelined(SRMfcc *m, SRModelSet *set, SRBatch *pcm, int nd, double *sums_out, int *argmax_out,
                                int flags, const OpenSetFetch *open) {
    SRBatch *feat_ws = &per_device<SRBatch>();   // reused across steps: the serving loop allocates nothing
    mfcc_extract_batch(*m, *pcm, nd, 1, *feat_ws);
    if (open) {      // the decision kernel reads the device's sums: no delivery by finalize itself (open_set.hip)
        score_resolved(*set, *feat_ws, false, flags, 0, sums_out, argmax_out, nullptr, open);
        return;
    }
    // (small result sets land in host memory by themselves: SCORE_HOST_DELIVER, score.hpp)
    const int deliver = (sums_out && argmax_out && host_deliverable((size_t)pcm->n_utt, (size_t)set->host.n_models)) ? SCORE_HOST_DELIVER : 0;
    score_resolved(*set, *feat_ws, false, flags, deliver, sums_out, argmax_out, nullptr);
}

}  // extern "C"

namespace sr {
void predict_pcm(SRMfcc *m, SRModelSet *set, SRBatch *pcm, int nd, double *sums_out, int *argmax_out, int flags,
                 const OpenSetFetch *open) {
    if (!m || !set || !pcm) fail("null argument");
    ensure_device();
    predict_unpipelined(m, set, pcm, nd, sums_out, argmax_out, flags, open);
}
}  // namespace sr

extern "C" {

int sr_predict_pcm_batch(SRMfcc *m, SRModelSet *set, SRBatch *pcm, int nd, double *sums_out,
                         int *argmax_out, int flags) {
    SR_TRY
    predict_pcm(m, set, pcm, nd, sums_out, argmax_out, flags, nullptr);
    return 0;
    SR_CATCH(-1)
}

// ---- the open-set decision (open_set.hip).  Every argument is checked before the device is touched. ----

int sr_open_set_decide(const double *sums, int U, int S, int bg, const int64_t *n_frames, double threshold, int *label_out,
                       double *margin_out) {
    SR_TRY
    if (U < 0 || S <= 0) fail("sr_open_set_decide: bad shape (%d utterances x %d models)", U, S);
    if (!label_out || !margin_out) fail("sr_open_set_decide: null output (labels and margins are both required)");
    if (U > 0 && (!sums || !n_frames)) fail("sr_open_set_decide: null argument");
    const OpenSetRule rule{bg, threshold};
    open_set_check(rule, S);
    for (int u = 0; u < U; u++)
        if (n_frames[u] < 0) fail("sr_open_set_decide: utterance %d has a negative frame count", u);
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_open_set_decide");
    open_set_decide_host(sums, U, S, rule, n_frames, label_out, margin_out);
    return 0;
    SR_CATCH(-1)
}

int sr_score_batch_set_open(SRModelSet *set, SRBatch *features, int bg, double threshold, double *sums_out, int *label_out,
                            double *margin_out, int flags) {
    SR_TRY
    if (!set || !features) fail("sr_score_batch_set_open: null argument");
    if (!label_out || !margin_out) fail("sr_score_batch_set_open: null output (labels and margins are both required)");
    const OpenSetFetch open{{bg, threshold}, label_out, margin_out};
    open_set_check(open.rule, set->host.n_models);
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_score_batch_set_open");
    score_batch_set_open(*set, *features, sums_out, open, flags);
    return 0;
    SR_CATCH(-1)
}

int sr_predict_pcm_batch_open(SRMfcc *m, SRModelSet *set, SRBatch *pcm, int nd, int bg, double threshold, double *sums_out,
                              int *label_out, double *margin_out, int flags) {
    SR_TRY
    if (!m || !set || !pcm) fail("sr_predict_pcm_batch_open: null argument");
    if (!label_out || !margin_out) fail("sr_predict_pcm_batch_open: null output (labels and margins are both required)");
    const OpenSetFetch open{{bg, threshold}, label_out, margin_out};
    open_set_check(open.rule, set->host.n_models);
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_predict_pcm_batch_open");
    predict_pcm(m, set, pcm, nd, sums_out, nullptr, flags, &open);
    return 0;
    SR_CATCH(-1)
}

// ---- top-C Gaussian selection (gmm_topc.hip).  Every refusal comes before the device is touched. ----

int sr_score_batch_set_topc(SRModelSet *set, SRBatch *features, int bg, int top_c, double *sums_out, int *argmax_out, int *topc_out,
                            float *frame_ll_out, int flags) {
    SR_TRY
    if (!set || !features) fail("sr_score_batch_set_topc: null argument");
    score_batch_set_topc(*set, *features, bg, top_c, sums_out, argmax_out, topc_out, frame_ll_out, flags);
    return 0;
    SR_CATCH(-1)
}

int sr_predict_pcm_batch_topc(SRMfcc *m, SRModelSet *set, SRBatch *pcm, int nd, int bg, int top_c, double *sums_out, int *argmax_out,
                              int flags) {
    SR_TRY
    if (!m || !set || !pcm) fail("sr_predict_pcm_batch_topc: null argument");
    if (pcm->kind == SRBatch::FEATURES) fail("sr_predict_pcm_batch_topc takes a PCM batch; score a feature batch with sr_score_batch_set_topc");
    {   // the set's and the rule's refusals before the feature stage runs (the batch is PCM here: that check is the other entry point's)
        const int K = set->host.model_mixtures.empty() ? 0 : set->host.model_mixtures[0];
        std::string why;
        if (!topc_check(topc_set_tied(*set), set->host.n_models, K, set->host.dim, bg, top_c, true, why)) fail("%s", why.c_str());
    }
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_predict_pcm_batch_topc");
    ensure_device();
    SRBatch *feat_ws = &per_device<SRBatch>();   // the fused calls' feature workspace: nothing leaves the device
    mfcc_extract_batch(*m, *pcm, nd, 1, *feat_ws);
    score_batch_set_topc(*set, *feat_ws, bg, top_c, sums_out, argmax_out, nullptr, nullptr, flags);
    return 0;
    SR_CATCH(-1)
}

int sr_topc_plan(int K, int D, int S, int top_c, int64_t n_frames, int64_t scratch_bytes, int n_cu, int32_t *out, int n_out) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 16) fail("sr_topc_plan writes 16 fields");
    if (n_cu <= 0) {
        ensure_device();
        n_cu = ctx().n_cu;
    }
    TopcPlan p;
    std::string why;
    if (!plan_topc(K, D, S, top_c, n_frames, scratch_bytes, n_cu, p, why)) fail("%s", why.c_str());
    const int64_t v[16] = {p.tp, p.cr, p.row_bytes, p.chunk, p.n_chunks, p.run, TOPC_STAGE, p.eval_waves, p.eval_grid_x, p.eval_grid_y,
                           p.select_grid, p.route_grid, p.combine_wg, TOPC_TILE, p.rank_lds, 0};
    for (int i = 0; i < 16; i++) out[i] = (int32_t)std::min<int64_t>(v[i], INT32_MAX);
    return 16;
    SR_CATCH(-1)
}

// ---- batched Baum-Welch statistics (bw_stats.hip).  Every refusal comes before the device is touched. ----

int sr_bw_stats_batch(SRModelSet *set, int model, SRBatch *feats, double *N, double *F, double *ll, int64_t *dropped) {
    SR_TRY
    if (!set || !feats) fail("sr_bw_stats_batch: null argument");
    bw_stats_batch(*set, model, *feats, N, F, ll, dropped);
    return 0;
    SR_CATCH(-1)
}

SRStats *sr_bw_stats_resident(SRModelSet *set, int model, SRBatch *feats, double *ll, int64_t *dropped) {
    SR_TRY
    if (!set || !feats) fail("sr_bw_stats_resident: null argument");
    return bw_stats_resident(*set, model, *feats, ll, dropped);
    SR_CATCH(nullptr)
}

// ---- statistics handles (jfa_stats.hip) ----

SRStats *sr_stats_from_host(int64_t n, int K, int D, const double *N, const double *F) {
    SR_TRY
    return stats_from_host(n, K, D, N, F);
    SR_CATCH(nullptr)
}

int sr_stats_info(const SRStats *s, int64_t *out, int n_out) {
    SR_TRY
    stats_info(s, out, n_out);
    return 4;
    SR_CATCH(-1)
}

int sr_stats_get(const SRStats *s, double *N, double *F) {
    SR_TRY
    stats_get(s, N, F);
    return 0;
    SR_CATCH(-1)
}

SRStats *sr_stats_take(const SRStats *s, const int64_t *rows, int64_t n_rows) {
    SR_TRY
    return stats_take(s, rows, n_rows);
    SR_CATCH(nullptr)
}

void sr_stats_close(SRStats *s) {
    SR_TRY
    stats_close(s);
    SR_CATCH_VOID
}

int sr_bw_plan(int S, int model, int K, int D, int batch_is_features, int feat_dim, const int64_t *lengths, int64_t n_utt,
               int64_t range_frames, int64_t scratch_bytes, int n_cu, int64_t *ranges_out, int64_t range_cap, int64_t *out, int n_out) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 12) fail("sr_bw_plan writes 12 fields");
    std::string why;
    if (!bw_check(batch_is_features != 0, S, model, K, D, feat_dim, why)) fail("%s", why.c_str());
    if (n_cu <= 0) {
        ensure_device();
        n_cu = ctx().n_cu;
    }
    BwPlan p;
    if (!plan_bw(K, D, lengths, n_utt, range_frames, scratch_bytes, n_cu, p, why)) fail("%s", why.c_str());
    const int64_t n = (int64_t)p.ranges.size();
    const int64_t v[12] = {p.dp, p.ncb, p.n_mix_blocks, p.slab_bytes, n, p.group_ranges, p.n_groups, p.lse_grid, p.stats_lds,
                           p.reduce_blocks, p.stats_rounds, bw_range_rows(0, K, D, range_frames)};
    std::memcpy(out, v, sizeof v);
    if (ranges_out)
        for (int64_t i = 0; i < std::min(n, range_cap); i++) {
            ranges_out[3 * i] = p.ranges[i].utt;
            ranges_out[3 * i + 1] = p.ranges[i].first;
            ranges_out[3 * i + 2] = p.ranges[i].rows;
        }
    return 12;
    SR_CATCH(-1)
}

// ---- a set of speakers MAP-adapted from one UBM in one batched fit (map_batch.hip).  Every refusal comes before the device is touched. ----
namespace {
thread_local std::vector<std::string> g_map_batch_messages;      // of the calling thread's last sr_map_fit_batch
}  // namespace

int sr_map_fit_batch(GMM *const *models, int S, GMM *ubm, const float *X, const int64_t *row_offsets, int dim, const struct Parameter *param,
                     long seed, int *iterations_out, int *status) {
    SR_TRY
    g_map_batch_messages.clear();
    if (!models || !ubm || !X || !row_offsets || !param || !iterations_out || !status) fail("sr_map_fit_batch: null argument");
    if (S < 1) fail("sr_map_fit_batch: at least one speaker is needed (got %d)", S);
    if (row_offsets[0] != 0) fail("sr_map_fit_batch: row_offsets must start at 0 (got %lld)", (long long)row_offsets[0]);
    for (int s = 0; s < S; s++)
        if (row_offsets[s + 1] < row_offsets[s]) fail("sr_map_fit_batch: row_offsets must not decrease (speaker %d)", s);
    if (!ubm->trained()) fail("UBM has no parameters");
    if (ubm->dim != dim) fail("UBM dim %d != data dim %d", ubm->dim, dim);
    {
        std::vector<const GMM *> seen(models, models + S);
        for (int s = 0; s < S; s++) {
            if (!seen[(size_t)s]) fail("sr_map_fit_batch: null GMM handle (speaker %d)", s);
            if (seen[(size_t)s] == ubm) fail("sr_map_fit_batch: speaker %d's handle is the UBM's", s);
        }
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) fail("sr_map_fit_batch: the same handle is given twice");
    }
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_map_fit_batch");
    return map_fit_batch(models, S, ubm, X, row_offsets, dim, *param, seed, iterations_out, status, g_map_batch_messages);
    SR_CATCH(-1)
}

const char *sr_map_fit_batch_error(int s) {
    const auto &m = g_map_batch_messages;
    return s >= 0 && (size_t)s < m.size() ? m[(size_t)s].c_str() : "";
}

void sr_map_fit_batch_stats(long *calls, long *speakers_batched, long *speakers_single, long *speakers_handed_over, long *passes) {
    map_fit_batch_stats(calls, speakers_batched, speakers_single, speakers_handed_over, passes);
}

long sr_map_fit_batch_bytes(void) { return map_fit_batch_bytes(); }

int sr_map_fit_plan(int K, int D, const int64_t *lengths, int S, const struct Parameter *param, int64_t scratch_bytes, int n_cu,
                    int64_t *speakers_out, int64_t *groups_out, int64_t group_cap, int64_t *tiles_out, int64_t tile_cap,
                    int64_t *chunks_out, int64_t chunk_cap, int64_t *out, int n_out) {
    SR_TRY
    if (!out || !param) fail("null argument");
    if (n_out < 12) fail("sr_map_fit_plan writes 12 fields");
    if (n_cu <= 0) {
        ensure_device();
        n_cu = ctx().n_cu;
    }
    MapPlan p;
    std::string why;
    if (!plan_map_batch(K, D, lengths, S, *param, scratch_bytes, n_cu, p, why)) fail("%s", why.c_str());
    const int64_t v[12] = {(int64_t)p.batched.size(), p.n_single, p.n_error, (int64_t)p.groups.size(), (int64_t)p.tiles.size(),
                           (int64_t)p.chunks.size(), p.n_kb, (int64_t)p.lds_density, (int64_t)p.lds_stats, p.max_group_bytes, p.waves,
                           MAP_STATE};
    std::memcpy(out, v, sizeof v);
    if (speakers_out)
        for (int s = 0; s < S; s++) {
            const MapSpeakerPlan &sp = p.speakers[(size_t)s];
            const int64_t r[6] = {sp.route, sp.group, sp.slot, sp.n_pad, sp.n_chunks, sp.scratch_bytes};
            std::memcpy(speakers_out + 6 * (size_t)s, r, sizeof r);
        }
    if (groups_out)
        for (int64_t g = 0; g < std::min<int64_t>((int64_t)p.groups.size(), group_cap); g++) {
            const MapGroupPlan &gp = p.groups[(size_t)g];
            const int64_t r[6] = {p.batched[(size_t)gp.first], gp.count, gp.n_tiles, gp.n_chunks, gp.scratch_bytes, gp.tile0};
            std::memcpy(groups_out + 6 * g, r, sizeof r);
        }
    for (int which = 0; which < 2; which++) {
        const std::vector<MapTileRow> &rows = which ? p.chunks : p.tiles;
        int64_t *dst = which ? chunks_out : tiles_out;
        const int64_t cap = which ? chunk_cap : tile_cap;
        if (!dst) continue;
        for (int64_t i = 0; i < std::min<int64_t>((int64_t)rows.size(), cap); i++) {
            dst[3 * i] = rows[(size_t)i].speaker;
            dst[3 * i + 1] = rows[(size_t)i].first;
            dst[3 * i + 2] = rows[(size_t)i].local;
        }
    }
    return 12;
    SR_CATCH(-1)
}

// ---- JFA factor estimation (jfa.hip).  Every refusal comes before the device is touched. ----

SRJfa *sr_jfa_open(int64_t G, int K, int D, const double *N, const double *Fc, const double *E) {
    SR_TRY
    return jfa_open(G, K, D, N, Fc, E);
    SR_CATCH(nullptr)
}

int sr_jfa_factors(SRJfa *h, const double *W, int R, double *y, double *A, double *C, int64_t *bad_groups) {
    SR_TRY
    if (!h) fail("sr_jfa_factors: null argument");
    jfa_factors(*h, W, R, y, A, C, bad_groups);
    return 0;
    SR_CATCH(-1)
}

int sr_jfa_update(int K, int D, int R, const double *A, const double *C, double *W, int64_t *skipped) {
    SR_TRY
    jfa_update(K, D, R, A, C, W, skipped);
    return 0;
    SR_CATCH(-1)
}

int sr_jfa_train(SRJfa *h, double *W, int R, int n_iter, double *y, int64_t *skipped) {
    SR_TRY
    if (!h) fail("sr_jfa_train: null argument");
    jfa_train(*h, W, R, n_iter, y, skipped);
    return 0;
    SR_CATCH(-1)
}

void sr_jfa_close(SRJfa *h) {
    SR_TRY
    jfa_close(h);
    SR_CATCH_VOID
}

int sr_jfa_plan(int64_t G, int K, int D, int R, int64_t scratch_bytes, int lds_rows, int n_cu, int64_t *out, int n_out) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 32) fail("sr_jfa_plan writes 32 fields");
    std::string why;
    JfaPlan p;
    if (n_cu > 0) {
        if (!plan_jfa(G, K, D, R, scratch_bytes, lds_rows, n_cu, p, why)) fail("%s", why.c_str());
    } else {
        if (!plan_jfa(G, K, D, R, scratch_bytes, lds_rows, 1, p, why)) fail("%s", why.c_str());      // the refusals first
        ensure_device();
        if (!plan_jfa(G, K, D, R, scratch_bytes, lds_rows, ctx().n_cu, p, why)) fail("%s", why.c_str());
    }
    const int64_t v[32] = {p.chunk, p.n_chunks, p.bytes_N, p.bytes_Fc, p.bytes_E, p.bytes_P, p.bytes_A, p.bytes_C, p.bytes_W, p.bytes_y,
                           p.bytes_scratch, p.path, p.lds_rows, p.gram.x, p.gram.y, p.gemm_L.x, p.gemm_L.y, p.gemm_b.x, p.gemm_b.y,
                           p.gemm_A.x, p.gemm_A.y, p.gemm_C.x, p.gemm_C.y, p.gram_lds, p.gemm_lds, p.factor_lds, p.update_lds,
                           p.factor_rounds, JFA_KSTEP, JFA_MAX_R, JFA_LDS_MAX_R, 0};
    std::memcpy(out, v, sizeof v);
    return 32;
    SR_CATCH(-1)
}

// ---- grouping and centring on the device, the z / d iteration (jfa_stats.hip) ----

SRJfa *sr_jfa_open_centred(const SRStats *s, const double *E, const double *m, int mode, const int64_t *ids, int64_t n_labels, const double *d,
                           const double *z, const double *v, int Ry, const double *y, const double *u, int Ru, const double *x) {
    SR_TRY
    return jfa_open_centred(s, E, m, mode, ids, n_labels, d, z, v, Ry, y, u, Ru, x);
    SR_CATCH(nullptr)
}

int sr_jfa_statistics(SRJfa *h, double *N, double *Fc) {
    SR_TRY
    if (!h) fail("sr_jfa_statistics: null argument");
    jfa_statistics(*h, N, Fc);
    return 0;
    SR_CATCH(-1)
}

int sr_jfa_zd(SRJfa *h, double *d, int n_iter, double *z, double *a, double *b) {
    SR_TRY
    if (!h) fail("sr_jfa_zd: null argument");
    jfa_zd(*h, d, n_iter, z, a, b);
    return 0;
    SR_CATCH(-1)
}

int sr_jfa_centre_plan(int64_t n, int64_t n_labels, int K, int D, int Ry, int Ru, int mode, int64_t scratch_bytes, int64_t *out, int n_out) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 16) fail("sr_jfa_centre_plan writes 16 fields");
    std::string why;
    JfaCentrePlan p;
    if (!plan_jfa_centre(n, n_labels, K, D, Ry, Ru, mode, scratch_bytes, p, why)) fail("%s", why.c_str());
    const int64_t v[16] = {p.mode, p.chunk, p.n_chunks, p.bytes_scratch, p.bytes_N, p.bytes_Fc, p.bytes_yv, p.bytes_z, p.vec, p.gemm_xu.x,
                           p.gemm_xu.y, p.gemm_yv.x, p.gemm_yv.y, p.centre.x, p.centre.y, JFA_TILE};
    std::memcpy(out, v, sizeof v);
    return 16;
    SR_CATCH(-1)
}

// ---- JFA trial scoring (jfa_score.hip) ----

int sr_jfa_score_integrated_stats(const SRStats *tst, int64_t J, int Ry, int Ru, const double *m, const double *E, const double *d, const double *v,
                                  const double *u, const double *z, const double *y, const unsigned char *mask, int64_t mask_rows, int64_t mask_cols,
                                  double *out, int64_t *empty_segments, int64_t *bad_segments) {
    SR_TRY
    jfa_score_stats(JFA_SCORE_INTEGRATED, tst, J, Ry, Ru, m, E, d, v, u, z, y, nullptr, mask, mask_rows, mask_cols, out, empty_segments, bad_segments);
    return 0;
    SR_CATCH(-1)
}

int sr_jfa_score_linear_stats(const SRStats *tst, int64_t J, int Ry, int Ru, const double *m, const double *E, const double *d, const double *v,
                              const double *u, const double *z, const double *y, const double *x, const unsigned char *mask, int64_t mask_rows,
                              int64_t mask_cols, double *out, int64_t *empty_segments) {
    SR_TRY
    jfa_score_stats(JFA_SCORE_LINEAR, tst, J, Ry, Ru, m, E, d, v, u, z, y, x, mask, mask_rows, mask_cols, out, empty_segments, nullptr);
    return 0;
    SR_CATCH(-1)
}

int sr_jfa_score_integrated(int64_t T, int64_t J, int K, int D, int Ry, int Ru, const double *N, const double *F, const double *m, const double *E,
                            const double *d, const double *v, const double *u, const double *z, const double *y, const unsigned char *mask,
                            int64_t mask_rows, int64_t mask_cols, double *out, int64_t *empty_segments, int64_t *bad_segments) {
    SR_TRY
    jfa_score(JFA_SCORE_INTEGRATED, T, J, K, D, Ry, Ru, N, F, m, E, d, v, u, z, y, nullptr, mask, mask_rows, mask_cols, out, empty_segments, bad_segments);
    return 0;
    SR_CATCH(-1)
}

int sr_jfa_score_linear(int64_t T, int64_t J, int K, int D, int Ry, int Ru, const double *N, const double *F, const double *m, const double *E,
                        const double *d, const double *v, const double *u, const double *z, const double *y, const double *x,
                        const unsigned char *mask, int64_t mask_rows, int64_t mask_cols, double *out, int64_t *empty_segments) {
    SR_TRY
    jfa_score(JFA_SCORE_LINEAR, T, J, K, D, Ry, Ru, N, F, m, E, d, v, u, z, y, x, mask, mask_rows, mask_cols, out, empty_segments, nullptr);
    return 0;
    SR_CATCH(-1)
}

int sr_jfa_score_plan(int64_t T, int64_t J, int K, int D, int Ry, int Ru, int mode, int64_t scratch_bytes, int lds_rows, int n_cu, int64_t *out,
                      int n_out) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 56) fail("sr_jfa_score_plan writes 56 fields");
    std::string why;
    JfaScorePlan p;
    if (n_cu > 0) {
        if (!plan_jfa_score(T, J, K, D, Ry, Ru, mode, scratch_bytes, lds_rows, n_cu, p, why)) fail("%s", why.c_str());
    } else {
        if (!plan_jfa_score(T, J, K, D, Ry, Ru, mode, scratch_bytes, lds_rows, 1, p, why)) fail("%s", why.c_str());      // the refusals first
        ensure_device();
        if (!plan_jfa_score(T, J, K, D, Ry, Ru, mode, scratch_bytes, lds_rows, ctx().n_cu, p, why)) fail("%s", why.c_str());
    }
    const int64_t v[56] = {p.mode, p.chunk, p.n_chunks, p.seg_bytes, p.bytes_scratch, p.bytes_M, p.bytes_ME, p.bytes_uE, p.bytes_P, p.bytes_q,
                           p.bytes_G, p.bytes_N, p.bytes_F, p.bytes_lin, p.bytes_quad, p.bytes_a, p.bytes_out, p.bytes_comp, p.path, p.lds_rows,
                           p.gemm_yv.x, p.gemm_yv.y, p.synth.x, p.scale_M.x, p.scale_u.x, p.gram.x, p.gram.y, p.cross.x, p.cross.y, p.cross_z,
                           p.gemm_L.x, p.gemm_L.y, p.gemm_a.x, p.gemm_a.y, p.gemm_lin.x, p.gemm_lin.y, p.gemm_quad.x, p.gemm_quad.y, p.gemm_h.x,
                           p.gemm_h.y, p.kscore.x, p.gemm_xu.x, p.gemm_xu.y, p.comp.x, p.gemm_out.x, p.gemm_out.y, p.gram_lds, p.gemm_lds,
                           p.cross_lds, p.kscore_lds, p.kscore_rounds, JFA_MAX_R, JFA_LDS_MAX_R, JFA_SCORE_MAX_J, 0, 0};
    std::memcpy(out, v, sizeof v);
    return 56;
    SR_CATCH(-1)
}

// ---- score normalisation (score_norm.hip).  Every refusal comes before the device is touched. ----

int sr_score_norm(int mode, int64_t J, int64_t T, int64_t Cz, int64_t Ct, int top_n, const double *S, const double *Ez, const double *Tt,
                  const double *Zt, double *out, int64_t *degenerate) {
    SR_TRY
    score_norm(mode, J, T, Cz, Ct, top_n, S, Ez, Tt, Zt, out, degenerate);
    return 0;
    SR_CATCH(-1)
}

int sr_score_norm_select(int64_t rows, int64_t C, int top_n, const double *X, int64_t *idx, double *mu, double *sigma) {
    SR_TRY
    score_norm_select(rows, C, top_n, X, idx, mu, sigma);
    return 0;
    SR_CATCH(-1)
}

int sr_score_norm_plan(int mode, int64_t J, int64_t T, int64_t Cz, int64_t Ct, int top_n, int64_t scratch_bytes, int n_cu, int64_t *out,
                       int n_out) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 40) fail("sr_score_norm_plan writes 40 fields");
    std::string why;
    NormPlan p;
    if (n_cu > 0) {
        if (!plan_score_norm(mode, J, T, Cz, Ct, top_n, scratch_bytes, n_cu, p, why)) fail("%s", why.c_str());
    } else {
        if (!plan_score_norm(mode, J, T, Cz, Ct, top_n, scratch_bytes, 1, p, why)) fail("%s", why.c_str());      // the refusals first
        ensure_device();
        if (!plan_score_norm(mode, J, T, Cz, Ct, top_n, scratch_bytes, ctx().n_cu, p, why)) fail("%s", why.c_str());
    }
    const int64_t v[40] = {p.mode, p.n_sel, p.n_sel_test, p.chunk, p.n_chunks, p.fixed_bytes, p.seg_bytes, p.bytes_scratch, p.bytes_S, p.bytes_Ez,
                           p.bytes_Tt, p.bytes_Zt, p.bytes_out, p.bytes_moments, p.bytes_tnorm, p.bytes_counts, p.select_enrol.x, p.select_test.x,
                           p.select_zt.x, p.select_lds_enrol, p.select_lds_test, p.shift_enrol.x, p.shift_test.x, p.gemm_enrol.x, p.gemm_enrol.y,
                           p.gemm_test.x, p.gemm_test.y, p.gemm_lds, p.apply.x, p.apply.y, p.select_rounds, NORM_MAX_C, NORM_MAX_ROWS, NORM_WG,
                           0, 0, 0, 0, 0, 0};
    std::memcpy(out, v, sizeof v);
    return 40;
    SR_CATCH(-1)
}

// ---- score calibration and fusion (calib.hip).  Every refusal comes before the device is touched. ----

int sr_calib_train(int S, int64_t n, const double *X, const int8_t *lab, double prior, double ridge, double tol, int max_pass, const double *theta0,
                   int resume, double *state, int64_t *counts) {
    SR_TRY
    calib_train(S, n, X, lab, prior, ridge, tol, max_pass, theta0, resume, state, counts);
    return 0;
    SR_CATCH(-1)
}

int sr_calib_eval(int S, int64_t n, const double *X, const int8_t *lab, double prior, double ridge, const double *theta, double *f, double *g,
                  double *H, int64_t *counts) {
    SR_TRY
    calib_eval(S, n, X, lab, prior, ridge, theta, f, g, H, counts);
    return 0;
    SR_CATCH(-1)
}

int sr_calib_apply(int S, int64_t n, const double *X, const double *theta, double *out) {
    SR_TRY
    calib_apply(S, n, X, theta, out);
    return 0;
    SR_CATCH(-1)
}

int sr_calib_counts(int64_t n, const double *llr, const int8_t *lab, int m, const double *thr, int64_t *miss, int64_t *fa, int64_t *counts) {
    SR_TRY
    calib_counts(n, llr, lab, m, thr, miss, fa, counts);
    return 0;
    SR_CATCH(-1)
}

int sr_calib_plan(int S, int64_t n, int n_thr, int call, int64_t scratch_bytes, int n_cu, int64_t *out, int n_out) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 28) fail("sr_calib_plan writes 28 fields");
    if (call < 0 || call > 2) fail("sr_calib_plan: call is 0 (train / eval), 1 (apply) or 2 (counts)");
    std::string why;
    CalibPlan p;
    if (!plan_calib(S, n, n_thr, scratch_bytes, n_cu > 0 ? n_cu : 1, p, why)) fail("%s", why.c_str());          // the refusals first
    if (scratch_bytes > 0 && !calib_check_bound(p, call == 1 ? "apply" : call == 2 ? "counts" : "train", scratch_bytes, why)) fail("%s", why.c_str());
    if (n_cu <= 0) {
        ensure_device();
        if (!plan_calib(S, n, n_thr, scratch_bytes, ctx().n_cu, p, why)) fail("%s", why.c_str());
    }
    const int64_t v[28] = {p.S, p.n, p.n_blocks, p.acc, p.state_len, p.bytes_X, p.bytes_lab, p.bytes_partial, p.bytes_state, p.bytes_out,
                           p.bytes_thr, p.bytes_counts, p.resident_train, p.resident_apply, p.resident_counts, p.pass_grid, p.step_grid,
                           p.apply_grid, p.counts_grid, p.pass_rounds, CALIB_MAX_S, CALIB_MAX_THR, CALIB_BLOCK, CALIB_WG,
                           CALIB_CADENCE, CALIB_MAX_PASS, CALIB_MAX_N, 0};
    std::memcpy(out, v, sizeof v);
    return 28;
    SR_CATCH(-1)
}

// ---- the i-vector back end (plda.hip).  Every refusal comes before the device is touched. ----

int sr_backend_fit(int kind, int64_t n, int R, const double *X, const int64_t *ids, int64_t n_labels, double *mu, double *A) {
    SR_TRY
    backend_fit(kind, n, R, X, ids, n_labels, mu, A);
    return 0;
    SR_CATCH(-1)
}

int sr_backend_apply(int64_t n, int R, const double *X, const double *mu, const double *A, int length_norm, double *Y, int64_t *zero_rows) {
    SR_TRY
    backend_apply(n, R, X, mu, A, length_norm, Y, zero_rows);
    return 0;
    SR_CATCH(-1)
}

int sr_cosine_score(int64_t J, int64_t T, int R, const double *E, const double *X, double *out) {
    SR_TRY
    cosine_score(J, T, R, E, X, out);
    return 0;
    SR_CATCH(-1)
}

int sr_plda_train(int64_t n, int R, const double *X, const int64_t *ids, int64_t n_labels, int n_iter, int default_start, double *mu, double *Sb,
                  double *Sw, int *iterations, int *n_classes, int *stop) {
    SR_TRY
    plda_train(n, R, X, ids, n_labels, n_iter, default_start, mu, Sb, Sw, iterations, n_classes, stop);
    return 0;
    SR_CATCH(-1)
}

int sr_plda_score(int64_t J, int64_t T, int R, const double *mu, const double *Sb, const double *Sw, const double *E, const int64_t *enrol_n,
                  const double *X, double *out, int64_t *bad_classes) {
    SR_TRY
    plda_score(J, T, R, mu, Sb, Sw, E, enrol_n, X, out, bad_classes);
    return 0;
    SR_CATCH(-1)
}

int sr_plda_plan(int kind, int R, int64_t rows, int64_t groups, int64_t T, const int64_t *counts, int64_t scratch_bytes, int lds_rows, int n_cu,
                 int64_t *out, int n_out, int64_t *perm, int64_t *classes) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 36) fail("sr_plda_plan writes 36 fields");
    if (kind != PLDA_TRAIN && kind != PLDA_SCORE) fail("sr_plda_plan: the kind is 0 (training) or 1 (scoring)");
    std::string why;
    PldaPlan p;
    auto plan = [&](int cu) {
        const bool ok = kind == PLDA_TRAIN ? plan_plda_train(rows, R, counts, groups, lds_rows, cu, p, why)
                                           : plan_plda_score(rows, T, R, counts, scratch_bytes, lds_rows, cu, p, why);
        if (!ok) fail("%s", why.c_str());
    };
    if (n_cu > 0) {
        plan(n_cu);
    } else {
        plan(1);                               // the refusals first
        ensure_device();
        plan(ctx().n_cu);
    }
    const int64_t v[36] = {p.kind, p.R, p.rows, p.groups, p.T, (int64_t)p.classes.size(), p.sum_chunk, p.sum_chunks, p.grp_chunk, p.grp_chunks,
                           p.chunk, p.n_chunks, p.seg_bytes, p.bytes_scratch, p.bytes_blocks, p.bytes_rows, p.path, p.lds_rows, p.factor_lds,
                           p.gemm_lds, p.centre.x, p.class_sums.x, p.class_sums.y, p.invert.x, p.gemm_rows.x, p.gemm_rows.y, p.gemm_acc.x,
                           p.gemm_acc.y, p.rowdot.x, p.gemm_cross.x, p.gemm_cross.y, p.assemble.x, p.invert_rounds,
                           PLDA_MAX_R, PLDA_MAX_ROWS, p.tri.y};
    std::memcpy(out, v, sizeof v);
    if (perm) std::memcpy(perm, p.perm.data(), p.perm.size() * sizeof(int64_t));
    if (classes)
        for (size_t c = 0; c < p.classes.size(); c++)
            classes[3 * c] = p.classes[c].count, classes[3 * c + 1] = p.classes[c].start, classes[3 * c + 2] = p.classes[c].size;
    return 36;
    SR_CATCH(-1)
}

// ---- the symmetric eigen-solver and what the back end builds on it (eig.hip, backend_eig.hip).  Every refusal comes first. ----

int sr_sym_eig(int R, const double *A, double *w, double *V, int *sweeps, int *converged) {
    SR_TRY
    sym_eig(R, A, w, V, sweeps, converged);
    return 0;
    SR_CATCH(-1)
}

int sr_gen_eig(int R, const double *Sb, const double *Sw, double *psi, double *V, int *sweeps, int *status) {
    SR_TRY
    gen_eig(R, Sb, Sw, psi, V, sweeps, status);
    return 0;
    SR_CATCH(-1)
}

int sr_lda_fit(int64_t n, int R, const double *X, const int64_t *ids, int64_t n_labels, int P, double *mu, double *A, double *psi) {
    SR_TRY
    lda_fit(n, R, X, ids, n_labels, P, mu, A, psi);
    return 0;
    SR_CATCH(-1)
}

int sr_backend_project(int64_t n, int R, int P, const double *X, const double *mu, const double *A, int length_norm, double *Y, int64_t *zero_rows) {
    SR_TRY
    backend_project(n, R, P, X, mu, A, length_norm, Y, zero_rows);
    return 0;
    SR_CATCH(-1)
}

int sr_plda_score_diag(int64_t J, int64_t T, int R, const double *mu, const double *V, const double *psi, const double *E, const int64_t *enrol_n,
                       const double *X, double *out, int64_t *bad_classes) {
    SR_TRY
    plda_score_diag(J, T, R, mu, V, psi, E, enrol_n, X, out, bad_classes);
    return 0;
    SR_CATCH(-1)
}

int sr_eig_plan(int R, int n_cu, int64_t *out, int n_out, int *schedule) {
    SR_TRY
    if (!out) fail("null argument");
    if (n_out < 24) fail("sr_eig_plan writes 24 fields");
    std::string why;
    EigPlan p;
    if (n_cu > 0) {
        if (!plan_eig(R, n_cu, p, why)) fail("%s", why.c_str());
    } else {
        if (!plan_eig(R, 1, p, why)) fail("%s", why.c_str());      // the refusals first
        ensure_device();
        if (!plan_eig(R, ctx().n_cu, p, why)) fail("%s", why.c_str());
    }
    const int64_t v[24] = {p.R, p.b, p.blocks, p.phantom, p.rounds, p.pairs, p.single, p.max_sweeps, p.inner_sweeps, p.solve_lds, p.update_lds,
                           p.solve_grid, p.cols_x, p.cols_y, p.cols_z, p.rows_x, p.rows_y, p.launches_per_sweep, p.bytes_work, p.pair_rounds,
                           PLDA_MAX_R, EIG_TILE_ROWS, EIG_N, EIG_WG};
    std::memcpy(out, v, sizeof v);
    if (schedule)
        for (size_t i = 0; i < p.schedule.size(); i++) schedule[2 * i] = p.schedule[i].p, schedule[2 * i + 1] = p.schedule[i].q;
    return 24;
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

int sr_hbm_copy_gbps(size_t bytes, int iters, double *gbps_out) {
    SR_TRY
    if (!gbps_out || bytes == 0 || iters <= 0) fail("bad arguments to sr_hbm_copy_gbps");
    ensure_device();
    DevBuf<char> a(bytes), b(bytes);
    SR_HIP(hipMemsetAsync(a.p, 1, bytes, ctx().stream));
    hipEvent_t e0, e1;
    SR_HIP(hipEventCreate(&e0));
    SR_HIP(hipEventCreate(&e1));
    SR_HIP(hipMemcpyAsync(b.p, a.p, bytes, hipMemcpyDeviceToDevice, ctx().stream));   // warm
    SR_HIP(hipEventRecord(e0, ctx().stream));
    for (int i = 0; i < iters; i++)
        SR_HIP(hipMemcpyAsync(b.p, a.p, bytes, hipMemcpyDeviceToDevice, ctx().stream));
    SR_HIP(hipEventRecord(e1, ctx().stream));
    SR_HIP(hipStreamSynchronize(ctx().stream));
    float ms = 0.f;
    SR_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *gbps_out = 2.0 * (double)bytes * iters / ((double)ms * 1e-3) / 1e9;
    return 0;
    SR_CATCH(-1)
}

int sr_profile_enable(int on) {
    SR_TRY
    if (on) {
        ensure_device();
        profile_prewarm();
    }
    ctx().profiling = on != 0;
    return 0;
    SR_CATCH(-1)
}

int sr_profile_reset(void) {
    SR_TRY
    profile_reset();
    return 0;
    SR_CATCH(-1)
}

int sr_profile_get(int kind, double *total_ms, long *launches) {
    SR_TRY
    profile_get(kind, total_ms, launches);
    return 0;
    SR_CATCH(-1)
}

int64_t sr_ltsd_num_windows(int64_t n_samples, int winsize) {
    SR_TRY
    return ltsd_num_windows(n_samples, winsize);
    SR_CATCH(-1)
}

int sr_ltsd_noise_spectrum(SRBatch *noise, int winsize, float *avg_amp_out) {
    SR_TRY
    if (!noise || !avg_amp_out) fail("null argument");
    ltsd_noise_spectrum(*noise, winsize, avg_amp_out);
    return 0;
    SR_CATCH(-1)
}

int sr_ltsd_compute(SRBatch *pcm, int winsize, int order, const float *noise_amp, float *ltsd_out,
                    int64_t *win_offsets_out) {
    SR_TRY
    if (!pcm || !noise_amp || !ltsd_out) fail("null argument");
    ltsd_compute(*pcm, winsize, order, noise_amp, ltsd_out, win_offsets_out);
    return 0;
    SR_CATCH(-1)
}

int sr_set_option(const char *key, long value) {
    SR_TRY
    if (!key) fail("null key");
    const std::string k(key);
    if (k == "score_frames_per_lane") {
        if (value != 0 && value != 1 && value != 2 && value != 4) fail("frames per lane must be 0/1/2/4");
        score_options().frames_per_lane = (int)value;
    } else if (k == "score_model_groups") {
        score_options().model_groups = (int)value;
    } else if (k == "score_packed") {
        score_options().packed = (int)value;
    } else if (k == "score_engine") {
        if (value < 0 || value > 6 || value == 2)
            fail("score_engine must be 0 (auto), 1 (vector ALU), 3 (split-bf16 matrix cores), 4 (split-bf16, shared-sigma form), "
                 "5 (split-fp16 matrix cores) or 6 (split-fp16, shared-sigma form); 2 was the fp32 matrix-core engine, removed in round 5 "
                 "(never selected: 1.45-1.8x slower than split-bf16 at the same accuracy)");
        score_options().engine = (int)value;
    } else if (k == "score_h2s_shape") {
        if (value < 0 || value > 6)
            fail("score_h2s_shape must be 0 (automatic), 1 (4-wave workgroups), 2 (12-wave workgroups), 3 (12 waves, image loop pipelined inside the wave), "
                 "4 (4 waves on one tile, the block's models split between them), 5 (as 3, on the flat image where 3 takes the compact one) "
                 "or 6 (as 3, one quadratic half per block where 3 forms one per two blocks)");
        score_options().h2s_shape = (int)value;
    } else if (k == "flush_list_cap") {
        if (value < 0) fail("flush_list_cap must be >= 0");
        score_options().flush_list_cap = (int)value;
    } else if (k == "score_h2s_pack_tails") {
        if (value != 0 && value != 1) fail("score_h2s_pack_tails must be 0 or 1");
        score_options().h2s_pack_tails = (int)value;
    } else if (k == "score_h2s_force_exc") {
        score_options().h2s_force_exc = value != 0;
    } else if (k == "score_split_shape") {
        if (value != 0 && value != 1 && value != 8 && value != 12 && value != 16)
            fail("score_split_shape must be 0 (automatic), 1 (4-wave workgroups) or 8 / 12 / 16 (waves of the wide, pipelined form)");
        score_options().split_shape = (int)value;
    } else if (k == "score_mfma_ft") {
        if (value < 0 || value > 4) fail("score_mfma_ft must be 0..4");
        score_options().mfma_ft = (int)value;
    } else if (k == "flush_order") {
        if (value != 1 && value != 2)
            fail("flush_order must be 2 (partial products as the reference DSO's compiler forms them: even / odd dimensions) or "
                 "1 (the source's order, gmm.cc:192-195)");
        flush_order_option() = (int)value;
    } else if (k == "kmeans_assign_engine") {
        if (value != 0 && value != 1) fail("kmeans_assign_engine must be 0 (fast full search, exact pass for what it cannot decide) or 1 (exact pass only)");
        set_kmeans_assign_engine((int)value);
    } else if (k == "reference_side_effects") {
        if (value != 0 && value != 1) fail("reference_side_effects must be 0 or 1");
        set_reference_side_effects((int)value);
    } else if (k == "em_stats_engine") {
        if (value < 0 || value > 3)
            fail("em_stats_engine must be 0 (automatic), 1 (vector ALU), 2 (fp64 matrix cores, responsibilities on the vector ALU) or "
                 "3 (automatic, an iteration per launch: no whole-fit kernel)");
        set_em_stats_engine((int)value);
    } else if (k == "multi_merge_same_device") {
        multi_merge_option().store(value != 0);
    } else if (k == "multi_numa_bind") {
        if (value != 0 && value != 1) fail("multi_numa_bind must be 0 or 1");
        numa_bind_option().store((int)value);
    } else if (k == "debug_capture_delay_ms") {
        if (value < 0 || value > 1000) fail("debug_capture_delay_ms must be 0 .. 1000");
        stream_debug_capture_delay_ms().store((int)value);         // test hook (tests/test_gpu_pipeline.py)
    } else if (k == "debug_em_small_absent_workgroup") {
        if (value != 0 && value != 1) fail("debug_em_small_absent_workgroup must be 0 or 1");
        set_em_small_test_absent((int)value);                       // test hook (tests/test_gpu_em_small.py): a workgroup of the whole-fit kernel stays away from a barrier
    } else if (k == "debug_verify_clean_counters") {
        if (value != 0 && value != 1) fail("debug_verify_clean_counters must be 0 or 1");
        score_options().verify_clean_counters = (int)value;        // test hook (tests/test_gpu_interleave.py): checked in score_device
    } else if (k == "debug_helper_max_models") {
        if (value < 0) fail("debug_helper_max_models must be >= 0 (0: the default)");
        fork_proxy_set_max_models(value);                           // test hook (tests/test_gpu_fork.py): applies in the helper, where it is forwarded
    } else if (k == "topc_scratch_mib") {
        if (value < 1 || value > (1L << 20)) fail("topc_scratch_mib must be within 1 .. %ld (the default is %ld)", 1L << 20, (long)(TOPC_DEFAULT_SCRATCH >> 20));
        set_topc_scratch_mib(value);
    } else if (k == "bw_scratch_mib") {
        if (value < 1 || value > (1L << 20)) fail("bw_scratch_mib must be within 1 .. %ld (the default is %ld)", 1L << 20, (long)(BW_DEFAULT_SCRATCH >> 20));
        set_bw_scratch_mib(value);
    } else if (k == "bw_range_frames") {
        if (value < 0 || value > (long)BW_MAX_RANGE_FRAMES) fail("bw_range_frames must be 0 (automatic) or 1 .. %ld frames", (long)BW_MAX_RANGE_FRAMES);
        set_bw_range_frames(value);
    } else if (k == "jfa_scratch_mib") {
        if (value < 1 || value > (1L << 20)) fail("jfa_scratch_mib must be within 1 .. %ld (the default is %ld)", 1L << 20, (long)(JFA_DEFAULT_SCRATCH >> 20));
        set_jfa_scratch_mib(value);
    } else if (k == "norm_scratch_mib") {
        if (value < 1 || value > (1L << 20)) fail("norm_scratch_mib must be within 1 .. %ld (the default is %ld)", 1L << 20, (long)(NORM_DEFAULT_SCRATCH >> 20));
        set_norm_scratch_mib(value);
    } else if (k == "calib_scratch_mib") {
        if (value < 1 || value > (1L << 20)) fail("calib_scratch_mib must be within 1 .. %ld (the default is %ld)", 1L << 20, (long)(CALIB_DEFAULT_SCRATCH >> 20));
        set_calib_scratch_mib(value);
    } else if (k == "plda_scratch_mib") {
        if (value < 1 || value > (1L << 20)) fail("plda_scratch_mib must be within 1 .. %ld (the default is %ld)", 1L << 20, (long)(PLDA_DEFAULT_SCRATCH >> 20));
        set_plda_scratch_mib(value);
    } else if (k == "jfa_lds_rows") {
        if (value < 0 || value > JFA_LDS_MAX_R) fail("jfa_lds_rows must be 0 (automatic) or 1 .. %d rows", JFA_LDS_MAX_R);
        set_jfa_lds_rows(value);
    } else if (k == "full_fit_batch_bytes") {
        if (value < 1) fail("full_fit_batch_bytes must be >= 1 (the default is %ld)", 1L << 30);
        set_full_fit_batch_bytes(value);
    } else if (k == "map_fit_batch_bytes") {
        if (value < 1) fail("map_fit_batch_bytes must be >= 1 (the default is %ld)", (long)MAP_DEFAULT_SCRATCH);
        set_map_fit_batch_bytes(value);
    } else if (k == "silence_block") {
        if (value < 0 || value > SILENCE_MAX_REL) fail("silence_block must be 0 (automatic) or 1 .. 2^30 positions per block");
        set_silence_block(value);
    } else if (k == "norm_tile") {
        if (value < 0 || value > FEATNORM_MAX_TILE || value % FEATNORM_WAVE != 0)
            fail("norm_tile must be 0 (automatic) or a multiple of 64 up to 1024 frames per workgroup");
        set_feature_norm_tile(value);
    } else if (k == "mfcc_generic") {
        mfcc_set_force_generic(value != 0);
    } else if (k == "mfcc_precision") {
        if (value != 0 && value != 2)
            fail("mfcc_precision must be 2 (float64 spectrum, ln and DCT for every frame: the reference's arithmetic, MFCC.py:59-70) or "
                 "0 (fp32 throughout: ~1.5x faster, features up to 2e-2 off on voices whose mel bands lie > 60 dB apart)");
        mfcc_set_precision((int)value);
    } else {
        fail("unknown option '%s'", key);
    }
    fork_proxy_note_option(key, value);
    return 0;
    SR_CATCH(-1)
}

const char *sr_last_score_kernel(void) { return last_score_kernel(); }
int sr_last_em_stats_engine(void) { return sr::last_em_stats_engine(); }

void sr_flush_stats(long *calls, long *pairs, long *frames) { flush_stats(calls, pairs, frames); }

void sr_kmeans_fast_stats(long *passes, long *rechecked) { kmeans_fast_stats(passes, rechecked); }

int sr_mfma_peak_probe(double ms_target, double *tflops, double *mhz) {
    SR_TRY
    if (!(ms_target > 0.0) || ms_target > 2000.0) fail("ms_target must be in (0, 2000]");
    mfma_peak_probe(ms_target, tflops, mhz);
    return 0;
    SR_CATCH(-1)
}

int sr_mfma_streamed_probe(double ms_target, double *tflops, double *mhz) {
    SR_TRY
    if (!(ms_target > 0.0) || ms_target > 2000.0) fail("ms_target must be in (0, 2000]");
    mfma_peak_probe(ms_target, tflops, mhz, 1);
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

// ---- full-covariance GMMs (gmm_full.hip) ----
SRFullGMM *sr_fullgmm_create(int K, int D, const double *weights, const double *means, const double *prec_chol) {
    SR_TRY
    if (K < 1) fail("n_components must be >= 1 (got %d)", K);
    if (D < 1 || D > FULL_MAX_D) fail("full-covariance models support 1 <= D <= %d dims (got %d)", FULL_MAX_D, D);
    const int given = (weights != nullptr) + (means != nullptr) + (prec_chol != nullptr);
    if (given != 0 && given != 3) fail("give weights, means and prec_chol together, or none of them");
    auto g = std::make_unique<SRFullGMM>();
    g->K = K;
    g->D = D;
    if (given) {
        g->weights.assign(weights, weights + K);
        g->means.assign(means, means + (size_t)K * D);
        g->prec_chol.assign(prec_chol, prec_chol + (size_t)K * D * D);
        for (int k = 0; k < K; k++) {
            if (!(g->weights[k] >= 0.0) || !std::isfinite(g->weights[k])) fail("weight %d is not a finite value >= 0", k);
            for (int i = 0; i < D; i++) {
                if (!(g->prec_chol[((size_t)k * D + i) * D + i] > 0.0)) fail("precisions_cholesky[%d] has a diagonal entry <= 0", k);
                for (int j = 0; j < i; j++)
                    if (g->prec_chol[((size_t)k * D + i) * D + j] != 0.0) fail("precisions_cholesky[%d] is not upper triangular", k);
            }
        }
        for (double v : g->means)
            if (!std::isfinite(v)) fail("means must be finite");
        for (double v : g->prec_chol)
            if (!std::isfinite(v)) fail("precisions_cholesky must be finite");
        g->trained = true;
    }
    return g.release();
    SR_CATCH(nullptr)
}

int sr_fullgmm_fit(SRFullGMM *g, const double *X, int64_t n, int D, const SRFullFitParams *params, SRFullFitStats *out) {
    SR_TRY
    if (!g || !X || !params || !out) fail("null argument");
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_fullgmm_fit");
    fullgmm_fit(*g, X, (long)n, D, *params, *out);
    return 0;
    SR_CATCH(-1)
}

namespace {
thread_local std::vector<std::string> g_fit_batch_messages;      // of the calling thread's last sr_fullgmm_fit_batch
}  // namespace

int sr_fullgmm_fit_batch(SRFullGMM *const *models, int S, const double *X, const int64_t *row_offsets, int D, const SRFullFitParams *params,
                         SRFullFitStats *out, int *status) {
    SR_TRY
    g_fit_batch_messages.clear();
    if (!models || !X || !row_offsets || !params || !out || !status) fail("null argument");
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_fullgmm_fit_batch");
    fullgmm_fit_batch(models, S, X, row_offsets, D, params, out, status, g_fit_batch_messages);
    return 0;
    SR_CATCH(-1)
}

const char *sr_fullgmm_fit_batch_error(int s) {
    const auto &m = g_fit_batch_messages;
    return s >= 0 && (size_t)s < m.size() ? m[(size_t)s].c_str() : "";
}

void sr_full_fit_batch_stats(long *calls, long *speakers, long *iterations) { full_fit_batch_stats(calls, speakers, iterations); }

long sr_full_fit_batch_bytes(void) { return full_fit_batch_bytes(); }

int sr_full_fit_plan(int K, int D, const int64_t *lengths, const int *init_given, const int *max_iter, int S, int64_t bound_bytes,
                     int64_t *speakers_out, int64_t *groups_out, int64_t group_cap, int64_t *out, int n_out) {
    SR_TRY
    if (!out || !lengths) fail("null argument");
    if (n_out < 7) fail("sr_full_fit_plan writes 7 fields");
    if (S < 1) fail("a plan needs at least one speaker (S = %d)", S);
    std::vector<int> given((size_t)S, 0), iters((size_t)S, 100);
    if (init_given) given.assign(init_given, init_given + S);
    if (max_iter) iters.assign(max_iter, max_iter + S);
    FullFitPlan p;
    std::string why;
    if (!plan_full_fit(K, D, lengths, given.data(), iters.data(), S, bound_bytes == 0 ? (int64_t)full_fit_batch_bytes() : bound_bytes, p, why))
        fail("%s", why.c_str());
    const int64_t v[7] = {(int64_t)p.groups.size(), (int64_t)p.wl_lp.size(), (int64_t)p.wl_lse.size(), (int64_t)p.wl_cov.size(),
                          (int64_t)p.lds_logprob, p.max_group_bytes, full_speaker_bytes(K, D, lengths[0])};
    std::memcpy(out, v, sizeof v);
    if (speakers_out)
        for (int s = 0; s < S; s++) {
            const FullSpeakerPlan &sp = p.speakers[(size_t)s];
            const int64_t r[8] = {sp.n, sp.row0, sp.n_chunks, sp.chunk, sp.o_partial, sp.bytes, sp.group, sp.slot};
            std::memcpy(speakers_out + 8 * (size_t)s, r, sizeof r);
        }
    if (groups_out)
        for (int64_t g = 0; g < std::min<int64_t>((int64_t)p.groups.size(), group_cap); g++) {
            const FullGroupPlan &gp = p.groups[(size_t)g];
            const FullCounts &c = gp.counts;
            const int64_t r[28] = {gp.first, gp.count, gp.rows, gp.lp0, gp.lse0, gp.cov0, gp.max_iter, gp.any_kmeans, gp.any_given, gp.bytes,
                                   c.X, c.w, c.logw, c.mu, c.prec, c.logdet, c.cov, c.lp, c.lpn, c.nk, c.partial, c.head,
                                   c.spk, c.rec, c.wl_lp, c.wl_lse, c.wl_cov, c.label};
            std::memcpy(groups_out + 28 * g, r, sizeof r);
        }
    return 7;
    SR_CATCH(-1)
}

int sr_fullgmm_info(SRFullGMM *g, int *K, int *D) {
    SR_TRY
    if (!g) fail("null handle");
    if (K) *K = g->K;
    if (D) *D = g->D;
    return g->trained ? 1 : 0;
    SR_CATCH(-1)
}

int sr_fullgmm_get(SRFullGMM *g, double *weights, double *means, double *covariances, double *prec_chol) {
    SR_TRY
    if (!g) fail("null handle");
    if (!g->trained) fail("the model has no parameters yet (fit it first)");
    const size_t K = g->K, D = g->D;
    if (weights) std::memcpy(weights, g->weights.data(), sizeof(double) * K);
    if (means) std::memcpy(means, g->means.data(), sizeof(double) * K * D);
    if (prec_chol) std::memcpy(prec_chol, g->prec_chol.data(), sizeof(double) * K * D * D);
    if (covariances) {
        if (g->covariances.empty()) std::memset(covariances, 0, sizeof(double) * K * D * D);
        else std::memcpy(covariances, g->covariances.data(), sizeof(double) * K * D * D);
    }
    return 0;
    SR_CATCH(-1)
}

void sr_fullgmm_free(SRFullGMM *g) { delete g; }

SRFullSet *sr_fullset_create(SRFullGMM *const *models, int S) {
    SR_TRY
    if (!models) fail("null argument");
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_fullset_create");
    auto set = std::make_unique<SRFullSet>();
    fullset_pack(*set, models, S);
    return set.release();
    SR_CATCH(nullptr)
}

int sr_fullset_score_batch(SRFullSet *set, SRBatch *batch, double *sums_out, int *argmax_out, float *frame_ll_out) {
    SR_TRY
    if (!set || !batch) fail("null argument");
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_fullset_score_batch");
    fullset_score(*set, *batch, sums_out, argmax_out, frame_ll_out);
    return 0;
    SR_CATCH(-1)
}

int sr_fullset_predict_pcm_batch(SRMfcc *m, SRFullSet *set, SRBatch *pcm, int nd, double *sums_out, int *argmax_out) {
    SR_TRY
    if (!m || !set || !pcm) fail("null argument");
    if (gpu_runtime_lost()) fail_gpu_runtime_lost("sr_fullset_predict_pcm_batch");
    fullset_predict_pcm(*m, *set, *pcm, nd, sums_out, argmax_out);
    return 0;
    SR_CATCH(-1)
}

void sr_fullset_free(SRFullSet *set) { delete set; }

}  // extern "C"
