// abi_stats.cpp -- what is computed from Baum-Welch statistics against a UBM: the statistics and their handles, the batched MAP
// fit, JFA.
#include "abi_internal.hpp"

#include "bw_plan.hpp"
#include "bw_stats.hpp"
#include "gmm_model.hpp"
#include "jfa.hpp"
#include "jfa_plan.hpp"
#include "map_batch.hpp"
#include "map_plan.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

using namespace sr;

extern "C" {

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
    n_cu = plan_n_cu(n_cu);
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
    n_cu = plan_n_cu(n_cu);
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

}  // extern "C"
