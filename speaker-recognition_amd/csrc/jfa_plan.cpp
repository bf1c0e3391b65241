// jfa_plan.cpp -- the decisions of the JFA factor estimation, centring and trial scoring (jfa_plan.hpp); the GEMM's grids, the
// factorisation's path and their LDS bytes are the dense layer's (dense64_plan.hpp).  Host-only.
#include "jfa_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>

namespace sr {

static std::string fmt(const char *f, long long a = 0, long long b = 0) {
    char buf[320];
    snprintf(buf, sizeof buf, f, a, b);
    return buf;
}

bool jfa_check_shape(int64_t G, int K, int D, std::string &why) {
    if (G < 1 || K < 1 || D < 1) {
        why = fmt("JFA factors: need at least one group, one mixture and one dimension (G, K, D >= 1); K x D = %lld x %lld", K, D);
        return false;
    }
    if (G > ((int64_t)1 << 31) - 1 || (int64_t)K * D > ((int64_t)1 << 31) - 1) {
        why = "JFA factors: more than 2^31 - 1 groups or supervector columns; split the corpus";
        return false;
    }
    return true;
}

bool jfa_check_rank(int R, std::string &why) {
    if (R < 1) {
        why = "JFA factors: the loading matrix needs at least one row (R >= 1)";
        return false;
    }
    if (R > JFA_MAX_R) {
        why = fmt("JFA factors are built for up to %lld factors, the loading matrix has %lld rows; train fewer factors", JFA_MAX_R, R);
        return false;
    }
    return true;
}

std::string jfa_text_non_finite(const char *what, int64_t element) {
    char buf[256];
    snprintf(buf, sizeof buf, "JFA factors: %s holds a non-finite value at element %lld; drop that row or repair the statistics", what,
             (long long)element);
    return buf;
}

std::string jfa_text_negative(int64_t element, int K) {
    return fmt("JFA factors: N holds a negative occupancy at group %lld, mixture %lld; occupancies are sums of posteriors", element / K, element % K);
}

bool jfa_check_finite(const double *v, int64_t n, const char *what, std::string &why) {
    for (int64_t i = 0; i < n; i++)
        if (!std::isfinite(v[i])) {
            why = jfa_text_non_finite(what, i);
            return false;
        }
    return true;
}

bool jfa_check_raw_stats(int64_t n, int K, int D, const double *N, const double *F, std::string &why) {
    if (!jfa_check_shape(n, K, D, why)) return false;
    if (!N || !F) {
        why = "JFA statistics: null argument (N and F are both required)";
        return false;
    }
    if (!jfa_check_finite(N, n * K, "N", why) || !jfa_check_finite(F, n * (int64_t)K * D, "F", why)) return false;
    for (int64_t i = 0; i < n * K; i++)
        if (N[i] < 0.0) {
            why = jfa_text_negative(i, K);
            return false;
        }
    return true;
}

bool jfa_check_stats(int64_t G, int K, int D, const double *N, const double *Fc, const double *E, std::string &why) {
    if (!jfa_check_shape(G, K, D, why)) return false;
    if (!N || !Fc || !E) {
        why = "JFA factors: null argument (N, Fc and E are all required)";
        return false;
    }
    const int64_t kd = (int64_t)K * D;
    if (!jfa_check_finite(N, G * K, "N", why) || !jfa_check_finite(Fc, G * kd, "Fc", why) || !jfa_check_finite(E, kd, "E", why)) return false;
    for (int64_t i = 0; i < G * K; i++)
        if (N[i] < 0.0) {
            why = jfa_text_negative(i, K);
            return false;
        }
    for (int64_t i = 0; i < kd; i++)
        if (!(E[i] > 0.0)) {
            why = fmt("JFA factors: E must be positive, element %lld is not; pass the UBM's variances", i);
            return false;
        }
    return true;
}

bool plan_jfa(int64_t G, int K, int D, int R, int64_t scratch_bytes, int lds_rows, int n_cu, JfaPlan &p, std::string &why) {
    p = JfaPlan();
    if (!jfa_check_shape(G, K, D, why) || !jfa_check_rank(R, why)) return false;
    if (!dense_check_lds_rows(lds_rows, why)) return false;
    if (n_cu < 1) {
        why = "JFA factors: the plan needs the number of compute units";
        return false;
    }
    const int64_t rr = (int64_t)R * R, kd = (int64_t)K * D, block = rr * (int64_t)sizeof(double);
    const int64_t fit = scratch_bytes / block;
    if (fit >= G) p.chunk = G;
    else p.chunk = fit / DENSE_KSTEP * DENSE_KSTEP;
    p.chunk = std::min<int64_t>(p.chunk, (int64_t)65535 * DENSE_TILE);       // (a chunk's row tiles are the L launch's grid y)
    if (p.chunk < 1) {
        why = fmt("JFA factors: the scratch bound of %lld bytes is below one chunk of %lld bytes (16 groups' R x R blocks); raise the option jfa_scratch_mib",
                  scratch_bytes, std::min<int64_t>(G, DENSE_KSTEP) * block);
        return false;
    }
    if (rr * (int64_t)K > ((int64_t)1 << 40)) {
        why = "JFA factors: K x R x R exceeds 2^40 elements; train fewer factors";
        return false;
    }
    p.n_chunks = (G + p.chunk - 1) / p.chunk;
    p.bytes_N = G * K * 8;
    p.bytes_Fc = G * kd * 8;
    p.bytes_E = 2 * kd * 8;
    p.bytes_P = p.bytes_A = (int64_t)K * rr * 8;
    p.bytes_C = (int64_t)R * kd * 8;
    p.bytes_W = 2 * p.bytes_C;
    p.bytes_y = 2 * G * R * 8;
    p.bytes_scratch = p.chunk * block;
    p.lds_rows = dense_lds_limit(lds_rows);
    p.path = R <= p.lds_rows ? 0 : 1;
    const int64_t gt = (R + JFA_GRAM_TILE - 1) / JFA_GRAM_TILE;
    p.gram = Grid2{K, gt * gt};         // (mixtures along x: the larger limit)
    p.gemm_L = dense_gemm_grid(p.chunk, rr);
    p.gemm_b = dense_gemm_grid(p.chunk, R);
    p.gemm_A = dense_gemm_grid(K, rr);
    p.gemm_C = dense_gemm_grid(R, kd);
    p.gram_lds = 2 * JFA_GRAM_TILE * (JFA_GRAM_DSTEP + 1) * (int)sizeof(double) + JFA_GRAM_DSTEP * (int)sizeof(double);
    p.gemm_lds = dense_gemm_lds_bytes();
    p.factor_lds = p.update_lds = jfa_factor_lds_bytes(R, p.path);
    p.factor_rounds = (p.chunk + n_cu - 1) / n_cu;
    return true;
}

// ---- resident statistics: grouping and centring ----

bool jfa_centre_check_shape(int64_t n, int K, int D, int mode, int64_t n_labels, int Ry, int Ru, bool has_v, bool has_u, std::string &why) {
    if (mode != JFA_CENTRE_GROUPS && mode != JFA_CENTRE_SESSIONS) {
        why = "JFA centring: the mode is 0 (groups are speakers) or 1 (groups are sessions)";
        return false;
    }
    if (!jfa_check_shape(n, K, D, why)) return false;
    if (n_labels < 1 || n_labels > ((int64_t)1 << 31) - 1) {
        why = fmt("JFA centring: n_labels is %lld; pass the number of labels, 1 .. 2^31 - 1 (the largest label + 1)", n_labels);
        return false;
    }
    if (has_v && (Ry < 1 || Ry > JFA_MAX_R)) {
        why = fmt("JFA centring is built for 1 .. %lld factors, Ry is %lld; pass v [Ry][K D] with its y, or neither", JFA_MAX_R, Ry);
        return false;
    }
    if (has_u && (Ru < 1 || Ru > JFA_MAX_R)) {
        why = fmt("JFA centring is built for 1 .. %lld factors, Ru is %lld; pass u [Ru][K D] with its x, or neither", JFA_MAX_R, Ru);
        return false;
    }
    const int64_t kd = (int64_t)K * D, cap = (int64_t)1 << 36;
    if (n > cap / kd) {          // (a label without sessions takes no row: at most n rows are ever held)
        why = "JFA centring: statistics of more than 2^36 values; split the corpus";
        return false;
    }
    return true;
}

bool jfa_centre_check_labels(const int64_t *ids, int64_t n, int64_t n_labels, std::string &why) {
    if (!ids) {
        why = "JFA centring: null argument (ids: one 0-based label per session)";
        return false;
    }
    for (int64_t j = 0; j < n; j++)
        if (ids[j] < 0 || ids[j] >= n_labels) {
            char buf[256];
            snprintf(buf, sizeof buf, "JFA centring: ids[%lld] is %lld, outside 0 .. n_labels - 1 = %lld; labels are 0-based, pass n_labels = the largest + 1",
                     (long long)j, (long long)ids[j], (long long)(n_labels - 1));
            why = buf;
            return false;
        }
    return true;
}

bool plan_jfa_centre(int64_t n, int64_t n_labels, int K, int D, int Ry, int Ru, int mode, int64_t scratch_bytes, JfaCentrePlan &p, std::string &why) {
    p = JfaCentrePlan();
    if (!jfa_centre_check_shape(n, K, D, mode, n_labels, Ry, Ru, Ry != 0, Ru != 0, why)) return false;
    const int64_t kd = (int64_t)K * D, row = kd * (int64_t)sizeof(double);
    p.mode = mode;
    p.vec = kd % JFA_CENTRE_VEC == 0 ? JFA_CENTRE_VEC : 1;
    if (Ru > 0) {
        // a function of n, K D and the bound only: whole GEMM row tiles, so that a chunk's product is full tiles but the last
        const int64_t fit = scratch_bytes / row;
        p.chunk = fit >= n ? n : fit / DENSE_TILE * DENSE_TILE;
        p.chunk = std::min<int64_t>(p.chunk, (int64_t)65535 * DENSE_TILE);
        if (p.chunk < 1) {
            why = fmt("JFA centring: the scratch bound of %lld bytes is below one chunk of %lld bytes (64 sessions' rows of the x u product); "
                      "raise the option jfa_scratch_mib", scratch_bytes, std::min<int64_t>(n, DENSE_TILE) * row);
            return false;
        }
        p.bytes_scratch = p.chunk * row;
    } else {
        p.chunk = n;
    }
    p.n_chunks = (n + p.chunk - 1) / p.chunk;
    const int64_t rows = mode == JFA_CENTRE_SESSIONS ? n : std::min(n, n_labels), labels = std::min(n, n_labels);
    p.bytes_N = rows * K * 8;
    p.bytes_Fc = rows * row;
    p.bytes_yv = Ry > 0 ? labels * row : 0;
    p.bytes_z = labels * row;
    const int64_t col_blocks = (kd / p.vec + JFA_WG - 1) / JFA_WG;
    if (col_blocks > 65535) {
        why = "JFA centring: more than 2^24 supervector columns; split the model";
        return false;
    }
    if (Ru > 0) p.gemm_xu = dense_gemm_grid(p.chunk, kd);
    if (Ry > 0) p.gemm_yv = dense_gemm_grid(labels, kd);
    p.centre = Grid2{std::min(rows, mode == JFA_CENTRE_SESSIONS ? p.chunk : rows), col_blocks};
    p.counts = Grid2{rows, (K + JFA_WG - 1) / JFA_WG};
    return true;
}

// ---- trial scoring ----

bool jfa_score_check_shape(int64_t T, int64_t J, int K, int D, int Ry, int Ru, int mode, std::string &why) {
    if (mode != JFA_SCORE_INTEGRATED && mode != JFA_SCORE_LINEAR) {
        why = "JFA scoring: the mode is 0 (integrated) or 1 (linear)";
        return false;
    }
    if (T < 1 || J < 1 || K < 1 || D < 1 || Ry < 1 || Ru < 1) {
        why = fmt("JFA scoring: need at least one test segment, one model, one mixture, one dimension, one eigenvoice and one eigenchannel "
                  "(T, J, K, D, Ry, Ru >= 1); T x J = %lld x %lld", T, J);
        return false;
    }
    if (Ry > JFA_MAX_R || Ru > JFA_MAX_R) {
        why = fmt("JFA scoring is built for up to %lld factors, v or u has %lld rows; score with fewer factors", JFA_MAX_R, std::max(Ry, Ru));
        return false;
    }
    const int64_t kd = (int64_t)K * D, cap = (int64_t)1 << 36;
    if (T > (int64_t)65535 * DENSE_TILE || J > JFA_SCORE_MAX_J || kd > ((int64_t)1 << 31) - 1 || T > cap / kd || J + 1 > cap / kd) {
        why = fmt("JFA scoring: more than %lld test segments or %lld models, or statistics or models of more than 2^36 values; split the trial list",
                  (int64_t)65535 * DENSE_TILE, JFA_SCORE_MAX_J);
        return false;
    }
    return true;
}

static bool score_check_inputs(bool resident, int64_t T, int64_t J, int K, int D, int Ry, int Ru, int mode, const double *N, const double *F,
                               const double *m, const double *E, const double *d, const double *v, const double *u, const double *z, const double *y,
                               const double *x, const unsigned char *mask, int64_t mask_rows, int64_t mask_cols, std::string &why) {
    if (!jfa_score_check_shape(T, J, K, D, Ry, Ru, mode, why)) return false;
    if ((!resident && (!N || !F)) || !m || !E || !v || !u || !y) {
        why = "JFA scoring: null argument (N, F, m, E, v, u and y are all required; d, z, x and the mask may be absent)";
        return false;
    }
    if (mode == JFA_SCORE_LINEAR && !x) {
        why = "JFA scoring: linear mode needs the test segments' channel factors x [T][Ru]; estimate them (estimate_x_and_u) or score in integrated mode";
        return false;
    }
    if (mask && (mask_rows != J || mask_cols != T)) {
        char buf[256];
        snprintf(buf, sizeof buf, "JFA scoring: the mask is [%lld][%lld], the score matrix [%lld][%lld]; pass one uint8 per (model, segment) pair",
                 (long long)mask_rows, (long long)mask_cols, (long long)J, (long long)T);
        why = buf;
        return false;
    }
    const int64_t kd = (int64_t)K * D;
    if ((!resident && (!jfa_check_finite(N, T * K, "N", why) || !jfa_check_finite(F, T * kd, "F", why))) || !jfa_check_finite(m, kd, "m", why) ||
        !jfa_check_finite(E, kd, "E", why) || (d && !jfa_check_finite(d, kd, "d", why)) || !jfa_check_finite(v, Ry * kd, "v", why) ||
        !jfa_check_finite(u, Ru * kd, "u", why) || (z && !jfa_check_finite(z, J * kd, "z", why)) || !jfa_check_finite(y, J * Ry, "y", why) ||
        (x && !jfa_check_finite(x, T * Ru, "x", why)))
        return false;
    for (int64_t i = 0; !resident && i < T * K; i++)
        if (N[i] < 0.0) {
            why = fmt("JFA scoring: N holds a negative occupancy at segment %lld, mixture %lld; occupancies are sums of posteriors", i / K, i % K);
            return false;
        }
    for (int64_t i = 0; i < kd; i++)
        if (!(E[i] > 0.0)) {
            why = fmt("JFA scoring: E must be positive, element %lld is not; pass the UBM's variances", i);
            return false;
        }
    return true;
}

bool jfa_score_check_inputs(int64_t T, int64_t J, int K, int D, int Ry, int Ru, int mode, const double *N, const double *F, const double *m,
                            const double *E, const double *d, const double *v, const double *u, const double *z, const double *y, const double *x,
                            const unsigned char *mask, int64_t mask_rows, int64_t mask_cols, std::string &why) {
    return score_check_inputs(false, T, J, K, D, Ry, Ru, mode, N, F, m, E, d, v, u, z, y, x, mask, mask_rows, mask_cols, why);
}

bool jfa_score_check_inputs_resident(int64_t T, int64_t J, int K, int D, int Ry, int Ru, int mode, const double *m, const double *E, const double *d,
                                     const double *v, const double *u, const double *z, const double *y, const double *x, const unsigned char *mask,
                                     int64_t mask_rows, int64_t mask_cols, std::string &why) {
    return score_check_inputs(true, T, J, K, D, Ry, Ru, mode, nullptr, nullptr, m, E, d, v, u, z, y, x, mask, mask_rows, mask_cols, why);
}

static Grid2 flat_grid(int64_t n) { return Grid2{(n + JFA_WG - 1) / JFA_WG, 1}; }

bool plan_jfa_score(int64_t T, int64_t J, int K, int D, int Ry, int Ru, int mode, int64_t scratch_bytes, int lds_rows, int n_cu, JfaScorePlan &p,
                    std::string &why) {
    p = JfaScorePlan();
    if (!jfa_score_check_shape(T, J, K, D, Ry, Ru, mode, why)) return false;
    if (!dense_check_lds_rows(lds_rows, why)) return false;
    if (n_cu < 1) {
        why = "JFA scoring: the plan needs the number of compute units";
        return false;
    }
    const int64_t rr = (int64_t)Ru * Ru, kd = (int64_t)K * D, J1 = J + 1;
    p.mode = mode;
    p.lds_rows = dense_lds_limit(lds_rows);
    p.path = Ru <= p.lds_rows ? 0 : 1;
    p.bytes_N = T * K * 8;
    p.bytes_F = T * kd * 8;
    p.bytes_uE = 2 * (int64_t)Ru * kd * 8;
    p.bytes_out = J * T * 8;
    p.gemm_lds = dense_gemm_lds_bytes();
    p.gemm_yv = dense_gemm_grid(J, kd);
    if (mode == JFA_SCORE_LINEAR) {
        p.chunk = T;
        p.n_chunks = 1;
        p.bytes_M = p.bytes_ME = J * kd * 8;
        p.bytes_comp = T * kd * 8;
        p.synth = p.scale_M = flat_grid(J * kd);
        p.gemm_xu = dense_gemm_grid(T, kd);
        p.comp = flat_grid(T * kd);
        p.gemm_out = dense_gemm_grid(J, T);
        return true;
    }
    p.seg_bytes = (rr + J1 * Ru) * (int64_t)sizeof(double);
    p.chunk = std::min<int64_t>(std::min<int64_t>(T, scratch_bytes / p.seg_bytes), (int64_t)65535 * DENSE_TILE);      // (row tiles: the GEMMs' grid y)
    if (p.chunk < 1) {
        why = fmt("JFA scoring: the scratch bound of %lld bytes is below one test segment's blocks of %lld bytes (Ru x Ru and (J + 1) x Ru doubles); "
                  "raise the option jfa_scratch_mib or score fewer models at a time", scratch_bytes, p.seg_bytes);
        return false;
    }
    if (rr * (int64_t)K > ((int64_t)1 << 40) || (int64_t)K * Ru * J1 > ((int64_t)1 << 40)) {
        why = "JFA scoring: K x Ru x Ru or K x Ru x (J + 1) exceeds 2^40 elements; score fewer models at a time";
        return false;
    }
    p.n_chunks = (T + p.chunk - 1) / p.chunk;
    p.bytes_scratch = p.chunk * p.seg_bytes;
    p.bytes_M = p.bytes_ME = J1 * kd * 8;
    p.bytes_P = (int64_t)K * rr * 8;
    p.bytes_q = J1 * K * 8;
    p.bytes_G = (int64_t)K * Ru * J1 * 8;
    p.bytes_lin = p.bytes_quad = T * J1 * 8;
    p.bytes_a = T * Ru * 8;
    p.synth = p.scale_M = flat_grid(J1 * kd);
    p.scale_u = flat_grid(Ru * kd);
    const int64_t gr = (Ru + JFA_GRAM_TILE - 1) / JFA_GRAM_TILE, gj = (J1 + JFA_GRAM_TILE - 1) / JFA_GRAM_TILE;
    p.gram = Grid2{K, gr * gr};
    p.cross = Grid2{K, gj};
    p.cross_z = gr;
    p.gemm_L = dense_gemm_grid(p.chunk, rr);
    p.gemm_a = dense_gemm_grid(p.chunk, Ru);
    p.gemm_lin = dense_gemm_grid(p.chunk, J1);
    p.gemm_quad = dense_gemm_grid(p.chunk, J1);
    p.gemm_h = dense_gemm_grid(p.chunk, Ru * J1);
    p.kscore = Grid2{p.chunk, 1};
    p.gram_lds = 2 * JFA_GRAM_TILE * (JFA_GRAM_DSTEP + 1) * (int)sizeof(double) + JFA_GRAM_DSTEP * (int)sizeof(double);
    p.cross_lds = 3 * JFA_GRAM_TILE * (JFA_GRAM_DSTEP + 1) * (int)sizeof(double);
    p.kscore_lds = jfa_factor_lds_bytes(Ru, p.path);
    p.kscore_rounds = (p.chunk + n_cu - 1) / n_cu;
    return true;
}

}  // namespace sr
