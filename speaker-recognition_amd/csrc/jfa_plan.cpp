// jfa_plan.cpp -- the decisions of the JFA factor estimation (jfa_plan.hpp).  Host-only.
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

bool jfa_check_finite(const double *v, int64_t n, const char *what, std::string &why) {
    for (int64_t i = 0; i < n; i++)
        if (!std::isfinite(v[i])) {
            char buf[256];
            snprintf(buf, sizeof buf, "JFA factors: %s holds a non-finite value at element %lld; drop that row or repair the statistics",
                     what, (long long)i);
            why = buf;
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
            why = fmt("JFA factors: N holds a negative occupancy at group %lld, mixture %lld; occupancies are sums of posteriors", i / K, i % K);
            return false;
        }
    for (int64_t i = 0; i < kd; i++)
        if (!(E[i] > 0.0)) {
            why = fmt("JFA factors: E must be positive, element %lld is not; pass the UBM's variances", i);
            return false;
        }
    return true;
}

int jfa_lds_limit(int lds_rows) { return lds_rows <= 0 ? JFA_LDS_MAX_R : std::min(lds_rows, JFA_LDS_MAX_R); }

int jfa_factor_lds_bytes(int R, int path) {
    // the panel [R][JFA_NB + 1], two vectors [R], and on the LDS path the block itself
    return (int)(((int64_t)R * (JFA_NB + 1) + 2 * (int64_t)R + (path == 0 ? (int64_t)R * R : 0)) * (int64_t)sizeof(double));
}

static JfaGrid gemm_grid(int64_t M, int64_t N) { return JfaGrid{(N + JFA_TILE - 1) / JFA_TILE, (M + JFA_TILE - 1) / JFA_TILE}; }

bool plan_jfa(int64_t G, int K, int D, int R, int64_t scratch_bytes, int lds_rows, int n_cu, JfaPlan &p, std::string &why) {
    p = JfaPlan();
    if (!jfa_check_shape(G, K, D, why) || !jfa_check_rank(R, why)) return false;
    if (lds_rows < 0 || lds_rows > JFA_LDS_MAX_R) {
        why = fmt("jfa_lds_rows must be 0 (automatic) or 1 .. %lld", JFA_LDS_MAX_R);
        return false;
    }
    if (n_cu < 1) {
        why = "JFA factors: the plan needs the number of compute units";
        return false;
    }
    const int64_t rr = (int64_t)R * R, kd = (int64_t)K * D, block = rr * (int64_t)sizeof(double);
    const int64_t fit = scratch_bytes / block;
    if (fit >= G) p.chunk = G;
    else p.chunk = fit / JFA_KSTEP * JFA_KSTEP;
    p.chunk = std::min<int64_t>(p.chunk, (int64_t)65535 * JFA_TILE);       // (a chunk's row tiles are the L launch's grid y)
    if (p.chunk < 1) {
        why = fmt("JFA factors: the scratch bound of %lld bytes is below one chunk of %lld bytes (16 groups' R x R blocks); raise the option jfa_scratch_mib",
                  scratch_bytes, std::min<int64_t>(G, JFA_KSTEP) * block);
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
    p.lds_rows = jfa_lds_limit(lds_rows);
    p.path = R <= p.lds_rows ? 0 : 1;
    const int64_t gt = (R + JFA_GRAM_TILE - 1) / JFA_GRAM_TILE;
    p.gram = JfaGrid{K, gt * gt};         // (mixtures along x: the larger limit)
    p.gemm_L = gemm_grid(p.chunk, rr);
    p.gemm_b = gemm_grid(p.chunk, R);
    p.gemm_A = gemm_grid(K, rr);
    p.gemm_C = gemm_grid(R, kd);
    p.gram_lds = 2 * JFA_GRAM_TILE * (JFA_GRAM_DSTEP + 1) * (int)sizeof(double) + JFA_GRAM_DSTEP * (int)sizeof(double);
    p.gemm_lds = 2 * JFA_KSTEP * (JFA_TILE + 4) * (int)sizeof(double);
    p.factor_lds = p.update_lds = jfa_factor_lds_bytes(R, p.path);
    p.factor_rounds = (p.chunk + n_cu - 1) / n_cu;
    return true;
}

}  // namespace sr
