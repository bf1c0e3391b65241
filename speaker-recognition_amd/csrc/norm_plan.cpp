// norm_plan.cpp -- the decisions of score normalisation (norm_plan.hpp); the grids and LDS bytes of as2's products are the dense
// layer's (dense64_plan.hpp).  Host-only.
#include "norm_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>

namespace sr {

static std::string fmt(const char *f, long long a = 0, long long b = 0, long long c = 0) {
    char buf[400];
    snprintf(buf, sizeof buf, f, a, b, c);
    return buf;
}

const char *norm_mode_name(int mode) {
    static const char *names[6] = {"z", "t", "zt", "s", "as1", "as2"};
    return mode >= 0 && mode < 6 ? names[mode] : "?";
}

bool norm_mode_adaptive(int mode) { return mode == NORM_AS1 || mode == NORM_AS2; }
bool norm_needs_enrol(int mode) { return mode != NORM_T; }
bool norm_needs_test(int mode) { return mode != NORM_Z; }
bool norm_needs_zt(int mode) { return mode == NORM_ZT; }

int norm_select_lds_bytes(int64_t C) { return (int)(C * (int64_t)sizeof(double)) + NORM_SELECT_FIXED_LDS; }

static bool check_cohort(const char *which, const char *matrix, int64_t C, std::string &why) {
    if (C < 1) {
        char buf[256];
        snprintf(buf, sizeof buf, "score normalisation: %s is %lld; a cohort needs at least one member (%s holds one score per member)", which,
                 (long long)C, matrix);
        why = buf;
        return false;
    }
    if (C > NORM_MAX_C) {
        char buf[320];
        snprintf(buf, sizeof buf, "score normalisation is built for cohorts of up to %lld members (a cohort row and the selection's histogram share "
                 "a compute unit's LDS), %s is %lld; thin the cohort", (long long)NORM_MAX_C, which, (long long)C);
        why = buf;
        return false;
    }
    return true;
}

bool norm_check_shape(int mode, int64_t J, int64_t T, int64_t Cz, int64_t Ct, int top_n, std::string &why) {
    if (mode < NORM_Z || mode > NORM_AS2) {
        why = "score normalisation: the mode is 0 (z), 1 (t), 2 (zt), 3 (s), 4 (as1) or 5 (as2)";
        return false;
    }
    if (J < 1 || T < 1) {
        why = fmt("score normalisation: need at least one model and one test segment (J, T >= 1); J x T = %lld x %lld", J, T);
        return false;
    }
    if (J > NORM_MAX_ROWS || T > NORM_MAX_ROWS || J > (((int64_t)1 << 36) / T)) {
        why = fmt("score normalisation: more than %lld models or test segments, or a score matrix of more than 2^36 values; split the trial list",
                  NORM_MAX_ROWS);
        return false;
    }
    if (norm_needs_enrol(mode) && !check_cohort("Cz", "Ez", Cz, why)) return false;
    if (norm_needs_test(mode) && !check_cohort("Ct", "Tt", Ct, why)) return false;
    if (norm_mode_adaptive(mode) && top_n < 2) {
        why = fmt("score normalisation: top_n is %lld; an adaptive mode takes the moments of the top_n >= 2 largest cohort scores "
                  "(top_n >= the cohort's size selects everything)", top_n);
        return false;
    }
    if (mode == NORM_AS2 && Cz != Ct) {
        why = fmt("score normalisation: as2 needs one cohort whose members are both segments and models (Cz = Ct), got Cz = %lld and Ct = %lld; "
                  "score the same cohort on both sides or use as1", Cz, Ct);
        return false;
    }
    return true;
}

static bool check_finite(const double *v, int64_t n, const char *what, std::string &why) {
    for (int64_t i = 0; i < n; i++)
        if (!std::isfinite(v[i])) {
            char buf[256];
            snprintf(buf, sizeof buf, "score normalisation: %s holds a non-finite value at element %lld; drop that trial or cohort member", what,
                     (long long)i);
            why = buf;
            return false;
        }
    return true;
}

bool norm_check_inputs(int mode, int64_t J, int64_t T, int64_t Cz, int64_t Ct, int top_n, const double *S, const double *Ez, const double *Tt,
                       const double *Zt, std::string &why) {
    if (mode < NORM_Z || mode > NORM_AS2) return norm_check_shape(mode, J, T, Cz, Ct, top_n, why);
    if (!S) {
        why = "score normalisation: null argument (S, the score matrix [J][T])";
        return false;
    }
    const char *missing = nullptr;
    if (norm_needs_enrol(mode) && !Ez) missing = "Ez [J][Cz], the models against the Z-cohort";
    else if (norm_needs_test(mode) && !Tt) missing = "Tt [Ct][T], the T-cohort models against the test segments";
    else if (norm_needs_zt(mode) && !Zt) missing = "Zt [Ct][Cz], the T-cohort models against the Z-cohort";
    if (missing) {
        char buf[320];
        snprintf(buf, sizeof buf, "score normalisation: mode %s needs %s; score that matrix and pass it", norm_mode_name(mode), missing);
        why = buf;
        return false;
    }
    if (!norm_check_shape(mode, J, T, Cz, Ct, top_n, why)) return false;
    if (!check_finite(S, J * T, "S", why)) return false;
    if (norm_needs_enrol(mode) && !check_finite(Ez, J * Cz, "Ez", why)) return false;
    if (norm_needs_test(mode) && !check_finite(Tt, Ct * T, "Tt", why)) return false;
    if (norm_needs_zt(mode) && !check_finite(Zt, Ct * Cz, "Zt", why)) return false;
    return true;
}

bool norm_check_select(int64_t rows, int64_t C, int top_n, const double *X, std::string &why) {
    if (rows < 1 || rows > NORM_MAX_ROWS) {
        why = fmt("cohort selection: rows is %lld; pass 1 .. %lld rows of cohort scores", rows, NORM_MAX_ROWS);
        return false;
    }
    if (!check_cohort("C", "X", C, why)) return false;
    if (top_n < 2) {
        why = fmt("cohort selection: top_n is %lld; the moments are taken over the top_n >= 2 largest scores of a row", top_n);
        return false;
    }
    if (!X) {
        why = "cohort selection: null argument (X, the cohort scores [rows][C])";
        return false;
    }
    return check_finite(X, rows * C, "X", why);
}

static Grid2 flat_grid(int64_t n) { return Grid2{(n + NORM_WG - 1) / NORM_WG, 1}; }

bool plan_score_norm(int mode, int64_t J, int64_t T, int64_t Cz, int64_t Ct, int top_n, int64_t scratch_bytes, int n_cu, NormPlan &p,
                     std::string &why) {
    p = NormPlan();
    if (!norm_check_shape(mode, J, T, Cz, Ct, top_n, why)) return false;
    if (n_cu < 1) {
        why = "score normalisation: the plan needs the number of compute units";
        return false;
    }
    const bool enrol = norm_needs_enrol(mode), test = norm_needs_test(mode), adaptive = norm_mode_adaptive(mode);
    if (!enrol) Cz = 0;
    if (!test) Ct = 0;
    p.mode = mode;
    p.n_sel = adaptive ? std::min<int64_t>(top_n, Cz) : Cz;
    p.n_sel_test = adaptive ? std::min<int64_t>(top_n, Ct) : Ct;
    p.bytes_S = p.bytes_out = J * T * 8;
    p.bytes_Ez = J * Cz * 8;
    p.bytes_Tt = Ct * T * 8;
    p.bytes_Zt = norm_needs_zt(mode) ? Ct * Cz * 8 : 0;
    p.bytes_tnorm = norm_needs_zt(mode) ? p.bytes_Tt : 0;
    const int64_t moment = 2 * 8 + 4;          // mu, sigma, flag
    p.bytes_moments = ((enrol ? J : 0) + (test ? T : 0) + (norm_needs_zt(mode) ? Ct : 0)) * moment;
    p.chunk = T;
    if (mode == NORM_AS2) {
        const int64_t C = Cz;
        p.fixed_bytes = 3 * J * C * 8;
        p.seg_bytes = (3 * C + 4 * J) * 8;
        p.chunk = scratch_bytes < p.fixed_bytes + p.seg_bytes ? 0 : std::min(T, (scratch_bytes - p.fixed_bytes) / p.seg_bytes);
        if (p.chunk < 1) {
            char buf[400];
            snprintf(buf, sizeof buf, "score normalisation: the scratch bound of %lld bytes is below one chunk of %lld bytes (the selection and the "
                     "shifted copies of Ez, 3 J C doubles, and one test segment's 3 C + 4 J); raise the option norm_scratch_mib or normalise fewer "
                     "models at a time", (long long)scratch_bytes, (long long)(p.fixed_bytes + p.seg_bytes));
            why = buf;
            return false;
        }
        p.bytes_scratch = p.fixed_bytes + p.chunk * p.seg_bytes;
        p.shift_enrol = flat_grid(J * C);
        p.shift_test = flat_grid(p.chunk * C);
        p.gemm_enrol = p.gemm_test = dense_gemm_grid(J, p.chunk);
        p.gemm_lds = dense_gemm_lds_bytes();
    }
    p.n_chunks = (T + p.chunk - 1) / p.chunk;
    if (enrol) {
        p.select_enrol = Grid2{J, 1};
        p.select_lds_enrol = norm_select_lds_bytes(Cz);
    }
    if (test) {
        p.select_test = Grid2{p.chunk, 1};
        p.select_lds_test = norm_select_lds_bytes(Ct);
    }
    if (norm_needs_zt(mode)) p.select_zt = Grid2{Ct, 1};
    p.apply = Grid2{J, (p.chunk + NORM_WG - 1) / NORM_WG};
    p.bytes_counts = mode == NORM_AS2 ? 2 * 4 * p.apply.x * p.apply.y : 0;
    const int64_t widest = std::max(std::max(p.select_enrol.x, p.select_test.x), p.select_zt.x);
    p.select_rounds = (widest + n_cu - 1) / n_cu;
    return true;
}

}  // namespace sr
