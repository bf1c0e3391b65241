// calib_plan.cpp -- the decisions of score calibration (calib_plan.hpp).  Host-only.
#include "calib_plan.hpp"

#include <cmath>
#include <cstdio>

namespace sr {

static std::string fmt(const char *f, long long a = 0, long long b = 0, long long c = 0) {
    char buf[480];
    snprintf(buf, sizeof buf, f, a, b, c);
    return buf;
}

const char *calib_stop_name(int code) {
    static const char *names[4] = {"CONVERGED", "CAP", "SINGULAR", "STALLED"};
    return code >= 0 && code < 4 ? names[code] : "?";
}

bool calib_check_shape(int S, int64_t n, std::string &why) {
    if (S < 1 || S > CALIB_MAX_S) {
        why = fmt("calibration is built for up to %lld systems (the pass kernel keeps f, g and H in registers), S is %lld; fuse in two stages "
                  "or drop a system", CALIB_MAX_S, S);
        return false;
    }
    if (n < 1) {
        why = fmt("calibration: n is %lld; need at least one trial (n >= 1)", n);
        return false;
    }
    if (n > CALIB_MAX_N) {
        why = fmt("calibration: n is %lld, more than 2^35 trials in one call; split the trial list", n);
        return false;
    }
    return true;
}

bool calib_check_params(double prior, double ridge, double tol, int max_pass, std::string &why) {
    char buf[320];
    if (!(prior > 0.0 && prior < 1.0)) {
        snprintf(buf, sizeof buf, "calibration: the prior is %g; it is a probability strictly inside (0, 1)", prior);
        why = buf;
        return false;
    }
    if (!(ridge >= 0.0) || !std::isfinite(ridge)) {
        snprintf(buf, sizeof buf, "calibration: the ridge is %g; it is a finite value >= 0 (0 switches it off)", ridge);
        why = buf;
        return false;
    }
    if (!(tol >= 0.0)) {
        snprintf(buf, sizeof buf, "calibration: tol is %g; the Newton decrement is compared with a value >= 0", tol);
        why = buf;
        return false;
    }
    if (max_pass < 1 || max_pass > CALIB_MAX_PASS) {
        why = fmt("calibration: max_pass is %lld; a call makes 1 .. %lld passes (resume from its state for more)", max_pass, CALIB_MAX_PASS);
        return false;
    }
    return true;
}

bool calib_check_trials(int S, int64_t n, const double *X, const int8_t *lab, CalibCounts &c, std::string &why) {
    c = CalibCounts();
    if (!lab) {
        why = "calibration: null argument (lab, the labels [n]: 1 target, 0 non-target, negative not a trial)";
        return false;
    }
    for (int64_t i = 0; i < n; i++) {
        const int l = lab[i];
        if (l > 1) {
            why = fmt("calibration: label %lld is %lld; a label is 1 (target), 0 (non-target) or negative (not a trial)", i, l);
            return false;
        }
        if (l < 0) {
            c.n_skip++;
            continue;
        }
        (l ? c.n_t : c.n_n)++;
        if (X)
            for (int s = 0; s < S; s++)
                if (!std::isfinite(X[(int64_t)s * n + i])) {
                    why = fmt("calibration: system %lld holds a non-finite score at trial %lld; mark that trial as skipped (a negative label) "
                              "or drop it", s, i);
                    return false;
                }
    }
    if (c.n_t < 1 || c.n_n < 1) {
        why = fmt("calibration: %lld targets and %lld non-targets; need at least one trial of each class", c.n_t, c.n_n);
        return false;
    }
    return true;
}

bool calib_check_theta(int S, const double *theta, const char *name, std::string &why) {
    for (int s = 0; s <= S; s++)
        if (!std::isfinite(theta[s])) {
            char buf[256];
            snprintf(buf, sizeof buf, "calibration: %s holds a non-finite value at element %d (S weights, then the offset)", name, s);
            why = buf;
            return false;
        }
    return true;
}

bool calib_check_thresholds(int m, const double *thr, std::string &why) {
    if (m < 1 || m > CALIB_MAX_THR) {
        why = fmt("calibration: %lld thresholds; one counts call takes 1 .. %lld of them", m, CALIB_MAX_THR);
        return false;
    }
    if (!thr) {
        why = "calibration: null argument (thr, the thresholds [m])";
        return false;
    }
    for (int j = 0; j < m; j++)
        if (std::isnan(thr[j])) {
            why = fmt("calibration: threshold %lld is a NaN (-inf and +inf are thresholds, a NaN is not)", j);
            return false;
        }
    return true;
}

bool plan_calib(int S, int64_t n, int n_thr, int64_t scratch_bytes, int n_cu, CalibPlan &p, std::string &why) {
    p = CalibPlan();
    if (!calib_check_shape(S, n, why)) return false;
    if (n_thr < 0 || n_thr > CALIB_MAX_THR) {
        why = fmt("calibration: %lld thresholds; one counts call takes 1 .. %lld of them", n_thr, CALIB_MAX_THR);
        return false;
    }
    if (n_cu < 1) {
        why = "calibration: the plan needs the number of compute units";
        return false;
    }
    (void)scratch_bytes;        // nothing of the plan depends on the bound: it refuses or it does not (calib_check_bound)
    p.S = S;
    p.n = n;
    p.acc = calib_acc(S);
    p.state_len = calib_state_len(S);
    p.n_blocks = (n + CALIB_BLOCK - 1) / CALIB_BLOCK;
    p.bytes_X = (int64_t)S * n * 8;
    p.bytes_lab = n;
    p.bytes_partial = p.n_blocks * p.acc * 8;
    p.bytes_state = (int64_t)p.state_len * 8;
    p.bytes_out = n * 8;
    p.bytes_thr = (int64_t)CALIB_MAX_THR * 8;
    p.bytes_counts = p.n_blocks * 2 * CALIB_MAX_THR * 4;
    p.resident_train = p.bytes_X + p.bytes_lab + p.bytes_partial + p.bytes_state;
    p.resident_apply = p.bytes_X + p.bytes_out + (int64_t)(S + 1) * 8;
    p.resident_counts = n * 8 + p.bytes_lab + p.bytes_thr + p.bytes_counts;
    p.pass_grid = p.counts_grid = p.apply_grid = p.n_blocks;
    p.step_grid = 1;
    p.pass_rounds = (p.n_blocks + n_cu - 1) / n_cu;
    return true;
}

bool calib_check_bound(const CalibPlan &p, const char *call, int64_t scratch_bytes, std::string &why) {
    const std::string c(call);
    const int64_t need = c == "apply" ? p.resident_apply : c == "counts" ? p.resident_counts : p.resident_train;
    if (need <= scratch_bytes) return true;
    char buf[480];
    snprintf(buf, sizeof buf, "calibration (%s): the arrays resident on the device take %lld bytes (%d system(s) x %lld trials), the bound is "
             "%lld bytes; raise the option calib_scratch_mib or calibrate on fewer trials at a time", call, (long long)need, p.S, (long long)p.n,
             (long long)scratch_bytes);
    why = buf;
    return false;
}

}  // namespace sr
