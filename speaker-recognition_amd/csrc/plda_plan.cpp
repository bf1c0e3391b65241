// plda_plan.cpp -- the decisions of the i-vector back end (plda_plan.hpp); the GEMM's grids, the factorisation's path and their LDS
// bytes are the dense layer's (dense64_plan.hpp).  Host-only.
#include "plda_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>

namespace sr {

static std::string fmt(const char *f, long long a = 0, long long b = 0, long long c = 0) {
    char buf[400];
    snprintf(buf, sizeof buf, f, a, b, c);
    return buf;
}

bool plda_check_rank(int R, std::string &why) {
    if (R < 1) {
        why = "PLDA back end: the vectors need at least one dimension (R >= 1)";
        return false;
    }
    if (R > PLDA_MAX_R) {
        why = fmt("PLDA back end is built for vectors of up to %lld dimensions, these have %lld; extract fewer factors", PLDA_MAX_R, R);
        return false;
    }
    return true;
}

bool plda_check_rows(int64_t n, const char *what, std::string &why) {
    char buf[320];
    if (n < 1) {
        snprintf(buf, sizeof buf, "PLDA back end: %s is %lld; pass at least one row", what, (long long)n);
        why = buf;
        return false;
    }
    if (n > PLDA_MAX_ROWS) {
        snprintf(buf, sizeof buf, "PLDA back end: %s is %lld, more than the %lld rows of one call; split the list", what, (long long)n,
                 (long long)PLDA_MAX_ROWS);
        why = buf;
        return false;
    }
    return true;
}

bool plda_check_finite(const double *v, int64_t n, const char *what, std::string &why) {
    for (int64_t i = 0; i < n; i++)
        if (!std::isfinite(v[i])) {
            char buf[256];
            snprintf(buf, sizeof buf, "PLDA back end: %s holds a non-finite value at element %lld; drop that vector", what, (long long)i);
            why = buf;
            return false;
        }
    return true;
}

bool plda_check_symmetric(const double *M, int R, const char *what, std::string &why) {
    if (!plda_check_finite(M, (int64_t)R * R, what, why)) return false;
    double scale = 0.0;
    for (int i = 0; i < R; i++) scale = std::max(scale, std::fabs(M[(int64_t)i * R + i]));
    for (int i = 0; i < R; i++)
        for (int j = 0; j < i; j++)
            if (std::fabs(M[(int64_t)i * R + j] - M[(int64_t)j * R + i]) > 1e-9 * scale) {
                char buf[320];
                snprintf(buf, sizeof buf, "PLDA back end: %s is not symmetric (elements [%d][%d] and [%d][%d] differ); a covariance is: "
                         "pass (%s + %s^T) / 2", what, i, j, j, i, what, what);
                why = buf;
                return false;
            }
    return true;
}

bool plda_check_labels(const int64_t *ids, int64_t n, int64_t S, std::string &why) {
    if (!ids) {
        why = "PLDA training: null argument (ids, one 0-based speaker label per row of X)";
        return false;
    }
    if (S < 1 || S > n) {
        why = fmt("PLDA training: the number of labels is %lld for %lld rows; labels run 0 .. S - 1 and every one has a row (1 <= S <= n)", S, n);
        return false;
    }
    std::vector<char> seen((size_t)S, 0);
    for (int64_t i = 0; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= S) {
            why = fmt("PLDA training: row %lld has label %lld, outside 0 .. %lld; renumber the speakers 0 .. S - 1", i, ids[i], S - 1);
            return false;
        }
        seen[(size_t)ids[i]] = 1;
    }
    for (int64_t s = 0; s < S; s++)
        if (!seen[(size_t)s]) {
            why = fmt("PLDA training: label %lld of 0 .. %lld has no row; renumber the speakers that occur 0 .. S - 1", s, S - 1);
            return false;
        }
    return true;
}

bool plda_check_enrol(const int64_t *enrol_n, int64_t J, std::string &why) {
    if (!enrol_n) {
        why = "PLDA scoring: null argument (enrol_n, the number of enrolment vectors of each model)";
        return false;
    }
    for (int64_t j = 0; j < J; j++)
        if (enrol_n[j] < 1 || enrol_n[j] > ((int64_t)1 << 40)) {
            why = fmt("PLDA scoring: enrol_n of model %lld is %lld; a model is enrolled from at least one vector (enrol_n >= 1)", j, enrol_n[j]);
            return false;
        }
    return true;
}

static Grid2 flat_grid(int64_t n) { return Grid2{(n + PLDA_WG - 1) / PLDA_WG, 1}; }

static bool check_common(int R, int lds_rows, int n_cu, std::string &why) {
    if (!plda_check_rank(R, why)) return false;
    if (!dense_check_lds_rows(lds_rows, why)) return false;
    if (n_cu < 1) {
        why = "PLDA back end: the plan needs the number of compute units";
        return false;
    }
    return true;
}

// Sorts the groups by (count, index), fills perm and the classes; returns the widest class.
static int64_t sort_by_count(const std::vector<int64_t> &count, PldaPlan &p) {
    const int64_t G = (int64_t)count.size();
    p.perm.resize((size_t)G);
    std::iota(p.perm.begin(), p.perm.end(), (int64_t)0);
    std::stable_sort(p.perm.begin(), p.perm.end(), [&](int64_t a, int64_t b) { return count[(size_t)a] < count[(size_t)b]; });
    int64_t widest = 0;
    for (int64_t s = 0; s < G; s++) {
        const int64_t c = count[(size_t)p.perm[(size_t)s]];
        if (p.classes.empty() || p.classes.back().count != c) p.classes.push_back(PldaClass{c, s, 0});
        widest = std::max(widest, ++p.classes.back().size);
    }
    return widest;
}

static void fill_paths(int R, int lds_rows, PldaPlan &p) {
    p.R = R;
    p.lds_rows = dense_lds_limit(lds_rows);
    p.path = R <= p.lds_rows ? 0 : 1;
    p.factor_lds = dense_factor_lds_bytes(R, p.path, 1);
    p.gemm_lds = dense_gemm_lds_bytes();
}

bool plan_plda_train(int64_t n, int R, const int64_t *ids, int64_t S, int lds_rows, int n_cu, PldaPlan &p, std::string &why) {
    p = PldaPlan();
    if (!check_common(R, lds_rows, n_cu, why) || !plda_check_rows(n, "n, the number of training vectors", why)) return false;
    if (!plda_check_labels(ids, n, S, why)) return false;
    p.kind = PLDA_TRAIN;
    p.rows = n;
    p.groups = S;
    fill_paths(R, lds_rows, p);
    std::vector<int64_t> count((size_t)S, 0);
    for (int64_t i = 0; i < n; i++) count[(size_t)ids[i]]++;
    const int64_t widest = sort_by_count(count, p);
    // the rows in the order of their speaker's sorted position: a counting sort, a speaker's rows in ascending order
    std::vector<int64_t> pos((size_t)S);
    for (int64_t s = 0; s < S; s++) pos[(size_t)p.perm[(size_t)s]] = s;
    p.row_start.assign((size_t)S + 1, 0);
    for (int64_t s = 0; s < S; s++) p.row_start[(size_t)s + 1] = p.row_start[(size_t)s] + count[(size_t)p.perm[(size_t)s]];
    p.row_order.resize((size_t)n);
    std::vector<int64_t> next(p.row_start.begin(), p.row_start.end() - 1);
    for (int64_t i = 0; i < n; i++) p.row_order[(size_t)next[(size_t)pos[(size_t)ids[i]]]++] = i;
    p.sum_chunk = std::min(n, PLDA_SUM_CHUNK);
    p.sum_chunks = (n + p.sum_chunk - 1) / p.sum_chunk;
    p.grp_chunk = std::min(S, PLDA_SUM_CHUNK);
    p.grp_chunks = (S + p.grp_chunk - 1) / p.grp_chunk;
    const int64_t rr = (int64_t)R * R, nc = (int64_t)p.classes.size();
    p.bytes_blocks = (9 + nc) * rr * 8;
    p.bytes_rows = (2 * n + 4 * S) * R * 8;
    p.centre = flat_grid(n * R);
    p.class_sums = Grid2{S, (R + PLDA_WG - 1) / PLDA_WG};
    p.invert = Grid2{std::max<int64_t>(2, nc), 1};
    p.gemm_rows = dense_gemm_grid(std::max(widest, p.grp_chunk), R);
    p.gemm_acc = dense_gemm_grid(R, R);
    if (p.path == 1) p.tri = Grid2{p.invert.x, (R + PLDA_ROWS_PER_WG - 1) / PLDA_ROWS_PER_WG};
    p.invert_rounds = (p.invert.x + n_cu - 1) / n_cu;
    return true;
}

bool plan_plda_score(int64_t J, int64_t T, int R, const int64_t *enrol_n, int64_t scratch_bytes, int lds_rows, int n_cu, PldaPlan &p,
                     std::string &why) {
    p = PldaPlan();
    if (!check_common(R, lds_rows, n_cu, why)) return false;
    if (!plda_check_rows(J, "J, the number of models", why) || !plda_check_rows(T, "T, the number of test segments", why)) return false;
    if (J > (((int64_t)1 << 36) / T)) {
        why = "PLDA scoring: a score matrix of more than 2^36 values; split the trial list";
        return false;
    }
    if (!plda_check_enrol(enrol_n, J, why)) return false;
    p.kind = PLDA_SCORE;
    p.rows = p.groups = J;
    p.T = T;
    fill_paths(R, lds_rows, p);
    const int64_t widest = sort_by_count(std::vector<int64_t>(enrol_n, enrol_n + J), p);
    p.seg_bytes = (2 * (int64_t)R + 2) * 8;
    p.chunk = scratch_bytes < p.seg_bytes ? 0 : std::min(T, scratch_bytes / p.seg_bytes);
    if (p.chunk < 1) {
        why = fmt("PLDA scoring: the scratch bound of %lld bytes is below one chunk of %lld bytes (a test segment's centred row, its row of "
                  "X P_c and its two quadratic forms); raise the option plda_scratch_mib", scratch_bytes, p.seg_bytes);
        return false;
    }
    p.n_chunks = (T + p.chunk - 1) / p.chunk;
    p.bytes_scratch = p.chunk * p.seg_bytes;
    const int64_t rr = (int64_t)R * R, nc = (int64_t)p.classes.size();
    p.bytes_blocks = (5 + 2 * nc) * rr * 8;
    p.bytes_rows = (4 * J * R + J * T + J) * 8;
    p.centre = flat_grid(std::max(J, p.chunk) * R);
    p.invert = Grid2{std::max<int64_t>(2, nc + 1), 1};
    p.gemm_rows = dense_gemm_grid(std::max(widest, p.chunk), R);
    p.rowdot = Grid2{(std::max(J, p.chunk) + PLDA_ROWS_PER_WG - 1) / PLDA_ROWS_PER_WG, 1};
    p.gemm_cross = dense_gemm_grid(widest, p.chunk);
    p.assemble = flat_grid(widest * p.chunk);
    if (p.path == 1) p.tri = Grid2{p.invert.x, (R + PLDA_ROWS_PER_WG - 1) / PLDA_ROWS_PER_WG};
    p.invert_rounds = (p.invert.x + n_cu - 1) / n_cu;
    return true;
}

}  // namespace sr
