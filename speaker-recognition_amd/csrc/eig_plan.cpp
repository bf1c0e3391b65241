// eig_plan.cpp -- the decisions of the symmetric eigen-solver and of the diagonalised scorer (eig_plan.hpp).  Host-only.
#include "eig_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>

namespace sr {

bool eig_check_rank(int R, std::string &why) {
    char buf[320];
    if (R < 1) {
        why = "eigen-solver: the matrix needs at least one row (R >= 1)";
        return false;
    }
    if (R > PLDA_MAX_R) {
        snprintf(buf, sizeof buf, "eigen-solver is built for matrices of up to %d rows, this one has %d; reduce the dimension (extract fewer factors)",
                 PLDA_MAX_R, R);
        why = buf;
        return false;
    }
    return true;
}

bool eig_check_matrix(const double *A, int R, const char *what, std::string &why) {
    if (!eig_check_rank(R, why)) return false;
    if (!A) {
        why = std::string("eigen-solver: null argument (") + what + " [R][R])";
        return false;
    }
    return plda_check_symmetric(A, R, what, why);
}

EigPair eig_round_robin(int n, int r, int slot) {
    const int m = n - 1;
    int a = slot == 0 ? r : (r + slot) % m, b = slot == 0 ? m : (r + m - slot) % m;
    if (a > b) std::swap(a, b);
    return EigPair{a, b};
}

bool plan_eig(int R, int n_cu, EigPlan &p, std::string &why) {
    p = EigPlan();
    if (!eig_check_rank(R, why)) return false;
    if (n_cu < 1) {
        why = "eigen-solver: the plan needs the number of compute units";
        return false;
    }
    p.R = R;
    p.blocks = (R + EIG_B - 1) / EIG_B;
    p.single = R <= EIG_N ? 1 : 0;
    p.phantom = p.blocks % 2;
    const int players = p.blocks + p.phantom;
    p.pairs = players / 2;
    p.solve_lds = (2 * EIG_N * EIG_LD + 5 * EIG_B + EIG_WG) * (int)sizeof(double);
    p.update_lds = (EIG_N * EIG_LD + EIG_TILE_ROWS * EIG_LD) * (int)sizeof(double);
    const int64_t rr = (int64_t)R * R;
    if (p.single) {                            // the whole matrix is one sub-problem: no rounds, no table
        p.solve_grid = 1;
        p.launches_per_sweep = 0;
        p.bytes_work = 2 * rr * 8;
        p.pair_rounds = 1;
        return true;
    }
    p.rounds = players - 1;
    p.schedule.resize((size_t)p.rounds * p.pairs);
    for (int r = 0; r < p.rounds; r++)
        for (int s = 0; s < p.pairs; s++) p.schedule[(size_t)r * p.pairs + s] = eig_round_robin(players, r, s);
    const int64_t working = p.pairs - p.phantom, tiles = (R + EIG_TILE_ROWS - 1) / EIG_TILE_ROWS;
    p.solve_grid = working;
    p.cols_x = working, p.cols_y = tiles, p.cols_z = 2;
    p.rows_x = working, p.rows_y = tiles;
    p.launches_per_sweep = 3 * (int64_t)p.rounds + 2;
    p.bytes_work = 2 * rr * 8 + (int64_t)p.pairs * EIG_N * EIG_N * 8 + (int64_t)p.rounds * p.pairs * 2 * 4 + (int64_t)R * 8;
    p.pair_rounds = (p.cols_x * p.cols_y * p.cols_z + n_cu - 1) / n_cu;
    return true;
}

bool plan_diag_chunks(int64_t T, int R, int64_t n_classes, int64_t scratch_bytes, DiagChunks &c, std::string &why) {
    c = DiagChunks();
    c.seg_bytes = (2 * (int64_t)R + n_classes + 1) * 8;
    c.chunk = scratch_bytes < c.seg_bytes ? 0 : std::min(T, scratch_bytes / c.seg_bytes);
    if (c.chunk < 1) {
        char buf[400];
        snprintf(buf, sizeof buf, "diagonalised PLDA scoring: the scratch bound of %lld bytes is below one chunk of %lld bytes (a test segment's "
                 "centred row, its row of U and its quadratic forms); raise the option plda_scratch_mib", (long long)scratch_bytes,
                 (long long)c.seg_bytes);
        why = buf;
        return false;
    }
    c.n_chunks = (T + c.chunk - 1) / c.chunk;
    c.bytes_scratch = c.chunk * c.seg_bytes;
    return true;
}

bool lda_check_dims(int P, int R, int64_t n_labels, std::string &why) {
    const int64_t top = std::min<int64_t>(R, n_labels - 1);
    if (P < 1 || P > top) {
        char buf[400];
        snprintf(buf, sizeof buf, "LDA: P, the dimensions kept, is %d; the between-class covariance of %lld classes in %d dimensions has rank "
                 "at most %lld: pass 1 <= P <= min(R, classes - 1)", P, (long long)n_labels, R, (long long)std::max<int64_t>(top, 0));
        why = buf;
        return false;
    }
    return true;
}

bool diag_psi_usable(const double *psi, int R) {
    double top = 0.0;
    for (int d = 0; d < R; d++) {
        if (!std::isfinite(psi[d])) return false;
        top = std::max(top, std::fabs(psi[d]));
    }
    for (int d = 0; d < R; d++)
        if (psi[d] < -1e-9 * top) return false;
    return true;
}

}  // namespace sr
