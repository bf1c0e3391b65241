// eig_checks.cpp -- the decisions of csrc/eig_plan.cpp under the host sanitizers (tests/test_eig_cpu.py builds this with
// -fsanitize=address,undefined and runs it): every refusal's text, and the plan swept over every R of 1 .. 512 and several device
// sizes -- the blocks cover the columns exactly once, the phantom makes their number even, every pair of blocks meets exactly once
// per sweep, no block appears twice in a round, exactly one pair of a round holds the phantom when there is one, the LDS bytes fit
// the device, the scorer's chunks cover the segments exactly once under the bound.  Host code only: no GPU, nothing loaded into Python.
#include "eig_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

using namespace sr;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            failures++;                                                      \
        }                                                                    \
    } while (0)

static bool has(const std::string &why, const char *needle) {
    if (why.find(needle) != std::string::npos) return true;
    std::printf("refusal text '%s' lacks '%s'\n", why.c_str(), needle);
    return false;
}

static void check_plan(int R, int n_cu) {
    EigPlan p;
    std::string why;
    CHECK(plan_eig(R, n_cu, p, why));
    CHECK(p.R == R && p.b == EIG_B && p.blocks == (R + EIG_B - 1) / EIG_B && p.phantom == p.blocks % 2);
    CHECK(p.single == (R <= 2 * EIG_B ? 1 : 0) && p.max_sweeps == 40 && p.pairs == (p.blocks + p.phantom) / 2);
    CHECK(p.solve_lds <= 160 * 1024 && p.update_lds <= 160 * 1024 && p.solve_lds >= 2 * EIG_N * EIG_N * 8);
    if (p.single) {
        CHECK(p.rounds == 0 && p.schedule.empty() && p.solve_grid == 1 && p.launches_per_sweep == 0);
        return;
    }
    const int players = p.blocks + p.phantom;
    CHECK(p.rounds == players - 1 && (int)p.schedule.size() == p.rounds * p.pairs);
    CHECK(p.solve_grid == p.pairs - p.phantom && p.cols_x == p.solve_grid && p.rows_x == p.solve_grid && p.cols_z == 2);
    CHECK(p.cols_y == (R + EIG_TILE_ROWS - 1) / EIG_TILE_ROWS && p.rows_y == p.cols_y && p.launches_per_sweep == 3 * p.rounds + 2);
    CHECK(p.pair_rounds == (p.cols_x * p.cols_y * p.cols_z + n_cu - 1) / n_cu && p.bytes_work > 2 * (int64_t)R * R * 8);
    std::vector<int> met((size_t)players * players, 0);
    for (int r = 0; r < p.rounds; r++) {
        std::vector<char> seen((size_t)players, 0);
        int phantoms = 0;
        for (int k = 0; k < p.pairs; k++) {
            const EigPair &e = p.schedule[(size_t)r * p.pairs + k];
            CHECK(e.p >= 0 && e.p < e.q && e.q < players);
            if (e.p < 0 || e.q >= players) continue;
            CHECK(!seen[(size_t)e.p] && !seen[(size_t)e.q]);                 // no block twice in a round
            seen[(size_t)e.p] = seen[(size_t)e.q] = 1;
            met[(size_t)e.p * players + e.q]++;
            phantoms += e.q >= p.blocks ? 1 : 0;
            CHECK(e.p < p.blocks);                                           // the phantom is never the first of a pair
        }
        CHECK(phantoms == p.phantom);
    }
    for (int a = 0; a < players; a++)
        for (int b = a + 1; b < players; b++) CHECK(met[(size_t)a * players + b] == 1);      // every pair exactly once per sweep
}

int main() {
    std::string why;
    EigPlan p;
    // the refusals
    CHECK(!plan_eig(0, 256, p, why) && has(why, "R >= 1"));
    CHECK(!plan_eig(-3, 256, p, why) && has(why, "R >= 1"));
    CHECK(!plan_eig(513, 256, p, why) && has(why, "up to 512 rows, this one has 513; reduce the dimension"));
    CHECK(!plan_eig(std::numeric_limits<int>::max(), 256, p, why) && has(why, "up to 512 rows"));
    CHECK(!plan_eig(5, 0, p, why) && has(why, "compute units"));
    const double good[4] = {2.0, 0.5, 0.5, 1.0}, skew[4] = {2.0, 0.5, 0.1, 1.0};
    const double nan2[4] = {2.0, 0.5, std::nan(""), 1.0};
    CHECK(eig_check_matrix(good, 2, "A", why));
    CHECK(!eig_check_matrix(nullptr, 2, "A", why) && has(why, "null argument (A [R][R])"));
    CHECK(!eig_check_matrix(good, 0, "A", why) && has(why, "R >= 1"));
    CHECK(!eig_check_matrix(skew, 2, "Sb", why) && has(why, "Sb is not symmetric") && has(why, "pass (Sb + Sb^T) / 2"));
    CHECK(!eig_check_matrix(nan2, 2, "Sw", why) && has(why, "Sw holds a non-finite value at element 2"));
    CHECK(!lda_check_dims(0, 5, 4, why) && has(why, "P, the dimensions kept, is 0") && has(why, "1 <= P <= min(R, classes - 1)"));
    CHECK(!lda_check_dims(4, 5, 4, why) && has(why, "rank at most 3"));
    CHECK(!lda_check_dims(6, 5, 40, why) && has(why, "rank at most 5"));
    CHECK(!lda_check_dims(1, 5, 1, why) && has(why, "rank at most 0"));
    CHECK(lda_check_dims(3, 5, 4, why) && lda_check_dims(5, 5, 40, why) && lda_check_dims(1, 1, 2, why));
    // psi
    const double psi_ok[3] = {4.0, 1.0, -1e-12}, psi_neg[3] = {4.0, 1.0, -1e-3}, psi_inf[3] = {4.0, std::numeric_limits<double>::infinity(), 1.0};
    const double zeros[3] = {0.0, 0.0, 0.0};
    CHECK(diag_psi_usable(psi_ok, 3) && !diag_psi_usable(psi_neg, 3) && !diag_psi_usable(psi_inf, 3) && diag_psi_usable(zeros, 3));
    // the plan at every size and a few device sizes
    for (int R = 1; R <= PLDA_MAX_R; R++)
        for (int n_cu : {1, 64, 256}) check_plan(R, n_cu);
    CHECK(plan_eig(200, 256, p, why) && p.blocks == 7 && p.phantom == 1 && p.rounds == 7 && p.pairs == 4 && p.solve_grid == 3);
    CHECK(plan_eig(512, 256, p, why) && p.blocks == 16 && p.phantom == 0 && p.rounds == 15 && p.pairs == 8 && p.launches_per_sweep == 47);
    CHECK(EIG_MAX_BLOCKS == 16);
    // the round robin on its own: n = 2 .. 64 players
    for (int n = 2; n <= 64; n += 2) {
        std::vector<int> met((size_t)n * n, 0);
        for (int r = 0; r < n - 1; r++)
            for (int k = 0; k < n / 2; k++) {
                const EigPair e = eig_round_robin(n, r, k);
                CHECK(e.p >= 0 && e.p < e.q && e.q < n);
                if (e.p >= 0 && e.q < n) met[(size_t)e.p * n + e.q]++;
            }
        for (int a = 0; a < n; a++)
            for (int b = a + 1; b < n; b++) CHECK(met[(size_t)a * n + b] == 1);
    }
    // the scorer's chunks
    DiagChunks c;
    for (int R : {1, 5, 65, 400, 512})
        for (int64_t nc : {1, 7, 100})
            for (int64_t T : {(int64_t)1, (int64_t)1000, (int64_t)100000}) {
                const int64_t seg = (2 * (int64_t)R + nc + 1) * 8;
                for (int64_t bound : {seg, 3 * seg + 5, (int64_t)1 << 20, (int64_t)1 << 30}) {
                    CHECK(plan_diag_chunks(T, R, nc, bound, c, why));
                    CHECK(c.seg_bytes == seg && c.chunk == std::min(T, bound / seg) && c.chunk >= 1 && c.bytes_scratch <= bound);
                    CHECK(c.n_chunks == (T + c.chunk - 1) / c.chunk && (c.n_chunks - 1) * c.chunk < T);
                }
                CHECK(!plan_diag_chunks(T, R, nc, seg - 1, c, why) && has(why, "raise the option plda_scratch_mib"));
                CHECK(!plan_diag_chunks(T, R, nc, 0, c, why));
            }
    CHECK(plan_diag_chunks(1000, 65, 5, 1 << 20, c, why) && c.n_chunks == 2);
    if (failures) {
        std::printf("%d eig check(s) failed\n", failures);
        return 1;
    }
    std::printf("eig checks ok\n");
    return 0;
}
