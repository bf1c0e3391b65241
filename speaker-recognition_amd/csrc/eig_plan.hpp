// eig_plan.hpp -- what the float64 symmetric eigen-solver (eig.hip: two-sided block Jacobi) and the diagonalised PLDA scorer
// (backend_eig.hip) decide before they touch the device: the refusals, the cut of the R columns into blocks of EIG_B, the phantom
// block that makes their number even, the round-robin tournament of a sweep as a table (every pair of blocks meets once, no block
// twice in a round), the launch shapes and the LDS bytes -- as a pure function of R and the number of compute units.
// Host-only C++17, nothing of HIP: eig.hip consumes it, sr_eig_plan hands it to tests, tests/host/eig_checks.cpp runs it under the
// host sanitizers.
#pragma once

#include "plda_plan.hpp"

#include <cstdint>
#include <string>
#include <vector>

namespace sr {

constexpr int EIG_B = 32;                       // columns of a block: a pair's 64 x 64 sub-problem and its rotation Q, 2 x 32.5 KiB of LDS
constexpr int EIG_N = 2 * EIG_B;                // the largest sub-problem, and the largest R of the single-launch path
constexpr int EIG_LD = EIG_N + 1;               // row stride of the sub-problem and of Q in LDS (odd: a column walks over the banks)
constexpr int EIG_WG = 256;
constexpr int EIG_MAX_SWEEPS = 40;              // the cap: reached, the call returns what it has with converged = 0
// Inner sweeps of a pair's sub-problem inside one round (multi-block path).  The sub-problem need not be solved: with 2, 3, 4 or 15 the
// numpy model of the sweep (tests/eig_cases.py) takes the same number of outer sweeps, give or take one (R = 65 .. 200, condition 10
// and 1e6, indefinite, multiple eigenvalues), and a round with 15 measured 1.2 ms on the device against 0.84 ms with 3.
constexpr int EIG_INNER_SWEEPS = 3;
constexpr int EIG_TILE_ROWS = 64;               // rows (columns) of A or V that one workgroup of an update stage takes through a pair's Q
constexpr int EIG_MAX_BLOCKS = (PLDA_MAX_R + EIG_B - 1) / EIG_B;

struct EigPair {
    int p = 0, q = 0;               // block indices, p < q; q == the phantom's index: the pair does no work and is not launched
};

struct EigPlan {
    int R = 0;
    int b = EIG_B;
    int blocks = 0;                 // ceil(R / b): the last may be narrower
    int phantom = 0;                // 1: an empty block (index `blocks`) makes the number even
    int rounds = 0;                 // rounds of a sweep: blocks + phantom - 1 (0 on the single-launch path)
    int pairs = 0;                  // pairs of a round, a phantom pair included: (blocks + phantom) / 2
    int single = 0;                 // 1: R <= 2 b, the first stage alone is the solver, in one launch
    int max_sweeps = EIG_MAX_SWEEPS, inner_sweeps = EIG_INNER_SWEEPS;
    int solve_lds = 0;              // bytes: the sub-problem, Q, the rotations of a step, the reduction's lanes
    int update_lds = 0;             // bytes: Q and a tile
    int64_t solve_grid = 0;         // workgroups of a round's first stage: the pairs that work (the fewest over the rounds: a phantom round has one less)
    int64_t cols_x = 0, cols_y = 0, cols_z = 0;   // the column stage: (working pairs, row tiles, A and V)
    int64_t rows_x = 0, rows_y = 0;               // the row stage: (working pairs, column tiles)
    int64_t launches_per_sweep = 0; // 3 per round and the two of the off-diagonal maximum
    int64_t bytes_work = 0;         // A's working copy, V, the Q of every pair, the tables
    int64_t pair_rounds = 0;        // rounds a stage's launch makes over the chip (ceil(widest grid / n_cu))
    std::vector<EigPair> schedule;  // [rounds][pairs], row-major
};

// The refusals; true, or false with the text (it names the remedy).
bool eig_check_rank(int R, std::string &why);                               // 1 .. PLDA_MAX_R
// A [R][R]: not null, finite, symmetric by plda_check_symmetric's rule.
bool eig_check_matrix(const double *A, int R, const char *what, std::string &why);
// The members of round r of the tournament of n (even) players: slot 0 is (r, n - 1), slot k is ((r + k) mod (n - 1), (r - k) mod (n - 1)).
EigPair eig_round_robin(int n, int r, int slot);
// Fill `p` and return true, or false with the reason.  n_cu: compute units (>= 1).
bool plan_eig(int R, int n_cu, EigPlan &p, std::string &why);

// The diagonalised scorer's chunks: a test segment takes its centred row, its row of U and its n_classes + 1 quadratic forms inside the
// bound (the option plda_scratch_mib).
struct DiagChunks {
    int64_t seg_bytes = 0, chunk = 0, n_chunks = 0, bytes_scratch = 0;
};
bool plan_diag_chunks(int64_t T, int R, int64_t n_classes, int64_t scratch_bytes, DiagChunks &c, std::string &why);
// LDA: 1 <= P <= min(R, n_labels - 1).
bool lda_check_dims(int P, int R, int64_t n_labels, std::string &why);
// psi [R]: a value that is not finite, or negative beyond rounding (below -1e-9 of the largest magnitude): false (no text: the scorer
// zeroes and counts); `(c + 1) psi_d + 1 <= 0` is the caller's, per class.
bool diag_psi_usable(const double *psi, int R);

}  // namespace sr
