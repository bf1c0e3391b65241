// plda_plan.hpp -- what the i-vector back end (plda.hip: centring, whitening, WCCN, length normalisation, cosine scoring, and the
// two-covariance Gaussian PLDA  x_ij = mu + y_i + e_ij,  y ~ N(0, Sb),  e ~ N(0, Sw),  both full R x R) decides before it touches the
// device: the refusals, the count classes (speakers, or models, with the same number of vectors share Phi_c = (Sb^-1 + c Sw^-1)^-1)
// and the permutation that sorts by count so that a class is a contiguous row range, the chunks of the sums and of the test
// segments, the factorisation path, the launch shapes -- as a pure function of the shapes, the labels or counts, the bound, the
// option jfa_lds_rows and the number of compute units.  The GEMM's grids, the factorisation's path and the LDS bytes of both come
// from the dense layer (dense64_plan.hpp); nothing of JFA's is needed here.
// Host-only C++17, nothing of HIP: plda.hip consumes it, sr_plda_plan hands it to tests, tests/host/plda_checks.cpp runs it under the
// host sanitizers.
#pragma once

#include "dense64_plan.hpp"

#include <cstdint>
#include <string>
#include <vector>

namespace sr {

constexpr int PLDA_MAX_R = DENSE_MAX_R;         // the factorisation is dense_cholesky's: its panel of 16 columns x R rows lives in LDS
constexpr int PLDA_WG = 256;                    // lanes of every workgroup of the path (plda.hip asserts it equal to the dense layer's)
constexpr int PLDA_ROWS_PER_WG = PLDA_WG / 64;  // the row kernels (dot products, normalisation): a wave per row
constexpr int64_t PLDA_SUM_CHUNK = 1 << 16;     // rows (vectors, or speakers) per launch of an accumulating product: a multiple of DENSE_KSTEP
constexpr int64_t PLDA_MAX_ROWS = (int64_t)65535 * DENSE_TILE;    // vectors, models or segments of one call (row tiles: the GEMM's grid y)
constexpr int64_t PLDA_DEFAULT_SCRATCH = (int64_t)1 << 30;
constexpr int PLDA_TRAIN = 0, PLDA_SCORE = 1;
constexpr int PLDA_WHITEN = 0, PLDA_WCCN = 1;
// sr_plda_train's stop codes: why the iterations ended where they did (the pair returned is the last one that factored).
constexpr int PLDA_STOP_NONE = 0, PLDA_STOP_SB = 1, PLDA_STOP_SW = 2, PLDA_STOP_PHI = 3, PLDA_STOP_NON_FINITE = 4;
static_assert(PLDA_SUM_CHUNK % DENSE_KSTEP == 0, "a chunk of a sum is whole reduction tiles");

// The groups (speakers of a training set, models of a trial list) with `count` vectors: `size` of them, at the sorted positions start ..
struct PldaClass {
    int64_t count = 0, start = 0, size = 0;
};

struct PldaPlan {
    int kind = 0, R = 0;
    int64_t rows = 0;               // training vectors n (train); models J (score)
    int64_t groups = 0;             // speakers S (train); models J (score)
    int64_t T = 0;                  // test segments (score)
    std::vector<PldaClass> classes; // ascending count
    std::vector<int64_t> perm;      // sorted position -> label (train) or model (score): by count, then by label -- stable
    std::vector<int64_t> row_order; // train: the rows of X in the order of their speaker's sorted position, a speaker's rows ascending
    std::vector<int64_t> row_start; // train: [groups + 1], the sorted speaker's rows are row_order[row_start[s] .. row_start[s + 1])
    int64_t sum_chunk = 0, sum_chunks = 0;      // train: vectors per launch of T2's product, and the launches
    int64_t grp_chunk = 0, grp_chunks = 0;      // train: speakers per launch of the products summed over speakers
    int64_t chunk = 0, n_chunks = 0;            // score: test segments per chunk
    int64_t seg_bytes = 0, bytes_scratch = 0;   // score, inside the bound: a segment's centred row, its row of X P_c, and its two quadratic forms
    int64_t bytes_blocks = 0;       // the R x R blocks: Sb, Sw, their inverses, T2 and the four sums (train); a Phi_c and a P_c per class
    int64_t bytes_rows = 0;         // the row arrays outside the bound: X, F, G, Yhat, n Yhat (train); E, G, Yhat, M and out (score)
    int path = 0, lds_rows = 0;     // factorisation: 0 whole block in LDS, 1 in place in global memory with panels in LDS (dense64_plan.hpp)
    int factor_lds = 0, gemm_lds = 0;
    Grid2 centre, class_sums, invert, gemm_rows, gemm_acc, rowdot, gemm_cross, assemble;      // grids (of a full chunk; of the widest class)
    Grid2 tri;                   // path 1: the factor's inverse, x = the blocks of the widest launch, y = groups of four columns (zeros on path 0)
    int64_t invert_rounds = 0;      // rounds the widest factorisation launch makes over the chip at one workgroup a unit
};

// The refusals; true, or false with the text (it names the remedy).
bool plda_check_rank(int R, std::string &why);
bool plda_check_rows(int64_t n, const char *what, std::string &why);        // 1 .. PLDA_MAX_ROWS
bool plda_check_finite(const double *v, int64_t n, const char *what, std::string &why);
// Sb or Sw: finite, and symmetric within 1e-9 of its largest diagonal magnitude (the device reads the lower triangle).
bool plda_check_symmetric(const double *M, int R, const char *what, std::string &why);
// ids [n] in [0, S), every label with at least one row.
bool plda_check_labels(const int64_t *ids, int64_t n, int64_t S, std::string &why);
bool plda_check_enrol(const int64_t *enrol_n, int64_t J, std::string &why);

// Fill `p` and return true, or false with the reason.  lds_rows: the option jfa_lds_rows; n_cu: compute units (>= 1).
bool plan_plda_train(int64_t n, int R, const int64_t *ids, int64_t S, int lds_rows, int n_cu, PldaPlan &p, std::string &why);
bool plan_plda_score(int64_t J, int64_t T, int R, const int64_t *enrol_n, int64_t scratch_bytes, int lds_rows, int n_cu, PldaPlan &p,
                     std::string &why);

}  // namespace sr
