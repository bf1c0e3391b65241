// norm_plan.hpp -- what score normalisation (score_norm.hip: Z, T, ZT, S and the two adaptive S-norms of a score matrix S [J][T] against
// impostor cohorts) decides before it touches the device: the refusals, the cut of the test segments into chunks whose adaptive
// scratch fits the bound, the bytes of every array, the launch shapes -- as a pure function of the mode, the shapes, top_n, the
// bound and the number of compute units.  The grids and the LDS bytes of as2's four products are the dense layer's
// (dense64_plan.hpp).
// Host-only C++17, nothing of HIP: score_norm.hip consumes it, sr_score_norm_plan hands it to tests, tests/host/norm_checks.cpp runs
// it under the host sanitizers.
//   Ez [J][Cz]   the models against the Z-cohort          Tt [Ct][T]   the T-cohort models against the test segments
//   Zt [Ct][Cz]  the T-cohort models against the Z-cohort (zt only)
#pragma once

#include "dense64_plan.hpp"

#include <cstdint>
#include <string>

namespace sr {

constexpr int NORM_Z = 0, NORM_T = 1, NORM_ZT = 2, NORM_S = 3, NORM_AS1 = 4, NORM_AS2 = 5;
constexpr int NORM_WG = 256;                    // lanes of every workgroup of the path
constexpr int NORM_BINS = 256;                  // bins of the radix select's histogram: one byte of the key a pass
// THE BUILT LIMIT ON A COHORT.  A cohort row lives in LDS as C 64-bit keys next to the 256-bin histogram and a few words of scan
// state: 16384 x 8 B = 128 KiB + 1 KiB + 96 B of the 160 KiB a gfx950 compute unit has.
constexpr int64_t NORM_MAX_C = 16384;
constexpr int NORM_SELECT_FIXED_LDS = NORM_BINS * 4 + 96;       // histogram + wave totals of the scans and the sums
constexpr int64_t NORM_MAX_ROWS = (int64_t)65535 * DENSE_TILE;        // models or test segments of one call (row tiles: the GEMM's grid y)
constexpr int64_t NORM_DEFAULT_SCRATCH = (int64_t)1 << 30;

struct NormPlan {
    int mode = 0;
    int64_t n_sel = 0;              // values a moment pair is taken over on the enrolment side: min(top_n, Cz) in the adaptive modes, else Cz
    int64_t n_sel_test = 0;         // the same on the test side (Ct)
    int64_t chunk = 0, n_chunks = 0;        // test segments per chunk (as2; every other mode: all T in one)
    // as2, inside the bound: SelE, Es, Es .* Es [J][C] once per call; per test segment a row of SelT [C], a column of Ts and of
    // Ts .* Ts [C] and a column of each of the four products [J]
    int64_t fixed_bytes = 0, seg_bytes = 0, bytes_scratch = 0;
    // outside the bound
    int64_t bytes_S = 0, bytes_Ez = 0, bytes_Tt = 0, bytes_Zt = 0, bytes_out = 0;
    int64_t bytes_moments = 0;      // mu, sigma and the degenerate flag of every row and column a mode takes moments of
    int64_t bytes_tnorm = 0;        // zt: the z-normalised copy of Tt
    int64_t bytes_counts = 0;       // as2: two integer counts per workgroup of the apply kernel
    Grid2 select_enrol, select_test, select_zt;      // x = workgroups = rows (select_test: of a full chunk)
    int select_lds_enrol = 0, select_lds_test = 0;
    Grid2 shift_enrol, shift_test;                   // the elementwise shifted copies (as2)
    Grid2 gemm_enrol, gemm_test;                     // Es SelT^T and SelE Ts of a full chunk (each launched twice)
    int gemm_lds = 0;
    Grid2 apply;                                     // x = models, y = blocks of 256 test segments (of a full chunk in as2)
    int64_t select_rounds = 0;      // rounds the largest selection launch makes over the chip at one workgroup a unit
};

const char *norm_mode_name(int mode);
bool norm_mode_adaptive(int mode);
// Which of Ez, Tt, Zt the mode reads.
bool norm_needs_enrol(int mode);
bool norm_needs_test(int mode);
bool norm_needs_zt(int mode);

int norm_select_lds_bytes(int64_t C);

// The shape's refusals (Cz / Ct of a matrix the mode does not read are ignored); true, or false with the text (it names the remedy).
bool norm_check_shape(int mode, int64_t J, int64_t T, int64_t Cz, int64_t Ct, int top_n, std::string &why);
// The arrays': a matrix the mode needs is missing, a non-finite value anywhere.  (Reads every element given.)
bool norm_check_inputs(int mode, int64_t J, int64_t T, int64_t Cz, int64_t Ct, int top_n, const double *S, const double *Ez, const double *Tt,
                       const double *Zt, std::string &why);
// The selection stage alone: rows x C values.
bool norm_check_select(int64_t rows, int64_t C, int top_n, const double *X, std::string &why);

// Fills `p` and returns true, or false with the reason.  n_cu: compute units (>= 1).
bool plan_score_norm(int mode, int64_t J, int64_t T, int64_t Cz, int64_t Ct, int top_n, int64_t scratch_bytes, int n_cu, NormPlan &p,
                     std::string &why);

}  // namespace sr
