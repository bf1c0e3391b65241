// jfa_plan.hpp -- what the JFA factor estimation (jfa.hip: for every group g -- a speaker, or a session -- of centred statistics
// N[g], Fc[g] and a loading matrix W [R][K D]:  L_g = I + sum_c N[g][c] P_c,  y_g = L_g^-1 W (Fc_g ./ E),  Q_g = L_g^-1 + y_g y_g^T,
// A_c = sum_g N[g][c] Q_g,  C = sum_g y_g Fc_g^T,  W_c <- A_c^-1 C_c) decides before it touches the device: the refusals, the cut
// of the groups into chunks whose R x R blocks fit the scratch bound, the factorisation path, the launch shapes -- as a pure
// function of (G, K, D, R), the bound, the option jfa_lds_rows and the number of compute units.
// Host-only C++17, nothing of HIP: jfa.hip consumes it, sr_jfa_plan hands it to tests, tests/host/jfa_checks.cpp runs it under the
// host sanitizers.
#pragma once

#include <cstdint>
#include <string>

namespace sr {

constexpr int JFA_MAX_R = 512;              // largest rank built: the factorisation's panel of JFA_NB columns x R rows lives in LDS
constexpr int JFA_LDS_MAX_R = 112;          // largest R x R block the whole-matrix-in-LDS path takes (112^2 x 8 B = 98 KiB + the panel)
constexpr int JFA_NB = 16;                  // columns of a Cholesky panel
constexpr int JFA_KSTEP = 16;               // reduction step of the GEMM kernel: a tile of 16 = four 16x16x4 matrix instructions
constexpr int JFA_TILE = 64;                // a GEMM workgroup's output tile, 64 x 64: four waves of 16 rows x 64 columns
constexpr int JFA_WG = 256;                 // lanes of every workgroup of the path
constexpr int JFA_GRAM_TILE = 16;           // the gram kernel's output tile, 16 x 16 per mixture
constexpr int JFA_GRAM_DSTEP = 64;          // dimensions of a mixture it stages at a time
constexpr int64_t JFA_DEFAULT_SCRATCH = (int64_t)1 << 30;

struct JfaGrid {
    int64_t x = 0, y = 0;
};

struct JfaPlan {
    int64_t chunk = 0;              // groups per chunk: G when they all fit, else a multiple of JFA_KSTEP
    int64_t n_chunks = 0;
    int64_t bytes_N = 0, bytes_Fc = 0, bytes_E = 0;     // resident with the handle (E: the variances and their reciprocals)
    int64_t bytes_P = 0, bytes_A = 0, bytes_C = 0, bytes_W = 0, bytes_y = 0;     // per call, outside the bound (W: W and W ./ E; y: b and y)
    int64_t bytes_scratch = 0;      // chunk x R x R x 8: the L / Q blocks, what the bound bounds
    int path = 0;                   // factorisation: 0 whole block in LDS, 1 in place in global memory with panels in LDS
    int lds_rows = 0;               // largest R the LDS path takes under the option as given
    JfaGrid gram, gemm_L, gemm_b, gemm_A, gemm_C;       // grids (of a full chunk)
    int gram_lds = 0, gemm_lds = 0, factor_lds = 0, update_lds = 0;
    int64_t factor_rounds = 0;      // rounds a full chunk's factorisation makes over the chip at one workgroup a unit
};

// The shape's refusals; true, or false with the text (it names the remedy).
bool jfa_check_shape(int64_t G, int K, int D, std::string &why);
bool jfa_check_rank(int R, std::string &why);
// The statistics' refusals: a non-finite value, a negative N, E <= 0.  (Reads G K + G K D + K D doubles.)
bool jfa_check_stats(int64_t G, int K, int D, const double *N, const double *Fc, const double *E, std::string &why);
// A non-finite value among the n doubles of `what`.
bool jfa_check_finite(const double *v, int64_t n, const char *what, std::string &why);

// Largest R the LDS path takes for the option value (0 = automatic).
int jfa_lds_limit(int lds_rows);
int jfa_factor_lds_bytes(int R, int path);

// Fills `p` and returns true, or false with the reason.  lds_rows: the option jfa_lds_rows; n_cu: compute units (>= 1).
bool plan_jfa(int64_t G, int K, int D, int R, int64_t scratch_bytes, int lds_rows, int n_cu, JfaPlan &p, std::string &why);

}  // namespace sr
