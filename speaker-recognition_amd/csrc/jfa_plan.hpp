// jfa_plan.hpp -- what the JFA factor estimation (jfa.hip: for every group g -- a speaker, or a session -- of centred statistics
// N[g], Fc[g] and a loading matrix W [R][K D]:  L_g = I + sum_c N[g][c] P_c,  y_g = L_g^-1 W (Fc_g ./ E),  Q_g = L_g^-1 + y_g y_g^T,
// A_c = sum_g N[g][c] Q_g,  C = sum_g y_g Fc_g^T,  W_c <- A_c^-1 C_c) decides before it touches the device: the refusals, the cut
// of the groups into chunks whose R x R blocks fit the scratch bound, the factorisation path, the launch shapes -- as a pure
// function of (G, K, D, R), the bound, the option jfa_lds_rows and the number of compute units.  The GEMM's grids, the
// factorisation's path and the LDS bytes of both come from the dense layer (dense64_plan.hpp); what is JFA's own is below.
// Host-only C++17, nothing of HIP: jfa.hip consumes it, sr_jfa_plan hands it to tests, tests/host/jfa_checks.cpp runs it under the
// host sanitizers.
#pragma once

#include "dense64_plan.hpp"

#include <cstdint>
#include <string>

namespace sr {

// The layer's values under the names sr_jfa_plan, sr_jfa_centre_plan and sr_jfa_score_plan report and JFA's own kernels use: aliases.
constexpr int JFA_MAX_R = DENSE_MAX_R;      // largest rank built
constexpr int JFA_LDS_MAX_R = DENSE_LDS_MAX_R;      // largest R x R block the whole-matrix-in-LDS path takes
constexpr int JFA_KSTEP = DENSE_KSTEP;      // the GEMM's reduction step: a chunk of groups is a multiple of it
constexpr int JFA_TILE = DENSE_TILE;        // the GEMM's output tile: a chunk of the centring's x u product is a multiple of it
constexpr int JFA_WG = DENSE_WG;            // lanes of every workgroup of the path: JFA's own kernels are written for the layer's
constexpr int JFA_GRAM_TILE = 16;           // the gram kernel's output tile, 16 x 16 per mixture
constexpr int JFA_GRAM_DSTEP = 64;          // dimensions of a mixture it stages at a time
constexpr int64_t JFA_DEFAULT_SCRATCH = (int64_t)1 << 30;

struct JfaPlan {
    int64_t chunk = 0;              // groups per chunk: G when they all fit, else a multiple of DENSE_KSTEP
    int64_t n_chunks = 0;
    int64_t bytes_N = 0, bytes_Fc = 0, bytes_E = 0;     // resident with the handle (E: the variances and their reciprocals)
    int64_t bytes_P = 0, bytes_A = 0, bytes_C = 0, bytes_W = 0, bytes_y = 0;     // per call, outside the bound (W: W and W ./ E; y: b and y)
    int64_t bytes_scratch = 0;      // chunk x R x R x 8: the L / Q blocks, what the bound bounds
    int path = 0;                   // factorisation: 0 whole block in LDS, 1 in place in global memory with panels in LDS
    int lds_rows = 0;               // largest R the LDS path takes under the option as given
    Grid2 gram, gemm_L, gemm_b, gemm_A, gemm_C;       // grids (of a full chunk)
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

// The dynamic LDS of jfa_factor_kernel and jfa_kscore_kernel: the layer's panel and block, and JFA's two work vectors [R].
inline int jfa_factor_lds_bytes(int R, int path) { return dense_factor_lds_bytes(R, path, 2); }

// Fills `p` and returns true, or false with the reason.  lds_rows: the option jfa_lds_rows; n_cu: compute units (>= 1).
bool plan_jfa(int64_t G, int K, int D, int R, int64_t scratch_bytes, int lds_rows, int n_cu, JfaPlan &p, std::string &why);

// ---- resident statistics, grouping and centring (jfa_stats.hip): raw statistics N [n][K], F [n][K D] stay on the device from the
// Baum-Welch pass on; the centred, group-summed rows of a factor handle are formed there.  With labels ids [n] in [0, n_labels):
//   mode 0 (groups = the labels that occur, ascending)   N_g = sum_{j in g} N_j
//          Fc_g = sum_{j in g} (F_j - N_j (x) (x_j u)) - N_g (x) (m + z_g .* d + y_g v)
//   mode 1 (groups = sessions)                            Fc_j = (F_j - N_j (x) (x_j u)) - N_j (x) (m + z_s .* d + y_s v),  s = ids[j]
// The session-sized product x u is formed a chunk of sessions at a time under the bound; chunk boundaries depend on n, K D and
// the bound only.  A group's sessions are added in ascending session order, a later chunk continuing from what the row holds.
constexpr int JFA_CENTRE_GROUPS = 0, JFA_CENTRE_SESSIONS = 1;
constexpr int JFA_CENTRE_VEC = 2;           // doubles per lane of the centring kernel where K D is even: 16-byte accesses

struct JfaCentrePlan {
    int mode = 0;
    int64_t chunk = 0, n_chunks = 0;        // sessions per chunk (without the x u term: all n in one)
    int64_t bytes_scratch = 0;              // chunk x K D x 8: the x u product, what the bound bounds (0 without the term)
    int64_t bytes_N = 0, bytes_Fc = 0;      // of the handle that results: G rows (G = n in mode 1, <= min(n, n_labels) in mode 0: the bound here)
    int64_t bytes_yv = 0, bytes_z = 0;      // per call, outside the bound: one row per label that can occur
    int vec = 1;                            // doubles per lane
    Grid2 gemm_xu, gemm_yv, centre, counts;      // grids of a full chunk (centre: x = groups at most, y = column blocks)
};

// The refusals of the shapes and of the labels (null, negative, >= n_labels); true, or false with the text (it names the remedy).
bool jfa_centre_check_shape(int64_t n, int K, int D, int mode, int64_t n_labels, int Ry, int Ru, bool has_v, bool has_u, std::string &why);
bool jfa_centre_check_labels(const int64_t *ids, int64_t n, int64_t n_labels, std::string &why);
bool plan_jfa_centre(int64_t n, int64_t n_labels, int K, int D, int Ry, int Ru, int mode, int64_t scratch_bytes, JfaCentrePlan &p, std::string &why);
// Raw statistics as a handle takes them: a non-finite value in N or F, a negative N (the texts of jfa_check_stats).
bool jfa_check_raw_stats(int64_t n, int K, int D, const double *N, const double *F, std::string &why);
// The two texts alone, for the device-side check of a resident pass's result.
std::string jfa_text_non_finite(const char *what, int64_t element);
std::string jfa_text_negative(int64_t element, int K);

// ---- trial scoring (jfa_score.hip): the score matrix [J][T] of J models against T test segments, with the channel factors
// integrated out (the reference's kscore_famous_19.m) or by the linear approximation (linear_scoring.m).  With M_0 = m,
// M_j = m + z_j .* d + y_j v, J1 = J + 1:
//   q [J1][K] = sum_d M_j^2 / E      G [K][Ru][J1] = u_c (M_j,c ./ E_c)      once per call;
//   L_t = I + sum_c N[t][c] P_c      a_t = u (F_t ./ E)      lin = F (M ./ E)^T      quad = N q^T      h [t][Ru][J1] = N G
//   quad2[t][j] = || chol(L_t)^-1 (a_t - h[t][.][j]) ||^2      s = (lin - quad / 2 + quad2 / 2) / n_t      out[j-1][t] = s[t][j] - s[t][0]
// The segments run in chunks whose L and h blocks fit the bound; nothing is summed over a chunk, so a chunk is any number of segments.
constexpr int JFA_SCORE_INTEGRATED = 0, JFA_SCORE_LINEAR = 1;
constexpr int64_t JFA_SCORE_MAX_J = (int64_t)65535 * JFA_GRAM_TILE - 1;       // (the cross kernel's model tiles are its grid y)

struct JfaScorePlan {
    int mode = 0;
    int64_t chunk = 0, n_chunks = 0;        // test segments per chunk (linear mode: all T in one)
    int64_t seg_bytes = 0;                  // inside the bound, per segment: the L block (Ru^2) and the h block ((J + 1) Ru), in doubles x 8
    int64_t bytes_scratch = 0;              // chunk x seg_bytes
    // outside the bound
    int64_t bytes_M = 0, bytes_ME = 0, bytes_uE = 0, bytes_P = 0, bytes_q = 0, bytes_G = 0, bytes_N = 0, bytes_F = 0;
    int64_t bytes_lin = 0, bytes_quad = 0, bytes_a = 0, bytes_out = 0, bytes_comp = 0;      // comp: linear mode's compensated statistics
    int path = 0, lds_rows = 0;             // the factorisation path of jfa_kscore_kernel, as JfaPlan's
    Grid2 gemm_yv, synth, scale_M, scale_u, gram, cross, gemm_L, gemm_a, gemm_lin, gemm_quad, gemm_h, kscore;      // integrated (yv, synth, scale_M: both)
    int64_t cross_z = 0;                    // the cross kernel's third grid dimension: tiles of 16 channel factors
    Grid2 gemm_xu, comp, gemm_out;        // linear
    int gram_lds = 0, gemm_lds = 0, cross_lds = 0, kscore_lds = 0;
    int64_t kscore_rounds = 0;              // rounds a full chunk's kscore launch makes over the chip at one workgroup a unit
};

// The refusals of the shape; of the arrays (a non-finite value anywhere, a negative N, E <= 0, linear mode without x, a mask that is not
// [J][T]; d, z, x, mask may be null).  true, or false with the text (it names the remedy).
bool jfa_score_check_shape(int64_t T, int64_t J, int K, int D, int Ry, int Ru, int mode, std::string &why);
bool jfa_score_check_inputs(int64_t T, int64_t J, int K, int D, int Ry, int Ru, int mode, const double *N, const double *F, const double *m,
                            const double *E, const double *d, const double *v, const double *u, const double *z, const double *y, const double *x,
                            const unsigned char *mask, int64_t mask_rows, int64_t mask_cols, std::string &why);
// The same with the segments' statistics in a resident handle (validated when it was made): N and F are not read.
bool jfa_score_check_inputs_resident(int64_t T, int64_t J, int K, int D, int Ry, int Ru, int mode, const double *m, const double *E, const double *d,
                                     const double *v, const double *u, const double *z, const double *y, const double *x, const unsigned char *mask,
                                     int64_t mask_rows, int64_t mask_cols, std::string &why);
bool plan_jfa_score(int64_t T, int64_t J, int K, int D, int Ry, int Ru, int mode, int64_t scratch_bytes, int lds_rows, int n_cu, JfaScorePlan &p,
                    std::string &why);

}  // namespace sr
