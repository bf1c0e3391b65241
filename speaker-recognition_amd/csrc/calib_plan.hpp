// calib_plan.hpp -- what score calibration and fusion (calib.hip: prior-weighted linear logistic regression of S score rows X [S][n]
// against labels lab [n], its objective Cllr, the affine map, the error counts at thresholds) decides before it touches the device:
// the refusals, the bytes of every array, the block count, the grids, the layout and the length of the state -- as a pure function
// of S, n, the number of thresholds, the bound and the number of compute units.
// Host-only C++17, nothing of HIP: calib.hip consumes it, sr_calib_plan hands it to tests, tests/host/calib_checks.cpp runs it under
// the host sanitizers.
#pragma once

#include <cstdint>
#include <string>

namespace sr {

// THE BUILT LIMIT ON THE SYSTEMS OF ONE FUSION: the pass kernel keeps f, g and the upper triangle of H -- 1 + (S + 1) +
// (S + 1)(S + 2) / 2 float64 accumulators, 55 at S = 8 -- in registers, one instance per S.
constexpr int CALIB_MAX_S = 8;
constexpr int CALIB_WG = 256;                   // lanes of every workgroup of the path
constexpr int CALIB_BLOCK = 4096;               // consecutive trials a workgroup of the pass and counts kernels owns
constexpr int CALIB_MAX_THR = 16;               // thresholds of one counts call
constexpr int64_t CALIB_MAX_N = (int64_t)1 << 35;       // trials of one call (blocks x lanes stays below 2^32, the bytes stay in int64)
constexpr int64_t CALIB_DEFAULT_SCRATCH = (int64_t)8192 << 20;
constexpr int CALIB_MAX_PASS = 1000;
constexpr int CALIB_CADENCE = 4;                // the host reads the stop word back after every CADENCE-th pass + step pair
constexpr int CALIB_HALVINGS = 20;              // the line search gives up once t < 2^-20

// stop codes
constexpr int CALIB_CONVERGED = 0, CALIB_CAP = 1, CALIB_SINGULAR = 2, CALIB_STALLED = 3;

// The state: doubles.  With P = S + 1:
//   [0] stop (-1 while running, else the code)   [1] phase (0: the pass at theta0 is pending, 1: a line-search trial is pending)
//   [2] passes  [3] accepted steps  [4] halvings  [5] f at theta  [6] t  [7] lam2  [8] n_t  [9] n_n  [10] skipped
//   [11] the cap on [2]  [12] S  [13 .. 15] 0
//   [16 ..] theta [P] (the last accepted point), trial [P] (what the next pass evaluates), d [P], g [P] at theta,
//   H at theta [P (P + 1) / 2] (upper triangle by rows)
constexpr int CALIB_ST_STOP = 0, CALIB_ST_PHASE = 1, CALIB_ST_PASSES = 2, CALIB_ST_ACCEPTED = 3, CALIB_ST_HALVINGS = 4, CALIB_ST_F = 5,
              CALIB_ST_T = 6, CALIB_ST_LAM2 = 7, CALIB_ST_NT = 8, CALIB_ST_NN = 9, CALIB_ST_SKIP = 10, CALIB_ST_CAP = 11, CALIB_ST_S = 12,
              CALIB_ST_HEAD = 16;

constexpr int calib_acc(int S) { return 1 + (S + 1) + (S + 1) * (S + 2) / 2; }
constexpr int calib_state_len(int S) { return CALIB_ST_HEAD + 4 * (S + 1) + (S + 1) * (S + 2) / 2; }
constexpr int calib_off_theta(int) { return CALIB_ST_HEAD; }
constexpr int calib_off_trial(int S) { return CALIB_ST_HEAD + (S + 1); }
constexpr int calib_off_d(int S) { return CALIB_ST_HEAD + 2 * (S + 1); }
constexpr int calib_off_g(int S) { return CALIB_ST_HEAD + 3 * (S + 1); }
constexpr int calib_off_H(int S) { return CALIB_ST_HEAD + 4 * (S + 1); }

struct CalibPlan {
    int S = 0, acc = 0, state_len = 0;
    int64_t n = 0, n_blocks = 0;
    int64_t bytes_X = 0, bytes_lab = 0, bytes_partial = 0, bytes_state = 0;        // training and evaluation
    int64_t bytes_out = 0;                                                           // apply: z [n]
    int64_t bytes_thr = 0, bytes_counts = 0;                                         // counts: 2 x 16 integers per workgroup
    int64_t resident_train = 0, resident_apply = 0, resident_counts = 0;             // what each call keeps on the device, against the bound
    int64_t pass_grid = 0, step_grid = 0, apply_grid = 0, counts_grid = 0;
    int64_t pass_rounds = 0;        // rounds the pass kernel makes over the chip at one workgroup a unit
};

struct CalibCounts {
    int64_t n_t = 0, n_n = 0, n_skip = 0;
};

const char *calib_stop_name(int code);

// The shape's refusals; true, or false with the text (it names the remedy).
bool calib_check_shape(int S, int64_t n, std::string &why);
bool calib_check_params(double prior, double ridge, double tol, int max_pass, std::string &why);
// The arrays': a null argument, a label above 1, no target or no non-target, a non-finite score at a trial (skipped positions are
// not looked at).  Fills the counts.  X may be null for a caller that has no scores to check (labels only).
bool calib_check_trials(int S, int64_t n, const double *X, const int8_t *lab, CalibCounts &c, std::string &why);
bool calib_check_theta(int S, const double *theta, const char *name, std::string &why);
bool calib_check_thresholds(int m, const double *thr, std::string &why);

// Fills `p` and returns true, or false with the reason.  n_thr: 0 .. 16.  n_cu: compute units (>= 1).
bool plan_calib(int S, int64_t n, int n_thr, int64_t scratch_bytes, int n_cu, CalibPlan &p, std::string &why);
// The bound against one call's resident bytes ("train", "apply" or "counts").
bool calib_check_bound(const CalibPlan &p, const char *call, int64_t scratch_bytes, std::string &why);

}  // namespace sr
