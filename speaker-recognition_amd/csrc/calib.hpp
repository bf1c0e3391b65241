// calib.hpp -- score calibration and fusion on the device (calib.hip).
#pragma once

#include <cstdint>

namespace sr {

void calib_train(int S, int64_t n, const double *X, const int8_t *lab, double prior, double ridge, double tol, int max_pass, const double *theta0,
                 int resume, double *state, int64_t *counts);
void calib_eval(int S, int64_t n, const double *X, const int8_t *lab, double prior, double ridge, const double *theta, double *f, double *g,
                double *H, int64_t *counts);
void calib_apply(int S, int64_t n, const double *X, const double *theta, double *out);
void calib_counts(int64_t n, const double *llr, const int8_t *lab, int m, const double *thr, int64_t *miss, int64_t *fa, int64_t *counts);
void set_calib_scratch_mib(long v);
long calib_scratch_mib();

}  // namespace sr
