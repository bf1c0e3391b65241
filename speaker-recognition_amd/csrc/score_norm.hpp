// score_norm.hpp -- score normalisation on the device (score_norm.hip).
#pragma once

#include <cstdint>

namespace sr {

void score_norm(int mode, int64_t J, int64_t T, int64_t Cz, int64_t Ct, int top_n, const double *S, const double *Ez, const double *Tt,
                const double *Zt, double *out, int64_t *degenerate);
void score_norm_select(int64_t rows, int64_t C, int top_n, const double *X, int64_t *idx, double *mu, double *sigma);
void set_norm_scratch_mib(long v);
long norm_scratch_mib();

}  // namespace sr
