// em.hpp -- diagonal-covariance EM / MAP training: the driver (em.hip), its whole-fit and float64 engines (em_small.hip,
// em_f64.hip) and the options they read.
#pragma once

#include "gmm_model.hpp"

struct Parameter;

namespace sr {

// em.hip
int train_em(GMM &gmm, const GMM *ubm, const float *X, long n, int dim, const Parameter &param, long seed);
void set_em_stats_engine(int v);
int em_stats_engine();
int last_em_stats_engine();
void set_reference_side_effects(int v);
int reference_side_effects();
// em_small.hip, em_f64.hip: true = done; false = handed back (gmm untouched)
bool train_em_small(GMM &gmm, const GMM *ubm, const float *dX, long n, int dim, const Parameter &param, double relevance, int *iterations);
bool train_em_f64(GMM &gmm, const GMM *ubm, const float *dX, long n, int dim, const Parameter &param, double relevance, int *iterations);
void set_em_small_test_absent(int v);   // em_small.hip

}  // namespace sr
