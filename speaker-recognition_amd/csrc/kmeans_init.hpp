// kmeans_init.hpp -- the start in front of EM on the device (kmeans_init.hip): the reference's initialisation of a GMM and the
// labels of the library's seeded k-means; the engine option and the two counters of its nearest-centre search.
#pragma once

#include "gmm_model.hpp"

#include <vector>

struct Parameter;

namespace sr {

// init_gaussians (gmm.cc:306-361).  seed < 0: the reference's stream (the library-wide restated rand()).
void init_gmm_like_reference(GMM &g, const float *X, long n, int dim, const Parameter &param, long seed);
// Labels of the library's seeded k-means (k-means|| + Lloyd on the full data, then the nearest centre of every point): the
// initialisation of a full-covariance fit (gmm_full_fit.hip, sklearn's init_params='kmeans' with this library's k-means).
std::vector<int> kmeans_labels(const float *X, long n, int dim, int K, long seed);
void set_kmeans_assign_engine(int v);       // 0: the fast full search with the exact pass behind it; 1: the exact pass alone
void kmeans_fast_stats(long *passes, long *rechecked);     // full searches taken the fast way; points they left to the exact pass

}  // namespace sr
