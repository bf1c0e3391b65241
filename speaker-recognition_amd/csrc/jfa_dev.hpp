// jfa_dev.hpp -- what jfa.hip (factor estimation), jfa_score.hip (trial scoring) and jfa_stats.hip (resident statistics, centring,
// z / d) share: the two handle types and the host launchers each of them defines for the others (bw_stats.hip includes it for the
// statistics handle its resident entry fills).  Nothing here is the dense layer's: the three include dense64.hpp for
// the GEMM every product goes through, and dense64_dev.hpp for the factorisation inside jfa_factor_kernel and jfa_kscore_kernel.
#pragma once

#include "common.hpp"
#include "jfa.hpp"
#include "jfa_plan.hpp"

#include <vector>

// A factor handle: what sr_jfa_open uploads, or what sr_jfa_open_centred forms on the device (jfa_stats.hip).
struct SRJfa {
    int64_t G = 0;
    int K = 0, D = 0, device = 0;
    sr::DevBuf<double> N, Fc, E, iE;                    // resident for the handle's life
    sr::DevBuf<double> W, WE, P, A, C, Y, B, L;         // per call, grown on demand
    sr::DevBuf<double> zd_d, zd_z, zd_a, zd_b;          // sr_jfa_zd's, grown on demand
    sr::DevBuf<int> flags;
    std::vector<int> h_flags;
};

// Raw statistics of n sessions on one device (jfa_stats.hip): N [n][K], F [n][K D], validated when the handle was made.
struct SRStats {
    int64_t n = 0;
    int K = 0, D = 0, device = 0;
    sr::DevBuf<double> N, F;
};

namespace sr {

// WE = W .* iE over n elements of rows of kd columns (jfa_scale_kernel); P [K][R][R] from W [R][K D] (jfa_gram_kernel).  No timer of their own.
void launch_scale(hipStream_t st, const double *W, const double *iE, double *WE, int64_t n, int64_t kd);
void launch_gram(hipStream_t st, const double *W, const double *iE, double *P, int R, int K, int D);
// jfa.hip: the handle's device and the runtime, as every call on a handle checks them.
void jfa_check_handle(SRJfa &h, const char *what);
// jfa_score.hip: the scoring launches on device-resident statistics dN [T][K], dF [T][K D] and totals d_nt [T] (on the calling thread's
// device; everything else host memory as jfa_score takes it).  `pl`: the plan for this device.
void jfa_score_device(const JfaScorePlan &pl, int64_t T, int64_t J, int K, int D, int Ry, int Ru, const double *dN, const double *dF,
                      const double *d_nt, const double *m, const double *E, const double *d, const double *v, const double *u, const double *z,
                      const double *y, const double *x, const unsigned char *mask, double *out, int64_t *bad_segments);
// jfa_stats.hip: nt [T] = a segment's K counts added in mixture order; returns the segments with nt <= 0 (synchronises).  T_JFA_GRAM.
int64_t launch_segment_totals(hipStream_t st, const double *N, int64_t T, int K, double *nt);
// jfa_stats.hip: the check of a resident pass's result (the texts of jfa_check_raw_stats; synchronises); the live-handle registry.
void stats_check_device(const SRStats &s);
const SRStats &stats_live(const SRStats *s, const char *what);
SRStats *stats_new(int64_t n, int K, int D);      // an empty registered handle on the calling thread's device, buffers allocated

}  // namespace sr
