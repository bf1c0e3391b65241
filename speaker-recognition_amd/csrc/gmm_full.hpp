// gmm_full.hpp -- full-covariance GMMs (C ABI handles `SRFullGMM *` / `SRFullSet *`): scikit-learn's GaussianMixture layout,
// float64 EM on the device (csrc/gmm_full_fit.hip, planned by csrc/full_plan.cpp), fp32 matrix-core scoring of a packed set of
// speakers (csrc/gmm_full.hip).
#pragma once

#include "batch.hpp"
#include "common.hpp"
#include "full_plan.hpp"
#include "mfcc.hpp"

#include "../../include/pygmm_hip.h"

#include <string>
#include <vector>

// One model: weights[K], means[K][D], precisions_cholesky[K][D][D] (upper triangular P_k, precision = P_k P_k^T), float64 on the
// host.  covariances[K][D][D] exists after a fit (the M-step's), empty for a model built from arrays.
struct SRFullGMM {
    int K = 0, D = 0;
    bool trained = false;
    std::vector<double> weights, means, prec_chol, covariances;
};

// S models of one dimension packed for the scoring kernel (gmm_full.hip: the lane image of P_k^T, the means, the constants).
struct SRFullSet {
    int S = 0, D = 0, ns = 0, nrb = 0, device = -1;
    std::vector<int> kbeg;           // [S + 1] first mixture of every model
    sr::DevBuf<float> P;             // [K_total][nrb][ns][64]
    sr::DevBuf<float> mu;            // [K_total][64]
    sr::DevBuf<float> c;             // [K_total]  ln w + sum ln P_ii - D/2 ln 2 pi
    sr::DevBuf<int> d_kbeg;
    sr::DevBuf<float> fll;           // [S][n] per-frame log-likelihoods of the last call
    sr::DevBuf<double> sums;         // [U][S]
    // the device-side decision (fullcov_finalize_kernel): sums [U][S], then argmax [U] as int right behind them -- one copy back
    sr::DevBuf<double> res;
    sr::PinnedBuf<double> h_res;     // sr_fullset_predict_pcm_batch's landing place for that copy
};

namespace sr {
constexpr double FC_LN_2PI = 1.8378770664093453;
// (FULL_MAX_D: full_plan.hpp.)  Both fits run gmm_full_fit.hip's one EM driver, in which a speaker's bits do not depend on the speakers fitted with it.
// One model, a group of one: a failed fit throws and leaves the handle untouched; it moves none of full_fit_batch_stats' counters
// and full_fit_batch_bytes does not bear on it.
void fullgmm_fit(SRFullGMM &g, const double *X, long n, int D, const SRFullFitParams &p, SRFullFitStats &out);
// S models of one K and D in one set of launches per EM iteration (the stop rule per speaker, on the device); every fitted
// speaker gets the bits fullgmm_fit gives it alone.  status[s]: 0 fitted, -1 failed (messages[s] says why; the handle is untouched).
void fullgmm_fit_batch(SRFullGMM *const *models, int S, const double *X, const int64_t *row_offsets, int D, const SRFullFitParams *params,
                       SRFullFitStats *out, int *status, std::vector<std::string> &messages);
long full_fit_batch_bytes();
void set_full_fit_batch_bytes(long bytes);       // sr_set_option("full_fit_batch_bytes"): the workspace bound of a group of speakers
void full_fit_batch_stats(long *calls, long *speakers, long *iterations);
void fullset_pack(SRFullSet &set, const SRFullGMM *const *models, int S);
void fullset_score(SRFullSet &set, SRBatch &batch, double *sums, int *argmax, float *frame_ll);
// Launches only (capturable): scoring + finalize of a feature batch on the calling thread's stream.  Returns set.res: sums [U][S]
// with int argmax [U] right behind them.  fullset_reserve sizes the set's workspaces up front (a pipeline of pieces reserves for
// its largest piece, so that no piece reallocates -- a hipFree -- under the kernels of the one before).
const double *fullset_score_device(SRFullSet &set, SRBatch &feat);
// The serving stream's voice-activity front end: utterance u is the first d_cnt[u] rows (a device table) of its slot in `feat`.
// Results go to the caller's d_res: sums [U][S], then argmax [U] as int.  An utterance with d_cnt[u] == 0 gets sums 0, argmax -1.
void fullset_score_device_masked(SRFullSet &set, SRBatch &feat, const int *d_cnt, double *d_res);
// fullcov_finalize_kernel over any per-frame values fll [S][n]: utterance u's sum over rows [d_off[u], d_off[u] + d_cnt[u]) in the
// fixed order of that kernel; argmax of the means, or of the sums themselves when `plain` (a diagonal set's decision)
void masked_finalize(const float *fll, long n, const int64_t *d_off, const int *d_cnt, int U, int S, bool plain, double *d_sums, int *d_argmax);
void fullset_reserve(SRFullSet &set, int64_t n_rows, int n_utt);
// MFCC (+ LPC columns or deltas) -> scoring -> finalize -> one copy back (sr_fullset_predict_pcm_batch)
void fullset_predict_pcm(SRMfcc &m, SRFullSet &set, SRBatch &pcm, int nd, double *sums, int *argmax);
}  // namespace sr
