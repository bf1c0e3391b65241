// em_f64.hip -- EM / MAP iterations in float64 on the device for SHORT data and models of any size: what a speaker's MAP enrolment
// from a large UBM is (gmmubm.cc:29-81: 512 - 2048 mixtures adapted on one utterance of ~3000 frames; interface.py:55-109).
//
// Why: iteration at a time through the scoring engines (em.hip) such an iteration is ~0.25 ms of kernels inside ~3 ms of host work
// (K = 2048, 3000 frames): the model packed into the engines' layouts again (1.1 ms), and -- most mixtures of a large UBM see next to
// nothing of a short utterance -- the sums of every mixture whose responsibilities are 0 in fp32 and tiny in the reference's float64
// formed again on host threads (0.7 ms).  In float64 there is nothing to pack and nothing to redo: the model stays on the device as
// plain arrays, an iteration is five or six launches, and the host waits -- for 16 bytes -- only where the stop rule wants the total.
//
//   e64_density  (128 frames, block of 64 mixtures; a thread = 2 frames x 16 mixtures): log densities -> L[k][frame]; the block's
//                maximum and sum of exponentials per frame
//   e64_lse      (64 frames): the frame's total from its blocks' pairs (a term below DBL_MIN is 0, a frame without a surviving term
//                carries no responsibility and counts ln 1e-15: gmm.cc:482-498, :34-38, lse.hpp); the chunk's sum and flag
//   e64_stats    (64 frames, block of 64 mixtures): responsibilities exp(lp - ll), the three sums of the block's mixtures over the
//                chunk's frames -> partial[chunk][k][2 D + 1]
//   e64_head     total log-likelihood and the (accumulating) flag
//   e64_mstep    sums over the chunks in order + the M-step of gmm.cc:388-437 / gmmubm.cc:53-74 (em.hip's host M-step restated) in place
//   e64_weights  (EM only) weights N_k / n normalised by their sum in mixture order, the mixtures' constants
// The stop rule (gmm.cc:622-650) reads the total under the updated model off the NEXT iteration's e64_head, as em_small.hip does; a
// live frame within 110 nats of the underflow boundary hands the fit to the iteration-at-a-time path (partial-product flushes).
#include "score.hpp"
#include "em.hpp"
#include "em_f64_dev.hpp"

#include "../../include/pygmm_hip.h"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

namespace sr {

namespace {

// (the shapes, E64Args and the kernels' bodies: map_plan.hpp and em_f64_dev.hpp, shared with the batched enrolment of map_batch.hip)
__global__ __launch_bounds__(256)
void e64_derive_kernel(const E64Args a, int what /* 1: h, 2: c, 3: both */) {
    e64_derive_body(a, what, blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(E64_THREADS)
void e64_density_kernel(const E64Args a) {
    extern __shared__ __attribute__((aligned(16))) double e64_lds[];
    e64_density_body(a, e64_lds, blockIdx.x, blockIdx.y);
}

__global__ __launch_bounds__(256)
void e64_lse_kernel(const E64Args a) {
    e64_lse_body(a, blockIdx.x);
}

__global__ __launch_bounds__(E64_STHREADS)
void e64_stats_kernel(const E64Args a) {
    extern __shared__ __attribute__((aligned(16))) double e64_lds[];
    e64_stats_body(a, e64_lds, blockIdx.x, blockIdx.y);
}

// total log-likelihood of the pass (the chunks' sums: two per lane, then the wave's fixed-order sum) and the flag, which ACCUMULATES
// over the passes of a fit (the host does not wait for every pass)
__global__ __launch_bounds__(64)
void e64_head_kernel(const E64Args a) {
    double ll, b;
    e64_head_sums(a, ll, b);
    if (threadIdx.x == 0) {
        a.head[0] = ll;
        a.head[1] += b;
    }
}

__global__ __launch_bounds__(256)
void e64_mstep_kernel(const E64Args a) {
    e64_mstep_body(a, blockIdx.x * 256 + threadIdx.x);
}


// EM only: update_weights (gmm.cc:388-394) -- the quotients side by side, their sum in mixture order -- and the constants.  One
// workgroup (after e64_mstep_kernel: the constants take the new sigmas).
__global__ __launch_bounds__(1024)
void e64_weights_kernel(const E64Args a) {
    __shared__ double s_sum;
    const int D = a.dim, REC = 2 * D + 1;
    for (int k = threadIdx.x; k < a.K; k += 1024) {
        double nk = 0.0;
        for (int c = 0; c < a.n_chunks; c++) nk += a.partial[((size_t)c * a.K + k) * REC + 2 * D];
        if (nk == 0.0) nk = 1e-6;
        a.w[k] = nk / (double)a.n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double wsum = 0.0;
        for (int k = 0; k < a.K; k++) wsum += a.w[k];
        s_sum = wsum;
    }
    __syncthreads();
    const double wsum = s_sum;
    for (int k = threadIdx.x; k < a.K; k += 1024) {
        const double w = a.w[k] / wsum;
        a.w[k] = w;
        double c = w > 0.0 ? log(w) : -__builtin_inf();
        for (int d = 0; d < D; d++) c -= log(E64_SQRT_2_PI * a.sg[k * D + d]);
        a.c[k] = c;
    }
}

struct E64Workspace {
    DevBuf<double> model, L, ms, partial, small;
    PinnedBuf<double> h_head, h_model;
};

}  // namespace

// The fit of `gmm` (its parameters are the start) on the n resident frames dX, an iteration = four launches.  true: done -- gmm holds
// the result, *iterations the count train_em returns; false: a frame this path leaves to the other one (gmm untouched).
bool train_em_f64(GMM &gmm, const GMM *ubm, const float *dX, long n, int dim, const Parameter &param, double relevance, int *iterations) {
    const int K = gmm.nr_mixtures, KD = K * dim, REC = 2 * dim + 1;
    auto &w = per_device<E64Workspace>();
    E64Args a;
    a.X = dX;
    a.n = (int)n;
    a.dim = dim;
    a.K = K;
    a.n_pad = (int)((n + E64_DFR - 1) / E64_DFR) * E64_DFR;
    a.n_chunks = a.n_pad / E64_FR;                 // (the last 64-frame chunk may be all padding: zeros in every sum)
    a.n_kb = (K + E64_KB - 1) / E64_KB;
    a.map = ubm ? 1 : 0;
    a.min_sigma = std::sqrt(param.min_covar);
    a.relevance = relevance;
    // model block: w [K], mu [KD], sg [KD], h [KD], c [K], ubm mu [KD]
    std::vector<double> init((size_t)K + 2 * (size_t)KD);
    for (int k = 0; k < K; k++) init[k] = gmm.weights[k];
    for (int i = 0; i < KD; i++) {
        init[K + i] = gmm.mean[i];
        init[K + KD + i] = gmm.sigma[i];
    }
    w.model.ensure((size_t)2 * K + 4 * (size_t)KD);
    a.w = w.model.p;
    a.mu = a.w + K;
    a.sg = a.mu + KD;
    a.h = a.sg + KD;
    a.c = a.h + KD;
    double *ubm_mu = a.c + K;
    a.ubm_mu = ubm_mu;
    SR_HIP(hipMemcpyAsync(a.w, init.data(), init.size() * sizeof(double), hipMemcpyHostToDevice, ctx().stream));
    if (ubm) SR_HIP(hipMemcpyAsync(ubm_mu, ubm->mean.data(), (size_t)KD * sizeof(double), hipMemcpyHostToDevice, ctx().stream));
    w.L.ensure((size_t)a.n_kb * E64_KB * a.n_pad);
    w.ms.ensure((size_t)2 * a.n_kb * a.n_pad);
    w.partial.ensure((size_t)a.n_chunks * K * REC);
    w.small.ensure((size_t)2 * a.n_chunks + 2 + a.n_pad);
    w.h_head.ensure(2);
    a.L = w.L.p;
    a.mb = w.ms.p;
    a.sb = w.ms.p + (size_t)a.n_kb * a.n_pad;
    a.partial = w.partial.p;
    a.llpart = w.small.p;
    a.head = w.small.p + 2 * a.n_chunks;
    a.llf = a.head + 2;
    SR_HIP(hipMemsetAsync(a.head, 0, 2 * sizeof(double), ctx().stream));
    hipStream_t st = ctx().stream;
    const unsigned g_kd = (unsigned)((KD + 255) / 256);
    hipLaunchKernelGGL(e64_derive_kernel, dim3(g_kd), dim3(256), 0, st, a, 3);
    const size_t lds_a = e64_density_lds(dim), lds_b = e64_stats_lds(dim);
    if (lds_a > 64 * 1024)
        SR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&e64_density_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_a));
    if (lds_b > 64 * 1024)
        SR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&e64_stats_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
    const dim3 grid_a((unsigned)(a.n_pad / E64_DFR), (unsigned)a.n_kb), grid_b((unsigned)a.n_chunks, (unsigned)a.n_kb);
    const int nit = param.nr_iteration;
    double last_ll = -std::numeric_limits<double>::max();
    int done = nit;
    for (int it = 0;; it++) {
        const bool ll_only = it == nit;                // the total after the LAST iteration, when that one is an odd one (gmm.cc:622)
        if (ll_only && ((nit - 1) & 1) == 0) break;
        hipLaunchKernelGGL(e64_density_kernel, grid_a, dim3(E64_THREADS), lds_a, st, a);
        hipLaunchKernelGGL(e64_lse_kernel, dim3((unsigned)a.n_chunks), dim3(256), 0, st, a);
        hipLaunchKernelGGL(e64_stats_kernel, grid_b, dim3(E64_STHREADS), lds_b, st, a);
        hipLaunchKernelGGL(e64_head_kernel, dim3(1), dim3(64), 0, st, a);
        SR_HIP(hipGetLastError());
        // the host waits only where the stop rule wants the total (every second pass) and at the end; the flag accumulates
        const bool wants_ll = ll_only || (it >= 1 && ((it - 1) & 1));
        if (wants_ll) {
            SR_HIP(hipMemcpyAsync(w.h_head.p, a.head, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
            sync_stream();
            if (w.h_head.p[1] > 0.0) return false;
        }
        // the total under the model as iteration it - 1 left it: the reference takes it after odd iterations (gmm.cc:622-650)
        if (it >= 1 && ((it - 1) & 1)) {
            const double ll = w.h_head.p[0];
            if (param.verbosity >= 1) printf("iter %d: ll %lf\n", it - 1, ll);
            const double ll_diff = ll - last_ll;
            if (std::fabs(ll_diff) / std::fabs(ll) < param.threshold && ll_diff < param.threshold) {
                done = it;
                break;
            }
            last_ll = ll;
        }
        if (ll_only) break;
        hipLaunchKernelGGL(e64_mstep_kernel, dim3(g_kd), dim3(256), 0, st, a);
        if (!ubm) hipLaunchKernelGGL(e64_weights_kernel, dim3(1), dim3(1024), 0, st, a);
    }
    w.h_model.ensure((size_t)K + 2 * (size_t)KD);
    SR_HIP(hipMemcpyAsync(w.h_model.p, a.w, ((size_t)K + 2 * (size_t)KD) * sizeof(double), hipMemcpyDeviceToHost, st));
    SR_HIP(hipMemcpyAsync(w.h_head.p, a.head, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    sync_stream();
    if (w.h_head.p[1] > 0.0) return false;
    for (int k = 0; k < K; k++) gmm.weights[k] = w.h_model.p[k];
    for (int i = 0; i < KD; i++) {
        gmm.mean[i] = w.h_model.p[K + i];
        gmm.sigma[i] = w.h_model.p[K + KD + i];
    }
    gmm.drop_single();
    *iterations = done;
    return true;
}

}  // namespace sr
