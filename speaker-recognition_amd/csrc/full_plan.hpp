// full_plan.hpp -- what the float64 full-covariance fit (gmm_full_fit.hip: fullgmm_fit, a group of one, and fullgmm_fit_batch) decides
// before it touches the device: the cut of the speakers into groups whose workspace stays under the bound, and per group the
// per-speaker table (rows, covariance chunking, the slice of `partial`), the three work lists the frame-parallel kernels read,
// the element count of every workspace buffer and the loop's length -- as a pure function of K, D, the speakers' frame counts,
// their kind of start and max_iter, and the bound.  The shapes the kernels are built on and the four per-speaker formulas live
// here, each once: the .hip file includes this header.
// Host-only C++17, nothing of HIP: gmm_full_fit.hip consumes it, sr_full_fit_plan hands it to tests, tests/host/full_checks.cpp
// runs it under the host sanitizers.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace sr {

constexpr int FULL_MAX_D = 64;
constexpr int FE_FB = 32;          // frames of a density workgroup
constexpr int FE_PQ = 9;           // covariance pairs per thread: 9 x 256 >= 64 x 65 / 2
static_assert(FE_PQ * 256 >= FULL_MAX_D * (FULL_MAX_D + 1) / 2, "fe_cov: 256 threads x FE_PQ slots must hold the upper triangle at FULL_MAX_D");
constexpr int FE_CB = 32;          // frames staged per covariance step
constexpr int FULL_MAX_GROUP = 65535;                       // speakers of a group: fe_means, fe_chol and fe_derive take the speaker as a grid's y
constexpr int FULL_MAX_K = 65535;                           // fe_logprob and fe_cov take the mixture as a grid's y
constexpr int64_t FULL_DEFAULT_BYTES = (int64_t)1 << 30;    // sr_set_option("full_fit_batch_bytes")

// a speaker's launch geometry, each formula once
inline long fe_lp_blocks(long n) { return (n + FE_FB - 1) / FE_FB; }                      // density workgroups
inline long fe_lse_blocks(long n) { return (n + 255) / 256; }                             // log-sum-exp / one-hot workgroups
inline int fe_n_chunks(long n) { return (int)std::min<long>(32, (n + 255) / 256); }       // covariance chunks
inline size_t fe_partial_len(long n, int K, int D) { return (size_t)fe_n_chunks(n) * K * (D * (D + 1) / 2); }

// sizes of the device structs of gmm_full_fit.hip (which static_asserts them): the per-speaker table entry FeSpk, the record FeRec
constexpr size_t FE_SPK_BYTES = 72, FE_REC_BYTES = 16;

// a work item (the device reads the lists as int2): block `block` (FE_FB frames / 256 frames / a covariance chunk) of the speaker at `slot`
struct FullWork {
    int32_t slot, block;
};

// elements of every buffer of a group's workspace (FeBatchWorkspace; `label` is uploaded for the k-means speakers only, and counted always)
struct FullCounts {
    int64_t X = 0, w = 0, logw = 0, mu = 0, prec = 0, logdet = 0, cov = 0, lp = 0, lpn = 0, nk = 0, partial = 0, head = 0;     // double
    int64_t spk = 0, rec = 0;                       // FeSpk, FeRec
    int64_t wl_lp = 0, wl_lse = 0, wl_cov = 0;      // FullWork
    int64_t label = 0;                              // int
    int64_t bytes() const {
        return (int64_t)sizeof(double) * (X + w + logw + mu + prec + logdet + cov + lp + lpn + nk + partial + head) +
               (int64_t)FE_SPK_BYTES * spk + (int64_t)FE_REC_BYTES * rec + (int64_t)sizeof(FullWork) * (wl_lp + wl_lse + wl_cov) +
               (int64_t)sizeof(int) * label;
    }
};

struct FullSpeakerPlan {
    int64_t n = 0, row0 = 0;            // frames; first row inside its group's X / lp / lpn
    int n_chunks = 0, chunk = 0;        // the covariance chunking: chunk c is frames [c chunk, min(n, (c + 1) chunk))
    int64_t o_partial = 0;              // its slice of the group's `partial`, in doubles
    int64_t bytes = 0;                  // the workspace of a group of this speaker alone
    int group = -1, slot = -1;
};

struct FullGroupPlan {
    int first = 0, count = 0;           // speakers [first, first + count) of the call
    int64_t rows = 0;
    int64_t lp0 = 0, lse0 = 0, cov0 = 0;        // where its ranges of the plan's three work lists start (their lengths: counts.wl_*)
    int max_iter = 0;                   // the longest of its speakers
    bool any_kmeans = false, any_given = false;
    FullCounts counts;
    int64_t bytes = 0;                  // counts.bytes()
};

struct FullFitPlan {
    int K = 0, D = 0;
    std::vector<FullSpeakerPlan> speakers;      // [S]
    std::vector<FullGroupPlan> groups;
    std::vector<FullWork> wl_lp, wl_lse, wl_cov;        // group after group
    size_t lds_logprob = 0;             // fe_logprob's dynamic LDS: P, mu, FE_FB frames' differences, 256 partial squares
    int64_t max_group_bytes = 0;
};

// the workspace of a group of one speaker of n frames, in bytes
int64_t full_speaker_bytes(int K, int D, int64_t n);

// Fills `p` and returns true, or false with the reason: a shape outside 1 <= K <= FULL_MAX_K, 1 <= D <= FULL_MAX_D, no speaker, a
// speaker without frames, a bound below 1 byte, a group whose work lists or block indices pass INT_MAX.  n: [S] frames per
// speaker; init_given, max_iter: [S].  The cut: in call order, greedy; a speaker that alone exceeds the bound is a group of its
// own; at most FULL_MAX_GROUP speakers to a group.
bool plan_full_fit(int K, int D, const int64_t *n, const int *init_given, const int *max_iter, int64_t S, int64_t bound_bytes, FullFitPlan &p,
                   std::string &why);

}  // namespace sr
