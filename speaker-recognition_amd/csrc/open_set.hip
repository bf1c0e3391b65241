// open_set.hip -- the reference's open-set decision (GMMSet.predict_one_with_rejection, src/testbench/gmmset.py:69-81) on
// per-utterance sums that are FINAL: behind gmm_finalize_kernel, and behind gmm_flush.hip's patch where a pass had pairs in
// the partial-product band.  For an utterance of n frames, in float64 and in the reference's order:
//   q[s]   = sums[s] / n          for every column s but the background (the UBM) column bg
//   best   = the first maximum of q  (the QUOTIENTS are compared: two sums one ulp apart may round to one quotient, and the
//            reference's max(enumerate(...)) then keeps the lower index)
//   margin = q[best] - sums[bg] / n
//   label  = best unless margin < threshold, then -1 (the reference's None)
// n <= 0, or no column besides bg: label -1, margin NaN.
// NaN sums follow the reference's max(enumerate(...)), which starts from the first quotient and replaces it on `>` alone: a NaN
// in the first column besides bg stays (nothing compares above it), the margin is NaN, `margin < threshold` is false and that first
// column is the label; a NaN anywhere else never wins.  A NaN in the bg column likewise gives margin NaN and accepts the best.
// One wave per utterance, lanes striding the models, four waves per workgroup; no LDS, no atomics, no scratch.
// Frame counts: a device table of ints (`counts`: a voice-activity session's, stream.cpp) or the batch's row offsets.
// `utts` (or null: all of them in order) lists the utterances to decide: the ones gmm_flush.hip patched.
#include "score.hpp"
#include "wave_ops.hpp"

#include <climits>
#include <cmath>

namespace sr {

namespace {

constexpr int OPEN_SET_WAVES = 4;

__global__ __launch_bounds__(64 * OPEN_SET_WAVES)
void open_set_decision_kernel(const double *__restrict__ sums, const int *__restrict__ utts, int n_items, int n_models, int bg,
                              const int64_t *__restrict__ off, const int *__restrict__ counts, double threshold,
                              int *__restrict__ label, double *__restrict__ margin) {
    const int lane = threadIdx.x & 63;
    const int item = blockIdx.x * OPEN_SET_WAVES + (threadIdx.x >> 6);
    if (item >= n_items) return;                                 // (whole wave: the reduction below sees 64 active lanes)
    const int u = utts ? utts[item] : item;
    const int64_t n = counts ? (int64_t)counts[u] : off[u + 1] - off[u];
    const double *row = sums + (int64_t)u * n_models;
    const double dn = (double)n;
    double best = -INFINITY;
    int best_i = INT_MAX;
    if (n > 0) {
        for (int s = lane; s < n_models; s += 64) {
            if (s == bg) continue;
            const double q = row[s] / dn;
            if (q > best || (q == best && s < best_i)) {
                best = q;
                best_i = s;
            }
        }
    }
    wave_first_max_f64(best, best_i);
    if (lane == 0) {
        double m = NAN;
        int lab = -1;
        const int first = bg == 0 ? 1 : 0;                       // where the reference's max() starts
        if (n > 0 && first < n_models) {
            if (row[first] / dn != row[first] / dn) {            // a NaN there is never replaced: accepted with margin NaN
                lab = first;
            } else {                                             // (then best_i is a column: `first` compares)
                m = best - row[bg] / dn;
                lab = !(m < threshold) ? best_i : -1;
            }
        }
        label[u] = lab;
        margin[u] = m;
    }
}

struct OpenSetStaging {
    DevBuf<double> sums, out;
    DevBuf<int64_t> off;
    PinnedBuf<double> h_out;
};

}  // namespace

void launch_open_set(const double *d_sums, int n_models, const OpenSetRule &rule, const int64_t *d_off, const int *d_counts,
                     const int *d_utts, int n_items, double *d_margin, int *d_label) {
    if (n_items <= 0) return;
    if (rule.bg < 0 || rule.bg >= n_models) fail("open-set decision: background column %d outside [0, %d)", rule.bg, n_models);
    if (!d_off && !d_counts) fail("open-set decision: no frame counts");
    hipLaunchKernelGGL(open_set_decision_kernel, dim3((unsigned)((n_items + OPEN_SET_WAVES - 1) / OPEN_SET_WAVES)),
                       dim3(64 * OPEN_SET_WAVES), 0, ctx().stream, d_sums, d_utts, n_items, n_models, rule.bg, d_off, d_counts,
                       rule.threshold, d_label, d_margin);
    SR_HIP(hipGetLastError());
}

// Host sums -> the decision: upload, kernel, one copy back.
void open_set_decide_host(const double *sums, int U, int S, const OpenSetRule &rule, const int64_t *n_frames, int *label_out,
                          double *margin_out) {
    ensure_device();
    if (U == 0) return;
    auto &st = per_device<OpenSetStaging>();
    std::vector<int64_t> off((size_t)U + 1, 0);
    for (int u = 0; u < U; u++) off[u + 1] = off[u] + n_frames[u];
    st.sums.upload(sums, (size_t)U * S);
    st.off.upload(off.data(), off.size());
    st.out.ensure(open_set_doubles((size_t)U));
    st.h_out.ensure(open_set_doubles((size_t)U));
    launch_open_set(st.sums.p, S, rule, st.off.p, nullptr, nullptr, U, st.out.p, open_set_labels(st.out.p, (size_t)U));
    SR_HIP(hipMemcpyAsync(st.h_out.p, st.out.p, open_set_bytes((size_t)U), hipMemcpyDeviceToHost, ctx().stream));
    sync_stream();
    std::memcpy(margin_out, st.h_out.p, (size_t)U * sizeof(double));
    std::memcpy(label_out, open_set_labels(st.h_out.p, (size_t)U), (size_t)U * sizeof(int));
}

}  // namespace sr
