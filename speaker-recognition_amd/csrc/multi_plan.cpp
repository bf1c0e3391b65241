// multi_plan.cpp -- the decisions of the one-process multi-GPU predictor (multi_plan.hpp).  Host-only.
#include "multi_plan.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>

namespace sr {

std::vector<int> multi_active_slots(const int *devices, int n_slots, bool merge) {
    std::vector<int> active;
    for (int k = 0; k < n_slots; k++) {
        bool first = true;
        if (merge)
            for (int a : active) first = first && devices[a] != devices[k];
        if (first) active.push_back(k);
    }
    return active;
}

// Many utterances that are small against a slot's share: contiguous ranges of about equal sample counts, in the caller's order --
// a slot's PCM is then ONE run of the caller's buffer and travels as a few large copies (dealt round-robin, 1000 equal utterances
// over 2 slots were 1000 copies of 320 KB: 15 ms of copy calls for 6 ms of PCIe time).
// Few or very uneven utterances: longest-first greedy by sample count (what shard.partition_utterances does in Python).
std::vector<std::vector<int>> multi_partition(const int64_t *off, int n_utt, int n_active) {
    std::vector<std::vector<int>> utts((size_t)std::max(0, n_active));
    if (n_utt == 0 || utts.empty()) return utts;
    const int64_t total = off[n_utt];
    int64_t longest = 0;
    for (int u = 0; u < n_utt; u++) longest = std::max(longest, off[u + 1] - off[u]);
    const size_t ns = utts.size();
    if (longest * 8 * (int64_t)ns <= total) {
        int u = 0;
        for (size_t k = 0; k < ns; k++) {
            const int64_t hi = total * (int64_t)(k + 1) / (int64_t)ns;
            while (u < n_utt && (k + 1 == ns || off[u + 1] <= hi)) utts[k].push_back(u++);
        }
        return utts;
    }
    std::vector<int> order(n_utt);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return off[a + 1] - off[a] > off[b + 1] - off[b]; });
    std::vector<int64_t> load(ns, 0);
    for (int u : order) {
        const size_t k = std::min_element(load.begin(), load.end()) - load.begin();
        utts[k].push_back(u);
        load[k] += off[u + 1] - off[u];
    }
    for (auto &l : utts) std::sort(l.begin(), l.end());
    return utts;
}

std::vector<int64_t> multi_slot_offsets(const int64_t *off, const std::vector<int> &utts) {
    const int U = (int)utts.size();
    std::vector<int64_t> so((size_t)U + 1, 0);
    for (int i = 0; i < U; i++) so[i + 1] = so[i] + (off[utts[i] + 1] - off[utts[i]]);
    return so;
}

// The measured adaptation took four calls to settle -- two equal-piece passes, one that allocated the new pieces' buffers, one
// more -- 350 / 337 / 454 / 335 ms before 276 on configs[2]: hence an estimate from the set's arithmetic at the rate its engine
// class sustains (multi.cpp: frame_seconds).  configs[2]: 16.7 Mflop per frame / 700 TFLOP/s + MFCC 2.7 ns = 26.5 ns against
// 5.8 ns of link: 4.6; configs[1]: 0.93.  The votes correct a wrong guess.
bool multi_first_schedule(MultiSchedule &ms, int64_t total, double dev_s_per_frame, double link_s_per_frame) {
    if (!(ms.rho_samples == 0 || !(total > ms.rho_samples / 2 && total < ms.rho_samples * 2))) return false;
    ms.schedule = dev_s_per_frame / link_s_per_frame >= 3.5 ? 1 : 0;
    ms.votes = 0;
    return true;
}

// This pass's device time per byte against the link's (55 GB/s, what page-locked copies reach on this platform): everything but
// the first piece's upload is kernels when rho >= 1, and when it is not the estimate only has to stay below 1.
void multi_vote(MultiSchedule &ms, int64_t total, int n_chunks, double seconds, int64_t first_piece_samples) {
    if (!(total > 0 && n_chunks > 1)) return;
    const double link_s = (double)total * sizeof(int16_t) / 55e9;
    const double first = link_s * (double)(first_piece_samples) / (double)total;
    const double rho_seen = std::max(0.0, seconds - first) / link_s;
    const bool change = ms.schedule ? rho_seen < 2.5 : rho_seen >= 3.5;
    ms.votes = change ? ms.votes + 1 : 0;
    if (ms.votes >= 2) {
        ms.schedule ^= 1;
        ms.votes = 0;
    }
    ms.rho_samples = total;
}

// Piece boundaries: whole utterances; pieces of at least ~2 MB of PCM (smaller ones are all launch overhead and kernel tails).
//
// Copy and kernels take about the same time on this path (configs[1]: 5.6 and 5.3 ms), so the call ends at about
// copy(everything) + kernels(last piece): equal pieces, enough of them that the last one is short and few enough that
// the per-piece launches do not add up (round 4's sweep, HISTORY.md section 5; page-locked PCM: 1 piece 11.3 ms, 2 8.7,
// 4 7.5, 6 7.2, 8 7.25; a small-first / small-last shape, round 4's first attempt, 7.7)
//
// Round 6: (nearly) equal pieces -- eight now, each MULTI_MILD_GROWTH x the one before: with the float64 feature stage a piece's
// kernels are the longer leg by a fifth -- are right when copy and kernels are about as long.  When the kernels are the longer leg by a
// factor rho (configs[2]: 3.2 GB = 58 ms of link time under 280 ms of kernels, rho ~ 4.8) the only exposed copy is the
// FIRST piece's, and a piece may be rho times everything before it without the device ever waiting for its bytes:
// cumulative shares S_k = rho S_{k-1} + s_0, S_{n-1} = 1  =>  s_0 = (rho - 1) / (rho^n - 1).  Two shapes only (a new
// shape means new buffers and tables for every piece): the balanced one above, and four pieces growing by MULTI_GROWTH = 3
// (2.5 / 7.5 / 22.5 / 67.5 %) once two passes in a row on a batch of about this size measured rho >= 3.5; back to the
// balanced one when two in a row measure < 2.5 (multi_vote).  Pieces are whole utterances and an utterance's results do not
// depend on the batch around it: the bits are the same for any cut.
MultiPieces plan_slot_pieces(const int64_t *slot_offsets, int U, int schedule) {
    MultiPieces p;
    const int64_t *so_begin = slot_offsets, *so_end = slot_offsets + U + 1;
    const int64_t total = slot_offsets[U];
    const int want = MULTI_DEFAULT_PIECES;
    const double rho = schedule ? MULTI_GROWTH : MULTI_MILD_GROWTH;
    const int want_n = schedule ? 4 : want;
    const int n_chunks = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(want_n, U), total / ((int64_t)1 << 20)));
    double cum[MULTI_CHUNKS + 1];                    // cumulative shares S_k, cum[n_chunks] = 1
    {
        const double s0 = rho > 1.0 + 1e-9 ? (rho - 1.0) / (std::pow(rho, n_chunks) - 1.0) : 1.0 / n_chunks;
        cum[0] = 0.0;
        for (int c = 1; c <= n_chunks; c++) cum[c] = rho * cum[c - 1] + s0;
        for (int c = 1; c <= n_chunks; c++) cum[c] = std::min(1.0, cum[c] / cum[n_chunks]);
    }
    for (int c = 0; c < n_chunks; c++) {
        const int64_t lo = (int64_t)((double)total * cum[c]), hi = (int64_t)((double)total * cum[c + 1]);
        p.u0[c] = c == 0 ? 0 : (int)(std::lower_bound(so_begin, so_end, lo) - so_begin);
        p.u1[c] = c == n_chunks - 1 ? U : (int)(std::lower_bound(so_begin, so_end, hi) - so_begin);
        p.u0[c] = std::min(p.u0[c], U);
        p.u1[c] = std::max(p.u0[c], std::min(p.u1[c], U));
    }
    for (int c = 1; c < n_chunks; c++) p.u0[c] = p.u1[c - 1];      // contiguous cover
    p.n = n_chunks;
    return p;
}

}  // namespace sr
