// multi_plan.hpp -- what the one-process multi-GPU predictor (multi.cpp: sr_multi_predict_pcm / _open, diagonal and full-covariance
// sets) decides before it touches a device: which slots take work, which utterances each of them gets, the shape of a slot's next
// pass (its memory across calls: an estimate first, then a vote on what the passes measured), and the cut of a slot's utterances
// into pieces -- as pure functions of the sample offsets, the slots' device indices, the merge option and the slot's schedule.
// Host-only C++17, nothing of HIP: multi.cpp consumes it, sr_multi_plan hands it to tests, tests/host/multi_checks.cpp runs it under
// the host sanitizers against the decisions recorded from the commit before it became a file of its own (tests/host/multi_table.inc).
#pragma once

#include <cstdint>
#include <vector>

namespace sr {

constexpr int MULTI_CHUNKS = 8;         // a slot's utterances are uploaded and scored in up to this many pieces
constexpr int MULTI_DEFAULT_PIECES = 8; // ... and in this many when copy and kernels are about as long: eight, each 1.1 x the one before
constexpr double MULTI_MILD_GROWTH = 1.1;   // (round 6, configs[1] from page-locked PCM, 12 calls each in one session: 6 equal pieces 7.4-7.8 ms,
                                        // 8 equal 7.3-7.5, 8 x 1.1 7.13-7.30, 8 x 1.2 7.26-7.43, 8 x 1.3 7.5-7.6, 5 x 1.25 7.8-7.9, 4 x 1.5 8.4-8.6:
                                        // the kernels of a piece -- 1.15 ms against its 0.95 ms of link time -- are the longer leg by a little)
constexpr double MULTI_GROWTH = 3.0;    // kernel-bound slots (plan_slot_pieces): every piece this many times everything before it

// The slots that take work, by index.  Slots that share a device are ONE queue on it (round 4): the device's lock would serialise
// their pieces anyway, in an order nobody chose, with both slots' tails at the end.  With `merge` the first slot of a device takes
// the work of all of them; without it every slot has its own share and thread (what the tests of the threaded path on a one-GPU
// box use).
std::vector<int> multi_active_slots(const int *devices, int n_slots, bool merge);

// Utterances -> active slots: for each of them its utterance indices, ascending.  off: [n_utt + 1] cumulative samples.
std::vector<std::vector<int>> multi_partition(const int64_t *off, int n_utt, int n_active);

// The cumulative sample counts [utts.size() + 1] of a slot's utterances, in the slot's order.
std::vector<int64_t> multi_slot_offsets(const int64_t *off, const std::vector<int> &utts);

// What the last passes told about a slot's work: device time per PCM byte against the link's time per byte (rho >= 1: the kernels
// are the longer leg) on a batch of rho_samples samples -- two passes in a row that agree change the shape of the next pass's
// pieces.  schedule: 0 = (nearly) equal pieces, 1 = growing pieces.
struct MultiSchedule {
    int schedule = 0, votes = 0;
    int64_t rho_samples = 0;
};

// The FIRST pass on a batch of `total` samples -- none before it, or the last one measured was of less than half or more than
// twice the size -- starts from an estimate: device seconds per frame against the link's seconds per frame.  Resets the votes and
// returns true then; leaves `ms` alone otherwise.
bool multi_first_schedule(MultiSchedule &ms, int64_t total, double dev_s_per_frame, double link_s_per_frame);

// After a pass of `seconds` over `total` samples in n_chunks pieces, the first of first_piece_samples: this pass's device time per
// byte against the link's, and the two-in-a-row vote (>= 3.5: growing pieces, < 2.5: back to equal ones).  A pass of one piece or
// of no samples says nothing.
void multi_vote(MultiSchedule &ms, int64_t total, int n_chunks, double seconds, int64_t first_piece_samples);

// A slot's U utterances cut into n pieces of whole utterances, piece c = [u0[c], u1[c]): a contiguous cover of [0, U), a piece may
// be empty.  slot_offsets: [U + 1] cumulative samples.
struct MultiPieces {
    int n = 1;
    int u0[MULTI_CHUNKS] = {}, u1[MULTI_CHUNKS] = {};
};
MultiPieces plan_slot_pieces(const int64_t *slot_offsets, int U, int schedule);

// f(i, j) for every maximal run [i, j] of utts[i0 .. i1) whose utterances are neighbours in the caller's buffer: such a run
// travels as one copy.
template <class F>
void for_each_run(const int *utts, int i0, int i1, F &&f) {
    for (int i = i0; i < i1;) {
        int j = i;
        while (j + 1 < i1 && utts[j + 1] == utts[j] + 1) j++;
        f(i, j);
        i = j + 1;
    }
}

}  // namespace sr
