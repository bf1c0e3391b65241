// silence_plan.hpp -- what the energy-threshold silence removal (silence.hip; the reference's src/filters/silence.py:11-50)
// decides before it touches the device: frame length and shift in samples, the grid of candidate frame positions, the cut of
// that grid into blocks, the width of a block's transfer map and the shapes of the launches, as a pure function of the call's
// parameters, the longest utterance and the option "silence_block".  Host-only C++17, nothing of HIP: silence.hip consumes it,
// sr_silence_plan hands it to tests, tests/host/silence_checks.cpp runs it under the host sanitizers.
#pragma once

#include <cstdint>
#include <string>

namespace sr {

constexpr int SILENCE_WG = 256;                 // lanes of every workgroup of silence.hip
constexpr int SILENCE_SCAN_ITEMS = 8;           // int64 values a lane scans: a scan tile is SILENCE_WG * 8 = 2048 values
constexpr int64_t SILENCE_MAX_REL = (int64_t)1 << 30;   // offsets inside a block and inside a transfer map are int32
constexpr int64_t SILENCE_CHAIN_MAX = 2048;     // blocks of the longest utterance under the automatic block size

struct SilencePlan {
    int64_t L = 0, S = 0;           // int(frame_duration * fs), int(frame_shift * fs): silence.py:24-25
    int64_t g = 0;                  // gcd(L, S): every frame start the walk visits is a multiple of it
    int64_t Lg = 0, Sg = 0;         // L / g, S / g: the two jumps, in positions
    int64_t K = 0;                  // min(L, S): samples a kept frame contributes (fewer at the end of the signal)
    int64_t max_pos = 0;            // positions of the longest utterance: ceil(max_samples / g)
    int64_t E = 0;                  // entries of a block's transfer map: min(max(Lg, Sg), max_pos)
    int64_t B = 0;                  // positions per block
    int64_t blocks_max = 0;         // blocks of the longest utterance: ceil(max_pos / B)
    int variant = 0;                // 0: a workgroup takes blocks_per_wg whole blocks, a lane per (block, entry);
                                    // 1: E above the workgroup -- a workgroup per block, its lanes loop over the entries
    int blocks_per_wg = 1;
    int64_t list_cap = 1;           // kept frames a block can hold: ceil(B / Sg)
    int chunk_lanes = 1;            // lanes that add up one position's g squares (1, or a wave of 64 when g >= 32)
};

// Fills `p` and returns true, or returns false with the reason in `why`: L < 1, S < 1 (the reference loops forever there),
// products that are no sample counts (NaN, >= 2^62), max_samples < 1, a block option outside 0 .. 2^30, or a transfer map
// wider than 2^30 entries (a frame and an utterance of more than 2^30 positions each).  block_option 0: B = max(256, 4 E, ceil(max_pos / 2048)).
bool plan_silence(double fs, double frame_duration, double frame_shift, int64_t max_samples, int64_t block_option, SilencePlan &p,
                  std::string &why);

// grid of a launch that covers `items` with `per_wg` of them per workgroup, capped (the kernels stride over the rest)
int silence_grid(int64_t items, int64_t per_wg);

}  // namespace sr
