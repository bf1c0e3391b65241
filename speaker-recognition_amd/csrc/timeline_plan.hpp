// timeline_plan.hpp -- what the timeline (timeline.hip: sliding-window sums of the per-frame matrix, the per-window decision, the
// reference GUI's hold rule, a Viterbi decode with a switch penalty and a minimum turn length) decides before it touches the
// device: the window count, the refusals, the forward kernel's variant for a number of states, the windows whose emissions it
// prefetches, where the minimum-duration chain lives, the sum kernel's span and grid, the back-pointer bytes.  Host-only C++17,
// nothing of HIP: timeline.hip consumes it, sr_timeline_plan hands it to tests, tests/host/timeline_checks.cpp runs it under the
// host sanitizers.
//
// A recording of n frames, window W >= 1, hop H >= 1 (independent): Nw = 0 if n = 0, else 1 + ceil(max(0, n - W) / H) windows;
// window j covers frames [j H, min(j H + W, n)).  With W < H that count can name a window that starts at or behind frame n (the
// last frames fall into the gap between two windows): such a window is not formed, Nw = min(that, ceil(n / H)).
#pragma once

#include <cstdint>
#include <string>

namespace sr {

constexpr int TIMELINE_RAW = 0, TIMELINE_HOLD = 1, TIMELINE_VITERBI = 2;
constexpr int TIMELINE_MAX_S = 4096;                // states (columns) the forward kernel is built for
constexpr int TIMELINE_MAX_M = 16;                  // minimum turn length, windows
constexpr int TIMELINE_WAVE = 64;
constexpr int TIMELINE_LANE_STATES = 1024;          // up to here a lane per state
constexpr int TIMELINE_LOOP_STATES = 4;             // above: a workgroup of 1024 lanes, four states a lane
constexpr int TIMELINE_TILE = 8, TIMELINE_TILE_LOOP = 2;   // windows whose emissions a lane holds ahead of the step it is at
constexpr int TIMELINE_RED_DOUBLES = 48;            // the forward kernel's cross-wave maximum: [2][16] values, [2][16] ranks
constexpr int TIMELINE_CHAIN_LDS_BYTES = 48 << 10;  // a longer chain goes to global memory
constexpr int TIMELINE_SUM_WG = 256;                // sum kernel: four waves, a window each, a lane per column
constexpr int TIMELINE_SUM_WINDOWS = 4;
constexpr int TIMELINE_SUM_COLS = 64;
constexpr int TIMELINE_SUM_CHUNK = 64;              // frames staged at a time
constexpr int TIMELINE_SUM_STRIDE = 65;             // floats between two staged frames: odd, so the transposed writes spread over the banks

struct TimelinePlan {
    int S = 0, m = 0;
    int64_t windows = 0;            // of a recording of n_frames
    int variant = 0;                // 0: one wave, S <= 64; 1: a lane per state, S <= 1024; 2: lanes loop over states, S <= 4096
    int lanes = 0;                  // of the forward kernel's workgroup (one per recording)
    int states_per_lane = 0;
    int tile = 0;                   // windows of emissions prefetched
    int s_pad = 0;                  // lanes x states_per_lane: the stride of a chain slot
    int chain_slots = 0;            // m - 1 values per state, a ring; m <= 2: none stored (m = 2 keeps its one value in a register)
    bool chain_lds = false;         // the ring fits TIMELINE_CHAIN_LDS_BYTES
    int fwd_lds_bytes = 0;
    int words = 0;                  // 64-bit words of stay bits per window: ceil(S / 64)
    int bp_bytes_per_window = 0;    // 8 words + 4 (the entering argmax)
    int64_t sum_span = 0;           // frames a sum workgroup walks at most: 3 H + W
    int sum_lds_bytes = 0;
    int64_t sum_grid_x = 0;         // ceil(windows / 4)
    int sum_grid_y = 0;             // ceil(S / 64)
};

inline int64_t timeline_windows(int64_t n, int64_t W, int64_t H) {
    if (n <= 0 || W < 1 || H < 1) return 0;
    const int64_t rest = n > W ? n - W : 0;
    const int64_t reach = 1 + rest / H + (rest % H != 0);           // windows until one reaches the end
    const int64_t starts = n / H + (n % H != 0);                    // windows that start inside the recording
    return reach < starts ? reach : starts;
}

// Fills `p` and returns true, or returns false with the reason in `why`: S outside 1 .. 4096, min_dur outside 1 .. 16, window < 1,
// hop < 1, a negative frame count.
bool plan_timeline(int S, int min_dur, int64_t n_frames, int64_t window, int64_t hop, TimelinePlan &p, std::string &why);

// The decision's refusals: bg outside [-1, S), a NaN threshold, mode outside 0 .. 2, a NaN or negative beta, min_dur outside
// 1 .. 16, S outside 1 .. 4096.
bool timeline_check(int S, int bg, double threshold, int mode, double beta, int min_dur, std::string &why);

}  // namespace sr
