// timeline_plan.cpp -- the launch decisions and refusals of the timeline (timeline_plan.hpp): pure host code, nothing of HIP is
// called here.
#include "timeline_plan.hpp"

#include <algorithm>

namespace sr {

bool timeline_check(int S, int bg, double threshold, int mode, double beta, int min_dur, std::string &why) {
    if (S < 1 || S > TIMELINE_MAX_S) {
        why = "the decode is built for 1 .. 4096 columns, got " + std::to_string(S) + " (score the set in parts)";
        return false;
    }
    if (bg < -1 || bg >= S) {
        why = "background column " + std::to_string(bg) + " outside [-1, " + std::to_string(S) + ") (-1: every column is a speaker)";
        return false;
    }
    if (threshold != threshold) {
        why = "the threshold is a NaN";
        return false;
    }
    if (mode != TIMELINE_RAW && mode != TIMELINE_HOLD && mode != TIMELINE_VITERBI) {
        why = "mode must be 0 (raw), 1 (hold) or 2 (viterbi), got " + std::to_string(mode);
        return false;
    }
    if (beta != beta || beta < 0.0) {
        why = "the switch penalty beta must be a number >= 0";
        return false;
    }
    if (min_dur < 1 || min_dur > TIMELINE_MAX_M) {
        why = "min_dur must be 1 .. 16 windows, got " + std::to_string(min_dur);
        return false;
    }
    return true;
}

bool plan_timeline(int S, int min_dur, int64_t n_frames, int64_t window, int64_t hop, TimelinePlan &p, std::string &why) {
    p = TimelinePlan();
    if (!timeline_check(S, -1, 0.0, TIMELINE_RAW, 0.0, min_dur, why)) return false;
    if (window < 1) {
        why = "the window must hold at least 1 frame, got " + std::to_string(window);
        return false;
    }
    if (hop < 1) {
        why = "the hop must be at least 1 frame, got " + std::to_string(hop);
        return false;
    }
    if (n_frames < 0) {
        why = "a negative frame count";
        return false;
    }
    p.S = S;
    p.m = min_dur;
    p.windows = timeline_windows(n_frames, window, hop);
    p.words = (S + TIMELINE_WAVE - 1) / TIMELINE_WAVE;
    if (S <= TIMELINE_WAVE) {
        p.variant = 0;
        p.lanes = TIMELINE_WAVE;
        p.states_per_lane = 1;
    } else if (S <= TIMELINE_LANE_STATES) {
        p.variant = 1;
        p.lanes = p.words * TIMELINE_WAVE;
        p.states_per_lane = 1;
    } else {
        p.variant = 2;
        p.lanes = TIMELINE_LANE_STATES;
        p.states_per_lane = TIMELINE_LOOP_STATES;
    }
    p.tile = p.variant == 2 ? TIMELINE_TILE_LOOP : TIMELINE_TILE;
    p.s_pad = p.lanes * p.states_per_lane;
    p.chain_slots = min_dur > 2 ? min_dur - 1 : 0;
    const int64_t chain_bytes = (int64_t)p.chain_slots * p.s_pad * (int64_t)sizeof(double);
    p.chain_lds = p.chain_slots > 0 && chain_bytes <= TIMELINE_CHAIN_LDS_BYTES;
    p.fwd_lds_bytes = TIMELINE_RED_DOUBLES * (int)sizeof(double) + (p.chain_lds ? (int)chain_bytes : 0);
    p.bp_bytes_per_window = p.words * 8 + 4;
    // hop and window are ints at the C ABI; the sum saturates for what a test may pass beyond that
    const int64_t cap = INT64_MAX / 8;
    p.sum_span = std::min(hop, cap) * (TIMELINE_SUM_WINDOWS - 1) + std::min(window, cap);
    p.sum_lds_bytes = TIMELINE_SUM_CHUNK * TIMELINE_SUM_STRIDE * (int)sizeof(float);
    p.sum_grid_x = (p.windows + TIMELINE_SUM_WINDOWS - 1) / TIMELINE_SUM_WINDOWS;
    p.sum_grid_y = (S + TIMELINE_SUM_COLS - 1) / TIMELINE_SUM_COLS;
    return true;
}

}  // namespace sr
