// silence_plan.cpp -- the launch decisions of the silence removal (silence_plan.hpp): pure host code, nothing of HIP is called here.
#include "silence_plan.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>

namespace sr {

static bool sample_count(double v, const char *name, int64_t &out, std::string &why) {
    // Python's int(): truncation towards zero of the float64 product
    if (!(v == v) || v >= 4611686018427387904.0 /* 2^62 */ || v <= -4611686018427387904.0) {
        why = std::string(name) + " * fs is not a sample count";
        return false;
    }
    out = (int64_t)v;
    if (out < 1) {
        why = std::string(name) + " * fs gives " + std::to_string(out) + " samples: it must be at least 1";
        return false;
    }
    return true;
}

bool plan_silence(double fs, double frame_duration, double frame_shift, int64_t max_samples, int64_t block_option, SilencePlan &p,
                  std::string &why) {
    p = SilencePlan();
    if (!sample_count(frame_duration * fs, "frame_duration", p.L, why)) return false;
    if (!sample_count(frame_shift * fs, "frame_shift", p.S, why)) return false;
    if (max_samples < 1) {
        why = "an utterance without samples";
        return false;
    }
    if (block_option < 0 || block_option > SILENCE_MAX_REL) {
        why = "silence_block must be 0 (automatic) or 1 .. 2^30 positions";
        return false;
    }
    p.g = std::gcd(p.L, p.S);
    p.Lg = p.L / p.g;
    p.Sg = p.S / p.g;
    p.K = std::min(p.L, p.S);
    p.max_pos = max_samples / p.g + (max_samples % p.g != 0);
    // a jump is at most max(Lg, Sg) positions, so the walk enters a block at one of that many offsets -- and an offset at or
    // beyond the longest utterance's positions is past the end of every utterance: no live walk ever holds it
    p.E = std::min(std::max(p.Lg, p.Sg), p.max_pos);
    if (p.E > SILENCE_MAX_REL) {
        why = "frames and utterances of more than 2^30 positions each";
        return false;
    }
    // automatic: at least 256 positions and 4 E (the maps table then takes at most a byte per position), and few enough blocks
    // that the one serial part -- an utterance's chain of look-ups -- stays at SILENCE_CHAIN_MAX steps however long it is
    const int64_t for_chain = p.max_pos / SILENCE_CHAIN_MAX + (p.max_pos % SILENCE_CHAIN_MAX != 0);
    p.B = block_option ? block_option : std::min(SILENCE_MAX_REL, std::max<int64_t>({256, 4 * p.E, for_chain}));
    p.blocks_max = p.max_pos / p.B + (p.max_pos % p.B != 0);
    p.variant = p.E > SILENCE_WG ? 1 : 0;
    p.blocks_per_wg = p.variant ? 1 : (int)(SILENCE_WG / p.E);
    p.list_cap = p.B / p.Sg + (p.B % p.Sg != 0);
    p.chunk_lanes = p.g >= 32 ? 64 : 1;
    return true;
}

int silence_grid(int64_t items, int64_t per_wg) {
    const int64_t n = items / per_wg + (items % per_wg != 0);
    return (int)std::min<int64_t>(std::max<int64_t>(n, 1), (int64_t)1 << 20);
}

}  // namespace sr
