// map_plan.cpp -- the decisions of the batched MAP enrolment call (map_plan.hpp).  Host-only.
#include "map_plan.hpp"

#include <algorithm>
#include <cstdio>

namespace sr {

static std::string fmt(const char *f, long long a = 0, long long b = 0) {
    char buf[320];
    snprintf(buf, sizeof buf, f, a, b);
    return buf;
}

EmSmallShape em_small_shape(int K, int D, long n) {
    EmSmallShape best{0, 1, 0, 0};
    const int R = K * (D + 1);
    for (int fr : {128, 64}) {
        if (fr > 64 && (n + fr / 2 - 1) / (fr / 2) == (n + fr - 1) / fr) continue;      // (half the frames: as many workgroups)
        int seg = 1;
        while (seg * 2 <= fr / 64 && R * seg * 2 <= EMF_THREADS) seg *= 2;
        const size_t lds = (size_t)(3 * K + 3 * K * D + K * fr + EMF_THREADS + fr + K * (2 * D + 1) + 2 + 2 * R * seg) * sizeof(double) +
                           (size_t)fr * (D + 1) * sizeof(float);
        if (lds > 150 * 1024) continue;
        best = {fr, seg, (int)((n + fr - 1) / fr), lds};
        break;
    }
    return best;
}

bool em_small_shape_eligible(int K, int dim, long n, const Parameter &param, int n_cu) {
    return K >= 1 && K <= EMF_MAX_K && dim >= 1 && dim <= EMF_MAX_D && n >= 1 &&
           n <= EMF_MAX_FRAMES && em_small_shape(K, dim, n).grid >= 1 && em_small_shape(K, dim, n).grid <= n_cu / 2 && param.nr_iteration >= 1 && param.verbosity < 2;
}

bool em_f64_shape_eligible(int K, int dim, long n, const Parameter &param) {
    return K >= 1 && dim >= 1 && dim <= E64_MAX_D && n >= 1 && n <= E64_MAX_FRAMES && param.nr_iteration >= 1 && param.verbosity < 2 &&
           (long)((K + E64_KB - 1) / E64_KB * E64_KB) * ((n + E64_DFR - 1) / E64_DFR * E64_DFR) <= E64_MAX_CELLS;
}

size_t e64_density_lds(int dim) {
    return (size_t)(2 * E64_KB * dim + E64_KB + 4 * E64_DFR) * sizeof(double) + (size_t)E64_DFR * (dim + 1) * sizeof(float);
}

size_t e64_stats_lds(int dim) {
    return (size_t)(E64_KB * E64_FR + E64_KB * dim) * sizeof(double) + (size_t)E64_FR * (dim + 1) * sizeof(float);
}

// the doubles of a batched speaker's slices, in the order they lie in its group's scratch after the means and the states
struct MapSlices {
    int64_t n_pad, n_chunks, L, mb, sb, llf, partial, llpart;
    int64_t own() const { return L + mb + sb + llf + partial + llpart; }
};
static MapSlices map_slices(int K, int D, int64_t n) {
    MapSlices s;
    const int64_t n_kb = (K + E64_KB - 1) / E64_KB;
    s.n_pad = (n + E64_DFR - 1) / E64_DFR * E64_DFR;
    s.n_chunks = s.n_pad / E64_FR;                  // (the last 64-frame chunk may be all padding: zeros in every sum)
    s.L = n_kb * E64_KB * s.n_pad;
    s.mb = s.sb = n_kb * s.n_pad;
    s.llf = s.n_pad;
    s.partial = s.n_chunks * K * (2 * (int64_t)D + 1);
    s.llpart = 2 * s.n_chunks;
    return s;
}

int64_t map_speaker_scratch_bytes(int K, int D, int64_t n) {
    return (map_slices(K, D, n).own() + MAP_STATE + (int64_t)K * D) * (int64_t)sizeof(double);
}

bool plan_map_batch(int K, int D, const int64_t *lengths, int64_t S, const Parameter &param, int64_t scratch_bytes, int n_cu, MapPlan &p,
                    std::string &why) {
    p = MapPlan();
    if (K < 1 || D < 1) {
        why = "MAP enrolment: the UBM has no mixtures";
        return false;
    }
    if (S < 1 || !lengths) {
        why = "MAP enrolment: at least one speaker is needed";
        return false;
    }
    if (S > INT32_MAX) {
        why = "MAP enrolment: more than 2^31 - 1 speakers in one call";
        return false;
    }
    if (scratch_bytes < 1) {
        why = fmt("map_fit_batch_bytes must be >= 1 (the default is %lld)", MAP_DEFAULT_SCRATCH);
        return false;
    }
    if (n_cu < 1) {
        why = "MAP enrolment: the plan needs the number of compute units";
        return false;
    }
    p.K = K;
    p.D = D;
    p.n_kb = (K + E64_KB - 1) / E64_KB;
    p.lds_density = e64_density_lds(std::min(D, E64_MAX_D));
    p.lds_stats = e64_stats_lds(std::min(D, E64_MAX_D));
    p.speakers.resize((size_t)S);
    int64_t first = 0;
    for (int64_t s = 0; s < S; s++) {
        MapSpeakerPlan &sp = p.speakers[(size_t)s];
        const int64_t n = lengths[s];
        if (n < 0) {
            why = fmt("MAP enrolment: speaker %lld has a negative length", s);
            return false;
        }
        if (n > ((int64_t)1 << 38) - first) {
            why = "MAP enrolment: more than 2^38 frames in one call";
            return false;
        }
        sp.n = n;
        sp.first = first;
        first += n;
        if (n == 0) {
            sp.route = MAP_ROUTE_ERROR;                 // (the single fit's "X.size() == 0": of this speaker alone)
            p.n_error++;
        } else if (em_f64_shape_eligible(K, D, (long)n, param) && !em_small_shape_eligible(K, D, (long)n, param, n_cu)) {
            sp.route = MAP_ROUTE_BATCHED;
            p.batched.push_back((int)s);
        } else {
            sp.route = MAP_ROUTE_SINGLE;
            p.n_single++;
        }
    }
    if (p.n_kb > 65535 && !p.batched.empty()) {         // (cannot happen inside E64_MAX_CELLS; the mixture blocks are a grid's y)
        why = fmt("MAP enrolment: %lld mixture blocks, a launch takes at most 65535", p.n_kb);
        return false;
    }
    // groups: consecutive batched speakers whose scratch fits the bound; a speaker above it is a group of its own
    const int64_t KD = (int64_t)K * D;
    size_t at = 0;
    while (at < p.batched.size()) {
        MapGroupPlan g;
        g.first = (int)at;
        g.tile0 = (int64_t)p.tiles.size();
        g.chunk0 = (int64_t)p.chunks.size();
        int64_t bytes = 0;
        while (at < p.batched.size()) {
            const int64_t b = map_speaker_scratch_bytes(K, D, p.speakers[(size_t)p.batched[at]].n);
            if (g.count > 0 && b > scratch_bytes - bytes) break;
            bytes += b;
            g.count++;
            at++;
        }
        g.scratch_bytes = bytes;
        // the group's scratch, in doubles: the means of its speakers, their states, then every speaker's own slices
        int64_t off = (int64_t)g.count * (KD + MAP_STATE);
        for (int i = 0; i < g.count; i++) {
            const int s = p.batched[(size_t)g.first + i];
            MapSpeakerPlan &sp = p.speakers[(size_t)s];
            const MapSlices sl = map_slices(K, D, sp.n);
            sp.group = (int)p.groups.size();
            sp.slot = i;
            sp.n_pad = (int)sl.n_pad;
            sp.n_chunks = (int)sl.n_chunks;
            sp.scratch_bytes = map_speaker_scratch_bytes(K, D, sp.n);
            sp.off_mu = (int64_t)i * KD;
            sp.off_L = off;
            sp.off_mb = sp.off_L + sl.L;
            sp.off_sb = sp.off_mb + sl.mb;
            sp.off_llf = sp.off_sb + sl.sb;
            sp.off_partial = sp.off_llf + sl.llf;
            sp.off_llpart = sp.off_partial + sl.partial;
            off = sp.off_llpart + sl.llpart;
            // tiles and chunks counted from the speaker's own first frame; the padding after its own last frame
            for (int32_t t = 0; t < sp.n_pad / E64_DFR; t++) p.tiles.push_back(MapTileRow{sp.first, s, i, t, 0});
            for (int32_t c = 0; c < sp.n_chunks; c++) p.chunks.push_back(MapTileRow{sp.first, s, i, c, 0});
        }
        g.n_tiles = (int64_t)p.tiles.size() - g.tile0;
        g.n_chunks = (int64_t)p.chunks.size() - g.chunk0;
        if (g.n_chunks > INT32_MAX) {                   // (the tables' rows are a grid's x)
            why = fmt("MAP enrolment: a group of %lld chunks, a launch takes at most 2^31 - 1; lower map_fit_batch_bytes", g.n_chunks);
            return false;
        }
        p.max_group_bytes = std::max(p.max_group_bytes, bytes);
        p.waves = std::max(p.waves, (g.n_tiles * p.n_kb + 2 * (int64_t)n_cu - 1) / (2 * (int64_t)n_cu));
        p.groups.push_back(g);
    }
    return true;
}

}  // namespace sr
