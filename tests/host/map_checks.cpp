// map_checks.cpp -- csrc/map_plan.cpp (the routes, the groups, the tile tables and the launch shapes of the batched MAP enrolment)
// under the host sanitizers: a stand-alone program, built by tests/test_map_batch_cpu.py with g++ -fsanitize=address,undefined.
// It sweeps the plan over model shapes, ragged speaker sets, bounds and device sizes and checks the invariants the kernels rely on
// -- every batched speaker's tiles and chunks exactly once, counted from its own first frame; the slices of a group disjoint and
// inside the group's scratch; a group within the bound unless it is one speaker; a speaker's cut independent of its neighbours and
// of the bound -- and every refusal's text.
#include "map_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

using namespace sr;

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                             \
        }                                                                           \
    } while (0)

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

static Parameter params(int nit = 200, int verbosity = 0) {
    Parameter p = {};
    p.nr_iteration = nit;
    p.verbosity = verbosity;
    p.threshold = 0.01;
    p.min_covar = 1e-3;
    return p;
}

static void check_plan(int K, int D, const std::vector<int64_t> &len, int64_t bound, int n_cu) {
    MapPlan p;
    std::string why;
    const Parameter prm = params();
    if (!plan_map_batch(K, D, len.data(), (int64_t)len.size(), prm, bound, n_cu, p, why)) {
        CHECK(!why.empty());
        return;
    }
    const int64_t S = (int64_t)len.size(), KD = (int64_t)K * D;
    CHECK((int64_t)p.speakers.size() == S && (int64_t)p.n_kb * E64_KB >= K && (int64_t)(p.n_kb - 1) * E64_KB < K && p.n_kb <= 65535);
    int64_t row = 0, n_b = 0, n_s = 0, n_e = 0;
    for (int64_t s = 0; s < S; s++) {
        const MapSpeakerPlan &sp = p.speakers[(size_t)s];
        CHECK(sp.first == row && sp.n == len[(size_t)s]);
        row += len[(size_t)s];
        const bool f64 = em_f64_shape_eligible(K, D, (long)sp.n, prm), small = em_small_shape_eligible(K, D, (long)sp.n, prm, n_cu);
        const int want = sp.n == 0 ? MAP_ROUTE_ERROR : (f64 && !small) ? MAP_ROUTE_BATCHED : MAP_ROUTE_SINGLE;
        CHECK(sp.route == want);
        n_b += want == MAP_ROUTE_BATCHED;
        n_s += want == MAP_ROUTE_SINGLE;
        n_e += want == MAP_ROUTE_ERROR;
        if (want != MAP_ROUTE_BATCHED) {
            CHECK(sp.group == -1 && sp.scratch_bytes == 0);
            continue;
        }
        CHECK(sp.n_pad % E64_DFR == 0 && sp.n_pad >= sp.n && sp.n_pad - sp.n < E64_DFR && sp.n_chunks == sp.n_pad / E64_FR);
        CHECK(sp.scratch_bytes == map_speaker_scratch_bytes(K, D, sp.n) && sp.scratch_bytes % 8 == 0);
        CHECK(sp.group >= 0 && sp.group < (int)p.groups.size());
    }
    CHECK((int64_t)p.batched.size() == n_b && p.n_single == n_s && p.n_error == n_e);
    // groups: consecutive batched speakers, within the bound unless alone; the tables: every tile and chunk once, in order
    size_t at = 0;
    int64_t t_at = 0, c_at = 0, largest = 0;
    for (size_t g = 0; g < p.groups.size(); g++) {
        const MapGroupPlan &gp = p.groups[g];
        CHECK(gp.first == (int)at && gp.count >= 1 && gp.tile0 == t_at && gp.chunk0 == c_at);
        int64_t bytes = 0, tiles = 0, chunks = 0;
        std::vector<std::pair<int64_t, int64_t>> spans;              // (offset, length) of every slice, in doubles
        spans.emplace_back(0, (int64_t)gp.count * (KD + MAP_STATE));
        for (int i = 0; i < gp.count; i++) {
            const int s = p.batched[at + (size_t)i];
            const MapSpeakerPlan &sp = p.speakers[(size_t)s];
            CHECK(sp.group == (int)g && sp.slot == i && sp.off_mu == (int64_t)i * KD);
            bytes += sp.scratch_bytes;
            const int64_t n_kb = p.n_kb;
            spans.emplace_back(sp.off_L, n_kb * E64_KB * sp.n_pad);
            spans.emplace_back(sp.off_mb, n_kb * sp.n_pad);
            spans.emplace_back(sp.off_sb, n_kb * sp.n_pad);
            spans.emplace_back(sp.off_llf, (int64_t)sp.n_pad);
            spans.emplace_back(sp.off_partial, (int64_t)sp.n_chunks * K * (2 * D + 1));
            spans.emplace_back(sp.off_llpart, 2 * (int64_t)sp.n_chunks);
            for (int t = 0; t < sp.n_pad / E64_DFR; t++) {
                const MapTileRow &r = p.tiles[(size_t)(t_at + tiles + t)];
                CHECK(r.speaker == s && r.slot == i && r.first == sp.first && r.local == t);
            }
            tiles += sp.n_pad / E64_DFR;
            for (int c = 0; c < sp.n_chunks; c++) {
                const MapTileRow &r = p.chunks[(size_t)(c_at + chunks + c)];
                CHECK(r.speaker == s && r.slot == i && r.first == sp.first && r.local == c);
            }
            chunks += sp.n_chunks;
        }
        CHECK(gp.scratch_bytes == bytes && (bytes <= bound || gp.count == 1));
        CHECK(gp.n_tiles == tiles && gp.n_chunks == chunks && chunks <= INT32_MAX);
        std::sort(spans.begin(), spans.end());
        int64_t end = 0;
        for (const auto &sp : spans) {
            CHECK(sp.first == end);                                  // disjoint, no gap
            end = sp.first + sp.second;
        }
        CHECK(end * 8 == bytes);
        // greedy: the next speaker did not fit
        if (g + 1 < p.groups.size()) {
            const int next = p.batched[at + (size_t)gp.count];
            CHECK(bytes + p.speakers[(size_t)next].scratch_bytes > bound);
        }
        largest = std::max(largest, bytes);
        at += (size_t)gp.count;
        t_at += tiles;
        c_at += chunks;
    }
    CHECK(at == p.batched.size() && t_at == (int64_t)p.tiles.size() && c_at == (int64_t)p.chunks.size() && p.max_group_bytes == largest);
    // a speaker's cut is its own: alone, and under a bound of one byte, it has the same padding, chunks and scratch
    MapPlan one_each;
    CHECK(plan_map_batch(K, D, len.data(), S, prm, 1, n_cu, one_each, why));
    CHECK(one_each.groups.size() == p.batched.size());
    for (int64_t s = 0; s < S; s++) {
        const MapSpeakerPlan &a = p.speakers[(size_t)s], &b = one_each.speakers[(size_t)s];
        CHECK(a.route == b.route && a.n_pad == b.n_pad && a.n_chunks == b.n_chunks && a.scratch_bytes == b.scratch_bytes);
        if (b.route == MAP_ROUTE_BATCHED) CHECK(b.slot == 0 && b.off_mu == 0);
    }
}

int main() {
    const int Ks[] = {1, 32, 33, 64, 65, 512, 2048};
    const int Ds[] = {1, 13, 39, 40, 41, 64, 65};
    const std::vector<std::vector<int64_t>> sets = {
        {1}, {0}, {0, 0, 5}, {300}, {1, 63, 64, 65, 127, 128, 129, 300}, {3000, 3000, 3000, 0, 2999, 3001}, {8192, 8193, 1, 8192},
        std::vector<int64_t>(200, 3000)};
    for (int K : Ks)
        for (int D : Ds)
            for (const auto &s : sets)
                for (int64_t bound : {(int64_t)1, (int64_t)1 << 20, (int64_t)64 << 20, (int64_t)1 << 30})
                    for (int n_cu : {1, 256}) check_plan(K, D, s, bound, n_cu);

    // a bound of exactly one speaker's scratch, and one byte less
    {
        const std::vector<int64_t> len(5, 300);
        const int64_t one = map_speaker_scratch_bytes(130, 13, 300);
        MapPlan p;
        std::string why;
        const Parameter prm = params();
        CHECK(plan_map_batch(130, 13, len.data(), 5, prm, 2 * one, 256, p, why) && p.groups.size() == 3 && p.groups[0].count == 2 && p.groups[2].count == 1);
        CHECK(plan_map_batch(130, 13, len.data(), 5, prm, 2 * one - 1, 256, p, why) && p.groups.size() == 5);
        CHECK(plan_map_batch(130, 13, len.data(), 5, prm, one, 256, p, why) && p.groups.size() == 5);
        CHECK(plan_map_batch(130, 13, len.data(), 5, prm, one - 1, 256, p, why) && p.groups.size() == 5);
        CHECK(plan_map_batch(130, 13, len.data(), 5, prm, 5 * one, 256, p, why) && p.groups.size() == 1);
    }

    // the routes at the engines' edges
    const Parameter prm = params();
    CHECK(em_small_shape_eligible(32, 40, 3000, prm, 256) && !em_small_shape_eligible(33, 40, 3000, prm, 256));
    CHECK(!em_small_shape_eligible(32, 41, 3000, prm, 256) && !em_small_shape_eligible(32, 40, 8193, prm, 256));
    CHECK(!em_small_shape_eligible(16, 13, 3000, prm, 1));                // (the grid is bounded by half the compute units)
    CHECK(em_f64_shape_eligible(2048, 64, 8192, prm) && !em_f64_shape_eligible(2048, 65, 8192, prm) && !em_f64_shape_eligible(2048, 64, 8193, prm));
    CHECK(!em_f64_shape_eligible(64, 13, 0, prm) && !em_f64_shape_eligible(64, 13, 300, params(0)) && !em_f64_shape_eligible(64, 13, 300, params(5, 2)));
    CHECK(em_f64_shape_eligible(4096, 13, 8192, prm) && !em_f64_shape_eligible(4097, 13, 8192, prm));      // 32 Mi cells of L

    // the refusals, with their texts
    MapPlan p;
    std::string why;
    const int64_t len[3] = {5, -1, 7};
    CHECK(!plan_map_batch(0, 13, len, 1, prm, 1 << 20, 256, p, why) && has(why, "no mixtures"));
    CHECK(!plan_map_batch(8, 0, len, 1, prm, 1 << 20, 256, p, why) && has(why, "no mixtures"));
    CHECK(!plan_map_batch(8, 13, len, 0, prm, 1 << 20, 256, p, why) && has(why, "at least one speaker"));
    CHECK(!plan_map_batch(8, 13, nullptr, 1, prm, 1 << 20, 256, p, why) && has(why, "at least one speaker"));
    CHECK(!plan_map_batch(8, 13, len, 3, prm, 1 << 20, 256, p, why) && has(why, "speaker 1 has a negative length"));
    CHECK(!plan_map_batch(8, 13, len, 1, prm, 0, 256, p, why) && has(why, "map_fit_batch_bytes must be >= 1"));
    CHECK(!plan_map_batch(8, 13, len, 1, prm, 1 << 20, 0, p, why) && has(why, "compute units"));
    const int64_t huge[2] = {(int64_t)1 << 38, 1};
    CHECK(!plan_map_batch(8, 13, huge, 2, prm, 1 << 20, 256, p, why) && has(why, "2^38 frames"));

    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("map checks ok");
    return 0;
}
