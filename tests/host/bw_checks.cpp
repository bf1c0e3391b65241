// bw_checks.cpp -- csrc/bw_plan.cpp (the refusals, the range table, the groups and the launch shapes of the batched Baum-Welch
// statistics) under the host sanitizers: a stand-alone program, built by tests/test_bw_cpu.py with g++ -fsanitize=address,undefined.
// It sweeps the plan over model shapes, ragged batches, range lengths, bounds and device sizes, checks the invariants the kernels
// rely on -- every frame in exactly one range, no range across an utterance, an utterance's cut independent of its neighbours and
// of the bound, the slabs of a group within the bound -- and every refusal's text.
#include "bw_plan.hpp"

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

// the cut of utterance u as (first row within the utterance, rows) pairs
static std::vector<std::pair<int64_t, int64_t>> cut_of(const BwPlan &p, const std::vector<int64_t> &len, int64_t u) {
    int64_t off = 0;
    for (int64_t i = 0; i < u; i++) off += len[i];
    std::vector<std::pair<int64_t, int64_t>> c;
    for (const BwRange &r : p.ranges)
        if (r.utt == u) c.emplace_back(r.first - off, r.rows);
    return c;
}

static void check_plan(int K, int D, const std::vector<int64_t> &len, int64_t range_frames, int64_t bound, int n_cu) {
    BwPlan p;
    std::string why;
    if (!plan_bw(K, D, len.data(), (int64_t)len.size(), range_frames, bound, n_cu, p, why)) {
        CHECK(!why.empty());
        return;
    }
    CHECK(p.dp >= D && p.dp <= BW_MAX_DIM && p.ncb * 16 >= p.dp + 1 && (p.ncb - 1) * 16 < p.dp + 1);
    CHECK((int64_t)p.n_mix_blocks * BW_WG_MIX >= K && (int64_t)(p.n_mix_blocks - 1) * BW_WG_MIX < K && p.n_mix_blocks <= 65535);
    CHECK(p.slab_bytes == (int64_t)p.n_mix_blocks * BW_WG_MIX * p.ncb * 16 * 8 && p.slab_bytes <= bound);
    CHECK(p.stats_lds > 0 && p.stats_lds <= 80 * 1024);                         // two workgroups share a compute unit's 160 KiB
    CHECK(p.reduce_blocks * BW_WG >= (int64_t)K * (D + 1) && (p.reduce_blocks - 1) * BW_WG < (int64_t)K * (D + 1));
    // every frame exactly once, in order, no range across an utterance
    int64_t row = 0, total = 0;
    size_t at = 0;
    for (size_t u = 0; u < len.size(); u++) {
        const int64_t end = row + len[u];
        const int64_t want = bw_range_rows(len[u], K, D, range_frames);
        CHECK(want >= 1 && (range_frames == 0 || want == range_frames));
        int64_t n_u = 0;
        while (at < p.ranges.size() && p.ranges[at].utt == (int32_t)u) {
            const BwRange &r = p.ranges[at];
            CHECK(r.first == row && r.rows >= 1 && r.first + r.rows <= end);
            CHECK(r.rows == want || r.first + r.rows == end);                   // only an utterance's last range is short
            row += r.rows;
            at++;
            n_u++;
        }
        CHECK(row == end);
        if (range_frames == 0) CHECK(n_u <= BW_MAX_AUTO_RANGES);
        total += len[u];
    }
    CHECK(at == p.ranges.size());
    CHECK(p.lse_grid * BW_WG >= total && (p.lse_grid - 1) * BW_WG < total);
    // groups: within the bound, covering the table
    const int64_t n = (int64_t)p.ranges.size();
    CHECK(p.group_ranges >= 1 && p.group_ranges * p.slab_bytes <= bound && p.group_ranges < ((int64_t)1 << 31));
    CHECK(n == 0 ? p.n_groups == 0 : ((p.n_groups - 1) * p.group_ranges < n && p.n_groups * p.group_ranges >= n));
    CHECK(p.stats_rounds >= (n > 0 ? 1 : 0));
    // an utterance's cut is its own: alone, and under another bound, it is cut the same
    for (size_t u = 0; u < len.size(); u++) {
        BwPlan alone, other;
        const std::vector<int64_t> one{len[u]};
        CHECK(plan_bw(K, D, one.data(), 1, range_frames, bound, n_cu, alone, why));
        CHECK(cut_of(alone, one, 0) == cut_of(p, len, (int64_t)u));
        CHECK(plan_bw(K, D, len.data(), (int64_t)len.size(), range_frames, p.slab_bytes, 7, other, why));
        CHECK(cut_of(other, len, (int64_t)u) == cut_of(p, len, (int64_t)u));
        CHECK(other.group_ranges == 1 && other.n_groups == n);
    }
}

int main() {
    const int Ks[] = {1, 17, 64, 65, 256, 512, 2048};
    const int Ds[] = {1, 13, 39, 40};
    const std::vector<std::vector<int64_t>> batches = {
        {}, {0}, {0, 0, 0}, {1}, {300}, {0, 1, 3, 63, 64, 65, 127, 128, 129, 259}, {1023, 1024, 1025, 2051, 0, 5},
        {262144, 262145, 300000}, {1000000}};
    const int64_t Rs[] = {0, 1, 128, 1000, (int64_t)1 << 30};
    const int64_t bounds[] = {(int64_t)1 << 20, (int64_t)3 << 20, (int64_t)1 << 30};
    for (int K : Ks)
        for (int D : Ds)
            for (const auto &b : batches)
                for (int64_t R : Rs) {
                    int64_t tot = 0;
                    for (int64_t l : b) tot += l;
                    if (R == 1 && tot > 3000) continue;                         // (a range per frame: small batches only)
                    for (int64_t bound : bounds)
                        for (int n_cu : {1, 256}) check_plan(K, D, b, R, bound, n_cu);
                }

    // the automatic cut: 1024 frames, grown in whole tiles once an utterance would have more than 256 ranges
    CHECK(bw_range_rows(0, 512, 39, 0) == 1024 && bw_range_rows(262144, 512, 39, 0) == 1024 && bw_range_rows(262145, 512, 39, 0) == 1152);
    CHECK(bw_range_rows(1000000, 8, 1, 0) == 3968 && bw_range_rows(5, 8, 1, 77) == 77);

    // the refusals, in order, with their texts
    std::string why;
    CHECK(!bw_check(true, 0, 0, 8, 13, 13, why) && has(why, "empty model set"));
    CHECK(!bw_check(false, 2, 0, 8, 13, 13, why) && has(why, "take a feature batch") && has(why, "sr_mfcc_extract_batch"));
    CHECK(!bw_check(true, 2, 2, 8, 13, 13, why) && has(why, "model index 2 outside [0, 2)"));
    CHECK(!bw_check(true, 2, -1, 8, 13, 13, why) && has(why, "model index -1 outside [0, 2)"));
    CHECK(!bw_check(true, 2, 1, 0, 13, 13, why) && has(why, "no mixtures"));
    CHECK(!bw_check(true, 2, 1, 8, 41, 41, why) && has(why, "up to 40 dimensions, the model has 41"));
    CHECK(!bw_check(true, 2, 1, 65535 * 64 + 1, 13, 13, why) && has(why, "at most 4194240"));
    CHECK(!bw_check(true, 2, 1, 8, 13, 39, why) && has(why, "feature dim 39 != model dim 13"));
    CHECK(bw_check(true, 2, 1, 8, 40, 40, why));
    BwPlan p;
    const int64_t len[3] = {5, -1, 7};
    CHECK(!plan_bw(8, 41, len, 1, 0, 1 << 20, 256, p, why) && has(why, "up to 40 dimensions"));
    CHECK(!plan_bw(8, 13, len, 3, 0, 1 << 20, 256, p, why) && has(why, "utterance 1 has a negative length"));
    CHECK(!plan_bw(8, 13, len, 1, -1, 1 << 20, 256, p, why) && has(why, "bw_range_frames must be 0 (automatic) or 1 .. 1073741824"));
    CHECK(!plan_bw(8, 13, len, 1, ((int64_t)1 << 30) + 1, 1 << 20, 256, p, why) && has(why, "bw_range_frames"));
    CHECK(!plan_bw(8, 13, len, 1, 0, 1 << 20, 0, p, why) && has(why, "compute units"));
    CHECK(!plan_bw(8, 13, nullptr, 1, 0, 1 << 20, 256, p, why) && has(why, "utterance table"));
    CHECK(!plan_bw(512, 39, len, 1, 0, 196607, 256, p, why) && has(why, "below one range's slab of 196608") && has(why, "bw_scratch_mib"));
    CHECK(plan_bw(512, 39, len, 1, 0, 196608, 256, p, why) && p.group_ranges == 1 && p.n_groups == 1);
    const int64_t huge[2] = {(int64_t)1 << 38, 1};
    CHECK(!plan_bw(8, 13, huge, 2, 1 << 30, 1 << 20, 256, p, why) && has(why, "2^38 frames"));

    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("bw checks ok");
    return 0;
}
