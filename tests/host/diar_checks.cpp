// diar_checks.cpp -- csrc/diar_plan.cpp swept over dimensions, segment lengths, batches and bounds, with its refusals and the two
// functions on a merge log; a stand-alone program for the host sanitizers (tests/test_diar_cpu.py builds it with
// -fsanitize=address,undefined).
#include "diar_plan.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

using namespace sr;

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            std::exit(1);                                                     \
        }                                                                     \
    } while (0)

int main() {
    std::string why;
    DiarPlan p;
    DiarParams prm;
    long plans = 0;
    // base segments
    for (int64_t L : {1, 2, 7, 100})
        for (int64_t n : {(int64_t)0, (int64_t)1, L - 1, L, L + 1, 2 * L + L / 2, (int64_t)360000}) {
            const int64_t ns = diar_segments(n, L);
            CHECK(ns == (n <= 0 ? 0 : n < L ? 1 : n / L));
            if (ns > 0) CHECK((ns - 1) * L < n && n - (ns - 1) * L < 2 * L);      // the last segment: at least one frame, fewer than 2 L
        }
    CHECK(diar_segments(5, 0) == 0 && diar_segments(-1, 3) == 0);
    // the bucket and the layout of a statistic for every D
    for (int D = 1; D <= DIAR_MAX_D; D++) {
        const int b = diar_bucket(D);
        CHECK(b >= D && b <= 64 && b % 16 == 0 && (b == 16 || b - 16 < D));
        CHECK(diar_stat_len(D) == 1 + D + D * (D + 1) / 2);
        const int64_t len[2] = {1000, 37};
        prm = DiarParams();
        CHECK(plan_diar(D, prm, len, 2, DIAR_DEFAULT_SCRATCH, p, why));
        plans++;
        CHECK(p.bucket == b && p.stat_len == diar_stat_len(D));
        CHECK(p.entries_per_lane >= 1 && p.entries_per_lane <= DIAR_STATS_MAX_ENTRIES);
        CHECK((int64_t)p.entries_per_lane * DIAR_STATS_WG >= p.stat_len - 1);     // every entry of (s, Q) has an owner
        CHECK(p.stats_lds_bytes == DIAR_STATS_CHUNK * D * 4 && p.stats_lds_bytes <= 65536);
        CHECK(p.change_lds_bytes == 2 * p.stat_len * 8 && p.change_lds_bytes <= 65536);
        CHECK(p.n_seg[0] == 10 && p.n_seg[1] == 1 && p.group_begin.size() == 2 && p.group_begin[1] == 2);
    }
    // groups respect the bound and cover every recording once, in order
    for (int D : {1, 13, 39, 64})
        for (int64_t L : {10, 100})
            for (int change : {DIAR_CHANGE_UNIFORM, DIAR_CHANGE_BIC}) {
                std::vector<int64_t> len;
                for (int u = 0; u < 23; u++) len.push_back((u * 7919) % 3001);
                prm = DiarParams();
                prm.L = (int)L;
                prm.change = change;
                int64_t largest = 0;
                for (int64_t n : len) largest = std::max(largest, diar_recording_bytes(D, diar_segments(n, L), std::min<int64_t>(diar_segments(n, L), DIAR_MAX_INIT)));
                for (int64_t bound : {largest, largest + 1, 2 * largest, 3 * largest + 17, DIAR_DEFAULT_SCRATCH}) {
                    CHECK(plan_diar(D, prm, len.data(), (int)len.size(), bound, p, why));
                    plans++;
                    CHECK(p.group_begin.front() == 0 && p.group_begin.back() == (int)len.size());
                    for (size_t g = 0; g + 1 < p.group_begin.size(); g++) {
                        CHECK(p.group_begin[g] < p.group_begin[g + 1]);
                        int64_t sum = 0;
                        for (int u = p.group_begin[g]; u < p.group_begin[g + 1]; u++) sum += p.bytes[(size_t)u];
                        CHECK(sum <= bound);
                        // greedy: the next recording would not have fitted
                        if (g + 2 < p.group_begin.size()) CHECK(sum + p.bytes[(size_t)p.group_begin[g + 1]] > bound);   // (23 recordings: far from the count cap)
                    }
                    for (size_t u = 0; u < len.size(); u++) {
                        CHECK(p.n_seg[u] == diar_segments(len[u], L) && p.n_init_bound[u] == std::min<int64_t>(p.n_seg[u], DIAR_MAX_INIT));
                        CHECK(p.bytes[u] == diar_recording_bytes(D, p.n_seg[u], p.n_init_bound[u]));
                    }
                }
                CHECK(!plan_diar(D, prm, len.data(), (int)len.size(), largest - 1, p, why));
                CHECK(why.find("larger L") != std::string::npos && why.find("bytes") != std::string::npos);
            }
    // a group holds at most 65535 recordings (the grid's y), however small they are
    {
        std::vector<int64_t> len((size_t)2 * DIAR_MAX_GROUP + 3, 5);
        len[7] = 0;
        prm = DiarParams();
        CHECK(plan_diar(1, prm, len.data(), (int)len.size(), DIAR_DEFAULT_SCRATCH, p, why));
        CHECK(p.group_begin.size() == 4 && p.group_begin[1] == DIAR_MAX_GROUP && p.group_begin[2] == 2 * DIAR_MAX_GROUP);
        CHECK(p.group_begin[3] == (int)len.size());
    }
    // the pair kernel's index arithmetic: every pair once, in row-major order (every n up to 300; the ends and a stride at 4096)
    for (int64_t n = 2; n <= 300; n++) {
        int64_t q = 0;
        for (int64_t i = 0; i < n; i++)
            for (int64_t j = i + 1; j < n; j++, q++) {
                int64_t gi, gj;
                diar_pair_of(n, q, gi, gj);
                CHECK(gi == i && gj == j);
            }
        CHECK(q == n * (n - 1) / 2);
    }
    {
        const int64_t n = DIAR_MAX_INIT, total = n * (n - 1) / 2;
        for (int64_t q = 0; q < total; q += (q < 10000 || q > total - 10000) ? 1 : 997) {
            int64_t gi, gj;
            diar_pair_of(n, q, gi, gj);
            CHECK(gi >= 0 && gi < gj && gj < n && gi * (2 * n - gi - 1) / 2 + (gj - gi - 1) == q);
        }
    }
    prm = DiarParams();
    CHECK(plan_diar(13, prm, nullptr, 0, 1 << 20, p, why) && p.group_begin.size() == 1);
    // the 4096 limit
    {
        prm = DiarParams();
        prm.L = 1;
        prm.change = DIAR_CHANGE_UNIFORM;
        const int64_t ok_len = 4096, bad_len = 4097;
        CHECK(plan_diar(2, prm, &ok_len, 1, (int64_t)1 << 40, p, why) && p.n_init_bound[0] == 4096);
        CHECK(!plan_diar(2, prm, &bad_len, 1, (int64_t)1 << 40, p, why) && why.find("4096") != std::string::npos);
        prm.change = DIAR_CHANGE_BIC;           // the detector decides: the plan takes the bound
        CHECK(plan_diar(2, prm, &bad_len, 1, (int64_t)1 << 40, p, why) && p.n_seg[0] == 4097 && p.n_init_bound[0] == 4096);
    }
    // refusals
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    auto with = [](auto f) {
        DiarParams q;
        f(q);
        return q;
    };
    CHECK(diar_check_params(1, DiarParams(), why) && diar_check_params(64, DiarParams(), why));
    CHECK(!diar_check_params(0, DiarParams(), why) && !diar_check_params(65, DiarParams(), why) && why.find("64") != std::string::npos);
    CHECK(!diar_check_params(13, with([](DiarParams &q) { q.L = 0; }), why));
    CHECK(!diar_check_params(13, with([](DiarParams &q) { q.m = 0; }), why));
    CHECK(!diar_check_params(13, with([](DiarParams &q) { q.change = 2; }), why) && !diar_check_params(13, with([](DiarParams &q) { q.change = -1; }), why));
    CHECK(!diar_check_params(13, with([](DiarParams &q) { q.lambda = 0.0; }), why) && !diar_check_params(13, with([&](DiarParams &q) { q.lambda = nan; }), why));
    CHECK(!diar_check_params(13, with([&](DiarParams &q) { q.lambda = inf; }), why));
    CHECK(!diar_check_params(13, with([](DiarParams &q) { q.ridge = -1e-9; }), why) && !diar_check_params(13, with([&](DiarParams &q) { q.ridge = inf; }), why));
    CHECK(!diar_check_params(13, with([&](DiarParams &q) { q.ridge = nan; }), why));
    CHECK(diar_check_params(13, with([](DiarParams &q) { q.ridge = 0.0; }), why));
    CHECK(!diar_check_params(13, with([&](DiarParams &q) { q.threshold = nan; }), why));
    CHECK(diar_check_params(13, with([&](DiarParams &q) { q.threshold = inf; }), why) && diar_check_params(13, with([&](DiarParams &q) { q.threshold = -inf; }), why));
    CHECK(!ahc_check_stop(0.0, 0, 0, why) && !ahc_check_stop(0.0, 3, 2, why) && !ahc_check_stop(0.0, 1, -1, why));
    CHECK(ahc_check_stop(0.0, 3, 3, why) && ahc_check_stop(0.0, 3, 0, why) && ahc_check_stop(0.0, 1, 7, why));
    const int64_t neg = -1;
    CHECK(!plan_diar(13, DiarParams(), &neg, 1, 1 << 20, p, why) && !plan_diar(13, DiarParams(), nullptr, 1, 1 << 20, p, why));
    CHECK(!plan_diar(13, DiarParams(), nullptr, 0, 0, p, why));
    // the matrix's refusals
    {
        std::vector<double> d = {0, 1, 2, 1, 0, 3, 2, 3, 0};
        CHECK(ahc_check_matrix(3, d.data(), 0, why) && ahc_check_matrix(0, nullptr, 2, why));
        CHECK(!ahc_check_matrix(3, d.data(), 3, why) && !ahc_check_matrix(3, d.data(), -1, why) && !ahc_check_matrix(3, nullptr, 0, why));
        CHECK(!ahc_check_matrix(DIAR_MAX_INIT + 1, d.data(), 0, why));
        d[1] = 1.5;
        CHECK(!ahc_check_matrix(3, d.data(), 0, why) && why.find("symmetric") != std::string::npos);
        d[1] = d[3] = nan;
        CHECK(!ahc_check_matrix(3, d.data(), 0, why));
        d[1] = d[3] = -inf;
        CHECK(!ahc_check_matrix(3, d.data(), 0, why));
        d[1] = d[3] = inf;
        CHECK(ahc_check_matrix(3, d.data(), 0, why));
        d[0] = nan;                             // (the diagonal is not read)
        CHECK(ahc_check_matrix(3, d.data(), 0, why));
    }
    // the labels of a log and its cuts
    {
        const int32_t mi[4] = {1, 0, 0, 0}, mj[4] = {3, 2, 4, 1};
        const double md[4] = {-5.0, -3.0, -4.0, 2.0};
        int32_t lab[5];
        CHECK(diar_labels(5, mi, mj, 0, lab) == 5 && lab[0] == 0 && lab[4] == 4);
        CHECK(diar_labels(5, mi, mj, 2, lab) == 3 && lab[0] == 0 && lab[1] == 1 && lab[2] == 0 && lab[3] == 1 && lab[4] == 2);
        CHECK(diar_labels(5, mi, mj, 4, lab) == 1 && lab[3] == 0);
        CHECK(diar_labels(0, nullptr, nullptr, 0, nullptr) == 0);
        CHECK(diar_labels(5, mi, mj, 5, lab) == -1);
        const int32_t bad_i[2] = {1, 1}, bad_j[2] = {3, 3};
        CHECK(diar_labels(5, bad_i, bad_j, 2, lab) == -1);                        // 3 is gone
        const int32_t rev_i[1] = {3}, rev_j[1] = {1};
        CHECK(diar_labels(5, rev_i, rev_j, 1, lab) == -1);
        CHECK(diar_cut_steps(5, md, 4, 0.0, 1, 0) == 3 && diar_cut_steps(5, md, 4, -3.5, 1, 0) == 1);     // a prefix: step 2 is not reached
        CHECK(diar_cut_steps(5, md, 4, inf, 1, 0) == 4 && diar_cut_steps(5, md, 4, inf, 3, 0) == 2);
        CHECK(diar_cut_steps(5, md, 4, -inf, 1, 2) == 3 && diar_cut_steps(5, md, 4, -inf, 2, 2) == 3 && diar_cut_steps(5, md, 4, -inf, 1, 0) == 0);
        const double stuck[2] = {-1.0, inf};
        CHECK(diar_cut_steps(5, stuck, 2, inf, 1, 1) == 1);                       // never a step at +inf
    }
    std::printf("diar checks ok: %ld plans\n", plans);
    return 0;
}
