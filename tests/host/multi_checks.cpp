// multi_checks.cpp -- csrc/multi_plan.cpp (which slots take work, utterances per slot, a slot's pieces and its schedule across calls)
// under the host sanitizers: a stand-alone program, built by tests/test_host_sanitizers.py with g++ -fsanitize=address,undefined
// from multi_plan.cpp alone.  It reproduces the decisions recorded in multi_table.inc and checks, over the table and over seeded
// random length vectors, what multi.cpp relies on: every utterance in exactly one active slot, a slot's list ascending, its pieces
// a contiguous cover of [0, U) with u0 <= u1, 1 <= n <= MULTI_CHUNKS, and no two active slots on one device when they merge.
#include "multi_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>

using namespace sr;

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: check failed: %s (%s)\n", __FILE__, __LINE__, #cond, context.c_str()); \
            failures++;                                                             \
        }                                                                           \
    } while (0)
static std::string context;

struct Run { int64_t count, samples; };
struct Span { int first, count; };
struct Cut { int u0, u1; };
struct PartitionCase { const char *name; std::vector<Run> lengths; int n_active; std::vector<std::vector<Span>> slots; };
struct PiecesCase { const char *name; std::vector<Run> lengths; int schedule; std::vector<Cut> pieces; };
struct State { int schedule, votes; int64_t rho_samples; };
struct Step { int op; int64_t total; int n_chunks; double a, b; int64_t first; State after; };
struct ScheduleCase { const char *name; State before; std::vector<Step> steps; };
#include "multi_table.inc"

static std::vector<int64_t> offsets_of(const std::vector<Run> &runs) {
    std::vector<int64_t> off{0};
    for (const Run &r : runs)
        for (int64_t i = 0; i < r.count; i++) off.push_back(off.back() + r.samples);
    return off;
}
static std::vector<int> list_of(const std::vector<Span> &spans) {
    std::vector<int> l;
    for (const Span &s : spans)
        for (int i = 0; i < s.count; i++) l.push_back(s.first + i);
    return l;
}

static void check_pieces(const std::vector<int64_t> &so, int schedule, const MultiPieces &p) {
    const int U = (int)so.size() - 1;
    CHECK(p.n >= 1 && p.n <= MULTI_CHUNKS && p.n <= (schedule ? 4 : MULTI_DEFAULT_PIECES));
    CHECK(p.n == 1 || (p.n <= U && (int64_t)p.n * ((int64_t)1 << 20) <= so[U]));
    CHECK(p.u0[0] == 0 && p.u1[p.n - 1] == U);
    for (int c = 0; c < p.n; c++) {
        CHECK(p.u0[c] <= p.u1[c]);
        if (c) CHECK(p.u0[c] == p.u1[c - 1]);
    }
}

// the whole plan of a call, as sr_multi_plan and multi.cpp compose it
static void check_call(const std::vector<int64_t> &off, const std::vector<int> &devices, bool merge, int schedule) {
    const int n_utt = (int)off.size() - 1, n_slots = (int)devices.size();
    const std::vector<int> active = multi_active_slots(devices.data(), n_slots, merge);
    CHECK(!active.empty() && active[0] == 0);
    for (size_t a = 0; a < active.size(); a++) {
        CHECK(active[a] >= 0 && active[a] < n_slots && (a == 0 || active[a] > active[a - 1]));
        if (merge)
            for (size_t b = 0; b < a; b++) CHECK(devices[active[a]] != devices[active[b]]);
    }
    if (!merge) CHECK((int)active.size() == n_slots);
    for (int k = 0; k < n_slots; k++) {                   // every device that has a slot has an active one
        bool served = false;
        for (int a : active) served = served || devices[a] == devices[k];
        CHECK(served);
    }
    const auto utts = multi_partition(off.data(), n_utt, (int)active.size());
    CHECK(utts.size() == active.size());
    std::vector<int> seen((size_t)n_utt, 0);
    for (const auto &l : utts) {
        for (size_t i = 0; i < l.size(); i++) {
            CHECK(l[i] >= 0 && l[i] < n_utt && (i == 0 || l[i] > l[i - 1]));
            if (l[i] >= 0 && l[i] < n_utt) seen[l[i]]++;
        }
        const std::vector<int64_t> so = multi_slot_offsets(off.data(), l);
        CHECK(so.size() == l.size() + 1 && so[0] == 0);
        for (size_t i = 0; i < l.size(); i++) CHECK(so[i + 1] - so[i] == off[l[i] + 1] - off[l[i]]);
        check_pieces(so, schedule, plan_slot_pieces(so.data(), (int)l.size(), schedule));
        // the runs of neighbours: every position once, in order, maximal
        int next = 0;
        for_each_run(l.data(), 0, (int)l.size(), [&](int i, int j) {
            CHECK(i == next && j >= i && j < (int)l.size() && l[j] - l[i] == j - i);
            CHECK(j + 1 == (int)l.size() || l[j + 1] != l[j] + 1);
            next = j + 1;
        });
        CHECK(next == (int)l.size());
    }
    for (int u = 0; u < n_utt; u++) CHECK(seen[u] == 1);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {                                   // xorshift64*
    rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

int main() {
    const std::vector<std::vector<int>> device_sets = {{0}, {0, 0}, {0, 1}, {0, 1, 0}, {0, 1, 2, 3, 0, 1, 2, 3}, {0, 0, 0, 1}};

    for (const PartitionCase &c : kPartitionCases) {
        context = c.name;
        const std::vector<int64_t> off = offsets_of(c.lengths);
        const auto utts = multi_partition(off.data(), (int)off.size() - 1, c.n_active);
        CHECK((int)utts.size() == c.n_active && c.slots.size() == utts.size());
        for (size_t k = 0; k < utts.size() && k < c.slots.size(); k++) CHECK(utts[k] == list_of(c.slots[k]));
        for (const auto &d : device_sets)
            for (int merge = 0; merge < 2; merge++) check_call(off, d, merge != 0, 0);
    }
    context = "no active slot";
    const int64_t two[3] = {0, 5, 9};
    CHECK(multi_partition(two, 2, 0).empty() && multi_active_slots(nullptr, 0, true).empty());

    for (const PiecesCase &c : kPiecesCases) {
        context = std::string(c.name) + (c.schedule ? ", growing" : ", equal");
        const std::vector<int64_t> so = offsets_of(c.lengths);
        const MultiPieces p = plan_slot_pieces(so.data(), (int)so.size() - 1, c.schedule);
        CHECK(p.n == (int)c.pieces.size());
        for (int i = 0; i < p.n && i < (int)c.pieces.size(); i++) CHECK(p.u0[i] == c.pieces[i].u0 && p.u1[i] == c.pieces[i].u1);
        check_pieces(so, c.schedule, p);
        for (const auto &d : device_sets) check_call(so, d, true, c.schedule);
    }

    for (const ScheduleCase &c : kScheduleCases) {
        MultiSchedule ms;
        ms.schedule = c.before.schedule, ms.votes = c.before.votes, ms.rho_samples = c.before.rho_samples;
        int at = 0;
        for (const Step &st : c.steps) {
            context = std::string(c.name) + ", step " + std::to_string(at++);
            const MultiSchedule was = ms;
            if (st.op == 0) {
                const bool reset = multi_first_schedule(ms, st.total, st.a, st.b);
                CHECK(reset || (ms.schedule == was.schedule && ms.votes == was.votes));
                CHECK(!reset || ms.votes == 0);
                CHECK(ms.rho_samples == was.rho_samples);
            } else {
                multi_vote(ms, st.total, st.n_chunks, st.a, st.first);
            }
            CHECK(ms.schedule == st.after.schedule && ms.votes == st.after.votes && ms.rho_samples == st.after.rho_samples);
            CHECK((ms.schedule == 0 || ms.schedule == 1) && (ms.votes == 0 || ms.votes == 1));
        }
    }

    // seeded random length vectors: few and many utterances, even and wildly uneven, with zero-length ones, small and large totals
    for (int trial = 0; trial < 400; trial++) {
        context = "random trial " + std::to_string(trial);
        const int n_utt = (int)(rnd() % (trial % 4 == 0 ? 12 : 400));
        const int64_t scale = (int64_t)1 << (4 + rnd() % 17);
        std::vector<int64_t> off{0};
        for (int u = 0; u < n_utt; u++) {
            const uint64_t kind = rnd() % 16;
            const int64_t len = kind == 0 ? 0 : kind == 1 ? (int64_t)(rnd() % (uint64_t)(scale * 64)) : (int64_t)(rnd() % (uint64_t)scale);
            off.push_back(off.back() + len);
        }
        const auto &d = device_sets[trial % device_sets.size()];
        check_call(off, d, (trial / 6) % 2 == 0, (trial / 12) % 2);
    }

    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("multi checks ok");
    return 0;
}
