// full_checks.cpp -- csrc/full_plan.cpp (the group cut, the per-speaker tables, the work lists and the buffer sizes of the float64
// full-covariance fit) under the host sanitizers: a stand-alone program, built by tests/test_full_plan_cpu.py with
// g++ -fsanitize=address,undefined.  It sweeps the plan over K 1..65, D 1..64, the frame-count edges of tests/fullfit_cases.py,
// ragged speaker sets of 1 to 300 speakers (and one past the 65535 cap) and bounds from 1 byte to 4 GiB, and checks what the
// driver and the kernels of csrc/gmm_full_fit.hip rely on, and every refusal.
//
// What fe_cov and fe_chol require of a speaker's (n_chunks, chunk), read from their bodies:
//   * fe_cov's workgroup (k, c) sums frames [c chunk, min(n, (c + 1) chunk)) and writes partial[(c K + k) npairs + p] for every pair
//     p, also when its range is empty (zeros);
//   * fe_chol adds partial[(c K + k) npairs + p] over c = 0 .. n_chunks - 1, in that order, and reads nothing else of the frames.
//   So every frame must lie in exactly one chunk 0 .. n_chunks - 1 (chunk >= 1 and n_chunks chunk >= n), every c of that range must
//   be a row of the covariance work list in every iteration (fe_chol would add a stale sum otherwise), no other c may be (it would
//   write past the slice), and the slice of `partial` must hold n_chunks K npairs doubles.  Nothing is asked of chunk's divisibility:
//   both kernels handle a step tail (t0 + fr < e).
#include "full_plan.hpp"

#include <climits>
#include <cstdio>
#include <cstdlib>

using namespace sr;

static int failures = 0;
static long plans = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                             \
        }                                                                           \
    } while (0)

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

// splitmix64 of (seed, index), as tests/em_parent_cases.py's _uniform
static uint64_t hash64(uint64_t seed, uint64_t i) {
    uint64_t z = (i + 1) * 0x9E3779B97F4A7C15ull + seed * 0xD1342543DE82EF95ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// fe_spk_bytes as the driver had it before the plan existed, term by term: X, lp, lpn, partial, prec and cov, mu, w logw logdet
// nk, head; the three work lists; the labels; the table entry and the record
static int64_t closed_form_bytes(int64_t n, int K, int D) {
    const int64_t KD = (int64_t)K * D;
    const int64_t n_chunks = std::min<int64_t>(32, (n + 255) / 256), partial = n_chunks * K * (D * (D + 1) / 2);
    return 8 * (n * D + n * K + n + partial + 2 * KD * D + KD + 4 * K + 2) + 8 * ((n + 31) / 32 + (n + 255) / 256 + n_chunks) + 4 * n + 72 + 16;
}

static void check_list(const std::vector<FullWork> &list, int64_t at, int64_t len, const FullSpeakerPlan *spk, int count, long (*blocks)(const FullSpeakerPlan &)) {
    // every (slot, block) of the group exactly once, in ascending order
    int64_t i = at;
    for (int s = 0; s < count; s++)
        for (long b = 0; b < blocks(spk[s]); b++, i++) {
            CHECK(i < at + len && i < (int64_t)list.size());
            if (i >= (int64_t)list.size()) return;
            CHECK(list[(size_t)i].slot == s && list[(size_t)i].block == b);
        }
    CHECK(i == at + len);
}

static void check_plan(int K, int D, const std::vector<int64_t> &len, int64_t bound) {
    const int64_t S = (int64_t)len.size();
    std::vector<int> given((size_t)S), iters((size_t)S);
    for (int64_t s = 0; s < S; s++) {
        given[(size_t)s] = (int)(hash64(7, (uint64_t)s) & 1);
        iters[(size_t)s] = 1 + (int)(hash64(9, (uint64_t)s) % 200);
    }
    FullFitPlan p;
    std::string why;
    plans++;
    if (!plan_full_fit(K, D, len.data(), given.data(), iters.data(), S, bound, p, why)) {
        CHECK(!why.empty());
        CHECK(false);               // nothing in the sweep is a shape the plan may refuse
        return;
    }
    const int64_t npairs = D * (D + 1) / 2;
    CHECK(p.K == K && p.D == D && (int64_t)p.speakers.size() == S && !p.groups.empty());
    CHECK(p.lds_logprob == 8 * ((size_t)D * D + D + 32 * (D + 1) + 256) && p.lds_logprob <= 160 * 1024);
    CHECK(K <= 65535);              // a grid's y in fe_logprob and fe_cov
    int next = 0;
    int64_t lp = 0, lse = 0, cov = 0, max_bytes = 0;
    for (size_t gi = 0; gi < p.groups.size(); gi++) {
        const FullGroupPlan &g = p.groups[gi];
        const FullCounts &c = g.counts;
        // the groups partition the speakers in order; the three lists lie group after group
        CHECK(g.first == next && g.count >= 1 && g.count <= 65535 && g.lp0 == lp && g.lse0 == lse && g.cov0 == cov);
        next += g.count;
        lp += c.wl_lp;
        lse += c.wl_lse;
        cov += c.wl_cov;
        const FullSpeakerPlan *spk = p.speakers.data() + g.first;
        int64_t rows = 0, partial = 0, sum_bytes = 0, n_lp = 0, n_lse = 0, n_cov = 0;
        int max_iter = 0;
        bool any_kmeans = false, any_given = false;
        for (int i = 0; i < g.count; i++) {
            const FullSpeakerPlan &sp = spk[i];
            const int64_t n = len[(size_t)(g.first + i)];
            CHECK(sp.n == n && sp.group == (int)gi && sp.slot == i);
            CHECK(sp.row0 == rows);                         // prefix sums of the lengths
            CHECK(sp.o_partial == partial);                 // the slices tile `partial` without gap or overlap
            rows += n;
            partial += (int64_t)fe_partial_len((long)n, K, D);
            CHECK(sp.n_chunks == fe_n_chunks((long)n) && sp.n_chunks >= 1 && sp.n_chunks <= 32);
            // fe_cov / fe_chol (above): chunks 0 .. n_chunks - 1 cover the frames, each once; the slice holds their sums
            CHECK(sp.chunk >= 1 && (int64_t)sp.n_chunks * sp.chunk >= n && (int64_t)(sp.n_chunks - 1) * sp.chunk < n);
            CHECK((int64_t)fe_partial_len((long)n, K, D) == sp.n_chunks * K * npairs);
            CHECK(sp.bytes == closed_form_bytes(n, K, D) && sp.bytes == full_speaker_bytes(K, D, n));
            // what is narrowed to int in the tables and the lists
            CHECK(fe_lp_blocks((long)n) <= INT_MAX && (n + sp.n_chunks - 1) / sp.n_chunks <= INT_MAX);
            sum_bytes += sp.bytes;
            n_lp += fe_lp_blocks((long)n);
            n_lse += fe_lse_blocks((long)n);
            n_cov += sp.n_chunks;
            max_iter = std::max(max_iter, iters[(size_t)(g.first + i)]);
            (given[(size_t)(g.first + i)] ? any_given : any_kmeans) = true;
        }
        CHECK(g.rows == rows && g.max_iter == max_iter && g.any_kmeans == any_kmeans && g.any_given == any_given);
        // the lists: lengths by the per-speaker formulas, every (slot, block) once and ascending
        CHECK(c.wl_lp == n_lp && c.wl_lse == n_lse && c.wl_cov == n_cov);
        CHECK(c.wl_lp <= INT_MAX && c.wl_lse <= INT_MAX && c.wl_cov <= INT_MAX);         // grid x, narrowed to unsigned at the launch
        check_list(p.wl_lp, g.lp0, c.wl_lp, spk, g.count, [](const FullSpeakerPlan &sp) { return fe_lp_blocks((long)sp.n); });
        check_list(p.wl_lse, g.lse0, c.wl_lse, spk, g.count, [](const FullSpeakerPlan &sp) { return fe_lse_blocks((long)sp.n); });
        check_list(p.wl_cov, g.cov0, c.wl_cov, spk, g.count, [](const FullSpeakerPlan &sp) { return (long)sp.n_chunks; });
        // every buffer
        const int64_t SK = (int64_t)g.count * K;
        CHECK(c.X == rows * D && c.lp == rows * K && c.lpn == rows && c.label == rows && c.partial == partial);
        CHECK(c.w == SK && c.logw == SK && c.logdet == SK && c.nk == SK && c.mu == SK * D && c.prec == SK * D * D && c.cov == SK * D * D);
        CHECK(c.head == 2 * (int64_t)g.count && c.spk == g.count && c.rec == g.count);
        // a group's bytes: the sum over its buffers, which is the sum over its speakers alone
        const int64_t by_buffers = 8 * (c.X + c.w + c.logw + c.mu + c.prec + c.logdet + c.cov + c.lp + c.lpn + c.nk + c.partial + c.head) +
                                   72 * c.spk + 16 * c.rec + 8 * (c.wl_lp + c.wl_lse + c.wl_cov) + 4 * c.label;
        CHECK(g.bytes == by_buffers && g.bytes == c.bytes() && g.bytes == sum_bytes);
        max_bytes = std::max(max_bytes, g.bytes);
        // above the bound only alone; greedy: the next speaker would not have fitted, or the cap was reached
        CHECK(g.bytes <= bound || g.count == 1);
        if (next < S) CHECK(g.count == 65535 || g.bytes + closed_form_bytes(len[(size_t)next], K, D) > bound);
    }
    CHECK(next == S && lp == (int64_t)p.wl_lp.size() && lse == (int64_t)p.wl_lse.size() && cov == (int64_t)p.wl_cov.size());
    CHECK(p.max_group_bytes == max_bytes);
}

static void check_refusals() {
    FullFitPlan p;
    std::string why;
    // (32 (2^31 - 1) + 1 frames: the first count whose density blocks pass INT_MAX; refused before a list is built)
    const int64_t one[1] = {100}, none[1] = {0}, neg[2] = {5, -2}, huge[1] = {32 * (int64_t)INT_MAX + 1};
    const int given[2] = {0, 0}, iters[2] = {100, 100};
    CHECK(!plan_full_fit(0, 3, one, given, iters, 1, 1 << 20, p, why) && has(why, "K 0"));
    CHECK(!plan_full_fit(2, 0, one, given, iters, 1, 1 << 20, p, why) && has(why, "D 0"));
    CHECK(!plan_full_fit(2, 65, one, given, iters, 1, 1 << 20, p, why) && has(why, "D 65"));
    CHECK(!plan_full_fit(65536, 3, one, given, iters, 1, 1 << 20, p, why) && has(why, "65536 components"));
    CHECK(!plan_full_fit(2, 3, one, given, iters, 0, 1 << 20, p, why) && has(why, "S = 0"));
    CHECK(!plan_full_fit(2, 3, nullptr, given, iters, 1, 1 << 20, p, why));
    CHECK(!plan_full_fit(2, 3, one, given, iters, 1, 0, p, why) && has(why, "full_fit_batch_bytes must be >= 1"));
    CHECK(!plan_full_fit(2, 3, none, given, iters, 1, 1 << 20, p, why) && has(why, "speaker 0 has 0 frames"));
    CHECK(!plan_full_fit(2, 3, neg, given, iters, 2, 1 << 20, p, why) && has(why, "speaker 1 has -2 frames"));
    CHECK(!plan_full_fit(2, 3, huge, given, iters, 1, 1 << 20, p, why) && has(why, "speaker 0 has 68719476705 frames"));
    CHECK(p.groups.empty() && p.speakers.empty());          // a refused plan is empty
    // the largest K plans (one small speaker)
    CHECK(plan_full_fit(65535, 1, one, given, iters, 1, 1, p, why) && p.groups.size() == 1);
}

int main() {
    const int64_t edges[] = {31, 32, 33, 255, 256, 257, 8191, 8192, 8193, 16385};
    const int64_t bounds[] = {1, 4096, (int64_t)1 << 20, (int64_t)1 << 26, (int64_t)1 << 30, (int64_t)4 << 30};
    // every K and D: each edge alone (and n = K), at the default bound and at 1 byte
    for (int K = 1; K <= 65; K++)
        for (int D = 1; D <= 64; D++) {
            std::vector<int64_t> all(1, K);
            check_plan(K, D, all, (int64_t)1 << 30);
            for (int64_t n : edges) {
                check_plan(K, D, std::vector<int64_t>(1, n), (K + D) % 2 ? 1 : (int64_t)1 << 30);
                all.push_back(n);
            }
            if ((K * 64 + D) % 97 == 0) check_plan(K, D, all, (int64_t)1 << ((K + D) % 33));      // the edges together, some bound
        }
    // ragged sets: the edges and hashed lengths up to 20 000, S up to 300, every bound
    const int Ks[] = {1, 2, 32, 64, 65}, Ds[] = {1, 2, 28, 63, 64}, Ss[] = {1, 2, 3, 7, 40, 100, 300};
    for (int K : Ks)
        for (int D : Ds)
            for (int S : Ss) {
                std::vector<int64_t> len((size_t)S);
                for (int s = 0; s < S; s++) {
                    const uint64_t h = hash64((uint64_t)(K * 100 + D), (uint64_t)(S * 1000 + s));
                    len[(size_t)s] = h % 3 == 0 ? (s % 11 == 10 ? K : edges[s % 11]) : (int64_t)K + (int64_t)((h >> 8) % 20000);
                    if (len[(size_t)s] < K) len[(size_t)s] = K;
                }
                for (int64_t bound : bounds) check_plan(K, D, len, bound);
                // bounds that fall between speakers: a hashed multiple of the first speaker's bytes
                check_plan(K, D, len, closed_form_bytes(len[0], K, D) * (1 + (int64_t)(hash64(3, (uint64_t)S) % 9)));
                check_plan(K, D, len, closed_form_bytes(len[0], K, D) - 1);
            }
    // the documented set and its two recorded cuts
    {
        FullFitPlan p;
        std::string why;
        const std::vector<int64_t> len(100, 5600);
        const std::vector<int> given(100, 0), iters(100, 100);
        CHECK(plan_full_fit(32, 28, len.data(), given.data(), iters.data(), 100, (int64_t)1 << 30, p, why) && p.groups.size() == 1);
        CHECK(plan_full_fit(32, 28, len.data(), given.data(), iters.data(), 100, (int64_t)512 << 20, p, why) && p.groups.size() == 2 &&
              p.groups[0].count == 98 && p.groups[1].count == 2);
        check_plan(32, 28, len, (int64_t)512 << 20);
    }
    // the cap: 70 000 one-frame speakers under a bound that would hold them all
    {
        const std::vector<int64_t> len(70000, 1);
        check_plan(1, 1, len, (int64_t)4 << 30);
        FullFitPlan p;
        std::string why;
        const std::vector<int> given(70000, 0), iters(70000, 1);
        CHECK(plan_full_fit(1, 1, len.data(), given.data(), iters.data(), 70000, (int64_t)4 << 30, p, why) && p.groups.size() == 2 &&
              p.groups[0].count == 65535 && p.groups[1].count == 70000 - 65535);
    }
    check_refusals();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("full checks ok: %ld plans\n", plans);
    return 0;
}
