// topc_checks.cpp -- csrc/topc_plan.cpp (the refusals and the launch decisions of top-C scoring) under the host sanitizers: a
// stand-alone program, built by tests/test_topc_cpu.py with g++ -fsanitize=address,undefined.  It sweeps the plan over set shapes,
// batch lengths, bounds and device sizes and checks the invariants the kernels rely on, and every refusal's text.
#include "topc_plan.hpp"

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

static void check_plan(int K, int D, int S, int C, int64_t n, int64_t bound, int n_cu) {
    TopcPlan p;
    std::string why;
    if (!plan_topc(K, D, S, C, n, bound, n_cu, p, why)) {
        CHECK(!why.empty());
        return;
    }
    CHECK(p.tp >= D && (p.tp == 16 || p.tp == 40 || p.tp == 64) && p.tp % 4 == 0);
    CHECK(p.cr == 0 ? C > TOPC_MAX_REG_C : (p.cr >= C && p.cr <= TOPC_MAX_REG_C));
    CHECK(p.row_bytes >= (int64_t)C * S * 4 && p.row_bytes <= bound);
    CHECK(p.eval_waves >= 1 && p.eval_waves <= 4 && (int64_t)p.eval_grid_y * 64 * p.eval_waves >= S &&
          (int64_t)(p.eval_grid_y - 1) * 64 * p.eval_waves < S);
    CHECK(p.combine_wg >= 64 && p.combine_wg <= 256 && p.combine_wg % 64 == 0);
    CHECK(p.rank_lds == (p.cr == 0 ? K * 4 : 0) && p.rank_lds <= 32768);
    if (n == 0) {
        CHECK(p.chunk == 0 && p.n_chunks == 0);
        return;
    }
    CHECK(p.chunk >= 1 && p.chunk <= n && p.chunk * p.row_bytes <= bound);
    CHECK((p.n_chunks - 1) * p.chunk < n && p.n_chunks * p.chunk >= n);          // every frame in exactly one chunk
    CHECK(p.chunk * C + TOPC_WG < ((int64_t)1 << 31));                           // pairs and launch dimensions are int32
    CHECK(p.run == 256 || p.run == TOPC_STAGE);
    CHECK(p.eval_grid_x >= (p.chunk * C + p.run - 1) / p.run + K && p.eval_grid_x < ((int64_t)1 << 31));
    CHECK(p.select_grid * TOPC_WG >= p.chunk && (p.select_grid - 1) * TOPC_WG < p.chunk);
    CHECK(p.route_grid * TOPC_WG >= p.chunk * C && (p.route_grid - 1) * TOPC_WG < p.chunk * C);
}

int main() {
    const int Ks[] = {1, 5, 33, 64, 512, 2048, 8192, 8193};
    const int Ds[] = {1, 13, 16, 17, 39, 40, 41, 64, 65};
    const int Ss[] = {1, 2, 64, 65, 201, 256, 257, 1001};
    const int Cs[] = {0, 1, 3, 5, 6, 8, 9, 64, 512};
    const int64_t ns[] = {0, 1, 63, 64, 65, 1000, 19200, 1000000, (int64_t)12500000, (int64_t)1 << 33, -1};
    const int64_t bounds[] = {0, 3, 100, 4096, (int64_t)1 << 20, (int64_t)1 << 30, (int64_t)1 << 40};
    const int cus[] = {0, 1, 256};
    for (int K : Ks)
        for (int D : Ds)
            for (int S : Ss)
                for (int C : Cs)
                    for (int64_t n : ns)
                        for (int64_t b : bounds)
                            for (int cu : cus) check_plan(K, D, S, C, n, b, cu);
    TopcPlan p;
    std::string why;
    // the headline shape under the default bound: 1 GiB / (5 x 201 x 4 + 44) frames per chunk
    CHECK(plan_topc(512, 39, 201, 5, 10000000, TOPC_DEFAULT_SCRATCH, 256, p, why));
    CHECK(p.tp == 40 && p.cr == 5 && p.row_bytes == 5 * 201 * 4 + 44 && p.chunk == TOPC_DEFAULT_SCRATCH / p.row_bytes && p.eval_waves == 4 &&
          p.eval_grid_y == 1 && p.run == 256);
    // a bound below one frame's row is refused, one row is enough
    CHECK(!plan_topc(512, 39, 201, 5, 1000, 5 * 201 * 4 + 43, 256, p, why) && has(why, "topc_scratch_mib"));
    CHECK(plan_topc(512, 39, 201, 5, 1000, 5 * 201 * 4 + 44, 256, p, why) && p.chunk == 1 && p.n_chunks == 1000);
    // the refusals, each with its remedy
    CHECK(!topc_check(false, 3, 8, 13, 0, 2, true, why) && has(why, "share sigma and weights") && has(why, "sr_score_batch_set"));
    CHECK(!topc_check(true, 3, 8, 13, -1, 2, true, why) && has(why, "background column -1 outside [0, 3)"));
    CHECK(!topc_check(true, 3, 8, 13, 3, 2, true, why) && has(why, "background column 3 outside [0, 3)"));
    CHECK(!topc_check(true, 3, 8, 13, 0, 0, true, why) && has(why, "top_c 0 outside [1, 8]"));
    CHECK(!topc_check(true, 3, 8, 13, 0, 9, true, why) && has(why, "top_c 9 outside [1, 8]"));
    CHECK(!topc_check(true, 3, 8, 13, 0, 2, false, why) && has(why, "feature batch") && has(why, "sr_predict_pcm_batch_topc"));
    CHECK(!topc_check(true, 3, 8, 65, 0, 2, true, why) && has(why, "64 dimensions"));
    CHECK(!topc_check(true, 3, 8193, 13, 0, 9, true, why) && has(why, "8192"));
    CHECK(topc_check(true, 1, 8, 13, 0, 8, true, why));
    if (failures) return 1;
    std::printf("topc checks ok\n");
    return 0;
}
