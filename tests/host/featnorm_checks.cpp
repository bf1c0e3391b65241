// featnorm_checks.cpp -- csrc/featnorm_plan.cpp (the launch decisions of the short-time feature normalisation) under the host
// sanitizers: a stand-alone program, built by tests/test_featnorm_cpu.py with g++ -fsanitize=address,undefined.  It sweeps the plan
// over modes, windows, widths, utterance lengths and tile options, checks the invariants the kernel relies on, and walks the tiles
// of an utterance the way the kernel does: every staged row range must fit the column stride the plan sized.
#include "featnorm_plan.hpp"

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

static void check_plan(int mode, int W, int dim, int64_t T, long tile, int n_cu) {
    FeatNormPlan p;
    std::string why;
    const bool ok = plan_feature_norm(mode, W, true, dim, T, tile, n_cu, p, why);
    const bool want = mode >= 0 && mode <= 2 && W >= 2 && W <= 1024 && dim >= 1 && T >= 0 && tile >= 0 && tile <= 1024 && tile % 64 == 0 && n_cu >= 1;
    CHECK(ok == want);
    if (!ok) {
        CHECK(!why.empty());
        return;
    }
    CHECK(p.F == (tile ? tile : FEATNORM_AUTO_TILE) && p.F % FEATNORM_WAVE == 0);
    const int64_t N = std::min<int64_t>(W, T);
    CHECK(p.span_max >= 1 && p.span_max <= p.F + W - 1 && (T == 0 || p.span_max <= T));
    CHECK(p.stride >= p.span_max && p.stride < p.span_max + 8 && p.stride % 8 == 4);
    CHECK(p.cols >= 1 && p.cols <= FEATNORM_MAX_COLS && p.cols <= dim && p.passes >= 1);
    CHECK((int64_t)p.passes * p.cols >= dim && (int64_t)(p.passes - 1) * p.cols < dim);
    CHECK(p.lds_bytes == p.cols * p.stride * 4 && p.lds_bytes <= FEATNORM_LDS_FLOATS * 4);
    CHECK(p.tiles_max == (T + p.F - 1) / p.F);
    CHECK(p.table == (mode == FEATNORM_WARP && T >= W && (double)T * dim >= 4.0 * (2 * W - 1)));
    CHECK(p.table_len == (p.table ? 2 * W - 1 : 0));
    const int grid = featnorm_grid(p.tiles_max, n_cu);
    CHECK(grid >= 1 && grid <= std::max<int64_t>(1, std::min<int64_t>(p.tiles_max, (int64_t)n_cu * FEATNORM_WGS_PER_CU)));
    if (T > 100000) return;
    // the kernel's view of every tile (and of a shorter utterance in the same batch: T2 <= T)
    for (int64_t T2 : {T, T / 2, std::min<int64_t>(T, W - 1), std::min<int64_t>(T, 1)}) {
        if (T2 < 1) continue;
        const int64_t N2 = std::min<int64_t>(W, T2);
        int64_t prev = -1;
        for (int64_t f0 = 0; f0 < T2; f0 += p.F) {
            const int64_t Fc = std::min<int64_t>(p.F, T2 - f0);
            const int64_t b = featnorm_window_start(f0, T2, W), e = featnorm_window_start(f0 + Fc - 1, T2, W) + N2;
            CHECK(b >= 0 && e <= T2 && e - b <= p.stride && e - b <= p.span_max);
            CHECK((e - b + 3) / 4 * 4 <= p.stride);                      // the walk reads whole groups of four
            for (int64_t t = f0; t < f0 + Fc; t++) {
                const int64_t s = featnorm_window_start(t, T2, W);
                CHECK(s >= b && s + N2 <= e && s <= t && t < s + N2 && s >= prev);      // the frame lies in its window; starts never step back
                prev = s;
            }
        }
    }
    (void)N;
}

int main() {
    const int windows[] = {-1, 0, 1, 2, 3, 8, 63, 64, 65, 300, 301, 1023, 1024, 1025};
    const int dims[] = {0, 1, 13, 39, 64, 65, 200};
    const int64_t lens[] = {-1, 0, 1, 2, 63, 64, 65, 255, 256, 257, 300, 301, 302, 1000, 2051, 3333, 10000000, (int64_t)1 << 40};
    const long tiles[] = {-64, -1, 0, 1, 63, 64, 128, 192, 1024, 1088};
    for (int mode = -1; mode <= 3; mode++)
        for (int W : windows)
            for (int dim : dims)
                for (int64_t T : lens)
                    for (long tile : tiles) check_plan(mode, W, dim, T, tile, 256);
    check_plan(0, 301, 39, 5000, 0, 0);
    check_plan(0, 301, 39, 5000, 0, 1);
    FeatNormPlan p;
    std::string why;
    CHECK(!plan_feature_norm(0, 301, false, 39, 100, 0, 256, p, why) && why.find("PCM") != std::string::npos);
    CHECK(!plan_feature_norm(3, 301, true, 39, 100, 0, 256, p, why) && why.find("mode") != std::string::npos);
    CHECK(!plan_feature_norm(0, 1, true, 39, 100, 0, 256, p, why) && why.find("window") != std::string::npos);
    CHECK(!plan_feature_norm(0, 1025, true, 39, 100, 0, 256, p, why) && why.find("window") != std::string::npos);
    CHECK(!plan_feature_norm(0, 301, true, 0, 100, 0, 256, p, why) && why.find("dim") != std::string::npos);
    CHECK(!plan_feature_norm(0, 301, true, 39, 100, -1, 256, p, why) && why.find("norm_tile") != std::string::npos);
    // the headline shape: 39 columns, 301 frames, automatic tile -- two even passes, three workgroups' worth of LDS per CU
    CHECK(plan_feature_norm(0, 301, true, 39, 10000, 0, 256, p, why));
    CHECK(p.F == 256 && p.span_max == 556 && p.stride == 556 && p.passes == 2 && p.cols == 20 && p.lds_bytes == 44480 && p.table && p.table_len == 601);
    if (failures) return 1;
    std::printf("featnorm checks ok\n");
    return 0;
}
