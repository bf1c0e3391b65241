// timeline_checks.cpp -- csrc/timeline_plan.cpp swept over column counts, minimum durations, lengths, windows and hops, with its
// refusals; a stand-alone program for the host sanitizers (tests/test_timeline_cpu.py builds it with -fsanitize=address,undefined).
#include "timeline_plan.hpp"

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

// the window count by walking the windows
static int64_t count_windows(int64_t n, int64_t W, int64_t H) {
    if (n <= 0) return 0;
    int64_t j = 0;
    while (j * H + W < n && (j + 1) * H < n) j++;
    return j + 1;
}

int main() {
    std::string why;
    TimelinePlan p;
    long plans = 0;
    for (int64_t W : {1, 2, 5, 8, 10, 150, 300})
        for (int64_t H : {1, 2, 5, 7, 8, 10, 40, 301})
            for (int64_t n : {(int64_t)0, (int64_t)1, W - 1, W, W + 1, W + H, W + H + 1, (int64_t)240, (int64_t)3000}) {
                CHECK(timeline_windows(n, W, H) == count_windows(n, W, H));
                const int64_t nw = timeline_windows(n, W, H);
                if (nw > 0) CHECK((nw - 1) * H < n && ((nw - 1) * H + W >= n || nw * H >= n));   // the last window starts inside; the next would not, or is not needed
            }
    CHECK(timeline_windows(5, 0, 1) == 0 && timeline_windows(5, 1, 0) == 0 && timeline_windows(-3, 1, 1) == 0);
    CHECK(timeline_windows(std::numeric_limits<int64_t>::max(), 1, 1) == std::numeric_limits<int64_t>::max());
    for (int S : {1, 2, 63, 64, 65, 201, 1024, 1025, 4095, 4096})
        for (int m = 1; m <= TIMELINE_MAX_M; m++)
            for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)149, (int64_t)150, (int64_t)151, (int64_t)360000, (int64_t)1 << 40}) {
                CHECK(plan_timeline(S, m, n, 150, 40, p, why));
                plans++;
                CHECK(p.windows == timeline_windows(n, 150, 40));
                CHECK(p.variant == (S <= 64 ? 0 : S <= 1024 ? 1 : 2));
                CHECK(p.lanes % 64 == 0 && p.lanes >= 64 && p.lanes <= 1024);
                CHECK(p.s_pad == p.lanes * p.states_per_lane && p.s_pad >= S);
                CHECK(p.words == (S + 63) / 64 && p.bp_bytes_per_window == 8 * p.words + 4);
                CHECK(p.chain_slots == (m > 2 ? m - 1 : 0));
                CHECK(p.chain_lds == (p.chain_slots > 0 && (int64_t)p.chain_slots * p.s_pad * 8 <= TIMELINE_CHAIN_LDS_BYTES));
                CHECK(p.fwd_lds_bytes == 384 + (p.chain_lds ? p.chain_slots * p.s_pad * 8 : 0) && p.fwd_lds_bytes <= 65536);
                CHECK(p.tile == (p.variant == 2 ? TIMELINE_TILE_LOOP : TIMELINE_TILE));
                CHECK(p.sum_span == 3 * 40 + 150 && p.sum_grid_x == (p.windows + 3) / 4 && p.sum_grid_y == (S + 63) / 64);
                // what the forward kernel indexes: a state's chain slot, a window's stay words
                std::vector<char> touched((size_t)p.chain_slots * p.s_pad, 0);
                for (int k = 0; k < p.chain_slots; k++)
                    for (int s = 0; s < S; s += (S > 64 ? 61 : 1)) touched.at((size_t)k * p.s_pad + s) = 1;
            }
    // the sum saturates instead of overflowing
    CHECK(plan_timeline(4, 1, 10, std::numeric_limits<int64_t>::max(), std::numeric_limits<int64_t>::max(), p, why) && p.sum_span > 0);
    // refusals
    CHECK(!plan_timeline(0, 1, 10, 5, 5, p, why) && !why.empty());
    CHECK(!plan_timeline(4097, 1, 10, 5, 5, p, why));
    CHECK(!plan_timeline(4, 0, 10, 5, 5, p, why));
    CHECK(!plan_timeline(4, 17, 10, 5, 5, p, why));
    CHECK(!plan_timeline(4, 1, -1, 5, 5, p, why));
    CHECK(!plan_timeline(4, 1, 10, 0, 5, p, why));
    CHECK(!plan_timeline(4, 1, 10, 5, 0, p, why));
    const double nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(timeline_check(4, -1, 0.0, 0, 0.0, 1, why) && timeline_check(4, 3, -1e300, 2, 1e300, 16, why));
    CHECK(!timeline_check(4, 4, 0.0, 0, 0.0, 1, why) && !timeline_check(4, -2, 0.0, 0, 0.0, 1, why));
    CHECK(!timeline_check(4, 0, nan, 0, 0.0, 1, why));
    CHECK(!timeline_check(4, 0, 0.0, 3, 0.0, 1, why) && !timeline_check(4, 0, 0.0, -1, 0.0, 1, why));
    CHECK(!timeline_check(4, 0, 0.0, 2, nan, 1, why) && !timeline_check(4, 0, 0.0, 2, -0.5, 1, why));
    CHECK(!timeline_check(4, 0, 0.0, 2, 1.0, 0, why) && !timeline_check(4, 0, 0.0, 2, 1.0, 17, why));
    CHECK(!timeline_check(4097, 0, 0.0, 0, 0.0, 1, why) && !timeline_check(0, -1, 0.0, 0, 0.0, 1, why));
    std::printf("timeline checks ok: %ld plans\n", plans);
    return 0;
}
