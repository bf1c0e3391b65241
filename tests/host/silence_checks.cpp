// silence_checks.cpp -- csrc/silence_plan.cpp (the launch decisions of the silence removal) under the host sanitizers: a
// stand-alone program, built by tests/test_silence_cpu.py with g++ -fsanitize=address,undefined.  It sweeps the plan over rates,
// frame shapes, utterance lengths and block options and checks the invariants the kernels rely on.
#include "silence_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <numeric>

using namespace sr;

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                             \
        }                                                                           \
    } while (0)

static void check_plan(double fs, double fd, double fsh, int64_t n, int64_t block) {
    SilencePlan p;
    std::string why;
    if (!plan_silence(fs, fd, fsh, n, block, p, why)) {
        CHECK(!why.empty());
        return;
    }
    CHECK(p.L == (int64_t)(fd * fs) && p.S == (int64_t)(fsh * fs) && p.L >= 1 && p.S >= 1);
    CHECK(p.g == std::gcd(p.L, p.S) && p.Lg * p.g == p.L && p.Sg * p.g == p.S);
    CHECK(p.K == (p.L < p.S ? p.L : p.S));
    CHECK((p.max_pos - 1) * p.g < n && p.max_pos * p.g >= n);
    CHECK(p.E >= 1 && p.E <= p.max_pos && p.E <= (p.Lg > p.Sg ? p.Lg : p.Sg) && p.E <= SILENCE_MAX_REL);
    CHECK(p.B >= 1 && p.B <= SILENCE_MAX_REL && (block == 0 || p.B == block));
    if (block == 0 && p.B < SILENCE_MAX_REL) {
        const int64_t for_chain = (p.max_pos + SILENCE_CHAIN_MAX - 1) / SILENCE_CHAIN_MAX;
        CHECK(p.B == std::max<int64_t>({256, 4 * p.E, for_chain}) && p.blocks_max <= SILENCE_CHAIN_MAX);
    }
    CHECK((p.blocks_max - 1) * p.B < p.max_pos && p.blocks_max * p.B >= p.max_pos);
    CHECK(p.variant == (p.E > SILENCE_WG));
    CHECK(p.blocks_per_wg >= 1 && (p.variant ? p.blocks_per_wg == 1 : p.blocks_per_wg * p.E <= SILENCE_WG));
    CHECK((p.list_cap - 1) * p.Sg < p.B && p.list_cap * p.Sg >= p.B);         // kept frames lie Sg apart inside B positions
    CHECK(p.chunk_lanes == 1 || p.chunk_lanes == 64);
    const int grid = silence_grid(p.blocks_max, p.blocks_per_wg);
    CHECK(grid >= 1 && grid <= (1 << 20));
}

int main() {
    const double rates[] = {1000, 8000, 11025, 16000, 22050, 44100, 48000, 96000};
    const double shapes[][2] = {{0.02, 0.01}, {0.025, 0.010}, {0.01, 0.02}, {1.0, 0.007}, {0.0301, 0.0007}, {3.0, 0.5}, {1e-9, 0.01},
                                {0.02, 0.0}, {0.02, -1.0}, {1e30, 0.01}};
    const int64_t lens[] = {0, 1, 2, 79, 80, 81, 159, 160, 161, 20011, 480000, (int64_t)3600 * 16000, (int64_t)1 << 33};
    const int64_t blocks[] = {0, 1, 8, 255, 256, 257, 100000, (int64_t)1 << 30, ((int64_t)1 << 30) + 1, -1};
    for (double fs : rates)
        for (auto &sh : shapes)
            for (int64_t n : lens)
                for (int64_t b : blocks) check_plan(fs, sh[0], sh[1], n, b);
    // the defaults at the rates of the reference's corpora
    struct { double fs; int64_t L, S, g, E; } want[] = {{8000, 160, 80, 80, 2}, {11025, 220, 110, 110, 2}, {16000, 320, 160, 160, 2},
                                                         {22050, 441, 220, 1, 441}, {44100, 882, 441, 441, 2}};
    for (auto &w : want) {
        SilencePlan p;
        std::string why;
        CHECK(plan_silence(w.fs, 0.02, 0.01, 480000, 0, p, why));
        CHECK(p.L == w.L && p.S == w.S && p.g == w.g && p.E == w.E && p.B == (4 * w.E > 256 ? 4 * w.E : 256));
    }
    SilencePlan p;
    std::string why;
    CHECK(!plan_silence(16000, 0.02, 0.00001, 1000, 0, p, why) && why.find("frame_shift") != std::string::npos);
    CHECK(!plan_silence(16000, 0.0, 0.01, 1000, 0, p, why) && why.find("frame_duration") != std::string::npos);
    CHECK(!plan_silence(16000, 0.02, 0.01, 0, 0, p, why));
    CHECK(!plan_silence(std::nan(""), 0.02, 0.01, 1000, 0, p, why));
    if (failures) return 1;
    std::printf("silence checks ok\n");
    return 0;
}
