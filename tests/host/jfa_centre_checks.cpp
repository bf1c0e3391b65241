// jfa_centre_checks.cpp -- the centring plan of csrc/jfa_plan.cpp (plan_jfa_centre and the refusals in front of it) under the host
// sanitizers (tests/test_jfa_resident_cpu.py builds this with -fsanitize=address,undefined and runs it): swept over sessions,
// labels, K, D, ranks, modes and bounds.  Host code only: no GPU, nothing loaded into Python.
#include "jfa_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

using namespace sr;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            failures++;                                                      \
        }                                                                    \
    } while (0)

static bool refused(int64_t n, int64_t n_labels, int K, int D, int Ry, int Ru, int mode, int64_t bound, const char *needle) {
    JfaCentrePlan p;
    std::string why;
    if (plan_jfa_centre(n, n_labels, K, D, Ry, Ru, mode, bound, p, why)) return false;
    if (why.find(needle) == std::string::npos || why.find("HIP") != std::string::npos) {
        std::printf("refusal text '%s' lacks '%s'\n", why.c_str(), needle);
        return false;
    }
    return true;
}

int main() {
    const int64_t GiB = (int64_t)1 << 30;
    CHECK(refused(0, 3, 5, 13, 0, 0, 0, GiB, "G, K, D >= 1"));
    CHECK(refused(4, 3, 0, 13, 0, 0, 0, GiB, "G, K, D >= 1"));
    CHECK(refused(4, 0, 5, 13, 0, 0, 0, GiB, "n_labels"));
    CHECK(refused(4, 3, 5, 13, 0, 0, 2, GiB, "the mode is 0"));
    CHECK(refused(4, 3, 5, 13, -1, 0, 0, GiB, "Ry is -1"));
    CHECK(refused(4, 3, 5, 13, JFA_MAX_R + 1, 0, 0, GiB, "Ry is 513"));
    CHECK(refused(4, 3, 5, 13, 0, JFA_MAX_R + 1, 1, GiB, "Ru is 513"));
    CHECK(refused(4, 3, 5, 13, 0, -7, 1, GiB, "Ru is -7"));
    CHECK(refused(210, 70, 17, 39, 0, 5, 0, 64 * 17 * 39 * 8 - 1, "raise the option jfa_scratch_mib"));
    CHECK(refused(3, 3, 17, 39, 0, 5, 1, 3 * 17 * 39 * 8 - 1, "raise the option jfa_scratch_mib"));
    CHECK(refused((int64_t)1 << 31, 3, 5, 13, 0, 0, 0, GiB, "split the corpus"));
    {
        std::string why;
        const int64_t ids[4] = {0, 2, 1, 2}, neg[4] = {0, -1, 1, 2};
        CHECK(jfa_centre_check_labels(ids, 4, 3, why));
        CHECK(!jfa_centre_check_labels(ids, 4, 2, why) && why.find("ids[1] is 2, outside 0 .. n_labels - 1 = 1") != std::string::npos);
        CHECK(!jfa_centre_check_labels(neg, 4, 3, why) && why.find("ids[1] is -1") != std::string::npos);
        CHECK(!jfa_centre_check_labels(nullptr, 4, 3, why) && why.find("null argument") != std::string::npos);
        std::vector<double> N(6, 1.0), F(12, 0.5);
        CHECK(jfa_check_raw_stats(3, 2, 2, N.data(), F.data(), why));
        F[7] = std::numeric_limits<double>::infinity();
        CHECK(!jfa_check_raw_stats(3, 2, 2, N.data(), F.data(), why) && why.find("F holds a non-finite value at element 7") != std::string::npos);
        N[5] = -0.5;
        CHECK(!jfa_check_raw_stats(3, 2, 2, N.data(), F.data(), why) && why.find("F holds") != std::string::npos);       // finiteness first
        F[7] = 0.0;
        CHECK(!jfa_check_raw_stats(3, 2, 2, N.data(), F.data(), why) && why.find("negative occupancy at group 2, mixture 1") != std::string::npos);
        CHECK(!jfa_check_raw_stats(3, 2, 2, nullptr, F.data(), why) && why.find("null argument") != std::string::npos);
    }
    long plans = 0;
    const int64_t ns[] = {1, 2, 63, 64, 65, 210, 1000, 4097};
    const int shapes[][2] = {{1, 1}, {3, 3}, {5, 39}, {17, 13}, {17, 39}, {512, 39}};
    const int ranks[] = {0, 1, 16, 65, 512};
    for (int64_t n : ns)
        for (auto &kd2 : shapes)
            for (int Ru : ranks)
                for (int mode = 0; mode < 2; mode++) {
                    const int K = kd2[0], D = kd2[1];
                    const int64_t kd = (int64_t)K * D, row = kd * 8;
                    const int64_t bounds[] = {std::min<int64_t>(n, 64) * row, 64 * row + 1, 200 * row, (int64_t)1 << 20, GiB};
                    for (int64_t bound : bounds) {
                        if (Ru > 0 && bound / row < std::min<int64_t>(n, 64)) continue;
                        int64_t first_chunk = -1;
                        for (int64_t labels : {(int64_t)1, n, 3 * n}) {
                            for (int Ry : {0, 17}) {
                                JfaCentrePlan p;
                                std::string why;
                                CHECK(plan_jfa_centre(n, labels, K, D, Ry, Ru, mode, bound, p, why));
                                plans++;
                                // every session in exactly one chunk; the scratch under the bound
                                CHECK(p.chunk >= 1 && p.chunk <= n && p.n_chunks == (n + p.chunk - 1) / p.chunk);
                                CHECK((p.n_chunks - 1) * p.chunk < n && n <= p.n_chunks * p.chunk);
                                CHECK(p.bytes_scratch == (Ru > 0 ? p.chunk * row : 0) && p.bytes_scratch <= bound);
                                CHECK(Ru > 0 || p.n_chunks == 1);
                                CHECK(p.n_chunks == 1 || p.chunk % JFA_TILE == 0);
                                // chunk boundaries: a function of n, K D and the bound only
                                if (first_chunk < 0) first_chunk = p.chunk;
                                CHECK(p.chunk == first_chunk);
                                CHECK(p.vec == (kd % 2 == 0 ? 2 : 1));
                                CHECK(p.centre.y * JFA_WG * p.vec >= kd && (p.centre.y - 1) * JFA_WG * p.vec < kd);
                                CHECK(p.bytes_Fc == (mode == 1 ? n : std::min(n, labels)) * row);
                                CHECK((Ru > 0) == (p.gemm_xu.x > 0) && (Ry > 0) == (p.gemm_yv.x > 0));
                            }
                        }
                    }
                }
    std::printf("%ld plans\n", plans);
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("jfa centre checks ok\n");
    return 0;
}
