// jfa_checks.cpp -- csrc/jfa_plan.cpp under the host sanitizers (tests/test_jfa_cpu.py builds this with -fsanitize=address,undefined
// and runs it): every refusal's text, and the plan swept over group counts, shapes, ranks, bounds, the jfa_lds_rows option and
// device sizes.  Host code only: no GPU, nothing loaded into Python.
#include "jfa_plan.hpp"

#include <cmath>
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

static bool refused(int64_t G, int K, int D, int R, int64_t bound, int lds_rows, int n_cu, const char *needle) {
    JfaPlan p;
    std::string why;
    if (plan_jfa(G, K, D, R, bound, lds_rows, n_cu, p, why)) return false;
    if (why.find(needle) == std::string::npos) {
        std::printf("refusal text '%s' lacks '%s'\n", why.c_str(), needle);
        return false;
    }
    return true;
}

int main() {
    const int64_t GiB = (int64_t)1 << 30;
    // ---- refusals of the shape, the rank, the option, the bound
    CHECK(refused(0, 8, 5, 7, GiB, 0, 256, "G, K, D >= 1"));
    CHECK(refused(4, 0, 5, 7, GiB, 0, 256, "G, K, D >= 1"));
    CHECK(refused(4, 8, 0, 7, GiB, 0, 256, "G, K, D >= 1"));
    CHECK(refused(4, 8, 5, 0, GiB, 0, 256, "R >= 1"));
    CHECK(refused(4, 8, 5, JFA_MAX_R + 1, GiB, 0, 256, "train fewer factors"));
    CHECK(refused(4, 8, 5, 7, GiB, -1, 256, "jfa_lds_rows"));
    CHECK(refused(4, 8, 5, 7, GiB, JFA_LDS_MAX_R + 1, 256, "jfa_lds_rows"));
    CHECK(refused(4, 8, 5, 7, GiB, 0, 0, "compute units"));
    CHECK(refused(70, 5, 39, 65, 16 * 65 * 65 * 8 - 1, 0, 256, "jfa_scratch_mib"));
    CHECK(refused(4, 8, 5, 7, 4 * 49 * 8 - 1, 0, 256, "jfa_scratch_mib"));
    CHECK(refused((int64_t)1 << 31, 8, 5, 7, GiB, 0, 256, "split the corpus"));
    // ---- refusals of the statistics
    {
        const int G = 3, K = 2, D = 2;
        std::vector<double> N(G * K, 1.0), F(G * K * D, 0.5), E(K * D, 2.0);
        std::string why;
        CHECK(jfa_check_stats(G, K, D, N.data(), F.data(), E.data(), why));
        CHECK(!jfa_check_stats(G, K, D, nullptr, F.data(), E.data(), why) && why.find("null argument") != std::string::npos);
        N[3] = -1e-300;
        CHECK(!jfa_check_stats(G, K, D, N.data(), F.data(), E.data(), why) && why.find("negative occupancy at group 1, mixture 1") != std::string::npos);
        N[3] = std::numeric_limits<double>::quiet_NaN();
        CHECK(!jfa_check_stats(G, K, D, N.data(), F.data(), E.data(), why) && why.find("N holds a non-finite value at element 3") != std::string::npos);
        N[3] = 0.0;
        F[11] = std::numeric_limits<double>::infinity();
        CHECK(!jfa_check_stats(G, K, D, N.data(), F.data(), E.data(), why) && why.find("Fc holds a non-finite value at element 11") != std::string::npos);
        F[11] = 0.0;
        E[2] = 0.0;
        CHECK(!jfa_check_stats(G, K, D, N.data(), F.data(), E.data(), why) && why.find("E must be positive, element 2") != std::string::npos);
        E[2] = -std::numeric_limits<double>::infinity();
        CHECK(!jfa_check_stats(G, K, D, N.data(), F.data(), E.data(), why) && why.find("E holds a non-finite") != std::string::npos);
        E[2] = 1.0;
        CHECK(jfa_check_stats(G, K, D, N.data(), F.data(), E.data(), why));
        CHECK(jfa_check_finite(nullptr, 0, "W", why));
    }
    // ---- the plan, swept
    const int64_t Gs[] = {1, 2, 15, 16, 17, 33, 70, 200, 1000, 100000};
    const int Ks[] = {1, 5, 17, 512}, Ds[] = {1, 13, 39}, Rs[] = {1, 3, 16, 17, 65, 112, 113, 130, 300, 320, 512};
    const int lds[] = {0, 1, 17, 64, 112}, cus[] = {1, 64, 256};
    long plans = 0;
    for (int64_t G : Gs)
        for (int K : Ks)
            for (int D : Ds)
                for (int R : Rs) {
                    const int64_t block = (int64_t)R * R * 8;
                    const int64_t bounds[] = {block, 16 * block, 16 * block + 1, 33 * block, (int64_t)1 << 20, GiB, (int64_t)1 << 40};
                    for (int64_t bound : bounds)
                        for (int lr : lds)
                            for (int n_cu : cus) {
                                JfaPlan p;
                                std::string why;
                                const bool ok = plan_jfa(G, K, D, R, bound, lr, n_cu, p, why);
                                const int64_t fit = bound / block;
                                if (fit < G && fit < JFA_KSTEP) {
                                    CHECK(!ok && why.find("jfa_scratch_mib") != std::string::npos);
                                    continue;
                                }
                                CHECK(ok);
                                if (!ok) continue;
                                plans++;
                                CHECK(p.chunk >= 1 && p.chunk <= G && p.chunk * block <= bound && p.bytes_scratch == p.chunk * block);
                                CHECK(p.n_chunks == (G + p.chunk - 1) / p.chunk && (p.n_chunks - 1) * p.chunk < G);      // every group once
                                CHECK(p.n_chunks == 1 || p.chunk % JFA_KSTEP == 0);
                                CHECK(p.lds_rows == (lr == 0 ? JFA_LDS_MAX_R : lr) && p.path == (R <= p.lds_rows ? 0 : 1));
                                CHECK(p.factor_lds == jfa_factor_lds_bytes(R, p.path) && p.factor_lds <= 160 * 1024 && p.update_lds == p.factor_lds);
                                CHECK(p.gemm_lds <= 64 * 1024 && p.gram_lds <= 64 * 1024);
                                CHECK(p.gemm_L.x * JFA_TILE >= (int64_t)R * R && p.gemm_L.y * JFA_TILE >= p.chunk && p.gemm_L.y <= 65535);
                                CHECK(p.gemm_b.x * JFA_TILE >= R && p.gemm_A.y * JFA_TILE >= K && p.gemm_C.x * JFA_TILE >= (int64_t)K * D);
                                CHECK(p.gram.x == K && p.gram.y * JFA_GRAM_TILE * JFA_GRAM_TILE >= (int64_t)R * R && p.gram.y <= 65535);
                                CHECK(p.bytes_N == G * K * 8 && p.bytes_Fc == G * K * D * 8 && p.bytes_P == (int64_t)K * block && p.bytes_A == p.bytes_P);
                                CHECK(p.factor_rounds == (p.chunk + n_cu - 1) / n_cu);
                            }
                }
    // R = 320 is accepted on the global-memory path, 512 is the built limit
    {
        JfaPlan p;
        std::string why;
        CHECK(plan_jfa(1000, 512, 39, 320, GiB, 0, 256, p, why) && p.path == 1 && p.chunk == 1000 && p.n_chunks == 1);
        CHECK(plan_jfa(2000, 512, 39, 320, GiB, 0, 256, p, why) && p.chunk == 1296 && p.n_chunks == 2);      // 1310 blocks fit: 81 x 16
        CHECK(plan_jfa(70, 5, 39, 65, (int64_t)1 << 20, 0, 256, p, why) && p.chunk == 16 && p.n_chunks == 5 && p.path == 0);
        CHECK(plan_jfa(70, 5, 39, 65, (int64_t)1 << 20, 1, 256, p, why) && p.path == 1);
    }
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("jfa checks ok (%ld plans)\n", plans);
    return 0;
}
