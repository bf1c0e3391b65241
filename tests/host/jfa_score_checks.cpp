// jfa_score_checks.cpp -- the trial-scoring decisions of csrc/jfa_plan.cpp under the host sanitizers (tests/test_jfa_score_cpu.py
// builds this with -fsanitize=address,undefined and runs it): every refusal's text, and plan_jfa_score swept over segment and model
// counts, shapes, ranks, both modes, bounds, the jfa_lds_rows option and device sizes.  Host code only: no GPU, nothing loaded into
// Python.
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

static bool has(const std::string &why, const char *needle) {
    if (why.find(needle) != std::string::npos) return true;
    std::printf("refusal text '%s' lacks '%s'\n", why.c_str(), needle);
    return false;
}

static bool refused(int64_t T, int64_t J, int K, int D, int Ry, int Ru, int mode, int64_t bound, int lds_rows, int n_cu, const char *needle) {
    JfaScorePlan p;
    std::string why;
    if (plan_jfa_score(T, J, K, D, Ry, Ru, mode, bound, lds_rows, n_cu, p, why)) return false;
    return has(why, needle);
}

struct Inputs {
    int64_t T = 3, J = 2;
    int K = 2, D = 2, Ry = 2, Ru = 3;
    std::vector<double> N, F, m, E, d, v, u, z, y, x;
    std::vector<unsigned char> mask;
    Inputs()
        : N(T * K, 1.0), F(T * K * D, 0.5), m(K * D, 0.1), E(K * D, 2.0), d(K * D, 0.2), v(Ry * K * D, 0.3), u(Ru * K * D, 0.4), z(J * K * D, 0.1),
          y(J * Ry, 1.0), x(T * Ru, 0.5), mask(J * T, 1) {}
    bool check(int mode, std::string &why, bool with_x = true, bool with_mask = true, int64_t mr = -1, int64_t mc = -1, bool with_dz = true) const {
        return jfa_score_check_inputs(T, J, K, D, Ry, Ru, mode, N.data(), F.data(), m.data(), E.data(), with_dz ? d.data() : nullptr, v.data(), u.data(),
                                      with_dz ? z.data() : nullptr, y.data(), with_x ? x.data() : nullptr, with_mask ? mask.data() : nullptr,
                                      mr < 0 ? J : mr, mc < 0 ? T : mc, why);
    }
};

int main() {
    const int64_t GiB = (int64_t)1 << 30;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // ---- refusals of the shape, the ranks, the mode, the option, the bound
    for (int mode = 0; mode < 2; mode++) {
        CHECK(refused(0, 2, 4, 5, 3, 2, mode, GiB, 0, 256, "T, J, K, D, Ry, Ru >= 1"));
        CHECK(refused(3, 0, 4, 5, 3, 2, mode, GiB, 0, 256, "T, J, K, D, Ry, Ru >= 1"));
        CHECK(refused(3, 2, 0, 5, 3, 2, mode, GiB, 0, 256, "T, J, K, D, Ry, Ru >= 1"));
        CHECK(refused(3, 2, 4, 0, 3, 2, mode, GiB, 0, 256, "T, J, K, D, Ry, Ru >= 1"));
        CHECK(refused(3, 2, 4, 5, 0, 2, mode, GiB, 0, 256, "T, J, K, D, Ry, Ru >= 1"));
        CHECK(refused(3, 2, 4, 5, 3, 0, mode, GiB, 0, 256, "T, J, K, D, Ry, Ru >= 1"));
        CHECK(refused(3, 2, 4, 5, JFA_MAX_R + 1, 2, mode, GiB, 0, 256, "score with fewer factors"));
        CHECK(refused(3, 2, 4, 5, 3, JFA_MAX_R + 1, mode, GiB, 0, 256, "score with fewer factors"));
        CHECK(refused(3, 2, 4, 5, 3, 2, mode, GiB, -1, 256, "jfa_lds_rows"));
        CHECK(refused(3, 2, 4, 5, 3, 2, mode, GiB, JFA_LDS_MAX_R + 1, 256, "jfa_lds_rows"));
        CHECK(refused(3, 2, 4, 5, 3, 2, mode, GiB, 0, 0, "compute units"));
        CHECK(refused((int64_t)1 << 31, 2, 4, 5, 3, 2, mode, GiB, 0, 256, "split the trial list"));
        CHECK(refused(3, JFA_SCORE_MAX_J + 1, 4, 5, 3, 2, mode, GiB, 0, 256, "split the trial list"));
        CHECK(refused(100000, 2, 65536, 64, 3, 2, mode, GiB, 0, 256, "split the trial list"));
    }
    CHECK(refused(3, 2, 4, 5, 3, 2, 2, GiB, 0, 256, "the mode is 0 (integrated) or 1 (linear)"));
    CHECK(refused(3, 2, 4, 5, 3, 2, 0, (2 * 2 + 3 * 2) * 8 - 1, 0, 256, "jfa_scratch_mib"));       // one segment: Ru^2 + (J + 1) Ru doubles
    {
        JfaScorePlan p;
        std::string why;
        CHECK(plan_jfa_score(3, 2, 4, 5, 3, 2, 0, (2 * 2 + 3 * 2) * 8, 0, 256, p, why) && p.chunk == 1 && p.n_chunks == 3);
        CHECK(plan_jfa_score(3, 2, 4, 5, 3, 2, 1, 1, 0, 256, p, why) && p.chunk == 3 && p.n_chunks == 1 && p.bytes_scratch == 0);      // linear: no bound
    }
    // ---- refusals of the arrays
    {
        Inputs in;
        std::string why;
        CHECK(in.check(0, why) && in.check(1, why) && in.check(0, why, false, false) && in.check(0, why, false, false, 0, 0, false));
        CHECK(!in.check(1, why, false) && has(why, "linear mode needs the test segments' channel factors x"));
        CHECK(!in.check(0, why, true, true, in.T, in.J) && has(why, "the mask is [3][2], the score matrix [2][3]"));
        CHECK(!jfa_score_check_inputs(in.T, in.J, in.K, in.D, in.Ry, in.Ru, 0, nullptr, in.F.data(), in.m.data(), in.E.data(), nullptr, in.v.data(),
                                      in.u.data(), nullptr, in.y.data(), nullptr, nullptr, 0, 0, why) &&
              has(why, "null argument"));
        struct {
            std::vector<double> *a;
            const char *name;
        } arrays[] = {{&in.N, "N"}, {&in.F, "F"}, {&in.m, "m"}, {&in.E, "E"}, {&in.d, "d"}, {&in.v, "v"}, {&in.u, "u"}, {&in.z, "z"}, {&in.y, "y"}, {&in.x, "x"}};
        for (auto &ar : arrays) {
            const size_t at = ar.a->size() - 1;
            const double keep = (*ar.a)[at];
            (*ar.a)[at] = at % 2 ? nan : inf;
            char needle[64];
            std::snprintf(needle, sizeof needle, "%s holds a non-finite value at element %zu", ar.name, at);
            CHECK(!in.check(1, why) && has(why, needle));
            (*ar.a)[at] = keep;
        }
        in.N[3] = -1e-300;
        CHECK(!in.check(0, why) && has(why, "negative occupancy at segment 1, mixture 1"));
        in.N[3] = 0.0;
        in.E[2] = 0.0;
        CHECK(!in.check(0, why) && has(why, "E must be positive, element 2"));
        in.E[2] = -1.0;
        CHECK(!in.check(1, why) && has(why, "E must be positive, element 2"));
        in.E[2] = 1.0;
        CHECK(in.check(0, why));
    }
    // ---- the plan, swept
    const int64_t Ts[] = {1, 2, 33, 2000, 100000}, Js[] = {1, 2, 70, 260, 1000};
    const int Ks[] = {1, 17, 512}, Ds[] = {1, 39}, Rus[] = {1, 16, 17, 65, 112, 113, 130, 512};
    const int lds[] = {0, 1, 17, 112}, cus[] = {1, 256};
    long plans = 0;
    for (int64_t T : Ts)
        for (int64_t J : Js)
            for (int K : Ks)
                for (int D : Ds)
                    for (int Ru : Rus) {
                        const int Ry = 1 + (int)((T + J) % 300);
                        const int64_t seg = ((int64_t)Ru * Ru + (J + 1) * Ru) * 8, kd = (int64_t)K * D;
                        const int64_t bounds[] = {seg - 1, seg, 3 * seg + 5, (int64_t)1 << 20, GiB, (int64_t)1 << 40};
                        for (int64_t bound : bounds)
                            for (int lr : lds)
                                for (int n_cu : cus)
                                    for (int mode = 0; mode < 2; mode++) {
                                        JfaScorePlan p;
                                        std::string why;
                                        const bool ok = plan_jfa_score(T, J, K, D, Ry, Ru, mode, bound, lr, n_cu, p, why);
                                        if (mode == 0 && bound < seg) {
                                            CHECK(!ok && why.find("jfa_scratch_mib") != std::string::npos);
                                            continue;
                                        }
                                        CHECK(ok);
                                        if (!ok) continue;
                                        plans++;
                                        CHECK(p.mode == mode && p.chunk >= 1 && p.chunk <= T && p.n_chunks == (T + p.chunk - 1) / p.chunk);
                                        CHECK((p.n_chunks - 1) * p.chunk < T);                                       // every segment once
                                        CHECK(p.bytes_N == T * K * 8 && p.bytes_F == T * kd * 8 && p.bytes_out == J * T * 8);
                                        CHECK(p.lds_rows == (lr == 0 ? JFA_LDS_MAX_R : lr) && p.path == (Ru <= p.lds_rows ? 0 : 1));
                                        CHECK(p.gemm_yv.x * JFA_TILE >= kd && p.gemm_yv.y * JFA_TILE >= J && p.gemm_lds <= 64 * 1024);
                                        if (mode == 1) {
                                            CHECK(p.chunk == T && p.bytes_scratch == 0 && p.bytes_comp == T * kd * 8 && p.bytes_M == J * kd * 8);
                                            CHECK(p.gemm_xu.x * JFA_TILE >= kd && p.gemm_xu.y * JFA_TILE >= T && p.gemm_xu.y <= 65535);
                                            CHECK(p.gemm_out.x * JFA_TILE >= T && p.gemm_out.y * JFA_TILE >= J && p.comp.x * JFA_WG >= T * kd);
                                            continue;
                                        }
                                        CHECK(p.seg_bytes == seg && p.chunk == std::min<int64_t>(T, bound / seg) && p.bytes_scratch == p.chunk * seg);
                                        CHECK(p.bytes_scratch <= bound);
                                        CHECK(p.bytes_M == (J + 1) * kd * 8 && p.bytes_ME == p.bytes_M && p.bytes_P == (int64_t)K * Ru * Ru * 8);
                                        CHECK(p.bytes_q == (J + 1) * K * 8 && p.bytes_G == (int64_t)K * Ru * (J + 1) * 8 && p.bytes_a == T * Ru * 8);
                                        CHECK(p.bytes_lin == T * (J + 1) * 8 && p.bytes_quad == p.bytes_lin && p.bytes_comp == 0);
                                        CHECK(p.kscore_lds == jfa_factor_lds_bytes(Ru, p.path) && p.kscore_lds <= 160 * 1024 && p.cross_lds <= 64 * 1024);
                                        CHECK(p.cross.x == K && p.cross.y * JFA_GRAM_TILE >= J + 1 && p.cross.y <= 65535 && p.cross_z * JFA_GRAM_TILE >= Ru);
                                        CHECK(p.gram.x == K && p.gram.y == p.cross_z * p.cross_z);
                                        CHECK(p.gemm_L.x * JFA_TILE >= (int64_t)Ru * Ru && p.gemm_L.y * JFA_TILE >= p.chunk && p.gemm_L.y <= 65535);
                                        CHECK(p.gemm_h.x * JFA_TILE >= (J + 1) * Ru && p.gemm_h.y == p.gemm_L.y && p.gemm_a.x * JFA_TILE >= Ru);
                                        CHECK(p.gemm_lin.x * JFA_TILE >= J + 1 && p.gemm_quad.x == p.gemm_lin.x && p.kscore.x == p.chunk);
                                        CHECK(p.kscore_rounds == (p.chunk + n_cu - 1) / n_cu);
                                        JfaScorePlan one;                                                           // the chunking does not depend on the device
                                        CHECK(plan_jfa_score(T, J, K, D, Ry, Ru, mode, bound, lr, 1, one, why) && one.chunk == p.chunk && one.path == p.path);
                                    }
                    }
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("jfa score checks ok (%ld plans)\n", plans);
    return 0;
}
