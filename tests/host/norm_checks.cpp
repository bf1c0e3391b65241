// norm_checks.cpp -- the decisions of csrc/norm_plan.cpp under the host sanitizers (tests/test_scorenorm_cpu.py builds this with
// -fsanitize=address,undefined and runs it): every refusal's text, and plan_score_norm swept over modes, shapes, cohort sizes,
// top_n, bounds and device sizes -- the chunks cover the test segments exactly once, the bytes stay under the bound, a bound below
// one chunk is refused with the remedy, nothing overflows at the limits.  Host code only: no GPU, nothing loaded into Python.
#include "norm_plan.hpp"

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

static bool has(const std::string &why, const char *needle) {
    if (why.find(needle) != std::string::npos) return true;
    std::printf("refusal text '%s' lacks '%s'\n", why.c_str(), needle);
    return false;
}

static bool refused(int mode, int64_t J, int64_t T, int64_t Cz, int64_t Ct, int top_n, int64_t bound, int n_cu, const char *needle) {
    NormPlan p;
    std::string why;
    if (plan_score_norm(mode, J, T, Cz, Ct, top_n, bound, n_cu, p, why)) return false;
    return has(why, needle);
}

int main() {
    const int64_t GiB = (int64_t)1 << 30;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // ---- refusals of the shape
    CHECK(refused(-1, 2, 3, 4, 4, 2, GiB, 256, "the mode is 0 (z)"));
    CHECK(refused(6, 2, 3, 4, 4, 2, GiB, 256, "the mode is 0 (z)"));
    for (int mode = NORM_Z; mode <= NORM_AS2; mode++) {
        CHECK(refused(mode, 0, 3, 4, 4, 2, GiB, 256, "J, T >= 1"));
        CHECK(refused(mode, 2, 0, 4, 4, 2, GiB, 256, "J, T >= 1"));
        CHECK(refused(mode, NORM_MAX_ROWS + 1, 3, 4, 4, 2, GiB, 256, "split the trial list"));
        CHECK(refused(mode, 3, NORM_MAX_ROWS + 1, 4, 4, 2, GiB, 256, "split the trial list"));
        CHECK(refused(mode, NORM_MAX_ROWS, NORM_MAX_ROWS, 4, 4, 2, GiB, 256, "2^36 values"));
        CHECK(refused(mode, std::numeric_limits<int64_t>::max(), std::numeric_limits<int64_t>::max(), 4, 4, 2, GiB, 256, "split the trial list"));
        CHECK(refused(mode, 2, 3, 4, 4, 2, GiB, 0, "number of compute units"));
        if (norm_needs_enrol(mode)) {
            CHECK(refused(mode, 2, 3, 0, 4, 2, GiB, 256, "Cz is 0"));
            CHECK(refused(mode, 2, 3, NORM_MAX_C + 1, mode == NORM_AS2 ? NORM_MAX_C + 1 : 4, 2, GiB, 256, "up to 16384 members"));
        }
        if (norm_needs_test(mode)) {
            CHECK(refused(mode, 2, 3, 4, 0, 2, GiB, 256, "Ct is 0"));
            CHECK(refused(mode, 2, 3, 4, NORM_MAX_C + 1, 2, GiB, 256, "thin the cohort"));
        }
        if (norm_mode_adaptive(mode)) {
            CHECK(refused(mode, 2, 3, 4, 4, 1, GiB, 256, "top_n >= 2"));
            CHECK(refused(mode, 2, 3, 4, 4, -5, GiB, 256, "top_n is -5"));
        }
    }
    CHECK(refused(NORM_AS2, 2, 3, 4, 5, 2, GiB, 256, "Cz = Ct"));
    {   // a matrix the mode does not read: its cohort size is ignored
        NormPlan p;
        std::string why;
        CHECK(plan_score_norm(NORM_Z, 2, 3, 4, -7, 0, GiB, 256, p, why) && p.bytes_Tt == 0 && p.select_test.x == 0);
        CHECK(plan_score_norm(NORM_T, 2, 3, NORM_MAX_C + 9, 4, 0, GiB, 256, p, why) && p.bytes_Ez == 0 && p.select_enrol.x == 0);
    }
    // ---- refusals of the arrays
    {
        const int64_t J = 2, T = 3, C = 4;
        std::vector<double> S(J * T, 0.5), Ez(J * C, 0.25), Tt(C * T, 0.75), Zt(C * C, 1.0);
        std::string why;
        for (int mode = NORM_Z; mode <= NORM_AS2; mode++) {
            CHECK(norm_check_inputs(mode, J, T, C, C, 2, S.data(), Ez.data(), Tt.data(), Zt.data(), why));
            CHECK(!norm_check_inputs(mode, J, T, C, C, 2, nullptr, Ez.data(), Tt.data(), Zt.data(), why) && has(why, "null argument (S"));
            if (norm_needs_enrol(mode))
                CHECK(!norm_check_inputs(mode, J, T, C, C, 2, S.data(), nullptr, Tt.data(), Zt.data(), why) && has(why, "needs Ez [J][Cz]"));
            else
                CHECK(norm_check_inputs(mode, J, T, C, C, 2, S.data(), nullptr, Tt.data(), nullptr, why));
            if (norm_needs_test(mode))
                CHECK(!norm_check_inputs(mode, J, T, C, C, 2, S.data(), Ez.data(), nullptr, Zt.data(), why) && has(why, "needs Tt [Ct][T]"));
            else
                CHECK(norm_check_inputs(mode, J, T, C, C, 2, S.data(), Ez.data(), nullptr, nullptr, why));
            if (norm_needs_zt(mode))
                CHECK(!norm_check_inputs(mode, J, T, C, C, 2, S.data(), Ez.data(), Tt.data(), nullptr, why) && has(why, "needs Zt [Ct][Cz]"));
            for (double bad : {nan, inf, -inf}) {
                std::vector<double> b = S;
                b[4] = bad;
                CHECK(!norm_check_inputs(mode, J, T, C, C, 2, b.data(), Ez.data(), Tt.data(), Zt.data(), why) && has(why, "S holds a non-finite value at element 4"));
                b = Ez, b[7] = bad;
                CHECK(norm_check_inputs(mode, J, T, C, C, 2, S.data(), b.data(), Tt.data(), Zt.data(), why) == !norm_needs_enrol(mode));
                if (norm_needs_enrol(mode)) CHECK(has(why, "Ez holds a non-finite value at element 7"));
                b = Tt, b[11] = bad;
                CHECK(norm_check_inputs(mode, J, T, C, C, 2, S.data(), Ez.data(), b.data(), Zt.data(), why) == !norm_needs_test(mode));
                if (norm_needs_test(mode)) CHECK(has(why, "Tt holds a non-finite value at element 11"));
                b = Zt, b[15] = bad;
                CHECK(norm_check_inputs(mode, J, T, C, C, 2, S.data(), Ez.data(), Tt.data(), b.data(), why) == !norm_needs_zt(mode));
                if (norm_needs_zt(mode)) CHECK(has(why, "Zt holds a non-finite value at element 15"));
            }
        }
        CHECK(!norm_check_inputs(9, J, T, C, C, 2, S.data(), Ez.data(), Tt.data(), Zt.data(), why) && has(why, "the mode is 0 (z)"));
        CHECK(norm_check_select(J, C, 2, Ez.data(), why) && norm_check_select(J, C, 99, Ez.data(), why));
        CHECK(!norm_check_select(0, C, 2, Ez.data(), why) && has(why, "rows is 0"));
        CHECK(!norm_check_select(J, 0, 2, Ez.data(), why) && has(why, "C is 0"));
        CHECK(!norm_check_select(J, NORM_MAX_C + 1, 2, Ez.data(), why) && has(why, "up to 16384 members"));
        CHECK(!norm_check_select(J, C, 1, Ez.data(), why) && has(why, "top_n >= 2"));
        CHECK(!norm_check_select(J, C, 2, nullptr, why) && has(why, "null argument (X"));
        Ez[5] = nan;
        CHECK(!norm_check_select(J, C, 2, Ez.data(), why) && has(why, "X holds a non-finite value at element 5"));
    }
    // ---- the plan, swept
    long plans = 0;
    for (int mode = NORM_Z; mode <= NORM_AS2; mode++)
        for (int64_t J : {(int64_t)1, (int64_t)17, (int64_t)200, (int64_t)65537})
            for (int64_t T : {(int64_t)1, (int64_t)63, (int64_t)2000, (int64_t)100000})
                for (int64_t C : {(int64_t)1, (int64_t)2, (int64_t)37, (int64_t)2000, NORM_MAX_C})
                    for (int top_n : {2, 40, 1 << 30})
                        for (int n_cu : {1, 64, 256}) {
                            const int64_t fixed = 3 * J * C * 8, seg = (3 * C + 4 * J) * 8;
                            for (int64_t bound : {fixed + seg - 1, fixed + seg, fixed + 3 * seg + 5, (int64_t)1 << 20, GiB, (int64_t)1 << 40}) {
                                NormPlan p;
                                std::string why;
                                const bool ok = plan_score_norm(mode, J, T, C, C, top_n, bound, n_cu, p, why);
                                plans++;
                                if (mode == NORM_AS2 && bound < fixed + seg) {
                                    CHECK(!ok && has(why, "raise the option norm_scratch_mib") && has(why, "below one chunk"));
                                    continue;
                                }
                                CHECK(ok);
                                if (!ok) continue;
                                CHECK(p.mode == mode && p.chunk >= 1 && p.chunk <= T && p.n_chunks >= 1);
                                CHECK((p.n_chunks - 1) * p.chunk < T && T <= p.n_chunks * p.chunk);        // every segment once
                                const bool enrol = norm_needs_enrol(mode), test = norm_needs_test(mode), adaptive = norm_mode_adaptive(mode);
                                CHECK(p.n_sel == (enrol ? (adaptive ? std::min<int64_t>(top_n, C) : C) : 0));
                                CHECK(p.n_sel_test == (test ? (adaptive ? std::min<int64_t>(top_n, C) : C) : 0));
                                CHECK(p.bytes_S == J * T * 8 && p.bytes_out == J * T * 8 && p.bytes_Ez == (enrol ? J * C * 8 : 0));
                                CHECK(p.bytes_Tt == (test ? C * T * 8 : 0) && p.bytes_Zt == (mode == NORM_ZT ? C * C * 8 : 0));
                                CHECK(p.bytes_tnorm == (mode == NORM_ZT ? C * T * 8 : 0));
                                CHECK(p.bytes_moments == ((enrol ? J : 0) + (test ? T : 0) + (mode == NORM_ZT ? C : 0)) * 20);
                                CHECK(p.select_enrol.x == (enrol ? J : 0) && p.select_test.x == (test ? p.chunk : 0));
                                CHECK(p.select_zt.x == (mode == NORM_ZT ? C : 0));
                                CHECK(p.select_lds_enrol == (enrol ? (int)(C * 8) + NORM_SELECT_FIXED_LDS : 0) && p.select_lds_enrol <= 160 * 1024);
                                CHECK(p.select_lds_test == (test ? (int)(C * 8) + NORM_SELECT_FIXED_LDS : 0) && p.select_lds_test <= 160 * 1024);
                                CHECK(p.apply.x == J && p.apply.y == (p.chunk + 255) / 256 && p.apply.y <= 65535);
                                const int64_t widest = std::max(std::max(p.select_enrol.x, p.select_test.x), p.select_zt.x);
                                CHECK(p.select_rounds == (widest + n_cu - 1) / n_cu);
                                if (mode == NORM_AS2) {
                                    CHECK(p.fixed_bytes == fixed && p.seg_bytes == seg && p.bytes_scratch == fixed + p.chunk * seg);
                                    CHECK(p.bytes_scratch <= bound);
                                    CHECK(p.chunk == std::min(T, (bound - fixed) / seg));          // as many segments as fit
                                    CHECK(p.gemm_enrol.x == (p.chunk + 63) / 64 && p.gemm_enrol.y == (J + 63) / 64 && p.gemm_enrol.y <= 65535);
                                    CHECK(p.gemm_test.x == p.gemm_enrol.x && p.gemm_test.y == p.gemm_enrol.y && p.gemm_lds == 2 * 16 * 68 * 8);
                                    CHECK(p.shift_enrol.x == (J * C + 255) / 256 && p.shift_test.x == (p.chunk * C + 255) / 256);
                                    CHECK(p.shift_test.x <= 0x7fffffffLL && p.shift_enrol.x <= 0x7fffffffLL);
                                    CHECK(p.bytes_counts == 8 * p.apply.x * p.apply.y);
                                } else {
                                    CHECK(p.chunk == T && p.n_chunks == 1 && p.bytes_scratch == 0 && p.fixed_bytes == 0 && p.seg_bytes == 0);
                                    CHECK(p.gemm_enrol.x == 0 && p.gemm_test.x == 0 && p.shift_enrol.x == 0 && p.bytes_counts == 0);
                                }
                            }
                        }
    // ---- at the limits: the largest shapes the checks let through, every product in int64
    {
        NormPlan p;
        std::string why;
        const int64_t J = NORM_MAX_ROWS, T = ((int64_t)1 << 36) / J;
        CHECK(plan_score_norm(NORM_AS2, J, T, NORM_MAX_C, NORM_MAX_C, 200, std::numeric_limits<int64_t>::max(), 256, p, why));
        CHECK(p.fixed_bytes == 3 * J * NORM_MAX_C * 8 && p.fixed_bytes > 0 && p.chunk == T && p.bytes_scratch > p.fixed_bytes);
        CHECK(refused(NORM_AS2, J, T, NORM_MAX_C, NORM_MAX_C, 200, std::numeric_limits<int64_t>::min(), 256, "norm_scratch_mib"));
        CHECK(refused(NORM_AS2, J, T, NORM_MAX_C, NORM_MAX_C, 200, 0, 256, "norm_scratch_mib"));
        CHECK(plan_score_norm(NORM_ZT, T, J, NORM_MAX_C, NORM_MAX_C, 0, 0, 1, p, why) && p.select_rounds == J && p.bytes_tnorm == NORM_MAX_C * J * 8);
    }
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("norm checks ok (%ld plans)\n", plans);
    return 0;
}
