// calib_checks.cpp -- the decisions of csrc/calib_plan.cpp under the host sanitizers (tests/test_calib_cpu.py builds this with
// -fsanitize=address,undefined and runs it): every refusal's text, the block counts at the edges of a block, the bytes of every
// array, the state length, the bound's refusal with its remedy, and nothing overflowing for n near 2^62.  Host code only: no GPU,
// nothing loaded into Python.
#include "calib_plan.hpp"

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

static bool plan_refused(int S, int64_t n, int n_thr, int n_cu, const char *needle) {
    CalibPlan p;
    std::string why;
    if (plan_calib(S, n, n_thr, 0, n_cu, p, why)) return false;
    return has(why, needle);
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    std::string why;
    // ---- the shape
    CHECK(plan_refused(0, 4, 0, 256, "up to 8 systems"));
    CHECK(plan_refused(9, 4, 0, 256, "up to 8 systems"));
    CHECK(plan_refused(1, 0, 0, 256, "n is 0; need at least one trial"));
    CHECK(plan_refused(1, -5, 0, 256, "need at least one trial"));
    CHECK(plan_refused(1, CALIB_MAX_N + 1, 0, 256, "split the trial list"));
    for (int64_t n : {((int64_t)1 << 62) - 1, (int64_t)1 << 62, ((int64_t)1 << 62) + 4097, std::numeric_limits<int64_t>::max()})
        for (int S = 1; S <= CALIB_MAX_S; S++) CHECK(plan_refused(S, n, 16, 1, "split the trial list"));
    CHECK(plan_refused(1, 4, 17, 256, "17 thresholds"));
    CHECK(plan_refused(1, 4, -1, 256, "thresholds"));
    CHECK(plan_refused(1, 4, 0, 0, "number of compute units"));
    // ---- the parameters
    CHECK(!calib_check_params(0.0, 0.0, 1e-16, 100, why) && has(why, "the prior is 0"));
    CHECK(!calib_check_params(1.0, 0.0, 1e-16, 100, why) && has(why, "strictly inside (0, 1)"));
    CHECK(!calib_check_params(nan, 0.0, 1e-16, 100, why) && has(why, "the prior is"));
    CHECK(!calib_check_params(0.5, -1e-9, 1e-16, 100, why) && has(why, "the ridge is"));
    CHECK(!calib_check_params(0.5, inf, 1e-16, 100, why) && has(why, "finite value >= 0"));
    CHECK(!calib_check_params(0.5, nan, 1e-16, 100, why) && has(why, "the ridge is"));
    CHECK(!calib_check_params(0.5, 0.0, -1.0, 100, why) && has(why, "tol is -1"));
    CHECK(!calib_check_params(0.5, 0.0, nan, 100, why) && has(why, "tol is"));
    CHECK(!calib_check_params(0.5, 0.0, 0.0, 0, why) && has(why, "max_pass is 0; a call makes 1 .. 1000 passes"));
    CHECK(!calib_check_params(0.5, 0.0, 0.0, 1001, why) && has(why, "max_pass is 1001"));
    CHECK(calib_check_params(0.5, 0.0, 0.0, 1, why) && calib_check_params(1e-3, 5.0, 1e-16, 1000, why));
    // ---- the trials
    {
        CalibCounts c;
        const double X[8] = {1.0, nan, 2.0, inf, 0.5, 0.25, 3.0, nan};          // [2][4]
        const int8_t skip_bad[4] = {1, -1, 0, -7};
        CHECK(calib_check_trials(2, 4, X, skip_bad, c, why) && c.n_t == 1 && c.n_n == 1 && c.n_skip == 2);          // skipped positions are not looked at
        const int8_t nan_trial[4] = {1, 0, 0, -1};
        CHECK(!calib_check_trials(2, 4, X, nan_trial, c, why) && has(why, "system 0 holds a non-finite score at trial 1"));
        const int8_t second[4] = {1, -1, 0, 0};
        const double X2[8] = {1.0, nan, 2.0, 4.0, 0.5, 0.25, 3.0, nan};
        CHECK(!calib_check_trials(2, 4, X2, second, c, why) && has(why, "system 1 holds a non-finite score at trial 3"));
        const int8_t no_tar[4] = {0, -1, 0, -1}, no_non[4] = {1, -1, 1, -1}, none[4] = {-1, -1, -1, -1}, above[4] = {1, 0, 2, 0};
        const double ok[4] = {1.0, 2.0, 3.0, 4.0};
        CHECK(!calib_check_trials(1, 4, ok, no_tar, c, why) && has(why, "0 targets and 2 non-targets"));
        CHECK(!calib_check_trials(1, 4, ok, no_non, c, why) && has(why, "2 targets and 0 non-targets"));
        CHECK(!calib_check_trials(1, 4, ok, none, c, why) && has(why, "need at least one trial of each class"));
        CHECK(!calib_check_trials(1, 4, ok, above, c, why) && has(why, "label 2 is 2"));
        CHECK(!calib_check_trials(1, 4, ok, nullptr, c, why) && has(why, "null argument (lab"));
        const double th_bad[3] = {1.0, nan, 0.0}, th_ok[3] = {1.0, -2.0, 0.0};
        CHECK(!calib_check_theta(2, th_bad, "theta0", why) && has(why, "theta0 holds a non-finite value at element 1"));
        CHECK(calib_check_theta(2, th_ok, "theta0", why));
        const double thr_ok[3] = {-inf, 0.0, inf}, thr_bad[2] = {0.0, nan};
        CHECK(calib_check_thresholds(3, thr_ok, why));
        CHECK(!calib_check_thresholds(2, thr_bad, why) && has(why, "threshold 1 is a NaN"));
        CHECK(!calib_check_thresholds(0, thr_ok, why) && has(why, "0 thresholds"));
        CHECK(!calib_check_thresholds(17, thr_ok, why) && has(why, "17 thresholds"));
        CHECK(!calib_check_thresholds(2, nullptr, why) && has(why, "null argument (thr"));
    }
    // ---- the plan: blocks, bytes, the state length
    const struct { int64_t n, blocks; } edges[] = {{1, 1}, {4095, 1}, {4096, 1}, {4097, 2}, {8192, 2}, {8193, 3}, {257 * 4096 + 1, 258},
                                                   {CALIB_MAX_N, CALIB_MAX_N / 4096}};
    for (const auto &e : edges)
        for (int S = 1; S <= CALIB_MAX_S; S++)
            for (int n_cu : {1, 64, 256}) {
                CalibPlan p;
                CHECK(plan_calib(S, e.n, 16, 0, n_cu, p, why));
                const int P = S + 1, A = 1 + P + P * (P + 1) / 2;
                CHECK(p.n_blocks == e.blocks && p.acc == A && p.state_len == 16 + 4 * P + P * (P + 1) / 2);
                CHECK(p.acc == calib_acc(S) && p.state_len == calib_state_len(S) && calib_off_H(S) + P * (P + 1) / 2 == p.state_len);
                CHECK(p.bytes_X == (int64_t)S * e.n * 8 && p.bytes_lab == e.n && p.bytes_partial == e.blocks * A * 8 && p.bytes_state == p.state_len * 8);
                CHECK(p.bytes_out == e.n * 8 && p.bytes_counts == e.blocks * 2 * 16 * 4 && p.bytes_thr == 128);
                CHECK(p.resident_train == p.bytes_X + p.bytes_lab + p.bytes_partial + p.bytes_state);
                CHECK(p.resident_apply == p.bytes_X + p.bytes_out + P * 8 && p.resident_counts == e.n * 9 + 128 + p.bytes_counts);
                CHECK(p.pass_grid == e.blocks && p.counts_grid == e.blocks && p.apply_grid == e.blocks && p.step_grid == 1);
                CHECK(p.pass_grid * CALIB_WG < ((int64_t)1 << 32));                  // a launch's lanes
                CHECK(p.pass_rounds == (e.blocks + n_cu - 1) / n_cu);
                // every trial lies in exactly one block
                CHECK((p.n_blocks - 1) * CALIB_BLOCK < e.n && e.n <= p.n_blocks * CALIB_BLOCK);
                // ---- the bound: exactly enough passes, one byte less is refused and told what to do
                for (const char *call : {"train", "apply", "counts"}) {
                    const int64_t need = call[0] == 't' ? p.resident_train : call[0] == 'a' ? p.resident_apply : p.resident_counts;
                    CHECK(calib_check_bound(p, call, need, why));
                    CHECK(!calib_check_bound(p, call, need - 1, why) && has(why, "raise the option calib_scratch_mib or calibrate on fewer trials") &&
                          has(why, call));
                }
            }
    CHECK(calib_acc(8) == 55 && calib_state_len(8) == 97 && calib_acc(1) == 6);
    CHECK(std::string(calib_stop_name(0)) == "CONVERGED" && std::string(calib_stop_name(1)) == "CAP" && std::string(calib_stop_name(2)) == "SINGULAR" &&
          std::string(calib_stop_name(3)) == "STALLED" && std::string(calib_stop_name(4)) == "?");
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("calib checks ok\n");
    return 0;
}
