// plda_checks.cpp -- the decisions of csrc/plda_plan.cpp under the host sanitizers (tests/test_plda_cpu.py builds this with
// -fsanitize=address,undefined and runs it): every refusal's text, and the two plans swept over dimensions, label patterns, counts,
// bounds, the option jfa_lds_rows and device sizes -- the classes cover the speakers (models) exactly once in ascending count, the
// permutation is one, a speaker's rows come in ascending order, the chunks cover the test segments exactly once under the bound, a
// bound below one chunk is refused with the remedy, nothing overflows at the limits.  Host code only: no GPU, nothing loaded into
// Python.
#include "plda_plan.hpp"

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

static bool train_refused(int64_t n, int R, const int64_t *ids, int64_t S, int lds_rows, int n_cu, const char *needle) {
    PldaPlan p;
    std::string why;
    if (plan_plda_train(n, R, ids, S, lds_rows, n_cu, p, why)) return false;
    return has(why, needle);
}

static bool score_refused(int64_t J, int64_t T, int R, const int64_t *en, int64_t bound, int lds_rows, int n_cu, const char *needle) {
    PldaPlan p;
    std::string why;
    if (plan_plda_score(J, T, R, en, bound, lds_rows, n_cu, p, why)) return false;
    return has(why, needle);
}

// The structure every plan must have: classes ascending and contiguous, perm a permutation sorted by (count, index).
static void check_classes(const PldaPlan &p, const std::vector<int64_t> &count) {
    const int64_t G = (int64_t)count.size();
    CHECK((int64_t)p.perm.size() == G && p.groups == G && !p.classes.empty());
    std::vector<char> seen((size_t)G, 0);
    for (int64_t v : p.perm) {
        CHECK(v >= 0 && v < G && !seen[(size_t)v]);
        if (v >= 0 && v < G) seen[(size_t)v] = 1;
    }
    int64_t at = 0;
    for (size_t c = 0; c < p.classes.size(); c++) {
        const PldaClass &k = p.classes[c];
        CHECK(k.start == at && k.size >= 1 && (c == 0 || p.classes[c - 1].count < k.count));
        for (int64_t s = k.start; s < k.start + k.size && s < G; s++) {
            CHECK(count[(size_t)p.perm[(size_t)s]] == k.count);
            CHECK(s == k.start || p.perm[(size_t)s - 1] < p.perm[(size_t)s]);       // stable: ascending index inside a class
        }
        at += k.size;
    }
    CHECK(at == G);
}

int main() {
    const int64_t GiB = (int64_t)1 << 30;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    std::string why;
    // ---- refusals of the shapes
    {
        const int64_t ids[4] = {0, 1, 1, 0}, en[3] = {1, 2, 1};
        CHECK(train_refused(4, 0, ids, 2, 0, 256, "R >= 1"));
        CHECK(train_refused(4, PLDA_MAX_R + 1, ids, 2, 0, 256, "up to 512 dimensions"));
        CHECK(train_refused(0, 3, ids, 2, 0, 256, "pass at least one row"));
        CHECK(train_refused(PLDA_MAX_ROWS + 1, 3, ids, 2, 0, 256, "split the list"));
        CHECK(train_refused(4, 3, nullptr, 2, 0, 256, "null argument (ids"));
        CHECK(train_refused(4, 3, ids, 0, 0, 256, "1 <= S <= n"));
        CHECK(train_refused(4, 3, ids, 5, 0, 256, "1 <= S <= n"));
        CHECK(train_refused(4, 3, ids, 1, 0, 256, "row 1 has label 1, outside 0 .. 0"));
        CHECK(train_refused(4, 3, ids, 3, 0, 256, "label 2 of 0 .. 2 has no row"));
        const int64_t neg[4] = {0, -1, 1, 0};
        CHECK(train_refused(4, 3, neg, 2, 0, 256, "row 1 has label -1"));
        CHECK(train_refused(4, 3, ids, 2, -1, 256, "jfa_lds_rows must be 0"));
        CHECK(train_refused(4, 3, ids, 2, DENSE_LDS_MAX_R + 1, 256, "jfa_lds_rows must be 0"));
        CHECK(train_refused(4, 3, ids, 2, 0, 0, "number of compute units"));
        CHECK(score_refused(0, 5, 3, en, GiB, 0, 256, "J, the number of models is 0"));
        CHECK(score_refused(3, 0, 3, en, GiB, 0, 256, "T, the number of test segments is 0"));
        CHECK(score_refused(3, PLDA_MAX_ROWS + 1, 3, en, GiB, 0, 256, "split the list"));
        CHECK(score_refused(3, 5, 513, en, GiB, 0, 256, "up to 512 dimensions"));
        CHECK(score_refused(3, 5, 3, nullptr, GiB, 0, 256, "null argument (enrol_n"));
        const int64_t zero[3] = {1, 0, 1};
        CHECK(score_refused(3, 5, 3, zero, GiB, 0, 256, "enrol_n of model 1 is 0"));
        CHECK(score_refused(3, 5, 3, en, 63, 0, 256, "below one chunk of 64 bytes"));
        CHECK(score_refused(3, 5, 3, en, 0, 0, 256, "raise the option plda_scratch_mib"));
        CHECK(score_refused(3, 5, 3, en, std::numeric_limits<int64_t>::min(), 0, 256, "plda_scratch_mib"));
        CHECK(score_refused(3, 5, 3, en, GiB, 0, 0, "number of compute units"));
    }
    // ---- refusals of the arrays
    {
        std::vector<double> M = {2.0, 0.5, 0.5, 3.0};
        CHECK(plda_check_symmetric(M.data(), 2, "Sb", why));
        M[1] = 0.5 + 1e-12;                    // rounding: within 1e-9 of the largest diagonal
        CHECK(plda_check_symmetric(M.data(), 2, "Sb", why));
        M[1] = 0.6;
        CHECK(!plda_check_symmetric(M.data(), 2, "Sw", why) && has(why, "Sw is not symmetric") && has(why, "pass (Sw + Sw^T) / 2"));
        for (double bad : {nan, inf, -inf}) {
            M[1] = M[2] = bad;
            CHECK(!plda_check_symmetric(M.data(), 2, "Sb", why) && has(why, "Sb holds a non-finite value at element 1"));
            std::vector<double> X(12, 0.25);
            X[7] = bad;
            CHECK(!plda_check_finite(X.data(), 12, "X", why) && has(why, "X holds a non-finite value at element 7; drop that vector"));
            CHECK(plda_check_finite(X.data(), 7, "X", why));
        }
    }
    // ---- the training plan, swept
    long plans = 0;
    for (int R : {1, 2, 16, 17, 112, 113, 512})
        for (int pattern = 0; pattern < 4; pattern++)
            for (int64_t S : {(int64_t)1, (int64_t)2, (int64_t)15, (int64_t)16, (int64_t)17, (int64_t)65, (int64_t)1000}) {
                // the speakers' counts: all equal, all 1, all distinct, cycling 1 .. 7; the rows interleaved so that sorting matters
                std::vector<int64_t> count((size_t)S);
                for (int64_t s = 0; s < S; s++) count[(size_t)s] = pattern == 0 ? 3 : pattern == 1 ? 1 : pattern == 2 ? S - s : 1 + (s * 5) % 7;
                std::vector<int64_t> ids, left = count;
                for (bool any = true; any;) {
                    any = false;
                    for (int64_t s = S - 1; s >= 0; s--)
                        if (left[(size_t)s] > 0) left[(size_t)s]--, ids.push_back(s), any = true;
                }
                const int64_t n = (int64_t)ids.size();
                for (int lds_rows : {0, 1, 64})
                    for (int n_cu : {1, 256}) {
                        PldaPlan p;
                        const bool ok = plan_plda_train(n, R, ids.data(), S, lds_rows, n_cu, p, why);
                        plans++;
                        CHECK(ok);
                        if (!ok) continue;
                        CHECK(p.kind == PLDA_TRAIN && p.R == R && p.rows == n);
                        check_classes(p, count);
                        CHECK((int64_t)p.row_order.size() == n && (int64_t)p.row_start.size() == S + 1 && p.row_start[0] == 0 && p.row_start[(size_t)S] == n);
                        std::vector<char> seen((size_t)n, 0);
                        for (int64_t s = 0; s < S; s++) {
                            CHECK(p.row_start[(size_t)s + 1] - p.row_start[(size_t)s] == count[(size_t)p.perm[(size_t)s]]);
                            for (int64_t r = p.row_start[(size_t)s]; r < p.row_start[(size_t)s + 1]; r++) {
                                const int64_t row = p.row_order[(size_t)r];
                                CHECK(row >= 0 && row < n && !seen[(size_t)row] && ids[(size_t)row] == p.perm[(size_t)s]);
                                CHECK(r == p.row_start[(size_t)s] || p.row_order[(size_t)r - 1] < row);
                                if (row >= 0 && row < n) seen[(size_t)row] = 1;
                            }
                        }
                        const int limit = lds_rows == 0 ? DENSE_LDS_MAX_R : lds_rows;
                        CHECK(p.lds_rows == limit && p.path == (R <= limit ? 0 : 1));
                        CHECK(p.factor_lds == (R * 17 + R + (p.path == 0 ? R * R : 0)) * 8 && p.factor_lds <= 160 * 1024);
                        CHECK(p.tri.y == (p.path == 1 ? (R + 3) / 4 : 0) && p.tri.x == (p.path == 1 ? p.invert.x : 0));
                        CHECK(p.sum_chunk == std::min(n, PLDA_SUM_CHUNK) && p.sum_chunk % DENSE_KSTEP * (p.sum_chunks > 1) == 0);
                        CHECK((p.sum_chunks - 1) * p.sum_chunk < n && n <= p.sum_chunks * p.sum_chunk);
                        CHECK((p.grp_chunks - 1) * p.grp_chunk < S && S <= p.grp_chunks * p.grp_chunk);
                        const int64_t nc = (int64_t)p.classes.size();
                        CHECK(p.invert.x == std::max<int64_t>(2, nc) && p.invert_rounds == (p.invert.x + n_cu - 1) / n_cu);
                        CHECK(p.gemm_acc.x == (R + 63) / 64 && p.gemm_acc.y == (R + 63) / 64 && p.gemm_rows.y <= 65535);
                        CHECK(p.class_sums.x == S && p.class_sums.y == (R + 255) / 256 && p.centre.x == (n * R + 255) / 256);
                        CHECK(p.bytes_blocks == (9 + nc) * (int64_t)R * R * 8 && p.bytes_rows == (2 * n + 4 * S) * R * 8);
                    }
            }
    // ---- the scoring plan, swept
    for (int R : {1, 5, 65, 400, 512})
        for (int64_t J : {(int64_t)1, (int64_t)63, (int64_t)65, (int64_t)1000})
            for (int64_t T : {(int64_t)1, (int64_t)64, (int64_t)2000, (int64_t)100000}) {
                std::vector<int64_t> en((size_t)J);
                for (int64_t j = 0; j < J; j++) en[(size_t)j] = 1 + (j * 3) % 7;
                const int64_t seg = (2 * (int64_t)R + 2) * 8;
                for (int64_t bound : {seg - 1, seg, 3 * seg + 5, (int64_t)1 << 20, GiB, (int64_t)1 << 50}) {
                    PldaPlan p;
                    const bool ok = plan_plda_score(J, T, R, en.data(), bound, 0, 256, p, why);
                    plans++;
                    if (bound < seg) {
                        CHECK(!ok && has(why, "below one chunk") && has(why, "raise the option plda_scratch_mib"));
                        continue;
                    }
                    CHECK(ok);
                    if (!ok) continue;
                    check_classes(p, en);
                    CHECK(p.kind == PLDA_SCORE && p.T == T && p.seg_bytes == seg && p.chunk == std::min(T, bound / seg));
                    CHECK(p.bytes_scratch == p.chunk * seg && p.bytes_scratch <= bound);
                    CHECK((p.n_chunks - 1) * p.chunk < T && T <= p.n_chunks * p.chunk);         // every segment once
                    int64_t widest = 0;
                    for (const PldaClass &k : p.classes) widest = std::max(widest, k.size);
                    CHECK(p.gemm_cross.x == (p.chunk + 63) / 64 && p.gemm_cross.y == (widest + 63) / 64 && p.gemm_cross.y <= 65535);
                    CHECK(p.assemble.x == (widest * p.chunk + 255) / 256 && p.assemble.x <= 0x7fffffffLL);
                    CHECK(p.invert.x == std::max<int64_t>(2, (int64_t)p.classes.size() + 1) && p.gemm_rows.y <= 65535);
                    CHECK(p.rowdot.x == (std::max(J, p.chunk) + 3) / 4 && p.tri.y == (R > DENSE_LDS_MAX_R ? (R + 3) / 4 : 0));
                }
            }
    // ---- at the limits: the largest shapes the checks let through, every product in int64
    {
        const int64_t J = PLDA_MAX_ROWS, T = ((int64_t)1 << 36) / J;
        std::vector<int64_t> en((size_t)J, 2);
        PldaPlan p;
        CHECK(plan_plda_score(J, T, PLDA_MAX_R, en.data(), std::numeric_limits<int64_t>::max(), 0, 1, p, why));
        CHECK(p.chunk == T && p.classes.size() == 1 && p.classes[0].size == J && p.assemble.x > 0 && p.bytes_rows > 0);
        CHECK(score_refused(J, T + 1, PLDA_MAX_R, en.data(), GiB, 0, 256, "2^36 values"));
        en[5] = ((int64_t)1 << 40) + 1;
        CHECK(score_refused(J, T, 3, en.data(), GiB, 0, 256, "enrol_n of model 5"));
    }
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("plda checks ok (%ld plans)\n", plans);
    return 0;
}
