// diar_plan.cpp -- the decisions of the diarisation of unknown speakers (diar_plan.hpp).  Host-only.
#include "diar_plan.hpp"

#include <cmath>
#include <cstdio>

namespace sr {

static std::string fmt(const char *f, long long a = 0, long long b = 0, long long c = 0) {
    char buf[480];
    snprintf(buf, sizeof buf, f, a, b, c);
    return buf;
}

static std::string fmtd(const char *f, double a) {
    char buf[320];
    snprintf(buf, sizeof buf, f, a);
    return buf;
}

int64_t diar_segments(int64_t n, int64_t L) {
    if (n <= 0 || L < 1) return 0;
    const int64_t k = n / L;
    return k > 0 ? k : 1;
}

bool ahc_check_stop(double threshold, int k_min, int k_max, std::string &why) {
    if (std::isnan(threshold)) {
        why = "clustering: the threshold is a NaN (-inf merges nothing, +inf merges down to k_min; a NaN is no threshold)";
        return false;
    }
    if (k_min < 1) {
        why = fmt("clustering: k_min is %lld; at least one cluster remains (k_min >= 1)", k_min);
        return false;
    }
    if (k_max != 0 && (k_max < 0 || k_max < k_min)) {
        why = fmt("clustering: k_max is %lld with k_min %lld; k_max is 0 (no cap) or at least k_min", k_max, k_min);
        return false;
    }
    return true;
}

bool diar_check_params(int D, const DiarParams &p, std::string &why) {
    if (D < 1 || D > DIAR_MAX_D) {
        why = fmt("diarisation is built for 1 .. %lld feature dimensions (the factorisation keeps a row per lane of one wave), D is %lld; "
                  "project the features or drop the deltas", DIAR_MAX_D, D);
        return false;
    }
    if (p.L < 1) {
        why = fmt("diarisation: a base segment holds %lld frames; L >= 1", p.L);
        return false;
    }
    if (p.change != DIAR_CHANGE_UNIFORM && p.change != DIAR_CHANGE_BIC) {
        why = fmt("diarisation: change mode %lld; 0 is uniform (every base segment is an initial cluster), 1 is bic", p.change);
        return false;
    }
    if (p.m < 1) {
        why = fmt("diarisation: the change detector's half-width is %lld segments; m >= 1", p.m);
        return false;
    }
    if (!(p.lambda > 0.0) || !std::isfinite(p.lambda)) {
        why = fmtd("diarisation: the penalty weight lambda is %g; it is a finite value > 0", p.lambda);
        return false;
    }
    if (!(p.ridge >= 0.0) || !std::isfinite(p.ridge)) {
        why = fmtd("diarisation: the ridge is %g; it is a finite value >= 0 (0 switches it off)", p.ridge);
        return false;
    }
    return ahc_check_stop(p.threshold, p.k_min, p.k_max, why);
}

bool ahc_check_matrix(int64_t n, const double *dist, int linkage, std::string &why) {
    if (linkage < AHC_AVERAGE || linkage > AHC_SINGLE) {
        why = fmt("clustering: linkage %lld; 0 is average, 1 complete, 2 single", linkage);
        return false;
    }
    if (n < 0 || n > DIAR_MAX_INIT) {
        why = fmt("clustering: %lld items; one call takes 0 .. %lld (the table is n^2 float64): cluster a subset, or centroids first", n, DIAR_MAX_INIT);
        return false;
    }
    if (n > 0 && !dist) {
        why = "clustering: null argument (dist, the dissimilarities [n][n])";
        return false;
    }
    for (int64_t i = 0; i < n; i++)
        for (int64_t j = i + 1; j < n; j++) {
            const double a = dist[i * n + j], b = dist[j * n + i];
            if (std::isnan(a) || std::isnan(b) || a == -INFINITY || b == -INFINITY) {
                why = fmt("clustering: the entry (%lld, %lld) is a NaN or -inf; drop the item or give the pair +inf (it then never merges)", i, j);
                return false;
            }
            if (a != b) {
                why = fmt("clustering: the matrix is not symmetric at (%lld, %lld); pass (M + M^T) / 2", i, j);
                return false;
            }
        }
    return true;
}

int64_t diar_recording_bytes(int D, int64_t n_seg, int64_t n_init) {
    const int64_t P = diar_stat_len(D);
    return (n_seg + n_init) * P * 8 + n_init * n_init * 8 + n_init * 40 + n_seg * 16 + (int64_t)DIAR_ARGMIN_BLOCKS * 16 + 64;
}

int64_t ahc_matrix_bytes(int64_t n) { return n * n * 8 + n * 32 + (int64_t)DIAR_ARGMIN_BLOCKS * 16 + 64; }

bool plan_diar(int D, const DiarParams &prm, const int64_t *lengths, int U, int64_t scratch_bytes, DiarPlan &p, std::string &why) {
    p = DiarPlan();
    if (!diar_check_params(D, prm, why)) return false;
    if (U < 0 || (U > 0 && !lengths)) {
        why = "diarisation: null argument (the recordings' lengths)";
        return false;
    }
    if (scratch_bytes < 1) {
        why = "diarisation: the bound on the tables must be at least 1 byte";
        return false;
    }
    p.D = D;
    p.bucket = diar_bucket(D);
    p.stat_len = diar_stat_len(D);
    p.entries_per_lane = (p.stat_len - 1 + DIAR_STATS_WG - 1) / DIAR_STATS_WG;
    p.stats_lds_bytes = DIAR_STATS_CHUNK * D * 4;
    p.change_lds_bytes = 2 * p.stat_len * 8;
    p.n_seg.resize((size_t)U);
    p.n_init_bound.resize((size_t)U);
    p.bytes.resize((size_t)U);
    p.group_begin.push_back(0);
    int64_t in_group = 0;
    for (int u = 0; u < U; u++) {
        if (lengths[u] < 0) {
            why = fmt("diarisation: recording %lld has a negative length", u);
            return false;
        }
        const int64_t ns = diar_segments(lengths[u], prm.L);
        if (prm.change == DIAR_CHANGE_UNIFORM && ns > DIAR_MAX_INIT) {
            why = fmt("diarisation: recording %lld has %lld base segments, each an initial cluster in uniform mode, and a recording takes "
                      "at most 4096; use longer segments (a larger L) or the bic change detector", u, ns);
            return false;
        }
        const int64_t ni = ns < DIAR_MAX_INIT ? ns : DIAR_MAX_INIT;
        const int64_t b = diar_recording_bytes(D, ns, ni);
        if (b > scratch_bytes) {
            char buf[480];
            snprintf(buf, sizeof buf, "diarisation: recording %d alone keeps %lld bytes on the device (%lld segments, up to %lld initial clusters "
                     "and their table), the bound is %lld bytes; use longer segments (a larger L) or raise the option diar_scratch_mib", u,
                     (long long)b, (long long)ns, (long long)ni, (long long)scratch_bytes);
            why = buf;
            return false;
        }
        p.n_seg[(size_t)u] = ns;
        p.n_init_bound[(size_t)u] = ni;
        p.bytes[(size_t)u] = b;
        if (in_group > 0 && (in_group + b > scratch_bytes || u - p.group_begin.back() >= DIAR_MAX_GROUP)) {
            p.group_begin.push_back(u);
            in_group = 0;
        }
        in_group += b;
    }
    if (U > 0) p.group_begin.push_back(U);
    return true;
}

int diar_labels(int64_t n, const int32_t *merge_i, const int32_t *merge_j, int64_t n_merges, int32_t *label_out) {
    if (n < 0 || n_merges < 0 || n_merges > (n > 0 ? n - 1 : 0)) return -1;
    std::vector<int32_t> root((size_t)n);
    std::vector<char> alive((size_t)n, 1);
    for (int64_t c = 0; c < n; c++) root[(size_t)c] = (int32_t)c;
    for (int64_t t = 0; t < n_merges; t++) {
        const int64_t i = merge_i[t], j = merge_j[t];
        if (i < 0 || j <= i || j >= n || !alive[(size_t)i] || !alive[(size_t)j]) return -1;
        alive[(size_t)j] = 0;
        for (int64_t c = j; c < n; c++)              // (members of j are >= j)
            if (root[(size_t)c] == j) root[(size_t)c] = (int32_t)i;
    }
    std::vector<int32_t> number((size_t)n, -1);
    int k = 0;
    for (int64_t c = 0; c < n; c++) {
        const int32_t r = root[(size_t)c];
        if (number[(size_t)r] < 0) number[(size_t)r] = k++;  // (a root is its cluster's smallest member: met first)
        label_out[c] = number[(size_t)r];
    }
    return k;
}

int64_t diar_cut_steps(int64_t n, const double *merge_d, int64_t n_merges, double threshold, int k_min, int k_max) {
    int64_t live = n, t = 0;
    while (t < n_merges) {
        const double d = merge_d[t];
        if (d == INFINITY) break;
        const bool go = (k_max > 0 && live > k_max) || (live > k_min && d < threshold);
        if (!go) break;
        live--;
        t++;
    }
    return t;
}

}  // namespace sr
