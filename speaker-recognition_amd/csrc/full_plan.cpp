// full_plan.cpp -- the decisions of the float64 full-covariance fit (full_plan.hpp).  Host-only.
#include "full_plan.hpp"

#include <climits>
#include <cstdio>

namespace sr {

static std::string fmt(const char *f, long long a = 0, long long b = 0) {
    char buf[320];
    snprintf(buf, sizeof buf, f, a, b);
    return buf;
}

// a speaker of n frames joins a group: what every buffer grows by
static void add_speaker(FullCounts &c, int K, int D, int64_t n) {
    const int64_t KD = (int64_t)K * D;
    c.X += n * D;
    c.lp += n * K;
    c.lpn += n;
    c.partial += (int64_t)fe_partial_len((long)n, K, D);
    c.prec += KD * D;
    c.cov += KD * D;
    c.mu += KD;
    c.w += K;
    c.logw += K;
    c.logdet += K;
    c.nk += K;
    c.head += 2;
    c.spk += 1;
    c.rec += 1;
    c.wl_lp += fe_lp_blocks((long)n);
    c.wl_lse += fe_lse_blocks((long)n);
    c.wl_cov += fe_n_chunks((long)n);
    c.label += n;
}

int64_t full_speaker_bytes(int K, int D, int64_t n) {
    FullCounts c;
    add_speaker(c, K, D, n);
    return c.bytes();
}

bool plan_full_fit(int K, int D, const int64_t *n, const int *init_given, const int *max_iter, int64_t S, int64_t bound_bytes, FullFitPlan &p,
                   std::string &why) {
    p = FullFitPlan();
    if (K < 1 || D < 1 || D > FULL_MAX_D) {
        why = fmt("full-covariance fit: K %lld, D %lld (K >= 1 and 1 <= D <= 64 are supported)", K, D);
        return false;
    }
    if (K > FULL_MAX_K) {                               // (the mixture is a grid's y in fe_logprob and fe_cov)
        why = fmt("full-covariance fit: %lld components, a launch takes at most %lld", K, FULL_MAX_K);
        return false;
    }
    if (S < 1 || S > INT_MAX || !n || !init_given || !max_iter) {
        why = fmt("full-covariance fit: a plan needs between 1 and 2^31 - 1 speakers (S = %lld)", S);
        return false;
    }
    if (bound_bytes < 1) {
        why = fmt("full_fit_batch_bytes must be >= 1 (the default is %lld)", FULL_DEFAULT_BYTES);
        return false;
    }
    for (int64_t s = 0; s < S; s++)
        if (n[s] < 1 || fe_lp_blocks((long)n[s]) > INT_MAX) {       // (block indices and `chunk` are ints)
            why = fmt("full-covariance fit: speaker %lld has %lld frames (1 to 32 (2^31 - 1) are supported)", s, n[s]);
            return false;
        }
    p.K = K;
    p.D = D;
    p.lds_logprob = sizeof(double) * ((size_t)D * D + D + FE_FB * (D + 1) + 256);
    p.speakers.resize((size_t)S);
    int at = 0;
    while (at < S) {
        FullGroupPlan g;
        g.first = at;
        g.lp0 = (int64_t)p.wl_lp.size();
        g.lse0 = (int64_t)p.wl_lse.size();
        g.cov0 = (int64_t)p.wl_cov.size();
        while (at < S && g.count < FULL_MAX_GROUP) {
            FullSpeakerPlan &sp = p.speakers[(size_t)at];
            sp.n = n[at];
            sp.bytes = full_speaker_bytes(K, D, sp.n);
            if (g.count > 0 && sp.bytes > bound_bytes - g.bytes) break;
            sp.group = (int)p.groups.size();
            sp.slot = g.count;
            sp.row0 = g.rows;
            sp.n_chunks = fe_n_chunks((long)sp.n);
            sp.chunk = (int)((sp.n + sp.n_chunks - 1) / sp.n_chunks);
            sp.o_partial = g.counts.partial;
            add_speaker(g.counts, K, D, sp.n);
            if (g.counts.wl_lp > INT_MAX) {             // (a list's length is a grid's x; the other two lists are shorter)
                why = fmt("full-covariance fit: a group of %lld density blocks, a launch takes at most 2^31 - 1; lower full_fit_batch_bytes",
                          g.counts.wl_lp);
                return false;
            }
            g.bytes = g.counts.bytes();
            g.rows += sp.n;
            g.max_iter = std::max(g.max_iter, max_iter[at]);
            (init_given[at] ? g.any_given : g.any_kmeans) = true;
            for (long b = 0; b < fe_lp_blocks((long)sp.n); b++) p.wl_lp.push_back(FullWork{sp.slot, (int32_t)b});
            for (long b = 0; b < fe_lse_blocks((long)sp.n); b++) p.wl_lse.push_back(FullWork{sp.slot, (int32_t)b});
            for (int c = 0; c < sp.n_chunks; c++) p.wl_cov.push_back(FullWork{sp.slot, c});
            g.count++;
            at++;
        }
        p.max_group_bytes = std::max(p.max_group_bytes, g.bytes);
        p.groups.push_back(g);
    }
    return true;
}

}  // namespace sr
