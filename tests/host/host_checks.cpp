// Host-side checks of csrc/gmm_model.cpp, csrc/score_plan.cpp (the dispatcher's decisions: mode "plan") and csrc/mfcc_plan.cpp (the MFCC
// stage's table layout and launch decisions: mode "mfcc"); model packers, text format, tail packing, the MFCC kernels' mel sweep starts), built by tests/test_host_sanitizers.py with -fsanitize=address,undefined (and once
// with -fsanitize=thread): the model packers (every layout, threaded and not), the text parser on mutated model texts, and
// the printf / strtod-free number conversions against libc.  Test infrastructure: not part of lib/pygmm.so.
#include "gmm_model.hpp"
#include "mfcc_plan.hpp"
#include "score_plan.hpp"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <stdexcept>

namespace sr {
void fail(const char *fmt, ...) {                      // the library's throws sr::Error; any exception type serves here
    char b[256];
    va_list a;
    va_start(a, fmt);
    vsnprintf(b, sizeof b, fmt, a);
    va_end(a);
    throw std::runtime_error(b);
}
// (an SRModelSet's device buffers stay empty here; their destructors still name these)
bool gpu_runtime_lost() { return false; }
std::atomic<long> g_devbuf_epoch{0};
}  // namespace sr
extern "C" hipError_t hipFree(void *) { return hipSuccess; }
using namespace sr;

static std::vector<GMM> make_set(int S, int K, int D, bool shared, unsigned seed) {
    std::mt19937 r(seed);
    std::normal_distribution<double> nd;
    std::vector<GMM> ms(S);
    for (int s = 0; s < S; s++) {
        GMM &g = ms[s];
        g.nr_mixtures = K;
        g.dim = D;
        if (s == 0 || !shared) {
            g.weights.assign(K, 1.0 / K);
            g.mean.resize((size_t)K * D);
            g.sigma.resize((size_t)K * D);
            for (auto &v : g.mean) v = nd(r) * 3;
            for (auto &v : g.sigma) v = 0.5 + std::abs(nd(r));
        } else {
            g = ms[0];
            for (size_t i = 0; i < g.mean.size(); i += 3) g.mean[i] += 0.1 * nd(r);
        }
    }
    return ms;
}

static int check_packers(int S, int K, int D) {
    for (int shared = 0; shared < 2; shared++) {
        auto ms = make_set(S, K, D, shared != 0, 7 + shared);
        ms[S / 2].weights[K / 2] = 0.0;                 // a dead mixture
        std::vector<const GMM *> v;
        for (auto &g : ms) v.push_back(&g);
        auto host = pack_models(v);
        auto b3 = pack_models_split(v, SPLIT_BF16X3);
        auto h2 = pack_models_split(v, SPLIT_F16X2);
        if (host.params.empty() || b3.params.empty() || h2.params.empty()) return 1;
        if (models_share_sigma_and_weights(v) != (shared != 0 && false)) {
            // (the dead mixture breaks weight sharing on purpose: both answers are exercised below)
        }
        ms[S / 2].weights[K / 2] = 1.0 / K;
        if (shared) {
            if (!models_share_sigma_and_weights(v)) return 2;
            auto sh = pack_models_bx3_shared(v);
            auto hs = pack_models_h2_shared(v);
            if (sh.params.empty() || hs.params.empty() || !(hs.amp > 0)) return 3;
        }
    }
    return 0;
}

static int check_parser(int iters) {
    std::mt19937 r(3);
    auto ms = make_set(1, 5, 7, false, 11);
    const std::string base = gmm_format_text(ms[0]);
    GMM back;
    gmm_parse_text(base, back);
    if (gmm_format_text(back) != base) return 1;
    const char junk[] = "0123456789.eE+-xX nanif\n\t,;:pP";
    long parsed = 0;
    for (int it = 0; it < iters; it++) {
        std::string t = base;
        const int nmut = 1 + (int)(r() % 4);
        for (int m = 0; m < nmut; m++) {
            switch (r() % 4) {
            case 0: t.resize(r() % (t.size() + 1)); break;
            case 1: if (!t.empty()) t[r() % t.size()] = junk[r() % (sizeof junk - 1)]; break;
            case 2: if (!t.empty()) t.insert(r() % t.size(), 1, junk[r() % (sizeof junk - 1)]); break;
            default: if (!t.empty()) t.erase(r() % t.size(), 1 + r() % 3);
            }
        }
        try {
            GMM h;
            gmm_parse_text(std::string(t.data(), t.size()), h);
            parsed++;
            if (h.trained() && h.dim <= 64) (void)pack_models({&h});
        } catch (const std::exception &) {
        }
    }
    return parsed > 0 ? 0 : 2;
}

// the text format's numbers against printf("%g") / strtod, through the only doors the file has: format and parse
static int check_numbers(int n) {
    std::mt19937_64 r(7);
    std::uniform_real_distribution<double> u(0, 1);
    GMM g;
    g.nr_mixtures = 1;
    g.dim = n;
    g.weights = {1.0};
    g.mean.resize(n);
    g.sigma.assign(n, 1.0);
    for (int i = 0; i < n; i++) {
        double v;
        switch (i % 5) {
        case 0: v = (u(r) - 0.5) * 20; break;
        case 1: v = std::pow(10.0, (u(r) - 0.5) * 40) * (u(r) < 0.5 ? -1 : 1); break;
        case 2: v = (std::floor(u(r) * 1e6) + 0.5) * std::pow(10.0, (int)(u(r) * 24) - 12); break;   // ties at the 7th digit
        case 3: v = (double)(long)(u(r) * 2000000) * std::pow(10.0, (int)(u(r) * 30) - 15); break;
        default: { uint64_t b = r(); std::memcpy(&v, &b, 8); if (!(std::fabs(v) < 1e300)) v = 1.0; }
        }
        g.mean[i] = v;
    }
    const std::string text = gmm_format_text(g);
    // line 0: "1", line 1: weights, line 2: "dim cov", line 3: means
    size_t pos = 0;
    for (int l = 0; l < 3; l++) pos = text.find('\n', pos) + 1;
    const char *p = text.c_str() + pos;
    for (int i = 0; i < n; i++) {
        char want[64];
        const int len = snprintf(want, sizeof want, "%g", g.mean[i]);
        if (std::strncmp(p, want, (size_t)len) != 0 || p[len] != ' ') {
            fprintf(stderr, "format of %.17g: got '%.24s', libc '%s'\n", g.mean[i], p, want);
            return 1;
        }
        p += len + 1;
    }
    GMM back;
    gmm_parse_text(text, back);
    for (int i = 0; i < n; i++) {
        char w[64];
        snprintf(w, sizeof w, "%g", g.mean[i]);
        const double ref = std::strtod(w, nullptr);
        if (std::memcmp(&ref, &back.mean[i], 8) != 0) {
            fprintf(stderr, "parse of '%s': %.17g, libc %.17g\n", w, back.mean[i], ref);
            return 2;
        }
    }
    return 0;
}

// pack_tail_tiles: every tile exactly once; full tiles alone and in order; packs of <= 4 tiles and <= 32 columns, all behind the full ones
static int check_tail_packing() {
    std::mt19937 rng(5);
    for (int round = 0; round < 200; round++) {
        const int n = (int)(rng() % 400);
        std::vector<int> counts(n);
        for (int &c : counts) c = (rng() % 3 == 0) ? 1 + (int)(rng() % 31) : 32;
        if (round == 0) counts.assign(64, 8);                          // only tails: 16 packs of 4
        if (round == 1) counts.assign(10, 32);                         // no tails
        for (int pack = 0; pack < 2; pack++) {
            const auto items = pack_tail_tiles(counts, 32, pack != 0);
            std::vector<int> seen(counts.size(), 0);
            bool in_packs = false;
            int last_full = -1;
            for (const auto &it : items) {
                int cols = 0, members = 0;
                for (int p = 0; p < 4; p++) {
                    if (it.t[p] < 0) continue;
                    if (p > 0 && it.t[p - 1] < 0) return 1;               // members are packed to the front
                    if (it.t[p] >= (int)counts.size()) return 2;
                    seen[it.t[p]]++;
                    cols += counts[it.t[p]];
                    members++;
                }
                if (members == 0 || cols > 32) return 3;
                const bool is_pack = pack && counts[it.t[0]] < 32;
                if (!is_pack) {
                    if (members != 1 || in_packs) return 4;               // a full tile after a pack, or sharing its wave
                    if (it.t[0] <= last_full) return 5;
                    last_full = it.t[0];
                } else {
                    in_packs = true;
                    for (int p = 0; p < members; p++)
                        if (counts[it.t[p]] >= 32) return 6;
                }
            }
            for (int v : seen)
                if (v != 1) return 7;
            if (!pack && items.size() != counts.size()) return 8;
        }
        if (round == 0 && pack_tail_tiles(counts, 32, true).size() != 16) return 9;
    }
    return 0;
}

// mel_sweep_starts: starts are multiples of 4, never negative, never above the band's first column, the padded run fits the pass
// wherever the unshifted one did, and no group of bands served together conflicts more than with the unshifted starts; on the
// reference's own 16 kHz / 50-filter bank shape (runs growing with the band index) the first three passes come down to 2 extra
// cycles per read (round 5's choice: 4 / 6 / 4).
static int check_mel_starts() {
    std::mt19937 rng(11);
    for (int round = 0; round < 300; round++) {
        const int B = 1 + (int)(rng() % 64);
        int col0[64] = {0}, cnt[64] = {0}, start[64] = {0}, naive[64] = {0}, pass_len[4] = {0, 0, 0, 0};
        int c = (int)(rng() % 8);
        for (int b = 0; b < B; b++) {
            cnt[b] = (rng() % 20 == 0) ? 0 : 1 + (int)(rng() % (round % 3 == 0 ? 12 : 4 + 3 * b));
            col0[b] = c;
            c += 1 + (int)(rng() % (2 + cnt[b]));
            naive[b] = col0[b] & ~3;
            pass_len[b / 16] = std::max(pass_len[b / 16], ((cnt[b] + 15) / 16) * 16);
        }
        mel_sweep_starts(col0, cnt, B, pass_len, start);
        for (int b = 0; b < B; b++) {
            if (cnt[b] == 0) continue;
            if (start[b] < 0 || (start[b] & 3) || start[b] > col0[b]) return 1;
            const bool fitted = col0[b] - naive[b] + cnt[b] <= pass_len[b / 16];
            if (fitted && col0[b] - start[b] + cnt[b] > pass_len[b / 16]) return 2;
            if (!fitted && start[b] != naive[b]) return 3;
        }
        for (int ps = 0; ps < 4; ps++)
            if (mel_sweep_extra_cycles(start, cnt, B, ps) > mel_sweep_extra_cycles(naive, cnt, B, ps)) return 4;
    }
    // the 16 kHz bank of MFCC.py's defaults: first columns and run lengths as tests/golden's melbank has them
    const int col16k[50] = {1, 5, 10, 15, 20, 26, 31, 38, 44, 51, 58, 65, 73, 81, 90, 99, 108, 118, 129, 140, 152, 164, 177, 190, 204, 219, 235, 251, 268,
                            286, 305, 325, 346, 368, 392, 416, 442, 468, 497, 526, 558, 590, 625, 661, 699, 739, 781, 825, 871, 920};
    const int cnt16k[50] = {9, 10, 10, 11, 11, 12, 13, 13, 14, 14, 15, 16, 17, 18, 18, 19, 21, 22, 23, 24, 25, 26, 27, 29, 31, 32, 33, 35, 37, 39, 41, 43,
                            46, 48, 50, 52, 55, 58, 61, 64, 67, 71, 74, 78, 82, 86, 90, 95, 100, 104};
    const int len16k[4] = {32, 48, 96, 112};
    int st[64] = {0};
    mel_sweep_starts(col16k, cnt16k, 50, len16k, st);
    for (int ps = 0; ps < 3; ps++)
        if (mel_sweep_extra_cycles(st, cnt16k, 50, ps) > 2) return 5;
    if (mel_sweep_extra_cycles(st, cnt16k, 50, 3) != 0) return 6;
    for (int b = 0; b < 50; b++)
        if (col16k[b] - st[b] + cnt16k[b] > len16k[b / 16]) return 7;          // the kernels' unrolled sweep lengths (mel_preset_steps) stand
    return 0;
}

// ---- mode "plan": the dispatcher's decisions (csrc/score_plan.cpp) on sets packed by the library's own pack_model_set ----
// Models: deterministic doubles from splitmix64 of (seed, index), means in [-3, 3), sigmas in [0.5, 1.5).  Kinds: 0 independent
// models; 1 a UBM and MAP-like copies (shared sigma and weights, means moved by < 0.05); 2 orders K and K / 2 alternating;
// 3 every sigma x 0.01 (ill conditioned: amp > 2000); 4 mixture 0 of every model x 0.01 (a few ill-conditioned mixtures: hybrid).
// Expected values: the decisions of the commit BEFORE the plan existed (c90fed6), recorded from a scratch build of it whose
// score_device printed, at the end of its selection, {engine, F, FT, h2s_shape, splitp_w, split_cpm, frames per tile, partials per
// tile, saturation flag}, G and sum_g gcb[g] * (g + 1) -- run on an MI355X (n_cu = 256) over these very sets (built through
// sr_gmm_from_arrays from the same integers) and batches of n_utt utterances of utt_len zero frames.  A hybrid set has two
// rows: its vector half, then its matrix half.
static std::vector<double> unit(uint64_t seed, size_t n) {
    std::vector<double> u(n);
    for (size_t i = 0; i < n; i++) {
        uint64_t z = (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull + seed;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        u[i] = (double)(z >> 11) * (1.0 / 9007199254740992.0);
    }
    return u;
}
struct PlanSet { int S, K, D, kind; };
static std::vector<GMM> make_plan_set(const PlanSet &ps) {
    std::vector<GMM> ms(ps.S);
    for (int s = 0; s < ps.S; s++) {
        GMM &g = ms[s];
        const int K = (ps.kind == 2 && s % 2 == 1) ? ps.K / 2 : ps.K, D = ps.D;
        const int src = ps.kind == 1 ? 0 : s;
        const size_t n = (size_t)K * D;
        g.nr_mixtures = K;
        g.dim = D;
        g.weights.assign(K, 1.0 / K);
        g.mean = unit(1000 + 2 * src, n);
        g.sigma = unit(1001 + 2 * src, n);
        for (auto &v : g.mean) v = (v - 0.5) * 6.0;
        for (auto &v : g.sigma) v = 0.5 + v;
        if (ps.kind == 1 && s > 0) {
            const auto sh = unit(5000 + s, n);
            for (size_t i = 0; i < n; i++) g.mean[i] = g.mean[i] + 0.1 * (sh[i] - 0.5);
        }
        if (ps.kind == 3) for (auto &v : g.sigma) v = v * 0.01;
        if (ps.kind == 4) for (int d = 0; d < D; d++) g.sigma[d] = g.sigma[d] * 0.01;
    }
    return ms;
}
struct PlanCase {
    const char *name;
    int set, n_utt, utt_len;
    int opt[6];            // engine, h2s_shape, split_shape, frames_per_lane, model_groups, mfma_ft (as sr_set_option takes them)
    int flags, n_plans;
    struct { int v[9]; int G; long long gsum; } want[2];
    const char *fail;      // the error a forced engine must raise, or nullptr
};
#include "plan_table.inc"

static int check_plan() {
    const int n_cu = 256;
    int bad = 0, last_set = -1;
    std::unique_ptr<SRModelSet> set;
    for (const PlanCase &c : kPlanCases) {
        if (c.set != last_set) {          // (plan_table.inc is grouped by set: one packed set at a time, each packed once)
            const auto ms = make_plan_set(kPlanSets[c.set]);
            std::vector<const GMM *> v;
            for (auto &g : ms) v.push_back(&g);
            set = std::make_unique<SRModelSet>();
            pack_model_set(*set, v);
            last_set = c.set;
        }
        ScoreOptions opt;
        opt.engine = c.opt[0], opt.h2s_shape = c.opt[1], opt.split_shape = c.opt[2];
        opt.frames_per_lane = c.opt[3], opt.model_groups = c.opt[4], opt.mfma_ft = c.opt[5];
        const int64_t n_rows = (int64_t)c.n_utt * c.utt_len;
        const bool hybrid = set->hy_good && opt.engine == 0;
        if ((c.n_plans == 2) != hybrid) { printf("plan '%s': hybrid %d, recorded %d passes\n", c.name, (int)hybrid, c.n_plans); bad++; continue; }
        for (int h = 0; h < (hybrid ? 2 : 1); h++) {
            const SRModelSet &ss = !hybrid ? *set : h == 0 ? *set->hy_bad : *set->hy_good;
            std::string err;
            ScorePlan p;
            std::vector<int> gcb;
            try {
                p = plan_score(ss, n_rows, c.n_utt, opt, c.flags, n_cu);
                const int64_t n_tiles = (int64_t)c.n_utt * ((c.utt_len + p.tile_frames - 1) / p.tile_frames);
                gcb = plan_groups(ss, p, (int)n_tiles, opt, n_cu);
            } catch (const std::exception &e) {
                err = e.what();
            }
            if (c.fail || !err.empty()) {
                if (!c.fail || err != c.fail) { printf("plan '%s': error '%s', want '%s'\n", c.name, err.c_str(), c.fail ? c.fail : "(none)"); bad++; }
                continue;
            }
            const auto &w = c.want[h];
            const int got[9] = {(int)p.engine, p.F, p.FT, p.h2s_shape, p.splitp_w, p.split_cpm, p.tile_frames, p.per_tile, (int)p.writes_oor};
            long long gsum = 0;
            for (size_t g = 0; g < gcb.size(); g++) gsum += (long long)gcb[g] * (long long)(g + 1);
            if (std::memcmp(got, w.v, sizeof got) != 0 || (int)gcb.size() - 1 != w.G || gsum != w.gsum) {
                printf("plan '%s'[%d]: got {%d, %d, %d, %d, %d, %d, %d, %d, %d}, %d, %lld; want {%d, %d, %d, %d, %d, %d, %d, %d, %d}, %d, %lld\n", c.name, h,
                       got[0], got[1], got[2], got[3], got[4], got[5], got[6], got[7], got[8], (int)gcb.size() - 1, gsum,
                       w.v[0], w.v[1], w.v[2], w.v[3], w.v[4], w.v[5], w.v[6], w.v[7], w.v[8], w.G, w.gsum);
                bad++;
            }
        }
    }
    return bad;
}

// ---- mode "mfcc": the MFCC stage's mel-table layout and launch decisions (csrc/mfcc_plan.cpp) ----
// Pinned rows: what upload_tables / mfcc_extract_with / mfcc_launch_f64 computed inline before the plan became a function of its
// own, on 256 compute units and 100 frames (tests/mfcc_cases.py holds the full table; these are its corner stones).  Then a sweep
// over every FFT size and bank width for the invariants the kernels rely on.
struct MfccRow {
    double fs, win_ms, shift_ms;
    int fft, n_filters, n_ceps;
    int k2, wpb2, k0, n1, nz1, preset, wpb0, cp, pad_floats, pass_len[4], max_read;
    long lds0, lds2;
};
static const MfccRow kMfccRows[] = {
    // the reference's defaults: the 16 kHz lengths are mel preset 1; the 8 kHz bank has 32/48/96/96 and takes the run-time sweep
    {16000, 32, 16, 2048, 50, 13, MFCC_F64_FAST, 8, MFCC_F32_FAST, 16, 4, 1, 12, 16, 4608, {32, 48, 96, 112}, 1031, 144384, 161856},
    {8000, 32, 16, 2048, 50, 13, MFCC_F64_FAST, 8, MFCC_F32_FAST, 16, 4, 0, 12, 16, 4352, {32, 48, 96, 96}, 1031, 143360, 160832},
    // a 2-filter bank: 14592 padded floats -- 4-wave fp32 workgroups and the generic float64 kernel, both because of LDS
    {16000, 25, 10, 2048, 2, 1, MFCC_F64_GENERIC, 4, MFCC_F32_FAST, 16, 4, 0, 4, 16, 14592, {912, 0, 0, 0}, 1027, 106496, 149504},
    // 22050 Hz: 5120 padded floats -- 16 over what the float64 fast kernel has room for; fp32 keeps 12 waves
    {22050, 20, 10, 2048, 50, 13, MFCC_F64_GENERIC, 4, MFCC_F32_FAST, 16, 4, 0, 12, 16, 5120, {32, 48, 112, 128}, 1035, 146432, 149504},
    // frames of 513 samples: the NZ1 = 16 instance, 4 waves
    {16000, 32.0625, 16, 2048, 50, 13, MFCC_F64_GENERIC, 4, MFCC_F32_FAST, 16, 16, 1, 4, 16, 4608, {32, 48, 96, 112}, 1031, 91136, 149504},
    // 17 cepstra: both generic kernels, 32 CMVN columns
    {16000, 32, 16, 2048, 50, 17, MFCC_F64_GENERIC, 4, MFCC_F32_GENERIC, 0, 0, 0, 4, 32, 4608, {32, 48, 96, 112}, 1031, 74752, 149504},
    // FFT 1024 with frames of 640 samples (NZ1 8), FFT 512, FFT 4096 (one float64 wave per workgroup)
    {16000, 40, 20, 1024, 24, 13, MFCC_F64_GENERIC, 4, MFCC_F32_FAST, 8, 8, 0, 4, 16, 2560, {48, 112, 0, 0}, 515, 66560, 75776},
    {16000, 25, 10, 512, 64, 13, MFCC_F64_GENERIC, 4, MFCC_F32_FAST, 4, 4, 0, 12, 16, 1280, {16, 16, 16, 32}, 267, 118784, 38912},
    {16000, 25, 10, 4096, 50, 13, MFCC_F64_GENERIC, 1, MFCC_F32_GENERIC, 0, 0, 0, 4, 16, 8960, {48, 96, 192, 224}, 2059, 148480, 98816},
};

static int check_mfcc_plan() {
    const int n_cu = 256;
    int bad = 0, row = 0;
    for (const MfccRow &r : kMfccRows) {
        SRMfcc m(r.fs, r.win_ms, r.shift_ms, r.fft, r.n_filters, r.n_ceps, 0.95);
        const MelLayout mel = mel_layout(m);
        const MfccPlan p2 = plan_mfcc(m, mel, 2, false, 100, n_cu), p0 = plan_mfcc(m, mel, 0, false, 100, n_cu);
        const bool ok = p2.kernel == r.k2 && p2.wpb == r.wpb2 && p0.kernel == r.k0 && p0.n1 == r.n1 && p0.nz1 == r.nz1 && p0.preset == r.preset &&
                        p0.wpb == r.wpb0 && p0.cp == r.cp && p2.cp == r.cp && mel.pad_floats == r.pad_floats &&
                        std::memcmp(mel.pass_len, r.pass_len, sizeof r.pass_len) == 0 && mel.max_read == r.max_read &&
                        (long)p0.lds == r.lds0 && (long)p2.lds == r.lds2 && mel.n_empty == 0;
        if (!ok) {
            printf("mfcc row %d: k2 %d w2 %d k0 %d N1 %d NZ1 %d preset %d w0 %d cp %d pad %d len {%d, %d, %d, %d} max_read %d lds %zu %zu\n", row,
                   p2.kernel, p2.wpb, p0.kernel, p0.n1, p0.nz1, p0.preset, p0.wpb, p0.cp, mel.pad_floats, mel.pass_len[0], mel.pass_len[1],
                   mel.pass_len[2], mel.pass_len[3], mel.max_read, p0.lds, p2.lds);
            bad++;
        }
        // forced generic: never a fast kernel
        if (plan_mfcc(m, mel, 2, true, 100, n_cu).kernel != MFCC_F64_GENERIC || plan_mfcc(m, mel, 0, true, 100, n_cu).kernel != MFCC_F32_GENERIC) bad++;
        row++;
    }
    {   // frames per wave of the two fast kernels on the default extractor: one round is 256 x 12 (fp32) or 256 x 8 (float64) waves
        SRMfcc m(16000, 32, 16, 2048, 50, 13, 0.95);
        const MelLayout mel = mel_layout(m);
        const struct { int64_t n; int fpw0, fpw2; } want[] = {{1, 1, 1}, {3072, 1, 2}, {3073, 2, 2}, {2048, 1, 1}, {2049, 1, 2},
                                                               {8 * 3072 + 1, 8, 13}, {40 * 3072, 10, 60}, {200 * 2048, 34, 50}};
        for (const auto &w : want) {
            const MfccPlan p0 = plan_mfcc(m, mel, 0, false, w.n, n_cu), p2 = plan_mfcc(m, mel, 2, false, w.n, n_cu);
            if (p0.frames_per_wave != w.fpw0 || p2.frames_per_wave != w.fpw2) {
                printf("mfcc frames per wave at %lld frames: fp32 %lld, float64 %lld\n", (long long)w.n, (long long)p0.frames_per_wave, (long long)p2.frames_per_wave);
                bad++;
            }
        }
    }
    // every FFT size x bank width x a few rates and frame lengths: the invariants the kernels rely on
    const double rates[] = {8000, 11025, 16000, 22050, 44100, 48000};
    for (int fft = 32; fft <= 4096; fft *= 2)
        for (int B = 2; B <= 64; B++)
            for (double fs : rates) {
                const int L = std::min(fft, (int)(0.02 * fs));
                const int C = std::min(B - 1, B % 3 == 0 ? 17 : 13);
                SRMfcc m(fs, (L + 0.5) * 1000.0 / fs, (L / 2 + 0.5) * 1000.0 / fs, fft, B, C, 0.97);
                if (m.frame_len != L) return printf("mfcc sweep: frame of %d samples, wanted %d\n", m.frame_len, L), 1;
                const MelLayout mel = mel_layout(m);
                std::vector<char> used((size_t)std::max(4, mel.pad_floats), 0);
                for (int b = 0; b < B; b++) {
                    if (mel.cnt[b] == 0) continue;
                    if (mel.start[b] < 0 || (mel.start[b] & 3) || mel.start[b] > mel.first[b]) return printf("mfcc sweep: start of band %d\n", b), 2;
                    const int lead = mel.first[b] - mel.start[b];
                    if (lead + mel.cnt[b] > mel.pass_len[b / 16]) return printf("mfcc sweep: run of band %d leaves its pass\n", b), 3;
                    for (int e = 0; e < mel.pass_len[b / 16]; e++) {
                        const size_t i = mel.pad_index(b, e);
                        if (i >= used.size() || used[i]++) return printf("mfcc sweep: padded slot of band %d, element %d\n", b, e), 4;
                    }
                }
                if (mel.runs_contiguous && mel.max_read >= MFCC_PBUF_FLOATS) return printf("mfcc sweep: sweep reads float %d\n", mel.max_read), 5;
                for (int precision = 0; precision <= 2; precision += 2)
                    for (int64_t n : {(int64_t)1, (int64_t)5000, (int64_t)300000}) {
                        const MfccPlan p = plan_mfcc(m, mel, precision, false, n, n_cu);
                        const bool fast = p.kernel == MFCC_F32_FAST || p.kernel == MFCC_F64_FAST;
                        if (p.lds > (size_t)MFCC_LDS_BYTES || p.grid <= 0 || p.wpb <= 0) return printf("mfcc sweep: launch shape\n"), 6;
                        if (fast && (int64_t)p.grid * p.wpb * p.frames_per_wave < n) return printf("mfcc sweep: frames left over\n"), 7;
                        if (fast && ((int64_t)p.grid - 1) * p.wpb * p.frames_per_wave >= n) return printf("mfcc sweep: an idle workgroup\n"), 8;
                        if (fast && (C > 16 || !mel.runs_contiguous)) return printf("mfcc sweep: fast kernel outside its range\n"), 9;
                        if (p.preset != 0 && (p.n1 != 16 || mel.pass_len[0] != 32 || mel.pass_len[1] != 48 || mel.pass_len[2] != 96 || mel.pass_len[3] != 112))
                            return printf("mfcc sweep: preset\n"), 10;
                    }
            }
    return bad;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "mfcc") == 0) {
        const int bad = check_mfcc_plan();
        if (bad) return printf("mfcc plan: %d\n", bad), 90;
        printf("host checks ok\n");
        return 0;
    }
    if (argc > 1 && std::strcmp(argv[1], "plan") == 0) {
        const int bad = check_plan();
        if (bad) return printf("plan: %d cases differ\n", bad), 80;
        printf("host checks ok\n");
        return 0;
    }
    const bool big = argc > 1 && std::strcmp(argv[1], "threads") == 0;     // sizes at which the packers go multi-threaded
    int rc = big ? check_packers(150, 1024, 39) : (check_packers(17, 37, 13) | check_packers(31, 64, 39));
    if (rc) return printf("packers: %d\n", rc), 10 + rc;
    if (!big) {
        if ((rc = check_tail_packing())) return printf("tail packing: %d\n", rc), 40 + rc;
        if ((rc = check_mel_starts())) return printf("mel starts: %d\n", rc), 60 + rc;
        if ((rc = check_parser(20000))) return printf("parser: %d\n", rc), 20 + rc;
        if ((rc = check_numbers(300000))) return printf("numbers: %d\n", rc), 30 + rc;
    }
    printf("host checks ok\n");
    return 0;
}
