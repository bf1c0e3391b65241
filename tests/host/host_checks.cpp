// Host-side checks of what csrc/gmm_model.hpp declares, csrc/score_plan.cpp (the dispatcher's decisions: mode "plan") and csrc/mfcc_plan.cpp (the MFCC
// stage's table layout and launch decisions: mode "mfcc"); model packers, text format, tail packing, the MFCC kernels' mel sweep starts), built by tests/test_host_sanitizers.py with -fsanitize=address,undefined (and once
// with -fsanitize=thread): the model packers (every layout, threaded and not), the text parser on mutated model texts, and
// the printf / strtod-free number conversions against libc.  Mode "pack": every packer's image against tests/host/pack_table.inc.
// Test infrastructure: not part of lib/pygmm.so.
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

// ---- mode "pack": the packed images of every layout, pinned (tests/host/pack_table.inc) ----
// A row is one (set, layout) pair: an FNV-1a 64-bit hash over the raw bytes of every vector member of the packed struct (each
// member's byte count, as 8 bytes, goes in ahead of its bytes), every integer member exactly, every double member to a relative
// 1e-12 (libm's log / log2 may differ in the last place between CPUs; the images are fp32 or 16-bit roundings of such sums).
// Sets: make_plan_set's kinds 0 (independent), 1 (UBM + MAP-like copies), 2 (orders K and K / 2), then one of
//   mod 1  weight K / 2 of the middle model 0 (of every model for kind 1: the set stays shared)      -- the fp16 dead-mixture rule
//   mod 2  weight K / 2 of the middle model -0.25
//   mod 3  sigma (K / 2, D / 2) of the middle model 0, its mean 10 (mean - centre != 0: no NaN in the image) -- vector layout only;
//          flush_band comes out infinite
// Layouts: every one that accepts the set -- the matrix-core ones up to MAX_MATRIX_DIM dimensions, the shared-sigma ones where
// models_share_sigma_and_weights holds, the compact order for every h2-shared image (empty where the form does not apply).
// `pack print` writes the table; it is recorded ONCE from the commit named above the table, never from the code under test.
enum { PK_VECTOR, PK_BF16X3, PK_F16X2, PK_BX3_SHARED, PK_H2_SHARED, PK_H2_COMPACT, PK_LAYOUTS };
static const char *const kPackLayoutNames[PK_LAYOUTS] = {"PK_VECTOR", "PK_BF16X3", "PK_F16X2", "PK_BX3_SHARED", "PK_H2_SHARED", "PK_H2_COMPACT"};
struct PackSet { int S, K, D, kind, mod; };
struct PackRow {
    PackSet set;
    int layout;
    unsigned long long hash;
    long long iv[6];       // the struct's integer members in declaration order (h2-shared: then its ref's), the rest 0
    double dv[8];          // its double members in declaration order (h2-shared: then its ref's), the rest 0
};
struct PackError { const char *what, *text; };
#include "pack_table.inc"

struct Fnv {
    uint64_t h = 0xcbf29ce484222325ull;
    void bytes(const void *p, size_t n) {
        const unsigned char *b = (const unsigned char *)p;
        for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
    }
    template <class T>
    void vec(const std::vector<T> &v) {
        const uint64_t n = (uint64_t)v.size() * sizeof(T);
        bytes(&n, 8);
        if (n) bytes(v.data(), (size_t)n);
    }
};

static std::vector<GMM> make_pack_set(const PackSet &ps) {
    auto ms = make_plan_set(PlanSet{ps.S, ps.K, ps.D, ps.kind});
    const int mid = ps.S / 2, k = ms[mid].nr_mixtures / 2;
    if (ps.mod == 1)
        for (int s = 0; s < ps.S; s++)
            if (s == mid || ps.kind == 1) ms[s].weights[ms[s].nr_mixtures / 2] = 0.0;
    if (ps.mod == 2) ms[mid].weights[k] = -0.25;
    if (ps.mod == 3) {
        ms[mid].sigma[(size_t)k * ps.D + ps.D / 2] = 0.0;
        ms[mid].mean[(size_t)k * ps.D + ps.D / 2] = 10.0;
    }
    return ms;
}

static void add_split(const PackedSplit &p, Fnv &f, PackRow &r, int i0, int d0) {
    f.vec(p.params), f.vec(p.chunks), f.vec(p.model_chunk_begin), f.vec(p.center), f.vec(p.scale);
    r.iv[i0] = p.scheme, r.iv[i0 + 1] = p.parts, r.iv[i0 + 2] = p.ks;
    r.dv[d0] = p.amp, r.dv[d0 + 1] = p.pad_waste, r.dv[d0 + 2] = p.sigma_ratio, r.dv[d0 + 3] = p.coef_max;
}

// the rows of one set, in layout order
static std::vector<PackRow> pack_rows(const PackSet &ps, bool vector_and_h2_shared_only = false) {
    const auto ms = make_pack_set(ps);
    std::vector<const GMM *> v;
    for (auto &g : ms) v.push_back(&g);
    std::vector<PackRow> rows;
    auto row = [&](int layout) -> PackRow & {
        rows.push_back(PackRow{ps, layout, 0, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}});
        return rows.back();
    };
    const bool shared = models_share_sigma_and_weights(v);
    {
        const PackedModels p = pack_models(v);
        PackRow &r = row(PK_VECTOR);
        Fnv f;
        f.vec(p.params), f.vec(p.center), f.vec(p.chunks), f.vec(p.model_chunk_begin), f.vec(p.model_mixtures);
        r.hash = f.h;
        r.iv[0] = p.n_models, r.iv[1] = p.dim, r.iv[2] = p.dp, r.iv[3] = shared;
        r.dv[0] = p.flush_band;
    }
    if (ps.D > MAX_MATRIX_DIM || ps.mod == 3) return rows;
    for (int scheme : {SPLIT_BF16X3, SPLIT_F16X2}) {
        if (vector_and_h2_shared_only) break;
        const PackedSplit p = pack_models_split(v, scheme);
        PackRow &r = row(scheme == SPLIT_BF16X3 ? PK_BF16X3 : PK_F16X2);
        Fnv f;
        add_split(p, f, r, 0, 0);
        r.hash = f.h;
    }
    if (!shared) return rows;
    if (!vector_and_h2_shared_only) {
        const PackedBx3Shared p = pack_models_bx3_shared(v);
        PackRow &r = row(PK_BX3_SHARED);
        Fnv f;
        f.vec(p.params), f.vec(p.blocks), f.vec(p.center);
        r.hash = f.h;
        r.iv[0] = p.kq, r.iv[1] = p.kl, r.iv[2] = p.n_tiles;
        r.dv[0] = p.amp, r.dv[1] = p.pad_waste;
    }
    const PackedH2Shared hs = pack_models_h2_shared(v);
    {
        PackRow &r = row(PK_H2_SHARED);
        Fnv f;
        f.vec(hs.params), f.vec(hs.blocks), f.vec(hs.center), f.vec(hs.scale), f.vec(hs.q_desc), f.vec(hs.l_desc);
        r.iv[0] = hs.kqf, r.iv[1] = hs.klf, r.iv[2] = hs.n_tiles;
        r.dv[0] = hs.amp, r.dv[1] = hs.pad_waste, r.dv[2] = hs.sigma_ratio, r.dv[3] = hs.coef_max;
        add_split(hs.ref, f, r, 3, 4);
        r.hash = f.h;
    }
    if (!vector_and_h2_shared_only) {
        const PackedH2Compact p = pack_h2_compact(hs, ps.D);
        PackRow &r = row(PK_H2_COMPACT);
        Fnv f;
        f.vec(p.params), f.vec(p.blocks), f.vec(p.q_desc), f.vec(p.l_desc);
        r.hash = f.h;
        r.iv[0] = p.nk, r.iv[1] = p.nf, r.iv[2] = p.nb;
    }
    return rows;
}

static std::vector<PackSet> pack_sets() {
    static const int shapes[][3] = {{1, 1, 1},    {1, 4, 8},    {3, 5, 13},   {2, 33, 39}, {15, 32, 39}, {16, 32, 39}, {31, 64, 37},
                                    {16, 33, 40}, {4, 32, 64},  {2, 7, 65},   {2, 4, 100}, {2, 4, 130}};
    static const int kinds[][2] = {{0, 0}, {1, 0}, {2, 0}, {0, 1}, {1, 1}, {0, 2}, {0, 3}};      // {kind, mod}
    std::vector<PackSet> sets;
    for (const auto &sh : shapes)
        for (const auto &km : kinds) {
            if (km[0] == 1 && sh[0] < 2) continue;          // a UBM without copies is kind 0 again
            if (km[0] == 2 && sh[1] < 2) continue;          // no order K / 2 below K = 2
            if (km[1] == 3 && sh[0] * sh[1] < 2) continue;  // a lone mixture IS the centre
            sets.push_back(PackSet{sh[0], sh[1], sh[2], km[0], km[1]});
        }
    return sets;
}
// the set of mode "threads": host_parallel_for goes threaded at pieces x cost >= 2^22 (64 pieces for pack_models, 5 blocks for
// pack_models_h2_shared); its two rows stand at the end of the table
static const PackSet kThreadedPackSet = {64, 2048, 39, 1, 0};

static std::string pack_error(int which) {
    try {
        auto ms = make_plan_set(PlanSet{3, 5, 13, 0});
        std::vector<const GMM *> v;
        for (auto &g : ms) v.push_back(&g);
        GMM other;
        if (which == 0) ms[1] = GMM();
        if (which == 1) other = make_plan_set(PlanSet{1, 5, 14, 0})[0], v[1] = &other;
        if (which == 2) v.clear();
        if (which == 3) (void)pick_padded_dim(MAX_DIM + 1);
        else (void)pack_models(v);
    } catch (const std::exception &e) {
        return e.what();
    }
    return "(no error)";
}

static void print_double(double v) {
    if (std::isinf(v)) printf("%sINFINITY", v < 0 ? "-" : "");
    else printf("%.17g", v);
}

static int print_pack_table() {
    auto sets = pack_sets();
    printf("static const PackRow kPackRows[] = {\n");
    size_t n_single = 0;
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 1) sets.assign(1, kThreadedPackSet);
        for (const PackSet &ps : sets)
            for (const PackRow &r : pack_rows(ps, pass == 1)) {
                printf("    {{%d, %d, %d, %d, %d}, %s, 0x%016llxull, {", ps.S, ps.K, ps.D, ps.kind, ps.mod, kPackLayoutNames[r.layout], r.hash);
                for (int i = 0; i < 6; i++) printf("%s%lld", i ? ", " : "", r.iv[i]);
                printf("}, {");
                for (int i = 0; i < 8; i++) {
                    if (std::isnan(r.dv[i])) return fprintf(stderr, "a NaN among the doubles of a row\n"), 1;
                    printf("%s", i ? ", " : "");
                    print_double(r.dv[i]);
                }
                printf("}},\n");
                n_single += pass == 0;
            }
    }
    printf("};\nstatic const size_t kPackSingleRows = %zu;       // the rows of mode \"pack\"; the rest belong to mode \"threads\"\n", n_single);
    printf("static const PackError kPackErrors[] = {\n");
    static const char *const what[4] = {"an untrained model", "a model of another dimension", "an empty set", "dimension MAX_DIM + 1"};
    for (int i = 0; i < 4; i++) printf("    {\"%s\", \"%s\"},\n", what[i], pack_error(i).c_str());
    printf("};\n");
    return 0;
}

static bool same_double(double got, double want) {
    if (std::isinf(want) || std::isinf(got)) return got == want;
    return std::fabs(got - want) <= 1e-12 * std::max(std::fabs(got), std::fabs(want));     // (false for a NaN)
}

static int compare_pack_rows(const std::vector<PackRow> &got, const PackRow *want, size_t n_want) {
    int bad = 0;
    if (got.size() != n_want) return printf("pack: %zu rows, the table has %zu\n", got.size(), n_want), 1;
    for (size_t i = 0; i < got.size(); i++) {
        const PackRow &g = got[i], &w = want[i];
        bool ok = std::memcmp(&g.set, &w.set, sizeof g.set) == 0 && g.layout == w.layout && g.hash == w.hash && std::memcmp(g.iv, w.iv, sizeof g.iv) == 0;
        for (int d = 0; d < 8; d++) ok = ok && same_double(g.dv[d], w.dv[d]);
        if (ok) continue;
        bad++;
        printf("pack row %zu (%d x %d x %d kind %d mod %d, %s): hash %016llx, ints {%lld, %lld, %lld, %lld, %lld, %lld}, doubles {", i, g.set.S, g.set.K,
               g.set.D, g.set.kind, g.set.mod, kPackLayoutNames[g.layout], g.hash, g.iv[0], g.iv[1], g.iv[2], g.iv[3], g.iv[4], g.iv[5]);
        for (int d = 0; d < 8; d++) printf("%s%.17g", d ? ", " : "", g.dv[d]);
        printf("}; the table has %d x %d x %d kind %d mod %d, %s: hash %016llx, ints {%lld, %lld, %lld, %lld, %lld, %lld}, doubles {", w.set.S, w.set.K,
               w.set.D, w.set.kind, w.set.mod, kPackLayoutNames[w.layout], w.hash, w.iv[0], w.iv[1], w.iv[2], w.iv[3], w.iv[4], w.iv[5]);
        for (int d = 0; d < 8; d++) printf("%s%.17g", d ? ", " : "", w.dv[d]);
        printf("}\n");
    }
    return bad;
}

static int check_pack() {
    std::vector<PackRow> got;
    for (const PackSet &ps : pack_sets())
        for (const PackRow &r : pack_rows(ps)) got.push_back(r);
    int bad = compare_pack_rows(got, kPackRows, kPackSingleRows);
    for (int i = 0; i < 4; i++) {
        const std::string e = pack_error(i);
        if (e != kPackErrors[i].text) { printf("pack error of %s: '%s', want '%s'\n", kPackErrors[i].what, e.c_str(), kPackErrors[i].text); bad++; }
    }
    return bad;
}

static int check_pack_threaded() {
    const size_t n_all = sizeof kPackRows / sizeof kPackRows[0];
    return compare_pack_rows(pack_rows(kThreadedPackSet, true), kPackRows + kPackSingleRows, n_all - kPackSingleRows);
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "pack") == 0) {
        if (argc > 2 && std::strcmp(argv[2], "print") == 0) return print_pack_table();
        const int bad = check_pack();
        if (bad) return printf("pack: %d rows differ\n", bad), 70;
        printf("host checks ok\n");
        return 0;
    }
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
    if (big && (rc = check_pack_threaded())) return printf("threaded pack: %d rows differ\n", rc), 70;
    if (!big) {
        if ((rc = check_tail_packing())) return printf("tail packing: %d\n", rc), 40 + rc;
        if ((rc = check_mel_starts())) return printf("mel starts: %d\n", rc), 60 + rc;
        if ((rc = check_parser(20000))) return printf("parser: %d\n", rc), 20 + rc;
        if ((rc = check_numbers(300000))) return printf("numbers: %d\n", rc), 30 + rc;
    }
    printf("host checks ok\n");
    return 0;
}
