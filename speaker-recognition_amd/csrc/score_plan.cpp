// score_plan.cpp -- the dispatcher's decisions (score_plan.hpp): pure host code, nothing of HIP is called here.  The measured
// crossovers behind every threshold are recorded next to it; tests/host/host_checks.cpp (mode "plan") pins the outcomes.
#include "score_plan.hpp"

#include <algorithm>
#include <cmath>

namespace sr {

ScoreOptions &score_options() {
    static ScoreOptions o;
    return o;
}

static int auto_frames_per_lane(int64_t n_rows, int n_utt, int dp) {
    const int fmax = dp <= 40 ? 4 : dp <= 64 ? 2 : 1;
    if (n_utt == 0) return 1;
    const double mean_len = (double)n_rows / n_utt;
    // pick the largest F whose tiles are mostly full
    for (int f = fmax; f > 1; f >>= 1) {
        const double tile = 256.0 * f;
        const double tiles = std::ceil(mean_len / tile);
        if (mean_len / (tiles * tile) >= 0.80) return f;
    }
    return 1;
}

// best fp32-grade engine whose layout this set carries
static Engine precise_engine(const SRModelSet &set) {
    return mfma_ok(set.shared) ? Engine::SHARED_BF16 : mfma_ok(set.bx3) ? Engine::SPLIT_BF16 : Engine::VECTOR;
}

// engine choice: the matrix-core kernel when its layout exists, is well conditioned and not mostly padding; the vector-ALU
// kernel otherwise
Engine auto_engine(const SRModelSet &set, bool precise) {
    if (!precise && f16_ok(set.h2s)) return Engine::SHARED_F16;
    if (mfma_ok(set.shared)) return Engine::SHARED_BF16;
    if (!precise && f16_ok(set.h2)) return Engine::SPLIT_F16;
    return mfma_ok(set.bx3) ? Engine::SPLIT_BF16 : Engine::VECTOR;
}

static Engine pick_engine(const SRModelSet &set, int forced, bool precise) {
    switch (forced) {
        case 6:
            if (precise) return precise_engine(set);
            if (set.h2s.params.empty()) fail("split-fp16 shared-sigma engine requested but the set does not qualify (>= %d models with "
                                             "identical sigma and weights, packed with that engine available)", SHARED_MIN_MODELS);
            return Engine::SHARED_F16;
        case 5:
            if (precise) return set.bx3.params.empty() ? Engine::VECTOR : Engine::SPLIT_BF16;      // the precise re-run of a forced fp16 engine
            if (set.h2.params.empty()) fail("split-fp16 engine requested but the set has no fp16 layout (sets of more than 65536 mixtures pack "
                                            "only the layouts selected by score_engine when they are created)");
            return Engine::SPLIT_F16;
        case 4:
            if (set.shared.params.empty()) fail("shared-sigma engine requested but the set does not qualify (>= %d models with "
                                                "identical sigma and weights, packed with that engine available)", SHARED_MIN_MODELS);
            return Engine::SHARED_BF16;
        case 3:
            if (set.bx3.params.empty()) fail("split-bf16 engine requested but the set has no bf16x3 layout (sets of more than 65536 mixtures pack "
                                             "only the layouts selected by score_engine when they are created)");
            return Engine::SPLIT_BF16;
        case 0: return auto_engine(set, precise);
        default: return Engine::VECTOR;
    }
}

ScorePlan plan_score(const SRModelSet &set, int64_t n_rows, int n_utt, const ScoreOptions &opt, int flags, int n_cu) {
    const int S = set.host.n_models;
    const int DP = set.host.dp;
    ScorePlan p;
    p.engine = pick_engine(set, opt.engine, (flags & SCORE_PRECISE) != 0);
    const PackedSplit &split = p.engine == Engine::SPLIT_F16 ? set.h2 : set.bx3;
    int F = opt.frames_per_lane ? opt.frames_per_lane : auto_frames_per_lane(n_rows, n_utt, DP);
    if (DP > 40 && F > 2) F = 2;
    if (DP > 64) F = 1;
    // few workgroups (one utterance against one model: every E-step of a MAP enrolment): a lane that holds F frames runs
    // F times as long, so the frames go to more workgroups first (3000 frames x 1 model: 3 workgroups at F = 4, 12 at F = 1)
    if (!opt.frames_per_lane)
        while (F > 1 && ((n_rows + 256 * F - 1) / (256 * F)) * (int64_t)std::max(1, S) < 2 * (int64_t)n_cu) F >>= 1;
    p.F = F;
    if (p.split()) p.FT = opt.mfma_ft ? std::min(opt.mfma_ft, split_max_ft(split.ks)) : 1;   // one column tile per wave won or tied every sweep
    const int64_t n32 = (n_rows + 31) / 32 + n_utt;     // upper bound of the 32-frame tiles
    if (p.engine == Engine::SHARED_F16) {
        // one wide workgroup per CU (one copy of the parameter stream in LDS for all its waves) once its workgroups --
        // tile groups x model blocks, the most the grid can be cut into -- fill the chip six times over; three
        // 4-wave workgroups per CU below that (measured crossover on 201 models x 512 mixtures: 30-50 k frames;
        // at 250 k frames x 1001 models x 2048 mixtures the wide form is 25 % faster, 0.128 s against 0.169 s)
        // Round 4 (scripts/ab_h2s_small.py, 201 x 512 x 39, utterances of 300 frames): the pipelined 12-wave shape wins from
        // ~2000 frames up -- 8 utterances 0.177 against 0.196 ms, 64 utterances 0.76 against 0.95, 256 utterances 2.31 against
        // 3.09 -- and loses below (4 utterances 0.173 against 0.159: a few workgroups, latency-bound); round 3's rule ("fills
        // the chip six times over") kept the 4-wave shape up to 30-50 k frames.
        const bool wide = n32 >= 64 + n_utt;
        // ... and the smallest ones -- one serving utterance: ten tiles -- take the model-split shape: a workgroup per (tile, block)
        // with the block's models dealt to its four waves (gmm_score_h2_shared.hip).  Every such workgroup streams its block's
        // images for ONE tile, so beyond one workgroup per CU the stream (L2 / fabric, 6 TB/s measured) bounds it: 300 frames
        // 0.094 against 0.115 ms, 600 frames 0.123 against 0.114, 1200 frames 0.197 against 0.115 (scripts/ab_h2s_small.py)
        // Round 6: with the images fetched straight into registers (gmm_score_h2m_kernel: no LDS stage to wait out) two such
        // workgroups per CU run side by side -- 300 frames 0.074 ms, 600 and 900 frames 0.095 against 0.112 for the 4-wave shape,
        // 1200 frames (a third workgroup per CU: a second round) 0.141 against 0.111.
        const int64_t ms_wgs = n32 * (int64_t)set.h2s.blocks.size();
        const bool tiny = ms_wgs <= (int64_t)n_cu * (h2s_msplit_direct(set.h2s.klf) ? 2 : 1);
        p.h2s_shape = (opt.h2s_shape == 5 || opt.h2s_shape == 6) ? H2S_PIPELINED_SHAPE : opt.h2s_shape ? opt.h2s_shape - 1 : (tiny ? H2S_MSPLIT_SHAPE : wide ? H2S_PIPELINED_SHAPE : 0);
        if (p.h2s_shape == H2S_PIPELINED_SHAPE && !h2p_fits(set.h2s.kqf, set.h2s.klf)) p.h2s_shape = H2S_WIDE_SHAPE;
    }
    // the generic split-fp16 engine as ONE wide workgroup per CU (gmm_score_splitp.hip) once the batch fills the chip: the 4-wave
    // kernel re-streams every chunk per 128 frames, and the LDS-DMA that takes is what bounds it on large batches
    if (p.engine == Engine::SPLIT_F16 && p.FT == 1 && opt.split_shape != 1) {
        const std::vector<int> &mcb = split.model_chunk_begin;
        p.split_cpm = S > 0 ? mcb[1] - mcb[0] : 0;
        for (int s = 1; s < S; s++)
            if (mcb[s + 1] - mcb[s] != p.split_cpm) p.split_cpm = 0;       // models of different orders: the 4-wave kernel
        if (p.split_cpm > 0) {
            // Measured (profiles/r04_splitp.txt): every shape of this engine delivers the same MFMAs per second on real data -- the
            // socket's power cap sets the clock by the kernel's activity (zero-filled operands: 1.46x faster, same instructions) --
            // so the shapes differ by single percents: 8 waves (two workgroups per CU, one's frame prologue under the other's
            // chains) wins or ties from ~32 chunks per prologue up (configs[1]: 2.69 against 2.78-2.99 ms), the 4-wave kernel keeps
            // the short streams (one 256-mixture model: 0.33 against 0.38 ms) and the small batches
            const int w = splitp_waves_f16x2(split.ks, opt.split_shape ? opt.split_shape : 8);
            // ... and the long contractions only: with fewer than 5 steps (D < 32) a chunk is 6-12 MFMAs against the same ~60-instruction
            // update and the 4-wave kernel wins or ties (100 x 64 mixtures, 1 M frames: D = 26 2.40 against 2.45 ms, D = 20 2.02 / 2.17,
            // D = 13 1.74 / 1.82; configs[4]'s tick of 1024 windows, 20 x 256 x 13: 0.090 against 0.143 -- scripts/ab_split_shape.py)
            if (w > 0 && (opt.split_shape || (split.ks >= 5 && (int64_t)S * p.split_cpm >= 32 &&
                                              (n32 / w) * (int64_t)std::min(S, 16) >= (int64_t)6 * n_cu * splitp_resident_per_cu(w))))
                p.splitp_w = w;
        }
    }
    const bool mat = p.engine != Engine::VECTOR;
    p.tile_frames = (p.engine == Engine::SHARED_F16 || p.split()) ? 32 : mat ? 128 * p.FT : 256 * F;
    p.per_tile = mat ? 1 : 4;
    p.writes_oor = p.engine == Engine::SHARED_F16 || p.engine == Engine::SPLIT_F16;
    return p;
}

std::vector<int> plan_groups(const SRModelSet &set, const ScorePlan &p, int n_tiles, const ScoreOptions &opt, int n_cu) {
    const bool use_h2s = p.engine == Engine::SHARED_F16, use_shared = p.engine == Engine::SHARED_BF16, use_split = p.split();
    const int S = set.host.n_models;
    // model groups: enough workgroups to fill the chip several times over
    int G = opt.model_groups;
    if (G <= 0) {
        // enough workgroups for a short tail: >= ~16 rounds of resident ones for the vector and
        // fp32 matrix kernels; the split-bf16 kernel's workgroups are short, and every extra
        // group re-reads the frame tile, so ~6 rounds (4 resident per CU) are enough there
        const int target = use_h2s ? n_cu * h2s_resident_per_cu(set.h2s.kqf, set.h2s.klf, p.h2s_shape) * 6 : use_shared ? n_cu * 2 * 6
                           : p.splitp_w ? n_cu * splitp_resident_per_cu(p.splitp_w) * 8
                           : use_split ? n_cu * 4 * 6 : n_cu * 3 * 16;
        // (the split-fp16 shared-sigma engine's workgroups, and the wide generic ones, take several 32-frame tiles each)
        const int n_wg_tiles = use_h2s ? (n_tiles + h2s_tiles_per_wg(p.h2s_shape) - 1) / h2s_tiles_per_wg(p.h2s_shape)
                               : p.splitp_w ? (n_tiles + p.splitp_w - 1) / p.splitp_w
                               : use_split ? (n_tiles + 4 * p.FT - 1) / (4 * p.FT) : n_tiles;
        G = (target + n_wg_tiles - 1) / n_wg_tiles;
        if (use_h2s) {
            // Round 4: when the grid is a handful of rounds, WHICH handful matters more than having many workgroups: a
            // workgroup is a frame prologue (about three (block, mixture tile) steps' worth; scripts/debug/h2s_small_one.py
            // with a round-4 build that left the kernel after the prologue: 0.12 of 0.78 ms at 64 utterances x 300 frames) plus its blocks, and the chip runs
            // ceil(workgroups / resident) rounds of the longest one.  64 x 300 frames against 14 blocks: 14 groups = 700
            // workgroups = 3 rounds of (prologue + 1 block); 5 groups = 250 workgroups = 1 round of (prologue + 3 blocks).
            const int n_blocks = (int)set.h2s.blocks.size();
            const int64_t resident = (int64_t)n_cu * h2s_resident_per_cu(set.h2s.kqf, set.h2s.klf, p.h2s_shape);
            const double prologue = 3.0 / std::max(1, set.h2s.n_tiles);      // in units of one block
            double best = 0.0;
            int best_g = 1;
            for (int g = 1; g <= std::min(G, n_blocks); g++) {
                const int64_t rounds = ((int64_t)n_wg_tiles * g + resident - 1) / resident;
                const double cost = (double)rounds * (prologue + (double)((n_blocks + g - 1) / g));
                if (g == 1 || cost < best * 0.999) {
                    best = cost;
                    best_g = g;
                }
            }
            G = best_g;
        }
    }
    const int n_units = use_h2s ? (int)set.h2s.blocks.size()
                        : use_shared ? (int)set.shared.blocks.size() : S;     // what a group is a range of
    G = std::max(1, std::min(G, n_units));
    std::vector<int> gcb(G + 1);
    if (use_shared || use_h2s) {
        for (int g = 0; g <= G; g++) gcb[g] = (int)(((int64_t)g * n_units) / G);
    } else {
        const std::vector<int> &mcb = use_split ? (p.engine == Engine::SPLIT_F16 ? set.h2 : set.bx3).model_chunk_begin : set.host.model_chunk_begin;
        for (int g = 0; g <= G; g++) {
            const int model = (int)(((int64_t)g * S) / G);
            gcb[g] = mcb[model];
        }
    }
    return gcb;
}

std::vector<WorkItem> pack_tail_tiles(const std::vector<int> &counts, int frames_per_tile, bool pack_tails) {
    std::vector<WorkItem> work, packs;
    work.reserve(counts.size());
    int open_n = 4, open_cols = 0;                       // (no pack open)
    for (int t = 0; t < (int)counts.size(); t++) {
        const int c = counts[t];
        if (!pack_tails || c >= frames_per_tile) {
            work.push_back(WorkItem{{t, -1, -1, -1}});
            continue;
        }
        if (open_n == 4 || open_cols + c > frames_per_tile) {
            open_n = 0;
            open_cols = 0;
            packs.push_back(WorkItem{{-1, -1, -1, -1}});
        }
        packs.back().t[open_n++] = t;
        open_cols += c;
    }
    work.insert(work.end(), packs.begin(), packs.end());
    return work;
}

// ---------------- set creation ----------------

// amp_k = sum_d ((mu_kd - centre_d) / sigma_kd)^2 with the centre the matrix-core layouts use (mean of all means)
static std::vector<std::vector<double>> mixture_amps(const std::vector<const GMM *> &models) {
    const int dim = models[0]->dim;
    std::vector<double> centre(dim, 0.0);
    size_t cnt = 0;
    for (const GMM *g : models) {
        for (int k = 0; k < g->nr_mixtures; k++)
            for (int d = 0; d < dim; d++) centre[d] += g->mean[(size_t)k * dim + d];
        cnt += (size_t)g->nr_mixtures;
    }
    for (int d = 0; d < dim; d++) centre[d] = (double)(float)(centre[d] / (double)cnt);
    std::vector<std::vector<double>> amp(models.size());
    for (size_t s = 0; s < models.size(); s++) {
        const GMM &g = *models[s];
        amp[s].assign(g.nr_mixtures, 0.0);
        for (int k = 0; k < g.nr_mixtures; k++)
            for (int d = 0; d < dim; d++) {
                const double v = (g.mean[(size_t)k * dim + d] - centre[d]) / g.sigma[(size_t)k * dim + d];
                amp[s][k] += v * v;
            }
    }
    return amp;
}

static void pack_model_set_plain(SRModelSet &s, const std::vector<const GMM *> &models);

// true when the dispatcher would send the (plainly packed) set to the vector engine because of its conditioning alone
static bool ill_conditioned_only(const SRModelSet &s) {
    if (auto_engine(s, false) != Engine::VECTOR) return false;
    const double amp = !s.bx3.params.empty() ? s.bx3.amp : !s.shared.params.empty() ? s.shared.amp : 0.0;
    const double waste = !s.bx3.params.empty() ? s.bx3.pad_waste : !s.shared.params.empty() ? s.shared.pad_waste : 1.0;
    return amp > MFMA_MAX_AMP && waste <= MFMA_MAX_PAD_WASTE;
}

void pack_model_set(SRModelSet &s, const std::vector<const GMM *> &models) {
    pack_model_set_plain(s, models);
    if (score_options().engine != 0 || s.host.dim > MAX_MATRIX_DIM || !ill_conditioned_only(s)) return;
    // ---- hybrid form: the few offending mixtures on the vector engine, the rest on the matrix cores ----
    const int dim = models[0]->dim;
    const auto amp = mixture_amps(models);
    const bool shared = models.size() > 1 && models_share_sigma_and_weights(models);
    std::vector<std::vector<char>> bad(models.size());
    for (size_t m = 0; m < models.size(); m++) {
        bad[m].assign(models[m]->nr_mixtures, 0);
        for (int k = 0; k < models[m]->nr_mixtures; k++) bad[m][k] = amp[m][k] > 0.5 * F16_MAX_AMP;     // margin: the centre moves
    }
    if (shared)     // keep the sub-sets shared-sigma: the same mixtures leave every model
        for (int k = 0; k < models[0]->nr_mixtures; k++) {
            char any = 0;
            for (size_t m = 0; m < models.size(); m++) any |= bad[m][k];
            for (size_t m = 0; m < models.size(); m++) bad[m][k] = any;
        }
    size_t n_bad = 0, n_all = 0;
    int worst = 0;
    for (size_t m = 0; m < models.size(); m++) {
        int b = 0;
        for (char c : bad[m]) b += c;
        if (b == models[m]->nr_mixtures) return;             // a model made of such mixtures only: nothing to gain
        n_bad += (size_t)b;
        n_all += (size_t)models[m]->nr_mixtures;
        worst = std::max(worst, b);
    }
    if (n_bad == 0 || (double)n_bad > HYBRID_MAX_BAD_FRACTION * (double)n_all) return;
    std::vector<GMM> good_m(models.size()), bad_m(models.size());
    for (size_t m = 0; m < models.size(); m++) {
        const GMM &g = *models[m];
        for (int side = 0; side < 2; side++) {
            GMM &o = side ? bad_m[m] : good_m[m];
            o.dim = dim;
            for (int k = 0; k < g.nr_mixtures; k++) {
                if ((bad[m][k] != 0) != (side != 0)) continue;
                o.weights.push_back(g.weights[k]);            // un-normalised on purpose: the two parts add up to the model
                o.mean.insert(o.mean.end(), g.mean.begin() + (size_t)k * dim, g.mean.begin() + (size_t)(k + 1) * dim);
                o.sigma.insert(o.sigma.end(), g.sigma.begin() + (size_t)k * dim, g.sigma.begin() + (size_t)(k + 1) * dim);
            }
            if (o.weights.empty()) {                          // a model without such mixtures: one dead mixture (weight 0 adds nothing)
                o.weights.push_back(0.0);
                o.mean.insert(o.mean.end(), g.mean.begin(), g.mean.begin() + dim);
                o.sigma.insert(o.sigma.end(), g.sigma.begin(), g.sigma.begin() + dim);
            }
            o.nr_mixtures = (int)o.weights.size();
        }
    }
    std::vector<const GMM *> gp, bp;
    for (size_t m = 0; m < models.size(); m++) {
        gp.push_back(&good_m[m]);
        bp.push_back(&bad_m[m]);
    }
    auto good = std::make_unique<SRModelSet>();
    pack_model_set_plain(*good, gp);
    if (ill_conditioned_only(*good)) return;                  // still ill conditioned without them: stay on the vector engine
    auto badset = std::make_unique<SRModelSet>();
    badset->host = pack_models(bp);                           // vector layout only
    s.hy_good = std::move(good);
    s.hy_bad = std::move(badset);
    s.hy_bad_mixtures = worst;
}

static void pack_model_set_plain(SRModelSet &s, const std::vector<const GMM *> &models) {
    s.host = pack_models(models);
    size_t n_mix = 0;
    for (const GMM *g : models) n_mix += (size_t)g->nr_mixtures;
    if (s.host.dim > MAX_MATRIX_DIM) return;                // wide rows: the vector-ALU engine only
    const bool small = n_mix <= ((size_t)1 << 16);          // every layout is a few MB at most
    const int forced = score_options().engine;
    const bool shared_ok = (int)models.size() >= SHARED_MIN_MODELS && models[0]->dim <= 48 &&   // <= 3 + 4 contraction steps: no scratch
                           models_share_sigma_and_weights(models);
    // the shared-sigma forms: the split-fp16 one when the set is within its range, else split-bf16
    // (small sets carry both, so that either can be forced and the precise re-run has its layout)
    bool h2s_fits = false;
    if (shared_ok && (small || forced == 0 || forced == 6)) {
        s.h2s = pack_models_h2_shared(models);
        h2s_fits = f16_ok(s.h2s);
        if (!small && forced == 0 && !h2s_fits) s.h2s = PackedH2Shared();
    }
    if (shared_ok && (small || forced == 4 || (forced == 0 && !h2s_fits))) s.shared = pack_models_bx3_shared(models);
    if (small || forced == 3 || (forced == 0 && !shared_ok)) s.bx3 = pack_models_split(models, SPLIT_BF16X3);
    if (small || forced == 5 || (forced == 0 && !shared_ok)) s.h2 = pack_models_split(models, SPLIT_F16X2);
}

}  // namespace sr
