// h2c_checks.cpp -- the compact order of the pipelined shared-sigma kernel on the host: csrc/score_shapes.hpp's map (h2c_map,
// h2c_younger) and csrc/model_pack_shared.cpp's pack_h2_compact beside the flat pack_models_h2_shared.  A stand-alone program, built by
// tests/test_h2c_host.py with g++ -fsanitize=address,undefined (host code only).
//   map:   a wave's fragment reads and waits replayed on an in-order queue for every part length: the fragment an MFMA step names
//          has arrived, belongs to the image being multiplied, and its register is refilled only after the image's last use of it;
//          the chain holds every (part of A, part of z, half-step) product the three part products need, once
//   pack:  random MAP-shaped sets at D = 37, 38, 39: per mixture row of every image, the compact pack and the flat pack hold the same
//          multiset of (fp16 bits of the A slot, frame-side descriptor) pairs, the constant's two included; phantom images are zeros;
//          D = 40 has no compact form
#include "gmm_model.hpp"
#include "score_shapes.hpp"

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <deque>
#include <map>
#include <random>
#include <stdexcept>
#include <utility>
#include <vector>

namespace sr {
void fail(const char *fmt, ...) {                      // the library's throws sr::Error; any exception type serves here
    char b[256];
    va_list a;
    va_start(a, fmt);
    vsnprintf(b, sizeof b, fmt, a);
    va_end(a);
    throw std::runtime_error(b);
}
// (a GMM handle's cached sets and their device buffers stay empty here; their destructors still name these)
bool gpu_runtime_lost() { return false; }
std::atomic<long> g_devbuf_epoch{0};
}  // namespace sr
extern "C" hipError_t hipFree(void *) { return hipSuccess; }

using namespace sr;

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                             \
        }                                                                           \
    } while (0)

static void check_map(int h) {
    const H2cMap m = h2c_map(h);
    CHECK(h2c_map_ok(m));
    CHECK(m.nk == (3 * h + 1) / 2 && m.nf == h + (h & 1) && m.nb == m.nf);
    // the products: (A part, z part, half-step) of every half of every step; hi x lo, hi x hi, lo x hi of each half-step once
    std::map<std::vector<int>, int> seen;
    for (int u = 0; u < m.nk; u++)
        for (int hh = 0; hh < 2; hh++) {
            const int a = m.a_half[m.a_of[u]][hh], b = m.b_half[m.b_of[u]][hh];
            if (a < 0 || b < 0) continue;
            CHECK((a & 15) == (b & 15));                                  // the same eight dimensions on both sides
            seen[{a >> 4, b >> 4, a & 15}]++;
        }
    for (int p = 0; p < h; p++) {
        CHECK((seen[{0, 0, p}] == 1));                                   // hi(A) x lo(z)
        CHECK((seen[{0, 1, p}] == 1));                                   // hi(A) x hi(z)
        CHECK((seen[{1, 1, p}] == 1));                                   // lo(A) x hi(z)
        CHECK((seen[{1, 0, p}] == 0));
    }
    CHECK((int)seen.size() == 4 * h);                                     // (the absent lo x lo entries the lookups above created)
    // a wave's reads and waits over a few images, on a queue that returns in order
    std::deque<std::pair<int, int>> inflight;                             // {fragment, image}
    std::vector<int> holds(m.nf, -1), arrived(m.nf, -1);                  // image a register was last asked to hold / holds
    auto wait_for = [&](size_t keep) {
        while (inflight.size() > keep) {
            arrived[inflight.front().first] = inflight.front().second;
            inflight.pop_front();
        }
    };
    for (int f = 0; f < m.nf; f++) {                                      // in front of the loop: the first image, F0 F1 ..
        inflight.push_back({f, 0});
        holds[f] = 0;
    }
    for (int img = 0; img < 4; img++)
        for (int u = 0; u < m.nk; u++) {
            const int f = m.a_of[u];
            wait_for((size_t)h2c_younger(m, u));
            CHECK(holds[f] == img && arrived[f] == img);                  // read before its use, and not yet overwritten
            if (m.a_last[f] == u) {                                       // refilled only after the image's last use
                for (int later = u + 1; later < m.nk; later++) CHECK(m.a_of[later] != f);
                inflight.push_back({f, img + 1});
                holds[f] = img + 1;
            }
            CHECK(inflight.size() <= 15);
        }
    for (int r = 0; r < m.nb; r++) CHECK(m.b_last[r] >= 0 && m.b_last[r] < m.nk && m.b_of[m.b_last[r]] == r);
}

static GMM make_gmm(int K, int D, std::mt19937 &rng, const GMM *ubm) {
    std::normal_distribution<double> nd(0.0, 1.0);
    std::uniform_real_distribution<double> ud(0.5, 2.0);
    GMM g;
    g.dim = D;
    g.nr_mixtures = K;
    g.weights.resize(K);
    g.mean.resize((size_t)K * D);
    g.sigma.resize((size_t)K * D);
    double ws = 0.0;
    for (int k = 0; k < K; k++) ws += (g.weights[k] = ubm ? ubm->weights[k] : ud(rng));
    for (int k = 0; k < K; k++)
        if (!ubm) g.weights[k] /= ws;
    for (size_t e = 0; e < (size_t)K * D; e++) {
        g.sigma[e] = ubm ? ubm->sigma[e] : ud(rng);
        g.mean[e] = ubm ? ubm->mean[e] + 0.3 * nd(rng) : 3.0 * nd(rng);
    }
    return g;
}

// the multiset of (A bits, descriptor) pairs with a live frame side of row i of an image of `nsteps` steps
static std::vector<std::pair<int, int>> row_pairs(const uint16_t *img, int nsteps, int i, const std::vector<uint16_t> &desc) {
    std::vector<std::pair<int, int>> out;
    for (int c = 0; c < nsteps * 16; c++) {
        const int ks = c >> 4, hh = (c >> 3) & 1, j = c & 7;
        if (desc[c] != 0) out.push_back({img[((size_t)ks * 64 + i + 32 * hh) * 8 + j], desc[c]});
    }
    std::sort(out.begin(), out.end());
    return out;
}

static void check_pack(int D, int K, int S, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<GMM> store;
    store.reserve(S);
    store.push_back(make_gmm(K, D, rng, nullptr));
    for (int s = 1; s < S; s++) store.push_back(make_gmm(K, D, rng, &store[0]));
    std::vector<const GMM *> models;
    for (const GMM &g : store) models.push_back(&g);
    const PackedH2Shared flat = pack_models_h2_shared(models);
    const PackedH2Compact cpt = pack_h2_compact(flat, D);
    if (!h2c_applies(D, flat.klf)) {
        CHECK(cpt.nk == 0 && cpt.params.empty());
        return;
    }
    const H2cMap m = h2c_map(h2c_half_steps(D));
    CHECK(cpt.nk == m.nk && cpt.nf == m.nf && cpt.nb == m.nb && cpt.nk == flat.klf);
    CHECK(cpt.q_desc.size() == (size_t)m.nb * 16 && cpt.l_desc.size() == (size_t)m.nb * 16);
    const int kimg = std::max(flat.kqf, flat.klf);
    const size_t flat_u16 = (size_t)kimg * 512, img_u16 = (size_t)m.nf * 512;
    const size_t per_block = (size_t)flat.n_tiles * (1 + SHARED_SB);
    CHECK(cpt.blocks.size() == flat.blocks.size());
    CHECK(cpt.params.size() == flat.blocks.size() * per_block * img_u16);
    CHECK((4 * m.nf) % 12 == 0 && (4 * m.nf) / 12 == 2);                  // a stage of four images: two 1 KiB pieces per wave
    // step-indexed views of the compact tables: A slot of step u = stored fragment a_of[u], frame side = register b_of[u]
    std::vector<uint16_t> qd((size_t)m.nk * 16), ld((size_t)m.nk * 16);
    for (int u = 0; u < m.nk; u++)
        for (int c = 0; c < 16; c++) {
            qd[16 * u + c] = cpt.q_desc[16 * m.b_of[u] + c];
            ld[16 * u + c] = cpt.l_desc[16 * m.b_of[u] + c];
        }
    std::vector<uint16_t> steps((size_t)m.nk * 512);
    for (size_t b = 0; b < flat.blocks.size(); b++) {
        CHECK(cpt.blocks[b].first_model == flat.blocks[b].first_model && cpt.blocks[b].n_models == flat.blocks[b].n_models);
        CHECK((size_t)cpt.blocks[b].offset_u4 * 8 == b * per_block * img_u16);
        CHECK((size_t)flat.blocks[b].offset_u4 * 8 == b * per_block * flat_u16);
        for (size_t ti = 0; ti < per_block; ti++) {
            const int j_img = (int)(ti % (1 + SHARED_SB));
            const uint16_t *ci = cpt.params.data() + (b * per_block + ti) * img_u16;
            const uint16_t *fi = flat.params.data() + (b * per_block + ti) * flat_u16;
            if (j_img > flat.blocks[b].n_models) {                        // a phantom model: zeros
                CHECK(std::all_of(ci, ci + img_u16, [](uint16_t v) { return v == 0; }));
                continue;
            }
            for (int u = 0; u < m.nk; u++) std::copy(ci + (size_t)m.a_of[u] * 512, ci + (size_t)m.a_of[u] * 512 + 512, steps.begin() + (size_t)u * 512);
            for (int i = 0; i < MT; i++) {
                const bool lin = j_img != 0;
                const auto want = row_pairs(fi, lin ? flat.klf : flat.kqf, i, lin ? flat.l_desc : flat.q_desc);
                const auto got = row_pairs(steps.data(), m.nk, i, lin ? ld : qd);
                CHECK(want.size() == (size_t)(lin ? 3 * D + 2 : 3 * D));
                CHECK(got == want);
            }
        }
    }
}

int main() {
    for (int h = 1; h <= 10; h++) check_map(h);
    CHECK(h2c_applies(37, 8) && h2c_applies(38, 8) && h2c_applies(39, 8) && !h2c_applies(40, 8) && !h2c_applies(42, 8));
    CHECK(h2c_built(37, 8) && h2c_built(39, 8) && !h2c_built(40, 8) && !h2c_built(31, 6));
    // 50 mixtures: a ragged last tile; 17 and 22 models: a block plus one, a last block of 7
    check_pack(37, 50, 17, 1u);
    check_pack(38, 32, 22, 2u);
    check_pack(39, 96, 16, 3u);
    check_pack(39, 33, 12, 4u);
    check_pack(40, 32, 16, 5u);
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("h2c checks ok\n");
    return 0;
}
