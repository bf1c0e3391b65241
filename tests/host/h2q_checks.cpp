// h2q_checks.cpp -- pairs of blocks in the compact pipelined shared-sigma kernel, on the host: the pair arithmetic of
// csrc/score_shapes.hpp (h2q_*: what the kernel indexes its stages and images with) and the premise pairing rests on -- in
// csrc/model_pack_shared.cpp's pack_h2_compact every block's quadratic-half image of a mixture tile holds the same bytes.  A stand-alone
// program, built by tests/test_h2q_host.py with g++ -fsanitize=address,undefined (host code only).
//   pairs:  for every (15, m), m = 0 .. 15 (0: a lone block), a mixture tile is walked stage by stage from h2q_stage_block /
//           h2q_stage_image and compared with the order [Q][L_0 .. L_14][L'_0 .. L'_(m-1)] written out by hand: stages, images
//           executed, index, parity and model of the last executed image, every model's image executed exactly once, the second
//           block's Q image never read, reads never further than one image behind the second block's tile
//   lone:   a lone block of m = 1 .. 15 models runs the stages it always ran: ceil((1 + m) / 4), an odd last image
//   pack:   random MAP-shaped sets at D = 37, 38, 39: image 0 of tile t is byte-identical in every block; the packed host vector
//           carries no padding
//   count:  201 models execute 210 images per mixture tile paired, 216 block by block; the issue's other set sizes
#include "gmm_model.hpp"
#include "score_shapes.hpp"

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
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
bool gpu_runtime_lost() { return false; }
std::atomic<long> g_devbuf_epoch{0};
}  // namespace sr
extern "C" hipError_t hipFree(void *) { return hipSuccess; }

using namespace sr;

static int failures = 0;
#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            failures++;                                                           \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
        }                                                                         \
    } while (0)

constexpr int SB = SHARED_SB, G = H2Q_G;
static_assert(SB == H2Q_SB, "the pair arithmetic is written for the set's block size");

static void check_pair(int m2) {
    const int m1 = SB;
    // by hand: images 0 = Q, 1 .. 15 = the first block's models, 16 .. 15 + m2 the second's; whole stages of four, a full pair one short
    const int n_real = 1 + m1 + m2;
    const int stages = (n_real + G - 1) / G;
    const int executed = std::min(stages * G, 1 + 2 * SB);
    CHECK(h2q_pairs(SB, m1, m2) == (m2 > 0));
    CHECK(h2q_stages(G, m1, m2) == stages);
    CHECK(h2q_images(SB, G, m1, m2) == executed);
    CHECK(h2q_last_image(SB, G, m1, m2) == executed - 1);
    CHECK(h2q_last_parity(SB, G, m1, m2) == ((executed - 1) & 1));
    CHECK(h2q_last_model(SB, G, m1, m2) == executed - 2);
    if (m2 >= SB - 2) CHECK(executed == 31 && h2q_last_parity(SB, G, m1, m2) == 0);      // the full pair's last stage: image 30, even
    else CHECK(executed == stages * G && h2q_last_parity(SB, G, m1, m2) == 1);           // whole stages: an odd last image
    // the issue's formula for the second block's model that is summed apart
    if (m2 > 0) CHECK(h2q_last_model(SB, G, m1, m2) - SB == std::min(31, 4 * ((16 + m2 + 3) / 4)) - 17);
    // walk the tile: pair image p comes from stage p / G, slot p % G
    std::vector<int> seen_first(1 + SB, 0), seen_second(1 + SB + 1, 0);
    for (int p = 0; p < executed; p++) {
        const int s = p / G, blk = h2q_stage_block(SB, G, s), img = h2q_stage_image(SB, G, s) + p % G;
        CHECK(blk == (p <= SB ? 0 : 1));
        if (blk == 0) {
            CHECK(img == p && img <= SB);
            seen_first[img]++;
        } else {
            CHECK(m2 > 0);
            CHECK(img == p - SB && img >= 1 && img <= SB);       // model p - 16 of the second block is its image p - 15
            seen_second[img]++;
        }
    }
    for (int i = 0; i <= SB; i++) CHECK(seen_first[i] == 1);                         // Q and the first block's 15 images, once each
    CHECK(seen_second[0] == 0);                                                       // the second block's own Q image is never read
    for (int i = 1; i <= SB; i++) CHECK(seen_second[i] == (i <= m2 ? 1 : seen_second[i]) && seen_second[i] <= 1);
    // what the stages LOAD: four images each, the second block's last stage one image behind its tile and no further
    for (int s = 0; s < stages; s++) {
        const int first = h2q_stage_image(SB, G, s), last = first + G - 1;
        if (h2q_stage_block(SB, G, s) == 0) CHECK(first >= 0 && last <= SB);
        else CHECK(first >= 1 && last <= SB + 1 && (last <= SB || s == 2 * (1 + SB) / G - 1));
    }
}

static void check_lone(int m) {
    const int stages = (1 + m + G - 1) / G;
    CHECK(!h2q_pairs(SB, m, 0));
    CHECK(h2q_stages(G, m, 0) == stages && h2q_images(SB, G, m, 0) == stages * G);
    CHECK(h2q_last_parity(SB, G, m, 0) == 1 && h2q_last_model(SB, G, m, 0) == stages * G - 2);
    for (int s = 0; s < stages; s++) CHECK(h2q_stage_block(SB, G, s) == 0 && h2q_stage_image(SB, G, s) == s * G);
    if (m < SB) CHECK(!h2q_pairs(SB, m, 3));             // a short block never leads a pair
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

static void check_q_images(int D, int K, int S, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<GMM> store;
    store.reserve(S);
    store.push_back(make_gmm(K, D, rng, nullptr));
    for (int s = 1; s < S; s++) store.push_back(make_gmm(K, D, rng, &store[0]));
    std::vector<const GMM *> models;
    for (const GMM &g : store) models.push_back(&g);
    const PackedH2Shared flat = pack_models_h2_shared(models);
    const PackedH2Compact cpt = pack_h2_compact(flat, D);
    CHECK(h2c_built(D, flat.klf) && cpt.nf > 0);
    if (cpt.nf <= 0) return;
    const size_t img_u16 = (size_t)cpt.nf * 512;
    const size_t per_block = (size_t)flat.n_tiles * (1 + SB);
    const size_t n_blocks = cpt.blocks.size();
    CHECK(n_blocks == (size_t)(S + SB - 1) / SB && n_blocks >= 2);
    CHECK(cpt.params.size() == n_blocks * per_block * img_u16);          // the host vector is not padded (the device buffer is)
    bool any = false;
    for (size_t b = 0; b < n_blocks; b++) {
        CHECK((size_t)cpt.blocks[b].offset_u4 * 8 == b * per_block * img_u16);      // blocks lie end to end
        for (int t = 0; t < flat.n_tiles; t++) {
            const uint16_t *q0 = cpt.params.data() + ((size_t)t * (1 + SB)) * img_u16;
            const uint16_t *qb = cpt.params.data() + (b * per_block + (size_t)t * (1 + SB)) * img_u16;
            CHECK(std::memcmp(q0, qb, img_u16 * sizeof(uint16_t)) == 0);
            any = any || std::any_of(q0, q0 + img_u16, [](uint16_t v) { return v != 0; });
        }
    }
    CHECK(any);                                                            // (not identical for being empty)
}

int main() {
    for (int m2 = 0; m2 <= SB; m2++) check_pair(m2);
    for (int m = 1; m <= SB; m++) check_lone(m);
    // images executed per mixture tile: BASELINE configs[2]'s 201 models, and the GPU test's set sizes
    CHECK(h2q_group_images(SB, G, 201, false) == 216);
    const int paired201 = h2q_group_images(SB, G, 201, true);
    CHECK(paired201 == 210 || paired201 == 208);
    CHECK(h2q_group_images(SB, G, 16, true) == 20 && h2q_group_images(SB, G, 16, false) == 16 + 4);
    CHECK(h2q_group_images(SB, G, 30, true) == 31 && h2q_group_images(SB, G, 30, false) == 32);
    CHECK(h2q_group_images(SB, G, 31, true) == 31 + 4);
    CHECK(h2q_group_images(SB, G, 37, true) == 31 + 8);
    CHECK(h2q_group_images(SB, G, 45, true) == 31 + 16);
    CHECK(h2q_group_images(SB, G, 52, true) == 31 + 24 && h2q_group_images(SB, G, 52, false) == 48 + 8);
    // 50 mixtures: a ragged last tile; 96: three tiles; two, three and four blocks, the last one partial or full
    check_q_images(37, 50, 31, 11u);
    check_q_images(38, 96, 37, 12u);
    check_q_images(39, 96, 52, 13u);
    check_q_images(39, 32, 30, 14u);
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("h2q checks ok\n");
    return 0;
}
