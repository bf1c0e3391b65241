// em_width_checks.cpp -- what the host code says of every row of tests/em_width_cases.py, for 256 compute units.  Reads the rows from
// the file named on the command line -- per row int32 option, dim, K, has_model, int64 n and, with has_model, the start model as
// float64 weights [K], means [K][dim], sigmas [K][dim] -- and prints one line per row:
//   option dim K n dp engine ks grid_x grid_y block n_tiles wg_mix ncb wide amp pad_waste in_range
// dp is pick_padded_dim's, the launch is plan_em_stats', ncb is emm_ncb's.  A row with a model is packed by pack_models_split as
// em.hip packs an iteration's set, and the plan is asked as train_em asks it: with mfma_ok of that layout, its contraction steps
// and its 32-mixture tiles.  Built by tests/test_em_width_cases_cpu.py with the host compiler; test infrastructure.
#include "em_plan.hpp"
#include "gmm_model.hpp"
#include "score_plan.hpp"

#include <cstdarg>
#include <cstdio>
#include <stdexcept>

namespace sr {
void fail(const char *fmt, ...) {
    char b[256];
    va_list a;
    va_start(a, fmt);
    vsnprintf(b, sizeof b, fmt, a);
    va_end(a);
    throw std::runtime_error(b);
}
// (a GMM's cached set has device buffers whose destructors name these; none is ever filled here)
bool gpu_runtime_lost() { return false; }
std::atomic<long> g_devbuf_epoch{0};
}  // namespace sr
extern "C" hipError_t hipFree(void *) { return hipSuccess; }
using namespace sr;

static bool get(FILE *f, void *p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
    FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) return 2;
    const int n_cu = 256;
    int32_t head[4];
    while (get(f, head, sizeof head)) {
        const int option = head[0], dim = head[1], K = head[2];
        int64_t n = 0;
        if (!get(f, &n, sizeof n) || dim < 1 || K < 1) return 3;
        bool in_range = false;
        int ks = 0, n_mix_tiles = 0;
        double amp = 0.0, waste = 0.0;
        if (head[3]) {
            GMM g;
            g.nr_mixtures = K;
            g.dim = dim;
            g.weights.resize(K);
            g.mean.resize((size_t)K * dim);
            g.sigma.resize((size_t)K * dim);
            if (!get(f, g.weights.data(), sizeof(double) * K) || !get(f, g.mean.data(), sizeof(double) * K * dim) ||
                !get(f, g.sigma.data(), sizeof(double) * K * dim))
                return 3;
            const PackedSplit bx3 = pack_models_split({&g}, SPLIT_BF16X3);
            in_range = mfma_ok(bx3);
            ks = bx3.ks;
            n_mix_tiles = (int)bx3.chunks.size();
            amp = bx3.amp;
            waste = bx3.pad_waste;
        }
        const int dp = pick_padded_dim(dim);
        const EmStatsPlan p = plan_em_stats(K, dim, dp, (long)n, option, in_range, ks, n_mix_tiles, n_cu);
        std::printf("%d %d %d %lld %d %d %d %d %d %d %d %d %d %d %.17g %.17g %d\n", option, dim, K, (long long)n, dp, p.engine, p.ks, p.grid_x,
                    p.grid_y, p.block, p.n_tiles, p.wg_mix, p.dp <= 40 ? emm_ncb(p.dp) : 0, (int)p.wide, amp, waste, (int)in_range);
    }
    fclose(f);
    return 0;
}
