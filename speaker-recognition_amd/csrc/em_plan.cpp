// em_plan.cpp -- the trainer's route and the statistics launch of an iteration (em_plan.hpp).  Host-only: no device, no allocation.
#include "em_plan.hpp"

#include <algorithm>

namespace sr {

int em_route(int K, int dim, long n, const Parameter &param, int stats_engine_option, bool side_effects, int n_cu) {
    // a speaker-sized fit: every iteration, the stop rule included, in ONE launch (em_small.hip).  Not with the reference's side
    // effects on (a model file after every second iteration) nor with the per-phase trace (verbosity >= 2, in the eligibility rules).
    if (stats_engine_option == 0 && !side_effects && em_small_shape_eligible(K, dim, n, param, n_cu)) return EM_ROUTE_WHOLE_FIT;
    // short data, a model of any size (a speaker's MAP enrolment from a large UBM): float64 iterations on the device, nothing
    // packed, nothing redone on the host (em_f64.hip)
    if (stats_engine_option == 0 && !side_effects && em_f64_shape_eligible(K, dim, n, param)) return EM_ROUTE_F64;
    return EM_ROUTE_ITERATION;
}

EmStatsPlan plan_em_stats(int K, int dim, int DP, long n, int stats_engine_option, bool split_in_range, int bx3_ks, int n_mix_tiles,
                          int n_cu) {
    EmStatsPlan p;
    p.dp = DP;
    p.n_records = (K + EM_KB - 1) / EM_KB;
    p.k_pad = p.n_records * EM_KB;
    p.rec = 2 * DP + 1;
    p.n_elem = (size_t)p.k_pad * p.rec;
    p.reduce_grid = (int)((p.n_elem + 255) / 256);
    const bool use_mfma = stats_mfma_available(DP) && stats_engine_option != 1;
    // responsibilities on the 16-bit matrix cores when the model is inside the split-bf16 layout's range -- the engine
    // score_device has just taken for the denominators (em_stats_engine = 2 keeps them on the vector ALU)
    const bool use_split = use_mfma && (stats_engine_option == 0 || stats_engine_option == 3) && split_in_range && n_mix_tiles > 0 &&
                           stats_split_available(DP, bx3_ks);
    if (use_mfma) {
        // sums about the origin in float64 slabs, one per (frame chunk, mixture range); the chunks fill the chip four times over
        const int n_ranges = use_split ? (n_mix_tiles + EMS_TILES - 1) / EMS_TILES
                                       : (p.n_records + EMM_WG_MIX / EM_KB - 1) / (EMM_WG_MIX / EM_KB);
        p.engine = use_split ? 3 : 2;
        p.ks = use_split ? bx3_ks : 0;
        p.wg_mix = use_split ? EMS_WG_MIX : EMM_WG_MIX;
        p.n_tiles = (int)((n + EMM_FT - 1) / EMM_FT);
        const int n_chunks = std::max(1, std::min(p.n_tiles, (4 * n_cu + n_ranges - 1) / n_ranges));
        p.grid_x = n_ranges;
        p.grid_y = n_chunks;
        p.block = (use_split ? EMS_WAVES : EMM_WAVES) * 64;
        p.lds_bytes = use_split ? (size_t)ems_lds_bytes(bx3_ks) : emm_lds_bytes(DP);
        p.slab_f64 = true;
        p.slab_elems = stats_mfma_slab_doubles(DP, n_ranges, n_chunks, p.wg_mix);
        return p;
    }
    p.wide = DP > EM_MAX_REG_DIM;
    p.engine = p.wide || stats_vector_available(DP) ? 1 : 0;
    p.n_tiles = (int)((n + EMV_FT - 1) / EMV_FT);
    // (wide rows: a slab is K x (2 D + 1) floats per workgroup column -- one per CU, the records cut along gridDim.y instead)
    p.grid_x = std::min(p.n_tiles, n_cu * (dim > EM_MAX_REG_DIM ? 1 : 4));
    p.grid_y = std::max(1, std::min(p.wide ? (p.n_records + EM_CB - 1) / EM_CB : p.n_records, (4 * n_cu + p.grid_x - 1) / p.grid_x));
    p.block = 256;
    p.slab_elems = (size_t)p.grid_x * p.n_elem;
    return p;
}

}  // namespace sr
