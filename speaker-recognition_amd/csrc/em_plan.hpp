// em_plan.hpp -- what train_em (em.hip) decides before it touches the device: which trainer takes the fit (the whole-fit kernel,
// the float64 iteration engine, or an iteration per launch) and, for an iteration per launch, which statistics engine runs on
// which grid with which slabs -- as pure functions of the shape, the option, what the packed set says about itself and the
// number of compute units.  Host-only C++17, nothing of HIP: em.hip consumes it, tests/host/em_checks.cpp sweeps it under the
// host sanitizers.
#pragma once

#include "em_shapes.hpp"
#include "map_plan.hpp"

namespace sr {

constexpr int EM_ROUTE_ITERATION = 0, EM_ROUTE_WHOLE_FIT = 1, EM_ROUTE_F64 = 2;
// stats_engine_option: sr_set_option("em_stats_engine"); side_effects: the reference's model dump after every second iteration is
// on (the iteration path's alone).  A fit the whole-fit kernel is eligible for and hands back goes on an iteration per launch,
// not to the float64 engine: the caller's `else if`.
int em_route(int K, int dim, long n, const Parameter &param, int stats_engine_option, bool side_effects, int n_cu);

struct EmStatsPlan {
    int engine = 0;             // 1 vector ALU, 2 fp64 matrix cores, 3 responsibilities on the 16-bit ones; 0: no kernel built for dp
    bool wide = false;          // dp > MAX_REG_DIM: em_stats_wide_kernel
    int dp = 0, ks = 0;         // padded dim; contraction steps of the split-bf16 layout (engine 3)
    int n_records = 0, k_pad = 0, rec = 0;
    size_t n_elem = 0;          // k_pad * rec: the sums of an iteration
    int grid_x = 1, grid_y = 1, block = 256;
    int n_tiles = 0;            // frame tiles handed to the kernel: of 256 frames (engine 1) or 128
    size_t lds_bytes = 0;       // dynamic LDS of the launch
    size_t slab_elems = 0;      // doubles (slab_f64) or floats
    bool slab_f64 = false;
    int reduce_grid = 1, wg_mix = 0;    // the reduce kernel's workgroups of 256; mixtures per range of the float64 slabs
};
// split_in_range, bx3_ks, n_mix_tiles: the set's split-bf16 layout -- inside the range of the 16-bit engine, its contraction
// steps, its 32-mixture tiles (0 where the set carries none)
EmStatsPlan plan_em_stats(int K, int dim, int DP, long n, int stats_engine_option, bool split_in_range, int bx3_ks, int n_mix_tiles,
                          int n_cu);

}  // namespace sr
