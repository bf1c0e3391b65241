// kmeans_plan.hpp -- what the k-means start's device back end (kmeans_init.hip) decides before it launches: for a nearest-centre
// pass whether the fast search runs, which instantiations, the grids and every buffer's element count; for a Lloyd step on the
// full data the worker blocks of the reference's sums, the sort keys, every grid and every workspace buffer's element count --
// each a pure function of the shape.  The shape constants the kernels and the driver share live here, each once.
// Host-only C++17, nothing of HIP: kmeans_init.hip and kmeans_host.cpp consume it, tests/host/kmeans_checks.cpp sweeps it under
// the host sanitizers.
#pragma once

#include <cstddef>
#include <string>

namespace sr {

constexpr int KM_CH = 16;          // centres per LDS chunk
constexpr int KM_PP = 2;           // points per lane: a centre coordinate read from LDS serves both
constexpr int KM_MAX_ITER = 200;   // kmeans.cc:172, :272
constexpr int KM_BS_CHUNK = 4096;  // distances a block-sum workgroup stages through LDS at a time
// chunk records for the fast search: 16 centres per record, [d][16] doubles of -2 c, then the 16 ||c||^2; padded to whole KiB so
// that a record goes into LDS as 1 KiB LDS-DMA pieces
constexpr int km_rec_doubles(int dim_max) { return (dim_max * KM_CH + KM_CH + 127) / 128 * 128; }

constexpr int KM_FAST_MAX_DIM = 40;                // rows the fast search keeps in registers
constexpr long KM_FAST_MAX_N = (long)1 << 31;      // (exclusive) its list of undecided points holds them as int
constexpr long KM_ASSIGN_MAX_N = (long)1 << 32;    // (exclusive) at most 2^23 workgroups of KM_PP * 256 points: 2^31 threads, counted in 32 bits
constexpr int KM_MAX_CENTRES = 1 << 30;            // c_end + KM_CH - 1 and n_chunks * KM_CH stay inside an int

// One nearest-centre pass over n points of dim coordinates against centres [c_begin, c_end) of C [c_end][dim].
struct KmAssignPlan {
    std::string refusal;            // non-empty: nothing else is valid
    bool fast = false;              // the fast full search runs first, the exact kernel then takes its list
    int exact_dim_max = 0;          // kmeans_assign_kernel<16 | 40 | 64 | 128>
    int fast_dim_max = 0;           // kmeans_assign_fast_kernel<16 | 40> (0: not taken)
    unsigned grid = 0;              // of both nearest-centre kernels
    int n_chunks = 0;               // chunk records of the fast search (0: not taken)
    unsigned prep_grid = 0;         // kmeans_centre_prep_kernel
    // elements of every buffer the pass touches (the last four: 0 when the fast search is not taken)
    size_t C = 0, dist = 0, belong = 0, m2c = 0, cn_max = 0, list = 0, n_list = 0;
};
// engine: sr_set_option("kmeans_assign_engine"), 0 the fast search with the exact pass behind it, 1 the exact pass alone
KmAssignPlan plan_kmeans_assign(long n, int dim, int c_begin, int c_end, bool reset, int engine);

// One Lloyd step's cluster sums on the full data, in the reference's order: a worker block is ceil(n / concurrency) points.
struct KmLloydPlan {
    std::string refusal;
    long n = 0;
    int dim = 0, K = 0;
    long block = 0;                 // points of a worker block
    int n_blocks = 0;
    unsigned n_keys = 0;            // n_blocks * K: keys 0 .. n_keys - 1 are (block, cluster), n_keys a point without a cluster
    int end_bit = 0;                // the radix sort's: the smallest with n_keys < 2^end_bit
    size_t n_seg_elems = 0;         // n_keys * dim
    unsigned grid_block_sum = 0, grid_keys = 0, grid_segments = 0, grid_segment_sum = 0, grid_centroid = 0;
    // elements of every workspace buffer (key: each of key_in, key_out, idx_in, idx_out)
    size_t key = 0, seg = 0, csum = 0, csize = 0, bsum = 0, segsum = 0;
};
KmLloydPlan plan_lloyd_full(long n, int dim, int K, int concurrency);

}  // namespace sr
