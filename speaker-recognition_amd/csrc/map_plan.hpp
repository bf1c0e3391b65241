// map_plan.hpp -- what the batched MAP enrolment call (map_batch.hip: a set of speakers adapted from ONE UBM, every speaker the
// model and the iteration count of its single fit, bit for bit) decides before it touches the device: the route of every speaker
// (batched: its single fit would take the float64 iteration engine, em_f64.hip; single: everything else; a speaker without
// frames fails alone), the cut of the batched speakers into groups whose float64 scratch fits the bound, and per group the tile
// tables the kernels read -- as a pure function of the model's shape, the speakers' lengths, the training parameters, the bound
// and the number of compute units.  The two eligibility rules of train_em's engine choice live here so that they can be
// evaluated without a device: em_route (em_plan.cpp) calls them.
// Host-only C++17, nothing of HIP: map_batch.hip consumes it, sr_map_fit_plan hands it to tests, tests/host/map_checks.cpp runs
// it under the host sanitizers.
#pragma once

#include "../../include/pygmm_hip.h"

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace sr {

// ---- the float64 iteration engine's shapes (em_f64.hip) ----
constexpr int E64_FR = 64, E64_KB = 64, E64_THREADS = 256, E64_PER = E64_KB / 4;     // density: a thread = two frames x 16 mixtures
constexpr int E64_DFR = 128;                                                          // frames of a density workgroup
constexpr int E64_STHREADS = 512, E64_SPER = E64_KB / 8;                              // statistics: a thread = one frame x 8 mixtures
constexpr int E64_MAX_D = 64;
constexpr long E64_MAX_FRAMES = 8192, E64_MAX_CELLS = 32L << 20;                     // L: <= 256 MB

// ---- the whole-fit kernel's shapes (em_small.hip) ----
constexpr int EMF_THREADS = 1024;                 // a workgroup: 64 or 128 frames x 16 or 8 mixture groups
constexpr int EMF_MAX_K = 32, EMF_MAX_D = 40;
// the iteration's price grows with the workgroups that meet at its barriers (12 us at one, 27 at 47, 46 at 128, 16 x 13); from ~10 k
// frames on an iteration per launch costs the same (20 000 x 32 x 40: 30 ms either way)
constexpr long EMF_MAX_FRAMES = 8192;

// frames per workgroup, segments of a role's sweep, LDS bytes.  The fewer workgroups meet at the barrier the cheaper the iteration
// (~0.3 us each) and the longer a workgroup's own arithmetic: 16 x 13 on 2998 frames 26.8 us per iteration at 64 frames per workgroup,
// 19.5 at 128, 21.5 at 256 -- 128 where the LDS fits and 64 frames would not do with as few workgroups.
struct EmSmallShape {
    int fr, seg, grid;
    size_t lds;
};
EmSmallShape em_small_shape(int K, int D, long n);

// train_em's engine choice as functions of the shape alone (n_cu: compute units of the device)
bool em_small_shape_eligible(int K, int dim, long n, const Parameter &param, int n_cu);
bool em_f64_shape_eligible(int K, int dim, long n, const Parameter &param);

// LDS bytes of a density / statistics workgroup of the float64 engine at `dim` dimensions
size_t e64_density_lds(int dim);
size_t e64_stats_lds(int dim);

// ---- the batched call ----
constexpr int MAP_ROUTE_BATCHED = 0, MAP_ROUTE_SINGLE = 1, MAP_ROUTE_ERROR = -1;
constexpr int64_t MAP_DEFAULT_SCRATCH = (int64_t)1 << 30;
constexpr int MAP_STATE = 4;                      // doubles of a speaker's stop-rule state: last_ll, active, done_it, flag

// One row of a tile table: tile `local` (128 frames for the density table, 64 for the chunk table, counted from the speaker's
// own first frame) of the speaker at `slot` of its group, whose frames start at row `first` of the batch.  (The device reads
// the tables as such.)
struct MapTileRow {
    int64_t first;
    int32_t speaker;            // index in the call
    int32_t slot;               // index in the group
    int32_t local;
    int32_t pad;
};

struct MapSpeakerPlan {
    int route = MAP_ROUTE_ERROR;
    int64_t n = 0, first = 0;           // frames, first row in the batch
    int n_pad = 0, n_chunks = 0;        // train_em_f64's: frames padded to whole density tiles, 64-frame chunks of the padded range
    int64_t scratch_bytes = 0;          // float64 scratch of the speaker (0 unless batched)
    int group = -1, slot = -1;
    // offsets, in doubles, of the speaker's slices inside its group's scratch
    int64_t off_mu = 0, off_L = 0, off_mb = 0, off_sb = 0, off_llf = 0, off_partial = 0, off_llpart = 0;
};

struct MapGroupPlan {
    int first = 0, count = 0;           // the group's speakers: batched[first .. first + count)
    int64_t tile0 = 0, n_tiles = 0;     // its rows of the density table
    int64_t chunk0 = 0, n_chunks = 0;   // its rows of the chunk table
    int64_t scratch_bytes = 0;          // all of the group's speakers
    // grids: density (n_tiles, n_kb), log-sum-exp (n_chunks), statistics (n_chunks, n_kb), head (count), M-step (ceil(K D / 256), count)
};

struct MapPlan {
    int K = 0, D = 0, n_kb = 0;
    size_t lds_density = 0, lds_stats = 0;
    std::vector<MapSpeakerPlan> speakers;   // [S]
    std::vector<int> batched;               // the batched speakers in call order
    std::vector<MapGroupPlan> groups;
    std::vector<MapTileRow> tiles, chunks;  // group after group
    int64_t n_single = 0, n_error = 0;
    int64_t max_group_bytes = 0;
    int64_t waves = 0;                      // rounds the largest group's density launch makes over the chip at two workgroups a unit
};

// The float64 scratch of one batched speaker of n frames in bytes: L, the two per-block arrays, partial, llf, llpart, the
// stop-rule state and the speaker's means.
int64_t map_speaker_scratch_bytes(int K, int D, int64_t n);

// Fills `p` and returns true, or false with the reason: a shape without mixtures or dimensions, a negative length, a bound
// below 1 byte, no compute units, a table beyond the grid limits.  lengths: [S] frames per speaker.
bool plan_map_batch(int K, int D, const int64_t *lengths, int64_t S, const Parameter &param, int64_t scratch_bytes, int n_cu, MapPlan &p,
                    std::string &why);

}  // namespace sr
