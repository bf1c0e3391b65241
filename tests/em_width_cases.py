"""The diagonal statistics kernels at every padded row width they are built for: the table behind tests/test_gpu_em_widths.py and
tests/test_gpu_bw_widths.py (the device against the float64 oracles) and tests/test_em_width_cases_cpu.py (the table's own
conditions, without a GPU).

csrc/em.hip builds em_stats_kernel<DP> for 14 widths (wider rows: em_stats_wide_kernel, slices of 64 dimensions),
em_stats_mfma_kernel<DP> / em_reduce64_kernel<DP> for 9 and em_stats_split_kernel<DP, KS> for 12 (DP, KS) pairs; csrc/bw_stats.hip
builds bw_stats_kernel<DP> for 9.  The column indexing is different code at every width, so every instantiation gets its SMALLEST
dim (the previous width + 1: DP != dim, the zero-filled padding rows are live) and its LARGEST (dim == DP).  Everything here is
computed from the lists below, which tests/test_em_width_cases_cpu.py holds against the sources' own.

Pure Python + numpy: nothing of the package is imported here."""
import math
from collections import namedtuple

import numpy as np

# ---- the built widths, restated (the CPU test reads the sources' lists as text and compares) ----
KDIMS = [8, 13, 16, 24, 26, 32, 34, 39, 40, 48, 56, 64, 80, 96]          # model_pack.cpp: pick_padded_dim; SR_EM_VECTOR_DPS
MFMA_DPS = [8, 13, 16, 24, 26, 32, 34, 39, 40]                           # SR_EM_MFMA_DPS; SR_BW_DIMS
SPLIT_SHAPES = [(8, 1), (8, 2), (13, 2), (16, 2), (16, 3), (24, 3), (24, 4), (26, 4), (32, 4), (32, 5), (34, 5), (39, 5)]
WIDE_DC = 64                                                             # model_pack.hpp: slices of the wide kernels
WIDE_DIMS = [97, 128, 129]        # padded to 128 with the second slice half empty; whole slices; padded to 192

# the project's gates on one EM iteration (tests/test_gpu_pipeline.py::test_em_statistics_engines_vs_oracle)
GATE_W, GATE_MU, GATE_SG = 1e-5, 1e-4, 1e-3          # weights and means absolute, sigmas relative
ENGINES_AGREE = 2e-5                                 # engines 2 and 3: means absolute, sigmas relative
NO_WORSE = 1e-6                                      # engine 2 at least as close to the oracle as engine 1, within this
MIN_OCCUPANCY = 2.0                                  # frames of every mixture after the iteration
SWAP_MARGIN = 100.0                                  # neighbouring dimensions differ by this many gates
MFMA_MAX_AMP, MFMA_MAX_PAD_WASTE = 2000.0, 0.25      # score_plan.hpp: the split-bf16 layout's range


def padded(dim):
    """pick_padded_dim"""
    for d in KDIMS:
        if d >= dim:
            return d
    return -(-dim // WIDE_DC) * WIDE_DC


def ks_of(dim):
    """contraction steps of the split-bf16 layout: 8 slots a step, one of them the constant's"""
    return (dim + 8) // 8


def emm_ncb(dp):
    """16-column blocks of a mixture's 2 DP + 1 sums on the matrix cores: [x][x^2][the rest of x, of x^2, the count]"""
    return 2 * (dp // 16) + (2 * (dp % 16) + 1 + 15) // 16


def _ends(dims):
    return sorted(set([min(dims), max(dims)]))


# width -> its smallest and its largest dim
VECTOR_DIMS = {dp: _ends([d for d in range(1, KDIMS[-1] + 1) if padded(d) == dp]) for dp in KDIMS}
MFMA_DIMS = {dp: VECTOR_DIMS[dp] for dp in MFMA_DPS}
SPLIT_DIMS = {(dp, ks): _ends([d for d in range(1, MFMA_DPS[-1] + 1) if (padded(d), ks_of(d)) == (dp, ks)]) for dp, ks in SPLIT_SHAPES}
ENGINE1_DIMS = sorted(d for ds in VECTOR_DIMS.values() for d in ds)
ENGINE2_DIMS = sorted(d for ds in MFMA_DIMS.values() for d in ds)

# ---- the shapes ----
# K = 70: 18 records, the last with two dead mixtures; for the matrix-core kernel two workgroups of 64 mixtures, the second with 6 live
# ones and dead records behind them.  n = 300: two full 128-frame tiles and 44 frames, or one full 256-frame tile and 44.
BASE_K, BASE_N = 70, 300
# The split layout is offered only while at most a quarter of its 32-mixture tiles is padding (MFMA_MAX_PAD_WASTE): 70 mixtures in
# three tiles waste 27 %, and the plan would hand the row to engine 2.  73 is the smallest K inside the range that keeps what the
# base shape is for: three tiles in one workgroup, the last partly live (9 mixtures), a last record with dead mixtures (3 of 4).
SPLIT_K = 73
# at the largest dim of every width: one workgroup, mostly dead -- K = 5 for engine 2; the split layout's range starts at 24 of a
# tile's 32 (24 live of the workgroup's 128) -- and a last workgroup with one mixture (engine 2: 129) or one live tile (engine 3: 160)
FEW_K = {2: 5, 3: 24}
MANY_K = {2: 129, 3: 160}
FEW_N, MANY_N = 300, 600

Row = namedtuple("Row", "option engine dim K n kind")     # option: em_stats_engine as forced; engine: what the plan must report


def width_of(row):
    """the instantiation a row runs: DP, (DP, KS), or "wide\""""
    dp = padded(row.dim)
    if row.engine == 3:
        return (dp, ks_of(row.dim))
    return "wide" if dp > KDIMS[-1] else dp


def width_id(engine, width):
    return "e%d-%s" % (engine, "x".join(str(v) for v in width) if isinstance(width, tuple) else width)


def rows():
    """every short row of the table, in (engine, width) order"""
    out = []
    for dp in KDIMS:
        out += [Row(1, 1, d, BASE_K, BASE_N, "em") for d in VECTOR_DIMS[dp]]
    out += [Row(1, 1, d, BASE_K, BASE_N, "em") for d in WIDE_DIMS]
    for dp in MFMA_DPS:
        out += [Row(2, 2, d, BASE_K, BASE_N, "em") for d in MFMA_DIMS[dp]]
        D = MFMA_DIMS[dp][-1]
        out += [Row(2, 2, D, FEW_K[2], FEW_N, "em"), Row(2, 2, D, MANY_K[2], MANY_N, "em"), Row(2, 2, D, BASE_K, BASE_N, "map")]
    for shape in SPLIT_SHAPES:
        out += [Row(3, 3, d, SPLIT_K, BASE_N, "em") for d in SPLIT_DIMS[shape]]
        D = SPLIT_DIMS[shape][-1]
        out += [Row(3, 3, D, FEW_K[3], FEW_N, "em"), Row(3, 3, D, MANY_K[3], MANY_N, "em"), Row(3, 3, D, SPLIT_K, BASE_N, "map")]
    # there is no (40, 6): option 3 at D = 40 is engine 2's
    out.append(Row(3, 2, 40, SPLIT_K, BASE_N, "em"))
    return out


def twin_rows():
    """engine 2 on the engine-3 row of the largest dim of every split shape: what the two engines are compared on"""
    return [Row(2, 2, SPLIT_DIMS[s][-1], SPLIT_K, BASE_N, "em") for s in SPLIT_SHAPES]


# ---- long rows: chosen from plan_em_stats for 256 compute units (the CPU test asserts what each is for) ----
# D = 13: two mixed blocks; D = 32: REM = 0.
# Engines 2 and 3 cut the frames into n_chunks = min(n_tiles, ceil(4 n_cu / n_ranges)) chunks of ceil(n_tiles / n_chunks) tiles.
#   engine 2, K = 512: 8 ranges of 64 mixtures, 128 chunks; 129 tiles -> 2 tiles a chunk, 65 chunks with frames, the last with ONE
#     tile (of 45 frames), 63 chunks without a tile (their slabs are zeros the reduction adds)
#   engine 3, K = 512: 4 ranges of 128 mixtures, 256 chunks; 257 tiles -> the same picture at twice the frames
# Engine 1 cuts the records along gridDim.y = min(n_records, ceil(4 n_cu / grid_x)):
#   K = 68 (17 records), 64 tiles of 256 frames: gridDim.y = 16, 2 records a workgroup, 9 with records (the last with one), 7 return
#   K = 8, 1025 tiles: gridDim.x = 1024, workgroup 0 walks tiles 0 and 1024 (the tile loop's stride)
LONG_ROWS = [Row(2, 2, 13, 512, 128 * 128 + 45, "em"), Row(2, 2, 32, 512, 128 * 128 + 45, "em"),
             Row(3, 3, 13, 512, 2 * 128 * 128 + 45, "em"), Row(3, 3, 32, 512, 2 * 128 * 128 + 45, "em"),
             Row(1, 1, 13, 68, 64 * 256 - 100, "em"), Row(1, 1, 32, 68, 64 * 256 - 100, "em"),
             Row(1, 1, 13, 8, 1024 * 256 + 30, "em")]


def group_of(row):
    if row.option != row.engine:
        return "e%d-D%d-is-e%d" % (row.option, row.dim, row.engine)
    return width_id(row.engine, width_of(row))


def groups():
    """[(id, [rows])]: the short rows per (engine, width), then every long row on its own"""
    out = {}
    for r in rows():
        out.setdefault(group_of(r), []).append(r)
    return list(out.items()) + [("long-e%d-D%d-K%d" % (r.engine, r.dim, r.K), [r]) for r in LONG_ROWS]


# ---- the data ----
# Frame t belongs to cluster t % K, so every mixture has frames.  A cluster's centre in dimension d is one of K values spread
# evenly over +- A_d around an offset of its own, in an order drawn per dimension: the centres differ from dimension to dimension in
# every mixture.  The frames' spread is 0.5, 0.8, 0.65, 0.5, ... along d: neighbouring dimensions never share it.
# A_d = 0.8 A or 1.2 A with A = 2 sqrt(3): centres about 3 with a spread of 2, sigma 0.9 at the start -- the recipe of
# tests/test_gpu_pipeline.py::test_em_responsibilities_on_the_matrix_cores_vs_oracle, which the gate between engines 2 and 3 was set
# at: the split-bf16 layout's log2 densities carry an error that grows with amp = max_k sum_d ((mu - centre) / sigma)^2 (about 300
# here at D = 39, 2000 the layout's bound), and with four frames a mixture nothing averages it out.  Below D = 17 up to 160 clusters
# need more room to keep two frames each: A = 28 / D^0.75 there (D = 1: 70 clusters on a line of +- 28).
SPREAD = (0.5, 0.8, 0.65)
START_SIGMA = 0.9


def centre_half_width(dim):
    return max(2.0 * math.sqrt(3.0), 28.0 / dim ** 0.75)

_DATA = {}


def make_data(dim, K, n):
    """(cent [K, dim], X [n, dim] float32, start (weights, means, sigmas)) -- made once, read-only"""
    key = (dim, K, n)
    if key not in _DATA:
        rng = np.random.default_rng(100003 * dim + 101 * K + n)
        A = centre_half_width(dim)
        u = (2.0 * np.arange(K) + 1.0) / K - 1.0
        cent = np.empty((K, dim))
        for d in range(dim):
            cent[:, d] = 3.0 + 0.5 * ((3 * d) % 7 - 3) + A * (1.2 if d % 2 else 0.8) * u[rng.permutation(K)]
        spread = np.array([SPREAD[d % 3] for d in range(dim)])
        X = (cent[np.arange(n) % K] + spread * rng.standard_normal((n, dim))).astype(np.float32)
        r6 = np.vectorize(lambda v: float("%g" % v))
        start = (np.full(K, 1.0 / K), r6(cent + 0.2 * rng.standard_normal(cent.shape)), np.full((K, dim), START_SIGMA))
        for a in (cent, X) + start:
            a.setflags(write=False)
        _DATA[key] = (cent, X, start)
    return _DATA[key]


_WANT = {}


def oracle_iteration(go, row):
    """the float64 oracle's parameters after the row's iteration (EM, or means-only MAP at relevance 16 from the start as UBM) and
    every mixture's occupancy sum_t gamma_k(t) -- made once, read-only"""
    key = (row.dim, row.K, row.n, row.kind)
    if key not in _WANT:
        _, X, start = make_data(row.dim, row.K, row.n)
        p = go.GMMParams(*start)
        X64 = X.astype(np.float64)
        if row.kind == "map":
            want = go.em_iteration(p, X64, map_relevance=16.0, ubm=p)
            occ = oracle_iteration(go, row._replace(kind="em"))[3]
        else:
            want = go.em_iteration(p, X64)
            occ = want.weights * row.n             # (no frame underflows here: the weights are N_k / n)
        res = (np.asarray(want.weights), np.asarray(want.mean), np.asarray(want.sigma), np.asarray(occ))
        for a in res:
            a.setflags(write=False)
        _WANT[key] = res
    return _WANT[key]


def swap_margins(mean, sigma):
    """how far a swap of two neighbouring dimensions moves the answer, in gates: for every pair (d, d + 1) the largest move of
    any mixture, and of those the smallest -- (means, sigmas); inf for a single dimension"""
    if mean.shape[1] < 2:
        return math.inf, math.inf
    dm = np.max(np.abs(mean[:, 1:] - mean[:, :-1]), axis=0) / GATE_MU
    ds = np.max(np.abs(sigma[:, 1:] - sigma[:, :-1]) / np.minimum(sigma[:, 1:], sigma[:, :-1]), axis=0) / GATE_SG
    return float(dm.min()), float(ds.min())


def errors(got, want):
    """(weights, means, sigmas) of a fit against the oracle's, each in its gate's units"""
    w, mu, sg = got
    return (float(np.max(np.abs(w - want[0]))) / GATE_W, float(np.max(np.abs(mu - want[1]))) / GATE_MU,
            float(np.max(np.abs(sg - want[2]) / want[2])) / GATE_SG)


# ---- Baum-Welch: the recipe of tests/test_gpu_bw_stats.py::test_parity_ragged_batches at the widths it has not run ----
# (it runs D = 1, 13, 39, 40: DP 8, 13, 39, 40).  Every other width's smallest and largest dim, and D = 8 and 14: DP 8's largest,
# DP 16's smallest.
BW_DIMS = [8, 9, 14, 16, 17, 24, 25, 26, 27, 32, 33, 34, 35]
BW_KS = [17, 64, 65, 256]
BW_R = 128
BW_RAGGED = (0, 1, 3, 63, 64, 65, BW_R - 1, BW_R, BW_R + 1, 2 * BW_R + 3)
BW_LONG_DIMS = [16, 24, 32]          # the default range length also: an utterance of 1100 frames in front of the ragged ones
BW_LONG_K, BW_LONG_T = 65, 1100
BW_RESIDENT_DIMS = [16, 34]
# The model's seed is that test's 100 K + D; at three rows a mixture of the 256 has two neighbouring dimensions of F closer than 100
# F gates in every utterance (16, 61 and 65 gates), and the seed moves on by 100000 until none has
BW_SEED_STEPS = {(256, 26): 1, (256, 32): 2, (256, 33): 6}


def bw_ubm_seed(K, D):
    return 100 * K + D + 100000 * BW_SEED_STEPS.get((K, D), 0)


def bw_case(bc, K, D):
    """(ubm, utterances) of a ragged row, as test_parity_ragged_batches draws them"""
    ubm = bc.make_ubm(K, D, bw_ubm_seed(K, D))
    return ubm, [bc.draw(ubm, T, 7 * K + D + i) for i, T in enumerate(BW_RAGGED)]


def bw_long_case(bc, D):
    ubm = bc.make_ubm(BW_LONG_K, D, bw_ubm_seed(BW_LONG_K, D) + 1)
    return ubm, [bc.draw(ubm, T, 900 + D + i) for i, T in enumerate((BW_LONG_T,) + BW_RAGGED)]


def bw_swap_margin(want, K, D):
    """F gates by which neighbouring dimensions of a mixture's F differ: per (mixture, pair of dimensions) the largest over the
    utterances, and of those the smallest"""
    Nw, Fw = want[0], want[1].reshape(want[0].shape[0], K, D)
    r = np.abs(Fw[:, :, 1:] - Fw[:, :, :-1]) / (1e-4 * np.maximum(Nw, 1.0))[:, :, None]
    return float(np.min(np.max(r, axis=0)))
