"""The fits of tests/test_gpu_em_parent_bits.py and of its recorder (tests/golden/make_em_parent_bits.py): the smallest shapes
that reach every branch of the iteration-at-a-time trainer (csrc/em.hip: the three statistics engines, the wide rows, the set pool
with the carried set and the stop rule, the float64 redo of unsupported mixtures, a MAP fit's first E-step on the UBM handle's own
set), each a few milliseconds, all from fixed parameters (init_with_kmeans = -1 / a UBM).  The data come from an integer hash, not
from a library's generator or libm: the same bits under any numpy."""
import numpy as np

MAX_REG_DIM = 96                          # csrc/gmm_model.hpp: wider rows take em_stats_wide_kernel
_M = (1 << 64) - 1


def _uniform(seed, count):
    """count values k / 2^24, k the top 24 bits of splitmix64(seed, index): exact in float64"""
    z = (np.arange(1, count + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64((seed * 0xD1342543DE82EF95) & _M))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float64) / float(1 << 24)


def noise(seed, shape):
    """roughly normal, unit variance: the sum of four uniforms, centred (sums of 24-bit fractions: exact)"""
    n = int(np.prod(shape))
    u = _uniform(seed, 4 * n).reshape(4, n)
    return ((u[0] + u[1] + u[2] + u[3] - 2.0) * np.sqrt(3.0)).reshape(shape)


def _em_case(seed, K, D, n):
    """frames around K centres, the start a fifth of a sigma off them"""
    cent = 2.0 * noise(seed, (K, D))
    own = (np.arange(n) * 7 + seed) % K
    X = (cent[own] + 0.9 * noise(seed + 1, (n, D))).astype(np.float32)
    start = (np.full(K, 1.0 / K), cent + 0.2 * noise(seed + 2, (K, D)), np.full((K, D), 0.9))
    return X, start


def _map_far_case(seed, K, D, n, n_far):
    """a UBM of K mixtures 3 units apart per dimension (tens of sigmas in D = 39: a frame's responsibility for any mixture but
    its own is below fp32's range and above float64's), frames around the first eight; the last n_far frames 1000 units away"""
    cent = 3.0 * noise(seed, (K, D))
    own = (np.arange(n) * 5 + seed) % 8
    X = cent[own] + 0.9 * noise(seed + 1, (n, D))
    X[n - n_far:] += 1000.0
    return X.astype(np.float32), (np.full(K, 1.0 / K), cent, np.full((K, D), 0.9))


def _map_pair_case(seed, K, D, n_a, n_b):
    cent = 2.0 * noise(seed, (K, D))
    ubm = (np.full(K, 1.0 / K), cent, np.full((K, D), 0.9))
    Xs = []
    for j, n in enumerate((n_a, n_b)):
        own = (np.arange(n) * 3 + j) % K
        Xs.append((cent[own] + 0.3 * (j + 1) + 0.9 * noise(seed + 1 + j, (n, D))).astype(np.float32))
    return Xs, ubm


# name, em_stats_engine option, kind, arguments, iterations, threshold, min_covar, the engine sr_last_em_stats_engine() must report.
# The option-3 fits floor the variances at 0.5: with a handful of frames per mixture the default floor lets them collapse, the model
# leaves the split-bf16 layout's range (sum (mu / sigma)^2 <= 2000) and the trainer falls back to the fp64 matrix-core form.
# The stop rule (gmm.cc:643-650) asks for |ll - last_ll| / |ll| < threshold AND ll - last_ll < threshold: 1e6 is never met by the
# first check (last_ll = -DBL_MAX) and always by the second, after iteration 3 of 0..5.
CASES = (
    ("vector_k5_d13", 1, "em", (11, 5, 13, 300), 3, 0.0, 1e-3, 1),
    ("wide_k9_d97", 1, "em", (12, 9, MAX_REG_DIM + 1, 257), 3, 0.0, 1e-3, 1),
    ("mfma_k17_d26", 2, "em", (13, 17, 26, 129), 3, 0.0, 1e-3, 2),                 # one frame past a 128-frame tile
    ("split_k56_d13", 3, "em", (14, 56, 13, 333), 3, 0.0, 0.5, 3),
    ("split_k160_d39", 3, "em", (15, 160, 39, 130), 3, 0.0, 0.5, 3),              # 5 mixture tiles: the last workgroup has one live
    ("split_stop_k56_d13", 3, "em", (16, 56, 13, 333), 6, 1e6, 0.5, 3),
    ("map_far_k64_d39", 3, "map_far", (17, 64, 39, 70, 5), 2, 0.0, 1e-3, None),   # unsupported mixtures: the float64 redo on the host
    ("map_pair_k40_d13", 2, "map_pair", (18, 40, 13, 200, 150), 2, 0.0, 1e-3, 2), # two speakers of one UBM handle: its own set serves both
)


def unsupported(X, ubm):
    """mixtures whose float64 occupancy under the UBM is below the trainer's 1e-25 (and not an exact 0), over the frames near it"""
    w, mu, sg = ubm
    near = np.abs(X).max(axis=1) < 500.0
    lp = np.log(w)[None, :] - 0.5 * (((X[near, None, :].astype(np.float64) - mu[None]) / sg[None]) ** 2).sum(axis=2)
    g = np.exp(lp - lp.max(axis=1, keepdims=True))
    Nk = (g / g.sum(axis=1, keepdims=True)).sum(axis=0)
    return int(np.sum((Nk < 1e-25) & (Nk > 0)))


def run_case(case):
    """-> {suffix: array} of one case: iteration count(s), engine(s), weights, means, sigmas (float64)"""
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.pygmm import GMM
    name, opt, kind, args, iters, threshold, min_covar, _eng = case
    out = {}
    _lib.set_option("em_stats_engine", opt)
    try:
        if kind == "em":
            X, start = _em_case(*args)
            g = GMM.from_arrays(*start)
            g.nr_iteration, g.init_with_kmeans, g.threshold, g.min_covar = iters, -1, threshold, min_covar
            fits = [(g, g.fit(X), _lib.last_em_stats_engine())]
        else:
            if kind == "map_far":
                X, ubm = _map_far_case(*args)
                Xs = [X]
            else:
                Xs, ubm = _map_pair_case(*args)
            u = GMM.from_arrays(*ubm)
            fits = []
            for X in Xs:
                g = GMM(ubm[1].shape[0], nr_iteration=iters, threshold=threshold, min_covar=min_covar)
                it = g.fit(X, ubm=u)
                fits.append((g, it, _lib.last_em_stats_engine()))
        out["iterations"] = np.array([f[1] for f in fits], np.int64)
        out["engine"] = np.array([f[2] for f in fits], np.int64)
        for j, (g, _it, _e) in enumerate(fits):
            w, mu, sg = g.params()
            out["w%d" % j], out["mean%d" % j], out["sigma%d" % j] = w, mu, sg
    finally:
        _lib.set_option("em_stats_engine", 0)
    return out
