"""Cases and data for the float64 full-covariance EM kernels (csrc/gmm_full_fit.hip: the fe_* kernels behind fe_fit_group), shared by
tests/test_fullfit_cases_cpu.py, tests/test_gpu_fullfit_cases.py and the recorder tests/golden/make_fullfit_edge_golden.py.
Plain module (as tests/mfcc_cases.py, tests/em_parent_cases.py).  Every row is the smallest shape that reaches the edge it names:

  * pair slots: fe_cov gives a thread the upper-triangle pairs threadIdx.x + 256 q, q < FE_PQ = 9; a fit at width D uses
    slots(D) = ceil(D (D + 1) / 2 / 256) of them, and the rows bracket every count 1..9;
  * frame counts around FE_FB = FE_CB = 32, around the 256-frame blocks (log-sum-exp, block sums, the chunk count
    min(32, ceil(n / 256))), and past 8192, where the chunk count is pinned at 32 and a chunk stops being a multiple of 32;
  * K at 1, 64 | 65 (fe_derive's block of 64), n = K, n < D;
  * a component that receives no responsibility, frames far from the origin, and the default stop rule.

Nothing here comes from a library's random generator: the frames are sums of splitmix64 fractions (em_parent_cases.noise) shaped by
elementwise arithmetic only (no BLAS, whose summation order is a build's own), rounded to the 1/256 grid, so they are the same bits
anywhere and exact in float64 and fp32.  The start is tests/golden/make_fullcov_golden.init_params': uniform weights, K distinct
frames as means, the inverse data covariance (+ 0.1 I) as every precision -- rounded to float32 here, so that the start does not
hang on the last bits of a LAPACK build either.
"""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import numpy as np

import fullcov_oracle as fo
from em_parent_cases import noise

# kind: "plain"; "empty" (the last starting mean at +1000 in every coordinate, identity precisions: no frame gives that
# component any responsibility); "shift" (every frame + 100 per coordinate).  cov: the recorder keeps the final covariances.
Case = namedtuple("Case", "name K D n seed reg tol max_iter kind cov spread edge")


def _c(name, K, D, n, seed, edge, reg=1e-6, tol=0.0, max_iter=3, kind="plain", cov=True, spread=2.0):
    return Case(name, K, D, n, seed, reg, tol, max_iter, kind, cov, spread, edge)


def slots(D):
    """covariance pair slots a width uses: pairs D (D + 1) / 2 over 256 threads (full_plan.hpp: 9 x 256 >= 64 x 65 / 2)"""
    return (D * (D + 1) // 2 + 255) // 256


# Most of the frame-count series and the stop-rule rows keep no final covariances in the fixture (cov=False): at D = 64 a row's
# two triangles are 33 KB of incompressible float64, the series alone would take 330 KB, and every row together 730 KB of the
# fixture's 512 KiB.  The two rows of the series whose step tails fall inside the data (n = 257, n = 8193) keep theirs.  What the
# recorder keeps for the others instead is scikit-learn's score(X) of the fitted model, one number that every element of the
# final covariances enters; their covariances of iterations 1 and 2 are in the recorded weights, means and bound as for any row.
CASES = (
    # ---- pair slots: every count 1..9, and both sides of 256 (D 22 | 23), 1536 (D 55) and 2048 (D 63 | 64) pairs
    _c("slots1_d22", 2, 22, 300, 101, "253 pairs: slot 0 only, three threads idle"),
    _c("slots2_d23", 3, 23, 301, 102, "276 pairs: slot 1 holds 20 live threads"),
    _c("slots3_d32", 2, 32, 300, 103, "528 pairs; the scoring kernels' boundary width"),
    _c("slots4_d39", 3, 39, 299, 104, "780 pairs: the widest fit the suite had"),
    _c("slots5_d45", 2, 45, 300, 105, "1035 pairs: the first width with the guard rem >= npairs live in slot 4"),
    _c("slots5_d50", 3, 50, 303, 106, "1275 pairs: slot 4 nearly full"),
    _c("slots6_d51", 2, 51, 300, 107, "1326 pairs: slot 5 opens"),
    _c("slots7_d55", 3, 55, 330, 108, "1540 pairs: four past 1536, slot 6 holds 4 live threads"),
    _c("slots7_d59", 2, 59, 300, 109, "1770 pairs: slot 6 nearly full"),
    _c("slots8_d60", 3, 60, 360, 110, "1830 pairs: slot 7 opens"),
    _c("slots8_d63", 2, 63, 300, 111, "2016 pairs: slot 8 has no live thread"),
    _c("slots9_d64", 2, 64, 300, 112, "2080 pairs: slot 8 holds 32 live threads; 51 968 bytes of LDS in fe_logprob"),
    # ---- frame counts at D = 64, K = 2 (n < 2 D is rank deficient: reg_covar carries the condition number)
    _c("n2_k1_d64", 1, 64, 2, 120, "two frames, one component: a rank-1 covariance", reg=1e-2, cov=False),
    _c("n31_d64", 2, 64, 31, 121, "one short density block, one short covariance step", reg=1e-2, cov=False),
    _c("n32_d64", 2, 64, 32, 122, "exactly FE_FB = FE_CB frames", reg=1e-2, cov=False),
    _c("n33_d64", 2, 64, 33, 123, "a second block and step of one frame", reg=1e-2, cov=False),
    _c("n64_d64", 2, 64, 64, 124, "n = D", reg=1e-2, cov=False),
    _c("n255_d64", 2, 64, 255, 125, "one short log-sum-exp block", reg=1e-3, cov=False),
    _c("n256_d64", 2, 64, 256, 126, "exactly one 256-frame block and one chunk", reg=1e-3, cov=False),
    _c("n257_d64", 2, 64, 257, 127, "two chunks of 129 and 128 frames: a step tail inside the data", reg=1e-3),
    _c("n8192_d64", 2, 64, 8192, 128, "32 chunks of 256: the last size with whole steps", cov=False),
    _c("n8193_d64", 2, 64, 8193, 129, "32 chunks of 257: every chunk ends in a one-frame step"),
    # ---- large n
    _c("n16385_k7_d2", 7, 2, 16385, 130, "chunk 513; D = 2"),
    _c("n8225_k3_d45", 3, 45, 8225, 131, "chunk 258 at five pair slots"),
    # ---- K
    _c("k1_d64_n64", 1, 64, 64, 140, "one component, n = D", reg=1e-2),
    _c("k64_d3", 64, 3, 640, 141, "fe_derive: one full block of 64", reg=1e-3),
    _c("k65_d3", 65, 3, 650, 142, "fe_derive: a second block of one", reg=1e-3),
    _c("k5_d58_n5", 5, 58, 5, 143, "n = K: a frame per component", reg=1e-2),
    _c("rank_k2_d40_n24", 2, 40, 24, 144, "n < D: every covariance is rank deficient before reg_covar", reg=1e-2),
    # ---- degenerate and shifted
    _c("empty_k3_d48", 3, 48, 600, 150, "a component with nk = 10 eps, mean 0 / nk, covariance reg I", kind="empty"),
    _c("shift_k3_d13", 3, 13, 400, 151, "frames at +100 (a float64 E[x x^T] - mu mu^T is 1.2e-11 off here: four digits lost)", kind="shift"),
    # ---- the default stop rule (tol 1e-3, max_iter 100): converged, every bound change further than 1e-6 from tol
    _c("stop_k2_d64", 2, 64, 400, 160, "the stop rule at D = 64", tol=1e-3, max_iter=100, cov=False),
    _c("stop_k3_d5_n8200", 3, 5, 8200, 161, "the stop rule with the chunk count pinned", tol=1e-3, max_iter=100, cov=False),
)
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]

# Measured on the CPU (test_fullfit_cases_cpu.py asserts the bounds; these are the worst figures over all rows behind them):
#   fo.fit against scikit-learn 1.7.2         weights 1.0e-15, means 9.2e-16, covariances 7.6e-15 (slots8_d63), precision factor
#                                             4.7e-14 (rank_k2_d40_n24), bound 8.1e-15 relative                   (bound: 1e-12)
#   fo.fit on permuted frames against itself  weights 5.6e-15, means 6.0e-15 (n16385_k7_d2), covariances 3.9e-14 (n256_d64)
#                                                                                                                  (bound: 1e-11)
#   largest covariance condition number       1.3e4 (n31_d64, n33_d64: rank deficient at reg_covar 1e-2); 330 at most for the
#                                             rows at the default reg_covar                                        (bound: 1e6)
PERMUTATION_FLOOR = 1e-11
MAX_CONDITION = 1e6


def frames(K, D, n, seed, shift=0.0, spread=2.0):
    """[n][D] float64 on the 1/256 grid: frame i belongs to cluster i % K; a cluster has a centre, a scale and a banded full
    covariance of its own (z_d + a z_(d-1) + z_(d-2) / 4 around the ring of coordinates: condition number below 50).  The
    frames start_rows() picks as starting means sit on their centres: the shared starting precision is the inverse of the WHOLE
    data's covariance, which discounts the directions between the centres, so that from an outlying frame of a wide cluster the
    first E-step is decided by that frame's own noise and EM collapses a component onto a handful of frames."""
    own = np.arange(n) % K
    cent = spread * noise(seed, (K, D))
    z = noise(seed + 1, (n, D))
    z[start_rows(n, K, seed)] = 0.0
    a = ((own % 4) + 1) / 8.0
    s = 1.0 + (own % 3) / 2.0
    y = cent[own] + s[:, None] * (z + a[:, None] * np.roll(z, 1, axis=1) + 0.25 * np.roll(z, 2, axis=1))
    return np.round(y * 256.0) / 256.0 + shift


def start_rows(n, K, seed):
    """the K frames a fit starts from: frame k + K j, of cluster k"""
    return np.arange(K) + K * (seed % (n // K))


def start(X, K, seed, kind="plain"):
    """-> (weights, means, precisions): make_fullcov_golden.init_params with the frames picked by arithmetic (start_rows) and the precisions rounded to float32"""
    n, D = X.shape
    w = np.full(K, 1.0 / K)
    mu = X[start_rows(n, K, seed)].copy()
    if kind == "empty":
        mu[K - 1] = 1000.0
        return w, mu, np.repeat(np.eye(D)[None], K, axis=0)
    C = np.cov(X.T).reshape(D, D) + 0.1 * np.eye(D)
    prec = np.linalg.inv(C)
    prec = (0.5 * (prec + prec.T)).astype(np.float32).astype(np.float64)
    return w, mu, np.repeat(prec[None], K, axis=0)


@lru_cache(maxsize=None)
def build(name):
    """-> (X, (weights_init, means_init, precisions_init)) of a row; cached, read-only"""
    c = BY_NAME[name]
    X = frames(c.K, c.D, c.n, c.seed, 100.0 if c.kind == "shift" else 0.0, c.spread)
    init = start(X, c.K, c.seed, c.kind)
    for a in (X,) + init:
        a.setflags(write=False)
    return X, init


def oracle_fit(X, init, reg, tol, max_iter):
    return fo.fit(X, init[0], init[1], fo.precisions_to_cholesky(init[2]), tol=tol, reg_covar=reg, max_iter=max_iter)


@lru_cache(maxsize=None)
def restated(name):
    """fo.fit of a row, computed once for every test that needs it (do not write into it)"""
    c = BY_NAME[name]
    X, init = build(name)
    return oracle_fit(X, init, c.reg, c.tol, c.max_iter)


def permutation(n, seed):
    """a fixed permutation of n frames: the order of n hashed fractions"""
    return np.argsort(noise(seed + 7, (n,)), kind="stable")


def rel(a, b):
    """norm-wise relative difference ||a - b|| / ||b||"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(1e-300, float(np.linalg.norm(b))))


def load_golden(path):
    """tests/golden/fullfit_edge_golden.npz -> {name: dict(weights, means, covariances or None, prec_chol or None, score or None,
    lower_bound, n_iter, converged)}: the covariances expanded from their lower triangles, and scikit-learn's precision factor of
    them (its _compute_precision_cholesky, restated by fo.precision_cholesky: it reads the lower triangle only)"""
    out = {}
    with np.load(path) as npz:
        z = {k: npz[k] for k in npz.files}
    for c in CASES:
        p = c.name + "_"
        r = dict(weights=z[p + "w"], means=z[p + "mu"], lower_bound=float(z[p + "lower_bound"]), n_iter=int(z[p + "n_iter"]),
                 converged=bool(z[p + "converged"]), covariances=None, prec_chol=None, score=None)
        if p + "covl" in z:
            cov = np.zeros((c.K, c.D, c.D))
            i, j = np.tril_indices(c.D)
            cov[:, i, j] = z[p + "covl"]
            cov[:, j, i] = z[p + "covl"]
            r["covariances"], r["prec_chol"] = cov, fo.precision_cholesky(cov)
        if p + "score" in z:
            r["score"] = float(z[p + "score"])
        out[c.name] = r
    return out
