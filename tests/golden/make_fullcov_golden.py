#!/usr/bin/env python3
"""Known answers for the full-covariance GMMs (skgmm.GMM, csrc/gmm_full.hip) from scikit-learn itself.

    python tests/golden/make_fullcov_golden.py      # needs scikit-learn; writes tests/golden/fullcov_golden.npz

Seeded data, K in {1, 4, 32}, D in {1, 13, 28, 39}; frames are stored exactly as scikit-learn saw them (values on a 1/256
grid, exact in fp32 and float64), so a test hands the device the very numbers of the recorded answers.

Storage is kept small: frames on a grid of 1/256 as int16 (``X_q``: X = X_q / 256 exactly), precision factors of the scoring
models rounded to float32 and kept as their upper triangles, covariances as lower triangles, the initial precision once (every
component starts from the same one).  ``fullcov_oracle.load_golden`` expands them into full arrays.
  score_<c>_*   GaussianMixture.score_samples of a fixed model (weights, means, precisions_cholesky) on fixed frames, the last
                quarter of them outliers shifted by +60
  fit5_<c>_*    fit from explicit weights_init / means_init / precisions_init with tol=0, max_iter=5: weights, means and
                covariances after five iterations and the lower bound
  fitc_<c>_*    the same with the default tol: n_iter_, converged_, lower_bound_, weights and means (cases whose every
                bound change is further than 1e-6 from tol, so that n_iter_ does not hang on the last bits)
  collapsed_*   a fit whose Cholesky fails (a component collapsed onto repeated frames, reg_covar=0)
The GPU tests read only the .npz.
"""
import os
import sys
import warnings

import numpy as np
from sklearn.mixture import GaussianMixture

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fullcov_oracle as fo  # noqa: E402

SCORE_CASES = [("k1d1", 1, 1), ("k4d13", 4, 13), ("k32d28", 32, 28), ("k4d39", 4, 39)]
FIT_CASES = [("k1d1", 1, 1, 300), ("k4d13", 4, 13, 800), ("k32d28", 32, 28, 2000), ("k4d39", 4, 39, 500)]


def quantise(X):
    """-> (int16 codes, the float64 frames they stand for exactly)"""
    q = np.round(np.asarray(X) * 256.0)
    assert np.max(np.abs(q)) < 32767
    q = q.astype(np.int16)
    return q, q.astype(np.float64) / 256.0


def upper(a):
    """the upper triangles of [K][D][D] -> [K][D (D + 1) / 2]"""
    iu = np.triu_indices(a.shape[-1])
    return np.ascontiguousarray(a[:, iu[0], iu[1]])


def lower(a):
    """the lower triangles of [K][D][D], row by row -- the half a lower Cholesky factorisation reads (a computed covariance is
    symmetric only to its last bits, which a condition number of 1e8 turns into 1e-9 of the factor)"""
    il = np.tril_indices(a.shape[-1])
    return np.ascontiguousarray(a[:, il[0], il[1]])


def init_params(rng, X, K):
    """weights uniform, means = K distinct frames, precisions = the inverse data covariance (+ a little ridge)"""
    w = np.full(K, 1.0 / K)
    mu = X[rng.choice(len(X), K, replace=False)].copy()
    C = np.cov(X.T).reshape(X.shape[1], X.shape[1]) + 0.1 * np.eye(X.shape[1])
    prec = np.repeat(np.linalg.inv(C)[None], K, axis=0)
    prec = 0.5 * (prec + np.transpose(prec, (0, 2, 1)))
    return w, mu, prec


def main():
    out = {}
    for c, K, D in SCORE_CASES:
        rng = np.random.default_rng(1000 + K * 100 + D)
        model = fo.random_model(rng, K, D)
        X = fo.draw(rng, model, 320)
        X[240:] += 60.0
        Xq, X = quantise(X)
        P = fo.precision_cholesky(model[2]).astype(np.float32)
        gm = GaussianMixture(K, covariance_type="full")
        gm.weights_, gm.means_, gm.covariances_ = model
        gm.precisions_cholesky_ = P.astype(np.float64)
        out["score_%s_w" % c], out["score_%s_mu" % c], out["score_%s_Pu" % c] = model[0], model[1], upper(P)
        out["score_%s_X_q" % c] = Xq
        out["score_%s_ll" % c] = gm.score_samples(X)
    for c, K, D, n in FIT_CASES:
        for seed in range(2000, 2100):
            rng = np.random.default_rng(seed + K * 100 + D)
            Xq, X = quantise(fo.draw(rng, fo.random_model(rng, K, D), n))
            w, mu, prec = init_params(rng, X, K)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                g5 = GaussianMixture(K, covariance_type="full", tol=0, max_iter=5, weights_init=w, means_init=mu,
                                     precisions_init=prec).fit(X)
                gc = GaussianMixture(K, covariance_type="full", weights_init=w, means_init=mu, precisions_init=prec).fit(X)
            hist = fo.fit(X, w, mu, fo.precisions_to_cholesky(prec))["bounds"]
            changes = np.abs(np.diff(np.concatenate([[-np.inf], hist])))
            if not gc.converged_ or np.min(np.abs(changes - 1e-3)) < 1e-6:
                continue
            break
        else:
            raise SystemExit("no stable fit case for %s" % c)
        p = "fit_%s_" % c
        out[p + "X_q"] = Xq
        out[p + "w0"], out[p + "mu0"], out[p + "prec0_one"] = w, mu, prec[0]
        for tag, g in (("fit5_%s_" % c, g5), ("fitc_%s_" % c, gc)):
            out[tag + "w"], out[tag + "mu"] = g.weights_, g.means_
            out[tag + "n_iter"], out[tag + "converged"], out[tag + "lower_bound"] = g.n_iter_, int(g.converged_), g.lower_bound_
        out["fit5_%s_covl" % c] = lower(g5.covariances_)
    # a component that collapses onto repeated frames: its covariance is singular with reg_covar = 0
    rng = np.random.default_rng(77)
    Xq, X = quantise(np.concatenate([np.tile([[5.0, 5.0, 5.0]], (20, 1)), rng.normal(0, 1, (80, 3))]))
    w = np.array([0.5, 0.5])
    mu = np.array([[5.0, 5.0, 5.0], [0.0, 0.0, 0.0]])
    prec = np.array([np.eye(3) * 1e6, np.eye(3)])
    try:
        GaussianMixture(2, covariance_type="full", reg_covar=0.0, weights_init=w, means_init=mu, precisions_init=prec).fit(X)
        raise SystemExit("the collapsed case did not fail")
    except ValueError as e:
        assert "ill-defined empirical covariance" in str(e)
    out["collapsed_X_q"], out["collapsed_w0"], out["collapsed_mu0"], out["collapsed_prec0"] = Xq, w, mu, prec
    np.savez_compressed(os.path.join(HERE, "fullcov_golden.npz"), **out)
    print("wrote fullcov_golden.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
