"""The float64 full-covariance EM kernels on the MI355X at their width and frame-count edges (csrc/gmm_full.hip: fe_logprob,
fe_lse, fe_bound, fe_means, fe_cov, fe_chol, fe_weights, fe_derive, the one-hot start; driven by fe_fit_group).  The rows are
tests/fullfit_cases.py's; each fit is compared with scikit-learn's recorded answer (tests/golden/fullfit_edge_golden.npz) and with
the float64 restatement (tests/fullcov_oracle.py) run here, under the tolerances of
test_gpu_full_cov.py::test_fit_from_explicit_inits_matches_sklearn.  tests/test_fullfit_cases_cpu.py shows without a GPU that the
restatement's own noise (against scikit-learn, and under a permutation of the frames) is five orders below them."""
import os
import warnings
from functools import lru_cache

import numpy as np
import pytest

import fullcov_oracle as fo
import fullfit_cases as fc
from conftest import ll_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("weights_", "means_", "covariances_", "precisions_cholesky_")


@pytest.fixture(scope="module")
def g():
    return fc.load_golden(os.path.join(ROOT, "tests", "golden", "fullfit_edge_golden.npz"))


def _fit(X, init, **kw):
    from speaker_recognition_amd import skgmm
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", skgmm.ConvergenceWarning)
        return skgmm.GMM(len(init[0]), weights_init=init[0], means_init=init[1], precisions_init=init[2], **kw).fit(X)


@lru_cache(maxsize=None)
def _device_fit(name):
    """the device fit of a row, once for the tests that need it"""
    c = fc.BY_NAME[name]
    X, init = fc.build(name)
    return _fit(X, init, tol=c.tol, reg_covar=c.reg, max_iter=c.max_iter)


def _check_structure(m, tag):
    cov, P = m.covariances_, m.precisions_cholesky_
    assert all(np.all(np.isfinite(getattr(m, a))) for a in ARRAYS), tag
    assert np.array_equal(cov, np.transpose(cov, (0, 2, 1))), tag          # fe_chol writes both halves from one value
    assert not np.any(np.tril(P, -1)), tag                                 # upper triangular, the rest exactly zero


def _check_against(m, ref, tag, n_iter=None):
    """the device tolerances: 1e-9 norm-wise, the precision factor at max(1e-9, 1e-13 x condition number), the bound at 1e-10;
    ref: a dict of fc.load_golden or of fo.fit (None: not recorded) -> the figures"""
    figures = {}
    for attr, key in (("weights_", "weights"), ("means_", "means"), ("covariances_", "covariances")):
        if ref[key] is not None:
            figures[key] = (fc.rel(getattr(m, attr), ref[key]), 1e-9)
    if ref["prec_chol"] is not None:
        cond = max(np.linalg.cond(cv) for cv in ref["covariances"])
        figures["prec_chol"] = (fc.rel(m.precisions_cholesky_, ref["prec_chol"]), max(1e-9, 1e-13 * cond))
    lb = float(ref["lower_bound"])
    figures["lower_bound"] = (abs(m.lower_bound_ - lb) / max(1.0, abs(lb)), 1e-10)
    print(tag, " ".join("%s %.1e" % (k, v[0]) for k, v in figures.items()))
    for key, (d, tol) in figures.items():
        assert d < tol, (tag, key, d, tol)
    assert m.n_iter_ == int(ref["n_iter"]) and bool(m.converged_) == bool(ref["converged"]), (tag, m.n_iter_, m.converged_)
    return figures


@pytest.mark.parametrize("name", fc.NAMES)
def test_fit_matches_sklearn_and_the_restatement(g, name):
    c = fc.BY_NAME[name]
    m = _device_fit(name)
    _check_structure(m, name)
    _check_against(m, g[name], name + " vs sklearn:")
    _check_against(m, fc.restated(name), name + " vs restatement:")
    if c.tol == 0:
        assert m.n_iter_ == c.max_iter and not m.converged_
    if c.kind == "empty":
        assert abs(m.weights_[2] - 3.7e-18) < 1e-19 and not np.any(m.means_[2])
        assert np.array_equal(m.covariances_[2], c.reg * np.eye(c.D))


@pytest.mark.parametrize("D", [1, 64])
def test_kmeans_start_with_forced_labels(D):
    """K = 1: whatever k-means does, every label is 0, so the start is the M-step of all-ones responsibilities with the weights
    nk / n (fe_onehot, weight mode 1), and the fit two iterations from there"""
    from speaker_recognition_amd import skgmm
    n, reg = 257, 1e-6
    X = fc.frames(1, D, n, 170 + D)
    m = skgmm.GMM(1, max_iter=2, random_state=3).fit(X)
    _check_structure(m, D)
    w, mu, _cov, P = fo.m_step(X, np.ones((n, 1)), reg, normalise=False)
    assert abs(w[0] - 1.0) < 1e-15
    ref = fo.fit(X, w, mu, P, tol=1e-3, reg_covar=reg, max_iter=2)
    assert ref["n_iter"] == 2 and abs(ref["bounds"][1] - ref["bounds"][0]) < 1e-9           # (far inside tol: no knife edge)
    _check_against(m, ref, "kmeans K 1 D %d:" % D)


BATCH_N = (4, 33, 257, 8193, 300)       # 2 K frames; a step of one frame; two chunks; 32 chunks of 257; an ordinary speaker


@lru_cache(maxsize=None)
def _batch_speakers():
    """five K = 2 speakers at D = 64 -> (kwargs, data, the restatement of each, the single device fits)"""
    kws, Xs, refs = [], [], []
    for s, n in enumerate(BATCH_N):
        X = fc.frames(2, 64, n, 180 + s)
        init = fc.start(X, 2, 180 + s)
        reg = 1e-2 if n < 128 else 1e-6
        kws.append(dict(n_components=2, tol=0.0, max_iter=3, reg_covar=reg, weights_init=init[0], means_init=init[1],
                        precisions_init=init[2]))
        Xs.append(X)
        refs.append(fc.oracle_fit(X, init, reg, 0.0, 3))
    singles = [_fit(X, (kw["weights_init"], kw["means_init"], kw["precisions_init"]), tol=0.0, max_iter=3, reg_covar=kw["reg_covar"])
               for kw, X in zip(kws, Xs)]
    return kws, Xs, refs, singles


@pytest.mark.parametrize("limit, groups", [(None, 1), (1 << 20, 3)])
def test_batch_at_d64_is_the_single_fits(limit, groups):
    """fit_many at D = 64: bit-identical to the single fits and within the device tolerances of the restatement, in one group
    (the default full_fit_batch_bytes) and cut into three (1 MiB: the first three speakers, 8193 frames alone, the last alone)"""
    from speaker_recognition_amd import _lib, skgmm
    kws, Xs, refs, singles = _batch_speakers()
    gm = [skgmm.GMM(**kw) for kw in kws]
    default = _lib.full_fit_batch_bytes()
    it0 = _lib.full_fit_batch_stats()[2]
    try:
        if limit is not None:
            _lib.set_option("full_fit_batch_bytes", limit)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", skgmm.ConvergenceWarning)
            errors = skgmm.fit_many(gm, Xs)
    finally:
        _lib.set_option("full_fit_batch_bytes", default)
    assert _lib.full_fit_batch_bytes() == default
    assert errors == [None] * len(gm)
    assert _lib.full_fit_batch_stats()[2] - it0 == 3 * groups              # three iterations per group
    for s, (single, batched, ref) in enumerate(zip(singles, gm, refs)):
        for attr in ARRAYS:
            assert np.array_equal(getattr(single, attr), getattr(batched, attr)), (s, attr)
        assert (single.n_iter_, single.converged_, single.lower_bound_) == (batched.n_iter_, batched.converged_, batched.lower_bound_)
        _check_structure(batched, s)
        _check_against(batched, ref, "batch speaker %d (n %d):" % (s, BATCH_N[s]))


@pytest.mark.parametrize("name", ["slots9_d64", "slots3_d32"])
def test_fitted_model_hands_over_to_scoring(name):
    """the fitted parameters, as the fit leaves them on the handle, under the fp32 scoring kernels (D = 32 and D = 64: the widest
    model of either built kernel) against the restatement on the same parameters"""
    X, _ = fc.build(name)
    m = _device_fit(name)
    ll = m.score_samples(X)
    want = fo.score_samples(X, m.weights_, m.means_, m.precisions_cholesky_)
    assert ll.shape == want.shape and ll_close(ll, want, 1e-4) <= 1.0, ll_close(ll, want, 1e-4)
