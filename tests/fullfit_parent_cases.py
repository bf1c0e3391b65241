"""The fits of tests/test_gpu_fullfit_parent_bits.py and of its recorder (tests/golden/make_fullfit_parent_bits.py): what the
float64 full-covariance EM driver (csrc/gmm_full_fit.hip: fe_fit_group, planned by csrc/full_plan.cpp) computes, reduced to what a
512 KiB fixture can hold.  Plain module (as tests/em_parent_cases.py).  The cases:

  * every row of tests/fullfit_cases.py, fitted alone from its explicit start (``skgmm.GMM.fit``: a group of one);
  * the five D = 64 speakers of test_gpu_fullfit_cases.py (BATCH_N) as one batch, in one group and cut by a bound of 1 MiB;
  * seven K = 32, D = 28 speakers with the k-means start, of the sizes, seeds and reg_covar of test_gpu_full_fit_batch.py's
    ``kmeans_speakers``, in one group and under a bound of 1 byte (every speaker a group of its own).

All data are fullfit_cases.frames' (an integer hash, elementwise arithmetic): the same bits under any numpy.  A fit is kept as
n_iter, converged, lower_bound, the weights and means as float64, and a SHA-256 each of the raw bytes of precisions_cholesky_ and
covariances_ -- equality of bits is equality of digests; a speaker whose fit failed is kept as its message.  A batch also keeps the
three sr_full_fit_batch_stats deltas of its call."""
import hashlib
import warnings

import numpy as np

import fullfit_cases as fc

BATCH_N = (4, 33, 257, 8193, 300)               # test_gpu_fullfit_cases.py's
KM_K, KM_D = 32, 28
KM_SIZES = (5600, KM_K, 200, 256, 257, 9000, KM_K)      # test_gpu_full_fit_batch.py's SIZES

# name, kind, the bound (None: the default full_fit_batch_bytes)
BATCHES = (("d64_one_group", "d64", None), ("d64_cut_1mib", "d64", 1 << 20), ("kmeans_one_group", "kmeans", None),
           ("kmeans_bound_1", "kmeans", 1))
CASES = ["row/" + n for n in fc.NAMES] + ["batch/" + b[0] for b in BATCHES]


def _digest(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8).copy()


def _model(m, error=None):
    """-> what is kept of a fit"""
    if error is not None:
        return {"error": np.array(str(error))}
    return {"n_iter": np.array(m.n_iter_, np.int64), "converged": np.array(bool(m.converged_)),
            "lower_bound": np.array(m.lower_bound_, np.float64), "weights": np.array(m.weights_, np.float64),
            "means": np.array(m.means_, np.float64), "prec_chol_sha256": _digest(m.precisions_cholesky_),
            "cov_sha256": _digest(m.covariances_)}


def _d64_speakers():
    kws, Xs = [], []
    for s, n in enumerate(BATCH_N):
        X = fc.frames(2, 64, n, 180 + s)
        w, mu, prec = fc.start(X, 2, 180 + s)
        kws.append(dict(n_components=2, tol=0.0, max_iter=3, reg_covar=1e-2 if n < 128 else 1e-6, weights_init=w, means_init=mu,
                        precisions_init=prec))
        Xs.append(X)
    return kws, Xs


def _kmeans_speakers():
    kws, Xs = [], []
    for s, n in enumerate(KM_SIZES):
        Xs.append(fc.frames(8, KM_D, n, 300 + s))
        kw = dict(n_components=KM_K, random_state=100 + s)
        if s % len(KM_SIZES) == 6:
            kw["reg_covar"] = 1e-2
        kws.append(kw)
    return kws, Xs


def run_case(name):
    """-> {key: array} of a case of CASES, on the current device"""
    from speaker_recognition_amd import _lib, skgmm
    group, name = name.split("/")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", skgmm.ConvergenceWarning)
        if group == "row":
            c = fc.BY_NAME[name]
            X, init = fc.build(name)
            m = skgmm.GMM(c.K, weights_init=init[0], means_init=init[1], precisions_init=init[2], tol=c.tol, reg_covar=c.reg,
                          max_iter=c.max_iter).fit(X)
            return _model(m)
        _, kind, bound = next(b for b in BATCHES if b[0] == name)
        kws, Xs = _d64_speakers() if kind == "d64" else _kmeans_speakers()
        gm = [skgmm.GMM(**kw) for kw in kws]
        default = _lib.full_fit_batch_bytes()
        before = _lib.full_fit_batch_stats()
        try:
            if bound is not None:
                _lib.set_option("full_fit_batch_bytes", bound)
            errors = skgmm.fit_many(gm, Xs)
        finally:
            _lib.set_option("full_fit_batch_bytes", default)
        after = _lib.full_fit_batch_stats()
    out = {"stats": np.array([a - b for a, b in zip(after, before)], np.int64)}
    for s, (m, e) in enumerate(zip(gm, errors)):
        out.update({"%d/%s" % (s, k): v for k, v in _model(m, e).items()})
    return out
