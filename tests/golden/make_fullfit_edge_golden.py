#!/usr/bin/env python3
"""scikit-learn's own answers for the rows of tests/fullfit_cases.py (the full-covariance EM kernels at their width and
frame-count edges).

    python tests/golden/make_fullfit_edge_golden.py      # needs scikit-learn; writes tests/golden/fullfit_edge_golden.npz

Per row <name>: GaussianMixture(covariance_type='full', tol, reg_covar, max_iter, the row's explicit start).fit(X) ->
  <name>_w, _mu                          weights_, means_
  <name>_covl                            the lower triangles of covariances_, row by row (rows with cov=True; the half a lower
                                         Cholesky factorisation reads, as make_fullcov_golden.py keeps them)
  <name>_score                           score(X) of the fitted model (rows with cov=False: see the note above CASES)
  <name>_lower_bound, _n_iter, _converged
No frames and no starts are stored: fullfit_cases.build regenerates them from the integer hash.  The stop-rule rows are checked
as make_fullcov_golden.py chooses its own: converged, with every change of the bound further than 1e-6 from tol.

The archive is written entry by entry with a fixed timestamp, so that a second run gives the same bytes (numpy.savez stamps its
entries with the clock).
"""
import io
import os
import sys
import warnings
import zipfile

import numpy as np
from sklearn.mixture import GaussianMixture

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fullfit_cases as fc  # noqa: E402


def lower(a):
    il = np.tril_indices(a.shape[-1])
    return np.ascontiguousarray(a[:, il[0], il[1]])


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    out = {}
    for c in fc.CASES:
        X, (w, mu, prec) = fc.build(c.name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            g = GaussianMixture(c.K, covariance_type="full", tol=c.tol, reg_covar=c.reg, max_iter=c.max_iter, weights_init=w,
                                means_init=mu, precisions_init=prec).fit(X)
        if c.tol > 0:
            hist = fc.restated(c.name)["bounds"]
            changes = np.abs(np.diff(np.concatenate([[-np.inf], hist])))
            if not g.converged_ or np.min(np.abs(changes - c.tol)) < 1e-6:
                raise SystemExit("%s is no stable stop-rule case: give it another seed" % c.name)
        p = c.name + "_"
        out[p + "w"], out[p + "mu"] = g.weights_, g.means_
        if c.cov:
            out[p + "covl"] = lower(g.covariances_)
        else:
            out[p + "score"] = np.float64(g.score(X))
        out[p + "lower_bound"], out[p + "n_iter"], out[p + "converged"] = np.float64(g.lower_bound_), np.int64(g.n_iter_), \
            np.int64(g.converged_)
    path = os.path.join(HERE, "fullfit_edge_golden.npz")
    write_npz(path, out)
    print("wrote fullfit_edge_golden.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
