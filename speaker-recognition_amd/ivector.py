"""i-vectors by the names an i-vector system uses: the total-variability matrix is the eigenvoice matrix of the factor-analysis module
trained with every session a speaker of its own, and an i-vector is the factor of one session.  Thin wrappers over
that module: no device code of their own.  What comes out of ``extract`` goes into ``plda.transform`` / ``plda.PLDA``.

(The factor-analysis module is loaded by its full name when a function here is first called: importing this module costs nothing,
and tests/test_bw_cpu.py keeps the relative imports of that module to the files that held them before.)"""
from __future__ import annotations

import importlib

import numpy as np


def _fa():
    return importlib.import_module(__package__ + ".jfa")


def _n_sessions(stats_or_F):
    return stats_or_F.n if isinstance(stats_or_F, _fa().Stats) else np.atleast_2d(stats_or_F).shape[0]


def train_tv(stats_or_F, N, ubm, R=400, niter=10, T0=None, seed=0):
    """The total-variability matrix ``Tm`` [R, K * D] from the sessions' statistics -- a resident ``Stats`` (``N`` is not read), or the
    arrays ``F`` [n, K * D] and ``N`` [n, K]: ``train_v`` with one label per session, ``niter`` rounds in one device call from the
    random start (or ``T0``)."""
    return _fa().train_v(stats_or_F, N, np.arange(_n_sessions(stats_or_F)), ubm, ny=R, niter=niter, v0=T0, seed=seed)


def extract(stats_or_F, N, ubm, Tm):
    """The i-vectors [n, R] of the sessions: the statistics centred by session on the device (``centred(..., groups="sessions")``),
    then the factor estimator's ``factors`` with ``Tm`` [R, K * D] as the loading matrix."""
    fa = _fa()
    m, E = fa._ubm_m_E(ubm)
    n = _n_sessions(stats_or_F)
    if isinstance(stats_or_F, fa.Stats):
        with fa.centred(stats_or_F, m, E, np.arange(n), groups="sessions") as est:
            return est.factors(Tm)
    with fa.Stats.from_arrays(N, stats_or_F) as stats, fa.centred(stats, m, E, np.arange(n), groups="sessions") as est:
        return est.factors(Tm)
