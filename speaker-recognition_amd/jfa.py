"""The front of the reference's JFA leg (src/jfa/collect_suf_stats.m, sc_compute_suf_stats.m -- MATLAB there, one session at a
time on the host) on the device: zero- and first-order Baum-Welch statistics of whole corpora against one UBM in a single batched
pass (csrc/bw_stats.hip through ``core.ModelSet.bw_stats``), and the classical relevance-MAP supervector they give.

Orientation follows the reference where the names do: ``collect_suf_stats`` takes MATLAB-shaped arguments (``data`` dim x frames,
``m`` and ``v`` dim x gaussians with ``v`` holding VARIANCES, ``w`` a vector) and returns ``N`` (K,) and ``F`` (K * D,) in the
supervector order -- mixture-major, D values per mixture, what ``reshape(F, n_mixtures * dim, 1)`` of the dim x gaussians matrix
``data * gammas'`` is.  One difference in arithmetic: the posteriors are formed in the log domain, so a frame whose linear-domain
densities would all underflow -- where ``gaussian_posteriors.m`` divides 0 by 0 and every statistic of the session turns NaN --
contributes like any other frame; only a frame whose log-sum-exp is not finite (a NaN row, values beyond every density's range)
is left out."""
from __future__ import annotations

import numpy as np

from .core import Batch, ModelSet
from .pygmm import GMM


def as_ubm(ubm) -> GMM:
    """A ``pygmm.GMM`` as it is; a triple ``(weights [K], means [K, D], variances [K, D])`` or a mapping with the keys
    ``weights``, ``means``, ``variances`` (tests/golden/jfa_ubm.npz) as a new one."""
    if isinstance(ubm, GMM):
        return ubm
    if hasattr(ubm, "keys"):
        ubm = (ubm["weights"], ubm["means"], ubm["variances"])
    w, m, v = (np.asarray(a, dtype=np.float64) for a in ubm)
    if m.ndim != 2 or v.shape != m.shape or w.reshape(-1).shape != (m.shape[0],):
        raise ValueError("expected weights [K], means [K, D], variances [K, D]; got %r, %r, %r" % (w.shape, m.shape, v.shape))
    return GMM.from_arrays(w.reshape(-1), m, np.sqrt(v))


def compute_suf_stats(sessions, ubm):
    """``sessions``: a list of [T_s, D] feature matrices (or a feature ``Batch`` already on the device); ``ubm``: see ``as_ubm``.
    -> ``N`` [n_sessions, K], ``F`` [n_sessions, K * D]: the two arrays sc_compute_suf_stats.m saves, from one device pass."""
    g = as_ubm(ubm)
    feats = sessions if isinstance(sessions, Batch) else Batch.from_features([np.asarray(s) for s in sessions])
    return ModelSet([g]).bw_stats(feats, 0)


def collect_suf_stats(data, m, v, w):
    """One session, MATLAB orientation: ``data`` [D, T], ``m`` / ``v`` [D, K] (variances), ``w`` [K] or [K, 1].
    -> ``N`` (K,), ``F`` (K * D,)."""
    data, m, v = (np.asarray(a, dtype=np.float64) for a in (data, m, v))
    if data.ndim != 2 or m.ndim != 2 or m.shape != v.shape or data.shape[0] != m.shape[0]:
        raise ValueError("expected data [D, T], m and v [D, K]; got %r, %r, %r" % (data.shape, m.shape, v.shape))
    N, F = compute_suf_stats([data.T], (np.asarray(w, dtype=np.float64).reshape(-1), m.T, v.T))
    return N[0], F[0]


def map_supervectors(N, F, ubm, relevance=16.0):
    """Relevance-MAP means of every session from its statistics (host, float64; the rule of gmmubm.cc:53-74 applied once):
    ``alpha E_k + (1 - alpha) mu_k`` with ``E_k = F_k / N_k`` and ``alpha = N_k / (N_k + relevance)``, i.e.
    ``(F_k + relevance mu_k) / (N_k + relevance)``.  ``ubm``: see ``as_ubm`` (only its means are used).
    -> [n_sessions, K * D] in the supervector order."""
    N = np.atleast_2d(np.asarray(N, dtype=np.float64))
    F = np.atleast_2d(np.asarray(F, dtype=np.float64))
    if isinstance(ubm, GMM):
        mu = ubm.params()[1]
    elif hasattr(ubm, "keys"):
        mu = ubm["means"]
    else:
        mu = ubm[1]
    mu = np.asarray(mu, dtype=np.float64)
    K, D = mu.shape
    if N.shape[1] != K or F.shape != (N.shape[0], K * D):
        raise ValueError("expected N [n, %d] and F [n, %d]; got %r and %r" % (K, K * D, N.shape, F.shape))
    if not relevance > 0:
        raise ValueError("relevance must be positive")
    out = (F.reshape(-1, K, D) + relevance * mu[None]) / (N[:, :, None] + relevance)
    return out.reshape(-1, K * D)
