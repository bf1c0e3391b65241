"""The front of the reference's JFA leg (src/jfa/collect_suf_stats.m, sc_compute_suf_stats.m -- MATLAB there, one session at a
time on the host) on the device: zero- and first-order Baum-Welch statistics of whole corpora against one UBM in a single batched
pass (csrc/bw_stats.hip through ``core.ModelSet.bw_stats``), and the classical relevance-MAP supervector they give.

Orientation follows the reference where the names do: ``collect_suf_stats`` takes MATLAB-shaped arguments (``data`` dim x frames,
``m`` and ``v`` dim x gaussians with ``v`` holding VARIANCES, ``w`` a vector) and returns ``N`` (K,) and ``F`` (K * D,) in the
supervector order -- mixture-major, D values per mixture, what ``reshape(F, n_mixtures * dim, 1)`` of the dim x gaussians matrix
``data * gammas'`` is.  One difference in arithmetic: the posteriors are formed in the log domain, so a frame whose linear-domain
densities would all underflow -- where ``gaussian_posteriors.m`` divides 0 by 0 and every statistic of the session turns NaN --
contributes like any other frame; only a frame whose log-sum-exp is not finite (a NaN row, values beyond every density's range)
is left out.

Past the statistics, the rest of that leg: ``estimate_y_and_v``, ``estimate_x_and_u`` (csrc/jfa.hip through ``FactorEstimator``:
the gram matrices, the float64 GEMMs and the batched factorisation on the device), ``estimate_z_and_d`` and ``linear_scoring``
(elementwise work and one small product: host, float64, as ``map_supervectors``), and the four ``sc_*`` driver scripts as the
functions ``train_v``, ``train_u``, ``train_d`` and ``score_dot_product``.  The score matrix of a verification run on the device
(csrc/jfa_score.hip through ``score_trials``): ``kscore_famous_19``, the scorer with the channel factors integrated out, in the
reference's own orientation, and ``score_integrated``, the sibling of ``score_dot_product`` that scores with it.  Names, argument order and orientation are the
reference's: rows of ``F`` and ``N`` are segments, supervector columns are mixture-major, ``S`` is accepted and ignored, a scalar
``0`` for ``d``, ``u``, ``z``, ``y`` or ``x`` broadcasts as it does in MATLAB.  One stated difference: ``spk_ids`` are 0-BASED
integer labels -- row i of ``y`` and ``z`` belongs to label i, rows of labels that do not occur stay zero.  Where the reference's
``inv`` of an unoccupied mixture's accumulator gives Inf, the update here keeps that mixture's old columns (zeros in the
two-argument form, which has no old matrix).

The resident route (csrc/jfa_stats.hip): ``compute_suf_stats(..., resident=True)`` returns a ``Stats`` -- N and F stay on the
device -- and wherever a function here takes the pair ``F, N`` (or an ``(F, N)`` pair / mapping for ``trn`` / ``tst``) a ``Stats``
in place of ``F`` with ``N=None`` keeps every [sessions, K D] array there: grouping and centring run on the device
(``centred``), the z / d iteration too (``FactorEstimator.z_and_d``), the scorers read the handle.  Same outputs, same shapes, same
label rules; only factors and loading matrices cross the bus.  With host arrays nothing of this is reached."""
from __future__ import annotations

import ctypes as C

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


def compute_suf_stats(sessions, ubm, resident=False):
    """``sessions``: a list of [T_s, D] feature matrices (or a feature ``Batch`` already on the device); ``ubm``: see ``as_ubm``.
    -> ``N`` [n_sessions, K], ``F`` [n_sessions, K * D]: the two arrays sc_compute_suf_stats.m saves, from one device pass.
    ``resident``: -> a ``Stats`` that holds the two on the device instead."""
    g = as_ubm(ubm)
    feats = sessions if isinstance(sessions, Batch) else Batch.from_features([np.asarray(s) for s in sessions])
    if resident:
        return ModelSet([g]).bw_stats(feats, 0, resident=True)
    return ModelSet([g]).bw_stats(feats, 0)


class Stats:
    """Raw statistics ``N`` [n, K], ``F`` [n, K * D] of n sessions on the device (sr_stats_*): from ``compute_suf_stats(...,
    resident=True)`` / ``ModelSet.bw_stats(..., resident=True)`` or ``Stats.from_arrays``.  A context manager."""

    def __init__(self, handle):
        from . import _lib
        self._h = handle
        info = (C.c_int64 * 4)()
        _lib.check(_lib.lib().sr_stats_info(self._h, info, 4), "sr_stats_info")
        self.n, self.K, self.D, self.device = (int(v) for v in info)

    @classmethod
    def from_arrays(cls, N, F):
        from . import _lib
        N = _f64(np.atleast_2d(N))
        F = _f64(np.atleast_2d(F))
        n, K = N.shape
        if K < 1 or F.shape[0] != n or F.shape[1] % K:
            raise ValueError("expected N [n, K] and F [n, K * D]; got %r and %r" % (N.shape, F.shape))
        return cls(_lib.check(_lib.lib().sr_stats_from_host(n, K, F.shape[1] // K, _lib.as_dp(N), _lib.as_dp(F)), "sr_stats_from_host"))

    def _handle(self):
        from . import _lib
        if self._h is None:
            raise _lib.SRError("the statistics are closed")
        return self._h

    def get(self):
        """-> ``(N, F)`` as host arrays."""
        from . import _lib
        N, F = np.zeros((self.n, self.K)), np.zeros((self.n, self.K * self.D))
        _lib.check(_lib.lib().sr_stats_get(self._handle(), _lib.as_dp(N), _lib.as_dp(F)), "sr_stats_get")
        return N, F

    def take(self, rows):
        """A new ``Stats`` of the rows named (any order, repeats allowed; a boolean mask of n values selects), gathered on the device."""
        from . import _lib
        rows = np.asarray(rows)
        if rows.dtype == bool:
            rows = np.flatnonzero(rows)
        rows = np.arange(self.n)[rows] if rows.size else rows          # negative indices and slices' results as numpy reads them
        rows = np.ascontiguousarray(rows.reshape(-1), dtype=np.int64)
        return Stats(_lib.check(_lib.lib().sr_stats_take(self._handle(), _lib.as_i64p(rows), rows.size), "sr_stats_take"))

    def close(self):
        if self._h is not None:
            from . import _lib
            _lib.lib().sr_stats_close(self._h)
            self._h = None

    def __len__(self):
        return self.n

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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


# ---- factor estimation: eigenvoices, eigenchannels (csrc/jfa.hip) ----

def _f64(a, shape=None, name="array"):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != shape:
        raise ValueError("expected %s of shape %r, got %r" % (name, shape, a.shape))
    return a


class FactorEstimator:
    """The device handle of one set of groups (speakers, or sessions): occupancies ``N`` [G, K], CENTRED group-summed first-order
    statistics ``Fc`` [G, K * D] and the variances ``E`` [K * D] are copied to the device once and stay there over the iterations
    of a training run (``sr_jfa_open``).  A context manager.  ``bad_groups`` / ``skipped``: the counts of the last call."""

    def __init__(self, N, Fc, E):
        from . import _lib
        N = _f64(np.atleast_2d(N))
        Fc = _f64(np.atleast_2d(Fc))
        E = _f64(np.reshape(E, -1))
        G, K = N.shape
        if K < 1 or E.size % max(K, 1) or Fc.shape != (G, E.size):
            raise ValueError("expected N [G, K], Fc [G, K * D], E [K * D]; got %r, %r, %r" % (N.shape, Fc.shape, E.shape))
        self.G, self.K, self.D = G, K, E.size // K
        self.bad_groups = self.skipped = 0
        self._h = None
        self._h = _lib.check(_lib.lib().sr_jfa_open(G, K, self.D, _lib.as_dp(N), _lib.as_dp(Fc), _lib.as_dp(E)), "sr_jfa_open")

    @classmethod
    def _adopt(cls, handle, G, K, D, present=None):
        """An estimator around a handle the library made (``centred``)."""
        est = cls.__new__(cls)
        est.G, est.K, est.D = int(G), int(K), int(D)
        est.bad_groups = est.skipped = 0
        est.present = present
        est._h = handle
        return est

    def statistics(self):
        """-> ``(N [G, K], Fc [G, K * D])``: what the handle holds."""
        from . import _lib
        if self._h is None:
            raise _lib.SRError("the estimator is closed")
        N, Fc = np.zeros((self.G, self.K)), np.zeros((self.G, self.K * self.D))
        _lib.check(_lib.lib().sr_jfa_statistics(self._h, _lib.as_dp(N), _lib.as_dp(Fc)), "sr_jfa_statistics")
        return N, Fc

    def z_and_d(self, d, n_iter=1, want_z=False):
        """estimate_z_and_d.m on the handle's groups, ``n_iter`` rounds of ``d <- b / a`` in one device call (0: one evaluation,
        ``d`` comes back as it went in).  -> ``(d, a, b)`` or, with ``want_z``, ``(z [G, K * D], d, a, b)``; z, a and b are the
        last round's, for the d that round started from."""
        from . import _lib
        if self._h is None:
            raise _lib.SRError("the estimator is closed")
        kd = self.K * self.D
        d = np.array(np.broadcast_to(np.asarray(d, dtype=np.float64).reshape(-1), (kd,)), dtype=np.float64, order="C")
        a, b = np.zeros(kd), np.zeros(kd)
        z = np.zeros((self.G, kd)) if want_z else None
        _lib.check(_lib.lib().sr_jfa_zd(self._h, _lib.as_dp(d), int(n_iter), _lib.as_dp(z) if want_z else None, _lib.as_dp(a), _lib.as_dp(b)),
                   "sr_jfa_zd")
        return (z, d, a, b) if want_z else (d, a, b)

    def _loadings(self, W):
        W = np.array(np.atleast_2d(W), dtype=np.float64, order="C")
        if W.shape[1] != self.K * self.D:
            raise ValueError("expected W [R, %d], got %r" % (self.K * self.D, W.shape))
        return W

    def factors(self, W, accumulate=False):
        """-> ``y`` [G, R], or with ``accumulate`` ``(y, A [K, R, R], C [R, K * D])``."""
        from . import _lib
        if self._h is None:
            raise _lib.SRError("the estimator is closed")
        W = self._loadings(W)
        R = W.shape[0]
        y = np.zeros((self.G, R))
        A = np.zeros((self.K, R, R)) if accumulate else None
        Cm = np.zeros_like(W) if accumulate else None
        bad = C.c_int64(0)
        _lib.check(_lib.lib().sr_jfa_factors(self._h, _lib.as_dp(W), R, _lib.as_dp(y), _lib.as_dp(A) if accumulate else None,
                                             _lib.as_dp(Cm) if accumulate else None, C.byref(bad)), "sr_jfa_factors")
        self.bad_groups = int(bad.value)
        return (y, A, Cm) if accumulate else y

    def train(self, W, n_iter):
        """``n_iter`` rounds of factors -> accumulators -> update in one device call.  -> ``(W, y)``, ``y`` of the last round."""
        from . import _lib
        if self._h is None:
            raise _lib.SRError("the estimator is closed")
        W = self._loadings(W)
        R = W.shape[0]
        y = np.zeros((self.G, R))
        sk = C.c_int64(0)
        _lib.check(_lib.lib().sr_jfa_train(self._h, _lib.as_dp(W), R, int(n_iter), _lib.as_dp(y), C.byref(sk)), "sr_jfa_train")
        self.skipped = int(sk.value)
        return W, y

    def close(self):
        if self._h is not None:
            from . import _lib
            _lib.lib().sr_jfa_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def update_loadings(A, Cm, W_old, return_skipped=False):
    """The update alone: ``W_c = A_c^-1 C_c`` for every mixture whose ``A_c`` factors; the others keep ``W_old``'s columns.
    -> W (or ``(W, skipped)``)."""
    from . import _lib
    A = _f64(A)
    Cm = _f64(np.atleast_2d(Cm))
    if A.ndim != 3 or A.shape[1] != A.shape[2] or A.shape[1] != Cm.shape[0] or A.shape[0] < 1 or Cm.shape[1] % max(A.shape[0], 1):
        raise ValueError("expected A [K, R, R] and C [R, K * D]; got %r and %r" % (A.shape, Cm.shape))
    K, R = A.shape[0], A.shape[1]
    W = np.array(np.broadcast_to(np.asarray(W_old, dtype=np.float64), Cm.shape), dtype=np.float64, order="C")
    sk = C.c_int64(0)
    _lib.check(_lib.lib().sr_jfa_update(K, Cm.shape[1] // K, R, _lib.as_dp(A), _lib.as_dp(Cm), _lib.as_dp(W), C.byref(sk)), "sr_jfa_update")
    return (W, int(sk.value)) if return_skipped else W


def _labels(spk_ids, n):
    ids = np.asarray(spk_ids).reshape(-1)
    if ids.shape != (n,) or not np.issubdtype(ids.dtype, np.integer) or (n and ids.min() < 0):
        raise ValueError("spk_ids: %d 0-based integer labels, one per row of F and N" % n)
    return ids.astype(np.int64)


def _rows(a, n, width):
    """A factor matrix as [n, width]: a scalar, a column of n values or a full matrix -- MATLAB's broadcast of the sc_* scripts."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim < 2:
        a = a.reshape(-1, 1) if a.size > 1 else a.reshape(1, 1)
    if a.shape[0] < n and a.shape[0] != 1:
        raise ValueError("a factor matrix has %d rows, the labels need %d" % (a.shape[0], n))
    return np.broadcast_to(a[:n] if a.shape[0] >= n else a, (n, width if a.shape[1] == 1 else a.shape[1]))


def _times(f, W, n, kd):
    """f * W as [n, kd]: a matrix product when W is a loading matrix, the elementwise broadcast when it is the scalar 0."""
    W = np.asarray(W, dtype=np.float64)
    if W.ndim < 2:
        return np.broadcast_to(_rows(f, n, 1)[:, :1] * W, (n, kd)) if W.size == 1 else _rows(f, n, kd) * W.reshape(1, kd)
    return _rows(f, n, W.shape[0]) @ W


def _zd(z, d, n, kd):
    """z .* d as [n, kd] (d: the scalar 0 or a vector of kd values)."""
    return _rows(z, n, kd) * np.broadcast_to(np.asarray(d, dtype=np.float64).reshape(-1), (kd,))


def _stats(F, N, m, E):
    F = _f64(np.atleast_2d(F))
    N = _f64(np.atleast_2d(N))
    n, K = N.shape
    if K < 1 or F.shape[0] != n or F.shape[1] % K:
        raise ValueError("expected N [n, K] and F [n, K * D]; got %r and %r" % (N.shape, F.shape))
    kd = F.shape[1]
    return F, N, np.repeat(N, kd // K, axis=1), _f64(np.reshape(m, -1), (kd,), "m"), _f64(np.reshape(E, -1), (kd,), "E")


def _speaker_sums(a, ids, n_spk):
    out = np.zeros((n_spk,) + a.shape[1:])
    np.add.at(out, ids, a)
    return out


def _finish(est, W, nargout):
    if nargout == 1:
        return est.factors(W), None, None
    f, A, Cm = est.factors(W, accumulate=True)
    return f, A, Cm


# ---- the resident route: grouping and centring on the device (csrc/jfa_stats.hip) ----

def _absent(a):
    return a is None or (np.ndim(a) == 0 and a == 0)


def _term(f, W, n, kd, names):
    """A (factor, loading) pair for the device, or (None, None) where the term is absent: either side the scalar 0, or factors
    that are all zero (the sc_* scripts' columns of zeros)."""
    if _absent(W) or _absent(f):
        return None, None
    W = np.asarray(W, dtype=np.float64)
    if W.ndim < 2:
        raise ValueError("%s: the resident route takes a loading matrix [R, %d] or the scalar 0" % (names[1], kd))
    W = _f64(W)
    if W.shape[1] != kd:
        raise ValueError("expected %s [R, %d], got %r" % (names[1], kd, W.shape))
    f = _f64(_rows(f, n, W.shape[0]))
    if f.shape != (n, W.shape[0]):
        raise ValueError("expected %s [%d, %d], got %r" % (names[0], n, W.shape[0], f.shape))
    return (f, W) if f.any() else (None, None)


def centred(stats, m, E, spk_ids, groups="speakers", d=0, v=0, u=0, z=0, y=0, x=0):
    """The grouping and centring of ``estimate_*`` / ``train_*`` on the device (sr_jfa_open_centred) -> ``FactorEstimator``.
    ``groups`` "speakers": a row per label that occurs, ascending (``.present``), ``Fc_g = sum_j (F_j - N_j (x_j u)) -
    N_g (m + z_g d + y_g v)``; "sessions": a row per session, ``Fc_j = F_j - N_j (m + z_s d + y_s v + x_j u)``.  A term whose factor
    or loading is the scalar 0 is absent."""
    from . import _lib
    if groups not in ("speakers", "sessions"):
        raise ValueError("groups is 'speakers' or 'sessions', got %r" % (groups,))
    if not isinstance(stats, Stats):
        raise TypeError("centred takes a Stats (compute_suf_stats(..., resident=True) or Stats.from_arrays)")
    n, kd = stats.n, stats.K * stats.D
    m, E = _f64(np.reshape(m, -1), (kd,), "m"), _f64(np.reshape(E, -1), (kd,), "E")
    ids = np.ascontiguousarray(_labels(spk_ids, n))
    n_labels = int(ids.max()) + 1
    y, v = _term(y, v, n_labels, kd, ("y", "v"))
    x, u = _term(x, u, n, kd, ("x", "u"))
    if _absent(d) or _absent(z):
        z = d = None
    else:
        d = _f64(np.broadcast_to(np.asarray(d, dtype=np.float64).reshape(-1), (kd,)))
        z = _f64(_rows(z, n_labels, kd))
        if not (z.any() and d.any()):
            z = d = None
    opt = lambda a: _lib.as_dp(a) if a is not None else None                        # noqa: E731
    h = _lib.check(_lib.lib().sr_jfa_open_centred(stats._handle(), _lib.as_dp(E), _lib.as_dp(m), 0 if groups == "speakers" else 1, _lib.as_i64p(ids),
                                                  n_labels, opt(d), opt(z), opt(v), v.shape[0] if v is not None else 0, opt(y), opt(u),
                                                  u.shape[0] if u is not None else 0, opt(x)), "sr_jfa_open_centred")
    present = np.unique(ids)
    return FactorEstimator._adopt(h, present.size if groups == "speakers" else n, stats.K, stats.D, present)


def _resident_y_and_v(stats, m, E, d, v, u, z, x, spk_ids, nargout):
    W = _f64(np.atleast_2d(v))
    with centred(stats, m, E, spk_ids, "speakers", d=d, u=u, z=z, x=x) as est:
        f, A, Cm = _finish(est, W, nargout)
        out = np.zeros((int(est.present.max()) + 1, W.shape[0]))
        out[est.present] = f
    if nargout == 1:
        return out
    return (out, A, Cm) if nargout == 3 else (out, update_loadings(A, Cm, W))


def _resident_x_and_u(stats, m, E, d, v, u, z, y, spk_ids, nargout):
    W = _f64(np.atleast_2d(u))
    with centred(stats, m, E, spk_ids, "sessions", d=d, v=v, z=z, y=y) as est:
        f, A, Cm = _finish(est, W, nargout)
    if nargout == 1:
        return f
    return (f, A, Cm) if nargout == 3 else (f, update_loadings(A, Cm, W))


def _resident_z_and_d(stats, m, E, d, v, u, y, x, spk_ids, nargout):
    with centred(stats, m, E, spk_ids, "speakers", v=v, u=u, y=y, x=x) as est:
        zg, d_new, a, b = est.z_and_d(d, n_iter=0 if nargout != 2 else 1, want_z=True)
        zz = np.zeros((int(est.present.max()) + 1, stats.K * stats.D))
        zz[est.present] = zg
    if nargout == 1:
        return zz
    return (zz, a, b) if nargout == 3 else (zz, d_new)


def _pair(t):
    """``trn`` / ``tst`` as (F, N): an (F, N) pair, a mapping with those keys, or a ``Stats`` (-> (stats, None))."""
    if isinstance(t, Stats):
        return t, None
    return (t["F"], t["N"]) if hasattr(t, "keys") else t


def _n_rows(F, N):
    return F.n if isinstance(F, Stats) else np.atleast_2d(N).shape[0]


def estimate_y_and_v(F, N, S=None, m=None, E=None, d=0, v=None, u=0, z=0, y=0, x=0, spk_ids=None, nargout=1):
    """estimate_y_and_v.m: speaker factors ``y`` [max label + 1, R] (``nargout`` 1), ``(y, v)`` with the updated eigenvoices (2) or
    ``(y, A, C)`` with the accumulators (3); ``estimate_y_and_v(A, C)`` updates from accumulators.  Groups are speakers; the
    centring ``Fs = sum_sessions F - (m + z d) Ns - sum_j (x_j u) N_j`` is done here in float64, the rest on the device."""
    if isinstance(F, Stats):
        return _resident_y_and_v(F, m, E, d, v, u, z, x, spk_ids, nargout)
    if m is None:
        return update_loadings(F, N, 0.0)
    F, N, Nx, m, E = _stats(F, N, m, E)
    n, kd = F.shape
    ids = _labels(spk_ids, n)
    n_spk = int(ids.max()) + 1 if n else 0
    W = _f64(np.atleast_2d(v))
    present = np.unique(ids)
    Fs = _speaker_sums(F - _times(x, u, n, kd) * Nx, ids, n_spk) - (m + _zd(z, d, n_spk, kd)) * _speaker_sums(Nx, ids, n_spk)
    Ns = _speaker_sums(N, ids, n_spk)
    out = np.zeros((n_spk, W.shape[0]))
    with FactorEstimator(Ns[present], Fs[present], E) as est:
        f, A, Cm = _finish(est, W, nargout)
    out[present] = f
    if nargout == 1:
        return out
    return (out, A, Cm) if nargout == 3 else (out, update_loadings(A, Cm, W))


def estimate_x_and_u(F, N, S=None, m=None, E=None, d=0, v=0, u=None, z=0, y=0, x=0, spk_ids=None, nargout=1):
    """estimate_x_and_u.m: channel factors ``x`` [n_sessions, R], ``(x, u)`` or ``(x, A, C)``; ``estimate_x_and_u(A, C)`` updates
    from accumulators.  Every session is its own group, ``Fh = F_j - N_j (m + y v + z d)`` with its speaker's y and z."""
    if isinstance(F, Stats):
        return _resident_x_and_u(F, m, E, d, v, u, z, y, spk_ids, nargout)
    if m is None:
        return update_loadings(F, N, 0.0)
    F, N, Nx, m, E = _stats(F, N, m, E)
    n, kd = F.shape
    ids = _labels(spk_ids, n)
    n_spk = int(ids.max()) + 1 if n else 0
    W = _f64(np.atleast_2d(u))
    shift = m + _times(y, v, n_spk, kd) + _zd(z, d, n_spk, kd)
    Fh = F - Nx * shift[ids]
    with FactorEstimator(N, Fh, E) as est:
        f, A, Cm = _finish(est, W, nargout)
    if nargout == 1:
        return f
    return (f, A, Cm) if nargout == 3 else (f, update_loadings(A, Cm, W))


def estimate_z_and_d(F, N, S=None, m=None, E=None, d=0, v=0, u=0, z=0, y=0, x=0, spk_ids=None, nargout=1):
    """estimate_z_and_d.m on the host in float64: ``z`` [max label + 1, K * D], ``(z, d)`` or ``(z, a, b)``;
    ``estimate_z_and_d(a, b)`` gives ``d = b / a``."""
    if isinstance(F, Stats):
        return _resident_z_and_d(F, m, E, d, v, u, y, x, spk_ids, nargout)
    if m is None:
        return np.asarray(N, dtype=np.float64) / np.asarray(F, dtype=np.float64)
    F, N, Nx, m, E = _stats(F, N, m, E)
    n, kd = F.shape
    ids = _labels(spk_ids, n)
    n_spk = int(ids.max()) + 1 if n else 0
    dv = np.broadcast_to(np.asarray(d, dtype=np.float64).reshape(-1), (kd,))
    Ns = _speaker_sums(Nx, ids, n_spk)
    Fs = _speaker_sums(F - _times(x, u, n, kd) * Nx, ids, n_spk) - (m + _times(y, v, n_spk, kd)) * Ns
    L = 1.0 + Ns / E * dv ** 2
    zz = Fs / E * dv / L
    present = np.zeros(n_spk, dtype=bool)
    present[ids] = True
    zz[~present] = 0.0
    if nargout == 1:
        return zz
    a = ((1.0 / L + zz ** 2) * Ns)[present].sum(axis=0)
    b = (zz * Fs)[present].sum(axis=0)
    return (zz, a, b) if nargout == 3 else (zz, b / a)


def linear_scoring(F, N, S=None, m=None, E=None, d=0, v=0, u=0, z=0, y=0, x=0, scores=None):
    """linear_scoring.m on the host in float64: -> [n_models, n_segments], the models ``z d + y v`` divided by E against the
    channel-compensated, count-normalised first-order statistics of the segments."""
    if isinstance(F, Stats):
        return score_trials(F, None, m, E, d, v, u, z, y, _f64(_rows(x, F.n, np.atleast_2d(u).shape[0])), mode="linear")
    F, N, Nx, m, E = _stats(F, N, m, E)
    n, kd = F.shape
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    n_mod = y.shape[0]
    dv = np.broadcast_to(np.asarray(d, dtype=np.float64).reshape(-1), (kd,))
    M = (_rows(z, n_mod, kd) * dv + _times(y, v, n_mod, kd)) / E
    Fc = (F - (m + _times(x, u, n, kd)) * Nx) / N.sum(axis=1, keepdims=True)
    return M @ Fc.T


def _ubm_m_E(ubm):
    """(m, E) supervectors [K * D] of a UBM given as ``as_ubm`` takes it."""
    if isinstance(ubm, GMM):
        _, mu, sg = ubm.params()
        var = np.asarray(sg, dtype=np.float64) ** 2
    elif hasattr(ubm, "keys"):
        mu, var = ubm["means"], ubm["variances"]
    else:
        mu, var = ubm[1], ubm[2]
    return np.asarray(mu, dtype=np.float64).reshape(-1), np.asarray(var, dtype=np.float64).reshape(-1)


def random_loadings(n_rows, E, seed=0):
    """The sc_* scripts' random start ``randn(n, K D) * sum(E) * 0.001`` from ``numpy.random.RandomState(seed)`` -- not MATLAB's
    stream: a run here starts from other numbers than a run of the scripts."""
    E = np.asarray(E, dtype=np.float64).reshape(-1)
    return np.random.RandomState(seed).randn(int(n_rows), E.size) * E.sum() * 0.001


def train_v(F, N, spk_ids, ubm, ny=300, niter=10, v0=None, seed=0):
    """sc_train_v_from_files.m: ``niter`` rounds of ``[y, v] = estimate_y_and_v(F, N, S, m, E, 0, v, 0, 0, 0, 0, spk_ids)`` from the
    random start (or ``v0``), as ONE device call.  -> v [ny, K * D]."""
    if isinstance(F, Stats):
        m, E = _ubm_m_E(ubm)
        with centred(F, m, E, spk_ids, "speakers") as est:
            return est.train(random_loadings(ny, E, seed) if v0 is None else v0, niter)[0]
    m, E = _ubm_m_E(ubm)
    F, N, Nx, m, E = _stats(F, N, m, E)
    ids = _labels(spk_ids, F.shape[0])
    present = np.unique(ids)
    n_spk = int(ids.max()) + 1
    Ns = _speaker_sums(N, ids, n_spk)
    Fs = _speaker_sums(F, ids, n_spk) - m * _speaker_sums(Nx, ids, n_spk)
    v = random_loadings(ny, E, seed) if v0 is None else v0
    with FactorEstimator(Ns[present], Fs[present], E) as est:
        return est.train(v, niter)[0]


def train_u(F, N, spk_ids, ubm, v, nx=300, niter=10, u0=None, seed=0):
    """sc_train_u_from_files.m: y once from ``v``, then ``niter`` rounds of ``[x, u] = estimate_x_and_u(...)`` with that y fixed, as
    one device call.  -> u [nx, K * D]."""
    if isinstance(F, Stats):
        m, E = _ubm_m_E(ubm)
        y = estimate_y_and_v(F, None, None, m, E, 0, v, 0, 0, 0, 0, spk_ids)
        with centred(F, m, E, spk_ids, "sessions", v=v, y=y) as est:
            return est.train(random_loadings(nx, E, seed) if u0 is None else u0, niter)[0]
    m, E = _ubm_m_E(ubm)
    y = estimate_y_and_v(F, N, None, m, E, 0, v, 0, 0, 0, 0, spk_ids)
    F, N, Nx, m, E = _stats(F, N, m, E)
    ids = _labels(spk_ids, F.shape[0])
    Fh = F - Nx * (m + y @ _f64(np.atleast_2d(v)))[ids]
    u = random_loadings(nx, E, seed) if u0 is None else u0
    with FactorEstimator(N, Fh, E) as est:
        return est.train(u, niter)[0]


def train_d(F, N, spk_ids, ubm, v, u, niter=10, d0=None, seed=0):
    """sc_train_d_from_files.m: y and x once, then ``niter`` rounds of ``[z, d] = estimate_z_and_d(...)`` (host).  -> d [K * D]."""
    if isinstance(F, Stats):
        m, E = _ubm_m_E(ubm)
        y = estimate_y_and_v(F, None, None, m, E, 0, v, 0, 0, 0, 0, spk_ids)
        x = estimate_x_and_u(F, None, None, m, E, 0, v, u, 0, y, 0, spk_ids)
        d = random_loadings(1, E, seed)[0] if d0 is None else np.asarray(d0, dtype=np.float64).reshape(-1)
        with centred(F, m, E, spk_ids, "speakers", v=v, u=u, y=y, x=x) as est:       # Fc_g does not depend on d: centred once
            return est.z_and_d(d, n_iter=int(niter))[0]
    m, E = _ubm_m_E(ubm)
    y = estimate_y_and_v(F, N, None, m, E, 0, v, 0, 0, 0, 0, spk_ids)
    x = estimate_x_and_u(F, N, None, m, E, 0, v, u, 0, y, 0, spk_ids)
    d = random_loadings(1, E, seed)[0] if d0 is None else np.asarray(d0, dtype=np.float64).reshape(-1)
    for _ in range(int(niter)):
        _, d = estimate_z_and_d(F, N, None, m, E, d, v, u, 0, y, x, spk_ids, nargout=2)
    return d


def score_dot_product(trn, tst, ubm, v, u, d):
    """sc_score_dot_product.m: every enrolment segment a speaker of its own; y and x jointly on the stacked [v; u], z, the test
    segments' channel factors against the UBM, then ``linear_scoring``.  ``trn`` / ``tst``: ``(F, N)`` pairs or mappings with
    those keys.  -> scores [n_enrolment, n_test]."""
    m, E = _ubm_m_E(ubm)
    tF, tN = _pair(trn)
    sF, sN = _pair(tst)
    v = _f64(np.atleast_2d(v))
    u = _f64(np.atleast_2d(u))
    ny = v.shape[0]
    vu = np.vstack([v, u])
    trn_ids = np.arange(_n_rows(tF, tN))
    tst_ids = np.arange(_n_rows(sF, sN))
    yx = estimate_y_and_v(tF, tN, None, m, E, d, vu, 0, 0, 0, 0, trn_ids)
    trn_z = estimate_z_and_d(tF, tN, None, m, E, d, vu, 0, 0, yx, 0, trn_ids)
    tst_x = estimate_x_and_u(sF, sN, None, m, E, d, v, u, 0, 0, 0, tst_ids)
    return linear_scoring(sF, sN, None, m, E, d, v, u, trn_z, yx[:, :ny], tst_x)


# ---- trial scoring on the device (csrc/jfa_score.hip) ----

def score_trials(F, N, m, E, d, v, u, z, y, x=None, mode="integrated", mask=None, return_counts=False):
    """The score matrix [J, T] of J models against T test segments in ONE device call, float64, row orientation as the rest of
    this module: raw statistics ``F`` [T, K * D] (not centred) and ``N`` [T, K], ``m``, ``E`` [K * D], ``d`` [K * D] (or None / 0),
    ``v`` [Ry, K * D], ``u`` [Ru, K * D], the models' ``z`` [J, K * D] (or None / 0) and ``y`` [J, Ry].
    ``mode`` "integrated": kscore_famous_19.m, the channel factors integrated out; "linear": linear_scoring.m, which needs the
    segments' channel factors ``x`` [T, Ru].  ``mask``: [J, T], where it is 0 the score is 0.0 exactly.  A segment of no frames
    scores 0.0 against every model.  ``return_counts``: -> (scores, {"empty_segments": n, "bad_segments": n})."""
    from . import _lib
    if mode not in ("integrated", "linear"):
        raise ValueError("mode is 'integrated' or 'linear', got %r" % (mode,))
    stats = F if isinstance(F, Stats) else None
    if stats is not None:
        T, K, kd = stats.n, stats.K, stats.K * stats.D
    else:
        F = _f64(np.atleast_2d(F))
        N = _f64(np.atleast_2d(N))
        T, K = N.shape
        if K < 1 or F.shape[0] != T or F.shape[1] % K:
            raise ValueError("expected N [T, K] and F [T, K * D]; got %r and %r" % (N.shape, F.shape))
        kd = F.shape[1]
    m, E = _f64(np.reshape(m, -1), (kd,), "m"), _f64(np.reshape(E, -1), (kd,), "E")
    v = _f64(np.atleast_2d(v))
    u = _f64(np.atleast_2d(u))
    y = _f64(np.atleast_2d(y))
    J = y.shape[0]
    if v.shape[1] != kd or u.shape[1] != kd or y.shape[1] != v.shape[0]:
        raise ValueError("expected v [Ry, %d], u [Ru, %d], y [J, Ry]; got %r, %r, %r" % (kd, kd, v.shape, u.shape, y.shape))

    def optional(a, shape, name):
        if a is None or (np.ndim(a) == 0 and a == 0):
            return None
        return _f64(np.reshape(a, shape), shape, name)

    d = optional(d, (kd,), "d")
    z = optional(z, (J, kd), "z")
    x = optional(x, (T, u.shape[0]), "x")
    if mask is not None:
        mask = np.asarray(mask)
        if mask.shape != (J, T):
            raise ValueError("a mask of shape %r for a score matrix [%d, %d]: pass one value per (model, segment) pair" % (mask.shape, J, T))
        mask = np.ascontiguousarray(mask != 0, dtype=np.uint8)
    out = np.zeros((J, T))
    empty, bad = C.c_int64(0), C.c_int64(0)
    opt = lambda a: _lib.as_dp(a) if a is not None else None                        # noqa: E731
    mk = (mask.ctypes.data_as(C.POINTER(C.c_uint8)), J, T) if mask is not None else (None, 0, 0)
    if stats is not None:
        head = (stats._handle(), J, v.shape[0], u.shape[0], _lib.as_dp(m), _lib.as_dp(E), opt(d), _lib.as_dp(v), _lib.as_dp(u), opt(z), _lib.as_dp(y))
        if mode == "integrated":
            _lib.check(_lib.lib().sr_jfa_score_integrated_stats(*head, *mk, _lib.as_dp(out), C.byref(empty), C.byref(bad)),
                       "sr_jfa_score_integrated_stats")
        else:
            _lib.check(_lib.lib().sr_jfa_score_linear_stats(*head, opt(x), *mk, _lib.as_dp(out), C.byref(empty)), "sr_jfa_score_linear_stats")
        return (out, {"empty_segments": int(empty.value), "bad_segments": int(bad.value)}) if return_counts else out
    head = (T, J, K, kd // K, v.shape[0], u.shape[0], _lib.as_dp(N), _lib.as_dp(F), _lib.as_dp(m), _lib.as_dp(E), opt(d), _lib.as_dp(v),
            _lib.as_dp(u), opt(z), _lib.as_dp(y))
    if mode == "integrated":
        _lib.check(_lib.lib().sr_jfa_score_integrated(*head, *mk, _lib.as_dp(out), C.byref(empty), C.byref(bad)), "sr_jfa_score_integrated")
    else:
        _lib.check(_lib.lib().sr_jfa_score_linear(*head, opt(x), *mk, _lib.as_dp(out), C.byref(empty)), "sr_jfa_score_linear")
    return (out, {"empty_segments": int(empty.value), "bad_segments": int(bad.value)}) if return_counts else out


def kscore_famous_19(F, N, S=None, m=None, E=None, d=0, v=None, u=None, z=0, y=None, x=0, scores=None):
    """kscore_famous_19.m in that file's OWN orientation, which is columns (its code, not its header comment, decides):
    ``F`` [K * D, T], ``N`` [K, T], ``m``, ``E``, ``d`` [K * D] (or [K * D, 1]), ``v`` [K * D, Ry], ``u`` [K * D, Ru], ``z`` [K * D, J],
    ``y`` [Ry, J]; ``S`` and ``x`` are accepted and ignored as there; ``scores``: the mask [J, T], a score where it is 1 (None: all).
    -> [J, T].  A transposing wrapper of ``score_trials``.  Not reproduced: the reference leaves the UBM's score un-subtracted
    where a score is exactly 0."""
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    J = y.shape[1]
    zt = None if (np.ndim(z) == 0 and z == 0) else np.reshape(np.asarray(z, dtype=np.float64), (-1, J)).T
    dv = None if (np.ndim(d) == 0 and d == 0) else np.reshape(d, -1)
    mask = None if scores is None else np.asarray(scores) == 1
    if isinstance(F, Stats):                                                         # (a handle has one orientation: rows are segments)
        return score_trials(F, None, np.reshape(m, -1), np.reshape(E, -1), dv, np.atleast_2d(np.asarray(v, dtype=np.float64)).T,
                            np.atleast_2d(np.asarray(u, dtype=np.float64)).T, zt, y.T, mode="integrated", mask=mask)
    return score_trials(np.atleast_2d(np.asarray(F, dtype=np.float64)).T, np.atleast_2d(np.asarray(N, dtype=np.float64)).T, np.reshape(m, -1),
                        np.reshape(E, -1), dv, np.atleast_2d(np.asarray(v, dtype=np.float64)).T, np.atleast_2d(np.asarray(u, dtype=np.float64)).T,
                        zt, y.T, mode="integrated", mask=mask)


def score_integrated(trn, tst, ubm, v, u, d):
    """The sibling of ``score_dot_product``: the same enrolment factors (every enrolment segment a speaker of its own; y and x jointly
    on the stacked [v; u], then z), scored against the test segments' raw statistics by the integrated scorer -- no point estimate
    of the test segments' channel factors.  -> scores [n_enrolment, n_test]."""
    m, E = _ubm_m_E(ubm)
    tF, tN = _pair(trn)
    sF, sN = _pair(tst)
    v = _f64(np.atleast_2d(v))
    u = _f64(np.atleast_2d(u))
    ny = v.shape[0]
    vu = np.vstack([v, u])
    trn_ids = np.arange(_n_rows(tF, tN))
    yx = estimate_y_and_v(tF, tN, None, m, E, d, vu, 0, 0, 0, 0, trn_ids)
    trn_z = estimate_z_and_d(tF, tN, None, m, E, d, vu, 0, 0, yx, 0, trn_ids)
    return score_trials(sF, sN, m, E, d, v, u, trn_z, yx[:, :ny], mode="integrated")


def score_normalised(trn, tst, cohort, ubm, v, u, d, norm="as2", top_n=200, scorer="integrated", return_counts=False):
    """A verification run's normalised score matrix [n_enrolment, n_test]: the ``cohort`` segments (impostors; an ``(F, N)`` pair, a
    mapping or a ``Stats`` as ``trn`` and ``tst``) are enrolled as models AND used as segments, the matrices the mode needs -- (trn,
    tst), (trn, cohort), (cohort, tst) and, for "zt", (cohort, cohort) -- come from ``score_integrated`` (``scorer`` "integrated") or
    ``score_dot_product`` ("dot_product"), and ``scorenorm.normalise`` is applied to them.  ``norm``: "z", "t", "zt", "s", "as1" or
    "as2"; ``top_n``: the adaptive modes' N."""
    from . import scorenorm
    if scorer not in ("integrated", "dot_product"):
        raise ValueError("scorer is 'integrated' or 'dot_product', got %r" % (scorer,))
    if norm not in scorenorm.MODES:
        raise ValueError("norm is one of %s, got %r" % (", ".join(repr(m) for m in scorenorm.MODES), norm))
    score = score_integrated if scorer == "integrated" else score_dot_product
    S = score(trn, tst, ubm, v, u, d)
    Ez = score(trn, cohort, ubm, v, u, d) if norm != "t" else None
    Tt = score(cohort, tst, ubm, v, u, d) if norm != "z" else None
    Zt = score(cohort, cohort, ubm, v, u, d) if norm == "zt" else None
    return scorenorm.normalise(S, norm, Ez, Tt, Zt, top_n=top_n if norm in ("as1", "as2") else None, return_counts=return_counts)
