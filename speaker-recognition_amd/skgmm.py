"""Full-covariance GMMs -- API mirror of the reference's ``src/gui/skgmm.py`` (``GMMSet`` :11-39), the speaker model its shipped
``ModelInterface`` uses (interface.py:24: scikit-learn's ``GaussianMixture(32)``, full covariance).

``GMM`` is the subset of ``sklearn.mixture.GaussianMixture`` the reference and its users touch, computed by this library: EM in
float64 on the device (csrc/gmm_full_fit.hip) exactly as ``GaussianMixture.fit`` runs it with ``covariance_type='full'`` and
``n_init=1``, and scoring on the fp32 matrix cores (csrc/gmm_full.hip).  Parameters use scikit-learn's layout, so they convert 1:1.

Differences from scikit-learn, all deliberate:
  * ``init_params='kmeans'`` takes its labels from this library's seeded k-means (k-means|| + Lloyd, csrc/kmeans_init.hip), not
    from scikit-learn's ``KMeans``; ``random_state=None`` means the fixed seed ``DEFAULT_SEED``, so fits are reproducible;
  * explicit initialisation needs all three of ``weights_init``, ``means_init``, ``precisions_init``;
  * ``score_samples`` is fp32 arithmetic (returned as float64); ``max_iter >= 1``; ``n_init`` must be 1.
Diagonal models are ``pygmm.GMM`` / ``gmmset.GMMSet`` (the reference's C++ back-end).
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
from scipy.linalg import solve_triangular

from . import _lib
from ._lib import lib
from .core import Batch

DEFAULT_SEED = 0
MAX_DIM = 64
_ILL_DEFINED = "Fitting the mixture model failed"


class ConvergenceWarning(UserWarning):
    """The fit stopped at max_iter before the lower bound settled (scikit-learn's ConvergenceWarning)."""


def _precision_cholesky_from_covariances(covariances):
    """P_k = inv(cholesky(cov_k))^T, upper triangular (sklearn.mixture._gaussian_mixture._compute_precision_cholesky)."""
    cov = np.asarray(covariances, dtype=np.float64)
    out = np.empty_like(cov)
    for k, c in enumerate(cov):
        try:
            L = np.linalg.cholesky(c)
        except np.linalg.LinAlgError:
            raise ValueError(_ILL_DEFINED + " because some components have ill-defined empirical covariance (for instance "
                             "caused by singleton or collapsed samples). Try to decrease the number of components, increase "
                             "reg_covar, or scale the input data.") from None
        out[k] = solve_triangular(L, np.eye(c.shape[0]), lower=True).T
    return out


def _precision_cholesky_from_precisions(precisions):
    """Upper triangular P_k with P_k P_k^T = precision_k (sklearn's _compute_precision_cholesky_from_precisions: the lower Cholesky
    factor of the reversed matrix, reversed)."""
    prec = np.asarray(precisions, dtype=np.float64)
    out = np.empty_like(prec)
    for k, p in enumerate(prec):
        if not np.allclose(p, p.T):
            raise ValueError("'precisions' should be symmetric, positive-definite")
        try:
            out[k] = np.linalg.cholesky(p[::-1, ::-1])[::-1, ::-1]
        except np.linalg.LinAlgError:
            raise ValueError("'precisions' should be symmetric, positive-definite") from None
    return out


def _raise_lib(what):
    msg = _lib.last_error()
    if msg.startswith(_ILL_DEFINED):
        raise ValueError(msg)
    raise _lib.SRError("%s failed: %s" % (what, msg))


class GMM(object):
    """GaussianMixture(covariance_type='full') on the device."""

    def __init__(self, n_components=1, *, covariance_type="full", tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1,
                 init_params="kmeans", random_state=None, weights_init=None, means_init=None, precisions_init=None):
        if covariance_type != "full":
            raise ValueError("skgmm.GMM supports covariance_type='full' only (got %r); diagonal models are pygmm.GMM / "
                             "gmmset.GMMSet" % (covariance_type,))
        if init_params != "kmeans":
            raise ValueError("init_params must be 'kmeans' (got %r), or pass weights_init / means_init / precisions_init"
                             % (init_params,))
        if n_init != 1:
            raise ValueError("n_init must be 1 (got %r)" % (n_init,))
        if int(n_components) < 1:
            raise ValueError("n_components must be >= 1 (got %r)" % (n_components,))
        if int(max_iter) < 1:
            raise ValueError("max_iter must be >= 1 (got %r)" % (max_iter,))
        if not (tol >= 0 and reg_covar >= 0):
            raise ValueError("tol and reg_covar must be >= 0")
        if random_state is not None and (not isinstance(random_state, (int, np.integer)) or random_state < 0):
            raise ValueError("random_state must be None or an int >= 0 (got %r)" % (random_state,))
        given = [v is not None for v in (weights_init, means_init, precisions_init)]
        if any(given) and not all(given):
            raise ValueError("give weights_init, means_init and precisions_init together, or none of them")
        self.n_components = int(n_components)
        self.covariance_type = covariance_type
        self.tol, self.reg_covar, self.max_iter, self.n_init = float(tol), float(reg_covar), int(max_iter), 1
        self.init_params, self.random_state = init_params, random_state
        self.weights_init, self.means_init, self.precisions_init = weights_init, means_init, precisions_init
        self._h = None
        self._version = 0

    # ---- parameters ----
    @property
    def precisions_(self):
        P = self.precisions_cholesky_
        return np.einsum("kij,klj->kil", P, P)

    def _set_params(self, weights, means, covariances, prec_chol):
        self.weights_, self.means_ = weights, means
        self.covariances_, self.precisions_cholesky_ = covariances, prec_chol
        self._version += 1

    @classmethod
    def from_arrays(cls, weights, means, covariances) -> "GMM":
        """A model from sklearn-layout parameters (weights [K], means [K][D], covariances [K][D][D]); no device work."""
        w = np.ascontiguousarray(weights, dtype=np.float64)
        mu = np.ascontiguousarray(means, dtype=np.float64)
        cov = np.ascontiguousarray(covariances, dtype=np.float64)
        K, D = mu.shape
        if w.shape != (K,) or cov.shape != (K, D, D):
            raise ValueError("shapes: weights [K], means [K][D], covariances [K][D][D]")
        if D > MAX_DIM:
            raise ValueError("full-covariance models support at most %d dims (got %d)" % (MAX_DIM, D))
        g = cls(K)
        g._set_params(w, mu, cov, _precision_cholesky_from_covariances(cov))
        g.converged_, g.n_iter_, g.lower_bound_ = True, 0, float("nan")
        return g

    def _check_X(self, X, D=None):
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("expected a 2-D [n_samples, n_features] array, got shape %r" % (X.shape,))
        if X.shape[1] > MAX_DIM:
            raise ValueError("full-covariance models support at most %d dims (got %d)" % (MAX_DIM, X.shape[1]))
        if D is not None and X.shape[1] != D:
            raise ValueError("X has %d features, the model %d" % (X.shape[1], D))
        return np.ascontiguousarray(X)

    def handle(self):
        """The device-side model (SRFullGMM *), built from the host parameters on first use."""
        if self._h is None:
            if not hasattr(self, "means_"):
                raise ValueError("this GMM is not fitted yet")
            w, mu, P = (np.ascontiguousarray(a, dtype=np.float64) for a in (self.weights_, self.means_, self.precisions_cholesky_))
            K, D = mu.shape
            h = lib().sr_fullgmm_create(K, D, _lib.as_dp(w), _lib.as_dp(mu), _lib.as_dp(P))
            if not h:
                _raise_lib("sr_fullgmm_create")
            self._h = C.c_void_p(h)
        return self._h

    # ---- training ----
    def fit(self, X, y=None) -> "GMM":
        X = self._check_X(X)
        n, D = X.shape
        K = self.n_components
        if n < K:
            raise ValueError("Expected n_samples >= n_components but got n_components = %d, n_samples = %d" % (K, n))
        h, init = self._new_handle(D)
        try:
            seed = DEFAULT_SEED if self.random_state is None else int(self.random_state)
            prm = _lib.FullFitParams(self.tol, self.reg_covar, self.max_iter, 1 if init else 0, seed)
            st = _lib.FullFitStats()
            if lib().sr_fullgmm_fit(h, _lib.as_dp(X), n, D, C.byref(prm), C.byref(st)) < 0:
                _raise_lib("sr_fullgmm_fit")
            fitted = self._read_handle(h, D)
        except BaseException:
            lib().sr_fullgmm_free(h)
            raise
        self._adopt(h, fitted, st)
        return self

    def _new_handle(self, D):
        """A fresh device-side model for a fit on D columns: the explicit initialisation when one was given, else no parameters.
        -> (handle, init_given)"""
        K = self.n_components
        init = self.weights_init is not None
        if init:
            w = np.ascontiguousarray(self.weights_init, dtype=np.float64)
            mu = np.ascontiguousarray(self.means_init, dtype=np.float64)
            if w.shape != (K,) or mu.shape != (K, D):
                raise ValueError("weights_init must be [%d], means_init [%d, %d]" % (K, K, D))
            prec = np.asarray(self.precisions_init, dtype=np.float64)
            if prec.shape != (K, D, D):
                raise ValueError("precisions_init must be [%d, %d, %d]" % (K, D, D))
            P = np.ascontiguousarray(_precision_cholesky_from_precisions(prec))
            h = lib().sr_fullgmm_create(K, D, _lib.as_dp(w), _lib.as_dp(mu), _lib.as_dp(P))
        else:
            h = lib().sr_fullgmm_create(K, D, None, None, None)
        if not h:
            _raise_lib("sr_fullgmm_create")
        return C.c_void_p(h), init

    def _read_handle(self, h, D):
        """-> (weights, means, covariances, precisions_cholesky) of the fitted handle ``h`` (``sr_fullgmm_get``)"""
        K = self.n_components
        w, mu = np.empty(K), np.empty((K, D))
        cov, P = np.empty((K, D, D)), np.empty((K, D, D))
        _lib.check(lib().sr_fullgmm_get(h, _lib.as_dp(w), _lib.as_dp(mu), _lib.as_dp(cov), _lib.as_dp(P)), "sr_fullgmm_get")
        return w, mu, cov, P

    def _adopt(self, h, fitted, st):
        """Become the fitted model: the handle ``h``, its parameters as ``_read_handle`` gave them, the fit's ``FullFitStats``."""
        self._free()
        self._h = h
        self._set_params(*fitted)
        self.converged_, self.n_iter_, self.lower_bound_ = bool(st.converged), int(st.n_iter), float(st.lower_bound)
        if not self.converged_:
            warnings.warn("Best performing initialization did not converge. Try different init parameters, or increase "
                          "max_iter, tol, or check for degenerate data.", ConvergenceWarning)

    # ---- scoring ----
    def score_samples(self, X) -> np.ndarray:
        """Per-frame log-likelihood (fp32 on the device, returned as float64)."""
        X = self._check_X(X, np.asarray(self.means_).shape[1] if hasattr(self, "means_") else None)
        s = FullSet([self])
        _, _, fll = s.score(Batch.from_features(X), frame_ll=True)
        return fll[0].astype(np.float64)

    def score(self, X, y=None) -> float:
        """Mean per-frame log-likelihood (as sklearn's score)."""
        return float(np.mean(self.score_samples(X)))

    # ---- lifetime / pickling: the float64 host parameters travel, the device handle is rebuilt on use ----
    def _free(self):
        if self._h is not None:
            try:
                lib().sr_fullgmm_free(self._h)
            except Exception:
                pass
            self._h = None

    def __del__(self):
        self._free()

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_h"] = None
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)
        self._h = None


def fit_many(gmms, Xs):
    """Fit the unfitted models ``gmms[s]`` on the matrices ``Xs[s]`` in one batched device EM (``sr_fullgmm_fit_batch``): all
    models share ``n_components`` and all matrices the feature width; frame counts, ``tol``, ``max_iter``, ``reg_covar``,
    ``random_state`` and explicit initialisations are per model.  Every fitted model ends up exactly as ``gmms[s].fit(Xs[s])``
    leaves it, bit for bit -- ``weights_``, ``means_``, ``covariances_``, ``precisions_cholesky_``, ``converged_``, ``n_iter_``,
    ``lower_bound_``, a device handle -- with a ``ConvergenceWarning`` per model that stopped at ``max_iter``.

    -> a list with one entry per model: ``None`` for a fitted model, and for a model whose fit failed on the device (an
    ill-defined empirical covariance) the ``ValueError`` that ``fit`` would have raised, as an object, not raised; that model is
    left as it was.  Bad arguments (lengths, shapes, too few rows, non-finite data) raise for the call as a whole, before
    any model changes."""
    gmms, Xs = list(gmms), list(Xs)
    if len(gmms) != len(Xs):
        raise ValueError("fit_many: %d models but %d matrices" % (len(gmms), len(Xs)))
    if not gmms:
        return []
    if len(set(id(g) for g in gmms)) != len(gmms):
        raise ValueError("fit_many: a model appears twice")
    K = gmms[0].n_components
    Xs = [g._check_X(X) for g, X in zip(gmms, Xs)]
    D = Xs[0].shape[1]
    for s, (g, X) in enumerate(zip(gmms, Xs)):
        if g.n_components != K:
            raise ValueError("fit_many: model %d has %d components, model 0 has %d" % (s, g.n_components, K))
        if X.shape[1] != D:
            raise ValueError("fit_many: matrix %d has %d features, matrix 0 has %d" % (s, X.shape[1], D))
        if X.shape[0] < K:
            raise ValueError("Expected n_samples >= n_components but got n_components = %d, n_samples = %d (model %d)"
                             % (K, X.shape[0], s))
    S = len(gmms)
    handles = []
    try:
        prm = (_lib.FullFitParams * S)()
        for s, g in enumerate(gmms):
            h, init = g._new_handle(D)
            handles.append(h)
            seed = DEFAULT_SEED if g.random_state is None else int(g.random_state)
            prm[s] = _lib.FullFitParams(g.tol, g.reg_covar, g.max_iter, 1 if init else 0, seed)
        off = np.zeros(S + 1, dtype=np.int64)
        np.cumsum([X.shape[0] for X in Xs], out=off[1:])
        Xall = Xs[0] if S == 1 else np.ascontiguousarray(np.concatenate(Xs, axis=0))
        st = (_lib.FullFitStats * S)()
        status = np.zeros(S, dtype=np.int32)
        arr = (C.c_void_p * S)(*[h.value for h in handles])
        if lib().sr_fullgmm_fit_batch(arr, S, _lib.as_dp(Xall), _lib.as_i64p(off), D, prm, st, _lib.as_i32p(status)) < 0:
            _raise_lib("sr_fullgmm_fit_batch")
        fitted = [None] * S
        errors = [None] * S
        for s in range(S):
            if status[s] != 0:
                errors[s] = ValueError(lib().sr_fullgmm_fit_batch_error(s).decode("utf-8", "replace"))
                continue
            fitted[s] = gmms[s]._read_handle(handles[s], D)
    except BaseException:
        for h in handles:
            lib().sr_fullgmm_free(h)
        raise
    for s, g in enumerate(gmms):
        if fitted[s] is None:
            lib().sr_fullgmm_free(handles[s])
            continue
        g._adopt(handles[s], fitted[s], st[s])
    return errors


class FullSet(object):
    """S trained full-covariance models of one dimension packed once on the device; every utterance of a batch against all of them
    in one launch."""

    def __init__(self, gmms):
        gmms = list(gmms)
        if not gmms:
            raise ValueError("empty model set")
        self._gmms = gmms                              # (keeps the handles alive)
        arr = (C.c_void_p * len(gmms))(*[g.handle().value for g in gmms])
        h = lib().sr_fullset_create(arr, len(gmms))
        if not h:
            _raise_lib("sr_fullset_create")
        self._h = C.c_void_p(h)
        self.size = len(gmms)

    def score(self, batch: Batch, frame_ll=False):
        """-> (sums [U][S] float64, argmax [U], per-frame LL [S][n] fp32 or None)."""
        U, n = batch.n_utt, batch.n_rows
        sums = np.zeros((U, self.size), np.float64)
        arg = np.zeros(U, np.int32)
        fll = np.zeros((self.size, n), np.float32) if frame_ll else None
        _lib.check(lib().sr_fullset_score_batch(self._h, batch._h, _lib.as_dp(sums), _lib.as_i32p(arg),
                                                _lib.as_fp(fll) if frame_ll else None), "sr_fullset_score_batch")
        return sums, arg, fll

    def predict_pcm(self, extractor, pcm: Batch, nd=0, out=None):
        """Fused decision on resident PCM (``core.MfccExtractor.predict_batch`` for full-covariance sets): MFCC (+ the
        extractor's LPC columns, or ``nd`` orders of deltas) -> scoring -> per-utterance sums and argmax on the device -> one copy
        back.  -> (sums float64[U, S], argmax int32[U]).  The sums are ``score``'s bits on the same features; argmax is the
        first maximum of sums / frames (as ``GMMSet.predict``), -1 for an utterance too short to yield a frame.  ``out`` =
        (float64[U, S], int32[U]) C-contiguous arrays to fill instead of fresh ones."""
        U, S = pcm.n_utt, self.size
        if out is None:
            sums = np.zeros((U, S), dtype=np.float64)
            arg = np.full(U, -1, dtype=np.int32)
        else:
            sums, arg = out
            if sums.shape != (U, S) or sums.dtype != np.float64 or not sums.flags.c_contiguous or arg.shape != (U,) or \
                    arg.dtype != np.int32 or not arg.flags.c_contiguous:
                raise ValueError("out must be (float64[%d, %d], int32[%d]), C-contiguous" % (U, S, U))
        _lib.check(lib().sr_fullset_predict_pcm_batch(extractor._h, self._h, pcm._h, int(nd), _lib.as_dp(sums), _lib.as_i32p(arg)),
                   "sr_fullset_predict_pcm_batch")
        return sums, arg

    def timeline(self, batch: Batch, window, hop, threshold=0.0, smooth="hold", switch_penalty=None, min_windows=1, scores=False):
        """``core.ModelSet.timeline`` for a full-covariance set (sr_fullset_timeline_batch): every column is a speaker (no "nobody"
        state).  -> a list of int32 label arrays, one per recording[, path scores, window sums per recording]."""
        from .core import _timeline_args, _timeline_call
        tail = _timeline_args(window, hop, None, threshold, smooth, switch_penalty, min_windows)
        tail = tail[:2] + tail[3:]                     # (no bg argument)
        return _timeline_call(lib().sr_fullset_timeline_batch, "sr_fullset_timeline_batch", (self._h, batch._h), tail,
                              np.diff(batch.offsets()), self.size, scores)

    def __len__(self):
        return self.size

    def __del__(self):
        try:
            if self._h is not None:
                lib().sr_fullset_free(self._h)
        except Exception:
            pass


class GMMSet(object):
    """One full-covariance GMM per speaker (src/gui/skgmm.py:11-39); the speaker of an utterance is the arg max of the per-frame
    mean log-likelihood, ties to the first speaker.  ``gmm_kwargs`` go to every ``GMM``."""

    def __init__(self, gmm_order=32, **gmm_kwargs):
        self.gmms = []
        self.gmm_order = gmm_order
        self.y = []
        self.gmm_kwargs = gmm_kwargs
        self._set, self._set_key = None, None

    def fit_new(self, x, label):
        self.y.append(label)
        gmm = GMM(self.gmm_order, **self.gmm_kwargs)
        gmm.fit(x)
        self.gmms.append(gmm)

    def fit_many(self, xs, labels):
        """``fit_new`` for every (x, label) pair, the fits in one batched device EM (``skgmm.fit_many``): the same models bit
        for bit, appended in order.  A speaker whose fit fails raises its ``ValueError`` with the set in the state a loop of
        ``fit_new`` leaves: the earlier speakers in ``gmms``, their labels and the failing one in ``y``.  Arguments the batch
        refuses as a whole (a matrix ``fit`` would refuse, matrices of different widths) go through that loop itself, which
        raises where it always did."""
        xs, labels = list(xs), list(labels)
        if len(xs) != len(labels):
            raise ValueError("fit_many: %d matrices but %d labels" % (len(xs), len(labels)))
        gmms = [GMM(self.gmm_order, **self.gmm_kwargs) for _ in labels]
        try:
            errors = fit_many(gmms, xs)
        except ValueError:
            # an argument error, raised before any model changed.  Device errors are _lib.SRError, a RuntimeError, and must
            # never land here: a failed batched fit is not to be answered by a second, sequential one
            for x, label in zip(xs, labels):
                self.fit_new(x, label)
            return
        for gmm, label, err in zip(gmms, labels, errors):
            self.y.append(label)
            if err is not None:
                raise err
            self.gmms.append(gmm)

    def gmm_score(self, gmm, x):
        """Summed per-frame log-likelihood of ``x`` under one model."""
        return float(np.sum(gmm.score_samples(x)))

    def before_pickle(self):
        self._set, self._set_key = None, None

    def after_pickle(self):
        pass

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_set"], d["_set_key"] = None, None
        return d

    def _full_set(self):
        # packed once; rebuilt only when the list of models (or a model's parameters) changes
        key = tuple((id(g), g._version) for g in self.gmms)
        if self._set is None or self._set_key != key:
            self._set = FullSet(self.gmms)
            self._set_key = key
        return self._set

    def predict_scores(self, feats):
        """[U][S] per-frame mean log-likelihood of every utterance under every speaker, one launch."""
        feats = [np.asarray(f, dtype=np.float64) for f in feats]
        sums, _, _ = self._full_set().score(Batch.from_features(feats))
        lens = np.array([len(f) for f in feats], dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return sums / lens[:, None]

    def predict(self, feats):
        """Batched predict_one: every utterance of the list against every speaker in one launch."""
        feats = list(feats)
        if not feats:
            return []
        scores = self.predict_scores(feats)
        out = []
        for u, f in enumerate(feats):
            if len(f) == 0:
                out.append(None)
                continue
            out.append(self.y[int(np.argmax(scores[u]))])        # (argmax: the first maximum)
        return out

    def predict_one(self, x):
        return self.predict([x])[0]
