"""Score calibration and fusion on the device (csrc/calib.hip through ``sr_calib_*``): the last link of a verification run, from a
normalised score matrix to log-likelihood ratios a threshold can be set on from a prior and costs.

Prior-weighted linear logistic regression (Bruemmer's FoCal / BOSARIS).  With S systems' scores ``X`` [S, n], labels 1 (target), 0
(non-target) or negative (not a trial: skipped everywhere and counted; its scores may hold anything), ``theta = (w_1 .. w_S, b)``,
``z_i = sum_s w_s X[s, i] + b``, ``tau = ln(P / (1 - P))`` for the training prior P and ``sp(a) = max(a, 0) + log1p(exp(-|a|))``:

    f(theta) = (1 / ln 2) [P / n_t sum_tar sp(-(z_i + tau)) + (1 - P) / n_n sum_non sp(z_i + tau)] + ridge / 2 sum_s w_s^2

``Calibrator.fit`` minimises f by damped Newton steps on the device (a pass is one streaming evaluation of f, its gradient and its
Hessian; the decisions are taken on the device too); ``transform`` applies the affine map.  One system calibrates, several fuse; a
quality measure, such as a duration, is just another row of ``scores``.  The ridge is on the weights only, never on the offset.

``cllr`` is f at S = 1, theta = (1, 0), P = 0.5, ridge = 0: 0 for perfect log-likelihood ratios, 1 for llr = 0, above 1 for scores
that mislead.  ``error_counts`` and ``act_dcf`` count misses and false alarms at thresholds on the device ("accept iff llr >= thr");
``bayes_threshold`` and ``min_cllr`` are host numpy (one sort), like ``scorenorm.eer`` / ``min_dcf``.  Float64 throughout; there is no
CPU path for the device calls."""
from __future__ import annotations

import ctypes as C

import numpy as np

MAX_THRESHOLDS = 16          # of one device call; error_counts takes any number in groups of as many
_HEAD = 16          # the state's header (include/pygmm_hip.h: sr_calib_train)


def _labels(labels):
    lab = np.asarray(labels)
    if lab.dtype == np.bool_:
        lab = lab.astype(np.int8)
    if not (np.issubdtype(lab.dtype, np.integer) or np.issubdtype(lab.dtype, np.floating)):
        raise ValueError("labels are numbers: 1 target, 0 non-target, negative not a trial; got dtype %s" % lab.dtype)
    if np.issubdtype(lab.dtype, np.floating):
        if np.isnan(lab).any():
            raise ValueError("labels hold a NaN; mark a trial to skip with a negative value")
        if (lab != np.round(lab)).any():
            raise ValueError("labels are whole numbers: 1 target, 0 non-target, negative not a trial")
    return np.where(lab < 0, -1, np.minimum(lab, 2)).astype(np.int8)           # (2: the library refuses a label above 1 by its index)


def _stack(scores, trial_shape=None, stacked=None):
    """-> (X [S, n] float64 contiguous, the trial shape, whether the systems came on an axis of their own).  ``scores``: a vector
    [n]; an array [S, n]; a list of S arrays of one shape (score matrices [J, T]); or, with ``trial_shape`` (the labels' shape)
    known, an array of exactly that shape: one system."""
    if isinstance(scores, (list, tuple)) and len(scores) and np.ndim(scores[0]) >= 1:
        mats = [np.asarray(m, dtype=np.float64) for m in scores]
        if any(m.shape != mats[0].shape for m in mats):
            raise ValueError("expected every system's scores in one shape, got %s" % ", ".join(str(m.shape) for m in mats))
        shape, single = mats[0].shape, False
        X = np.stack([m.reshape(-1) for m in mats])
    else:
        a = np.asarray(scores, dtype=np.float64)
        if a.ndim == 0:
            raise ValueError("expected scores as a vector [n], an array [S, n] or a list of S score matrices, got a scalar")
        if trial_shape is not None:
            single = a.shape == tuple(trial_shape)
        elif stacked is not None:
            single = not stacked
        else:
            single = a.ndim == 1
        shape = a.shape if single else a.shape[1:]
        X = a.reshape(1, -1) if single else a.reshape(a.shape[0], -1)
    if trial_shape is not None and tuple(shape) != tuple(trial_shape):
        raise ValueError("expected scores of the labels' shape %r, one array per system or stacked on a first axis; got trials of shape %r"
                         % (tuple(trial_shape), tuple(shape)))
    return np.ascontiguousarray(X), tuple(shape), not single


def _counts(c):
    return {"targets": int(c[0]), "non_targets": int(c[1]), "skipped": int(c[2])}


def evaluate(scores, labels, theta, prior=0.5, ridge=0.0):
    """One device pass at ``theta`` [S + 1] -> (f, g [S + 1], H [S + 1, S + 1], counts): the objective of the module text, its gradient
    and its Hessian, and the numbers of targets, non-targets and skipped entries."""
    from . import _lib
    lab = _labels(labels)
    X = _stack(scores, lab.shape)[0]
    S, n = X.shape
    th = np.ascontiguousarray(theta, dtype=np.float64).reshape(-1)
    if th.shape[0] != S + 1:
        raise ValueError("expected theta as %d weights and the offset, got %d values" % (S, th.shape[0]))
    lab = np.ascontiguousarray(lab.reshape(-1))
    f = C.c_double()
    g, H = np.zeros(S + 1), np.zeros((S + 1, S + 1))
    cnt = (C.c_int64 * 3)()
    _lib.check(_lib.lib().sr_calib_eval(S, n, _lib.as_dp(X), _lib.as_i8p(lab), float(prior), float(ridge), _lib.as_dp(th), C.byref(f),
                                        _lib.as_dp(g), _lib.as_dp(H), cnt), "sr_calib_eval")
    return float(f.value), g, H, _counts(cnt)


class Calibrator:
    """Linear logistic regression calibration / fusion.  ``prior``: the training prior P in (0, 1); ``ridge`` >= 0 on the weights (set
    one for separable data: without it there is no finite optimum, and ``fit`` ends with whichever stop code it reaches and finite
    weights); ``tol``: the Newton decrement g^T H^-1 g at which ``fit`` stops; ``max_pass``: passes of one ``fit`` call (1 .. 1000).

    After ``fit``: ``weights`` [S], ``offset``, ``objective`` (f at the weights), ``passes``, ``accepted``, ``halvings``, ``decrement``,
    ``stop`` ("CONVERGED", "CAP", "SINGULAR" or "STALLED") and ``counts`` (targets, non-targets, skipped)."""

    def __init__(self, prior=0.5, ridge=0.0, tol=1e-16, max_pass=100):
        self.prior, self.ridge, self.tol, self.max_pass = float(prior), float(ridge), float(tol), int(max_pass)
        self.weights = self.offset = self.objective = self.stop = self.counts = None
        self.passes = self.accepted = self.halvings = 0
        self.decrement = None
        self._state = None
        self._stacked = None

    def fit(self, scores, labels, theta0=None, resume=False):
        """``scores``: a vector [n]; an array [S, n]; or a list of S score matrices [J, T] with ``labels`` [J, T], a key matrix of 1 /
        0 / negative.  A quality measure, such as a duration, is just another row of ``scores``.  ``theta0`` [S + 1]: the start (zeros).
        ``resume``: continue a fit that ended by "CAP" on the same data for ``max_pass`` more passes -- ``max_pass = a`` and then a
        resume with ``b`` equal one fit with ``a + b``, bit for bit."""
        from . import _lib
        lab = _labels(labels)
        X, _, stacked = _stack(scores, lab.shape)
        S, n = X.shape
        lab = np.ascontiguousarray(lab.reshape(-1))
        n_state = _HEAD + 4 * (S + 1) + (S + 1) * (S + 2) // 2
        if resume:
            if self._state is None or self._state.shape[0] != n_state:
                raise ValueError("resume needs an earlier fit of this calibrator on the same systems")
            state = self._state.copy()
        else:
            state = np.zeros(n_state)
        th0 = None
        if theta0 is not None:
            th0 = np.ascontiguousarray(theta0, dtype=np.float64).reshape(-1)
            if th0.shape[0] != S + 1:
                raise ValueError("expected theta0 as %d weights and the offset, got %d values" % (S, th0.shape[0]))
        cnt = (C.c_int64 * 3)()
        _lib.check(_lib.lib().sr_calib_train(S, n, _lib.as_dp(X), _lib.as_i8p(lab), self.prior, self.ridge, self.tol, self.max_pass,
                                             _lib.as_dp(th0) if th0 is not None else None, 1 if resume else 0, _lib.as_dp(state), cnt),
                   "sr_calib_train")
        self._state = state
        self._stacked = stacked
        self.stop = _lib.CALIB_STOPS[int(state[0])]
        self.passes, self.accepted, self.halvings = int(state[2]), int(state[3]), int(state[4])
        self.objective, self.decrement = float(state[5]), float(state[7])
        self.weights, self.offset = state[_HEAD:_HEAD + S].copy(), float(state[_HEAD + S])
        self.counts = _counts(cnt)
        return self

    @property
    def theta(self):
        return None if self.weights is None else np.r_[self.weights, self.offset]

    def transform(self, scores):
        """The calibrated log-likelihood ratios ``sum_s w_s scores[s] + b`` in the input's trial shape: [n] for a vector or [S, n],
        [J, T] for a list of S matrices.  Elementwise over everything given: the same trial gives the same bits alone and in a batch."""
        from . import _lib
        if self.weights is None:
            raise ValueError("transform needs a fitted calibrator")
        X, shape, _ = _stack(scores, stacked=self._stacked)
        S, n = X.shape
        if S != self.weights.shape[0]:
            raise ValueError("fitted on %d system(s), got scores of %d" % (self.weights.shape[0], S))
        out = np.zeros(n)
        th = np.ascontiguousarray(self.theta)
        _lib.check(_lib.lib().sr_calib_apply(S, n, _lib.as_dp(X), _lib.as_dp(th), _lib.as_dp(out)), "sr_calib_apply")
        return out.reshape(shape)


def cllr(llr, labels):
    """Cllr of log-likelihood ratios, on the device: (1 / (2 ln 2)) [mean_tar sp(-llr) + mean_non sp(llr)]."""
    lab = _labels(labels)
    a = np.asarray(llr, dtype=np.float64)
    if a.shape != lab.shape:
        raise ValueError("expected one label per llr, got shapes %r and %r" % (a.shape, lab.shape))
    return evaluate(a.reshape(-1), lab.reshape(-1), [1.0, 0.0])[0]


def error_counts(llr, labels, thresholds, return_counts=False):
    """(misses [m], false alarms [m]) int64 at each of the ``thresholds``, on the device, exact.  A trial is accepted iff its llr is >=
    the threshold; a miss is a target not accepted, a false alarm a non-target accepted.  -inf and +inf are thresholds.
    ``return_counts``: -> (misses, false_alarms, {"targets", "non_targets", "skipped"})."""
    from . import _lib
    lab = _labels(labels)
    a = np.ascontiguousarray(llr, dtype=np.float64)
    if a.shape != lab.shape:
        raise ValueError("expected one label per llr, got shapes %r and %r" % (a.shape, lab.shape))
    a, lab = a.reshape(-1), np.ascontiguousarray(lab.reshape(-1))
    thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
    if thr.shape[0] < 1:
        raise ValueError("expected at least one threshold")
    miss, fa = np.zeros(thr.shape[0], dtype=np.int64), np.zeros(thr.shape[0], dtype=np.int64)
    cnt = (C.c_int64 * 3)()
    for j0 in range(0, thr.shape[0], MAX_THRESHOLDS):
        t = np.ascontiguousarray(thr[j0:j0 + MAX_THRESHOLDS])
        m, f = np.zeros(t.shape[0], dtype=np.int64), np.zeros(t.shape[0], dtype=np.int64)
        _lib.check(_lib.lib().sr_calib_counts(a.shape[0], _lib.as_dp(a), _lib.as_i8p(lab), t.shape[0], _lib.as_dp(t), _lib.as_i64p(m),
                                              _lib.as_i64p(f), cnt), "sr_calib_counts")
        miss[j0:j0 + t.shape[0]], fa[j0:j0 + t.shape[0]] = m, f
    return (miss, fa, _counts(cnt)) if return_counts else (miss, fa)


def bayes_threshold(p_target=0.01, c_miss=1.0, c_fa=1.0):
    """The threshold on a log-likelihood ratio that minimises the expected cost: ln(c_fa (1 - p_target) / (c_miss p_target))."""
    if not (0.0 < p_target < 1.0) or not (c_miss > 0.0 and c_fa > 0.0):
        raise ValueError("need 0 < p_target < 1 and positive costs")
    return float(np.log(c_fa * (1.0 - p_target) / (c_miss * p_target)))


def act_dcf(llr, labels, p_target=0.01, c_miss=1.0, c_fa=1.0):
    """The normalised actual detection cost of deciding at the Bayes threshold (accept iff llr >= ``bayes_threshold``; counted on the
    device):  (c_miss p_target P_miss + c_fa (1 - p_target) P_fa) / min(c_miss p_target, c_fa (1 - p_target))."""
    thr = bayes_threshold(p_target, c_miss, c_fa)
    miss, fa, cnt = error_counts(llr, labels, [thr], return_counts=True)
    p_miss, p_fa = miss[0] / cnt["targets"], fa[0] / cnt["non_targets"]
    return float((c_miss * p_target * p_miss + c_fa * (1.0 - p_target) * p_fa) / min(c_miss * p_target, c_fa * (1.0 - p_target)))


def pav_blocks(scores, labels):
    """Pool-adjacent-violators on the target indicator along ascending score -> (targets, trials) of each block, ascending: the block
    target shares are non-decreasing.  Trials with equal scores enter as one group and move together.  Negative labels are skipped."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    lab = _labels(labels).reshape(-1)
    if s.shape != lab.shape:
        raise ValueError("expected one label per score, got %d scores and %d labels" % (s.size, lab.size))
    keep = lab >= 0
    s, tar = s[keep], lab[keep] > 0
    if not np.all(np.isfinite(s)):
        raise ValueError("scores hold a non-finite value at a trial")
    if tar.sum() == 0 or (~tar).sum() == 0:
        raise ValueError("need at least one target and one non-target trial (got %d and %d)" % (tar.sum(), (~tar).sum()))
    order = np.argsort(s, kind="stable")
    s, tar = s[order], tar[order]
    first = np.r_[True, s[1:] != s[:-1]]
    start = np.flatnonzero(first)
    n_tar = np.add.reduceat(tar.astype(np.int64), start)
    n_all = np.diff(np.r_[start, s.shape[0]])
    bt, ba = [], []
    for t, a in zip(n_tar.tolist(), n_all.tolist()):
        bt.append(t), ba.append(a)
        while len(bt) > 1 and bt[-2] * ba[-1] >= bt[-1] * ba[-2]:          # share[-2] >= share[-1], in integers: pool
            t2, a2 = bt.pop(), ba.pop()
            bt[-1] += t2
            ba[-1] += a2
    return np.array(bt, dtype=np.int64), np.array(ba, dtype=np.int64)


def min_cllr(llr, labels):
    """The Cllr left after the best monotone recalibration of the scores, on the host: sort, pool adjacent violators of the target
    indicator (equal scores move together), give each block the llr  logit(block target share) - logit(n_t / (n_t + n_n)), and take
    Cllr of those values.  End points by the BOSARIS convention (``opt_loglr`` with the "raw" option, as its ``min_cllr`` uses it): no
    dummy trials are added, so a block of non-targets only at the low end and a block of targets only at the high end get -inf and +inf
    and cost nothing -- perfectly separated scores give 0, scores in reversed order at equal counts give 1."""
    bt, ba = pav_blocks(llr, labels)
    bn = ba - bt
    n_t, n_n = int(bt.sum()), int(bn.sum())
    sp = lambda a: np.maximum(a, 0.0) + np.log1p(np.exp(-np.abs(a)))           # noqa: E731
    with np.errstate(divide="ignore", invalid="ignore"):
        l = (np.log(bt.astype(np.float64)) - np.log(bn.astype(np.float64))) - (np.log(float(n_t)) - np.log(float(n_n)))
        ct = np.where(bt > 0, bt * sp(-l), 0.0).sum() / n_t
        cn = np.where(bn > 0, bn * sp(l), 0.0).sum() / n_n
    return float(0.5 * (ct + cn) / np.log(2.0))
