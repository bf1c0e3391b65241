"""The i-vector back end on the device (csrc/plda.hip through ``sr_backend_fit`` / ``sr_backend_apply`` / ``sr_cosine_score`` /
``sr_plda_train`` / ``sr_plda_score``): what a ``[sessions, R]`` array of i-vectors (``ivector.extract``) goes through on its way to a
score matrix that ``scorenorm.normalise`` and ``scorenorm.eer`` / ``min_dcf`` take.

    ``fit_transform(X, ids=None, kind="whiten")``   -> ``(mu, A)``: the mean, and ``A = chol(Sigma)^-1`` of the total covariance
                                                    ("whiten") or of the within-class covariance about the class means ("wccn")
    ``transform(X, mu, A, length_norm=True)``        -> ``(X - mu) A^T``, each row scaled to unit 2-norm
    ``cosine_score(E, X)``                           -> ``<e_j, x_t> / (|e_j| |x_t|)`` [J, T]
    ``PLDA().fit(X, ids).score(enrol, enrol_ids, X)`` -> the log-likelihood ratios [J, T] of the two-covariance Gaussian PLDA
                                                    ``x_ij = mu + y_i + e_ij``, ``y ~ N(0, Sb)``, ``e ~ N(0, Sw)``

    ``sym_eig(A)`` / ``gen_eig(Sb, Sw)``             -> ``(w, V)``: the float64 symmetric eigen-solver on the device (csrc/eig.hip, block
                                                    Jacobi), and ``Sb v = psi Sw v`` with ``V^T Sw V = I``, ``V^T Sb V = diag(psi)``
    ``LDA().fit(X, ids, n_dims).transform(X)``       -> ``(X - mu) A^T`` [n, n_dims], ``A Sw A^T = I``: the first link of the usual chain
    ``PLDA.diagonalise()`` -> ``DiagPLDA(mu, V, psi)`` whose ``score`` gives ``PLDA.score``'s result without any factorisation

Whitening and WCCN take the Cholesky form (any whitening matrix gives the same norms and PLDA is invariant under the rotation that is
left); LDA and the diagonalised scorer need eigenvectors and get them from the device's own solver (csrc/eig.hip, csrc/backend_eig.hip
through ``sr_sym_eig`` / ``sr_gen_eig`` / ``sr_lda_fit`` / ``sr_backend_project`` / ``sr_plda_score_diag``).  Float64 throughout; there is
no CPU path."""
from __future__ import annotations

import ctypes as C

import numpy as np

KINDS = ("whiten", "wccn")
STOP_CODES = ("", "Sb did not factor", "Sw did not factor", "a Sb^-1 + c Sw^-1 did not factor", "a round produced a non-finite value")


def _rows(a, name, R=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or (R is not None and a.shape[1] != R):
        raise ValueError("expected %s as [rows, %s], got shape %r" % (name, "R" if R is None else R, a.shape))
    return a


def _labels(ids, n, name="ids"):
    """-> (0-based dense labels [n] int64, the distinct values given, ascending)."""
    ids = np.asarray(ids).reshape(-1)
    if ids.shape[0] != n:
        raise ValueError("expected one label per row as %s (%d), got %d" % (name, n, ids.shape[0]))
    present, dense = np.unique(ids, return_inverse=True)
    return np.ascontiguousarray(dense, dtype=np.int64), present


def fit_transform(X, ids=None, kind="whiten"):
    """``X`` [n, R] -> ``(mu [R], A [R, R])`` with ``A`` lower triangular: "whiten": ``A Sigma A^T = I`` for the total covariance
    (ddof = 0) of the rows; "wccn": ``A W A^T = I`` for the within-class covariance, the rows taken about the means of their classes
    ``ids`` [n] (any hashable labels).  A covariance that does not factor (dependent columns, too few rows) is refused."""
    from . import _lib
    if kind not in KINDS:
        raise ValueError("kind is one of %s, got %r" % (", ".join(repr(k) for k in KINDS), kind))
    X = _rows(X, "X")
    n, R = X.shape
    dense, n_labels = None, 0
    if kind == "wccn":
        if ids is None:
            raise ValueError("kind 'wccn' needs ids, one class label per row")
        dense, present = _labels(ids, n)
        n_labels = int(present.size)
    mu, A = np.zeros(R), np.zeros((R, R))
    _lib.check(_lib.lib().sr_backend_fit(KINDS.index(kind), n, R, _lib.as_dp(X), _lib.as_i64p(dense) if dense is not None else None, n_labels,
                                         _lib.as_dp(mu), _lib.as_dp(A)), "sr_backend_fit")
    return mu, A


def transform(X, mu, A, length_norm=True, return_counts=False):
    """``(X - mu) A^T`` [n, R]; with ``length_norm`` every row scaled to unit 2-norm, a row whose norm is 0 or not finite becoming exact
    zeros.  ``return_counts``: -> (Y, {"zero_rows": n})."""
    from . import _lib
    X = _rows(X, "X")
    n, R = X.shape
    mu = np.ascontiguousarray(np.reshape(mu, -1), dtype=np.float64)
    A = np.ascontiguousarray(A, dtype=np.float64)
    if mu.shape != (R,) or A.shape != (R, R):
        raise ValueError("expected mu [%d] and A [%d, %d], got %r and %r" % (R, R, R, mu.shape, A.shape))
    Y = np.zeros((n, R))
    zeros = C.c_int64(0)
    _lib.check(_lib.lib().sr_backend_apply(n, R, _lib.as_dp(X), _lib.as_dp(mu), _lib.as_dp(A), 1 if length_norm else 0, _lib.as_dp(Y),
                                           C.byref(zeros)), "sr_backend_apply")
    return (Y, {"zero_rows": int(zeros.value)}) if return_counts else Y


def cosine_score(E, X):
    """``E`` [J, R] against ``X`` [T, R] -> the cosines [J, T]: one product and the row norms.  A pair with a zero vector scores 0.0."""
    from . import _lib
    E = _rows(E, "E")
    X = _rows(X, "X", E.shape[1])
    out = np.zeros((E.shape[0], X.shape[0]))
    _lib.check(_lib.lib().sr_cosine_score(E.shape[0], X.shape[0], E.shape[1], _lib.as_dp(E), _lib.as_dp(X), _lib.as_dp(out)), "sr_cosine_score")
    return out


def _square(a, name, R=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != a.shape[1] or (R is not None and a.shape[0] != R):
        raise ValueError("expected %s as a square [%s, %s] matrix, got shape %r" % (name, "R" if R is None else R, "R" if R is None else R, a.shape))
    return a


def sym_eig(A, return_info=False):
    """``A`` [R, R] symmetric (the lower triangle is read; need not be definite) -> ``(w [R] descending, V [R, R])``, column k of ``V``
    the unit eigenvector of ``w[k]``, its component of largest magnitude positive (the lowest index winning a tie).  A call that
    reaches the solver's cap of 40 sweeps raises ``ArithmeticError``; ``return_info``: -> (w, V, {"sweeps": n, "converged": 0 | 1})
    and no raise."""
    from . import _lib
    A = _square(A, "A")
    R = A.shape[0]
    w, V = np.zeros(R), np.zeros((R, R))
    sweeps, conv = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().sr_sym_eig(R, _lib.as_dp(A), _lib.as_dp(w), _lib.as_dp(V), C.byref(sweeps), C.byref(conv)), "sr_sym_eig")
    if return_info:
        return w, V, {"sweeps": int(sweeps.value), "converged": int(conv.value)}
    if not conv.value:
        raise ArithmeticError("sym_eig did not converge in %d sweeps" % sweeps.value)
    return w, V


def gen_eig(Sb, Sw, return_info=False):
    """``Sb v = psi Sw v`` for symmetric ``Sb`` and positive definite ``Sw`` [R, R] -> ``(psi [R] descending, V [R, R])`` with
    ``V^T Sw V = I`` and ``V^T Sb V = diag(psi)``.  An ``Sw`` that does not factor, or the sweep cap, raises ``ArithmeticError``;
    ``return_info``: -> (psi, V, {"sweeps": n, "status": 0 ok | 1 Sw did not factor (exact zeros) | 2 the cap}) and no raise."""
    from . import _lib
    Sb = _square(Sb, "Sb")
    R = Sb.shape[0]
    Sw = _square(Sw, "Sw", R)
    psi, V = np.zeros(R), np.zeros((R, R))
    sweeps, status = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().sr_gen_eig(R, _lib.as_dp(Sb), _lib.as_dp(Sw), _lib.as_dp(psi), _lib.as_dp(V), C.byref(sweeps), C.byref(status)), "sr_gen_eig")
    if return_info:
        return psi, V, {"sweeps": int(sweeps.value), "status": int(status.value)}
    if status.value == 1:
        raise ArithmeticError("gen_eig: Sw did not factor (it is not positive definite)")
    if status.value == 2:
        raise ArithmeticError("gen_eig did not converge in %d sweeps" % sweeps.value)
    return psi, V


class LDA:
    """Linear discriminant analysis.  After ``fit``: ``mu`` [R], ``A`` [n_dims, R] with ``A Sw A^T = I`` for the within-class covariance
    (the projection arrives WCCN-normalised) and ``A Sb A^T = diag(psi)``, ``psi`` [n_dims] descending."""

    def __init__(self, mu=None, A=None, psi=None):
        self.mu = None if mu is None else np.ascontiguousarray(np.reshape(mu, -1), dtype=np.float64)
        self.A = None if A is None else np.ascontiguousarray(A, dtype=np.float64)
        self.psi = None if psi is None else np.ascontiguousarray(np.reshape(psi, -1), dtype=np.float64)

    def fit(self, X, ids, n_dims):
        """``X`` [n, R] with class labels ``ids`` [n] (any hashable labels) -> self, keeping 1 <= ``n_dims`` <= min(R, classes - 1)
        directions."""
        from . import _lib
        X = _rows(X, "X")
        n, R = X.shape
        dense, present = _labels(ids, n)
        P = int(n_dims)
        top = min(R, int(present.size) - 1)
        if P < 1 or P > top:
            raise ValueError("n_dims is %d; %d classes in %d dimensions leave 1 <= n_dims <= min(R, classes - 1) = %d" % (P, present.size, R, top))
        mu, A, psi = np.zeros(R), np.zeros((P, R)), np.zeros(P)
        _lib.check(_lib.lib().sr_lda_fit(n, R, _lib.as_dp(X), _lib.as_i64p(dense), int(present.size), P, _lib.as_dp(mu), _lib.as_dp(A),
                                         _lib.as_dp(psi)), "sr_lda_fit")
        self.mu, self.A, self.psi = mu, A, psi
        return self

    def transform(self, X, length_norm=True, return_counts=False):
        """``(X - mu) A^T`` [n, n_dims]; ``length_norm`` and ``return_counts`` as ``transform`` has them."""
        from . import _lib
        if self.mu is None or self.A is None:
            raise ValueError("the projection has no parameters yet: fit it, or give mu and A")
        R = self.mu.shape[0]
        X = _rows(X, "X", R)
        if self.A.ndim != 2 or self.A.shape[1] != R or not 1 <= self.A.shape[0] <= R:
            raise ValueError("expected A as [n_dims <= %d, %d], got %r" % (R, R, self.A.shape))
        n, P = X.shape[0], self.A.shape[0]
        Y = np.zeros((n, P))
        zeros = C.c_int64(0)
        _lib.check(_lib.lib().sr_backend_project(n, R, P, _lib.as_dp(X), _lib.as_dp(self.mu), _lib.as_dp(self.A), 1 if length_norm else 0,
                                                 _lib.as_dp(Y), C.byref(zeros)), "sr_backend_project")
        return (Y, {"zero_rows": int(zeros.value)}) if return_counts else Y


def _enrolment_sums(enrol, enrol_ids, R, enrol_mode):
    """-> (E [J, R] the models' sums, counts [J]) as ``PLDA.score`` forms them.  ``PLDA.score`` keeps its own copy of these lines (it
    is left as it was); the two scorers are compared on the same enrolment, so a change to the sums or to the modes goes into both."""
    if enrol_mode not in ("by_the_book", "average"):
        raise ValueError("enrol_mode is 'by_the_book' or 'average', got %r" % (enrol_mode,))
    enrol = _rows(enrol, "enrol", R)
    dense, present = _labels(enrol_ids, enrol.shape[0], "enrol_ids")
    J = int(present.size)
    E = np.zeros((J, R))
    np.add.at(E, dense, enrol)                 # (in row order: the same sums from run to run)
    counts = np.bincount(dense, minlength=J).astype(np.int64)
    if enrol_mode == "average":
        E /= counts[:, None]
        counts = np.ones(J, dtype=np.int64)
    return E, counts


class DiagPLDA:
    """A two-covariance PLDA model diagonalised once (``PLDA.diagonalise``): ``mu`` [R], ``V`` [R, R] with ``V^T Sw V = I`` and
    ``V^T Sb V = diag(psi)``, ``psi`` [R].  ``score`` gives ``PLDA.score``'s log-likelihood ratios with no factorisation: two products
    with ``V``, one cross product over all models, one narrow product for the quadratic forms."""

    def __init__(self, mu, V, psi):
        self.mu = np.ascontiguousarray(np.reshape(mu, -1), dtype=np.float64)
        R = self.mu.shape[0]
        self.V = _square(V, "V", R)
        self.psi = np.ascontiguousarray(np.reshape(psi, -1), dtype=np.float64)
        if self.psi.shape != (R,):
            raise ValueError("expected psi [%d], got %r" % (R, self.psi.shape))

    def score(self, enrol, enrol_ids, X, enrol_mode="by_the_book", return_counts=False):
        """As ``PLDA.score``.  A ``psi`` that is negative beyond rounding or not finite, or a class with a ``(c + 1) psi_d + 1 <= 0`` (which includes ``c psi_d + 1 <= 0``), gives
        exact zeros in the class's rows and is counted in "bad_classes"."""
        from . import _lib
        R = self.mu.shape[0]
        E, counts = _enrolment_sums(enrol, enrol_ids, R, enrol_mode)
        X = _rows(X, "X", R)
        J = E.shape[0]
        out = np.zeros((J, X.shape[0]))
        bad = C.c_int64(0)
        _lib.check(_lib.lib().sr_plda_score_diag(J, X.shape[0], R, _lib.as_dp(self.mu), _lib.as_dp(self.V), _lib.as_dp(self.psi), _lib.as_dp(E),
                                                 _lib.as_i64p(counts), _lib.as_dp(X), _lib.as_dp(out), C.byref(bad)), "sr_plda_score_diag")
        return (out, {"bad_classes": int(bad.value)}) if return_counts else out


class PLDA:
    """Two-covariance Gaussian PLDA.  ``mu`` [R], ``Sb`` and ``Sw`` [R, R] after ``fit`` (or given); ``iterations``, ``n_classes``
    (the distinct speaker counts) and ``stop`` (0: every round ran; 1 .. 4: ``STOP_CODES``, the pair kept is the last that factored)
    describe the last ``fit``."""

    def __init__(self, mu=None, Sb=None, Sw=None):
        self.mu = None if mu is None else np.ascontiguousarray(np.reshape(mu, -1), dtype=np.float64)
        self.Sb = None if Sb is None else np.ascontiguousarray(Sb, dtype=np.float64)
        self.Sw = None if Sw is None else np.ascontiguousarray(Sw, dtype=np.float64)
        self.iterations = self.n_classes = self.stop = 0

    def fit(self, X, ids, n_iter=10, Sb0=None, Sw0=None):
        """``n_iter`` EM rounds on ``X`` [n, R] with speaker labels ``ids`` [n] in one device call, from ``Sb0`` / ``Sw0`` (default:
        both half the total covariance of the rows, formed on the device; give both or neither).  ``mu`` is the mean of the rows and
        is not re-estimated.  The pair the last round returns is checked for finite values, not factored: ``stop`` 0 does not promise
        that ``score`` or a further ``fit`` can factor it -- they report that themselves.  -> self."""
        from . import _lib
        X = _rows(X, "X")
        n, R = X.shape
        dense, present = _labels(ids, n)
        if (Sb0 is None) != (Sw0 is None):
            raise ValueError("give Sb0 and Sw0 together, or neither (both then start from half the total covariance, formed on the device)")
        default = Sb0 is None
        Sb = np.zeros((R, R)) if default else np.array(Sb0, dtype=np.float64, order="C")
        Sw = np.zeros((R, R)) if default else np.array(Sw0, dtype=np.float64, order="C")
        if Sb.shape != (R, R) or Sw.shape != (R, R):
            raise ValueError("expected Sb0 and Sw0 as [%d, %d], got %r and %r" % (R, R, Sb.shape, Sw.shape))
        mu = np.zeros(R)
        it, nc, stop = C.c_int(0), C.c_int(0), C.c_int(0)
        _lib.check(_lib.lib().sr_plda_train(n, R, _lib.as_dp(X), _lib.as_i64p(dense), int(present.size), int(n_iter), 1 if default else 0,
                                            _lib.as_dp(mu), _lib.as_dp(Sb), _lib.as_dp(Sw), C.byref(it), C.byref(nc), C.byref(stop)), "sr_plda_train")
        self.mu, self.Sb, self.Sw = mu, Sb, Sw
        self.iterations, self.n_classes, self.stop = int(it.value), int(nc.value), int(stop.value)
        return self

    def score(self, enrol, enrol_ids, X, enrol_mode="by_the_book", return_counts=False):
        """The log-likelihood ratios [J, T] of the J models enrolled from ``enrol`` [m, R] (``enrol_ids`` [m]: the model of each
        vector; the models are the distinct labels, ascending) against the test vectors ``X`` [T, R].  ``enrol_mode``
        "by_the_book": a model's vectors are its n_j observations; "average": a model is ONE observation, the mean of its vectors.
        A count class whose blocks do not factor gets exact zeros.  ``return_counts``: -> (out, {"bad_classes": n})."""
        from . import _lib
        if enrol_mode not in ("by_the_book", "average"):
            raise ValueError("enrol_mode is 'by_the_book' or 'average', got %r" % (enrol_mode,))
        if self.mu is None or self.Sb is None or self.Sw is None:
            raise ValueError("the model has no parameters yet: fit it, or give mu, Sb and Sw")
        R = self.mu.shape[0]
        enrol = _rows(enrol, "enrol", R)
        X = _rows(X, "X", R)
        dense, present = _labels(enrol_ids, enrol.shape[0], "enrol_ids")
        J = int(present.size)
        E = np.zeros((J, R))
        np.add.at(E, dense, enrol)             # (in row order: the same sums from run to run)
        counts = np.bincount(dense, minlength=J).astype(np.int64)
        if enrol_mode == "average":
            E /= counts[:, None]
            counts = np.ones(J, dtype=np.int64)
        out = np.zeros((J, X.shape[0]))
        bad = C.c_int64(0)
        _lib.check(_lib.lib().sr_plda_score(J, X.shape[0], R, _lib.as_dp(self.mu), _lib.as_dp(self.Sb), _lib.as_dp(self.Sw), _lib.as_dp(E),
                                            _lib.as_i64p(counts), _lib.as_dp(X), _lib.as_dp(out), C.byref(bad)), "sr_plda_score")
        return (out, {"bad_classes": int(bad.value)}) if return_counts else out

    def diagonalise(self, return_info=False):
        """-> ``DiagPLDA(mu, V, psi)`` with ``(psi, V) = gen_eig(Sb, Sw)``: paid once per model, not once per call and count class.
        Raises ``ArithmeticError`` as ``gen_eig`` does; ``return_info``: -> (DiagPLDA, gen_eig's info) and no raise."""
        if self.mu is None or self.Sb is None or self.Sw is None:
            raise ValueError("the model has no parameters yet: fit it, or give mu, Sb and Sw")
        if return_info:
            psi, V, info = gen_eig(self.Sb, self.Sw, return_info=True)
            return DiagPLDA(self.mu, V, psi), info
        psi, V = gen_eig(self.Sb, self.Sw)
        return DiagPLDA(self.mu, V, psi)
