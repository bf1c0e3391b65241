"""What the tests of the symmetric eigen-solver (csrc/eig.hip), of the generalised problem, LDA and the diagonalised PLDA scorer
(csrc/backend_eig.hip, plda.py) share: the generators, a numpy model of the block sweep, the numpy restatements, the named mutants
and the gates.

GATES.  eps = 2^-52 and u(k) = plda_cases.unit(R, k) = 8 (R + R) eps k with k = the sweeps taken + 1: each of the R - 1 rounds of a
sweep recombines every entry of A and of V once, by an orthogonal transformation whose rounding error is a few eps of the entries'
magnitude, |A|_2 at most; the errors of the sweeps add.
    eigenvalues     |w - eigvalsh(A)|_max <= u(k) |A|_2
    residual        |A V - V diag(w)|_max <= u(k) |A|_2
    orthogonality   |V^T V - I|_max <= u(k)
    eigenvectors    compared directly only where the gaps are prescribed (``gapped``): a vector turns by the perturbation over its gap
                    (Davis-Kahan), so the gate is u(k) over the smallest relative gap.
    generalised     V^T Sw V - I, V^T Sb V - diag(psi) (relative to |diag(psi)|), psi against eigvalsh of the restated M: the Cholesky
                    factor's inverse amplifies by kappa(Sw):  kappa(Sw) u(k).
    diagonal score  against plda_cases.score:  gate_score(R, f) + amp_s kappa(Sw) u(k)  (the model's own conditioning, and the
                    diagonalisation's error on every term of the score).
None of the constants is fitted to what the device returns."""
import numpy as np

import plda_cases as pc

EPS = pc.EPS
MAX_SWEEPS = 40
SEPARATED_SWEEPS = 20           # the well-separated spectra must converge within these
KINDS = ("spd10", "spd1e6", "indefinite", "rank_one", "identity", "sorted_diag", "multiple")
GEN_R = (1, 2, 17, 65, 113)


# The smallest sizes at which the kernels can still go wrong, as (multiplier of the plan's block width b, offset), b read from
# sr_eig_plan when a test runs: the smallest; b and b + 1; 2b - 1 and 2b, the largest single-launch size; 2b + 1, three blocks and
# the phantom; 3b; 3b + 1, four blocks; 112 and 113, the factorisation's LDS / global path boundary in gen_eig; 4b + 1, five blocks
# and the phantom; 200.
SHAPES = ((0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (2, -1), (2, 0), (2, 1), (3, 0), (3, 1), (0, 112), (0, 113), (4, 1), (0, 200))
SHAPE_IDS = ["%s%s" % ("%db" % m if m else "", ("%+d" % o if m else "%d" % o) if o or not m else "") for m, o in SHAPES]
# LDA: (R, the classes' counts).  Fewer classes than R + 1, so that the between-class covariance is rank-deficient and the limit
# min(R, classes - 1) binds on the classes (n - classes > R: Sw factors); and more classes than R, where it binds on R.
LDA_CASES = ((17, (5,) * 10), (65, (6,) * 20), (17, tuple(3 + i % 4 for i in range(25))), (65, tuple(3 + i % 4 for i in range(73))))


def shape(size, b):
    return size[0] * b + size[1]


def shapes(b):
    return sorted({shape(e, b) for e in SHAPES})


def lda_dims(R, counts):
    """P = 1, a value between, and the largest allowed: classes - 1, or R."""
    top = min(R, len(counts) - 1)
    return (1, (top + 1) // 2, top)


def _rotation(R, rng):
    Q, _ = np.linalg.qr(rng.standard_normal((R, R)))
    return Q


def _from_spectrum(ev, rng):
    Q = _rotation(ev.size, rng)
    M = (Q * ev) @ Q.T
    return 0.5 * (M + M.T)


_CACHE = {}


def matrix(kind, R):
    """The input of one case (read-only, cached)."""
    key = (kind, R)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * R + KINDS.index(kind) if kind in KINDS else 77 * R)
        if kind == "spd10":
            A = pc.spd(R, 10.0, rng)
        elif kind == "spd1e6":
            A = pc.spd(R, 1e6, rng)
        elif kind == "indefinite":
            A = _from_spectrum(np.linspace(-1.0, 1.5, R) if R > 1 else np.array([-0.5]), rng)
        elif kind == "rank_one":
            v = rng.standard_normal(R)
            A = np.outer(v, v)
        elif kind == "identity":
            A = np.eye(R)
        elif kind == "sorted_diag":
            A = np.diag(np.arange(1.0, R + 1.0))
        elif kind == "multiple":               # one eigenvalue of multiplicity R // 2, the rest distinct below it
            ev = np.concatenate([np.full(R // 2, 2.0), np.linspace(0.1, 1.0, R - R // 2)])
            A = _from_spectrum(ev, rng)
        elif kind == "gapped":                 # eigenvalues R, R - 1, .. 1: every gap 1, the smallest relative gap 1 / R
            A = _from_spectrum(np.arange(R, 0, -1.0), rng)
        else:
            raise ValueError(kind)
        A.setflags(write=False)
        _CACHE[key] = A
    return _CACHE[key]


def fix_signs(V):
    """Every column's component of largest magnitude positive, the lowest index winning a tie."""
    V = np.array(V)
    at = np.argmax(np.abs(V), axis=0)          # (argmax returns the first of equal values)
    V *= np.where(V[at, np.arange(V.shape[1])] < 0, -1.0, 1.0)
    return V


def reference(A):
    """-> (w descending, V signed) by LAPACK."""
    w, V = np.linalg.eigh(A)
    return w[::-1].copy(), fix_signs(V[:, ::-1])


def gate(R, sweeps):
    return pc.unit(R, sweeps + 1.0)


def figures(A, w, V):
    """-> (eigenvalue error, residual, orthogonality), the first two relative to |A|_2."""
    norm = float(np.linalg.norm(A, 2))
    scale = norm if norm > 0 else 1.0
    ev = float(np.max(np.abs(w - np.linalg.eigvalsh(A)[::-1]))) / scale
    res = float(np.max(np.abs(A @ V - V * w))) / scale
    orth = float(np.max(np.abs(V.T @ V - np.eye(A.shape[0]))))
    return ev, res, orth


# ---- a numpy model of the block sweep (csrc/eig.hip), rotation for rotation ----

def _round_robin(n, r, k):
    m = n - 1
    a, b = (r, m) if k == 0 else ((r + k) % m, (r + m - k) % m)
    return (a, b) if a < b else (b, a)


def jacobi(S, skip, stop, cap):
    """Cyclic Jacobi in the parallel ordering on S (a copy), |theta| <= pi / 4, a rotation with |a_pq| <= skip left out.
    -> (S, Q, sweeps)."""
    S = np.array(S)
    n = S.shape[0]
    Q = np.eye(n)
    ne = n + (n & 1)
    sweeps = 0

    def off():
        return float(np.max(np.abs(S - np.diag(np.diag(S))))) if n > 1 else 0.0

    while off() > stop and sweeps < cap:
        for r in range(ne - 1):
            pairs = [_round_robin(ne, r, k) for k in range(ne // 2)]
            pairs = [(p, q) for p, q in pairs if q < n and abs(S[p, q]) > skip]
            if not pairs:
                continue
            p, q = np.array(pairs).T
            apq, app, aqq = S[p, q], S[p, p], S[q, q]
            theta = (aqq - app) / (2.0 * apq)
            t = np.copysign(1.0, theta) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            Sp, Sq = S[:, p].copy(), S[:, q].copy()
            S[:, p], S[:, q] = c * Sp - s * Sq, s * Sp + c * Sq
            Sp, Sq = S[p, :].copy(), S[q, :].copy()
            S[p, :], S[q, :] = c[:, None] * Sp - s[:, None] * Sq, s[:, None] * Sp + c[:, None] * Sq
            S[p, p], S[q, q] = app - t * apq, aqq + t * apq
            S[p, q] = S[q, p] = 0.0
            Qp, Qq = Q[:, p].copy(), Q[:, q].copy()
            Q[:, p], Q[:, q] = c * Qp - s * Qq, s * Qp + c * Qq
        sweeps += 1
    return S, Q, sweeps


def block_jacobi(A, b, schedule=None, mutant=None, cap=MAX_SWEEPS, inner_cap=3):
    """The device's solver restated: blocks of b columns, the rounds of ``schedule`` (the plan's: [rounds][pairs] of (p, q), q == blocks the
    phantom; default the same round robin), the three stages of a round.  ``mutant`` "row_q": Q for Q^T in the row stage.
    -> (w descending, V signed, sweeps, converged)."""
    A = np.array(A, dtype=np.float64)
    R = A.shape[0]
    top = float(np.max(np.abs(A)))
    skip, stop = EPS * top, R * EPS * top
    if R <= 2 * b:
        S, Q, sweeps = jacobi(A, skip, stop, cap)
        order = np.argsort(-np.diag(S), kind="stable")
        return np.diag(S)[order], fix_signs(Q[:, order]), sweeps, int(np.max(np.abs(S - np.diag(np.diag(S))), initial=0.0) <= stop)
    blocks = -(-R // b)
    players = blocks + blocks % 2
    if schedule is None:
        schedule = [[_round_robin(players, r, k) for k in range(players // 2)] for r in range(players - 1)]
    V = np.eye(R)
    off = lambda: float(np.max(np.abs(A - np.diag(np.diag(A)))))                     # noqa: E731
    sweeps = 0
    while off() > stop and sweeps < cap:
        for rnd in schedule:
            work = [(p, q) for p, q in rnd if q < blocks]
            idx = [np.concatenate([np.arange(p * b, min(R, p * b + b)), np.arange(q * b, min(R, q * b + b))]) for p, q in work]
            solved = [jacobi(np.tril(A[np.ix_(i, i)]) + np.tril(A[np.ix_(i, i)], -1).T, skip, skip, inner_cap) for i in idx]
            for i, (S, Q, _) in zip(idx, solved):                                    # the columns
                A[:, i] = A[:, i] @ Q
                V[:, i] = V[:, i] @ Q
            for i, (S, Q, _) in zip(idx, solved):                                    # the rows
                A[i, :] = (Q if mutant == "row_q" else Q.T) @ A[i, :]
            for i, (S, Q, _) in zip(idx, solved):                                    # the solved block is the solver's
                A[np.ix_(i, i)] = np.tril(S) + np.tril(S, -1).T
        sweeps += 1
    order = np.argsort(-np.diag(A), kind="stable")
    return np.diag(A)[order], fix_signs(V[:, order]), sweeps, int(off() <= stop)


# ---- the generalised problem, LDA ----

def restated_M(Sb, Sw):
    Li = np.linalg.inv(np.linalg.cholesky(Sw))
    M = Li @ Sb @ Li.T
    return 0.5 * (M + M.T)


def gen_eig(Sb, Sw):
    """-> (psi descending, V) with V^T Sw V = I, V^T Sb V = diag(psi)."""
    Li = np.linalg.inv(np.linalg.cholesky(Sw))
    psi, Q = reference(restated_M(Sb, Sw))
    return psi, Li.T @ Q


def between_cov(X, ids):
    mu = X.mean(axis=0)
    Sb = np.zeros((X.shape[1],) * 2)
    for s in np.unique(ids):
        d = X[ids == s].mean(axis=0) - mu
        Sb += np.count_nonzero(ids == s) * np.outer(d, d)
    return Sb / X.shape[0]


def lda(X, ids, P):
    """-> (mu, A [P, R], psi [P], Sw, Sb)."""
    Sw, Sb = pc.within_cov(X, ids), between_cov(X, ids)
    psi, V = gen_eig(Sb, Sw)
    return X.mean(axis=0), V[:, :P].T.copy(), psi[:P], Sw, Sb


def project(X, mu, A, length_norm=True, mutant=None):
    return pc.transform(X, mu, A.T if mutant == "transposed" and A.shape[0] == A.shape[1] else A, length_norm)


# ---- the diagonalised score ----

DIAG_MUTANTS = {
    "v_not_transposed": "u = V (x - mu) for V^T (x - mu): shows at R > 1",
    "no_c": "c left out of g_cd: shows where a count is above 1",
    "no_logdet": "sum_d ln s_cd dropped",
    "psi_ascending": "psi read ascending where it is descending: shows at R > 1",
}


def diag_score(mu, V, psi, E, counts, X, mutant=None):
    """The score of the model diagonalised (the formulas of include/pygmm_hip.h, sr_plda_score_diag)."""
    if mutant == "psi_ascending":
        psi = psi[::-1]
    W = V.T if mutant == "v_not_transposed" else V
    U = (X - mu) @ W
    out = np.zeros((E.shape[0], X.shape[0]))
    s0 = 1.0 + psi
    a0 = (U * U / s0).sum(axis=1)
    for j, c in enumerate(counts):
        c = float(c)
        ebar = (E[j] / c - mu) @ W
        g = (1.0 if mutant == "no_c" else c) * psi / (c * psi + 1.0)
        s = 1.0 + psi / (c * psi + 1.0)
        m = g * ebar
        quad = (U * U / s).sum(axis=1) - 2.0 * U @ (m / s) + float((m * m / s).sum())
        ld = 0.0 if mutant == "no_logdet" else float(np.log(s).sum())
        out[j] = -0.5 * ld - 0.5 * quad + 0.5 * float(np.log(s0).sum()) + 0.5 * a0
    return out


def diag_mutant_shows(name, R, counts):
    if name in ("v_not_transposed", "psi_ascending"):
        return R > 1
    if name == "no_c":
        return max(counts) > 1
    return True


def gate_diag_score(R, f, kappa_w, sweeps):
    return pc.gate_score(R, f) + f["amp_s"] * kappa_w * gate(R, sweeps)
