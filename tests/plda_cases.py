"""The float64 numpy restatement of the i-vector back end (csrc/plda.hip, plda.py), its direct joint-Gaussian form, the generator, the
named mutants and the gates its tests share.

The model is the two-covariance PLDA  x_ij = mu + y_i + e_ij,  y ~ N(0, Sb),  e ~ N(0, Sw).  The restatement is written from the
formulas with ``np.linalg.inv`` and ``slogdet``; with n_i the vectors of speaker i, f_i = sum_j (x_ij - mu), T2 the scatter about mu:
    Phi_c = (Sb^-1 + c Sw^-1)^-1              yhat_i = Phi_{n_i} Sw^-1 f_i             Sb <- (sum_i Phi_{n_i} + Yhat^T Yhat) / S
    Sw <- (T2 - F^T Yhat - Yhat^T F + Yhat^T diag(n_i) Yhat + sum_i n_i Phi_{n_i}) / n
    score[j, t] = -1/2 ln det(Phi_c + Sw) - 1/2 (x - yhat_j)^T P_c (x - yhat_j) + 1/2 ln det(Sb + Sw) + 1/2 x^T P_0 x
The joint form knows none of this: the c vectors of one speaker stacked are Gaussian with covariance  I (x) Sw + 1 1^T (x) Sb,  the
score is  ln p(enrolment, x) - ln p(enrolment) - ln p(x),  the marginal likelihood the sum over the speakers.

GATES.  eps = 2^-52; a difference is taken relative to the restated array's largest magnitude (``rel``).  The unit is the forward
error of a backward-stable solve or inverse of an R x R system whose sums run over R terms,  u(k) = 8 (R + R) eps k  (the constant
and the form are DESIGN 3.5.2's); every condition number and every amplification factor is taken from the restatement's own
matrices, none from what the device returns:
    Phi_c     its argument Sb^-1 + c Sw^-1 carries u(kb) + u(kw), amplified by kP = cond of that argument, plus its own inverse:
              g_phi = kP (u(kb) + u(kw)) + u(kP)
    Yhat      = F Sw^-1 Phi: the two factors' errors and two R-term products, amplified by amp_y = max(|F| |Sw^-1| |Phi|) / max |Yhat|
              (the matrices of absolute values multiplied: the componentwise bound):  g_y = amp_y (u(kw) + g_phi + u(1))
    Sb'       a sum of positive semi-definite terms, no cancellation:  g_phi + 2 g_y + 8 (R + S) eps
    Sw'       T2 - F^T Yhat - Yhat^T F + Yhat^T N Yhat cancels down to the residual scatter: rho = (the terms' magnitudes) /
              (n |Sw'|):  rho (g_phi + 2 g_y + 8 (R + n) eps)
    n rounds  n times the one-round gate, the factors the largest over the rounds.
    score     P_c = (Phi_c + Sw)^-1: g_pc = kPc (g_phi + u(1)) + u(kPc); every term of the score (the log-determinants, a, the cross
              term, q, a_0) carries g_pc + 2 g_y + u(kP0) + u(1) of its own magnitude; amp_s = (the terms' magnitudes) / |score|.
    whiten    |cov((X - mu) A^T) - I| <= 8 (R + n) eps cond(Sigma);  a unit norm to 8 R eps.
    wccn      A = chol(W)^-1 against the restatement: 8 (R + n) eps cond(W).
    cosine    the product's error is 8 R eps |e| |x|: relative to the largest cosine, 8 R eps / max |cos|."""
import numpy as np

EPS = 2.0 ** -52
KAPPA_MAX = 1e6
KAPPA_TRUE = 10.0               # the condition number of the generator's Sb and of its Sw

# (R, the speakers' counts): every R of the training tests; one class, all ones, all distinct, and S at the reduction tile's edges
TRAIN_CASES = (
    (1, (3, 5)),                                        # S = 2
    (2, (4,) * 15),                                     # S = 15, one class
    (2, (2,) * 16),                                     # S = 16, one class
    (16, (1,) * 40),                                    # every count 1
    (17, tuple(range(1, 18))),                          # S = 17, every speaker a distinct count
    (16, tuple(1 + i % 5 for i in range(65))),          # S = 65
    (65, tuple(1 + i % 4 for i in range(65))),          # S = 65, n = 160
    (113, tuple(2 + i % 3 for i in range(80))),         # n = 239
)
# (R, J, T): the models' counts cycle 1 .. 7
SCORE_CASES = ((5, 7, 9), (1, 1, 1), (2, 63, 64), (17, 64, 65), (16, 65, 63), (65, 64, 1), (113, 1, 65))
# (R, n) of the transforms
TRANSFORM_R = (1, 2, 15, 16, 17, 63, 64, 65, 113)
TRANSFORM_N = (63, 64, 65, 200)                         # and R + 1
COSINE_SIZES = (1, 63, 64, 65)


# ---- the generator ----

def spd(R, kappa, rng):
    """A symmetric positive definite matrix with eigenvalues log-spaced over 1 / sqrt(kappa) .. sqrt(kappa): cond = kappa."""
    Q, _ = np.linalg.qr(rng.standard_normal((R, R)))
    ev = np.logspace(-0.5, 0.5, R) ** np.log10(kappa) if R > 1 else np.ones(1)
    M = (Q * ev) @ Q.T
    return 0.5 * (M + M.T)


def corpus(R, counts, seed):
    """Vectors of len(counts) speakers drawn from the model with known Sb (x 2) and Sw, both of condition KAPPA_TRUE, rows shuffled.
    -> dict(X [n, R], ids [n], mu_true, Sb_true, Sw_true)."""
    rng = np.random.default_rng(seed)
    Sb, Sw = 2.0 * spd(R, KAPPA_TRUE, rng), spd(R, KAPPA_TRUE, rng)
    mu = rng.standard_normal(R)
    ids = np.repeat(np.arange(len(counts)), counts)
    y = rng.multivariate_normal(np.zeros(R), Sb, len(counts), method="cholesky")
    X = mu + y[ids] + rng.multivariate_normal(np.zeros(R), Sw, ids.size, method="cholesky")
    order = rng.permutation(ids.size)
    return dict(X=np.ascontiguousarray(X[order]), ids=np.ascontiguousarray(ids[order]), mu_true=mu, Sb_true=Sb, Sw_true=Sw)


def total_cov(X):
    Xc = X - X.mean(axis=0)
    S = Xc.T @ Xc / X.shape[0]
    return 0.5 * (S + S.T)


def within_cov(X, ids):
    Xw = np.array(X, dtype=np.float64)
    for s in np.unique(ids):
        Xw[ids == s] -= X[ids == s].mean(axis=0)
    W = Xw.T @ Xw / X.shape[0]
    return 0.5 * (W + W.T)


# ---- the restatement ----

def _edge(A, mutant):
    """The "ragged GEMM edge zeroed" mutant: the columns past the last whole tile of 16 are lost."""
    if mutant == "edge" and A.shape[1] % 16:
        A = np.array(A)
        A[:, A.shape[1] // 16 * 16:] = 0.0
    return A


def phi(iSb, iSw, c, mutant=None):
    return np.linalg.inv(iSb + (c + 1 if mutant == "count" else c) * iSw)


def posterior_means(F, counts, iSb, iSw, mutant=None):
    """-> (Yhat [S, R], {c: Phi_c})."""
    Phi = {int(c): phi(iSb, iSw, int(c), mutant) for c in np.unique(counts)}
    Y = np.zeros_like(F)
    for i, c in enumerate(counts):
        Y[i] = F[i] @ Phi[int(c)] @ iSw if mutant == "transposed" else F[i] @ iSw @ Phi[int(c)]
    return _edge(Y, mutant), Phi


def _amp_yhat(F, counts, iSw, Phi, Y):
    """The componentwise bound of a product's rounding error, |F| |Sw^-1| |Phi_c| (Higham, Accuracy and Stability, 3.5), over |Yhat|."""
    A = np.abs(F) @ np.abs(iSw)
    top = max(float(np.max(A[counts == c] @ np.abs(Phi[int(c)]))) for c in np.unique(counts))
    return top / float(np.max(np.abs(Y)))


def em_step(X, ids, mu, Sb, Sw, mutant=None, want_factors=False):
    """One EM round -> (Sb', Sw') [, the gate's factors]."""
    n, R = X.shape
    S = int(ids.max()) + 1
    counts = np.bincount(ids, minlength=S)
    Xc = X - mu
    F = np.zeros((S, R))
    np.add.at(F, ids, Xc)
    T2 = Xc.T @ Xc
    iSb, iSw = np.linalg.inv(Sb), np.linalg.inv(Sw)
    Y, Phi = posterior_means(F, counts, iSb, iSw, mutant)
    sp = sum(Phi[int(c)] for c in counts)
    snp = sum((1 if mutant == "weight" else int(c)) * Phi[int(c)] for c in counts)
    FY, YnY = F.T @ Y, Y.T @ (counts[:, None] * Y)
    Sb1 = (sp + Y.T @ Y) / S
    Sw1 = (T2 - FY - FY.T + YnY + snp) / n
    Sb1, Sw1 = 0.5 * (Sb1 + Sb1.T), 0.5 * (Sw1 + Sw1.T)
    if not want_factors:
        return Sb1, Sw1
    big = lambda a: float(np.max(np.abs(a)))                                         # noqa: E731
    kP = max(float(np.linalg.cond(iSb + int(c) * iSw)) for c in np.unique(counts))
    amp_y = _amp_yhat(F, counts, iSw, Phi, Y)
    rho = (big(T2) + 2 * big(FY) + big(YnY) + big(snp)) / (n * big(Sw1))
    return Sb1, Sw1, dict(kb=float(np.linalg.cond(Sb)), kw=float(np.linalg.cond(Sw)), kP=kP, amp_y=amp_y, rho=rho)


def train(X, ids, Sb, Sw, n_iter, mutant=None):
    """-> (mu, [(Sb, Sw) after every round], the gate's factors, the largest of each over the rounds)."""
    mu = X.mean(axis=0)
    trace, worst = [], {}
    for _ in range(n_iter):
        Sb, Sw, f = em_step(X, ids, mu, Sb, Sw, mutant, want_factors=True)
        trace.append((Sb, Sw))
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in f.items()}
    return mu, trace, worst


def score(mu, Sb, Sw, E, counts, X, mutant=None, want_factors=False):
    """E [J, R] the models' raw enrolment sums, counts [J] -> the log-likelihood ratios [J, T] [, the gate's factors]."""
    R = mu.shape[0]
    iSb, iSw = np.linalg.inv(Sb), np.linalg.inv(Sw)
    F = E - counts[:, None] * mu
    Y, Phi = posterior_means(F, counts, iSb, iSw, mutant)
    Xc = X - mu
    P0 = np.linalg.inv(Sb + Sw)
    ld0 = np.linalg.slogdet(Sb + Sw)[1]
    a0 = np.einsum("tr,rs,ts->t", Xc, P0, Xc)
    out = np.zeros((E.shape[0], X.shape[0]))
    mags, kPc = 0.0, 0.0
    for j, c in enumerate(counts):
        C = Phi[int(c)] + Sw
        Pc = np.linalg.inv(C)
        ldc = 0.0 if mutant == "logdet" else np.linalg.slogdet(C)[1]
        d = Xc - Y[j]
        cross = Y[j] @ Pc @ Xc.T
        quad = np.einsum("tr,rs,ts->t", d, Pc, d)
        if mutant == "edge":                   # the cross term's columns past the last whole tile of 64 segments are lost
            lost = slice(X.shape[0] // 64 * 64, None)
            quad[lost] += 2.0 * cross[lost]
        out[j] = -0.5 * ldc - 0.5 * quad + 0.5 * ld0 + 0.5 * a0
        if want_factors:
            a, q = np.einsum("tr,rs,ts->t", Xc, Pc, Xc), float(Y[j] @ Pc @ Y[j])
            mags = max(mags, 0.5 * (abs(ldc) + abs(ld0) + float(np.max(a + 2 * np.abs(cross) + a0)) + q))
            kPc = max(kPc, float(np.linalg.cond(C)))
    if not want_factors:
        return out
    big = lambda a: float(np.max(np.abs(a)))                                         # noqa: E731
    kP = max(float(np.linalg.cond(iSb + int(c) * iSw)) for c in np.unique(counts))
    amp_y = _amp_yhat(F, counts, iSw, Phi, Y)
    return out, dict(kb=float(np.linalg.cond(Sb)), kw=float(np.linalg.cond(Sw)), kP=kP, kPc=kPc, kP0=float(np.linalg.cond(Sb + Sw)), amp_y=amp_y,
                     amp_s=mags / big(out))


def whiten(X, ids=None, kind="whiten"):
    """-> (mu, A = chol(covariance)^-1)."""
    C = total_cov(X) if kind == "whiten" else within_cov(X, ids)
    return X.mean(axis=0), np.linalg.inv(np.linalg.cholesky(C))


def transform(X, mu, A, length_norm=True, mutant=None):
    Y = (X - mu) @ (A if mutant == "transposed" else A.T)
    if length_norm:
        nrm = np.sqrt((Y * Y).sum(axis=1, keepdims=True))
        Y = np.where((nrm > 0) & np.isfinite(nrm), Y / np.where(nrm > 0, nrm, 1.0), 0.0)
    return Y


def cosine(E, X):
    return (E @ X.T) / (np.sqrt((E * E).sum(axis=1))[:, None] * np.sqrt((X * X).sum(axis=1))[None, :])


# ---- the joint form ----

def joint_cov(c, Sb, Sw):
    return np.kron(np.eye(c), Sw) + np.kron(np.ones((c, c)), Sb)


def joint_logpdf(rows, mu, Sb, Sw):
    """ln p of the rows [c, R] of ONE speaker: a Gaussian in c R dimensions."""
    c, R = rows.shape
    d = (rows - mu).reshape(-1)
    C = joint_cov(c, Sb, Sw)
    return -0.5 * (c * R * np.log(2 * np.pi) + np.linalg.slogdet(C)[1] + d @ np.linalg.solve(C, d))


def joint_score(mu, Sb, Sw, enrol_rows, x):
    """ln p(enrolment, x | one speaker) - ln p(enrolment) - ln p(x)."""
    return (joint_logpdf(np.vstack([enrol_rows, x[None]]), mu, Sb, Sw) - joint_logpdf(enrol_rows, mu, Sb, Sw) - joint_logpdf(x[None], mu, Sb, Sw))


def marginal_loglik(X, ids, mu, Sb, Sw):
    return float(sum(joint_logpdf(X[ids == s], mu, Sb, Sw) for s in np.unique(ids)))


# ---- the gates ----

def rel(got, want):
    """The largest difference relative to the largest magnitude of the restated array."""
    scale = float(np.max(np.abs(want))) if np.size(want) else 0.0
    return float(np.max(np.abs(np.asarray(got) - want))) / scale if scale > 0 else float(np.max(np.abs(got), initial=0.0))


def unit(R, k=1.0):
    return 8.0 * (R + R) * EPS * k


def gate_phi(R, f):
    return f["kP"] * (unit(R, f["kb"]) + unit(R, f["kw"])) + unit(R, f["kP"])


def gate_yhat(R, f):
    return f["amp_y"] * (unit(R, f["kw"]) + gate_phi(R, f) + unit(R))


def gate_em(R, n, S, f, n_iter=1):
    """-> (the gate of Sb', the gate of Sw') after n_iter rounds, f the largest factors over them."""
    g_phi, g_y = gate_phi(R, f), gate_yhat(R, f)
    return n_iter * (g_phi + 2 * g_y + 8.0 * (R + S) * EPS), n_iter * f["rho"] * (g_phi + 2 * g_y + 8.0 * (R + n) * EPS)


def gate_score(R, f):
    g_pc = f["kPc"] * (gate_phi(R, f) + unit(R)) + unit(R, f["kPc"])
    return f["amp_s"] * (g_pc + 2 * gate_yhat(R, f) + unit(R, f["kP0"]) + unit(R))


def gate_cov(R, n, kappa):
    return 8.0 * (R + n) * EPS * kappa


def gate_cosine(R, want):
    return 8.0 * R * EPS / float(np.max(np.abs(want)))


# ---- the shared, cached cases (read-only) ----

_CACHE = {}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def train_case(R, counts, n_iter=5):
    """The corpus, the start Sb = Sw = Sigma / 2, the restated rounds and the gate's factors after one round and over all."""
    key = ("train", R, counts, n_iter)
    if key not in _CACHE:
        c = corpus(R, counts, 100 * R + len(counts))
        half = total_cov(c["X"]) / 2.0
        mu, trace, worst = train(c["X"], c["ids"], half, half, n_iter)
        first = em_step(c["X"], c["ids"], mu, half, half, want_factors=True)[2]
        _CACHE[key] = _freeze(dict(c, start=half, mu=mu, trace=trace, first=first, worst=worst, kSigma=float(np.linalg.cond(2 * half))))
    return _CACHE[key]


def enrolment(mu, Sb, Sw, J, seed):
    """J models with 1 .. 7 enrolment vectors each (cycling, shuffled): -> (enrol [m, R], enrol_ids [m], the models' y [J, R])."""
    rng = np.random.default_rng(seed)
    R = mu.shape[0]
    counts = 1 + (np.arange(J) + seed) % 7
    y = rng.multivariate_normal(np.zeros(R), Sb, J, method="cholesky")
    ids = np.repeat(np.arange(J), counts)
    enrol = mu + y[ids] + rng.multivariate_normal(np.zeros(R), Sw, ids.size, method="cholesky")
    order = rng.permutation(ids.size)
    return np.ascontiguousarray(enrol[order]), np.ascontiguousarray(ids[order]), y


def score_case(R, J, T):
    """A model (mu, Sb, Sw of condition KAPPA_TRUE), J models of mixed counts, T test vectors (the first min(J, T) of them targets of
    the models in turn), the restated scores and the gate's factors."""
    key = ("score", R, J, T)
    if key not in _CACHE:
        rng = np.random.default_rng(7000 + 100 * R + J + T)
        Sb, Sw = 2.0 * spd(R, KAPPA_TRUE, rng), spd(R, KAPPA_TRUE, rng)
        mu = rng.standard_normal(R)
        enrol, ids, y = enrolment(mu, Sb, Sw, J, 3 + R + J)
        spk = rng.multivariate_normal(np.zeros(R), Sb, T, method="cholesky")
        k = min(J, T)
        spk[:k] = y[:k]
        X = mu + spk + rng.multivariate_normal(np.zeros(R), Sw, T, method="cholesky")
        E = np.zeros((J, R))
        np.add.at(E, ids, enrol)
        counts = np.bincount(ids, minlength=J)
        want, f = score(mu, Sb, Sw, E, counts, X, want_factors=True)
        _CACHE[key] = _freeze(dict(mu=mu, Sb=Sb, Sw=Sw, enrol=enrol, enrol_ids=ids, X=np.ascontiguousarray(X), E=E, counts=counts, want=want,
                                   factors=f))
    return _CACHE[key]


def transform_case(R, n):
    """n vectors of ceil(n / 4) classes (so that the within-class covariance has n - classes > R - 1 degrees of freedom where n > R
    allows it), with the restated whitening and WCCN and their condition numbers."""
    key = ("transform", R, n)
    if key not in _CACHE:
        n_cls = max(1, min(n // 4, n - R - 1))
        counts = tuple(n // n_cls + (1 if i < n % n_cls else 0) for i in range(n_cls))
        c = corpus(R, counts, 31 * R + n)
        mu, A = whiten(c["X"])
        _, Aw = whiten(c["X"], c["ids"], "wccn") if n - n_cls >= R else (None, None)
        _CACHE[key] = _freeze(dict(c, mu=mu, A=A, Aw=Aw, kSigma=float(np.linalg.cond(total_cov(c["X"]))),
                                   kW=float(np.linalg.cond(within_cov(c["X"], c["ids"]))) if Aw is not None else None))
    return _CACHE[key]


# The mutants: name -> (where it can show, what it is).  "train": em_step; "score": score; "transform": transform.
MUTANTS = {
    "transposed": ("train score transform", "a transposed operand: Yhat = F Phi Sw^-1 for F Sw^-1 Phi, (X - mu) A for (X - mu) A^T: shows at R > 1"),
    "weight": ("train", "n_i left out of Sw's last term: shows where a count is above 1"),
    "count": ("train score", "Phi of count c + 1"),
    "logdet": ("score", "ln det(Phi_c + Sw) dropped"),
    "edge": ("train score", "the ragged edge of a product zeroed: shows where R is no multiple of 16 (train), T none of 64 (score)"),
}


def mutant_shows(name, where, R, counts=(), T=0):
    """Can the mutant change anything on this case at all?"""
    if where not in MUTANTS[name][0].split():
        return False
    if name == "transposed":               # (with every count 1 all of a round's matrices are functions of the total covariance: they commute)
        return R > 1 and (where != "train" or max(counts) > 1)
    if name == "weight":
        return max(counts) > 1
    if name == "edge":
        return R % 16 != 0 or (where == "score" and T % 64 != 0)
    return True
