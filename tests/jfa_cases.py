"""The float64 numpy restatement of the JFA factor estimation (csrc/jfa.hip, jfa.py) and the generators its tests share.

Written from the formulas, with ``np.linalg.inv`` where the reference's estimate_y_and_v.m / estimate_x_and_u.m call ``inv``: for
every group g (a speaker, or a session), a loading matrix W [R, K D], variances E, occupancies N [G, K] and centred first-order
statistics Fc [G, K D]:
    P_c = W_c diag(1 / E_c) W_c^T        L_g = I + sum_c N[g, c] P_c        b_g = W (Fc_g / E)
    y_g = L_g^-1 b_g                     Q_g = L_g^-1 + y_g y_g^T
    A_c = sum_g N[g, c] Q_g              C = sum_g y_g Fc_g^T               W_c <- A_c^-1 C_c
``spk_ids`` are 0-based here as in jfa.py.  The step is the EM update of  J(W) = sum_g ( -1/2 ln det L_g + 1/2 b_g^T L_g^-1 b_g ),
the part of the marginal log-likelihood of the statistics that depends on W: tests/test_jfa_cpu.py checks that it never decreases.
"""
import numpy as np

EPS = 2.0 ** -52
SHAPES = ((12, 8, 5, 7), (40, 17, 13, 17), (70, 5, 39, 65), (6, 4, 3, 9))          # (G, K, D, R)


# ---- the computation ----

def grams(E, W, K):
    D = W.shape[1] // K
    return np.stack([(W[:, c * D:(c + 1) * D] / E[c * D:(c + 1) * D]) @ W[:, c * D:(c + 1) * D].T for c in range(K)])


def precisions(N, E, W):
    """L [G, R, R]."""
    P = grams(E, W, N.shape[1])
    return np.eye(W.shape[0])[None] + np.einsum("gc,cij->gij", N, P)


def factors(N, Fc, E, W):
    """-> y [G, R], A [K, R, R], C [R, K D]."""
    G, K = N.shape
    R = W.shape[0]
    L = precisions(N, E, W)
    y = np.zeros((G, R))
    A = np.zeros((K, R, R))
    C = np.zeros_like(W)
    for g in range(G):
        invL = np.linalg.inv(L[g])
        y[g] = ((Fc[g] / E) @ W.T) @ invL
        Q = invL + np.outer(y[g], y[g])
        A += N[g][:, None, None] * Q[None]
        C += np.outer(y[g], Fc[g])
    return y, A, C


def factors_solve(N, Fc, E, W):
    """The same by Cholesky solves instead of inv (the form the device takes)."""
    G, K = N.shape
    R = W.shape[0]
    L = precisions(N, E, W)
    y = np.zeros((G, R))
    A = np.zeros((K, R, R))
    C = np.zeros_like(W)
    for g in range(G):
        Lc = np.linalg.cholesky(L[g])
        y[g] = np.linalg.solve(Lc.T, np.linalg.solve(Lc, W @ (Fc[g] / E)))
        X = np.linalg.solve(Lc, np.eye(R))
        Q = X.T @ X + np.outer(y[g], y[g])
        A += N[g][:, None, None] * Q[None]
        C += np.outer(y[g], Fc[g])
    return y, A, C


def factors_ok(A_c):
    """Does the block factor?  (a pivot <= 0 or not finite fails: the device's rule)"""
    if not np.isfinite(A_c).all():
        return False
    try:
        np.linalg.cholesky(A_c)
        return True
    except np.linalg.LinAlgError:
        return False


def update(A, C, W, solve=False):
    """W_c = A_c^-1 C_c; a mixture whose A_c does not factor keeps the old W_c.  -> (W_new, skipped)."""
    K = A.shape[0]
    D = W.shape[1] // K
    out = np.array(W, dtype=np.float64)
    skipped = 0
    for c in range(K):
        if not factors_ok(A[c]):
            skipped += 1
            continue
        cols = slice(c * D, (c + 1) * D)
        out[:, cols] = np.linalg.solve(A[c], C[:, cols]) if solve else np.linalg.inv(A[c]) @ C[:, cols]
    return out, skipped


def step(N, Fc, E, W, solve=False):
    y, A, C = (factors_solve if solve else factors)(N, Fc, E, W)
    return update(A, C, W, solve)[0], y, A, C


def train(N, Fc, E, W, n_iter, solve=False):
    """-> (W, y of the last round, [W after every round])."""
    trace = []
    y = None
    for _ in range(n_iter):
        W, y, _, _ = step(N, Fc, E, W, solve)
        trace.append(W)
    return W, y, trace


def objective(N, Fc, E, W):
    L = precisions(N, E, W)
    b = (Fc / E) @ W.T
    J = 0.0
    for g in range(N.shape[0]):
        sign, logdet = np.linalg.slogdet(L[g])
        assert sign > 0
        J += -0.5 * logdet + 0.5 * b[g] @ np.linalg.solve(L[g], b[g])
    return J


def cond_L(N, E, W):
    return max(float(np.linalg.cond(Lg)) for Lg in precisions(N, E, W))


def cond_A(A):
    return max(float(np.linalg.cond(Ac)) for Ac in A if factors_ok(Ac))


def rel(got, want):
    """The largest difference relative to the largest magnitude of the restated array."""
    scale = float(np.max(np.abs(want))) if np.size(want) else 0.0
    return float(np.max(np.abs(np.asarray(got) - want))) / scale if scale > 0 else float(np.max(np.abs(got), initial=0.0))


def gate_y(R, K, D, kL):
    """Forward error of a backward-stable solve plus the K- and K D-term sums that form L and b in another order."""
    return 8.0 * (R + K * D) * EPS * kL


def gate_update(R, kA):
    return 8.0 * R * EPS * kA


def gate_step(R, K, D, kL, kA):
    return kA * 4.0 * gate_y(R, K, D, kL) + gate_update(R, kA)


# ---- reference-shaped entry points (0-based labels) ----

def _expand(N, kd):
    return np.repeat(N, kd // N.shape[1], axis=1)


def _mat(a, n, w):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim < 2:
        a = a.reshape(-1, 1) if a.size > 1 else a.reshape(1, 1)
    return np.broadcast_to(a if a.shape[0] == 1 else a[:n], (n, w if a.shape[1] == 1 else a.shape[1]))


def _prod(f, W, n, kd):
    W = np.asarray(W, dtype=np.float64)
    if W.ndim < 2:
        return np.zeros((n, kd)) + _mat(f, n, 1)[:, :1] * W
    return _mat(f, n, W.shape[0]) @ W


def _vec(d, kd):
    return np.broadcast_to(np.asarray(d, dtype=np.float64).reshape(-1), (kd,))


def estimate_y_and_v(F, N, S, m, E, d, v, u, z, y, x, spk_ids, nargout=1):
    F, N = np.asarray(F, dtype=np.float64), np.asarray(N, dtype=np.float64)
    n, kd = F.shape
    ids = np.asarray(spk_ids).reshape(-1)
    n_spk = int(ids.max()) + 1
    Nx = _expand(N, kd)
    xu = _prod(x, u, n, kd)
    zd = _mat(z, n_spk, kd) * _vec(d, kd)
    present = np.unique(ids)
    Ns = np.zeros((len(present), N.shape[1]))
    Fs = np.zeros((len(present), kd))
    for i, ii in enumerate(present):
        rows = np.flatnonzero(ids == ii)
        Ns[i] = N[rows].sum(axis=0)
        Fs[i] = F[rows].sum(axis=0) - (m + zd[ii]) * np.repeat(Ns[i], kd // N.shape[1])
        for jj in rows:
            Fs[i] -= xu[jj] * Nx[jj]
    yy, A, C = factors(Ns, Fs, E, v)
    out = np.zeros((n_spk, v.shape[0]))
    out[present] = yy
    if nargout == 1:
        return out
    return (out, A, C) if nargout == 3 else (out, update(A, C, v)[0])


def estimate_x_and_u(F, N, S, m, E, d, v, u, z, y, x, spk_ids, nargout=1):
    F, N = np.asarray(F, dtype=np.float64), np.asarray(N, dtype=np.float64)
    n, kd = F.shape
    ids = np.asarray(spk_ids).reshape(-1)
    n_spk = int(ids.max()) + 1
    shift = m + _prod(y, v, n_spk, kd) + _mat(z, n_spk, kd) * _vec(d, kd)
    Fh = F - _expand(N, kd) * shift[ids]
    xx, A, C = factors(N, Fh, E, u)
    if nargout == 1:
        return xx
    return (xx, A, C) if nargout == 3 else (xx, update(A, C, u)[0])


def estimate_z_and_d(F, N, S, m, E, d, v, u, z, y, x, spk_ids, nargout=1):
    F, N = np.asarray(F, dtype=np.float64), np.asarray(N, dtype=np.float64)
    n, kd = F.shape
    ids = np.asarray(spk_ids).reshape(-1)
    n_spk = int(ids.max()) + 1
    Nx = _expand(N, kd)
    yv = _prod(y, v, n_spk, kd)
    xu = _prod(x, u, n, kd)
    dv = _vec(d, kd)
    zz = np.zeros((n_spk, kd))
    a = np.zeros(kd)
    b = np.zeros(kd)
    for ii in np.unique(ids):
        rows = np.flatnonzero(ids == ii)
        Ns = Nx[rows].sum(axis=0)
        Fs = F[rows].sum(axis=0) - (m + yv[ii]) * Ns
        for jj in rows:
            Fs = Fs - xu[jj] * Nx[jj]
        L = 1.0 + Ns / E * dv ** 2
        zz[ii] = Fs / E * dv / L
        a += (1.0 / L + zz[ii] ** 2) * Ns
        b += zz[ii] * Fs
    if nargout == 1:
        return zz
    return (zz, a, b) if nargout == 3 else (zz, b / a)


def linear_scoring(F, N, S, m, E, d, v, u, z, y, x):
    F, N = np.asarray(F, dtype=np.float64), np.asarray(N, dtype=np.float64)
    n, kd = F.shape
    y = np.atleast_2d(y)
    n_mod = y.shape[0]
    M = (_mat(z, n_mod, kd) * _vec(d, kd) + y @ v) / E
    Fc = (F - (m + _prod(x, u, n, kd)) * _expand(N, kd)) / N.sum(axis=1, keepdims=True)
    return M @ Fc.T


def score_dot_product(trn, tst, m, E, v, u, d):
    """The chain of sc_score_dot_product.m on ``(F, N)`` pairs."""
    (tF, tN), (sF, sN) = trn, tst
    ny = v.shape[0]
    vu = np.vstack([v, u])
    tid, sid = np.arange(tN.shape[0]), np.arange(sN.shape[0])
    yx = estimate_y_and_v(tF, tN, None, m, E, d, vu, 0, 0, 0, 0, tid)
    tz = estimate_z_and_d(tF, tN, None, m, E, d, vu, 0, 0, yx, 0, tid)
    sx = estimate_x_and_u(sF, sN, None, m, E, d, v, u, 0, 0, 0, sid)
    return linear_scoring(sF, sN, None, m, E, d, v, u, tz, yx[:, :ny], sx)


# ---- generators ----

def random_start(R, E, seed=0):
    """The sc_* scripts' start, randn(R, K D) * sum(E) * 0.001, from numpy's RandomState (jfa.random_loadings)."""
    return np.random.RandomState(seed).randn(R, E.size) * E.sum() * 0.001


def corpus(G, K, D, R, seed, sessions=3, ubm=None):
    """A synthetic corpus of G speakers x `sessions` sessions: E from uniform(0.3, 1.5)^2, m normal, a true loading matrix
    normal(0, 0.3), sessions of 50 .. 400 frames with Dirichlet(2) occupancies, F = N (m + y v + 0.05 noise) + sqrt(N E) noise.
    ``ubm`` = (weights, means [K, D], variances [K, D]): m and E from it instead.
    -> dict(F [S, K D], N [S, K], spk_ids [S], m, E, v_true)."""
    rng = np.random.default_rng(seed)
    kd = K * D
    E = rng.uniform(0.3, 1.5, kd) ** 2
    m = rng.standard_normal(kd)
    if ubm is not None:
        m, E = np.asarray(ubm[1], dtype=np.float64).reshape(-1), np.asarray(ubm[2], dtype=np.float64).reshape(-1)
    v = rng.normal(0.0, 0.3, (R, kd))
    ids = np.repeat(np.arange(G), sessions)
    y = rng.standard_normal((G, R))
    frames = rng.integers(50, 401, G * sessions).astype(np.float64)
    N = frames[:, None] * rng.dirichlet(np.full(K, 2.0), G * sessions)
    Nx = np.repeat(N, D, axis=1)
    F = Nx * (m + y[ids] @ v + 0.05 * rng.standard_normal((G * sessions, kd))) + np.sqrt(Nx * E) * rng.standard_normal((G * sessions, kd))
    return dict(F=F, N=N, spk_ids=ids, m=m, E=E, v_true=v)


def centred(c):
    """The speakers' statistics of a corpus, centred on m: (Ns [G, K], Fs [G, K D])."""
    ids = c["spk_ids"]
    G = int(ids.max()) + 1
    K = c["N"].shape[1]
    kd = c["F"].shape[1]
    Ns = np.zeros((G, K))
    Fs = np.zeros((G, kd))
    np.add.at(Ns, ids, c["N"])
    np.add.at(Fs, ids, c["F"])
    return Ns, Fs - c["m"] * np.repeat(Ns, kd // K, axis=1)


_CASES = {}


def case(G, K, D, R, seed=None, n_iter=0):
    """The shared, cached case of a shape: statistics, the random start, the restated first step, condition numbers and, with
    n_iter, the restated training trace.  Treat what it returns as read-only."""
    key = (G, K, D, R, seed, n_iter)
    if key in _CASES:
        return _CASES[key]
    c = corpus(G, K, D, R, 1000 * G + 10 * K + R if seed is None else seed)
    Ns, Fs = centred(c)
    E = c["E"]
    W0 = random_start(R, E, 1)
    y, A, C = factors(Ns, Fs, E, W0)
    W1, _ = update(A, C, W0)
    out = dict(c, Ns=Ns, Fs=Fs, W0=W0, y=y, A=A, C=C, W1=W1, kL=cond_L(Ns, E, W0), kA=cond_A(A))
    if n_iter:
        W, yl, trace = train(Ns, Fs, E, W0, n_iter)
        kL, kA = out["kL"], out["kA"]
        for Wt in trace[:-1]:
            kL = max(kL, cond_L(Ns, E, Wt))
            kA = max(kA, cond_A(factors(Ns, Fs, E, Wt)[1]))
        out.update(W_train=W, y_train=yl, trace=trace, kL_train=kL, kA_train=kA)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASES[key] = out
    return out


# ---- the sc_* driver scripts, restated (jfa.train_v / train_u / train_d) ----

def train_v(F, N, ids, m, E, ny, niter, seed=0):
    c = dict(F=F, N=N, spk_ids=ids, m=m)
    Ns, Fs = centred(c)
    present = np.unique(ids)
    return train(Ns[present], Fs[present], E, random_start(ny, E, seed), niter)[0]


def train_u(F, N, ids, m, E, v, nx, niter, seed=0):
    y = estimate_y_and_v(F, N, None, m, E, 0, v, 0, 0, 0, 0, ids)
    Fh = F - _expand(N, F.shape[1]) * (m + y @ v)[ids]
    return train(N, Fh, E, random_start(nx, E, seed), niter)[0]


def train_d(F, N, ids, m, E, v, u, niter, seed=0):
    y = estimate_y_and_v(F, N, None, m, E, 0, v, 0, 0, 0, 0, ids)
    x = estimate_x_and_u(F, N, None, m, E, 0, v, u, 0, y, 0, ids)
    d = random_start(1, E, seed)[0]
    for _ in range(niter):
        _, d = estimate_z_and_d(F, N, None, m, E, d, v, u, 0, y, x, ids, nargout=2)
    return d
