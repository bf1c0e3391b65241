"""Score calibration (csrc/calib.hip, speaker_recognition_amd/calibration.py) restated in numpy from the definitions, for the CPU and
the GPU tests: the evaluation of (f, g, H), the damped Newton loop with its pass and halving counts, apply, the error counts and
pool-adjacent-violators; a second statement of each (f through np.logaddexp, g and H by central differences in np.longdouble, min Cllr
over the convex hull of all thresholds' operating points); the input generator, the named mutants and the gate.

Definitions (float64):  X [S][n], lab [n] (1 target, 0 non-target, negative: skipped), theta = (w_1 .. w_S, b), z_i = sum_s w_s X[s][i]
+ b, tau = ln(P / (1 - P)), sp(a) = max(a, 0) + log1p(exp(-|a|)), c_i = P / n_t (targets) or (1 - P) / n_n (non-targets):
    f = (1 / ln 2) sum_i c_i sp(-+(z_i + tau)) + lam / 2 sum_s w_s^2
    g = (1 / ln 2) sum_i c_i (s_i - [target]) a_i + lam (w, 0)          a_i = (X[:, i], 1), s_i = 1 / (1 + exp(-(z_i + tau)))
    H = (1 / ln 2) sum_i c_i s_i (1 - s_i) a_i a_i^T + lam diag(1 .. 1, 0)

THE EVAL GATE, per component of f, g and H (derived here, not chosen):
    eps [ (log2(n) + C_LIBM) sum_i |term_i| + (S + 3) sum_i |d term_i / d z| sum_s |w_s X[s][i]| ]
eps = 2^-52.  The first part: a sum of n terms through a tree of depth <= log2(n) + a few loses at most one rounding per level relative
to the sum of magnitudes, and a term is formed from library calls whose documented bounds are: exp 1 ulp, log1p 1 ulp (HIP
programming guide, "HIP math API", table "Double precision mathematical functions": exp -- 1, log1p -- 1; the same bounds hold for
glibc's, which numpy calls), division correctly rounded (IEEE-754; 1 counted), and at most five further roundings where the term is
assembled (c x, e q, x q, h x_k, x x_l):  C_LIBM = 1 + 1 + 1 + 5 = 8.  The second part: z is a chain of S fused multiply-adds and the
sum with tau, at most S + 1 roundings of magnitude <= sum_s |w_s x_s| each (S + 3 leaves room for the offset's and tau's part), and an
error dz in z moves a term by |d term / d z| dz.  The ridge's parts (lam / 2 w^2, lam w, lam) enter sum |term|."""
import functools

import numpy as np

EPS = 2.0 ** -52
C_LIBM = 8
MAX_S = 8
BLOCK = 4096
PIVOT_REL = 16 * EPS
STOPS = ("CONVERGED", "CAP", "SINGULAR", "STALLED")
MUTANTS = ("no_class_weights", "no_tau", "ridge_on_offset", "no_ln2", "accept_always", "skip_as_non", "gt_threshold")
EVAL_MUTANTS = MUTANTS[:4] + ("skip_as_non",)


def _classes(lab, mutant=None):
    lab = np.asarray(lab).reshape(-1)
    tar = lab > 0
    non = (lab <= 0) if mutant == "skip_as_non" else (lab == 0)
    return tar, non


def _prep(X, lab, theta, P, dtype, mutant):
    X = np.asarray(X, dtype=np.float64).reshape(-1, np.asarray(lab).size)
    tar, non = _classes(lab, mutant)
    keep = tar | non
    x = np.where(keep[None, :], X, 0.0).astype(dtype)           # a select: a skipped position's score never enters the arithmetic
    th = np.asarray(theta, dtype=dtype)
    n_t, n_n = int(tar.sum()), int(non.sum())
    Pd = dtype(P)
    if mutant == "no_class_weights":
        c = np.where(keep, dtype(1) / dtype(n_t + n_n), dtype(0))
    else:
        c = np.where(tar, Pd / dtype(n_t), np.where(non, (dtype(1) - Pd) / dtype(n_n), dtype(0)))
    tau = dtype(0) if mutant == "no_tau" else np.log(Pd / (dtype(1) - Pd))
    z = th[-1] + (th[:-1, None] * x).sum(axis=0)
    a = np.vstack([x, np.ones((1, x.shape[1]), dtype=dtype)])
    return x, th, tar, non, c.astype(dtype), tau, z, a, (n_t, n_n, int((~keep).sum()))


def _outer_sum(a, h):
    """sum_i h_i a_i a_i^T, every entry by np.sum over a contiguous vector (pairwise: the restatement must itself stay inside the gate)."""
    p = a.shape[0]
    out = np.zeros((p, p), dtype=a.dtype)
    for k in range(p):
        ah = a[k] * h
        for l in range(k, p):
            out[k, l] = out[l, k] = (ah * a[l]).sum()
    return out


def evaluate(X, lab, theta, P=0.5, lam=0.0, dtype=np.float64, mutant=None, parts=False):
    """(f, g [S + 1], H [S + 1][S + 1], (n_t, n_n, skipped)) from the definitions.  ``parts``: also the gate's two sums per component."""
    x, th, tar, non, c, tau, z, a, counts = _prep(X, lab, theta, P, dtype, mutant)
    S = x.shape[0]
    v = z + tau
    e = np.exp(-np.abs(v))
    l1p = np.log1p(e)
    q = dtype(1) / (dtype(1) + e)
    s = np.where(v >= 0, q, e * q)
    oms = np.where(v >= 0, e * q, q)
    ln2 = dtype(1) if mutant == "no_ln2" else np.log(dtype(2))
    spv = np.maximum(np.where(tar, -v, v), 0) + l1p
    r = c * np.where(tar, -oms, s)
    h = c * s * oms
    w = th[:-1]
    ridge_w = th.copy() if mutant == "ridge_on_offset" else np.r_[w, dtype(0)]
    dtype_lam = dtype(lam)
    f = (c * spv).sum() / ln2 + dtype_lam / 2 * (ridge_w * ridge_w).sum()
    g = (a * r[None, :]).sum(axis=1) / ln2 + dtype_lam * ridge_w
    ridge_d = np.r_[np.ones(S), 1.0 if mutant == "ridge_on_offset" else 0.0].astype(dtype)
    H = _outer_sum(a, h) / ln2 + dtype_lam * np.diag(ridge_d)
    if not parts:
        return f, g, H, counts
    # the gate's sums, in float64
    f64 = lambda u: np.asarray(u, dtype=np.float64)           # noqa: E731
    wx = np.abs(f64(w)[:, None] * f64(x)).sum(axis=0)
    aa, cc, ss, oo = np.abs(f64(a)), f64(c), f64(s), f64(oms)
    il2 = 1.0 / np.log(2.0)
    t_f, d_f = cc * f64(spv) * il2, np.abs(f64(r)) * il2
    t_g, d_g = np.abs(f64(r))[None, :] * aa * il2, (cc * ss * oo)[None, :] * aa * il2
    hh = cc * ss * oo
    t_H = _outer_sum(aa, hh) * il2
    d_H = _outer_sum(aa, hh * np.abs(1.0 - 2.0 * ss) * wx) * il2
    lw = float(lam) * np.abs(f64(ridge_w))
    sums = {"f": (t_f.sum() + 0.5 * float(lam) * float((f64(w) ** 2).sum()), (d_f * wx).sum()),
            "g": (t_g.sum(axis=1) + lw, (d_g * wx[None, :]).sum(axis=1)),
            "H": (t_H + float(lam) * np.eye(S + 1), d_H)}
    return f, g, H, counts, sums


def gate(X, lab, theta, P=0.5, lam=0.0):
    """{"f": scalar, "g": [S + 1], "H": [S + 1][S + 1]}: the eval gate of the module text at this input."""
    sums = evaluate(X, lab, theta, P, lam, parts=True)[4]
    n = max(2, int((np.asarray(lab).reshape(-1) >= 0).sum()))
    S = np.asarray(theta).size - 1
    return {k: EPS * ((np.log2(n) + C_LIBM) * t + (S + 3) * d) for k, (t, d) in sums.items()}


def worst_ratio(got, ref, g):
    """max over the components of |got - ref| / gate; got / ref: (f, g, H)."""
    out = 0.0
    for key, a, b in zip(("f", "g", "H"), got, ref):
        diff = np.abs(np.asarray(a, dtype=np.longdouble) - np.asarray(b, dtype=np.longdouble)).astype(np.float64)
        out = max(out, float(np.max(diff / g[key])))
    return out


def f_logaddexp(X, lab, theta, P=0.5, lam=0.0, dtype=np.longdouble):
    """The second statement of f: sp(a) = logaddexp(0, a)."""
    x, th, tar, non, c, tau, z, a, _ = _prep(X, lab, theta, P, dtype, None)
    v = z + tau
    zero = np.zeros_like(v)
    return (c * np.where(tar, np.logaddexp(zero, -v), np.logaddexp(zero, v))).sum() / np.log(dtype(2)) + dtype(lam) / 2 * (th[:-1] ** 2).sum()


def central_differences(X, lab, theta, P=0.5, lam=0.0, h=1e-5):
    """(g by central differences of f_logaddexp, H by central differences of the analytic g, tol_g, tol_H) in np.longdouble.  The
    tolerances: a central difference is off by h^2 / 6 |third derivative| -- every derivative of the logistic function is at most 1/4
    in magnitude, so at most h^2 M3 with M3 = (1 / ln 2) sum_i c_i |a_i|_1^3 -- plus the rounding of the two values, 4 eps_ld F / h
    with F the sum of the magnitudes of what is differenced."""
    ld = np.longdouble
    th = np.asarray(theta, dtype=ld)
    p = th.size
    x, _, tar, non, c, tau, z, a, _ = _prep(X, lab, theta, P, ld, None)
    a1 = np.abs(a).sum(axis=0)
    il2 = 1 / np.log(ld(2))
    M3 = float((c * a1 ** 3).sum() * il2) + 1.0
    F = float((c * (np.abs(z + tau) + 1) * (1 + a1)).sum() * il2) + float(lam) * float((th ** 2).sum() + np.abs(th).sum() + 1)
    eps_ld = float(np.finfo(ld).eps)
    g, H = np.zeros(p, dtype=ld), np.zeros((p, p), dtype=ld)
    for k in range(p):
        dk = np.zeros(p, dtype=ld)
        dk[k] = ld(h)
        g[k] = (f_logaddexp(X, lab, th + dk, P, lam) - f_logaddexp(X, lab, th - dk, P, lam)) / (2 * ld(h))
        H[:, k] = (evaluate(X, lab, th + dk, P, lam, dtype=ld)[1] - evaluate(X, lab, th - dk, P, lam, dtype=ld)[1]) / (2 * ld(h))
    tol = h * h * M3 + 4 * eps_ld * F / h
    return g, H, tol, tol * float(1 + a1.max())


# ---- the loop ----

def cholesky_solve(H, g):
    """(d = -H^-1 g, lam2 = -g^T d) or None where a pivot is not above 16 eps of its diagonal element or not finite."""
    p = g.size
    L = np.zeros((p, p))
    for j in range(p):
        piv = H[j, j] - float(np.dot(L[j, :j], L[j, :j]))
        if not (piv > PIVOT_REL * H[j, j]) or not np.isfinite(piv):
            return None
        L[j, j] = np.sqrt(piv)
        for i in range(j + 1, p):
            L[i, j] = (H[i, j] - float(np.dot(L[i, :j], L[j, :j]))) / L[j, j]
    y = np.zeros(p)
    for i in range(p):
        y[i] = (-g[i] - float(np.dot(L[i, :i], y[:i]))) / L[i, i]
    d = np.zeros(p)
    for i in range(p - 1, -1, -1):
        d[i] = (y[i] - float(np.dot(L[i + 1:, i], d[i + 1:]))) / L[i, i]
    return d, -float(np.dot(g, d))


def fit(X, lab, P=0.5, lam=0.0, theta0=None, tol=1e-16, max_pass=100, mutant=None):
    """The damped Newton loop of the issue.  -> dict(theta, f, passes, accepted, halvings, stop, lam2s, margins): lam2s the sequence of
    Newton decrements, margins |f_new - f| of every accept decision."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, np.asarray(lab).size)
    S = X.shape[0]
    theta = np.zeros(S + 1) if theta0 is None else np.array(theta0, dtype=np.float64)
    ev = lambda th: evaluate(X, lab, th, P, lam, mutant=mutant if mutant in EVAL_MUTANTS else None)[:3]          # noqa: E731
    out = dict(passes=1, accepted=0, halvings=0, lam2s=[], margins=[], thetas=[])
    with np.errstate(over="ignore", invalid="ignore"):
        f, g, H = ev(theta)
        while True:
            sol = cholesky_solve(H, g)
            if sol is None or not np.isfinite(sol[1]) or not np.all(np.isfinite(theta + sol[0])):
                stop = 2
                break
            d, lam2 = sol
            out["lam2s"].append(lam2)
            if lam2 <= tol:
                stop = 0
                break
            t, stop = 1.0, None
            while True:
                if out["passes"] == max_pass:
                    stop = 1
                    break
                out["passes"] += 1
                f_new, g_new, H_new = ev(theta + t * d)
                out["margins"].append((abs(float(f_new) - float(f)), theta + t * d))
                if mutant == "accept_always" or (np.isfinite(f_new) and f_new <= f):
                    theta, f, g, H = theta + t * d, f_new, g_new, H_new
                    out["accepted"] += 1
                    break
                t /= 2
                out["halvings"] += 1
                if t < 2.0 ** -20:
                    stop = 3
                    break
            if stop is not None:
                break
    out.update(theta=theta, f=float(f), g=g, H=H, stop=STOPS[stop])
    return out


def loop_is_decided(X, lab, P, lam, r, tol=1e-16):
    """The two conditions under which pass counts, halvings and the stop code may be asserted equal: no Newton decrement within a
    factor 100 of tol on either side, and no accept decision with |f_new - f| within 100 gates of f."""
    for l2 in r["lam2s"]:
        if tol > 0 and tol / 100 < l2 < tol * 100:
            return False
    for margin, th in r["margins"]:
        if np.all(np.isfinite(th)) and np.isfinite(margin) and margin <= 100 * gate(X, lab, th, P, lam)["f"]:
            return False
    return True


def optimality(X, lab, theta, P, lam, tol=1e-16):
    """(g^T H^-1 g at theta by the restatement, the bound max(tol, floor)): floor is the eval gate on g propagated through H^-1,
    (|H^-1| gate_g)^T |H| (|H^-1| gate_g) <= ... taken as gate_g^T |H^-1| gate_g."""
    f, g, H, _ = evaluate(X, lab, theta, P, lam)
    Hi = np.linalg.inv(H)
    gg = gate(X, lab, theta, P, lam)["g"]
    return float(g @ Hi @ g), max(tol, float(gg @ np.abs(Hi) @ gg))


def equal_weights_bound(X, lab, theta, P, lam, tol=1e-16):
    """How far apart the weights of two identical systems may end.  Along (1, -1) / sqrt(2) the data's part of H vanishes and the ridge
    alone curves f, so a point within the optimality criterion c = g^T H^-1 g <= max(tol, floor) of the optimum has
    lam (w_1 - w_2)^2 / 2 <= c."""
    return float(np.sqrt(2 * optimality(X, lab, theta, P, lam, tol)[1] / lam))


def apply(X, theta):
    X = np.asarray(X, dtype=np.float64)
    X = X.reshape(1, -1) if X.ndim == 1 else X
    th = np.asarray(theta, dtype=np.float64)
    z = (th[:-1, None] * X).sum(axis=0) + th[-1]
    return z, (X.shape[0] + 1) * EPS * (np.abs(th[:-1, None] * X).sum(axis=0) + abs(th[-1]))


def counts(llr, lab, thr, mutant=None):
    """(misses [m], false alarms [m]): accept iff llr >= thr."""
    llr, lab = np.asarray(llr, dtype=np.float64).reshape(-1), np.asarray(lab).reshape(-1)
    tar, non = _classes(lab, mutant if mutant == "skip_as_non" else None)
    llr = np.where(tar | non, llr, 0.0)
    thr = np.asarray(thr, dtype=np.float64).reshape(-1)
    acc = (llr[None, :] > thr[:, None]) if mutant == "gt_threshold" else (llr[None, :] >= thr[:, None])
    return (tar[None, :] & ~acc).sum(axis=1), (non[None, :] & acc).sum(axis=1)


def act_dcf(llr, lab, p_target=0.01, c_miss=1.0, c_fa=1.0, mutant=None):
    thr = np.log(c_fa * (1 - p_target) / (c_miss * p_target))
    miss, fa = counts(llr, lab, [thr], mutant)
    lab = np.asarray(lab).reshape(-1)
    p_miss, p_fa = miss[0] / (lab > 0).sum(), fa[0] / (lab == 0).sum()
    return float((c_miss * p_target * p_miss + c_fa * (1.0 - p_target) * p_fa) / min(c_miss * p_target, c_fa * (1.0 - p_target)))


def cllr(llr, lab):
    return float(evaluate(np.asarray(llr, dtype=np.float64).reshape(1, -1), lab, [1.0, 0.0])[0])


def _cllr_of_blocks(bt, bn):
    bt, bn = np.asarray(bt, dtype=np.float64), np.asarray(bn, dtype=np.float64)
    n_t, n_n = bt.sum(), bn.sum()
    tot = 0.0
    for t, m in zip(bt, bn):
        if t > 0 and m > 0:
            l = np.log(t / m) - np.log(n_t / n_n)
            tot += t / n_t * np.logaddexp(0, -l) + m / n_n * np.logaddexp(0, l)
    return float(0.5 * tot / np.log(2))


def pav(llr, lab):
    """(targets, non-targets) of the blocks pool-adjacent-violators leaves along ascending score; ties enter as one group."""
    llr, lab = np.asarray(llr, dtype=np.float64).reshape(-1), np.asarray(lab).reshape(-1)
    keep = lab >= 0
    llr, tar = llr[keep], lab[keep] > 0
    blocks = []
    for v in np.unique(llr):
        m = llr == v
        blocks.append([int(tar[m].sum()), int((~tar[m]).sum())])
        while len(blocks) > 1 and blocks[-2][0] * sum(blocks[-1]) >= blocks[-1][0] * sum(blocks[-2]):
            t, m2 = blocks.pop()
            blocks[-1][0] += t
            blocks[-1][1] += m2
    return [b[0] for b in blocks], [b[1] for b in blocks]


def min_cllr(llr, lab):
    return _cllr_of_blocks(*pav(llr, lab))


def min_cllr_hull(llr, lab):
    """The second statement (n <= 12): the operating points (false alarms, hits) of every threshold, their upper convex hull by brute
    force over all pairs of points, a block per hull edge."""
    llr, lab = np.asarray(llr, dtype=np.float64).reshape(-1), np.asarray(lab).reshape(-1)
    keep = lab >= 0
    llr, tar = llr[keep], lab[keep] > 0
    assert llr.size <= 12
    pts = [(0, 0)] + [(int((~tar & (llr >= v)).sum()), int((tar & (llr >= v)).sum())) for v in sorted(set(llr.tolist()), reverse=True)]
    on = []
    for i, (x0, y0) in enumerate(pts):
        for j, (x1, y1) in enumerate(pts):
            if j > i and all((x1 - x0) * (y - y0) - (y1 - y0) * (x - x0) <= 0 for x, y in pts):
                on.append((i, j))
    verts = sorted(set(i for e in on for i in e))
    bt = [pts[b][1] - pts[a][1] for a, b in zip(verts[:-1], verts[1:])]
    bn = [pts[b][0] - pts[a][0] for a, b in zip(verts[:-1], verts[1:])]
    return _cllr_of_blocks(bt[::-1], bn[::-1])


# ---- inputs ----

PARITY_S = (1, 2, 8)
PARITY_N = (2, 255, 256, 257, 4095, 4096, 4097, 8193, 257 * 4096 + 1)
PARITY_P = (0.5, 0.01)
PARITY_CASES = [(S, n, P) for S in PARITY_S for n in PARITY_N for P in PARITY_P]
PARITY_LAM = 0.01
BIG_CASE = (2, 4097, 0.5)           # |z| up to 1e4, theta at scale 1e3


@functools.lru_cache(maxsize=4)
def inputs(S, n, seed=0, skip=True, scale=1.0, offset=0.0, separable=False):
    """X [S][n], lab [n] int8: about 30 % targets, a tenth of the labels skipped (-1), at least one trial of each class; system s
    scores a target around +(1/2 + s / 8) and a non-target around -(1/2 + s / 8) with unit noise of its own and 0.3 of a noise the systems share."""
    rng = np.random.default_rng(1000 * S + n % 9973 + 7 * seed)
    lab = (rng.random(n) < 0.3).astype(np.int8)
    if skip and n > 2:
        lab[rng.random(n) < 0.1] = -1
    lab[0], lab[n - 1] = 1, 0
    sign = np.where(lab > 0, 1.0, -1.0)
    common = rng.standard_normal(n)
    X = np.stack([sign * (0.5 + s / 8) + (0.1 if separable else 1.0) * (0.3 * common + rng.standard_normal(n)) for s in range(S)])
    X = X * scale + offset
    X.setflags(write=False)
    lab.setflags(write=False)
    return X, lab


def parity_theta(S, seed=0, scale=1.0):
    rng = np.random.default_rng(77 + S + seed)
    return np.r_[rng.standard_normal(S) * 0.8 / np.sqrt(S), 0.3] * scale


@functools.lru_cache(maxsize=2)
def parity_reference(S, n, P):
    """(the np.longdouble statement (f, g, H), the gate) of a parity case: computed once, shared, never changed."""
    X, lab = inputs(S, n)
    th = parity_theta(S)
    ref = evaluate(X, lab, th, P, PARITY_LAM, dtype=np.longdouble)[:3]
    return ref, gate(X, lab, th, P, PARITY_LAM)


def big_inputs():
    S, n, P = BIG_CASE
    X, lab = inputs(S, n, seed=3)
    th = parity_theta(S, seed=3, scale=1e3)
    k = 9.5e3 / float(np.abs((th[:-1, None] * X).sum(axis=0)).max())          # |z| up to 9.5e3 + |b| = 9.8e3
    return X * k, lab, th, P


# fit inputs by name: (S, n, P, lam, generator keywords, theta0)
FIT_CASES = {
    "hand4": None,
    "n257_S2_P01": (2, 257, 0.01, 0.0, {}, None),
    "n4097_S8": (8, 4097, 0.5, 0.0, dict(seed=2), None),
    "scaled_1e3": (2, 257, 0.5, 0.0, dict(scale=1e3), None),
    "scaled_1e-3": (2, 257, 0.5, 0.0, dict(scale=1e-3), None),
    "offset_100": (1, 4097, 0.5, 0.0, dict(offset=100.0, seed=3), None),
    "halving": (1, 257, 0.5, 0.0, {}, (6.0, -4.0))          # a start far beyond the optimum: the full step overshoots,
}


def fit_inputs(name):
    """-> (X, lab, P, lam, theta0)."""
    if name == "hand4":            # two targets 2, -1 and two non-targets 1, -1.5: overlapping, so the optimum is finite
        return np.array([[2.0, -1.0, 1.0, -1.5]]), np.array([1, 1, 0, 0], dtype=np.int8), 0.5, 0.0, None
    S, n, P, lam, kw, th0 = FIT_CASES[name]
    X, lab = inputs(S, n, **kw)
    return X, lab, P, lam, None if th0 is None else np.array(th0)


def counts_inputs(n=8193):
    """llr [n] with every tenth value exactly on a threshold, labels with skipped entries, and 16 thresholds with -inf and +inf."""
    X, lab = inputs(1, n, seed=5)
    thr = np.r_[-np.inf, np.linspace(-3, 3, 14), np.inf]
    llr = X[0].copy()
    llr[::10] = thr[1 + (np.arange(llr[::10].size) % 14)]
    return llr, lab, thr
