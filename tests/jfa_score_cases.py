"""The float64 numpy restatements of JFA trial scoring (csrc/jfa_score.hip, jfa.score_trials) and what its tests share.

``kscore_m`` is a loop-for-loop transliteration of the reference's kscore_famous_19.m, in that file's own (column) orientation and
with its per-pair arithmetic -- ``chol(L, 'lower') \\ u'`` per segment, then ``MNe``, ``Fse``, ``lin``, ``quad``, ``quad2`` per
pair -- so that the device's restated chain (G once per call, h as one product) is checked against the reference's order of
operations, not against itself.  One stated difference: the UBM's score is subtracted from every score, also from one that is
exactly 0 (the reference skips those).  ``linear_m`` is linear_scoring.m the same way.

The generator (``inputs``): the segments are ``jfa_cases.corpus(T, K, D, Ry, 1000 T + 10 K + Ru, sessions=1)`` (its F, N, m, E and
its true loading matrix as v); the other inputs come from ``default_rng(7 T + J)`` in this order: u ~ normal(0, 0.3),
y ~ standard_normal, z ~ 0.1 standard_normal, d ~ uniform(0.1, 0.5), and for linear mode x ~ 0.3 standard_normal.

Gates, with eps = 2^-52, absolute differences of scores:
  integrated   g_s = 8 (Ry + Ru + K D) eps kappa_L max over pairs of max(|lin|, |quad| / 2, |quad2| / 2) / n_t, kappa_L the largest
               2-norm condition number of the L_t (asserted <= 1e6 first): the sums over Ry, Ru and K D terms taken in another
               order, the forward error of the triangular solve, relative to the largest of the three terms a score is the
               difference of;
  linear       8 (Ry + Ru + K D) eps max over pairs of sum_i |M_j[i] / E[i]| (|F[t][i]| + N |m + x u|[i]) / n_t: a sum of K D
               terms of those magnitudes, each carrying the errors of the Ry- and Ru-term sums inside it.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfa_cases as jc  # noqa: E402

EPS = jc.EPS
# (T, J, K, D, Ry, Ru)
SHAPES = ((1, 1, 1, 1, 1, 1), (3, 2, 4, 13, 3, 2), (5, 70, 5, 1, 4, 16), (33, 17, 17, 39, 17, 17), (4, 3, 65, 13, 5, 16), (5, 4, 4, 13, 3, 65),
          (2, 260, 3, 2, 2, 5), (3, 5, 6, 13, 4, 130))
LINEAR_SHAPES = (SHAPES[1], SHAPES[2], SHAPES[3], SHAPES[4])
BIG = SHAPES[3]


def kscore_m(F, N, m, E, d, v, u, z, y, scores=None):
    """kscore_famous_19.m.  F [K D, T], N [K, T], m, E, d [K D], v [K D, Ry], u [K D, Ru], z [K D, J], y [Ry, J], scores: the mask
    [J, T] or None.  -> dict(scores [J, T], lin, quad, quad2 [J + 1, T] (row 0: the UBM), kappa [T], sum_N [T])."""
    dim = F.shape[0] // N.shape[0]
    n_mix, n_seg = N.shape
    index_map = np.repeat(np.arange(n_mix), dim)
    M = np.tile(m[:, None], (1, y.shape[1])) + z * np.tile(d[:, None], (1, y.shape[1])) + v @ y
    M = np.hstack([m[:, None], M])
    uEuT = []
    for c in range(n_mix):
        el = slice(c * dim, (c + 1) * dim)
        uEuT.append(u[el].T @ (np.tile((1.0 / E[el])[:, None], (1, u.shape[1])) * u[el]))
    sum_N = N.sum(axis=0)
    mask = np.ones((M.shape[1], n_seg)) if scores is None else np.vstack([np.ones((1, n_seg)), np.asarray(scores, dtype=np.float64)])
    out = np.array(mask)
    lin_a, quad_a, quad2_a = (np.zeros_like(out) for _ in range(3))
    kappa = np.zeros(n_seg)
    for ii in range(n_seg):
        Nt = N[index_map, ii]
        Nte = Nt / E
        Fte = F[:, ii] / E
        L = np.eye(u.shape[1])
        for c in range(n_mix):
            L = L + uEuT[c] * N[c, ii]
        kappa[ii] = np.linalg.cond(L)
        cholLu = np.linalg.solve(np.linalg.cholesky(L), u.T)
        for jj in range(M.shape[1]):
            if mask[jj, ii] == 1:
                MNe = Nte * M[:, jj]
                Fse = Fte - MNe
                lin = Fte @ M[:, jj]
                quad = MNe @ M[:, jj]
                quad2 = cholLu @ Fse
                quad2 = quad2 @ quad2
                out[jj, ii] = (lin - 0.5 * quad + 0.5 * quad2) / sum_N[ii]
                lin_a[jj, ii], quad_a[jj, ii], quad2_a[jj, ii] = lin, quad, quad2
    ubm = out[0]
    final = np.where(mask[1:] == 1, out[1:] - ubm[None], 0.0)           # (the reference: only where the score is not exactly 0)
    return dict(scores=final, lin=lin_a, quad=quad_a, quad2=quad2_a, kappa=kappa, sum_N=sum_N)


def linear_m(F, N, m, E, d, v, u, z, y, x):
    """linear_scoring.m, its own (row) orientation.  -> (scores [J, T], the gate's magnitude sum per pair [J, T])."""
    M = z * np.tile(d[None], (z.shape[0], 1)) + y @ v
    M = M / np.tile(E[None], (M.shape[0], 1))
    shifts = np.tile(m[None], (F.shape[0], 1)) + x @ u
    dim = F.shape[1] // N.shape[1]
    index_map = np.repeat(np.arange(N.shape[1]), dim)
    shifts = shifts * N[:, index_map]
    sum_N = N.sum(axis=1, keepdims=True)
    Fc = (F - shifts) / sum_N
    mag = np.abs(M) @ ((np.abs(F) + np.abs(shifts)) / sum_N).T
    return M @ Fc.T, mag


def restated(F, N, m, E, d, v, u, z, y):
    """The device's chain in numpy, row orientation: G once per call, h as one product over K.  -> scores [J, T]."""
    T, K = N.shape
    kd = F.shape[1]
    D = kd // K
    Ru = u.shape[0]
    M = np.vstack([m[None], m[None] + z * d[None] + y @ v])
    ME = M / E
    q = (M * ME).reshape(-1, K, D).sum(axis=2)                                          # [J1, K]
    P = jc.grams(E, u, K)                                                               # [K, Ru, Ru]
    G = np.einsum("rcd,jcd->crj", u.reshape(Ru, K, D), ME.reshape(-1, K, D))            # [K, Ru, J1]
    lin, quad = F @ ME.T, N @ q.T
    a = F @ (u / E).T
    h = np.einsum("tc,crj->trj", N, G)
    L = np.eye(Ru)[None] + np.einsum("tc,cij->tij", N, P)
    s = np.zeros_like(lin)
    for t in range(T):
        w = np.linalg.solve(np.linalg.cholesky(L[t]), a[t][:, None] - h[t])
        s[t] = (lin[t] - quad[t] / 2 + (w * w).sum(axis=0) / 2) / N[t].sum()
    return (s[:, 1:] - s[:, :1]).T


def gate_integrated(shape, ref):
    T, J, K, D, Ry, Ru = shape
    terms = np.maximum(np.abs(ref["lin"]), np.maximum(np.abs(ref["quad"]) / 2, np.abs(ref["quad2"]) / 2)) / ref["sum_N"][None]
    return 8.0 * (Ry + Ru + K * D) * EPS * float(ref["kappa"].max()) * float(terms.max())


def gate_linear(shape, mag):
    T, J, K, D, Ry, Ru = shape
    return 8.0 * (Ry + Ru + K * D) * EPS * float(np.max(mag))


_CASES = {}


def inputs(T, J, K, D, Ry, Ru):
    """The shared, cached inputs of a shape in ROW orientation (score_trials's) with both restated score matrices.  Read-only."""
    key = (T, J, K, D, Ry, Ru)
    if key in _CASES:
        return _CASES[key]
    c = jc.corpus(T, K, D, Ry, 1000 * T + 10 * K + Ru, sessions=1)
    rng = np.random.default_rng(7 * T + J)
    kd = K * D
    u = rng.normal(0.0, 0.3, (Ru, kd))
    y = rng.standard_normal((J, Ry))
    z = 0.1 * rng.standard_normal((J, kd))
    d = rng.uniform(0.1, 0.5, kd)
    x = 0.3 * rng.standard_normal((T, Ru))
    out = dict(F=c["F"], N=c["N"], m=c["m"], E=c["E"], v=c["v_true"], u=u, y=y, z=z, d=d, x=x)
    out["ref"] = kscore_m(out["F"].T, out["N"].T, out["m"], out["E"], d, out["v"].T, u.T, z.T, y.T)
    out["linear"], out["linear_mag"] = linear_m(out["F"], out["N"], out["m"], out["E"], d, out["v"], u, z, y, x)
    for a in list(out.values()) + list(out["ref"].values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _CASES[key] = out
    return out


def args(c, **over):
    """score_trials's positional arguments (F, N, m, E, d, v, u, z, y) of a case."""
    a = dict(c, **over)
    return a["F"], a["N"], a["m"], a["E"], a["d"], a["v"], a["u"], a["z"], a["y"]


def score_integrated(trn, tst, m, E, v, u, d):
    """The chain of jfa.score_integrated restated: the enrolment factors of sc_score_dot_product.m, then kscore_famous_19.m.
    -> (scores [n_enrolment, n_test], the transliteration's dict for the gate)."""
    (tF, tN), (sF, sN) = trn, tst
    ny = v.shape[0]
    vu = np.vstack([v, u])
    tid = np.arange(tN.shape[0])
    yx = jc.estimate_y_and_v(tF, tN, None, m, E, d, vu, 0, 0, 0, 0, tid)
    tz = jc.estimate_z_and_d(tF, tN, None, m, E, d, vu, 0, 0, yx, 0, tid)
    ref = kscore_m(sF.T, sN.T, m, E, d, v.T, u.T, tz.T, yx[:, :ny].T)
    return ref["scores"], ref
