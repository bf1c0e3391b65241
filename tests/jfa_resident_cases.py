"""What the tests of the resident JFA route (csrc/jfa_stats.hip, jfa.Stats / jfa.centred) share: the centring cases, the numpy
restatement of the grouping and centring in any float type, and its gate.

For labels ids [n] below n_labels, N_j (x) w the row of K counts expanded over D:
  groups = speakers:  N_g = sum_{j in g} N_j,   Fc_g = sum_{j in g} (F_j - N_j (x) (x_j u)) - N_g (x) (m + z_g .* d + y_g v)
  groups = sessions:  Fc_j = F_j - N_j (x) (m + z_s .* d + y_s v + x_j u),  s = ids[j]
The gate, per element, derived and not measured:  |Fc - Fc*| <= 2 (n_g + Ry + Ru + 8) eps S,  S the same formula with every term
replaced by its absolute value, n_g the group's session count (1 for sessions), Ry / Ru counted where the term is present,
eps = 2^-52: the worst-case bound of a sum of that many rounded terms in any order, doubled."""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfa_cases as jc  # noqa: E402

EPS = jc.EPS
# (speakers, K, D, Ry, Ru, sessions)
CENTRING = ((9, 5, 39, 17, 5, 7), (12, 17, 13, 65, 16, 3), (4, 3, 3, 2, 2, 1))
TERMS = tuple(itertools.product((False, True), repeat=3))          # (z d, y v, x u) present?

_CASES = {}


def case(speakers, K, D, Ry, Ru, sessions):
    """A corpus of `speakers` x `sessions` sessions with shuffled labels, one label gap (label 2 does not occur), one speaker with
    a single session, one session whose N (and F) is all zero; factors and loadings for every optional term.  Cached, read-only."""
    key = (speakers, K, D, Ry, Ru, sessions)
    if key in _CASES:
        return _CASES[key]
    c = jc.corpus(speakers, K, D, Ry, 7000 + 100 * speakers + K, sessions=sessions)
    rng = np.random.default_rng(31 * speakers + K)
    F, N, ids = np.array(c["F"]), np.array(c["N"]), np.array(c["spk_ids"])
    keep = np.ones(len(ids), dtype=bool)
    keep[np.flatnonzero(ids == 1)[1:]] = False                       # speaker 1 keeps one session
    F, N, ids = F[keep], N[keep], ids[keep]
    N[len(ids) // 2] = 0.0                                           # a session of no frames
    F[len(ids) // 2] = 0.0
    ids = np.where(ids >= 2, ids + 1, ids)                           # the gap
    perm = rng.permutation(len(ids))
    F, N, ids = np.ascontiguousarray(F[perm]), np.ascontiguousarray(N[perm]), ids[perm].astype(np.int64)
    n, kd, n_labels = len(ids), K * D, int(ids.max()) + 1
    out = dict(F=F, N=N, ids=ids, n_labels=n_labels, m=c["m"], E=c["E"], K=K, D=D, Ry=Ry, Ru=Ru,
               v=rng.normal(0.0, 0.3, (Ry, kd)), u=rng.normal(0.0, 0.3, (Ru, kd)), y=rng.standard_normal((n_labels, Ry)),
               x=0.3 * rng.standard_normal((n, Ru)), z=0.1 * rng.standard_normal((n_labels, kd)), d=rng.uniform(0.1, 0.5, kd))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _CASES[key] = out
    return out


def terms(c, zd, yv, xu):
    """The keyword arguments of jfa.centred / ``centre`` for a combination of present terms."""
    kw = {}
    if zd:
        kw.update(z=c["z"], d=c["d"])
    if yv:
        kw.update(y=c["y"], v=c["v"])
    if xu:
        kw.update(x=c["x"], u=c["u"])
    return kw


def centre(c, groups, dtype=np.float64, d=None, z=None, v=None, y=None, u=None, x=None):
    """The restatement in `dtype`.  -> (N_g [G, K] float64 by np.add.at in session order, Fc [G, K D], S [G, K D], n_g [G, 1])."""
    T = dtype
    F, N, ids, K = c["F"].astype(T), c["N"].astype(T), c["ids"], c["K"]
    n, kd = F.shape
    Nx = np.repeat(N, kd // K, axis=1)
    m = c["m"].astype(T)
    shift, shift_abs = np.tile(m, (c["n_labels"], 1)), np.tile(np.abs(m), (c["n_labels"], 1))
    if z is not None:
        shift = shift + z.astype(T) * d.astype(T)
        shift_abs = shift_abs + np.abs(z.astype(T) * d.astype(T))
    if y is not None:
        shift = shift + y.astype(T) @ v.astype(T)
        shift_abs = shift_abs + np.abs(y.astype(T)) @ np.abs(v.astype(T))
    sess, sess_abs = F, np.abs(F)
    if x is not None:
        sess = F - Nx * (x.astype(T) @ u.astype(T))
        sess_abs = sess_abs + Nx * (np.abs(x.astype(T)) @ np.abs(u.astype(T)))
    if groups == "sessions":
        return c["N"], sess - Nx * shift[ids], sess_abs + Nx * shift_abs[ids], np.ones((n, 1))
    present = np.unique(ids)
    pos = np.searchsorted(present, ids)
    G = len(present)
    Ng = np.zeros((G, K))
    np.add.at(Ng, pos, c["N"])
    Fs, Ss, Nxg = np.zeros((G, kd), dtype=T), np.zeros((G, kd), dtype=T), np.zeros((G, kd), dtype=T)
    np.add.at(Fs, pos, sess)
    np.add.at(Ss, pos, sess_abs)
    np.add.at(Nxg, pos, Nx)
    return Ng, Fs - Nxg * shift[present], Ss + Nxg * shift_abs[present], np.bincount(pos, minlength=G).reshape(-1, 1).astype(np.float64)


def gate(c, n_g, S, yv, xu):
    """[G, K D]: the bound on |Fc - Fc*|."""
    return 2.0 * (n_g + (c["Ry"] if yv else 0) + (c["Ru"] if xu else 0) + 8.0) * EPS * np.asarray(S, dtype=np.float64)


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the elements (0 where both vanish)."""
    diff = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(want, dtype=np.longdouble)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0.0, 0.0, diff / bound)
    return float(r.max())
