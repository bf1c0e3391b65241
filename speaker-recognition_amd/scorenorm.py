"""Score normalisation of a verification run on the device (csrc/score_norm.hip through ``sr_score_norm``), and the two numbers such
a run reports.

A score matrix ``S`` [J, T] -- J models against T test segments, from ``jfa.score_trials`` / ``score_integrated`` /
``score_dot_product`` or, through ``llr_matrix``, from ``ModelSet.score`` -- is normalised against impostor cohorts:

    ``enrol_cohort``  Ez [J, Cz]   the models against the Z-cohort (impostor segments)
    ``cohort_test``   Tt [Ct, T]   the T-cohort models against the test segments
    ``cohort_cohort`` Zt [Ct, Cz]  the T-cohort models against the Z-cohort (``zt`` only)

With mu / sigma the mean and the population standard deviation (ddof = 0), and "top-N" the N largest values of a row (ties to the
lower index, -0.0 taken as +0.0):

    ``z``    (S - mu(Ez[j, :])) / sigma(Ez[j, :])
    ``t``    (S - mu(Tt[:, t])) / sigma(Tt[:, t])
    ``zt``   S' = z-norm of S by Ez; Tt' = z-norm of Tt by Zt (row c of Tt by row c of Zt); out = t-norm of S' by Tt'
    ``s``    (z + t) / 2
    ``as1``  as ``s``, the moments over the top-N of Ez[j, :] and over the top-N of Tt[:, t]
    ``as2``  Cz = Ct: cohort member c is both a segment and a model.  I_t = the top-N of Tt[:, t], I_j = the top-N of Ez[j, :];
             ((S - mu(Ez[j, I_t])) / sigma(Ez[j, I_t]) + (S - mu(Tt[I_j, t])) / sigma(Tt[I_j, t])) / 2

A moment pair whose variance is not > 0 (a constant cohort row) is degenerate: every trial that needs it gets 0.0 exactly, and the
pairs are counted per side (``return_counts``).  No NaN is ever written.  Float64 throughout; there is no CPU path.

``eer`` and ``min_dcf`` are host numpy: one sort and cumulative sums."""
from __future__ import annotations

import ctypes as C

import numpy as np

MODES = ("z", "t", "zt", "s", "as1", "as2")


def _matrix(a, name, shape=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or (shape is not None and any(w is not None and w != g for w, g in zip(shape, a.shape))):
        want = "a 2-D array" if shape is None else "[%s]" % ", ".join("?" if w is None else str(w) for w in shape)
        raise ValueError("expected %s as %s, got shape %r" % (name, want, a.shape))
    return a


def normalise(S, mode, enrol_cohort=None, cohort_test=None, cohort_cohort=None, top_n=None, return_counts=False):
    """``S`` [J, T] normalised by ``mode`` (see the module text) in one device call -> [J, T] float64.  A matrix the mode does not
    read may be None or anything: it is not looked at.  ``top_n``: the adaptive modes' N (>= 2; N >= the cohort's size selects everything).
    ``return_counts``: -> (out, {"degenerate_enrol": n, "degenerate_test": n}), the degenerate moment pairs by side: rows of Ez and
    columns of Tt (for ``zt``: columns of Tt' plus rows of Zt) in every mode but ``as2``, where they are (model, segment) pairs."""
    from . import _lib
    if mode not in MODES:
        raise ValueError("mode is one of %s, got %r" % (", ".join(repr(m) for m in MODES), mode))
    S = _matrix(S, "S")
    J, T = S.shape
    Ez = _matrix(enrol_cohort, "enrol_cohort", (J, None)) if mode != "t" else None       # (a matrix the mode does not read is ignored)
    Tt = _matrix(cohort_test, "cohort_test", (None, T)) if mode != "z" else None
    Cz = Ez.shape[1] if Ez is not None else 0
    Ct = Tt.shape[0] if Tt is not None else 0
    Zt = _matrix(cohort_cohort, "cohort_cohort", (Ct, Cz)) if mode == "zt" else None
    if mode in ("as1", "as2") and top_n is None:
        raise ValueError("mode %r needs top_n, the number of cohort scores the moments are taken over" % (mode,))
    out = np.zeros((J, T))
    counts = (C.c_int64 * 2)()
    opt = lambda a: _lib.as_dp(a) if a is not None else None                        # noqa: E731
    _lib.check(_lib.lib().sr_score_norm(MODES.index(mode), J, T, Cz, Ct, int(top_n or 0), _lib.as_dp(S), opt(Ez), opt(Tt), opt(Zt),
                                        _lib.as_dp(out), counts), "sr_score_norm")
    return (out, {"degenerate_enrol": int(counts[0]), "degenerate_test": int(counts[1])}) if return_counts else out


def znorm(S, enrol_cohort, return_counts=False):
    return normalise(S, "z", enrol_cohort=enrol_cohort, return_counts=return_counts)


def tnorm(S, cohort_test, return_counts=False):
    return normalise(S, "t", cohort_test=cohort_test, return_counts=return_counts)


def ztnorm(S, enrol_cohort, cohort_test, cohort_cohort, return_counts=False):
    return normalise(S, "zt", enrol_cohort, cohort_test, cohort_cohort, return_counts=return_counts)


def snorm(S, enrol_cohort, cohort_test, return_counts=False):
    return normalise(S, "s", enrol_cohort, cohort_test, return_counts=return_counts)


def asnorm(S, enrol_cohort, cohort_test, top_n, variant=2, return_counts=False):
    """Adaptive S-norm.  ``variant`` 1: each side's moments over its own top-N cohort scores; 2: over the cohort members the OTHER
    side selects (one cohort on both sides)."""
    if variant not in (1, 2):
        raise ValueError("variant is 1 or 2, got %r" % (variant,))
    return normalise(S, "as%d" % variant, enrol_cohort, cohort_test, top_n=top_n, return_counts=return_counts)


def select_cohort(X, top_n):
    """The selection stage alone on ``X`` [rows, C]: -> (idx [rows, min(top_n, C)] int64, the indices of each row's top-N ascending;
    mu [rows]; sigma [rows]), the moments (ddof = 0) of the selected values.  sigma 0.0 marks a degenerate row."""
    from . import _lib
    X = _matrix(X, "X")
    rows, Cn = X.shape
    top_n = int(top_n)
    idx = np.zeros((rows, max(1, min(top_n, Cn))), dtype=np.int64)
    mu, sigma = np.zeros(rows), np.zeros(rows)
    _lib.check(_lib.lib().sr_score_norm_select(rows, Cn, top_n, _lib.as_dp(X), _lib.as_i64p(idx), _lib.as_dp(mu), _lib.as_dp(sigma)),
               "sr_score_norm_select")
    return idx, mu, sigma


def llr_matrix(sums, n_frames, background=-1):
    """The per-frame log-likelihood ratio matrix [speakers, utterances] of a GMM-UBM run: ``sums`` [U, S] as ``ModelSet.score`` returns
    them (utterances x models, one of the models the background), ``n_frames`` [U] the utterances' frame counts, ``background`` the
    background model's column.  out[s, u] = (sums[u, s] - sums[u, background]) / n_frames[u]; an utterance of no frames gives 0.0."""
    sums = _matrix(sums, "sums")
    n = np.asarray(n_frames, dtype=np.float64).reshape(-1)
    if n.shape[0] != sums.shape[0]:
        raise ValueError("expected one frame count per row of sums (%d), got %d" % (sums.shape[0], n.shape[0]))
    bg = range(sums.shape[1])[background]
    diff = np.delete(sums, bg, axis=1) - sums[:, bg:bg + 1]
    return np.ascontiguousarray(np.where(n[:, None] > 0, diff / np.where(n > 0, n, 1.0)[:, None], 0.0).T)


def _operating_points(scores, is_target):
    """(p_fa, p_miss) over the thresholds "accept a trial whose score is >= theta": one point above every score, then one per
    DISTINCT score, descending -- trials with equal scores are accepted together."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    tar = np.asarray(is_target).reshape(-1).astype(bool)
    if s.shape != tar.shape:
        raise ValueError("expected one label per score, got %d scores and %d labels" % (s.size, tar.size))
    if not np.all(np.isfinite(s)):
        raise ValueError("scores hold a non-finite value")
    n_tar, n_imp = int(tar.sum()), int((~tar).sum())
    if n_tar == 0 or n_imp == 0:
        raise ValueError("need at least one target and one impostor trial (got %d and %d)" % (n_tar, n_imp))
    order = np.argsort(-s, kind="stable")
    s, tar = s[order], tar[order]
    last = np.r_[s[1:] != s[:-1], True]
    p_fa = np.r_[0.0, np.cumsum(~tar)[last] / n_imp]
    p_miss = np.r_[1.0, 1.0 - np.cumsum(tar)[last] / n_tar]
    return p_fa, p_miss


def eer(scores, is_target):
    """The equal error rate.  Convention: a trial is accepted when its score is >= the threshold, so trials with EQUAL scores move
    together (one operating point per distinct score); where no operating point has P_fa = P_miss exactly, the EER is where the
    straight line between the two neighbouring points crosses P_fa = P_miss.

    Worked example, 4 targets 0.9 0.8 0.6 0.3 and 4 impostors 0.7 0.4 0.2 0.1: descending 0.9T 0.8T 0.7I 0.6T ...; (P_fa, P_miss)
    runs (0, 1) (0, .75) (0, .5) (.25, .5) (.25, .25): the last has both equal, EER = 0.25.  Perfect separation passes through
    (0, 0): EER 0; all impostors above all targets passes through (1, 1): EER 1."""
    p_fa, p_miss = _operating_points(scores, is_target)
    k = int(np.argmax(p_fa >= p_miss))         # (the last point is (1, 0): there is one)
    if p_fa[k] == p_miss[k]:
        return float(p_fa[k])
    a, b = p_miss[k - 1] - p_fa[k - 1], p_fa[k] - p_miss[k]
    return float(p_fa[k - 1] + a / (a + b) * (p_fa[k] - p_fa[k - 1]))


def min_dcf(scores, is_target, p_target=0.01, c_miss=1.0, c_fa=1.0):
    """The minimum of the normalised detection cost  (c_miss p_target P_miss + c_fa (1 - p_target) P_fa) / min(c_miss p_target,
    c_fa (1 - p_target))  over the operating points of ``eer`` (ties move together; the point above every score, which rejects
    everything and costs 1 after normalisation when c_miss p_target is the smaller, is among them).

    In ``eer``'s example with the defaults the minimum is at (0, .5): 0.5."""
    if not (0.0 < p_target < 1.0) or not (c_miss > 0.0 and c_fa > 0.0):
        raise ValueError("need 0 < p_target < 1 and positive costs")
    p_fa, p_miss = _operating_points(scores, is_target)
    dcf = c_miss * p_target * p_miss + c_fa * (1.0 - p_target) * p_fa
    return float(dcf.min() / min(c_miss * p_target, c_fa * (1.0 - p_target)))
