"""Score normalisation restated in float64 numpy, written from the definitions (include/pygmm_hip.h, "Score normalisation"), for
tests/test_scorenorm_cpu.py and tests/test_gpu_scorenorm.py.

``restate`` gathers per trial: no products, no selection matrices.  ``as2_gemm`` is a second, differently written statement of
as2 -- ``np.partition`` for the selection, the four shifted products for the moments -- which is the form the device computes.
The named mutants (``MUTANTS``) are wrong on purpose: the CPU suite shows that the GPU tests' own inputs tell each of them from
the restatement by at least 20 gates.

The gate of a parity case (derived, not tuned): a moment pair is a C-term sum and a C-term sum of squares taken in another order
than the restatement's, about a shift that lies rho sigma from the values; the variance carries a relative error of
C eps (1 + rho^2), the division by sigma spreads it over a score that lies q sigma from the mean:
    g = 8 C eps (1 + rho^2) (1 + q),   eps = 2^-52
    rho = the largest |x - shift| / sigma over the moment sets used (shift: the set's first value in index order for the per-row
          and per-column moments, the full row's / column's mean for as2's products)
    q   = the largest |s - mu| / sigma over the trials."""
import functools
import math

import numpy as np

EPS = 2.0 ** -52
MODES = ("z", "t", "zt", "s", "as1", "as2")
# J and T from the GEMM's tile (64) and reduction (16) edges, every value once on either side
SHAPES = ((1, 65), (15, 16), (16, 17), (17, 63), (63, 64), (64, 1), (65, 15))
COHORTS = (37, 257)
TOP_N = {37: 10, 257: 40}
OFFSETS = (0.0, 300.0)                         # in units of the cohort scores' sigma (1)
RHO_MAX, Q_MAX = 16.0, 32.0                    # stated ceilings of the gate's two ratios on these inputs (a top-N set is narrow: q reaches 24)
PARITY_CASES = [(J, T, C, off) for (J, T) in SHAPES for C in COHORTS for off in OFFSETS]


def top_idx(row, n, ties="low", largest=True):
    """Indices, ascending, of the n largest values of ``row``: ties to the lower index, -0.0 as +0.0."""
    r = np.asarray(row, dtype=np.float64) + 0.0
    pos = np.arange(r.size)
    order = np.lexsort((pos if ties == "low" else -pos, -r if largest else r))
    return np.sort(order[:min(n, r.size)])


def moments(v, ddof=0):
    """(mu, sigma, degenerate) of a moment set; a constant set has variance 0 exactly."""
    v = np.asarray(v, dtype=np.float64)
    if v.size - ddof < 1 or v.max() == v.min():
        return float(v[0]) + 0.0, 0.0, True
    mu = float(v.mean())
    var = float(((v - mu) ** 2).sum() / (v.size - ddof))
    bad = not (var > 0.0 and np.isfinite(var))
    return mu, (0.0 if bad else float(np.sqrt(var))), bad


def moments_shifted(v):
    """(mu, sigma, degenerate) of a moment set by the textbook shifted two-pass form with exactly rounded sums (math.fsum): the
    deviations are taken from the set's first value.  For the selection test's rows: where the spread lies far below the magnitude
    (values that differ in their last mantissa bits: |mu| eps / sigma reaches 1) the mean-relative form of ``moments`` loses every
    digit of sigma -- the reference's error, not the kernel's."""
    v = np.asarray(v, dtype=np.float64) + 0.0
    d = v - v[0]
    if not d.any():
        return float(v[0]), 0.0, True
    sd = math.fsum(d) / v.size
    with np.errstate(all="ignore"):
        sq = (d - sd) ** 2
    var = math.fsum(sq) / v.size if np.isfinite(sq).all() else float("inf")
    bad = not (var > 0.0 and np.isfinite(var))
    return float(v[0] + sd), (0.0 if bad else math.sqrt(var)), bad


class _Track:
    """The gate's ratios as the restatement meets them."""

    def __init__(self):
        self.rho = self.q = 0.0

    def pair(self, values, shift, sigma):
        if sigma > 0:
            self.rho = max(self.rho, float(np.abs(np.asarray(values) - shift).max()) / sigma)

    def trial(self, s, mu, sigma):
        if sigma > 0:
            self.q = max(self.q, abs(s - mu) / sigma)


def _side(M, n, tr, ddof, **sel):
    """Per row of M: the selection, its moments."""
    out = []
    for row in M:
        idx = np.arange(row.size) if n is None else top_idx(row, n, **sel)
        mu, sg, bad = moments(row[idx], ddof)
        if tr is not None:
            tr.pair(row[idx], row[idx[0]], sg)
        out.append((idx, mu, sg, bad))
    return out


def restate(mode, S, Ez=None, Tt=None, Zt=None, top_n=None, ddof=0, ties="low", largest=True, swap=True, zt_order="zt"):
    """-> dict(out [J, T], degenerate_enrol, degenerate_test, rho, q).  The keyword arguments past top_n are the mutants' handles."""
    S = np.asarray(S, dtype=np.float64)
    J, T = S.shape
    tr = _Track()
    sel = dict(ties=ties, largest=largest)
    out = np.zeros((J, T))
    n = top_n if mode in ("as1", "as2") else None
    if mode == "zt" and zt_order == "tz":      # the mutant: t-norm first, the enrolment cohort t-normalised by Zt's columns
        a = restate("t", S, Tt=Tt, ddof=ddof)
        b = restate("t", Ez, Tt=Zt, ddof=ddof)
        c = restate("z", a["out"], Ez=b["out"], ddof=ddof)
        return dict(c, rho=max(a["rho"], b["rho"], c["rho"]), q=max(a["q"], b["q"], c["q"]))
    if mode == "zt":
        zc = _side(Zt, None, tr, ddof)
        Tn = np.zeros_like(Tt)
        for c, (_, mu, sg, bad) in enumerate(zc):
            for t in range(T):
                if not bad:
                    Tn[c, t] = (Tt[c, t] - mu) / sg
                    tr.trial(Tt[c, t], mu, sg)
        Tt = Tn
    own = None if mode == "as2" and swap else tr       # (as2 takes no moments over a side's own selection: those sets are not in rho)
    rows = _side(Ez, n, own, ddof, **sel) if mode != "t" else None
    cols = _side(Tt.T, n, own, ddof, **sel) if mode != "z" else None
    de = sum(r[3] for r in rows) if rows else 0
    dt = sum(c[3] for c in cols) if cols else 0
    if mode == "zt":
        dt += sum(c[3] for c in zc)
    if mode == "as2" and swap:
        de = dt = 0
        full_r = [float(r.mean()) for r in Ez]
        full_c = [float(c.mean()) for c in Tt.T]
    for j in range(J):
        for t in range(T):
            s = S[j, t]
            if mode == "as2" and swap:
                ve, vt = Ez[j, cols[t][0]], Tt[rows[j][0], t]
                me, se, be = moments(ve, ddof)
                mt, st, bt = moments(vt, ddof)
                tr.pair(ve, full_r[j], se)
                tr.pair(vt, full_c[t], st)
                de, dt = de + be, dt + bt
            else:
                _, me, se, be = rows[j] if rows else (0, 0.0, 1.0, False)
                _, mt, st, bt = cols[t] if cols else (0, 0.0, 1.0, False)
            if be or bt:
                continue
            if mode == "z":
                out[j, t] = (s - me) / se
                tr.trial(s, me, se)
            elif mode == "t":
                out[j, t] = (s - mt) / st
                tr.trial(s, mt, st)
            elif mode == "zt":
                z = (s - me) / se
                out[j, t] = (z - mt) / st
                tr.trial(s, me, se)
                tr.trial(z, mt, st)
            else:
                out[j, t] = 0.5 * ((s - me) / se + (s - mt) / st)
                tr.trial(s, me, se)
                tr.trial(s, mt, st)
    return dict(out=out, degenerate_enrol=int(de), degenerate_test=int(dt), rho=tr.rho, q=tr.q)


def select_partition(M, n):
    """The 0/1 selection rows of M [rows, C] by np.partition: everything above the n-th largest value, then the first of its equals."""
    M = np.asarray(M, dtype=np.float64) + 0.0
    C = M.shape[1]
    n = min(n, C)
    sel = np.zeros_like(M)
    for r, row in enumerate(M):
        thr = np.partition(row, C - n)[C - n]
        above = row > thr
        equal = np.flatnonzero(row == thr)[:n - int(above.sum())]
        sel[r, above] = 1.0
        sel[r, equal] = 1.0
    return sel


def as2_gemm(S, Ez, Tt, top_n, shift=True):
    """as2 in the device's form: the four products over 0/1 selections, the operands shifted by the full row's / column's mean
    (``shift=False``: the mutant).  No degenerate pairs handled: the parity inputs have none."""
    N = float(min(top_n, Ez.shape[1]))
    SelE, SelT = select_partition(Ez, top_n), select_partition(Tt.T, top_n)
    mr = Ez.mean(axis=1, keepdims=True) if shift else np.zeros((Ez.shape[0], 1))
    mc = Tt.mean(axis=0, keepdims=True) if shift else np.zeros((1, Tt.shape[1]))
    Es, Ts = Ez - mr, Tt - mc
    me, mt = Es @ SelT.T / N, SelE @ Ts / N
    ve, vt = (Es * Es) @ SelT.T / N - me * me, SelE @ (Ts * Ts) / N - mt * mt
    return 0.5 * ((S - (mr + me)) / np.sqrt(ve) + (S - (mc + mt)) / np.sqrt(vt))


MUTANTS = {                                    # name -> (the modes it shows in, restate's keyword arguments)
    "ddof1": (MODES, dict(ddof=1)),
    "ties_high": (("as2",), dict(ties="high")),
    "smallest": (("as1", "as2"), dict(largest=False)),
    "as2_unswapped": (("as2",), dict(swap=False)),
    "zt_order": (("zt",), dict(zt_order="tz")),
}


def gate(C, rho, q):
    return 8.0 * C * EPS * (1.0 + rho * rho) * (1.0 + q)


@functools.lru_cache(maxsize=None)
def inputs(J, T, C, offset, seed=None):
    """Scores of a run with one cohort of C members on both sides: impostor scores N(0, 1), every 7th trial a target at +3, the
    cohort matrices N(0, 1) with a per-member bias of N(0, 0.3) -- all moved by ``offset``.  In every row of Ez and every column
    of Tt the values of rank N and N + 1 are made EQUAL (N = TOP_N[C]): a tie straddles the N-th place, so that the tie rule
    shows in every as2 trial.  Read-only."""
    rng = np.random.default_rng(1000 * J + 10 * T + C + int(offset) if seed is None else seed)
    n = TOP_N[C]
    S = rng.standard_normal((J, T)) + 3.0 * (np.arange(J * T).reshape(J, T) % 7 == 0)
    bias = 0.3 * rng.standard_normal(C)
    Ez = rng.standard_normal((J, C)) + bias
    Tt = rng.standard_normal((C, T)) + bias[:, None]
    Zt = rng.standard_normal((C, C)) + bias
    for M in (Ez, Tt.T):
        for row in M:
            order = np.argsort(-row, kind="stable")
            row[order[n]] = row[order[n - 1]]
    out = dict(S=S + offset, Ez=Ez + offset, Tt=Tt + offset, Zt=Zt + offset, top_n=n)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(J, T, C, offset, mode):
    """The restatement of a parity case, computed once."""
    c = inputs(J, T, C, offset)
    return restate(mode, c["S"], c["Ez"], c["Tt"], c["Zt"], c["top_n"])


# ---- rows for the selection tests ----

def selection_rows(C, seed=0):
    """[rows, C] of the kinds the selection has to get right, and their names."""
    rng = np.random.default_rng(seed + C)
    one = np.float64(1.0).view(np.uint64)
    rows = {"mixed": rng.standard_normal(C), "negative": -np.abs(rng.standard_normal(C)) - 0.5,
            "denormal": rng.integers(-9, 10, C) * 5e-324, "quantised": rng.integers(0, 6, C).astype(np.float64),
            "constant": np.full(C, 0.75), "zeros": np.where(rng.random(C) < 0.5, -0.0, 0.0),
            "zeros_and_ones": np.where(rng.random(C) < 0.2, rng.integers(-1, 2, C) + 0.0, np.where(rng.random(C) < 0.4, -0.0, 0.0)),
            "wide": rng.standard_normal(C) * 10.0 ** rng.integers(-300, 300, C)}
    for b in range(8):                         # values that differ in the lowest two bits of byte b of the key only
        rows["byte%d" % b] = (one ^ (rng.integers(0, 4, C).astype(np.uint64) << np.uint64(8 * b))).view(np.float64)
    return list(rows), np.ascontiguousarray(np.vstack(list(rows.values())))
