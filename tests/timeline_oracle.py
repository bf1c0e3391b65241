"""The timeline's definitions restated in numpy / plain Python float64 (include/pygmm_hip.h, "Who spoke when"): window counts,
in-order float64 window sums, emissions, the raw decision, the hold rule, the Viterbi recurrence with a switch penalty and a
minimum turn length -- every operation one float64 add or one compare, in the order the header states -- and a brute-force
path enumerator that maximises the same score under the same run-length constraint."""
import itertools

import numpy as np

NEG = float("-inf")


def windows(n, W, H):
    if n <= 0:
        return 0
    # (W < H: a window that would start at or behind frame n is not formed)
    return min(1 + -(-max(0, n - W) // H), -(-n // H))


def window_sums(fll, W, H):
    """fll [S, n] fp32 -> (sums [Nw, S] float64 added in frame order, counts [Nw] int32)."""
    fll = np.asarray(fll, dtype=np.float32)
    S, n = fll.shape
    Nw = windows(n, W, H)
    sums = np.zeros((Nw, S), dtype=np.float64)
    counts = np.zeros(Nw, dtype=np.int32)
    for j in range(Nw):
        a, b = j * H, min(j * H + W, n)
        counts[j] = b - a
        if b > a:
            # np.add.accumulate is a sequential accumulate: ((x0 + x1) + x2) + ..., unlike np.sum's pairwise tree
            sums[j] = np.add.accumulate(fll[:, a:b].astype(np.float64), axis=1)[:, -1]
    return sums, counts


def emissions(sums, counts, bg=-1, threshold=0.0):
    """-> (e [Nw, S] float64 in COLUMN order, number of windows that held a NaN quotient)."""
    sums = np.asarray(sums, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = sums / np.asarray(counts, dtype=np.float64)[:, None]
        nan = np.isnan(q)
        bad = int(np.sum(nan.any(axis=1))) if len(q) else 0
        q = np.where(nan, NEG, q)
        if bg >= 0:
            q[:, bg] = q[:, bg] + np.float64(threshold)
            q[:, bg] = np.where(np.isnan(q[:, bg]), NEG, q[:, bg])
    return q, bad


def order(S, bg):
    """The states in priority order: the speaker columns ascending, the nobody state last."""
    return [s for s in range(S) if s != bg] + ([bg] if bg >= 0 else [])


def first_max(values, states):
    """The first maximum of values[s] over `states` in that order: replaced on `>` alone."""
    best = states[0]
    for s in states[1:]:
        if values[s] > values[best]:
            best = s
    return best


def raw(e, bg=-1):
    Nw, S = e.shape
    out = np.full(Nw, -1, dtype=np.int32)
    od = order(S, bg)
    for j in range(Nw):
        b = first_max(e[j], od)
        out[j] = -1 if (e[j][b] == NEG or b == bg) else b
    return out


def hold(r):
    shown = np.array(r, dtype=np.int32)
    for j in range(1, len(r)):
        if r[j] != -1 and r[j - 1] != -1 and r[j - 1] != r[j]:
            shown[j] = shown[j - 1]
    return shown


def viterbi(e, bg, beta, m):
    """-> (labels [Nw] int32, path score).  The recurrence of the header, states (s, k), k = 1 .. m; the states of one window
    are numpy vectors (elementwise float64 adds and compares: the operations of a loop over the states, bit for bit)."""
    e = np.asarray(e, dtype=np.float64)
    Nw, S = e.shape
    if Nw == 0:
        return np.zeros(0, dtype=np.int32), 0.0
    beta = np.float64(beta)
    od = np.array(order(S, bg))

    def first(v):                                    # np.argmax keeps the first maximum (no NaN inside the contract)
        return int(od[int(np.argmax(v[od]))])

    d = np.full((m + 1, S), NEG)                     # d[k][s], k = 1 .. m
    d[1] = e[0]
    stay = np.zeros((Nw, S), dtype=bool)
    ent = [0] * Nw
    for j in range(1, Nw):
        a = first(d[m])
        ent[j] = a
        enter = d[m][a] - beta
        nd = np.full((m + 1, S), NEG)
        if m == 1:
            st = d[1] >= enter
            nd[1] = e[j] + np.where(st, d[1], enter)
        else:
            st = d[m] >= d[m - 1]
            nd[m] = e[j] + np.where(st, d[m], d[m - 1])
            for k in range(2, m):
                nd[k] = e[j] + d[k - 1]
            nd[1] = e[j] + enter
        stay[j] = st
        d = nd
    bs, bk = first(d[m]), m
    for k in range(m - 1, 0, -1):
        s = first(d[k])
        if d[k][s] > d[bk][bs]:
            bs, bk = s, k
    score = float(d[bk][bs])
    labels = np.zeros(Nw, dtype=np.int32)
    s, k = bs, bk
    for j in range(Nw - 1, -1, -1):
        labels[j] = -1 if s == bg else s
        if j == 0:
            break
        if k == m:
            if not stay[j][s]:
                if m == 1:
                    s = ent[j]
                else:
                    k = m - 1
        elif k > 1:
            k -= 1
        else:
            s, k = ent[j], m
    return labels, score


def decide(sums, counts, bg=-1, threshold=0.0, mode=0, beta=0.0, m=1):
    """One recording: -> (labels, path score or NaN, windows with a NaN quotient)."""
    e, bad = emissions(sums, counts, bg, threshold)
    if mode == 0:
        return raw(e, bg), float("nan"), bad
    if mode == 1:
        return hold(raw(e, bg)), float("nan"), bad
    lab, score = viterbi(e, bg, beta, m)
    return lab, score, bad


def path_score(e, path, beta):
    """sum_j e_j(l_j) - beta * changes, added in window order (for the brute force: compared with a tolerance of rounding)."""
    total = 0.0
    for j, s in enumerate(path):
        total += float(e[j][s])
    return total - float(beta) * sum(1 for j in range(1, len(path)) if path[j] != path[j - 1])


def runs_ok(path, m):
    """Every run but the last holds at least m windows."""
    run = 1
    for j in range(1, len(path)):
        if path[j] != path[j - 1]:
            if run < m:
                return False
            run = 1
        else:
            run += 1
    return True


def brute_force(e, beta, m):
    """The best score over every state sequence that keeps the run-length constraint."""
    Nw, S = e.shape
    best = NEG
    for path in itertools.product(range(S), repeat=Nw):
        if runs_ok(path, m):
            best = max(best, path_score(e, path, beta))
    return best
