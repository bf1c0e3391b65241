"""A numpy restatement of the diarisation of unknown speakers (include/pygmm_hip.h "Who spoke when, nobody enrolled"), line by
line: base segments, statistics summed in frame order, the covariance and its log-determinant (LAPACK's Cholesky), delta-BIC, the
change detector's scores and peak rule, the agglomeration with its argmin, tie order, stop rule, log and labels, and the matrix
mode's Lance-Williams updates.  The agglomeration also reports, per step, what the GPU tests need to know whether a comparison of
merge sequences is fair: the best and the second-best distance, and the error bound of the distances of that step."""
import numpy as np

EPS = np.finfo(np.float64).eps


def segments(n, L):
    if n <= 0 or L < 1:
        return 0
    return max(n // L, 1)


def stat_len(D):
    return 1 + D + D * (D + 1) // 2


def tri_index(D):
    r, c = np.tril_indices(D)                  # the lower triangle by rows
    return r, c


def stats_of(x, D=None):
    """N, s, Q of the frames x [n, D] (fp32 values): every entry summed in frame order, one product and one add per frame."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    D = x.shape[1] if D is None else D
    r, c = tri_index(D)
    terms = np.concatenate([x, x[:, r] * x[:, c]], axis=1)
    acc = np.add.accumulate(np.concatenate([np.zeros((1, terms.shape[1])), terms], axis=0), axis=0)[-1]    # sequential: 0 + t0 + t1 ...
    return np.concatenate([[float(len(x))], acc])


def seg_stats(X, L):
    X = np.asarray(X, dtype=np.float32)
    n, D = X.shape
    ns = segments(n, L)
    out = np.zeros((ns, stat_len(D)))
    for i in range(ns):
        out[i] = stats_of(X[i * L:(n if i == ns - 1 else (i + 1) * L)], D)
    return out


def sum_in_order(stats):
    """The sum of statistics [k, P] in index order, element by element."""
    acc = np.zeros(stats.shape[1])
    for s in stats:
        acc = acc + s
    return acc


def cov(stat, D, ridge):
    """Sigma = (Q - s s^T / N) / N + ridge I for one statistic or a stack [K, P] -> [K, D, D]."""
    stat = np.atleast_2d(stat)
    N = stat[:, 0][:, None, None]
    s = stat[:, 1:1 + D]
    r, c = tri_index(D)
    Q = np.zeros((len(stat), D, D))
    Q[:, r, c] = stat[:, 1 + D:]
    Q[:, c, r] = stat[:, 1 + D:]
    return (Q - s[:, :, None] * s[:, None, :] / N) / N + ridge * np.eye(D)


def logdet(stat, D, ridge):
    """-> (ld [K], ok [K], kappa [K]): 2 sum log L_rr of LAPACK's lower Cholesky factor; not ok when a pivot is not positive or not
    finite; kappa the covariance's condition number from eigvalsh (inf when not ok)."""
    S = cov(stat, D, ridge)
    K = len(S)
    ld, ok, kappa = np.full(K, np.nan), np.zeros(K, bool), np.full(K, np.inf)
    good = np.isfinite(S).all(axis=(1, 2))
    idx = np.flatnonzero(good)
    try:
        Lf = np.linalg.cholesky(S[idx])
    except np.linalg.LinAlgError:              # one of the stack failed: one by one
        keep, facts = [], []
        for k in idx:
            try:
                facts.append(np.linalg.cholesky(S[k]))
                keep.append(k)
            except np.linalg.LinAlgError:
                pass
        idx, Lf = np.array(keep, np.int64), np.array(facts).reshape(len(keep), D, D)
    d = np.diagonal(Lf, axis1=1, axis2=2)
    fine = (d > 0).all(axis=1) & np.isfinite(d).all(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        ld[idx[fine]] = (2.0 * np.sum(np.log(d), axis=1))[fine]
    ok[idx[fine]] = True
    if ok.any():
        w = np.linalg.eigvalsh(S[ok])
        kappa[ok] = np.where(w[:, 0] > 0, w[:, -1] / np.where(w[:, 0] > 0, w[:, 0], 1.0), np.inf)
    return ld, ok, kappa


def penalty(D, lam):
    return lam * 0.5 * (D + D * (D + 1) // 2)


def bound(N, D, kappa):
    """Cholesky's backward error carried through the log-determinant of a cluster of N frames, with a margin of 8."""
    return 8.0 * N * D * D * EPS * kappa


def dbic_rows(sa, ld_a, ok_a, ka, SB, ld_b, ok_b, kb, D, lam, ridge):
    """delta-BIC of the cluster sa against every cluster of the stack SB -> (d [K] with +inf where a factorisation failed, bound [K])."""
    merged = sa[None, :] + SB
    ld_ab, ok_ab, k_ab = logdet(merged, D, ridge)
    Na, Nb = sa[0], SB[:, 0]
    with np.errstate(invalid="ignore"):
        d = 0.5 * ((Na + Nb) * ld_ab - Na * ld_a - Nb * ld_b) - penalty(D, lam) * np.log(Na + Nb)
    good = ok_ab & ok_b & bool(ok_a)
    d = np.where(good, d, np.inf)
    kap = np.maximum(np.maximum(k_ab, kb), ka)
    return d, np.where(good, bound(Na + Nb, D, kap), 0.0)


def bic_matrix(stats, D, lam=1.0, ridge=1e-3):
    """-> (dBIC [n, n] symmetric with 0 on the diagonal, bound [n, n], ld [n] (NaN where failed), failures)."""
    n = len(stats)
    ld, ok, kap = logdet(stats, D, ridge) if n else (np.zeros(0), np.zeros(0, bool), np.zeros(0))
    out, bnd = np.zeros((n, n)), np.zeros((n, n))
    for i in range(n - 1):
        d, b = dbic_rows(stats[i], ld[i], ok[i], kap[i], stats[i + 1:], ld[i + 1:], ok[i + 1:], kap[i + 1:], D, lam, ridge)
        out[i, i + 1:] = out[i + 1:, i] = d
        bnd[i, i + 1:] = bnd[i + 1:, i] = b
    return out, bnd, np.where(ok, ld, np.nan), int((~ok).sum())


def change_scores(seg, D, m, lam=1.0, ridge=1e-3):
    """c[b] for b = 1 .. n_seg - 1 (returned at index b - 1) and their bounds."""
    ns = len(seg)
    c, bnd = np.zeros(max(ns - 1, 0)), np.zeros(max(ns - 1, 0))
    for b in range(1, ns):
        a = sum_in_order(seg[max(0, b - m):b])
        r = sum_in_order(seg[b:min(ns, b + m)])
        la, oa, ka = logdet(a, D, ridge)
        lb, ob, kb = logdet(r, D, ridge)
        d, bd = dbic_rows(a, la[0], oa[0], ka[0], r[None, :], lb, ob, kb, D, lam, ridge)
        c[b - 1], bnd[b - 1] = d[0], bd[0]
    return c, bnd


def peaks(c, m):
    """kept[b - 1] for the scores c[b - 1]: c[b] > 0, c[b] >= c[b'] for every b' with |b - b'| < m, no earlier b' in that range
    with the same value."""
    nb = len(c)
    kept = np.zeros(nb, bool)
    for b in range(nb):
        v = c[b]
        keep = v > 0
        for k in range(max(0, b - (m - 1)), min(nb - 1, b + (m - 1)) + 1):
            if k == b:
                continue
            if (k < b and not v > c[k]) or (k > b and not v >= c[k]):
                keep = False
        kept[b] = keep
    return kept


def init_clusters(seg, kept):
    """-> (init_off [n_init + 1] in base-segment indices, statistics [n_init, P])."""
    ns = len(seg)
    if ns == 0:
        return np.zeros(1, np.int64), np.zeros((0, seg.shape[1] if seg.ndim == 2 else 1))
    off = [0] + [b for b in range(1, ns) if kept[b - 1]] + [ns]
    return np.array(off, np.int64), np.array([sum_in_order(seg[a:b]) for a, b in zip(off, off[1:])])


def labels_of(n, merge_i, merge_j):
    root = list(range(n))
    for i, j in zip(merge_i, merge_j):
        root = [int(i) if r == j else r for r in root]
    number, out = {}, []
    for r in root:
        number.setdefault(r, len(number))
        out.append(number[r])
    return np.array(out, np.int32)


def _goes(live, d, threshold, k_min, k_max):
    return d != np.inf and ((k_max > 0 and live > k_max) or (live > k_min and d < threshold))


def _first_min(dist, alive):
    """The live pair (i < j) of smallest distance, first in row-major order; also the second smallest value."""
    n = len(dist)
    mask = np.triu(np.outer(alive, alive), 1).astype(bool)
    if not mask.any():
        return None
    flat = np.where(mask, dist, np.inf).reshape(-1)
    best = int(np.argmin(flat))                # the first occurrence: row-major
    if not mask.reshape(-1)[best]:             # every live pair is +inf
        best = int(np.flatnonzero(mask.reshape(-1))[0])
    rest = np.delete(flat, best)
    return best // n, best % n, float(flat[best]), float(rest.min()) if len(rest) else np.inf


def agglomerate(stats, D, lam=1.0, ridge=1e-3, threshold=0.0, k_min=1, k_max=0):
    """-> dict(merge_i, merge_j, merge_d, labels, n_clusters, failed, steps): ``steps`` holds per decision (the stopping one
    included) (best, second, bound, own): bound the largest error bound among the distances alive at that step -- what a comparison
    of two of them is judged by --, own the bound of the chosen pair's distance, 8 (N_i + N_j) D^2 eps kappa with kappa the largest
    condition number of that pair's three covariances -- what its merged distance is held to."""
    stats = np.array(stats, dtype=np.float64)
    n = len(stats)
    dist, bnd, ld, failed = bic_matrix(stats, D, lam, ridge)
    ok = ~np.isnan(ld)
    kap = logdet(stats, D, ridge)[2] if n else np.zeros(0)
    alive = np.ones(n, bool)
    mi, mj, md, steps = [], [], [], []
    live = n
    while True:
        pick = _first_min(dist, alive)
        if pick is None:
            break
        i, j, d, second = pick
        mask = np.triu(np.outer(alive, alive), 1).astype(bool)
        steps.append((d, second, float(bnd[mask].max()), float(bnd[i, j])))
        if not _goes(live, d, threshold, k_min, k_max):
            break
        mi.append(i), mj.append(j), md.append(d)
        stats[i] = stats[i] + stats[j]
        alive[j] = False
        live -= 1
        l1, o1, k1 = logdet(stats[i], D, ridge)
        ld[i], ok[i], kap[i] = l1[0], o1[0], k1[0]
        ks = np.flatnonzero(alive & (np.arange(n) != i))
        if len(ks):
            dk, bk = dbic_rows(stats[i], ld[i], ok[i], kap[i], stats[ks], ld[ks], ok[ks], kap[ks], D, lam, ridge)
            dist[i, ks] = dist[ks, i] = dk
            bnd[i, ks] = bnd[ks, i] = bk
    lab = labels_of(n, mi, mj)
    return dict(merge_i=np.array(mi, np.int32), merge_j=np.array(mj, np.int32), merge_d=np.array(md), labels=lab,
                n_clusters=len(set(lab.tolist())), failed=failed, steps=steps)


def cluster(X, L, change="bic", m=2, lam=1.0, ridge=1e-3, threshold=0.0, k_min=1, k_max=0):
    """The whole chain on one recording's frames."""
    X = np.asarray(X, dtype=np.float32)
    D = X.shape[1]
    seg = seg_stats(X, L)
    if change == "bic":
        c, cb = change_scores(seg, D, m, lam, ridge)
        kept = peaks(c, m)
    else:
        c, cb = np.zeros(0), np.zeros(0)
        kept = np.ones(max(len(seg) - 1, 0), bool)
    init_off, cl = init_clusters(seg, kept)
    out = agglomerate(cl, D, lam, ridge, threshold, k_min, k_max)
    out.update(init_off=init_off, change=c, change_bound=cb, kept=kept, n_seg=len(seg))
    return out


def fair(steps, threshold, factor=4.0):
    """The condition under which two implementations must take the same steps: at every decision the best distance is further than
    ``factor`` bounds from the second best and from the threshold."""
    for d, second, b, _ in steps:
        if d == np.inf:
            continue
        if not (second - d > factor * b):
            return False
        if np.isfinite(threshold) and not (abs(d - threshold) > factor * b):
            return False
    return True


def ahc(dist, linkage=0, threshold=0.0, k_min=1, k_max=0):
    """The matrix mode: linkage 0 average -- (c_i d_ik + c_j d_jk) / (c_i + c_j) --, 1 complete, 2 single."""
    dist = np.array(dist, dtype=np.float64)
    n = len(dist)
    alive = np.ones(n, bool)
    cnt = np.ones(n)
    mi, mj, md = [], [], []
    live = n
    while True:
        pick = _first_min(dist, alive)
        if pick is None:
            break
        i, j, d, _ = pick
        if not _goes(live, d, threshold, k_min, k_max):
            break
        mi.append(i), mj.append(j), md.append(d)
        ks = np.flatnonzero(alive & (np.arange(n) != i) & (np.arange(n) != j))
        dik, djk = dist[i, ks], dist[j, ks]
        if linkage == 0:
            new = (cnt[i] * dik + cnt[j] * djk) / (cnt[i] + cnt[j])
        elif linkage == 1:
            new = np.where(dik >= djk, dik, djk)
        else:
            new = np.where(dik <= djk, dik, djk)
        dist[i, ks] = dist[ks, i] = new
        cnt[i] += cnt[j]
        alive[j] = False
        live -= 1
    lab = labels_of(n, mi, mj)
    return dict(merge_i=np.array(mi, np.int32), merge_j=np.array(mj, np.int32), merge_d=np.array(md), labels=lab,
                n_clusters=len(set(lab.tolist())))


def cut(n, merge_i, merge_j, merge_d, threshold=0.0, k_min=1, k_max=0):
    live, t = n, 0
    while t < len(merge_d) and _goes(live, merge_d[t], threshold, k_min, k_max):
        live -= 1
        t += 1
    return labels_of(n, merge_i[:t], merge_j[:t]), t
