"""The batched Baum-Welch statistics (csrc/bw_stats.hip) restated in float64 numpy, shared by tests/test_bw_cpu.py and
tests/test_gpu_bw_stats.py: the log-domain form the device computes (``stats``), the same by plain loops (``stats_loops``), the
linear-domain formula of the reference's gaussian_posteriors.m / collect_suf_stats.m (``stats_linear``), the gates, and the
makers of models and sessions.  A model here is (weights [K], means [K, D], variances [K, D]) -- VARIANCES, as the reference's
JFA tables hold them."""
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fixture_ubm():
    g = np.load(os.path.join(ROOT, "tests", "golden", "jfa_ubm.npz"))
    return g["weights"], g["means"], g["variances"]


def make_ubm(K, D, seed, shift=0.0):
    """K overlapping diagonal Gaussians in D dimensions around `shift`: the means' spread shrinks with sqrt(D), so that the
    posteriors stay soft at every D (in 39 dimensions means 2 sigma apart per dimension would make them one-hot and the
    statistics blind to the densities' last digits)."""
    rng = np.random.RandomState(seed)
    w = rng.uniform(0.5, 1.5, K)
    w /= w.sum()
    mu = rng.normal(0.0, 2.0 / np.sqrt(D), (K, D)) + shift
    var = rng.uniform(0.3, 1.5, (K, D)) ** 2
    return w, mu, var


def draw(ubm, T, seed):
    """T frames drawn from the model, fp32-representable (what the device sees), as float64."""
    w, mu, var = ubm
    rng = np.random.RandomState(seed)
    k = rng.choice(len(w), size=T, p=w / w.sum())
    x = mu[k] + rng.normal(size=(T, mu.shape[1])) * np.sqrt(var[k])
    return x.astype(np.float32).astype(np.float64)


FLT_MAX = float(np.finfo(np.float32).max)
LOG2E = 1.4426950408889634


def log_terms(X, ubm):
    """[T, K]: ln w_k + ln N(x_t; mu_k, var_k).  The device evaluates the densities in fp32 as log2 values: a term whose
    log2 distance sum_d (x_d - mu_kd)^2 log2e / (2 var_kd) is beyond fp32's range is -inf there, and so it is here -- that is
    what "values so large that every density is -inf" means."""
    w, mu, var = ubm
    X = np.asarray(X, dtype=np.float64)
    with np.errstate(all="ignore"):
        c = np.log(w) - 0.5 * np.sum(np.log(2.0 * np.pi * var), axis=1)
        q = ((X[:, None, :] - mu[None]) ** 2 / var[None]).sum(axis=2)
        return np.where(0.5 * LOG2E * q > FLT_MAX, -np.inf, c[None] - 0.5 * q)


def stats(X, ubm):
    """-> (N [K], F [K * D], ll, dropped, ll_t [T]) of one utterance, log domain: a frame contributes iff its log-sum-exp is
    finite (ll_t is NaN for a dropped frame)."""
    w, mu, var = ubm
    K, D = mu.shape
    X = np.asarray(X, dtype=np.float64).reshape(-1, D)
    if X.shape[0] == 0:
        return np.zeros(K), np.zeros(K * D), 0.0, 0, np.zeros(0)
    t = log_terms(X, ubm)
    with np.errstate(all="ignore"):
        m = np.max(t, axis=1)
        lse = m + np.log(np.sum(np.exp(t - m[:, None]), axis=1))
        live = np.isfinite(lse)
        gam = np.exp(t[live] - lse[live, None])
    N = gam.sum(axis=0)
    F = (gam.T @ X[live]).reshape(-1)
    return N, F, float(lse[live].sum()), int((~live).sum()), np.where(live, lse, np.nan)


def stats_loops(X, ubm):
    """The same, frame by frame and mixture by mixture."""
    w, mu, var = ubm
    K, D = mu.shape
    N, F, ll, dropped = np.zeros(K), np.zeros((K, D)), 0.0, 0
    for x in np.asarray(X, dtype=np.float64).reshape(-1, D):
        t = []
        for k in range(K):
            a, far = math.log(w[k]), 0.0
            for d in range(D):
                z = x[d] - mu[k, d]
                a += -0.5 * math.log(2.0 * math.pi * var[k, d]) - 0.5 * z * z / var[k, d] if math.isfinite(z) else float("nan")
                far += 0.5 * LOG2E * z * z / var[k, d] if math.isfinite(z) else 0.0
            t.append(-math.inf if far > FLT_MAX else a)
        top = max(t) if not any(math.isnan(v) for v in t) else float("nan")       # (all -inf: the total is not finite either)
        tot = top + math.log(sum(math.exp(v - top) for v in t)) if math.isfinite(top) else float("nan")
        if not math.isfinite(tot):
            dropped += 1
            continue
        ll += tot
        for k in range(K):
            g = math.exp(t[k] - tot)
            N[k] += g
            for d in range(D):
                F[k, d] += g * x[d]
    return N, F.reshape(-1), ll, dropped


def stats_linear(data, m, v, w):
    """The reference's formula in its own orientation and domain (data [D, T], m and v [D, K], w [K]): a = w / ((2 pi)^(D/2)
    sqrt(prod v)), gammas = a exp(-0.5 sum (x - m)^2 / v) normalised per frame, N = sum gammas, F = data gammas' column by column."""
    data, m, v = (np.asarray(a, dtype=np.float64) for a in (data, m, v))
    D, K = m.shape
    a = np.asarray(w, dtype=np.float64).reshape(-1) / ((2.0 * np.pi) ** (D / 2.0) * np.sqrt(np.prod(v, axis=0)))
    gam = np.empty((K, data.shape[1]))
    for k in range(K):
        gam[k] = np.exp((-0.5 / v[:, k]) @ (data - m[:, k:k + 1]) ** 2) * a[k]
    tot = gam.sum(axis=0)
    gam = gam / tot
    return gam.sum(axis=1), (data @ gam.T).reshape(-1, order="F"), tot


def batch_stats(utts, ubm):
    """-> N [U, K], F [U, K * D], ll [U], dropped [U], ll_t (list of [T_u]) of a list of utterances."""
    r = [stats(x, ubm) for x in utts]
    return (np.stack([a[0] for a in r]), np.stack([a[1] for a in r]), np.array([a[2] for a in r]),
            np.array([a[3] for a in r], dtype=np.int64), [a[4] for a in r])


def gates(N, F, ll, dropped, want, lengths):
    """The four gates against the restatement `want` = batch_stats(...): worst ratio of each (<= 1 passes), as a dict.
      |N - N*| <= 1e-5 T_u;  |F - F*| <= 1e-4 max(N*[u, k], 1);  |sum_k N[u, k] - (T_u - dropped[u])| <= 1e-5 T_u;
      |ll - ll*| <= 1e-4 sum_t max(1, |ll_t*|)."""
    Nw, Fw, llw, dw, llt = want
    U, K = Nw.shape
    T = np.maximum(np.asarray(lengths, dtype=np.float64), 1e-300)
    D = Fw.shape[1] // K
    out = {"dropped_equal": bool(np.array_equal(np.asarray(dropped), dw))}
    out["N"] = float(np.max(np.abs(N - Nw) / (1e-5 * T[:, None]), initial=0.0))
    out["F"] = float(np.max(np.abs(F - Fw).reshape(U, K, D) / (1e-4 * np.maximum(Nw, 1.0))[:, :, None], initial=0.0))
    out["sum"] = float(np.max(np.abs(N.sum(axis=1) - (np.asarray(lengths) - dw)) / (1e-5 * T), initial=0.0))
    den = np.array([1e-4 * np.sum(np.maximum(1.0, np.abs(a[np.isfinite(a)]))) for a in llt])
    out["ll"] = float(np.max(np.abs(ll - llw) / np.maximum(den, 1e-300), initial=0.0))
    return out


def passes(g):
    return g["dropped_equal"] and max(g["N"], g["F"], g["sum"], g["ll"]) <= 1.0
