"""Float64 numpy restatement of scikit-learn's full-covariance GaussianMixture (the arithmetic skgmm.GMM runs on the device):

  log_gaussian  sklearn.mixture._gaussian_mixture._estimate_log_gaussian_prob (covariance_type='full')
                + _compute_log_det_cholesky, plus GaussianMixture._estimate_log_weights
  e_step        sklearn.mixture._base.BaseMixture._e_step / _estimate_log_prob_resp (log-sum-exp over the mixtures)
  m_step        GaussianMixture._m_step: _estimate_gaussian_parameters (nk + 10 eps, means, _estimate_gaussian_covariances_full
                around the NEW means + reg_covar) + weights / sum + _compute_precision_cholesky
  fit           BaseMixture.fit_predict with n_init = 1 from explicit parameters: the bound of each E-step, taken before its
                M-step, against the previous one; stop when |change| < tol
"""
from __future__ import annotations

import numpy as np
from scipy.linalg import solve_triangular

LN_2PI = np.log(2 * np.pi)
ILL_DEFINED = ("Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance "
               "caused by singleton or collapsed samples). Try to decrease the number of components, increase reg_covar, or "
               "scale the input data.")


def weighted_log_prob(X, weights, means, prec_chol):
    """[n][K] ln w_k + ln N(x | mu_k, (P_k P_k^T)^-1)."""
    X = np.asarray(X, np.float64)
    n, D = X.shape
    K = len(weights)
    log_det = np.array([np.sum(np.log(np.diag(P))) for P in prec_chol])
    lp = np.empty((n, K))
    for k in range(K):
        y = X @ prec_chol[k] - means[k] @ prec_chol[k]
        lp[:, k] = np.sum(np.square(y), axis=1)
    return -0.5 * (D * LN_2PI + lp) + log_det + np.log(weights)


def logsumexp(a):
    m = np.max(a, axis=1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.log(np.sum(np.exp(a - m), axis=1)) + m[:, 0]


def score_samples(X, weights, means, prec_chol):
    return logsumexp(weighted_log_prob(X, weights, means, prec_chol))


def e_step(X, weights, means, prec_chol):
    """-> (mean log_prob_norm = the lower bound, log responsibilities)."""
    wlp = weighted_log_prob(X, weights, means, prec_chol)
    lpn = logsumexp(wlp)
    return float(np.mean(lpn)), wlp - lpn[:, None]


def precision_cholesky(cov):
    out = np.empty_like(cov)
    for k, c in enumerate(cov):
        try:
            L = np.linalg.cholesky(c)
        except np.linalg.LinAlgError:
            raise ValueError(ILL_DEFINED) from None
        out[k] = solve_triangular(L, np.eye(c.shape[0]), lower=True).T
    return out


def m_step(X, resp, reg_covar, normalise=True):
    """-> (weights, means, covariances, precisions_cholesky).  normalise=False: weights nk / n (GaussianMixture._initialize)."""
    X = np.asarray(X, np.float64)
    n, D = X.shape
    nk = resp.sum(axis=0) + 10 * np.finfo(resp.dtype).eps
    means = resp.T @ X / nk[:, None]
    cov = np.empty((len(nk), D, D))
    for k in range(len(nk)):
        diff = X - means[k]
        cov[k] = (resp[:, k] * diff.T) @ diff / nk[k]
        cov[k].flat[::D + 1] += reg_covar
    weights = nk / nk.sum() if normalise else nk / n
    return weights, means, cov, precision_cholesky(cov)


def precisions_to_cholesky(prec):
    return np.array([np.linalg.cholesky(p[::-1, ::-1])[::-1, ::-1] for p in prec])


def fit(X, weights, means, prec_chol, tol=1e-3, reg_covar=1e-6, max_iter=100):
    """EM from explicit parameters -> dict(weights, means, covariances, prec_chol, n_iter, converged, lower_bound, bounds)."""
    lower = -np.inf
    bounds = []
    converged = False
    w, mu, P, cov = np.asarray(weights, np.float64), np.asarray(means, np.float64), np.asarray(prec_chol, np.float64), None
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        prev = lower
        lower, log_resp = e_step(X, w, mu, P)
        w, mu, cov, P = m_step(X, np.exp(log_resp), reg_covar)
        bounds.append(lower)
        if abs(lower - prev) < tol:
            converged = True
            break
    return dict(weights=w, means=mu, covariances=cov, prec_chol=P, n_iter=n_iter, converged=converged, lower_bound=lower,
                bounds=np.array(bounds))


def em_iteration(X, weights, means, prec_chol, reg_covar=1e-6):
    """One E-step + M-step -> (bound before, bound after, new parameters)."""
    b0, log_resp = e_step(X, weights, means, prec_chol)
    w, mu, cov, P = m_step(X, np.exp(log_resp), reg_covar)
    b1, _ = e_step(X, w, mu, P)
    return b0, b1, (w, mu, cov, P)


def random_model(rng, K, D, spread=3.0):
    """A well-conditioned full-covariance model: (weights, means, covariances)."""
    w = rng.uniform(0.5, 1.5, K)
    w /= w.sum()
    mu = rng.normal(0, spread, (K, D))
    cov = np.empty((K, D, D))
    for k in range(K):
        A = rng.normal(0, 1, (D, D)) / np.sqrt(D)
        cov[k] = A @ A.T + np.diag(rng.uniform(0.3, 1.0, D))
    return w, mu, cov


def draw(rng, model, n):
    w, mu, cov = model
    comp = rng.choice(len(w), size=n, p=w)
    L = np.linalg.cholesky(cov)
    z = rng.normal(0, 1, (n, mu.shape[1]))
    return mu[comp] + np.einsum("nij,nj->ni", L[comp], z)


def load_golden(path):
    """tests/golden/fullcov_golden.npz expanded into full arrays (make_fullcov_golden.py stores them compactly):
    ``*_X`` float64 frames, ``score_<c>_P`` and ``fit5_<c>_cov`` full [K][D][D] (the covariances from their recorded lower
    triangles), ``fit_<c>_prec0`` [K][D][D].  ``fit5_<c>_P`` is scikit-learn's precision factor of those covariances
    (_compute_precision_cholesky, restated by precision_cholesky above: it reads the lower triangle only), which is what
    GaussianMixture stores next to them."""
    z = np.load(path)
    out = {k: z[k] for k in z.files}

    def full(t, half):
        K, m = t.shape
        D = int((np.sqrt(8 * m + 1) - 1) / 2)
        a = np.zeros((K, D, D), np.float64)
        i, j = np.triu_indices(D) if half == "upper" else np.tril_indices(D)
        a[:, i, j] = t
        if half == "symmetric from lower":
            a[:, j, i] = t
        return a

    for k in list(out):
        if k.endswith("_X_q"):
            out[k[:-2]] = out.pop(k).astype(np.float64) / 256.0
        elif k.startswith("score_") and k.endswith("_Pu"):
            out[k[:-1]] = full(out.pop(k).astype(np.float64), "upper")
        elif k.endswith("_covl"):
            out[k[:-1]] = full(out.pop(k), "symmetric from lower")
    for k in list(out):
        if k.endswith("_prec0_one"):
            c = k[len("fit_"):-len("_prec0_one")]
            K = len(out["fit_%s_w0" % c])
            out["fit_%s_prec0" % c] = np.repeat(out.pop(k)[None], K, axis=0)
        elif k.startswith("fit5_") and k.endswith("_cov"):
            out[k[:-3] + "P"] = precision_cholesky(out[k])
    return out
