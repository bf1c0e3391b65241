#!/usr/bin/env python3
"""Full-covariance GMMs (csrc/gmm_full.hip) on the device: scoring throughput and enrolment time; one JSON line on stdout.

    python scripts/time_full_cov.py [--frames 1000000] [--out profiles/full_cov.json]

Predict: S in {10, 100} speakers of K 32 x D 28 (and S 100 at D 39), 1 M resident fp32 frames in utterances of 300 drawn from the
models.  Kernel time from the library's device events (scoring + per-utterance sums) after a warm-up; algorithmic flops
K (2 D^2 + 3 D + 6) per frame-model against the 157.3 TF f32 matrix peak.  Enrol: K 32, D 28 on 5600 frames (k-means init + EM).
scikit-learn on the host's cores is the baseline where it imports ("absent" otherwise).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MATRIX_TF = 157.3


def model(rng, K, D):
    w = rng.uniform(0.5, 1.5, K)
    w /= w.sum()
    mu = rng.normal(0, 3.0, (K, D))
    A = rng.normal(0, 1, (K, D, D)) / np.sqrt(D)
    cov = A @ np.transpose(A, (0, 2, 1)) + np.array([np.diag(rng.uniform(0.3, 1.0, D)) for _ in range(K)])
    return w, mu, cov


def draw(rng, m, n):
    w, mu, cov = m
    comp = rng.choice(len(w), size=n, p=w)
    L = np.linalg.cholesky(cov)
    return (mu[comp] + np.einsum("nij,nj->ni", L[comp], rng.normal(0, 1, (n, mu.shape[1])))).astype(np.float32)


def predict_case(S, K, D, n_frames, utt_len, reps=5):
    from speaker_recognition_amd import _lib, skgmm
    from speaker_recognition_amd.core import Batch
    rng = np.random.default_rng(S * 1000 + D)
    models = [model(rng, K, D) for _ in range(S)]
    n_utt = n_frames // utt_len
    per = -(-n_utt // S) * utt_len                          # each speaker's utterances drawn from its own model
    X = np.concatenate([draw(rng, models[s], per) for s in range(S)])[:n_utt * utt_len]
    offsets = np.arange(0, n_utt * utt_len + 1, utt_len, dtype=np.int64)
    gmms = [skgmm.GMM.from_arrays(*m) for m in models]
    fs = skgmm.FullSet(gmms)
    batch = Batch.from_features(X, offsets)
    fs.score(batch)                                        # warm-up
    _lib.profile_enable(True)
    _lib.profile_reset()
    for _ in range(reps):
        fs.score(batch)
    ms, launches = _lib.profile_get(_lib.T_SCORE)
    _lib.profile_enable(False)
    ms /= reps
    flops = float(n_utt * utt_len) * S * K * (2 * D * D + 3 * D + 6)
    tf = flops / (ms * 1e-3) / 1e12
    return dict(S=S, K=K, D=D, frames=int(n_utt * utt_len), utt_len=utt_len, kernel_ms=round(ms, 3),
                frames_per_s=round(n_utt * utt_len / (ms * 1e-3)), frame_models_per_s=round(n_utt * utt_len * S / (ms * 1e-3)),
                algorithmic_tflops=round(tf, 2), share_of_f32_matrix_peak=round(tf / PEAK_F32_MATRIX_TF, 3)), (models, X)


def enrol_case(K=32, D=28, n=5600, reps=3):
    from speaker_recognition_amd import skgmm
    rng = np.random.default_rng(11)
    X = draw(rng, model(rng, 8, D), n).astype(np.float64)
    skgmm.GMM(K).fit(X)                                    # warm-up
    ts, g = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        g = skgmm.GMM(K).fit(X)
        ts.append((time.perf_counter() - t0) * 1e3)
    ms = float(np.median(ts))
    # EM alone, from the fitted model's own initialisation path: fit with explicit inits, max_iter iterations, tol 0
    w0 = np.full(K, 1.0 / K)
    mu0 = X[rng.choice(n, K, replace=False)]
    prec0 = np.repeat(np.linalg.inv(np.cov(X.T) + 0.1 * np.eye(D))[None], K, axis=0)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        skgmm.GMM(K, tol=0.0, max_iter=20, weights_init=w0, means_init=mu0, precisions_init=prec0).fit(X)
        t0 = time.perf_counter()
        skgmm.GMM(K, tol=0.0, max_iter=20, weights_init=w0, means_init=mu0, precisions_init=prec0).fit(X)
        t20 = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        skgmm.GMM(K, tol=0.0, max_iter=1, weights_init=w0, means_init=mu0, precisions_init=prec0).fit(X)
        t1 = (time.perf_counter() - t0) * 1e3
    return dict(K=K, D=D, frames=n, ms_per_fit=round(ms, 2), n_iter=int(g.n_iter_), converged=bool(g.converged_),
                us_per_em_iteration=round((t20 - t1) / 19 * 1e3, 1))


def sklearn_baseline(models, X, K=32, D=28, n=5600):
    try:
        from sklearn.mixture import GaussianMixture
    except Exception:
        return "absent"
    rng = np.random.default_rng(11)
    Xf = draw(rng, model(rng, 8, D), n).astype(np.float64)
    t0 = time.perf_counter()
    GaussianMixture(K, random_state=0).fit(Xf)
    fit_ms = (time.perf_counter() - t0) * 1e3
    sub = X[:100000].astype(np.float64)
    gm = GaussianMixture(K)
    w, mu, cov = models[0]
    from scipy.linalg import solve_triangular
    gm.weights_, gm.means_, gm.covariances_ = w, mu, cov
    gm.precisions_cholesky_ = np.array([solve_triangular(np.linalg.cholesky(c), np.eye(D), lower=True).T for c in cov])
    t0 = time.perf_counter()
    gm.score_samples(sub)
    s = time.perf_counter() - t0
    return dict(host_cpus=os.cpu_count(), fit_ms=round(fit_ms, 1), score_frame_models_per_s=round(len(sub) / s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from speaker_recognition_amd import _lib
    rec = dict(device=_lib.device_name(), predict=[], enrol=None, sklearn_host=None)
    keep = None
    for S, D in ((10, 28), (100, 28), (100, 39)):
        r, data = predict_case(S, 32, D, a.frames, 300)
        rec["predict"].append(r)
        if S == 10 and D == 28:
            keep = data
        print(json.dumps(r), file=sys.stderr)
    rec["enrol"] = enrol_case()
    print(json.dumps(rec["enrol"]), file=sys.stderr)
    rec["sklearn_host"] = sklearn_baseline(*keep)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
