#!/usr/bin/env python3
"""Enrolling a full-covariance speaker set: the loop of single fits (skgmm.GMM.fit, one sr_fullgmm_fit per speaker: a loop of
one-speaker groups through the EM driver) against the batched fit (skgmm.fit_many, one sr_fullgmm_fit_batch: the same driver on
groups of many); one JSON line on stdout.

    python scripts/time_full_enrol.py [--speakers 10,100] [--reps 5] [--out profiles/full_enrol.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_full_enrol.py --batch-only 100      # per-kernel times

Shape: K 32 x D 28 on 5600 frames per speaker (time_full_cov.py's enrolment shape), k-means start, the default stop rule.  Both
sides run in one process, alternating, after a warm-up of each; the figures are medians of wall time around the Python call.
The two sides give the same models bit for bit (checked here on every run), so the comparison is of time alone.

Split: with tol = 0 every fit runs exactly max_iter iterations, so (t(max_iter 41) - t(max_iter 1)) / 40 is the cost of one EM
iteration of the whole set -- per speaker in the loop, per batch iteration in the batched call -- and t(max_iter 1) minus one
iteration is the start: upload, k-means (host-sequenced, per speaker on both sides), the first M-step.  The headline's EM share is
its total minus that start.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, D, N = 32, 28, 5600


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
    return mu[comp] + np.einsum("nij,nj->ni", L[comp], rng.normal(0, 1, (n, mu.shape[1])))


def data(S):
    rng = np.random.default_rng(900 + S)
    return [draw(rng, model(rng, 8, D), N) for _ in range(S)]


def loop(Xs, **kw):
    from speaker_recognition_amd import skgmm
    gm = [skgmm.GMM(K, random_state=s, **kw) for s in range(len(Xs))]
    t0 = time.perf_counter()
    for g, X in zip(gm, Xs):
        g.fit(X)
    return (time.perf_counter() - t0) * 1e3, gm


def batched(Xs, **kw):
    from speaker_recognition_amd import skgmm
    gm = [skgmm.GMM(K, random_state=s, **kw) for s in range(len(Xs))]
    t0 = time.perf_counter()
    errors = skgmm.fit_many(gm, Xs)
    ms = (time.perf_counter() - t0) * 1e3
    assert errors == [None] * len(Xs), errors
    return ms, gm


def ab(Xs, reps, **kw):
    """-> (median ms of the loop, of the batched call, the models of the last run of each)"""
    loop(Xs, **kw)
    batched(Xs, **kw)
    tl, tb = [], []
    for _ in range(reps):
        ms, gl = loop(Xs, **kw)
        tl.append(ms)
        ms, gb = batched(Xs, **kw)
        tb.append(ms)
    for a, b in zip(gl, gb):
        for attr in ("weights_", "means_", "covariances_", "precisions_cholesky_"):
            assert np.array_equal(getattr(a, attr), getattr(b, attr)), "the batched fit differs from the single fit"
        assert a.n_iter_ == b.n_iter_ and a.lower_bound_ == b.lower_bound_
    return float(np.median(tl)), float(np.median(tb)), gl


def case(S, reps):
    Xs = data(S)
    l, b, gm = ab(Xs, reps)
    iters = [g.n_iter_ for g in gm]
    l1, b1, _ = ab(Xs, reps, tol=0.0, max_iter=1)
    l41, b41, _ = ab(Xs, reps, tol=0.0, max_iter=41)
    it_l, it_b = (l41 - l1) / 40.0, (b41 - b1) / 40.0
    start_l, start_b = l1 - it_l, b1 - it_b
    return {
        "S": S, "K": K, "D": D, "frames_per_speaker": N, "reps": reps,
        "n_iter": {"min": int(min(iters)), "median": float(np.median(iters)), "max": int(max(iters)), "sum": int(sum(iters))},
        "loop_ms": round(l, 2), "batched_ms": round(b, 2), "loop_over_batched": round(l / b, 3),
        "loop_ms_per_speaker": round(l / S, 2), "batched_ms_per_speaker": round(b / S, 2),
        "split": {
            "loop": {"start_ms": round(start_l, 2), "em_ms": round(l - start_l, 2), "ms_per_iteration_of_the_set": round(it_l, 3),
                     "us_per_speaker_iteration": round(1e3 * it_l / S, 1)},
            "batched": {"start_ms": round(start_b, 2), "em_ms": round(b - start_b, 2), "ms_per_batch_iteration": round(it_b, 3),
                        "us_per_speaker_iteration": round(1e3 * it_b / S, 1)},
            "em_share_loop_over_batched": round((l - start_l) / max(1e-9, b - start_b), 2),
            "start_share_of_batched": round(start_b / b, 3),
        },
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--speakers", default="10,100")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch-only", type=int, default=0, metavar="S", help="one warm-up and one batched fit of S speakers, nothing else")
    args = ap.parse_args()
    from speaker_recognition_amd import _lib
    warnings.simplefilter("ignore")
    if args.batch_only:
        Xs = data(args.batch_only)
        batched(Xs)
        ms, _ = batched(Xs)
        print(json.dumps({"S": args.batch_only, "batched_ms": round(ms, 2)}))
        return
    res = {"device": _lib.device_name().strip(), "full_fit_batch_bytes": _lib.full_fit_batch_bytes(), "cases": [case(int(s), args.reps) for s in args.speakers.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
