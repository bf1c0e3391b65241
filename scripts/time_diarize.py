#!/usr/bin/env python3
"""What the diarisation of unknown speakers costs on the device (csrc/diar.hip), in one run; one JSON line on stdout.

    python scripts/time_diarize.py [--out profiles/r27_diarize.json] [--scale 1.0]

Shapes, 39 dimensions, base segments of L = 100 frames, lambda = 0.3, four planted Gaussian speakers in turns of 2 to 8 segments:
  one_360000          1 recording x 360 000 frames, change modes "uniform" (3600 initial clusters) and "bic";
  batch_64x30000      64 recordings x 30 000 frames, both modes;
  matrix_1000 / 4000  the matrix mode (average linkage, the whole dendrogram) on n points' Euclidean distances.
Per call:
  call_ms            host wall clock around the call, median of 3 after a warm-up, timers off (uploads and the results' way home
                     included); the stages below come from one more call with the timers on (call_ms_with_timers);
  stats_ms           the statistics and gather kernels (timer kind SR_T_CMVN);
  factor_ms          every factorisation: cluster logdets, the pair table, change scores, the row updates (SR_T_SCORE_REF);
  loop_ms            the argmin and merge kernels of all steps (SR_T_ESTEP);
  merges, step_us    the steps taken by the longest recording, and call_ms over them;
  argmin_merge_us    loop_ms over those steps.
The numpy restatement (tests/diar_oracle.py) runs in the same process on a stated subset -- the first frames of the first recording,
the first points of the matrix -- and is extrapolated by the stated rule (its pair table grows with the square of the initial
clusters, its merge loop with the cube of n)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DIM, L = 39, 100
PENALTY = 0.3      # lambda.  At 39 dimensions the full-covariance penalty of lambda = 1 (2453 for two sides of 200 frames) exceeds what
                   # a change of speaker gains at these turns, and the bic mode keeps no boundary; at 0.3 it keeps the planted ones


def draw(n_utt, frames, seed, n_speakers=4):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_utt):
        means = rng.normal(0.0, 2.0, (n_speakers, DIM))
        scales = rng.uniform(0.7, 1.4, (n_speakers, DIM))
        X = np.empty((frames, DIM), np.float32)
        a = 0
        while a < frames:
            b = min(frames, a + L * int(rng.integers(2, 9)))
            s = int(rng.integers(0, n_speakers))
            X[a:b] = means[s] + scales[s] * rng.standard_normal((b - a, DIM))
            a = b
        out.append(X)
    return out


def timed(fn, reps=3):
    """call_ms with the timers off (an event pair per launch of a loop of thousands of steps would be in it); the stages from one more
    call with them on."""
    from speaker_recognition_amd import _lib
    _lib.profile_enable(False)
    fn()
    _lib.synchronize()
    calls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        _lib.synchronize()
        calls.append((time.perf_counter() - t0) * 1e3)
    _lib.profile_enable(True)
    _lib.profile_reset()
    t0 = time.perf_counter()
    fn()
    _lib.synchronize()
    profiled = (time.perf_counter() - t0) * 1e3
    stages = [_lib.profile_get(kind)[0] for kind in (_lib.T_CMVN, _lib.T_SCORE_REF, _lib.T_ESTEP)]
    _lib.profile_enable(False)
    out = dict(zip(("stats_ms", "factor_ms", "loop_ms"), (float(x) for x in stages)))
    out.update(call_ms=float(np.median(calls)), call_ms_with_timers=profiled)
    return out, res


def with_steps(t, merges):
    t["merges"] = int(merges)
    t["step_us"] = 1e3 * t["call_ms"] / max(1, merges)
    t["argmin_merge_us"] = 1e3 * t["loop_ms"] / max(1, merges)
    return t


def feature_shape(n_utt, frames, sub_frames):
    import diar_oracle as do
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    recs = draw(n_utt, frames, 2700 + n_utt)
    feats = Batch.from_features(recs)
    out = {"recordings": n_utt, "frames_each": frames, "plan": {k: v for k, v in _lib.diar_plan(DIM, [frames] * n_utt, L=L).items()
                                                               if k not in ("n_seg", "n_init_bound", "rec_bytes")}}
    for change in ("uniform", "bic"):
        t, res = timed(lambda: feats.diarize(L=L, change=change, penalty=PENALTY))
        with_steps(t, max(len(r["merge_d"]) for r in res))
        t["initial_clusters"] = [int(np.median([len(r["labels"]) for r in res])), int(max(len(r["labels"]) for r in res))]
        t["clusters"] = [int(min(r["n_clusters"] for r in res)), int(max(r["n_clusters"] for r in res))]
        # the restatement on the first sub_frames frames of the first recording, and the device on the same frames
        sub = recs[0][:sub_frames]
        t0 = time.perf_counter()
        want = do.cluster(sub, L, change=change, lam=PENALTY)
        host_ms = (time.perf_counter() - t0) * 1e3
        got = Batch.from_features([sub]).diarize(L=L, change=change, penalty=PENALTY)[0]
        n_sub, n_full = len(want["labels"]), t["initial_clusters"][1]
        t["numpy"] = {"frames": int(len(sub)), "initial_clusters": n_sub, "ms": host_ms, "labels_equal_device": got["labels"].tolist() == want["labels"].tolist(),
                      "rule": "ms x (initial clusters of the shape / of the subset)^2 x recordings",
                      "ms_extrapolated": host_ms * (n_full / max(1, n_sub)) ** 2 * n_utt}
        out[change] = t
    return out


def matrix_shape(n, n_sub):
    import diar_oracle as do
    from speaker_recognition_amd import diarize as dz
    rng = np.random.default_rng(4000 + n)
    pts = np.concatenate([rng.normal(c, 1.0, (n // 4 + 1, 8)) for c in rng.normal(0.0, 6.0, (4, 8))])[:n]
    g = pts @ pts.T
    d0 = np.sqrt(np.maximum(0.0, np.diag(g)[:, None] + np.diag(g)[None, :] - 2 * g))
    d0 = (d0 + d0.T) / 2
    t, (lab, log) = timed(lambda: dz.ahc(d0, linkage="average", threshold=float("inf")))
    with_steps(t, len(log[2]))
    t0 = time.perf_counter()
    want = do.ahc(d0[:n_sub, :n_sub], 0, threshold=float("inf"))
    host_ms = (time.perf_counter() - t0) * 1e3
    got = dz.ahc(d0[:n_sub, :n_sub], linkage="average", threshold=float("inf"))[1]
    t["numpy"] = {"n": n_sub, "ms": host_ms, "log_equal_device": bool(np.array_equal(got[2], want["merge_d"]) and np.array_equal(got[0], want["merge_i"])),
                  "rule": "ms x (n / n of the subset)^3", "ms_extrapolated": host_ms * (n / n_sub) ** 3}
    t["n"] = n
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks the shapes (a dry run)")
    args = ap.parse_args()
    from speaker_recognition_amd import _lib
    f = lambda n: max(4 * L, int(n * args.scale))  # noqa: E731
    out = {"device": _lib.device_name(), "dim": DIM, "L": L, "penalty": PENALTY, "timers": "call_ms: median of 3 calls after a warm-up, timers off; stages: HIP events around the launches of one more call",
           "one_360000": feature_shape(1, f(360000), f(30000)), "batch_64x30000": feature_shape(64, f(30000), f(30000)),
           "matrix_1000": matrix_shape(max(8, int(1000 * args.scale)), max(8, int(400 * args.scale))),
           "matrix_4000": matrix_shape(max(8, int(4000 * args.scale)), max(8, int(400 * args.scale)))}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
