#!/usr/bin/env python3
"""What the timeline costs on the device (csrc/timeline.hip), in one run; one JSON line on stdout.

    python scripts/time_timeline.py [--out profiles/r26_timeline.json] [--models 201] [--mixtures 512]

Three shapes against one set of 201 models x 512 mixtures x 39 dimensions (column 0 plays the background), window 150 frames, hop 40,
minimum turn 2 windows: 1 recording x 360 000 frames, 64 x 30 000, 1000 x 3000.  The features are draws from the models.  Per
shape and mode (none / hold / viterbi):
  call_ms          host wall clock around ModelSet.timeline, median of 3 after a warm-up;
  score_ms         device time of the scoring pass (timer kinds SR_T_SCORE + SR_T_FINALIZE), same calls;
  sum_ms           the window-sum kernel (SR_T_CMVN);
  decide_ms        the decision kernels, for viterbi with the forward kernel (SR_T_SCORE_REF);
  trace_ms         the traceback (SR_T_ESTEP), viterbi only;
  step_us          viterbi: decide_ms over the windows of the longest recording -- what one step of the sequential decode costs.
Two baselines in the same run:
  numpy            ModelSet.score(frame_ll=True) brought home, then the numpy restatement (tests/timeline_oracle.py) on the first
                   recordings, extrapolated to the shape; its labels are checked against the device's;
  window_loop      the loop the reference implies: the windows of the first recordings cut out as separate utterances and scored
                   by ONE ModelSet.score call (upload included), extrapolated to the shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
W, H, M, BETA, DIM = 150, 40, 2, 2.0, 39


def make_models(S, K):
    """S diagonal models of K mixtures: one draw of synth_gmm's distribution, the speakers' means shifted copies of it"""
    rng = np.random.default_rng(26)
    mean = rng.standard_normal((K, DIM))
    sigma = rng.uniform(0.2, 1.5, (K, DIM))
    w = rng.dirichlet(np.ones(K))
    return [(w, mean + (0.0 if s == 0 else 0.3) * rng.standard_normal((K, DIM)), sigma) for s in range(S)]


def draw(models, n_utt, frames, seed):
    """n_utt recordings of `frames` frames: turns of 200 frames, each drawn from one speaker's model"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_utt):
        X = np.empty((frames, DIM), np.float32)
        for a in range(0, frames, 200):
            w, mean, sigma = models[int(rng.integers(1, len(models)))]
            b = min(frames, a + 200)
            k = rng.choice(len(w), size=b - a, p=w)
            X[a:b] = mean[k] + sigma[k] * rng.standard_normal((b - a, DIM))
        out.append(X)
    return out


def timed(fn, reps=3):
    from speaker_recognition_amd import _lib
    fn()
    _lib.synchronize()
    rows = []
    for _ in range(reps):
        _lib.profile_reset()
        t0 = time.perf_counter()
        res = fn()
        _lib.synchronize()
        call = (time.perf_counter() - t0) * 1e3
        k = {name: _lib.profile_get(kind)[0] for name, kind in (("score", _lib.T_SCORE), ("finalize", _lib.T_FINALIZE), ("sum", _lib.T_CMVN),
                                                                ("decide", _lib.T_SCORE_REF), ("trace", _lib.T_ESTEP))}
        rows.append((call, k["score"] + k["finalize"], k["sum"], k["decide"], k["trace"]))
    med = np.median(np.array(rows), axis=0)
    return dict(zip(("call_ms", "score_ms", "sum_ms", "decide_ms", "trace_ms"), (float(x) for x in med))), res


def shape(ms, models, n_utt, frames, n_base):
    import timeline_oracle as to
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    recs = draw(models, n_utt, frames, 1000 + n_utt)
    feats = Batch.from_features(recs)
    S = len(models)
    nw = to.windows(frames, W, H)
    out = {"recordings": n_utt, "frames_each": frames, "windows_each": nw, "plan": _lib.timeline_plan(S, M, frames, W, H)}
    labels = {}
    for smooth, kw in (("none", {}), ("hold", {}), ("viterbi", dict(switch_penalty=BETA, min_windows=M))):
        t, res = timed(lambda: ms.timeline(feats, W, H, bg=0, threshold=0.0, smooth=smooth, **kw))
        if smooth == "viterbi":
            t["step_us"] = 1e3 * t["decide_ms"] / max(1, nw - 1)
        labels[smooth] = res
        out[smooth] = t
    # (a) the numpy restatement on the frame matrix brought home
    t0 = time.perf_counter()
    _, _, fll = ms.score(feats, frame_ll=True)
    home_ms = (time.perf_counter() - t0) * 1e3
    off = feats.offsets()
    t0 = time.perf_counter()
    same = True
    for u in range(n_base):
        wsum, wcnt = to.window_sums(fll[:, off[u]:off[u + 1]], W, H)
        for smooth, okw in (("none", dict(mode=0)), ("hold", dict(mode=1)), ("viterbi", dict(mode=2, beta=BETA, m=M))):
            same = same and bool(np.array_equal(to.decide(wsum, wcnt, bg=0, threshold=0.0, **okw)[0], labels[smooth][u]))
    host_ms = (time.perf_counter() - t0) * 1e3
    out["numpy"] = {"score_and_copy_home_ms": home_ms, "recordings_timed": n_base, "restatement_ms_three_modes_per_recording": host_ms / n_base,
                    "restatement_ms_extrapolated": host_ms / n_base * n_utt, "labels_equal_device": same}
    del fll
    # (b) the windows as separate utterances in one scoring call
    cut = [recs[u][j * H:j * H + W] for u in range(n_base) for j in range(nw)]
    t0 = time.perf_counter()
    wb = Batch.from_features(cut)
    ms.score(wb)
    _lib.synchronize()
    first = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    wb = Batch.from_features(cut)
    _, arg = ms.score(wb)
    _lib.synchronize()
    loop_ms = (time.perf_counter() - t0) * 1e3
    out["window_loop"] = {"recordings_timed": n_base, "windows_scored": len(cut), "frames_scored": int(sum(len(c) for c in cut)),
                          "upload_and_score_ms": loop_ms, "first_call_ms": first, "ms_extrapolated": loop_ms / n_base * n_utt,
                          "frames_scored_over_frames_of_the_recordings": float(sum(len(c) for c in cut)) / (n_base * frames)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--models", type=int, default=201)
    ap.add_argument("--mixtures", type=int, default=512)
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks the three shapes' frame counts (a dry run)")
    args = ap.parse_args()
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import ModelSet
    from speaker_recognition_amd.pygmm import GMM
    models = make_models(args.models, args.mixtures)
    ms = ModelSet([GMM.from_arrays(*m) for m in models])
    _lib.profile_enable(True)
    f = lambda n: max(W + H, int(n * args.scale))  # noqa: E731
    out = {"device": _lib.device_name(), "set": "%d x %d x %d" % (args.models, args.mixtures, DIM), "window": W, "hop": H, "min_windows": M,
           "switch_penalty": BETA, "timers": "medians of 3 calls after a warm-up; HIP events around the launches",
           "one_360000": shape(ms, models, 1, f(360000), 1), "batch_64x30000": shape(ms, models, 64, f(30000), 4),
           "batch_1000x3000": shape(ms, models, 1000, f(3000), 40), "scoring_kernel": _lib.last_score_kernel()}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
