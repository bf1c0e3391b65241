#!/usr/bin/env python3
"""Serving full-covariance speaker sets from PCM (FullSet.predict_pcm, ServingStream and MultiPredictor.from_full over skgmm
models): every case on the same inputs in one call; one JSON line on stdout.

    python scripts/time_full_serving.py [--frames 1000000] [--cases abc] [--out profiles/full_serving.json]

(a) 100 speakers x K 32 x D 28 (mix_feature: 13 MFCC + LPC-15) on ~1 M frames of resident 16 kHz int16 PCM in utterances of
    300 frames: the fused call against the per-utterance loop ModelInterface.predict runs (mix_feature, then GMMSet.predict_one,
    a host round trip each) and against GMMSet.predict on features already on the host.  Device time per stage from the
    library's events (MFCC + LPC, CMVN, scoring + finalize).
(b) 20 speakers x 32 x 28, 8 kHz 1 s windows: host-observed submit -> collect latency of one tick, plain and graph-replayed, for
    1 and 6 windows per tick.
(c) the multi predictor from page-locked PCM (the PCM of (a)), 2 slots against 1.  Slots beyond the visible GPUs share one.
Anything not run is reported as "not measured".
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def models_from(rng, X, S, K):
    """S models around real feature frames: K frames of X as means, half the frames' covariance (well conditioned)."""
    from speaker_recognition_amd import skgmm
    D = X.shape[1]
    cov0 = np.cov(X.T) + 1e-3 * np.eye(D)
    cov = 0.5 * cov0 + 0.05 * np.diag(np.diag(cov0))
    out = []
    for _ in range(S):
        mu = X[rng.choice(len(X), K, replace=False)] + 0.1 * rng.standard_normal((K, D))
        w = rng.uniform(0.5, 1.5, K)
        out.append(skgmm.GMM.from_arrays(w / w.sum(), mu, np.repeat(cov[None], K, axis=0)))
    return out


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def setup(fs, S, K, n_base=8, base_s=60.0, seed=1):
    from speaker_recognition_amd import skgmm, synth
    from speaker_recognition_amd.core import MfccExtractor
    ex = MfccExtractor(fs, n_lpc=15)
    base = [synth.synth_speech(9 * s, base_s, fs, seed=100 + s) for s in range(n_base)]
    X = np.concatenate([ex.extract(b[:fs * 10]) for b in base])
    gmms = models_from(np.random.default_rng(seed), X, S, K)
    gs = skgmm.GMMSet(K)
    gs.gmms, gs.y = gmms, ["spk%d" % s for s in range(S)]
    return ex, base, gmms, gs


def case_a(n_frames, loop_utts):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    from speaker_recognition_amd.feature import mix_feature
    fs, S, K, T = 16000, 100, 32, 300
    ex, base, gmms, gs = setup(fs, S, K)
    fset = gs._full_set()
    L = ex.FRAME_LEN + (T - 1) * ex.FRAME_SHIFT                 # samples of a 300-frame utterance
    assert ex.num_frames(L) == T
    U = n_frames // T
    rng = np.random.default_rng(2)
    off = np.arange(U + 1, dtype=np.int64) * L
    cat = np.empty(U * L, np.int16)
    for u in range(U):
        b = base[u % len(base)]
        o = int(rng.integers(0, len(b) - L))
        cat[u * L:(u + 1) * L] = b[o:o + L]
    batch = Batch.from_pcm((cat, off))
    out = {"S": S, "K": K, "D": 28, "utterances": U, "frames_per_utterance": T, "frames": U * T, "pcm_samples": int(U * L)}
    bufs = (np.zeros((U, S)), np.zeros(U, np.int32))
    fset.predict_pcm(ex, batch, out=bufs)                          # warm-up: tables, workspaces
    out["fused_ms"] = median_ms(lambda: fset.predict_pcm(ex, batch, out=bufs), 5)
    _lib.profile_enable(True)
    _lib.profile_reset()
    reps = 3
    for _ in range(reps):
        fset.predict_pcm(ex, batch, out=bufs)
    for name, kind in (("features_mfcc_lpc", _lib.T_MFCC), ("cmvn", _lib.T_CMVN), ("scoring_and_finalize", _lib.T_SCORE)):
        ms, _ = _lib.profile_get(kind)
        out["fused_device_ms_" + name] = round(ms / reps, 3)
    _lib.profile_enable(False)
    sums, arg = bufs
    fused_labels = [gs.y[a] for a in arg]
    log("(a) fused %.1f ms" % out["fused_ms"])
    # today's per-utterance loop (ModelInterface.predict: mix_feature + GMMSet.predict_one)
    n_loop = U if loop_utts <= 0 else min(U, loop_utts)
    feats, labels = [], []
    t0 = time.perf_counter()
    for u in range(n_loop):
        f = mix_feature((fs, cat[u * L:(u + 1) * L]))
        feats.append(f)
        labels.append(gs.predict_one(f))
        if u % 500 == 499:
            log("(a) loop %d / %d" % (u + 1, n_loop))
    loop_ms = (time.perf_counter() - t0) * 1e3
    out["per_utterance_predict_loop_ms"] = round(loop_ms * U / n_loop, 1)
    out["per_utterance_predict_loop_utterances_timed"] = n_loop
    out["per_utterance_predict_loop_labels_equal_fused"] = labels == fused_labels[:n_loop]
    if n_loop == U:
        gs.predict(feats)                                          # warm-up
        out["gmmset_predict_host_features_ms"] = median_ms(lambda: gs.predict(feats), 3)
        out["gmmset_predict_labels_equal_fused"] = gs.predict(feats) == fused_labels
    else:
        out["gmmset_predict_host_features_ms"] = "not measured"
    out["fused_speedup_vs_loop"] = round(out["per_utterance_predict_loop_ms"] / out["fused_ms"], 1)
    return out, (gmms, cat, off, sums, arg)


def case_b():
    from speaker_recognition_amd.core import ServingStream
    fs, S, K = 8000, 20, 32
    ex, base, gmms, gs = setup(fs, S, K, n_base=4, base_s=40.0, seed=3)
    fset = gs._full_set()
    audio = base[0]
    out = {"S": S, "K": K, "D": 28, "fs": fs, "window_s": 1.0, "frames_per_window": ex.num_frames(fs)}
    for n_win in (1, 6):
        pcm = np.stack([audio[(j % 39) * fs // 2:(j % 39) * fs // 2 + fs] for j in range(n_win)])
        for graph in (False, True):
            st = ServingStream(ex, fset, n_win, fs, graph=graph)
            lat = []
            for i in range(230):
                t1 = time.perf_counter()
                st.submit(pcm)
                st.collect()
                lat.append((time.perf_counter() - t1) * 1e3)
            lat = np.array(lat[30:])
            key = "stream_%d_windows%s" % (n_win, "_hipgraph" if graph else "")
            out[key] = {"latency_ms_p50": round(float(np.percentile(lat, 50)), 4),
                        "latency_ms_p99": round(float(np.percentile(lat, 99)), 4)}
            log("(b) %s p50 %.3f ms" % (key, out[key]["latency_ms_p50"]))
            del st
    return out


def case_c(data):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import MultiPredictor
    gmms, cat, off, sums, arg = data
    out = {"visible_devices": _lib.device_count(), "utterances": len(off) - 1, "pcm_bytes": int(cat.nbytes)}
    _lib.host_register(cat)
    try:
        for n_slots in (1, 2):
            mp = MultiPredictor.from_full(gmms, 16000, n_slots=n_slots)
            s, a = mp.predict_concat(cat, off)                     # warm-up: per-piece buffers and tables
            out["bits_equal_fused_%d_slots" % n_slots] = bool(np.array_equal(s, sums) and np.array_equal(a, arg))
            out["multi_%d_slots_ms" % n_slots] = median_ms(lambda: mp.predict_concat(cat, off), 5)
            log("(c) %d slots %.1f ms" % (n_slots, out["multi_%d_slots_ms" % n_slots]))
            del mp
    finally:
        _lib.host_unregister(cat)
    if out["visible_devices"] < 2:
        out["note"] = "one visible GPU: both slots of the 2-slot predictor share it (one queue)"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000000)
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--loop-utts", type=int, default=0, help="time the per-utterance loop on this many (0: all)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from speaker_recognition_amd import _lib
    res = {"device": _lib.device_name()}
    data = None
    if "a" in args.cases or "c" in args.cases:
        a, data = case_a(args.frames, args.loop_utts)
        res["a_fused_1M_frames"] = a if "a" in args.cases else "not measured"
    else:
        res["a_fused_1M_frames"] = "not measured"
    res["b_stream_latency"] = case_b() if "b" in args.cases else "not measured"
    res["c_multi_predictor"] = case_c(data) if "c" in args.cases else "not measured"
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
