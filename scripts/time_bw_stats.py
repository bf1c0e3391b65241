#!/usr/bin/env python3
"""What the batched Baum-Welch statistics cost on the device (csrc/bw_stats.hip), in one run; one JSON line on stdout.

    python scripts/time_bw_stats.py [--out profiles/r13_bw_stats.json] [--host-sessions 4]

Three shapes: (a) 1000 sessions x 1000 frames against a 512 x 39 model, (b) 64 sessions x 300 frames against the same model,
(c) 1000 sessions x 3000 frames against the reference's 256 x 13 JFA UBM (tests/golden/jfa_ubm.npz).  For each:
  * ModelSet.bw_stats on the resident feature batch (upload excluded; the call ends with N and F in host memory, so it includes
    their download: 8 U K (D + 1) bytes),
  * the device times of its three passes (log-sum-exp, statistics, reduce) from the library's event timers (SR_T_BW_*),
  * ModelSet.score of the same frames against the same one-model set: the exact pass that forms the same K x D densities and no
    statistics,
  * the float64 numpy restatement (tests/bw_cases.py) looped on the host over the first --host-sessions sessions in the same run
    (its time per session times the session count is the extrapolated figure),
and at (a) the four gates of tests/test_gpu_bw_stats.py on those sessions, as worst ratios (<= 1 passes).
Medians of 5 after a warm-up, host wall clock around a device synchronisation."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(fn, reps=5):
    from speaker_recognition_amd import _lib
    fn()
    _lib.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        _lib.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), res


def shape(name, ubm, n_sessions, frames, n_host, with_gates):
    import bw_cases as bc
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch, ModelSet
    from speaker_recognition_amd.pygmm import GMM
    K, D = ubm[1].shape
    X = bc.draw(ubm, n_sessions * frames, 1000 + K).astype(np.float32)
    off = np.arange(n_sessions + 1, dtype=np.int64) * frames
    feats = Batch.from_features(X, off)
    ms = ModelSet([GMM.from_arrays(ubm[0], ubm[1], np.sqrt(ubm[2]))])
    call_ms, res = median_ms(lambda: ms.bw_stats(feats, ll=True))
    score_ms, _ = median_ms(lambda: ms.score(feats))
    _lib.profile_enable(True)
    _lib.profile_reset()
    ms.bw_stats(feats)
    passes = {k: _lib.profile_get(kind) for k, kind in (("lse", _lib.T_BW_LSE), ("stats", _lib.T_BW_STATS), ("reduce", _lib.T_BW_REDUCE))}
    _lib.profile_enable(False)
    n_host = min(n_host, n_sessions)
    utts = [X[off[u]:off[u + 1]].astype(np.float64) for u in range(n_host)]
    t0 = time.perf_counter()
    want = bc.batch_stats(utts, ubm)
    host_s = time.perf_counter() - t0
    plan = _lib.bw_plan(K, D, np.diff(off))
    out = {"shape": name, "sessions": n_sessions, "frames_each": frames, "K": K, "D": D, "bw_stats_call_ms": call_ms,
           "result_bytes": int(8 * n_sessions * K * (D + 1)), "score_pass_ms": score_ms, "score_kernel": _lib.last_score_kernel(),
           "device_pass_ms": {k: v[0] for k, v in passes.items()}, "device_pass_launches": {k: int(v[1]) for k, v in passes.items()},
           "ranges": plan["n_ranges"], "groups": plan["n_groups"], "slab_bytes": plan["slab_bytes"],
           "host_numpy_sessions_timed": n_host, "host_numpy_ms_per_session": 1e3 * host_s / n_host,
           "host_numpy_ms_extrapolated": 1e3 * host_s / n_host * n_sessions}
    if with_gates:
        N, F, ll, dropped = (a[:n_host] for a in res)
        out["gates_worst_ratio"] = bc.gates(N, F, ll, dropped, want, [frames] * n_host)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--host-sessions", type=int, default=4)
    args = ap.parse_args()
    import bw_cases as bc
    from speaker_recognition_amd import _lib
    big = bc.make_ubm(512, 39, 77)
    out = {"device": _lib.device_name(),
           "shapes": [shape("a_1000x1000_512x39", big, 1000, 1000, args.host_sessions, True),
                      shape("b_64x300_512x39", big, 64, 300, args.host_sessions, False),
                      shape("c_1000x3000_fixture_256x13", bc.fixture_ubm(), 1000, 3000, args.host_sessions, False)]}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
