#!/usr/bin/env python3
"""Enrolling a MAP speaker set from one UBM: the loop of single fits (GMMSet.fit_new, one sr_train_f32 per speaker) against the
batched fit (GMMSet.fit_many, one sr_map_fit_batch); one JSON document.

    python scripts/time_map_enrol.py --out profiles/r15_map_enrol.json [--parent-lib PATH] [--reps 5] [--shapes 0,1,2]

Shapes: 200 speakers x 3000 frames x (512 x 39) (configs[2]); 1000 x 3000 x (2048 x 39) (configs[3]) under the default bound;
80 x 311 frames x (256 x 34), the reference's logged run.  The drop-in defaults: 200 iterations, threshold 0.01.
Both sides run in one process, alternating, after a warm-up of each; per shape the record holds the wall times of every repetition
around the Python call, their median and spread (max - min), the passes the batched call launched, the device time of its passes
(the library's event timers, kind T_ESTEP, in one extra profiled call outside the timed ones), the routes and the groups.  The two
sides give the same models bit for bit (checked on every run).  The condition the record states: at 200 x 512 x 39 the batched
median is below the loop's median by more than the loop's own spread.

--parent-lib: the single fit's kernels share their bodies with the batched ones (csrc/em_f64_dev.hpp); with the parent commit's
library given, the single fit's models from that library and from this build are compared bit for bit on three shapes (each
library in a fresh process of its own).
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(200, 3000, 512, 39), (1000, 3000, 2048, 39), (80, 311, 256, 34)]
DIGEST_SHAPES = [(3000, 512, 39), (3000, 2048, 39), (311, 256, 34)]
NEW_SYMBOLS = "sr_map_fit_batch,sr_map_fit_batch_error,sr_map_fit_batch_stats,sr_map_fit_batch_bytes,sr_map_fit_plan"


def speakers(ubm_raw, S, n, seed):
    """S matrices of n frames: the UBM's mixtures with a speaker's shift of the means"""
    w, mu, sg = ubm_raw
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(S):
        k = rng.choice(len(w), size=n, p=w / w.sum())
        shift = 0.3 * rng.standard_normal(mu.shape)
        out.append((mu[k] + shift[k] + sg[k] * rng.standard_normal((n, mu.shape[1]))).astype(np.float32))
    return out


def loop(ubm, xs):
    from speaker_recognition_amd.gmmset import GMMSet
    gs = GMMSet(ubm=ubm)
    t0 = time.perf_counter()
    for s, x in enumerate(xs):
        gs.fit_new(x, s)
    return (time.perf_counter() - t0) * 1e3, gs


def batched(ubm, xs):
    from speaker_recognition_amd.gmmset import GMMSet
    gs = GMMSet(ubm=ubm)
    t0 = time.perf_counter()
    gs.fit_many(xs, list(range(len(xs))))
    return (time.perf_counter() - t0) * 1e3, gs


def stats(v):
    return {"reps_ms": [round(x, 2) for x in v], "median_ms": round(float(np.median(v)), 2), "spread_ms": round(max(v) - min(v), 2)}


def case(S, n, K, D, reps):
    from speaker_recognition_amd import _lib, synth
    from speaker_recognition_amd.pygmm import GMM
    ubm_raw = synth.synth_gmm(K, D, 99)
    ubm = GMM.from_arrays(*ubm_raw)
    xs = speakers(ubm_raw, S, n, 1000 + S)
    loop(ubm, xs[:min(S, 8)])
    batched(ubm, xs)
    tl, tb, passes = [], [], []
    for _ in range(reps):
        ms, gl = loop(ubm, xs)
        tl.append(ms)
        before = _lib.map_fit_batch_stats()
        ms, gb = batched(ubm, xs)
        after = _lib.map_fit_batch_stats()
        tb.append(ms)
        passes.append(after[4] - before[4])
        assert after[1] - before[1] + after[2] - before[2] + after[3] - before[3] == S
    for a, b in zip(gl.gmms, gb.gmms):
        assert all(np.array_equal(x, y) for x, y in zip(a.params(), b.params())), "the batched fit differs from the single fit"
    routes = [after[i] - before[i] for i in (1, 2, 3)]
    _lib.profile_enable(True)
    _lib.profile_reset()
    batched(ubm, xs)
    dev_ms, dev_n = _lib.profile_get(_lib.T_ESTEP)
    _lib.profile_enable(False)
    plan = _lib.map_fit_plan(K, D, [n] * S, scratch_bytes=_lib.map_fit_batch_bytes(), n_cu=0)
    l, b = stats(tl), stats(tb)
    return {
        "S": S, "frames_per_speaker": n, "K": K, "D": D, "reps": reps, "loop": l, "batched": b,
        "loop_over_batched": round(l["median_ms"] / b["median_ms"], 3),
        "loop_ms_per_speaker": round(l["median_ms"] / S, 3), "batched_ms_per_speaker": round(b["median_ms"] / S, 3),
        "gain_exceeds_loop_spread": bool(l["median_ms"] - b["median_ms"] > l["spread_ms"]),
        "passes_launched": passes[-1], "device_ms_of_the_passes": round(dev_ms, 3), "timed_launch_groups": int(dev_n),
        "routes": {"batched": routes[0], "single": routes[1], "handed_over": routes[2]},
        "groups": {"count": plan["n_groups"], "speakers": [int(g[1]) for g in plan["groups"]][:8],
                   "largest_scratch_bytes": plan["max_group_bytes"], "density_grid_of_the_first": [int(plan["groups"][0][2]), plan["n_kb"]]},
        "same_bits_as_the_loop": True,
    }


def digest():
    """single fits at DIGEST_SHAPES with the library this process loaded -> one sha256 per shape (stdout, JSON)"""
    from speaker_recognition_amd import _lib, synth
    from speaker_recognition_amd.pygmm import GMM
    out = []
    for n, K, D in DIGEST_SHAPES:
        ubm_raw = synth.synth_gmm(K, D, 99)
        ubm = GMM.from_arrays(*ubm_raw)
        x = speakers(ubm_raw, 1, n, 77)[0]
        g = GMM(K)
        it = g.fit(x, ubm=ubm)
        assert _lib.last_em_stats_engine() == 5
        h = hashlib.sha256()
        for a in g.params():
            h.update(np.ascontiguousarray(a).tobytes())
        out.append({"frames": n, "K": K, "D": D, "iterations": int(it), "sha256": h.hexdigest()})
    print("DIGEST " + json.dumps(out))


def run_digest(lib_path):
    env = dict(os.environ)
    if lib_path:
        env["SR_PYGMM_LIB"] = lib_path
        env["SR_PYGMM_ALLOW_MISSING"] = NEW_SYMBOLS
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--digest"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST ")][0][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="0,1,2")
    ap.add_argument("--digest", action="store_true", help="(internal) print the single fit's digests with the loaded library")
    args = ap.parse_args()
    if args.digest:
        return digest()
    from speaker_recognition_amd import _lib
    doc = {"device": _lib.device_name(), "nr_iteration": 200, "threshold": 0.01, "map_fit_batch_bytes": _lib.map_fit_batch_bytes(), "cases": []}
    if args.parent_lib:
        mine, parent = run_digest(None), run_digest(os.path.abspath(args.parent_lib))
        doc["single_fit_vs_parent_library"] = {"this_build": mine, "parent": parent, "same_bits": mine == parent}
        assert mine == parent, "the single fit's models moved against the parent commit's library"
    for i in [int(v) for v in args.shapes.split(",") if v != ""]:
        doc["cases"].append(case(*SHAPES[i], args.reps))
        print(json.dumps(doc["cases"][-1]), flush=True)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
