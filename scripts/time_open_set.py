#!/usr/bin/env python3
"""What the open-set decision on the device costs (csrc/open_set.hip), in one run; one JSON line on stdout.

    python scripts/time_open_set.py [--out profiles/r10_open_set.json] [--reps 300] [--parent-lib <pygmm.so of the parent commit>]

(a) 64 utterances x 300 frames against the headline set (a 512-mixture UBM + 200 MAP speakers, 39 dims): the reference-shaped
    loop GMMSet.predict_with_reject (per utterance: the set, then the UBM, decided on the host) against
    GMMSet.predict_with_reject_batch (one pass, decided on the device); medians of 5 after a warm-up, labels checked equal.
(b) BASELINE configs[4]'s shape (20 speakers x 256 mixtures x 13 MFCC, one 1 s window of 8 kHz audio per tick): host-observed
    submit -> collect p50 of a stream with and without open_set=, the two streams alive in the same process and ticked in turn;
    plain, graph-replayed and voice-activity sessions.  --parent-lib runs the closed-set half once more in a child process on
    another build of the library (SR_PYGMM_LIB), in the same session."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FS = 8000
OPEN_SET_CALLS = ("sr_open_set_decide", "sr_score_batch_set_open", "sr_predict_pcm_batch_open", "sr_stream_set_open",
                  "sr_stream_collect_open", "sr_multi_predict_pcm_open")


def pcts(a):
    a = np.asarray(a)
    return {"p50_ms": float(np.percentile(a, 50)), "p25_ms": float(np.percentile(a, 25)), "p75_ms": float(np.percentile(a, 75)),
            "p99_ms": float(np.percentile(a, 99))}


def stream_scene():
    from speaker_recognition_amd import synth
    from speaker_recognition_amd.filters import VAD
    audio = synth.synth_speech(3, 40.0, FS)
    rng = np.random.default_rng(5)
    floor = rng.normal(0, 60, len(audio)).astype(np.int16)
    gate = (np.arange(len(audio)) // (FS * 3 // 2)) % 2 == 0
    scene = (np.where(gate, audio // 2, 0) + floor).astype(np.int16)
    vad = VAD()
    vad.init_noise(FS, rng.normal(0, 60, 3 * FS).astype(np.int16))
    return [scene[i * FS // 2:i * FS // 2 + FS][None] for i in range(70)], vad


def time_streams(reps, with_open, warm=30):
    """{mode: {closed: ..., open: ...}}: the streams of a mode are ticked in turn, one tick each, on the same PCM"""
    from speaker_recognition_amd import synth
    from speaker_recognition_amd.core import MfccExtractor, ModelSet, ServingStream
    from speaker_recognition_amd.pygmm import GMM
    ex = MfccExtractor(FS)
    ms = ModelSet([GMM.from_arrays(*synth.synth_gmm(256, 13, 7 + s)) for s in range(20)])
    ticks, vad = stream_scene()
    out = {}
    for mode, kw in (("plain", {}), ("graph", dict(graph=True)), ("vad", dict(vad=vad)), ("vad_graph", dict(vad=vad, graph=True))):
        streams = {"closed": ServingStream(ex, ms, 1, FS, **kw)}
        if with_open:
            streams["open"] = ServingStream(ex, ms, 1, FS, open_set=(0, 0.0), **kw)
        lat = {k: [] for k in streams}
        for i in range(warm + reps):
            for k, st in streams.items():
                t0 = time.perf_counter()
                st.submit(ticks[i % len(ticks)])
                st.collect_open() if k == "open" else st.collect()
                lat[k].append((time.perf_counter() - t0) * 1e3)
        out[mode] = {k: pcts(v[warm:]) for k, v in lat.items()}
        if with_open:
            c, o = out[mode]["closed"], out[mode]["open"]
            out[mode]["open_minus_closed_p50_us"] = 1e3 * (o["p50_ms"] - c["p50_ms"])
            out[mode]["closed_p25_to_p75_us"] = 1e3 * (c["p75_ms"] - c["p25_ms"])
    return out


def time_batch():
    from speaker_recognition_amd import synth
    from speaker_recognition_amd.gmmset import GMMSet
    from speaker_recognition_amd.pygmm import GMM
    ubm = synth.synth_gmm(512, 39, 99)
    spk = [synth.synth_map_speaker(ubm, 500 + s) for s in range(200)]
    gs = GMMSet(ubm=GMM.from_arrays(*ubm), reject_threshold=1.5)
    for s, m in enumerate(spk):
        gs._append("spk%d" % s, GMM.from_arrays(*m))
    utts = [synth.draw_frames(spk[u % 200] if u % 2 == 0 else synth.synth_gmm(512, 39, 9000 + u), 300, 700 + u) for u in range(64)]
    utts = [u.astype(np.float64) for u in utts]             # both sides are handed the same arrays

    def med(fn, arg):
        fn(arg)
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            res = fn(arg)
            t.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(t)), res
    loop_ms, loop = med(gs.predict_with_reject, utts)
    batch_ms, batch = med(gs.predict_with_reject_batch, utts)
    return {"workload": "64 utterances x 300 frames (float64 arrays on both sides), 201 models x 512 mixtures x 39 dims, threshold 1.5",
            "loop_ms": loop_ms,
            "batch_ms": batch_ms, "labels_equal": loop == batch, "accepted": sum(x is not None for x in batch),
            "rejected": sum(x is None for x in batch)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--closed-only", action="store_true", help="(the child of --parent-lib: the closed-set streams alone)")
    args = ap.parse_args()
    if args.closed_only:
        print(json.dumps(time_streams(args.reps, False)))
        return
    from speaker_recognition_amd import _lib
    out = {"device": _lib.device_name(), "reps": args.reps, "reject_batch": time_batch(),
           "stream_one_window_20x256x13": time_streams(args.reps, True)}
    if args.parent_lib:
        # (the parent's build has none of the open-set calls, and its closed-set half uses none)
        env = dict(os.environ, SR_PYGMM_LIB=os.path.abspath(args.parent_lib), SR_PYGMM_ALLOW_MISSING=",".join(OPEN_SET_CALLS))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--closed-only", "--reps", str(args.reps)], env=env,
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit("the parent library's run failed:\n" + r.stderr[-2000:])
        out["stream_parent_commit_library"] = json.loads(r.stdout.strip().splitlines()[-1])
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
