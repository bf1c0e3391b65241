#!/usr/bin/env python3
"""BASELINE configs[4] as one pipeline: the serving stream with the voice-activity front end on the device (ServingStream(vad=),
sr_stream_create_vad) against (a) the host chain bench.py:block_stream times (VAD.filter, the one-third rule, reset_pcm,
predict_batch: one window per call) and (b) the stream without the front end, in one run on one scene; one JSON line on stdout.

    python scripts/time_stream_vad.py [--out profiles/r08_stream_vad.json] [--reps 300]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/time_stream_vad.py --reps 50      # the per-kernel split

20 speakers x 256 mixtures x 13 MFCC (diagonal, the configs[4] shape) and 20 x 32 x 28 full-covariance (MFCC + LPC-15), 8 kHz, 1 s
windows at a 0.5 s step from bench.py's gated scene.  Host-observed submit -> collect latency, p50 / p99, for 1 and 1024 windows
per tick, plain and graph-replayed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FS = 8000


def pcts(a):
    a = np.asarray(a)
    return {"p50_ms": float(np.percentile(a, 50)), "p99_ms": float(np.percentile(a, 99))}


def time_stream(st, ticks, reps, warm=30):
    lat = []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        st.submit(ticks[i % len(ticks)])
        st.collect()
        lat.append((time.perf_counter() - t0) * 1e3)
    return pcts(lat[warm:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=300)
    args = ap.parse_args()
    from speaker_recognition_amd import skgmm, synth
    from speaker_recognition_amd.core import Batch, MfccExtractor, ModelSet, ServingStream
    from speaker_recognition_amd.filters import VAD
    from speaker_recognition_amd.pygmm import GMM
    ex = MfccExtractor(FS)
    diag = ModelSet([GMM.from_arrays(*synth.synth_gmm(256, 13, 7 + s)) for s in range(20)])
    audio = synth.synth_speech(3, 40.0, FS)
    rng = np.random.default_rng(5)
    floor = rng.normal(0, 60, len(audio)).astype(np.int16)
    gate = (np.arange(len(audio)) // (FS * 3 // 2)) % 2 == 0
    scene = (np.where(gate, audio // 2, 0) + floor).astype(np.int16)
    vad = VAD()
    vad.init_noise(FS, rng.normal(0, 60, 3 * FS).astype(np.int16))
    chunks = [scene[i * FS // 2:i * FS // 2 + FS] for i in range(70)]
    exl = MfccExtractor(FS, n_lpc=15)
    X = np.concatenate([exl.extract(synth.synth_speech(9 * s, 2.0, FS, seed=500 + s)) for s in range(8)])
    cov0 = np.cov(X.T) + 1e-3 * np.eye(X.shape[1])
    cov = 0.5 * cov0 + 0.05 * np.diag(np.diag(cov0))
    full = skgmm.FullSet([skgmm.GMM.from_arrays(np.full(32, 1 / 32), X[rng.choice(len(X), 32, replace=False)], np.repeat(cov[None], 32, axis=0))
                          for _ in range(20)])
    out = {"workload": "8 kHz, 1 s windows at a 0.5 s step of bench.py's gated scene; host-observed submit -> collect, %d ticks" % args.reps}

    def host_chain(e, score):
        vwin = Batch.from_pcm([scene[:FS]])
        lat = []
        for i in range(30 + args.reps):
            chunk = chunks[i % 70]
            t0 = time.perf_counter()
            voiced, _ = vad.filter(FS, chunk)
            if len(voiced) > len(chunk) / 3 and e.num_frames(len(voiced)) > 0:
                vwin.reset_pcm([voiced])
                score(vwin)
            lat.append((time.perf_counter() - t0) * 1e3)
        return pcts(lat[30:])

    for name, e, models, score in (("diag_20x256x13", ex, diag, lambda b: ex.predict_batch(diag, b, nd=0)),
                                   ("full_20x32x28", exl, full, lambda b: full.predict_pcm(exl, b))):
        r = {"host_chain_one_window": host_chain(e, score)}
        for n_win in (1, 1024):
            ticks = [np.stack([chunks[(t * 7 + j) % 70] for j in range(n_win)]) for t in range(10 if n_win == 1 else 3)]
            reps = args.reps if n_win == 1 else max(10, args.reps // 10)
            for graph in (False, True):
                key = "%d_window%s_%s" % (n_win, "" if n_win == 1 else "s", "graph" if graph else "plain")
                r["vad_stream_" + key] = time_stream(ServingStream(e, models, n_win, FS, graph=graph, vad=vad), ticks, reps)
                r["stream_without_vad_" + key] = time_stream(ServingStream(e, models, n_win, FS, graph=graph), ticks, reps)
        r["vad_stream_faster_than_host_chain_p50"] = r["vad_stream_1_window_plain"]["p50_ms"] < r["host_chain_one_window"]["p50_ms"]
        out[name] = r
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
