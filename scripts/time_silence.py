#!/usr/bin/env python3
"""What the silence removal on the device costs (csrc/silence.hip), in one run; one JSON line on stdout.

    python scripts/time_silence.py [--out profiles/r11_silence.json] [--utts 1000] [--oracle-utts 1000]

(a) Batch.remove_silence on --utts synthetic utterances of 30 s at 16 kHz (synth.py voices, gated on and off over a noise floor
    so that there is silence to remove), upload excluded, against the numpy restatement of the reference
    (tests/silence_oracle.py) looped on the host over the first --oracle-utts of them in the same run (its time per utterance
    times --utts is the extrapolated figure); the device's output of those utterances is checked bit for bit.
(b) One 1-hour recording against 64 recordings of the same total length, at 16 kHz (g = S) and at 22050 Hz (g = 1): whether the
    walk scales with blocks and not with frames.
(c) predict_batch on a raw batch against remove_silence followed by predict_batch on its result (20 models x 64 mixtures x 39
    dims, two delta orders), with the frame counts before and after.
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
FS = 16000


def gated_voices(n_utt, seconds, fs, n_voices=16):
    """n_utt utterances: one of n_voices synthetic voices each, switched on and off in stretches of 0.2 .. 1.5 s over a floor"""
    from speaker_recognition_amd import synth
    voices = [synth.synth_speech(3 * v, seconds, fs) for v in range(n_voices)]
    n = len(voices[0])
    floor = np.random.default_rng(9).integers(-40, 41, 2 * n, dtype=np.int16)
    out = []
    for u in range(n_utt):
        rng = np.random.default_rng(10_000 + u)
        runs = (rng.uniform(0.2, 1.5, int(seconds / 0.2) + 2) * fs).astype(np.int64)
        on = np.repeat((np.arange(len(runs)) + u) % 2 == 0, runs)[:n]
        start = int(rng.integers(0, n))
        out.append(np.where(on, voices[u % n_voices], floor[start:start + n]))
    return out


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


def part_a(sigs, n_oracle):
    import silence_oracle as so
    from speaker_recognition_amd.core import Batch
    b = Batch.from_pcm(sigs)
    ms, out = median_ms(lambda: b.remove_silence(FS))
    off = out.offsets()
    cat = out.download_pcm()
    t0 = time.perf_counter()
    want = [so.remove_silence(FS, x) for x in sigs[:n_oracle]]
    host_s = time.perf_counter() - t0
    equal = all(np.array_equal(cat[off[u]:off[u + 1]], w) for u, w in enumerate(want))
    n_in = int(sum(len(x) for x in sigs))
    return {"utterances": len(sigs), "seconds_each": len(sigs[0]) / FS, "samples_in": n_in, "samples_kept": int(off[-1]),
            "device_ms": ms, "device_gsamples_per_s": n_in / ms / 1e6,
            "host_numpy_utterances_timed": n_oracle, "host_numpy_ms_per_utterance": 1e3 * host_s / max(1, n_oracle),
            "host_numpy_ms_extrapolated": 1e3 * host_s / max(1, n_oracle) * len(sigs),
            "device_equals_host_on_timed_utterances": bool(equal)}, out


def part_b(fs):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    piece = gated_voices(64, 3600.0 / 64, fs, n_voices=4)
    long_one = np.concatenate(piece)
    plan = _lib.silence_plan(fs, max_samples=len(long_one))
    one, many = Batch.from_pcm([long_one]), Batch.from_pcm(piece)
    ms_one, out_one = median_ms(lambda: one.remove_silence(fs))
    ms_many, out_many = median_ms(lambda: many.remove_silence(fs))
    return {"fs": fs, "samples": int(len(long_one)), "g": plan["g"], "E": plan["E"], "B": plan["B"], "blocks_of_the_hour": plan["blocks"],
            "one_recording_ms": ms_one, "sixty_four_recordings_ms": ms_many, "one_over_sixty_four": ms_one / ms_many,
            "kept_one": out_one.n_rows, "kept_sixty_four": out_many.n_rows}


def part_c(sigs):
    from speaker_recognition_amd import synth
    from speaker_recognition_amd.core import Batch, MfccExtractor, ModelSet
    from speaker_recognition_amd.pygmm import GMM
    ex = MfccExtractor(FS)
    ms = ModelSet([GMM.from_arrays(*synth.synth_gmm(64, 39, 7 + s)) for s in range(20)])
    raw = Batch.from_pcm(sigs)
    t_raw, _ = median_ms(lambda: ex.predict_batch(ms, raw, nd=2))
    t_both, _ = median_ms(lambda: ex.predict_batch(ms, raw.remove_silence(FS), nd=2))
    t_rm, kept = median_ms(lambda: raw.remove_silence(FS))
    frames = lambda b: int(sum(ex.num_frames(int(n)) for n in np.diff(b.offsets())))     # noqa: E731
    return {"utterances": len(sigs), "models": "20 x 64 mixtures x 39 dims, nd = 2", "predict_raw_ms": t_raw,
            "remove_then_predict_ms": t_both, "remove_alone_ms": t_rm, "frames_raw": frames(raw), "frames_after_removal": frames(kept)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--utts", type=int, default=1000)
    ap.add_argument("--oracle-utts", type=int, default=1000)
    args = ap.parse_args()
    from speaker_recognition_amd import _lib
    sigs = gated_voices(args.utts, 30.0, FS)
    a, _ = part_a(sigs, min(args.oracle_utts, args.utts))
    out = {"device": _lib.device_name(), "a_batched_30s_16k": a, "b_one_hour": [part_b(16000), part_b(22050)],
           "c_predict": part_c(sigs[:min(200, args.utts)])}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
