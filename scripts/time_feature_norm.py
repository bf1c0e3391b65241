#!/usr/bin/env python3
"""What short-time feature normalisation on the device costs (csrc/featnorm.hip), in one run; one JSON line on stdout.

    python scripts/time_feature_norm.py [--out profiles/r25_feature_norm.json] [--oracle-utts 4]

Two shapes, window 301, 39 columns (13 cepstra with two delta orders, 25 ms frames every 10 ms at 16 kHz): 1000 utterances of 1000
frames (1 M frames) and 64 utterances of 300 frames.  The features are the MFCC stage's own output of synthetic voices, extracted
in the same run with the per-utterance CMVN off; that extraction is timed beside the normalisation of its frames.  For every mode:
  call_ms     host wall clock around Batch.normalise and a device synchronisation, median of 5 after a warm-up;
  device_ms   HIP events around the stage's launches (timer kind SR_T_CMVN), median of the same 5 calls;
  host_numpy  the numpy restatement (tests/featnorm_oracle.py) on the first --oracle-utts utterances, per utterance and
              extrapolated to the shape; the device's output of those utterances is checked against it within the tests' gates;
  rate        window comparisons per second (warp: one comparison = a value tested for < and for == and both counted, four
              vector instructions per lane) or float64 operations per second (cmn: one add per window value; cmvn: add, subtract,
              multiply, add), over device_ms, and the vector instructions per second they amount to beside the fp32 vector
              instruction rate of the MI355X (157.3 TFLOP/s = 78.6e12 lane instructions per second; no float64 vector rate is on record, so
              the float64 figures stand beside the same number and say so)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FS, W, ND = 16000, 301, 2
LANE_INSTR_PER_S = 157.3e12 / 2          # the fp32 vector peak counts a fused multiply-add as two


def voices(n_utt, frames, ex, n_voices=16):
    """n_utt int16 utterances that give `frames` feature rows each: n_voices synthetic voices, each utterance a rotation of one"""
    from speaker_recognition_amd import synth
    n = ex.FRAME_LEN
    while ex.num_frames(n) - ND < frames:
        n += ex.FRAME_SHIFT
    base = [synth.synth_speech(3 * v, n / FS + 0.1, FS)[:n] for v in range(n_voices)]
    rng = np.random.default_rng(25)
    return [np.roll(base[u % n_voices], int(rng.integers(0, n))) for u in range(n_utt)]


def timed(fn, kind, reps=5):
    """-> (median call ms, median device ms of timer `kind`, launches per call, last result)"""
    from speaker_recognition_amd import _lib
    fn()
    _lib.synchronize()
    call, dev, launches, res = [], [], 0, None
    for _ in range(reps):
        _lib.profile_reset()
        t0 = time.perf_counter()
        res = fn()
        _lib.synchronize()
        call.append((time.perf_counter() - t0) * 1e3)
        ms, launches = _lib.profile_get(kind)
        dev.append(ms)
    return float(np.median(call)), float(np.median(dev)), int(launches), res


def shape(n_utt, frames, n_oracle):
    import featnorm_oracle as fo
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch, MfccExtractor
    ex = MfccExtractor(FS, win_length_ms=25, win_shift_ms=10)
    pcm = Batch.from_pcm(voices(n_utt, frames, ex))
    mfcc_call, mfcc_dev, _, feats = timed(lambda: ex.extract_batch(pcm, nd=ND, cmvn=False), _lib.T_MFCC)
    off = feats.offsets()
    rows, dim = feats.n_rows, feats.dim
    frames = int(off[1])
    assert np.all(np.diff(off) == frames)
    X = feats.download()
    work = float(rows) * dim * min(W, frames)                   # window values visited
    out = {"utterances": n_utt, "frames_each": frames, "rows": int(rows), "dim": int(dim), "window": W,
           "plan": _lib.feature_norm_plan("warp", W, dim, frames, n_cu=0),
           "mfcc_same_frames": {"call_ms": mfcc_call, "device_ms_T_MFCC": mfcc_dev, "note": "nd=2, per-utterance CMVN off"}}
    for mode in ("warp", "cmn", "cmvn"):
        call, dev, launches, res = timed(lambda: feats.normalise(mode, W), _lib.T_CMVN)
        Y = res.download()
        t0 = time.perf_counter()
        want = [fo.normalise(X[off[u]:off[u + 1]], mode, W)[0] for u in range(n_oracle)]
        host_s = time.perf_counter() - t0
        worst = 0.0
        for u, w in enumerate(want):
            g = Y[off[u]:off[u + 1]].astype(np.float64)
            worst = max(worst, float(np.max(np.abs(g - w) / np.maximum(np.abs(w), 1.0))))
        gate = 2.0 ** -23
        ops = {"warp": 1, "cmn": 1, "cmvn": 4}[mode] * work
        instr = {"warp": 4, "cmn": 2, "cmvn": 7}[mode] * work   # cmn: convert, add; cmvn: + convert, subtract, multiply, add and the equality test
        m = {"call_ms": call, "device_ms": dev, "launches_per_call": launches,
             "host_numpy_utterances_timed": n_oracle, "host_numpy_ms_per_utterance": 1e3 * host_s / n_oracle,
             "host_numpy_ms_extrapolated": 1e3 * host_s / n_oracle * n_utt,
             "worst_relative_difference_on_timed_utterances": worst, "within_gate": bool(worst <= gate),
             ("window_comparisons_per_s" if mode == "warp" else "float64_operations_per_s"): ops / (dev * 1e-3) if dev > 0 else None,
             "lane_instructions_per_s_counted": instr / (dev * 1e-3) if dev > 0 else None,
             "share_of_fp32_vector_instruction_rate": instr / (dev * 1e-3) / LANE_INSTR_PER_S if dev > 0 else None}
        if mode != "warp":
            m["note"] = "float64 arithmetic beside the fp32 vector rate: no float64 vector peak is stated to compare with"
        out[mode] = m
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--oracle-utts", type=int, default=4)
    args = ap.parse_args()
    from speaker_recognition_amd import _lib
    _lib.profile_enable(True)
    out = {"device": _lib.device_name(), "timer": "SR_T_CMVN around the stage's launches; medians of 5 after a warm-up",
           "large_1000x1000x39": shape(1000, 1000, args.oracle_utts), "small_64x300x39": shape(64, 300, args.oracle_utts),
           "not_measured": "the 10 M frame headline shape; kernel-level counters (LDS and VALU utilisation)"}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
