#!/usr/bin/env python3
"""What top-C Gaussian selection (csrc/gmm_topc.hip) costs and gives up against the exact pass of the same build, in one run; one
JSON line on stdout.

    python scripts/time_topc.py [--out profiles/r12_topc.json] [--top-c 5] [--frames 1000000]

The headline set (a 512-mixture UBM + 200 MAP speakers, 39 dims; the bench's synthetic data: speaker_recognition_amd.synth) at
(a) `--frames` frames in 10 utterances and (b) 64 utterances x 300 frames: host-observed medians of 5 calls after a warm-up of
ModelSet.score and ModelSet.score_topc on a resident feature batch, the device time of each of the four stages (HIP events on the
library's stream, one profiled call), argmax agreement, and the mean and max per-frame |LL_topc - LL_exact| (at (a) on the first
100 000 frames: the per-frame values of all 201 models travel to the host for it)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(fn, n=5):
    fn()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        res = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), res


def stage_times(fn):
    from speaker_recognition_amd import _lib
    _lib.profile_enable(True)
    _lib.profile_reset()
    fn()
    out = {}
    for name, kind in (("select_ms", _lib.T_TOPC_SELECT), ("route_ms", _lib.T_TOPC_ROUTE), ("evaluate_ms", _lib.T_TOPC_EVAL),
                       ("combine_ms", _lib.T_TOPC_COMBINE), ("finalize_ms", _lib.T_FINALIZE), ("exact_score_ms", _lib.T_SCORE)):
        ms, launches = _lib.profile_get(kind)
        out[name] = ms
        out[name.replace("_ms", "_launches")] = launches
    _lib.profile_enable(False)
    return out


def one_shape(ms, models, lengths, top_c, ll_frames):
    from speaker_recognition_amd import _lib, synth
    from speaker_recognition_amd.core import Batch
    utts = [synth.draw_frames(models[1 + u % (len(models) - 1)], n, 700 + u) for u, n in enumerate(lengths)]
    feats = Batch.from_features(utts)
    n = int(sum(lengths))
    exact_ms, (e_sums, e_arg) = med(lambda: ms.score(feats))
    topc_ms, (t_sums, t_arg) = med(lambda: ms.score_topc(feats, 0, top_c))
    out = {"utterances": len(lengths), "frames": n, "exact_ms": exact_ms, "exact_kernel": _lib.last_score_kernel(), "topc_ms": topc_ms,
           "exact_over_topc": exact_ms / topc_ms, "plan": _lib.topc_plan(512, 39, len(models), top_c, n, n_cu=0)}
    out["topc_stages"] = stage_times(lambda: ms.score_topc(feats, 0, top_c))
    out["exact_stages"] = {k: v for k, v in stage_times(lambda: ms.score(feats)).items() if k.startswith(("exact", "finalize"))}
    spk_t, spk_e = np.argmax(t_sums[:, 1:], axis=1), np.argmax(e_sums[:, 1:], axis=1)
    out["argmax_agreement"] = float(np.mean(t_arg == e_arg))
    out["speaker_argmax_agreement"] = float(np.mean(spk_t == spk_e))
    out["mean_abs_dsum_per_frame"] = float(np.mean(np.abs(t_sums - e_sums) / np.maximum(1, np.array(lengths))[:, None]))
    # per-frame values of a prefix of whole utterances
    k, acc = 0, 0
    while k < len(lengths) and acc + lengths[k] <= ll_frames:
        acc += lengths[k]
        k += 1
    sub = Batch.from_features(utts[:max(1, k)])
    e_fll = ms.score(sub, frame_ll=True)[2].astype(np.float64)
    t_fll = ms.score_topc(sub, 0, top_c, frame_ll=True)[2].astype(np.float64)
    d = np.abs(t_fll - e_fll)
    out["per_frame"] = {"frames": int(e_fll.shape[1]), "mean_abs_dll": float(d.mean()), "max_abs_dll": float(d.max()),
                        "mean_abs_dll_speakers": float(d[1:].mean()), "max_abs_dll_background": float(d[0].max()),
                        "topc_never_above_exact_by": float(np.max(t_fll - e_fll))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--top-c", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1_000_000)
    args = ap.parse_args()
    from speaker_recognition_amd import _lib, synth
    from speaker_recognition_amd.core import ModelSet
    from speaker_recognition_amd.pygmm import GMM
    ubm = synth.synth_gmm(512, 39, 99)
    models = [ubm] + [synth.synth_map_speaker(ubm, 500 + s) for s in range(200)]
    ms = ModelSet([GMM.from_arrays(*m) for m in models])
    out = {"device": _lib.device_name(), "set": "UBM 512 x 39 + 200 MAP speakers (201 models), background column 0", "top_c": args.top_c,
           "large": one_shape(ms, models, [args.frames // 10] * 10, args.top_c, 100_000),
           "serving_64x300": one_shape(ms, models, [300] * 64, args.top_c, 64 * 300)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
