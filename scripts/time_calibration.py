#!/usr/bin/env python3
"""What score calibration costs on the device (csrc/calib.hip), in one run; one JSON line on stdout.

    python scripts/time_calibration.py [--out profiles/r24_calibration.json] [--shapes a,b]

Two trial lists: (a) 200 x 2000 = 4e5 trials, (b) 1000 x 100 000 = 1e8 trials; S = 1 and S = 3 systems; every 7th trial a target
around +1, the others non-targets around -1, unit noise; P = 0.01.  For each:
  * the whole call of Calibrator.fit and of cllr: host wall clock, median of 3 after a warm-up -- it includes the host's check of
    the labels and scores, the copy of the scores to the device and the state back;
  * the device time of every stage of one call from the library's event timers (the SR_T_JFA_* kinds the stages are booked to:
    SR_T_JFA_GEMM_A the pass kernel, SR_T_JFA_FACTOR the step kernel), the passes taken, the time per pass and the bytes per
    second a pass achieves over its 8 S + 1 bytes per trial;
  * the share of the call that is not device time (the host's check and the copy of the scores up), and the whole call of one
    evaluation (check + copy + one pass) next to it;
  * in the same run the numpy restatement's fit and Cllr on the host (tests/calib_cases.py); at more than 4e6 trials on the first
    4e6 trials, its time per pass scaled by n / 4e6 and multiplied by the device's pass count (stated in the record);
  * the largest difference between the two Cllr values (at more than 4e6 trials: on that subset)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HOST_SUBSET = 4_000_000
EXPECTED_PASS_MS_1E8_S1 = 0.2          # stated before the run: 9 bytes a trial at the 5.8 TB/s of jfa_stats's streaming kernel


def median_ms(fn, reps=3):
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


def shape(name, J, T, S, P=0.01):
    import calib_cases as cc
    from speaker_recognition_amd import _lib, calibration as cal
    n = J * T
    rng = np.random.default_rng(J + T + S)
    lab = (np.arange(n) % 7 == 0).astype(np.int8)
    X = np.empty((S, n))
    for s in range(S):
        X[s] = rng.standard_normal(n)
        X[s] += np.where(lab > 0, 1.0 + s / 4, -1.0 - s / 4)
    out = {"shape": name, "models": J, "segments": T, "trials": n, "systems": S, "prior": P, "plan": _lib.calib_plan(S, n, 0, "train", 0, 0)}
    kinds = (("pass", _lib.T_JFA_GEMM_A), ("step", _lib.T_JFA_FACTOR))

    def staged(fn):
        _lib.profile_enable(True)
        _lib.profile_reset()
        res = fn()
        st = {k: _lib.profile_get(kind) for k, kind in kinds}
        _lib.profile_enable(False)
        return res, st

    fit = lambda: cal.Calibrator(prior=P).fit(X, lab)          # noqa: E731
    m = {}
    m["call_ms"], c = median_ms(fit)
    c, st = staged(fit)
    m.update(stop=c.stop, passes=c.passes, halvings=c.halvings, objective=c.objective, theta=c.theta.tolist())
    m["device_stage_ms"] = {k: v[0] for k, v in st.items()}
    m["device_stage_launches"] = {k: int(v[1]) for k, v in st.items()}
    m["device_ms"] = float(sum(v[0] for v in st.values()))
    # (launches past the stop return at once: the pass kernel's time is that of the passes made, to a few microseconds)
    m["pass_ms"] = st["pass"][0] / c.passes
    m["step_ms"] = st["step"][0] / c.passes
    m["pass_bytes_per_s"] = (8 * S + 1) * n / (m["pass_ms"] * 1e-3)
    m["share_not_device"] = 1.0 - m["device_ms"] / m["call_ms"]
    m["eval_call_ms"], _ = median_ms(lambda: cal.evaluate(X, lab, c.theta, prior=P))
    out["fit"] = m
    # the host: the numpy restatement
    k = min(n, HOST_SUBSET)
    Xh, lh = X[:, :k], lab[:k]
    t0 = time.perf_counter()
    cc.evaluate(Xh, lh, c.theta, P, 0.0)
    pass_host = (time.perf_counter() - t0) * 1e3
    h = {"subset_trials": k, "pass_ms_on_subset": pass_host, "pass_ms": pass_host * n / k}
    if k == n:
        t0 = time.perf_counter()
        r = cc.fit(X, lab, P)
        h.update(fit_ms=(time.perf_counter() - t0) * 1e3, passes=r["passes"], stop=r["stop"], extrapolated=False)
    else:
        h.update(fit_ms=h["pass_ms"] * c.passes, passes=c.passes, extrapolated=True)
    out["host_numpy_fit"] = h
    if S == 1:
        q = {}
        llr = c.transform(X)
        q["call_ms"], got = median_ms(lambda: cal.cllr(llr, lab))
        (_, st) = staged(lambda: cal.cllr(llr, lab))
        q["device_ms"] = float(sum(v[0] for v in st.values()))
        q["pass_ms"] = st["pass"][0]
        q["pass_bytes_per_s"] = 9 * n / (q["pass_ms"] * 1e-3)
        q["cllr"] = got
        t0 = time.perf_counter()
        host = cc.cllr(llr[:k], lh)
        q["host_numpy_ms_on_subset"] = (time.perf_counter() - t0) * 1e3
        q["host_numpy_ms"] = q["host_numpy_ms_on_subset"] * n / k
        q["host_extrapolated"] = k != n
        q["max_abs_difference_to_host_numpy"] = abs((got if k == n else cal.cllr(llr[:k], lh)) - host)
        q["min_cllr_host"] = cal.min_cllr(llr[:k], lh)
        q["act_dcf"] = cal.act_dcf(llr, lab, P)
        out["cllr"] = q
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--shapes", default="a,b")
    args = ap.parse_args()
    from speaker_recognition_amd import _lib
    want = args.shapes.split(",")
    shapes = []
    for key, name, J, T in (("a", "a_200x2000", 200, 2000), ("b", "b_1000x100000", 1000, 100000)):
        if key in want:
            for S in (1, 3):
                shapes.append(shape("%s_S%d" % (name, S), J, T, S))
    out = {"device": _lib.device_name(), "expected_pass_ms_at_1e8_S1": EXPECTED_PASS_MS_1E8_S1, "host_subset_trials": HOST_SUBSET,
           "shapes": shapes}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
