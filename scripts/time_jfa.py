#!/usr/bin/env python3
"""What the JFA factor estimation costs on the device (csrc/jfa.hip), in one run; one JSON line on stdout.

    python scripts/time_jfa.py [--out profiles/r14_jfa.json] [--host-groups 8] [--shapes a,b,c]

Three shapes: (a) 200 speakers x (512 x 39), R = 100; (b) the same statistics, R = 300; (c) 1000 sessions x the reference's
256 x 13 JFA UBM (tests/golden/jfa_ubm.npz), R = 300.  Statistics from the generator of tests/jfa_cases.py (one session a group),
the loading matrix from the sc_* scripts' random start.  For each:
  * one factors (with accumulators) + update iteration through jfa.FactorEstimator / jfa.update_loadings: host wall clock, which
    includes the copies of W, y, A and C between host and device (A alone is 8 K R^2 bytes),
  * a 10-iteration FactorEstimator.train: one device call, W and y cross once,
  * the device time of every stage of one train iteration from the library's event timers (SR_T_JFA_*), and the achieved float64
    rate of each of the four GEMM launches (2 M N K_red floating-point operations over its device time),
  * in the same run the float64 numpy restatement (tests/jfa_cases.py) of the same iteration on the host: the factors pass over
    the first --host-groups groups (the gram matrices once, plus its time per group times the group count: marked extrapolated
    unless every group was timed) and the whole update,
and at (a), where the restatement runs over every group, the parity figures of tests/test_gpu_jfa.py as difference / gate.
Wall-clock figures are medians of 3 after a warm-up, around a device synchronisation."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def shape(name, G, K, D, R, ubm, n_host, full_host):
    import jfa_cases as jc
    from speaker_recognition_amd import _lib, jfa
    c = jc.corpus(G, K, D, min(R, 32), 4000 + G + R, sessions=1, ubm=ubm)
    N, E = c["N"], c["E"]
    Fc = c["F"] - c["m"] * np.repeat(N, D, axis=1)
    W0 = jc.random_start(R, E, 1)
    kd = K * D
    out = {"shape": name, "groups": G, "K": K, "D": D, "R": R, "plan": _lib.jfa_plan(G, K, D, R, 1 << 30, 0, 0)}
    with jfa.FactorEstimator(N, Fc, E) as est:
        def iteration():
            y, A, C = est.factors(W0, accumulate=True)
            return y, A, C, jfa.update_loadings(A, C, W0)
        out["factors_update_call_ms"], (y, A, C, W1) = median_ms(iteration)
        out["train_10_call_ms"], _ = median_ms(lambda: est.train(W0, 10), reps=1)
        _lib.profile_enable(True)
        _lib.profile_reset()
        est.train(W0, 1)
        kinds = (("gram", _lib.T_JFA_GRAM), ("gemm_L", _lib.T_JFA_GEMM_L), ("gemm_b", _lib.T_JFA_GEMM_B), ("gemm_A", _lib.T_JFA_GEMM_A),
                 ("gemm_C", _lib.T_JFA_GEMM_C), ("factor", _lib.T_JFA_FACTOR), ("update", _lib.T_JFA_UPDATE))
        stages = {k: _lib.profile_get(kind) for k, kind in kinds}
        _lib.profile_enable(False)
    out["device_stage_ms"] = {k: v[0] for k, v in stages.items()}
    out["device_stage_launches"] = {k: int(v[1]) for k, v in stages.items()}
    out["device_iteration_ms"] = float(sum(v[0] for v in stages.values()))
    flops = {"gemm_L": 2.0 * G * K * R * R, "gemm_b": 2.0 * G * R * kd, "gemm_A": 2.0 * K * G * R * R, "gemm_C": 2.0 * R * G * kd}
    out["gemm_flop"] = flops
    out["gemm_tflops_f64"] = {k: flops[k] / (stages[k][0] * 1e-3) / 1e12 if stages[k][0] > 0 else None for k in flops}
    # the restatement on the host
    n_host = G if full_host else min(n_host, G)
    t0 = time.perf_counter()
    jc.grams(E, W0, K)
    host_gram_s = time.perf_counter() - t0                              # (once per iteration, whatever the number of groups)
    t0 = time.perf_counter()
    yr, Ar, Cr = jc.factors(N[:n_host], Fc[:n_host], E, W0)
    host_groups_s = max(time.perf_counter() - t0 - host_gram_s, 0.0)
    host_factors_s = host_gram_s + host_groups_s / n_host * G
    t0 = time.perf_counter()
    Wr, _ = jc.update(A if n_host < G else Ar, C if n_host < G else Cr, W0)
    host_update_s = time.perf_counter() - t0
    out.update(host_numpy_groups_timed=n_host, host_numpy_gram_ms=1e3 * host_gram_s, host_numpy_factors_ms_per_group=1e3 * host_groups_s / n_host,
               host_numpy_factors_ms=1e3 * host_factors_s, host_numpy_extrapolated=bool(n_host < G),
               host_numpy_update_ms=1e3 * host_update_s, host_numpy_iteration_ms=1e3 * (host_factors_s + host_update_s))
    kL = jc.cond_L(N[:n_host], E, W0)
    out["parity_y_first_groups_over_gate"] = jc.rel(y[:n_host], yr) / jc.gate_y(R, K, D, kL)
    out["kappa_L_first_groups"] = kL
    if n_host == G:
        kA = jc.cond_A(Ar)
        gy = jc.gate_y(R, K, D, kL)
        out["kappa_A"] = kA
        out["parity_over_gate"] = {"y": jc.rel(y, yr) / gy, "A": jc.rel(A, Ar) / (4 * gy), "C": jc.rel(C, Cr) / (4 * gy),
                                   "update": jc.rel(jfa.update_loadings(Ar, Cr, W0), Wr) / jc.gate_update(R, kA),
                                   "step_W": jc.rel(W1, Wr) / jc.gate_step(R, K, D, kL, kA)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--host-groups", type=int, default=8)
    ap.add_argument("--shapes", default="a,b,c")
    args = ap.parse_args()
    import bw_cases as bc
    from speaker_recognition_amd import _lib
    want = args.shapes.split(",")
    shapes = []
    if "a" in want:
        shapes.append(shape("a_200x512x39_R100", 200, 512, 39, 100, None, args.host_groups, True))
    if "b" in want:
        shapes.append(shape("b_200x512x39_R300", 200, 512, 39, 300, None, args.host_groups, False))
    if "c" in want:
        shapes.append(shape("c_1000xfixture256x13_R300", 1000, 256, 13, 300, bc.fixture_ubm(), args.host_groups, False))
    out = {"device": _lib.device_name(), "shapes": shapes}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
