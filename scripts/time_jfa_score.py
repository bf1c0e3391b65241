#!/usr/bin/env python3
"""What JFA trial scoring costs on the device (csrc/jfa_score.hip), in one run; one JSON line on stdout.

    python scripts/time_jfa_score.py [--out profiles/r16_jfa_score.json] [--host-segments 2] [--host-models 4] [--shapes a,b,c]

Three shapes (models x test segments): (a) 200 x 2000 against 512 x 39, Ry = 300, Ru = 100; (b) 1000 x 1000 against the reference's
own 256 x 13 JFA UBM (tests/golden/jfa_ubm.npz), Ry = 300, Ru = 100; (c) 20 x 64 against 512 x 39, Ry = 100, Ru = 50.  Statistics
from the generator of tests/jfa_cases.py (one session a segment), the factors as tests/jfa_score_cases.py draws them.  For each:
  * the whole call through jfa.score_trials in both modes: host wall clock, median of 3 after a warm-up -- it includes the copy of
    N, F, v, u, z, y to the device and of the score matrix back;
  * the device time of every stage of one call from the library's event timers (the SR_T_JFA_* kinds the stages are booked to), and
    the achieved float64 rate of the GEMM launches booked to each kind (2 M N K_red floating-point operations over the kind's
    device time) against the data sheet's 78.6 TFLOP/s; two products share a kind where the header says so, their operations are
    summed;
  * the share of the scoring kernel (Cholesky + one forward substitution over J + 1 columns + scores) and its rate;
  * in the same run the loop-for-loop numpy transliteration of kscore_famous_19.m on the host, timed on --host-segments segments
    x --host-models models and EXTRAPOLATED (marked so): its set-up once, its per-segment part x T, its per-pair part x T (J + 1);
    at (c) it runs over every pair and gives the parity ratios (difference / gate) of tests/test_gpu_jfa_score.py;
  * for linear mode jfa.linear_scoring of the same inputs on the host, whole, in the same run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_F64_TFLOPS = 78.6


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


def host_transliteration_parts(F, N, m, E, d, v, u, z, y, n_seg, n_mod):
    """kscore_famous_19.m's statements (tests/jfa_score_cases.kscore_m) on the first n_seg segments x (UBM + n_mod - 1 models), timed in
    its three parts.  Arguments in the .m file's column orientation.  -> seconds (set-up, per segment, per pair)."""
    dim = F.shape[0] // N.shape[0]
    n_mix = N.shape[0]
    t0 = time.perf_counter()
    index_map = np.repeat(np.arange(n_mix), dim)
    M = m[:, None] + z * d[:, None] + v @ y
    M = np.hstack([m[:, None], M])
    uEuT = [u[c * dim:(c + 1) * dim].T @ ((1.0 / E[c * dim:(c + 1) * dim])[:, None] * u[c * dim:(c + 1) * dim]) for c in range(n_mix)]
    setup = time.perf_counter() - t0
    seg = pair = 0.0
    for ii in range(n_seg):
        t0 = time.perf_counter()
        Nte = N[index_map, ii] / E
        Fte = F[:, ii] / E
        L = np.eye(u.shape[1])
        for c in range(n_mix):
            L = L + uEuT[c] * N[c, ii]
        cholLu = np.linalg.solve(np.linalg.cholesky(L), u.T)
        seg += time.perf_counter() - t0
        t0 = time.perf_counter()
        for jj in range(n_mod):
            MNe = Nte * M[:, jj]
            Fse = Fte - MNe
            lin = Fte @ M[:, jj]
            quad = MNe @ M[:, jj]
            quad2 = cholLu @ Fse
            quad2 = quad2 @ quad2
            _ = (lin - 0.5 * quad + 0.5 * quad2) / N[:, ii].sum()
        pair += time.perf_counter() - t0
    return setup, seg / n_seg, pair / (n_seg * n_mod)


def shape(name, J, T, K, D, Ry, Ru, ubm, n_seg, n_mod, full_host):
    import jfa_cases as jc
    import jfa_score_cases as sc
    from speaker_recognition_amd import _lib, jfa
    c = jc.corpus(T, K, D, min(Ry, 32), 5000 + T + J, sessions=1, ubm=ubm)
    F, N, m, E = c["F"], c["N"], c["m"], c["E"]
    kd, J1 = K * D, J + 1
    rng = np.random.default_rng(7 * T + J)
    v = rng.normal(0.0, 0.3, (Ry, kd))
    u = rng.normal(0.0, 0.3, (Ru, kd))
    y = rng.standard_normal((J, Ry))
    z = 0.1 * rng.standard_normal((J, kd))
    d = rng.uniform(0.1, 0.5, kd)
    x = 0.3 * rng.standard_normal((T, Ru))
    a = (F, N, m, E, d, v, u, z, y)
    out = {"shape": name, "models": J, "segments": T, "K": K, "D": D, "Ry": Ry, "Ru": Ru,
           "plan": {k: val for k, val in _lib.jfa_score_plan(T, J, K, D, Ry, Ru, "integrated", 1 << 30, 0, 0).items()}}
    out["integrated_call_ms"], got = median_ms(lambda: jfa.score_trials(*a))
    out["linear_call_ms"], got_lin = median_ms(lambda: jfa.score_trials(*a, x=x, mode="linear"))
    kinds = (("gram_scale_cross_synth", _lib.T_JFA_GRAM), ("gemm_L", _lib.T_JFA_GEMM_L), ("gemm_over_KD", _lib.T_JFA_GEMM_B),
             ("gemm_over_K", _lib.T_JFA_GEMM_A), ("gemm_models", _lib.T_JFA_GEMM_C), ("kscore", _lib.T_JFA_FACTOR))
    flops = {"integrated": {"gemm_L": 2.0 * T * K * Ru * Ru, "gemm_over_KD": 2.0 * T * kd * (Ru + J1), "gemm_over_K": 2.0 * T * K * (J1 + J1 * Ru),
                            "gemm_models": 2.0 * J * kd * Ry},
             "linear": {"gemm_over_KD": 2.0 * J * T * kd, "gemm_models": 2.0 * J * kd * Ry + 2.0 * T * kd * Ru}}
    for mode in ("integrated", "linear"):
        _lib.profile_enable(True)
        _lib.profile_reset()
        jfa.score_trials(*a, x=x, mode=mode)
        stages = {k: _lib.profile_get(kind) for k, kind in kinds}
        _lib.profile_enable(False)
        out[mode + "_device_stage_ms"] = {k: val[0] for k, val in stages.items()}
        out[mode + "_device_stage_launches"] = {k: int(val[1]) for k, val in stages.items()}
        out[mode + "_device_ms"] = float(sum(val[0] for val in stages.values()))
        out[mode + "_gemm_flop"] = flops[mode]
        rate = {k: f / (stages[k][0] * 1e-3) / 1e12 if stages[k][0] > 0 else None for k, f in flops[mode].items()}
        out[mode + "_gemm_tflops_f64"] = rate
        out[mode + "_gemm_share_of_peak"] = {k: (r / PEAK_F64_TFLOPS if r is not None else None) for k, r in rate.items()}
    ks_ms = out["integrated_device_stage_ms"]["kscore"]
    ks_flop = T * (Ru ** 3 / 3.0 + J1 * float(Ru) * Ru)
    out["kscore_share_of_device_time"] = ks_ms / out["integrated_device_ms"] if out["integrated_device_ms"] > 0 else None
    out["kscore_flop"] = ks_flop
    out["kscore_tflops_f64"] = ks_flop / (ks_ms * 1e-3) / 1e12 if ks_ms > 0 else None
    # the transliteration on the host
    n_seg, n_mod = (T, J1) if full_host else (min(n_seg, T), min(n_mod, J1))
    setup, per_seg, per_pair = host_transliteration_parts(F.T, N.T, m, E, d, v.T, u.T, z.T, y.T, n_seg, n_mod)
    out.update(host_numpy_segments_timed=n_seg, host_numpy_models_timed=n_mod, host_numpy_setup_ms=1e3 * setup,
               host_numpy_ms_per_segment=1e3 * per_seg, host_numpy_ms_per_pair=1e3 * per_pair,
               host_numpy_integrated_ms=1e3 * (setup + per_seg * T + per_pair * T * J1), host_numpy_extrapolated=not full_host)
    t0 = time.perf_counter()
    host_lin = jfa.linear_scoring(F, N, None, m, E, d, v, u, z, y, x)
    out["host_linear_scoring_ms"] = 1e3 * (time.perf_counter() - t0)
    _, mag = sc.linear_m(F, N, m, E, d, v, u, z, y, x)
    out["parity_linear_vs_host_over_gate"] = float(np.abs(got_lin - host_lin).max()) / sc.gate_linear((T, J, K, D, Ry, Ru), mag)
    if full_host:
        ref = sc.kscore_m(F.T, N.T, m, E, d, v.T, u.T, z.T, y.T)
        out["kappa_L"] = float(ref["kappa"].max())
        out["parity_integrated_over_gate"] = float(np.abs(got - ref["scores"]).max()) / sc.gate_integrated((T, J, K, D, Ry, Ru), ref)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--host-segments", type=int, default=2)
    ap.add_argument("--host-models", type=int, default=4)
    ap.add_argument("--shapes", default="a,b,c")
    args = ap.parse_args()
    import bw_cases as bc
    from speaker_recognition_amd import _lib
    want = args.shapes.split(",")
    shapes = []
    if "c" in want:
        shapes.append(shape("c_20x64_512x39_Ry100_Ru50", 20, 64, 512, 39, 100, 50, None, args.host_segments, args.host_models, True))
    if "a" in want:
        shapes.append(shape("a_200x2000_512x39_Ry300_Ru100", 200, 2000, 512, 39, 300, 100, None, args.host_segments, args.host_models, False))
    if "b" in want:
        ubm = bc.fixture_ubm()
        shapes.append(shape("b_1000x1000_fixture256x13_Ry300_Ru100", 1000, 1000, 256, 13, 300, 100, ubm, args.host_segments, args.host_models, False))
    out = {"device": _lib.device_name(), "peak_f64_tflops_data_sheet": PEAK_F64_TFLOPS, "shapes": shapes}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
