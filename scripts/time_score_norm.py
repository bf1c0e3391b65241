#!/usr/bin/env python3
"""What score normalisation costs on the device (csrc/score_norm.hip), in one run; one JSON line on stdout.

    python scripts/time_score_norm.py [--out profiles/r21_score_norm.json] [--shapes a,b]

Two shapes (models x test segments, one cohort of C members on both sides, top-N): (a) 200 x 2000, C = 2000, N = 200; (b) 1000 x 1000,
C = 1000, N = 100.  Impostor scores N(0, 1), every 7th trial a target at +3, cohort scores N(0, 1) with a per-member bias.  For
every mode (z, t, zt, s, as1, as2):
  * the whole call through scorenorm.normalise: host wall clock, median of 3 after a warm-up -- it includes the copy of S and the
    cohort matrices to the device and of the result back;
  * the device time of every stage of one call from the library's event timers (the SR_T_JFA_* kinds the stages are booked to:
    selection, shifted copies, the two pairs of products, apply);
  * for as2 the float64 rate of the four products (2 J T C operations each) over the device time of their two kinds, against the
    data sheet's 78.6 TFLOP/s;
  * in the same run the same normalisation in vectorised numpy on the host (means and standard deviations along an axis;
    np.partition for as1 and for as2's selections, whose moments are the four shifted products), and the largest difference
    between the two."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def top_moments(M, n, axis):
    top = -np.partition(-M, n - 1, axis=axis)
    top = top[:, :n] if axis == 1 else top[:n]
    return top.mean(axis=axis, keepdims=True), top.std(axis=axis, keepdims=True)


MODES = ("z", "t", "zt", "s", "as1", "as2")


def select_rows(M, n):
    """The 0/1 selection of the n largest values of every row of M: everything above the n-th largest, then the first of its equals."""
    Cn = M.shape[1]
    sel = np.zeros_like(M)
    for r, row in enumerate(M):
        thr = np.partition(row, Cn - n)[Cn - n]
        above = row > thr
        sel[r, above] = 1.0
        sel[r, np.flatnonzero(row == thr)[:n - int(above.sum())]] = 1.0
    return sel


def as2_products(S, Ez, Tt, n):
    """as2 as the device forms it: four products over 0/1 selections, the operands shifted by the full row's / column's mean."""
    SelE, SelT = select_rows(Ez, n), select_rows(np.ascontiguousarray(Tt.T), n)
    mr, mc = Ez.mean(axis=1, keepdims=True), Tt.mean(axis=0, keepdims=True)
    Es, Ts = Ez - mr, Tt - mc
    me, mt = Es @ SelT.T / n, SelE @ Ts / n
    ve, vt = (Es * Es) @ SelT.T / n - me * me, SelE @ (Ts * Ts) / n - mt * mt
    return 0.5 * ((S - (mr + me)) / np.sqrt(ve) + (S - (mc + mt)) / np.sqrt(vt))


def host_numpy(mode, S, Ez, Tt, Zt, n):
    if mode == "as2":
        return as2_products(S, Ez, Tt, n)
    if mode == "zt":
        Tt = (Tt - Zt.mean(axis=1, keepdims=True)) / Zt.std(axis=1, keepdims=True)
    if mode == "as1":
        (me, se), (mt, st) = top_moments(Ez, n, 1), top_moments(Tt, n, 0)
    else:
        me, se = (Ez.mean(axis=1, keepdims=True), Ez.std(axis=1, keepdims=True)) if mode != "t" else (0.0, 1.0)
        mt, st = (Tt.mean(axis=0, keepdims=True), Tt.std(axis=0, keepdims=True)) if mode != "z" else (0.0, 1.0)
    if mode == "z":
        return (S - me) / se
    if mode == "t":
        return (S - mt) / st
    if mode == "zt":
        return ((S - me) / se - mt) / st
    return 0.5 * ((S - me) / se + (S - mt) / st)


def shape(name, J, T, Cn, n):
    from speaker_recognition_amd import _lib, scorenorm as sn
    rng = np.random.default_rng(J + T + Cn)
    bias = 0.3 * rng.standard_normal(Cn)
    S = rng.standard_normal((J, T)) + 3.0 * (np.arange(J * T).reshape(J, T) % 7 == 0)
    Ez, Tt, Zt = rng.standard_normal((J, Cn)) + bias, rng.standard_normal((Cn, T)) + bias[:, None], rng.standard_normal((Cn, Cn)) + bias
    out = {"shape": name, "models": J, "segments": T, "cohort": Cn, "top_n": n, "modes": {}}
    kinds = (("select", _lib.T_JFA_FACTOR), ("shifted_copies", _lib.T_JFA_GRAM), ("products_SelT", _lib.T_JFA_GEMM_A),
             ("products_SelE", _lib.T_JFA_GEMM_B), ("apply", _lib.T_JFA_UPDATE))
    for mode in MODES:
        a = (S, mode, Ez if mode != "t" else None, Tt if mode != "z" else None, Zt if mode == "zt" else None)
        kw = dict(top_n=n) if mode in ("as1", "as2") else {}
        m = {"plan": _lib.score_norm_plan(mode, J, T, Cn, Cn, n, 1 << 30, 0)}
        m["call_ms"], got = median_ms(lambda: sn.normalise(*a, **kw))
        _lib.profile_enable(True)
        _lib.profile_reset()
        _, counts = sn.normalise(*a, return_counts=True, **kw)
        stages = {k: _lib.profile_get(kind) for k, kind in kinds}
        _lib.profile_enable(False)
        m["degenerate"] = counts
        m["device_stage_ms"] = {k: v[0] for k, v in stages.items()}
        m["device_stage_launches"] = {k: int(v[1]) for k, v in stages.items()}
        m["device_ms"] = float(sum(v[0] for v in stages.values()))
        m["dominant_stage"] = max(stages, key=lambda k: stages[k][0])
        if mode == "as2":
            flop = 4 * 2.0 * J * T * Cn
            ms = stages["products_SelT"][0] + stages["products_SelE"][0]
            m["products_flop"] = flop
            m["products_tflops_f64"] = flop / (ms * 1e-3) / 1e12 if ms > 0 else None
            m["products_share_of_peak"] = m["products_tflops_f64"] / PEAK_F64_TFLOPS if ms > 0 else None
        t0 = time.perf_counter()
        host = host_numpy(mode, S, Ez, Tt, Zt, n)
        m["host_numpy_ms"] = 1e3 * (time.perf_counter() - t0)
        m["max_abs_difference_to_host_numpy"] = float(np.abs(got - host).max())
        out["modes"][mode] = m
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--shapes", default="a,b")
    args = ap.parse_args()
    from speaker_recognition_amd import _lib
    want = args.shapes.split(",")
    shapes = []
    if "a" in want:
        shapes.append(shape("a_200x2000_C2000_N200", 200, 2000, 2000, 200))
    if "b" in want:
        shapes.append(shape("b_1000x1000_C1000_N100", 1000, 1000, 1000, 100))
    out = {"device": _lib.device_name(), "peak_f64_tflops_data_sheet": PEAK_F64_TFLOPS, "shapes": shapes}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
