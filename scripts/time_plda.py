#!/usr/bin/env python3
"""What the i-vector back end costs on the device (csrc/plda.hip), in one run; one JSON line on stdout.

    python scripts/time_plda.py [--out profiles/r22_plda.json] [--parts fit,score_large,score_small]

Data drawn from the model itself (Sb and Sw of condition 10, as tests/plda_cases.py draws them):
  fit          PLDA.fit, 10 rounds, 5000 speakers x 10 sessions x R = 400;
  score_large  PLDA.score, 1000 models x 100 000 segments x R = 400, the models' enrolment counts cycling 1 .. 7 (seven count classes);
  score_small  the same at 200 x 2000.
For every part:
  * the whole call as a user writes it (`PLDA().fit(X, ids)` from the default start, `PLDA.score(enrol, ids, X)`): host wall clock,
    median, smallest and largest of 3 after a warm-up -- it includes the Python layer's checks and sums, the library's checks of its
    inputs, the copies to the device and back;
  * the device time of every stage of one call from the library's event timers (the SR_T_JFA_* kinds the stages are booked to);
  * for the scores the float64 rate of the cross term (2 J T R operations over SR_T_JFA_GEMM_C) and of all products, against the
    data sheet's 78.6 TFLOP/s;
  * in the same run the same computation in vectorised numpy on the host (the formulas of tests/plda_cases.py with one product per
    count class instead of a loop over models), timed on the first `host_segments` segments and scaled by T / host_segments where the
    part says so, and the largest difference between the two relative to the largest magnitude."""
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


def timed(fn, reps):
    from speaker_recognition_amd import _lib
    res = fn()
    _lib.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        _lib.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t)), "runs": reps}, res


def stages_of(fn):
    from speaker_recognition_amd import _lib
    kinds = (("elementwise_sums_rowdots", _lib.T_JFA_GRAM), ("factorisations", _lib.T_JFA_FACTOR), ("products_Sw_Pc", _lib.T_JFA_GEMM_B),
             ("products_Phi_YhatPc", _lib.T_JFA_GEMM_L), ("sums_over_rows", _lib.T_JFA_GEMM_A), ("cross_term", _lib.T_JFA_GEMM_C),
             ("update_assemble", _lib.T_JFA_UPDATE))
    _lib.profile_enable(True)
    _lib.profile_reset()
    fn()
    got = {k: _lib.profile_get(kind) for k, kind in kinds}
    _lib.profile_enable(False)
    return {"device_stage_ms": {k: v[0] for k, v in got.items()}, "device_stage_launches": {k: int(v[1]) for k, v in got.items()},
            "device_ms": float(sum(v[0] for v in got.values())), "dominant_stage": max(got, key=lambda k: got[k][0])}


def draw(R, counts, seed):
    import plda_cases as pc
    rng = np.random.default_rng(seed)
    Sb, Sw = 2.0 * pc.spd(R, 10.0, rng), pc.spd(R, 10.0, rng)
    Lb, Lw = np.linalg.cholesky(Sb), np.linalg.cholesky(Sw)
    mu = rng.standard_normal(R)
    ids = np.repeat(np.arange(len(counts)), counts)
    y = rng.standard_normal((len(counts), R)) @ Lb.T
    X = mu + y[ids] + rng.standard_normal((ids.size, R)) @ Lw.T
    return mu, Sb, Sw, np.ascontiguousarray(X), ids, (rng, Lb, Lw)


def host_fit(X, ids, Sb, Sw, n_iter):
    """tests/plda_cases.em_step with one product per count class."""
    n, R = X.shape
    S = int(ids.max()) + 1
    counts = np.bincount(ids, minlength=S)
    mu = X.mean(axis=0)
    Xc = X - mu
    F = np.zeros((S, R))
    np.add.at(F, ids, Xc)
    T2 = Xc.T @ Xc
    if Sb is None:
        Sb = Sw = T2 / (2.0 * n)
    for _ in range(n_iter):
        iSb, iSw = np.linalg.inv(Sb), np.linalg.inv(Sw)
        G = F @ iSw
        Y = np.zeros_like(F)
        sp, snp = np.zeros((R, R)), np.zeros((R, R))
        for c in np.unique(counts):
            Phi = np.linalg.inv(iSb + c * iSw)
            rows = counts == c
            Y[rows] = G[rows] @ Phi
            sp += rows.sum() * Phi
            snp += rows.sum() * c * Phi
        FY = F.T @ Y
        Sb = (sp + Y.T @ Y) / S
        Sw = (T2 - FY - FY.T + Y.T @ (counts[:, None] * Y) + snp) / n
        Sb, Sw = 0.5 * (Sb + Sb.T), 0.5 * (Sw + Sw.T)
    return Sb, Sw


def host_score(mu, Sb, Sw, E, counts, X):
    """tests/plda_cases.score with one product per count class."""
    iSb, iSw = np.linalg.inv(Sb), np.linalg.inv(Sw)
    G = (E - counts[:, None] * mu) @ iSw
    Xc = X - mu
    P0 = np.linalg.inv(Sb + Sw)
    ld0 = np.linalg.slogdet(Sb + Sw)[1]
    a0 = np.einsum("tr,tr->t", Xc @ P0, Xc)
    out = np.zeros((E.shape[0], X.shape[0]))
    for c in np.unique(counts):
        rows = counts == c
        Phi = np.linalg.inv(iSb + c * iSw)
        Pc = np.linalg.inv(Phi + Sw)
        Y = G[rows] @ Phi
        M = Y @ Pc
        q = np.einsum("jr,jr->j", M, Y)
        a = np.einsum("tr,tr->t", Xc @ Pc, Xc)
        out[rows] = -0.5 * np.linalg.slogdet(Phi + Sw)[1] - 0.5 * (a[None, :] - 2.0 * (M @ Xc.T) + q[:, None]) + 0.5 * ld0 + 0.5 * a0[None, :]
    return out


def rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def part_fit(S, sessions, R, n_iter):
    from speaker_recognition_amd import _lib, plda
    mu, Sb, Sw, X, ids, _ = draw(R, (sessions,) * S, 1)
    order = np.random.default_rng(2).permutation(ids.size)
    X, ids = np.ascontiguousarray(X[order]), np.ascontiguousarray(ids[order])
    fit = lambda: plda.PLDA().fit(X, ids, n_iter=n_iter)                                # noqa: E731
    out = {"part": "fit", "speakers": S, "sessions": sessions, "R": R, "rounds": n_iter, "plan": {k: v for k, v in _lib.plda_plan(
        "train", R, ids, n_cu=0).items() if k not in ("perm", "classes")}}
    spread, m = timed(fit, 3)
    out["call_ms"], out["call_ms_spread"] = spread["median"], spread
    out.update(stages_of(fit))
    out["stop"], out["iterations"] = m.stop, m.iterations
    t0 = time.perf_counter()
    hb, hw = host_fit(X, ids, None, None, n_iter)
    out["host_numpy_ms"] = 1e3 * (time.perf_counter() - t0)
    out["host_numpy_over_call"] = out["host_numpy_ms"] / out["call_ms"]
    out["max_rel_difference_to_host_numpy"] = max(rel(m.Sb, hb), rel(m.Sw, hw))
    out["recovered_Sb_rel_error"], out["recovered_Sw_rel_error"] = rel(m.Sb, Sb), rel(m.Sw, Sw)
    return out


def part_score(name, J, T, R, reps, host_segments):
    from speaker_recognition_amd import _lib, plda
    counts = 1 + np.arange(J) % 7
    mu, Sb, Sw, enrol, ids, (rng, Lb, Lw) = draw(R, tuple(counts), J + T)
    X = np.ascontiguousarray(mu + rng.standard_normal((T, R)) @ Lb.T + rng.standard_normal((T, R)) @ Lw.T)
    model = plda.PLDA(mu, Sb, Sw)
    score = lambda: model.score(enrol, ids, X)                                          # noqa: E731
    out = {"part": name, "models": J, "segments": T, "R": R, "count_classes": 7,
           "plan": {k: v for k, v in _lib.plda_plan("score", R, counts, T=T, n_cu=0).items() if k not in ("perm", "classes")}}
    spread, got = timed(score, reps)
    out["call_ms"], out["call_ms_spread"] = spread["median"], spread
    out.update(stages_of(score))
    st = out["device_stage_ms"]
    cross = 2.0 * J * T * R
    products = cross + 2.0 * T * R * R * 8 + 2.0 * J * R * R * 3
    out["cross_term_flop"], out["products_flop"] = cross, products
    out["cross_term_tflops_f64"] = cross / (st["cross_term"] * 1e-3) / 1e12
    out["cross_term_share_of_peak"] = out["cross_term_tflops_f64"] / PEAK_F64_TFLOPS
    gemm_ms = st["cross_term"] + st["products_Sw_Pc"] + st["products_Phi_YhatPc"]
    out["products_tflops_f64"] = products / (gemm_ms * 1e-3) / 1e12
    E = np.zeros((J, R))
    np.add.at(E, ids, enrol)
    n = min(T, host_segments)
    t0 = time.perf_counter()
    host = host_score(mu, Sb, Sw, E, counts, X[:n])
    ms = 1e3 * (time.perf_counter() - t0)
    out["host_segments"], out["host_numpy_ms_measured"] = n, ms
    out["host_numpy_ms"] = ms * T / n                  # (every term but the J x R model side scales with the segments)
    out["host_numpy_extrapolated"] = n < T
    out["host_numpy_over_call"] = out["host_numpy_ms"] / out["call_ms"]
    out["max_rel_difference_to_host_numpy"] = rel(got[:, :n], host)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parts", default="fit,score_large,score_small")
    args = ap.parse_args()
    from speaker_recognition_amd import _lib
    want = args.parts.split(",")
    parts = []
    if "fit" in want:
        parts.append(part_fit(5000, 10, 400, 10))
    if "score_small" in want:
        parts.append(part_score("score_small_200x2000", 200, 2000, 400, 3, 2000))
    if "score_large" in want:
        parts.append(part_score("score_large_1000x100000", 1000, 100000, 400, 3, 5000))
    out = {"device": _lib.device_name(), "peak_f64_tflops_data_sheet": PEAK_F64_TFLOPS, "parts": parts}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
