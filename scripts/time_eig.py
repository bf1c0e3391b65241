#!/usr/bin/env python3
"""What the symmetric eigen-solver, LDA and the diagonalised PLDA scorer cost on the device (csrc/eig.hip, csrc/backend_eig.hip), in
one run; one JSON line on stdout.

    python scripts/time_eig.py [--out profiles/r23_eig.json] [--parts sym_eig,score_small,score_large,lda]

Every figure is the median of 3 after a warm-up, with the smallest and the largest (time_plda.py's `timed`); the device time of a
call's stages comes from the library's event timers (the SR_T_JFA_* kinds the stages are booked to).
  sym_eig      plda.sym_eig at R = 100, 200, 400, 512 on SPD input of condition 10: the call, the device time, the sweeps, the
               launches of a sweep, the device time per round; np.linalg.eigh on the host in the same run.
  score_small  DiagPLDA.score at 200 models x 2000 segments x R = 400, seven count classes, against PLDA.score of the same build in
               the same run (that path is the parent commit's: the "before" figure); `diagonalise()` timed on its own; the float64
               rate of the cross product J x T x R.
  score_large  the same at 1000 x 100 000.
  lda          LDA.fit at 50 000 vectors x 400 dimensions, 5000 classes, P = 200."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from time_plda import PEAK_F64_TFLOPS, draw, rel, timed  # noqa: E402
from time_plda import stages_of as stages_once  # noqa: E402


def stages_of(fn, reps=3):
    """time_plda's device times of one call, taken `reps` times: the run with the median device time, and the smallest and largest."""
    runs = sorted((stages_once(fn) for _ in range(reps)), key=lambda r: r["device_ms"])
    out = dict(runs[len(runs) // 2])
    out["device_ms_spread"] = {"median": out["device_ms"], "min": runs[0]["device_ms"], "max": runs[-1]["device_ms"], "runs": reps}
    return out


def part_sym_eig(sizes):
    import plda_cases as pc
    from speaker_recognition_amd import _lib, plda
    rows = []
    for R in sizes:
        A = pc.spd(R, 10.0, np.random.default_rng(R))
        call = lambda: plda.sym_eig(A, return_info=True)                               # noqa: E731
        spread, (w, V, info) = timed(call, 3)
        st = stages_of(call)
        plan = _lib.eig_plan(R, n_cu=0)
        host, (wh, _) = timed(lambda: np.linalg.eigh(A), 3)                             # noqa: B023
        wh, host_ms = wh[::-1], host["median"]
        rounds = max(1, info["sweeps"] * plan["rounds"])
        rows.append({"R": R, "call_ms": spread["median"], "call_ms_spread": spread, "device_ms": st["device_ms"],
                     "device_stage_ms": st["device_stage_ms"], "sweeps": info["sweeps"], "converged": info["converged"],
                     "device_ms_spread": st["device_ms_spread"], "host_eigh_ms_spread": host, "rounds_per_sweep": plan["rounds"], "launches_per_sweep": plan["launches_per_sweep"],
                     "device_us_per_round": 1e3 * st["device_ms"] / rounds, "host_eigh_ms": host_ms, "host_eigh_over_call": host_ms / spread["median"],
                     "max_rel_difference_to_host": float(np.abs(w - wh).max() / np.abs(wh).max())})
    return {"part": "sym_eig", "input": "SPD, condition 10", "sizes": rows}


def part_score(name, J, T, R):
    from speaker_recognition_amd import plda
    counts = 1 + np.arange(J) % 7
    mu, Sb, Sw, enrol, ids, (rng, Lb, Lw) = draw(R, tuple(counts), J + T)
    X = np.ascontiguousarray(mu + rng.standard_normal((T, R)) @ Lb.T + rng.standard_normal((T, R)) @ Lw.T)
    model = plda.PLDA(mu, Sb, Sw)
    spread_d, (diag, info) = timed(lambda: model.diagonalise(return_info=True), 3)
    out = {"part": name, "models": J, "segments": T, "R": R, "count_classes": 7, "diagonalise_ms": spread_d["median"],
           "diagonalise_ms_spread": spread_d, "diagonalise_sweeps": info["sweeps"], "diagonalise_status": info["status"]}
    out["diagonalise_device"] = stages_of(lambda: model.diagonalise(return_info=True))
    fast = lambda: diag.score(enrol, ids, X)                                             # noqa: E731
    full = lambda: model.score(enrol, ids, X)                                            # noqa: E731
    spread, got = timed(fast, 3)
    out["call_ms"], out["call_ms_spread"] = spread["median"], spread
    out.update(stages_of(fast))
    spread_f, want = timed(full, 3)
    out["full_call_ms"], out["full_call_ms_spread"] = spread_f["median"], spread_f
    out["full_device"] = stages_of(full)
    out["full_over_diag_call"] = out["full_call_ms"] / out["call_ms"]
    out["full_over_diag_device"] = out["full_device"]["device_ms"] / out["device_ms"]
    cross = 2.0 * J * T * R
    products = cross + 2.0 * T * R * R + 2.0 * T * R * 8 + 2.0 * J * R * R
    out["cross_term_flop"], out["products_flop"] = cross, products
    # (every product of the call is booked to one kind: the rate is of all of them together)
    out["products_tflops_f64"] = products / (out["device_stage_ms"]["cross_term"] * 1e-3) / 1e12
    out["products_share_of_peak"] = out["products_tflops_f64"] / PEAK_F64_TFLOPS
    out["max_rel_difference_to_full"] = rel(got, want)
    return out


def part_lda(n_classes, per_class, R, P):
    from speaker_recognition_amd import plda
    mu, Sb, Sw, X, ids, _ = draw(R, (per_class,) * n_classes, 3)
    order = np.random.default_rng(4).permutation(ids.size)
    X, ids = np.ascontiguousarray(X[order]), np.ascontiguousarray(ids[order])
    fit = lambda: plda.LDA().fit(X, ids, P)                                              # noqa: E731
    spread, m = timed(fit, 3)
    out = {"part": "lda_fit", "vectors": int(ids.size), "classes": n_classes, "R": R, "P": P, "call_ms": spread["median"], "call_ms_spread": spread}
    out.update(stages_of(fit))
    out["psi_first"], out["psi_last"] = float(m.psi[0]), float(m.psi[-1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parts", default="sym_eig,score_small,score_large,lda")
    args = ap.parse_args()
    from speaker_recognition_amd import _lib
    want = args.parts.split(",")
    parts = []
    if "sym_eig" in want:
        parts.append(part_sym_eig((100, 200, 400, 512)))
    if "score_small" in want:
        parts.append(part_score("score_small_200x2000", 200, 2000, 400))
    if "score_large" in want:
        parts.append(part_score("score_large_1000x100000", 1000, 100000, 400))
    if "lda" in want:
        parts.append(part_lda(5000, 10, 400, 200))
    out = {"device": _lib.device_name(), "peak_f64_tflops_data_sheet": PEAK_F64_TFLOPS, "parts": parts}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
