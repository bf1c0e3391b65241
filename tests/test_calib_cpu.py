"""CPU side of score calibration (csrc/calib.hip, csrc/calib_plan.cpp, speaker_recognition_amd/calibration.py): the numpy restatement
(tests/calib_cases.py) against its second statements, inside its own gate, against the named mutants on the GPU tests' own inputs and
on cases worked by hand; the conditions under which the GPU tests may compare pass counts; the symbols, the option, the plan
(sr_calib_plan -- also under the host sanitizers, tests/host/calib_checks.cpp), every refusal without a device, the forked-process
refusal and the kernels' resource records."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calib_cases as cc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")
NEW = ["sr_calib_train", "sr_calib_eval", "sr_calib_apply", "sr_calib_counts", "sr_calib_plan"]
SMALL = [c for c in cc.PARITY_CASES if c[1] <= 257 and c[0] <= 2]


@pytest.mark.parametrize("case", cc.PARITY_CASES)
def test_the_restatement_stays_inside_its_gate(case):
    """The float64 restatement lies within one gate of the np.longdouble statement on every input of the GPU parity test: the
    reference alone, with the rounding of its own sums, fits the bound the device is held to."""
    S, n, P = case
    X, lab = cc.inputs(S, n)
    ref, g = cc.parity_reference(*case)
    ratio = cc.worst_ratio(cc.evaluate(X, lab, cc.parity_theta(S), P, cc.PARITY_LAM)[:3], ref, g)
    print("calib restatement %s: difference / gate = %.3g" % (case, ratio))
    assert ratio <= 1
    if n > 2:
        assert (lab < 0).sum() > 0 and abs((lab < 0).mean() - 0.1) < 0.06          # a tenth of the labels skipped


def test_the_restatement_on_the_large_scores_case():
    X, lab, th, P = cc.big_inputs()
    z = cc.apply(X, th)[0]
    assert 9e3 < np.abs(z).max() <= 1e4 and np.abs(th).max() > 5e2          # (theta = 1e3 x a draw of order one)
    got = cc.evaluate(X, lab, th, P, 0.0)
    assert all(np.all(np.isfinite(v)) for v in got[:3])
    ratio = cc.worst_ratio(got[:3], cc.evaluate(X, lab, th, P, 0.0, dtype=np.longdouble)[:3], cc.gate(X, lab, th, P, 0.0))
    assert ratio <= 1


@pytest.mark.parametrize("case", SMALL)
def test_second_statements_of_f_g_and_H(case):
    """f through np.logaddexp within the gate; g by central differences of that f and H by central differences of g, in np.longdouble,
    within the differences' own derived error."""
    S, n, P = case
    X, lab = cc.inputs(S, n)
    th = cc.parity_theta(S)
    ref, g = cc.parity_reference(*case)
    assert abs(float(cc.f_logaddexp(X, lab, th, P, cc.PARITY_LAM) - ref[0])) <= g["f"]
    gd, Hd, tol_g, tol_H = cc.central_differences(X, lab, th, P, cc.PARITY_LAM)
    assert float(np.abs(gd - ref[1]).max()) <= tol_g and float(np.abs(Hd - ref[2]).max()) <= tol_H
    assert tol_g < 1e-6 * float(np.abs(ref[1]).max()) and tol_H < 1e-6 * float(np.abs(ref[2]).max())          # (the tolerances bite)


@pytest.mark.parametrize("case", cc.PARITY_CASES[:-6:3] + cc.PARITY_CASES[-2:])
def test_the_inputs_distinguish_every_eval_mutant(case):
    """Class weights dropped, tau omitted, the ridge on the offset too, the 1 / ln 2 missing, skipped labels counted as non-targets:
    each lies at least 1000 gates from the restatement on the parity inputs where it can show (equal class weights cannot at n = 2
    with P = 0.5; tau cannot at P = 0.5; nothing is skipped at n = 2)."""
    S, n, P = case
    X, lab = cc.inputs(S, n)
    th = cc.parity_theta(S)
    ref, g = cc.parity_reference(*case)
    for m in cc.EVAL_MUTANTS:
        if (m == "no_tau" and P == 0.5) or (m == "skip_as_non" and n == 2) or (m == "no_class_weights" and n == 2 and P == 0.5):
            continue
        assert cc.worst_ratio(cc.evaluate(X, lab, th, P, cc.PARITY_LAM, mutant=m)[:3], ref, g) >= 1000, (m, case)


def test_hand_cases_of_cllr_min_cllr_and_act_dcf():
    from speaker_recognition_amd import calibration as cal
    lab = np.array([1, 1, 0, 0, -1])
    assert cc.cllr([0.0] * 5, lab) == 1.0                                   # llr = 0 says nothing: one bit
    assert cc.evaluate(np.zeros((1, 5)), lab, [1.0, 0.0])[3] == (2, 2, 1)
    # ln 3 for a target: log2(1 + 1/3); -ln 3 for a non-target the same; both classes -> log2(4/3)
    assert abs(cc.cllr([np.log(3), np.log(3), -np.log(3), -np.log(3), 99.0], lab) - np.log2(4 / 3)) < 1e-15
    for mc in (cal.min_cllr, cc.min_cllr, cc.min_cllr_hull):
        assert mc([3.0, 4.0, 1.0, 2.0], [1, 1, 0, 0]) == 0.0               # separated: the end blocks are pure and cost nothing
        assert mc([1.0, 2.0, 3.0, 4.0], [1, 1, 0, 0]) == 1.0               # reversed at equal counts: one block, llr 0
        # ties move together: targets (1, .5), non-targets (.5, 0): blocks {0}, {.5, .5}, {1} -> llr -inf, 0, +inf -> 1/2
        assert mc([1.0, 0.5, 0.5, 0.0], [1, 1, 0, 0]) == 0.5
        assert mc([1.0, 0.5, 0.5, 0.0, 7.0], [1, 1, 0, 0, -1]) == 0.5      # a skipped entry is not a trial
    # (apart, the tied pair would be ordered target-above-non-target or the reverse: 0 or more than 1/2)
    assert cc.min_cllr([1.0, 0.5 + 1e-9, 0.5, 0.0], [1, 1, 0, 0]) == 0.0
    rng = np.random.default_rng(3)
    for k in range(40):                                                     # PAV against the hull of every threshold's operating point
        n = int(rng.integers(2, 13))
        s = np.round(rng.standard_normal(n) * 2) / 2                        # many ties
        lab = (rng.random(n) < 0.5).astype(int)
        lab[0], lab[-1] = 1, 0
        a, b, c = cc.min_cllr(s, lab), cc.min_cllr_hull(s, lab), cal.min_cllr(s, lab)
        assert abs(a - b) < 1e-14 and abs(a - c) < 1e-14, (s, lab, a, b, c)
    # actual DCF with a score exactly on the threshold: accepted (>=).  P = 0.5, unit costs: thr = 0
    llr, lab = [0.0, -1.0, 0.0, 1.0], [1, 1, 0, 0]
    assert cal.bayes_threshold(0.5) == 0.0 and cal.bayes_threshold(0.01) == np.log(99.0)
    assert cal.bayes_threshold(0.5, c_miss=1.0, c_fa=10.0) == np.log(10.0)
    miss, fa = cc.counts(llr, lab, [0.0])
    assert (miss[0], fa[0]) == (1, 2)                                       # the target on the threshold is no miss; the non-target on it is a false alarm
    assert cc.act_dcf(llr, lab, 0.5) == (0.5 * 0.5 + 0.5 * 1.0) / 0.5
    m2, f2 = cc.counts(llr, lab, [0.0], mutant="gt_threshold")
    assert (m2[0], f2[0]) == (2, 1)                                         # ">" in place of ">=" moves both
    with pytest.raises(ValueError):
        cal.bayes_threshold(1.0)
    with pytest.raises(ValueError):
        cal.min_cllr([1.0, 2.0], [1, 1])


def test_the_counts_inputs_distinguish_their_mutants():
    llr, lab, thr = cc.counts_inputs()
    assert thr.size == 16 and np.isinf(thr[0]) and np.isinf(thr[-1]) and (lab < 0).sum() > 0
    assert sum(int((llr[lab >= 0] == t).sum()) for t in thr[1:-1]) > 100    # scores exactly on a threshold, at trials
    miss, fa = cc.counts(llr, lab, thr)
    assert miss[0] == 0 and fa[0] == (lab == 0).sum() and miss[-1] == (lab > 0).sum() and fa[-1] == 0
    for m in ("gt_threshold", "skip_as_non"):
        m2, f2 = cc.counts(llr, lab, thr, mutant=m)
        assert not (np.array_equal(miss, m2) and np.array_equal(fa, f2)), m


@pytest.mark.parametrize("name", list(cc.FIT_CASES))
def test_fit_inputs_converge_and_their_pass_counts_are_decided(name):
    """On every named input of the GPU fit test the restatement converges within the optimality criterion, and the two conditions
    hold under which its pass count, halvings and stop code may be asserted equal to the device's: no Newton decrement within a factor
    100 of tol on either side, no accept decision with |f_new - f| within 100 gates."""
    X, lab, P, lam, th0 = cc.fit_inputs(name)
    r = cc.fit(X, lab, P, lam, th0)
    print("calib fit %s: %s after %d passes, %d halvings, lam2 %s" % (name, r["stop"], r["passes"], r["halvings"], ["%.2g" % v for v in r["lam2s"]]))
    assert r["stop"] == "CONVERGED" and 4 <= r["passes"] <= 12 and r["passes"] == 1 + r["accepted"] + r["halvings"]
    assert cc.loop_is_decided(X, lab, P, lam, r)
    crit, bound = cc.optimality(X, lab, r["theta"], P, lam)
    assert crit <= bound
    if name == "halving":
        assert r["halvings"] >= 1
        # accepting without the f_new <= f test shows on this input
        m = cc.fit(X, lab, P, lam, th0, mutant="accept_always")
        assert m["halvings"] == 0 and (m["passes"], m["stop"]) != (r["passes"], r["stop"]) or not np.allclose(m["theta"], r["theta"])
    else:
        assert r["halvings"] == 0 or name == "n257_S2_P01"


def test_degenerate_fits_of_the_restatement():
    # separable data: a ridge gives a finite optimum; without one the loop still ends, with finite weights
    X, lab = cc.inputs(2, 257, separable=True)
    r = cc.fit(X, lab, 0.5, 1e-3)
    assert r["stop"] == "CONVERGED" and cc.optimality(X, lab, r["theta"], 0.5, 1e-3)[0] <= cc.optimality(X, lab, r["theta"], 0.5, 1e-3)[1]
    r0 = cc.fit(X, lab, 0.5, 0.0)
    assert r0["stop"] in cc.STOPS and np.all(np.isfinite(r0["theta"])) and r0["passes"] <= 100
    # two identical systems: H is singular at once; a ridge splits the weight evenly
    X1, lab1 = cc.inputs(1, 257)
    XX = np.vstack([X1, X1])
    s = cc.fit(XX, lab1, 0.5, 0.0)
    assert s["stop"] == "SINGULAR" and s["passes"] == 1 and np.array_equal(s["theta"], np.zeros(3))
    s = cc.fit(XX, lab1, 0.5, 1e-6)
    assert s["stop"] == "CONVERGED" and abs(s["theta"][0] - s["theta"][1]) <= cc.equal_weights_bound(XX, lab1, s["theta"], 0.5, 1e-6)
    # the cap: passes == max_pass exactly, and a capped fit continues to the uncapped one
    c = cc.fit(X1, lab1, 0.5, 0.0, max_pass=2)
    assert c["stop"] == "CAP" and c["passes"] == 2


def test_symbols_exported_and_declared(built_lib):
    from speaker_recognition_amd import _lib, calibration as cal
    header = open(os.path.join(ROOT, "include", "pygmm_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), "lib/pygmm.so does not export %s" % name
        assert re.search(r"\bint %s\(" % name, header), "%s is not declared in include/pygmm_hip.h" % name
        assert name in _lib.EXT_SYMBOLS
    assert "SR_T_COUNT 20" in header and "calib_scratch_mib" in header and "up to 8 systems" in header          # no timer kind is added
    for name in ("Calibrator", "cllr", "min_cllr", "error_counts", "act_dcf", "bayes_threshold", "evaluate"):
        assert callable(getattr(cal, name))
    for bad in (0, (1 << 20) + 1):
        with pytest.raises(_lib.SRError, match="calib_scratch_mib must be within 1 .. 1048576 .the default is 8192."):
            _lib.set_option("calib_scratch_mib", bad)
    _lib.set_option("calib_scratch_mib", 1)
    _lib.set_option("calib_scratch_mib", 1 << 20)
    _lib.set_option("calib_scratch_mib", 8192)


def test_plan_blocks_bytes_and_state(built_lib):
    from speaker_recognition_amd import _lib
    for S in (1, 2, 8):
        P = S + 1
        for n, blocks in ((1, 1), (4095, 1), (4096, 1), (4097, 2), (257 * 4096 + 1, 258), (10 ** 8, 24415)):
            p = _lib.calib_plan(S, n, 16)
            A = 1 + P + P * (P + 1) // 2
            assert (p["n_blocks"], p["acc"], p["state_len"]) == (blocks, A, 16 + 4 * P + P * (P + 1) // 2)
            assert p["bytes_X"] == 8 * S * n and p["bytes_lab"] == n and p["bytes_partial"] == 8 * A * blocks
            assert p["resident_train"] == 8 * S * n + n + 8 * A * blocks + 8 * p["state_len"]
            assert p["pass_grid"] == p["counts_grid"] == p["apply_grid"] == blocks and p["step_grid"] == 1
            for n_cu in (1, 64):                   # the device's size moves nothing but the rounds
                o = _lib.calib_plan(S, n, 16, n_cu=n_cu)
                assert o["pass_rounds"] == -(-blocks // n_cu)
                assert {k: v for k, v in o.items() if k != "pass_rounds"} == {k: v for k, v in p.items() if k != "pass_rounds"}
            assert _lib.calib_plan(S, n, 16, "train", p["resident_train"]) == p
            with pytest.raises(_lib.SRError, match="raise the option calib_scratch_mib or calibrate on fewer trials"):
                _lib.calib_plan(S, n, 16, "train", p["resident_train"] - 1)
    p = _lib.calib_plan(8, 1)
    assert (p["max_S"], p["max_thresholds"], p["block"], p["workgroup"], p["acc"]) == (8, 16, 4096, 256, 55)
    assert (p["cadence"], p["max_pass"], p["max_n"]) == (4, 1000, 1 << 35)
    # the flagship shape fits the default bound three systems wide, not sixteen GiB of it
    assert _lib.calib_plan(3, 10 ** 8)["resident_train"] < 8192 << 20 < _lib.calib_plan(8, 2 * 10 ** 8)["resident_train"]


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _i8(a):
    return a.ctypes.data_as(C.POINTER(C.c_int8)) if a is not None else None


def _case():
    return dict(S=2, n=4, X=np.array([[2.0, -1.0, 1.0, -1.5], [1.0, 0.5, -0.5, -1.0]]), lab=np.array([1, 1, 0, -1], dtype=np.int8), prior=0.5,
                ridge=0.0, tol=1e-16, max_pass=100, theta0=None, resume=0, state=np.zeros(16 + 12 + 6))


def _train(L, **over):
    a = dict(_case(), **over)
    return L.sr_calib_train(a["S"], a["n"], _dp(a["X"]), _i8(a["lab"]), a["prior"], a["ridge"], a["tol"], a["max_pass"], _dp(a["theta0"]),
                            a["resume"], _dp(a["state"]), None)


def _bad(arr, idx, value):
    out = np.array(arr)
    out.flat[idx] = value
    return out


REFUSALS = [(dict(S=0), "up to 8 systems .* S is 0"), (dict(S=9), "up to 8 systems .* S is 9; fuse in two stages or drop a system"),
            (dict(n=0), "n is 0; need at least one trial"), (dict(n=-3), "need at least one trial"), (dict(n=1 << 62), "split the trial list"),
            (dict(lab=np.array([0, -1, 0, -1], dtype=np.int8)), "0 targets and 2 non-targets; need at least one trial of each class"),
            (dict(lab=np.array([1, 1, 1, -1], dtype=np.int8)), "3 targets and 0 non-targets"),
            (dict(lab=np.array([1, 2, 0, -1], dtype=np.int8)), "label 1 is 2; a label is 1 .target., 0 .non-target. or negative"),
            (dict(prior=0.0), "the prior is 0; it is a probability strictly inside"), (dict(prior=1.0), "the prior is 1"),
            (dict(prior=np.nan), "the prior is"), (dict(ridge=-1.0), "the ridge is -1; it is a finite value >= 0"),
            (dict(ridge=np.inf), "the ridge is inf"), (dict(ridge=np.nan), "the ridge is"), (dict(tol=-1e-3), "tol is -0.001"),
            (dict(max_pass=0), "max_pass is 0; a call makes 1 .. 1000 passes"), (dict(max_pass=1001), "max_pass is 1001"),
            (dict(X=_bad(_case()["X"], 1, np.nan)), "system 0 holds a non-finite score at trial 1; mark that trial as skipped"),
            (dict(X=_bad(_case()["X"], 6, np.inf)), "system 1 holds a non-finite score at trial 2"),
            (dict(theta0=np.array([0.0, np.nan, 0.0])), "theta0 holds a non-finite value at element 1"),
            (dict(theta0=np.array([0.0, 0.0, np.inf])), "theta0 holds a non-finite value at element 2"),
            (dict(X=None), r"null argument \(X"), (dict(lab=None), r"null argument \(lab"), (dict(state=None), r"null argument \(state"),
            (dict(resume=1), "resume needs the state of a call with the same S that ended by CAP")]


def test_refusals_need_no_device(built_lib):
    """Every refusal fails on its arguments alone, with a text that names the argument and the remedy -- never the device."""
    from speaker_recognition_amd import _lib, calibration as cal
    L = built_lib
    for over, pat in REFUSALS:
        assert _train(L, **over) == -1, over
        assert re.search(pat, _lib.last_error()) and "HIP" not in _lib.last_error(), (over, _lib.last_error())
    # a skipped position may hold anything: this gets as far as the device
    c = _case()
    skipped_nan = _bad(c["X"], 3, np.nan)
    f, g, H, th = C.c_double(), np.zeros(3), np.zeros((3, 3)), np.array([1.0, 0.5, 0.0])
    ev = lambda **o: (lambda a: L.sr_calib_eval(a["S"], a["n"], _dp(a["X"]), _i8(a["lab"]), a["prior"], a["ridge"], _dp(a.get("theta", th)),  # noqa: E731
                                                 a.get("f", C.byref(f)), _dp(g), _dp(H), None))(dict(c, **o))
    for over, pat in ((dict(S=9), "up to 8 systems"), (dict(prior=2.0), "the prior is 2"), (dict(ridge=-1.0), "the ridge is -1"),
                      (dict(theta=None), r"null argument \(theta"), (dict(theta=np.array([np.nan, 0.0, 0.0])), "theta holds a non-finite value"),
                      (dict(f=None), r"null argument \(f"), (dict(X=_bad(c["X"], 0, np.nan)), "non-finite score at trial 0"),
                      (dict(lab=None), r"null argument \(lab")):
        assert ev(**over) == -1 and re.search(pat, _lib.last_error()) and "HIP" not in _lib.last_error(), (over, _lib.last_error())
    out = np.zeros(4)
    for args, pat in (((9, 4, _dp(c["X"]), _dp(th), _dp(out)), "up to 8 systems"), ((2, 0, _dp(c["X"]), _dp(th), _dp(out)), "n is 0"),
                      ((2, 4, None, _dp(th), _dp(out)), r"null argument \(X"), ((2, 4, _dp(c["X"]), None, _dp(out)), r"null argument \(theta"),
                      ((2, 4, _dp(c["X"]), _dp(th), None), r"null argument \(out"),
                      ((2, 4, _dp(c["X"]), _dp(np.array([1.0, np.inf, 0.0])), _dp(out)), "theta holds a non-finite value at element 1")):
        assert L.sr_calib_apply(*args) == -1 and re.search(pat, _lib.last_error()) and "HIP" not in _lib.last_error(), _lib.last_error()
    llr, thr = np.array([0.5, -0.5, 0.0, np.nan]), np.array([-np.inf, 0.0, np.inf])
    miss, fa = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64)
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None          # noqa: E731
    for args, pat in (((0, _dp(llr), _i8(c["lab"]), 3, _dp(thr), i64(miss), i64(fa)), "n is 0"),
                      ((4, _dp(llr), _i8(c["lab"]), 0, _dp(thr), i64(miss), i64(fa)), "0 thresholds; one counts call takes 1 .. 16"),
                      ((4, _dp(llr), _i8(c["lab"]), 17, _dp(thr), i64(miss), i64(fa)), "17 thresholds"),
                      ((4, _dp(llr), _i8(c["lab"]), 3, _dp(np.array([0.0, np.nan, 1.0])), i64(miss), i64(fa)), "threshold 1 is a NaN"),
                      ((4, _dp(llr), _i8(c["lab"]), 3, None, i64(miss), i64(fa)), r"null argument \(thr"),
                      ((4, None, _i8(c["lab"]), 3, _dp(thr), i64(miss), i64(fa)), r"null argument \(llr"),
                      ((4, _dp(llr), None, 3, _dp(thr), i64(miss), i64(fa)), r"null argument \(lab"),
                      ((4, _dp(llr), _i8(c["lab"]), 3, _dp(thr), None, i64(fa)), r"null argument \(miss and fa"),
                      ((4, _dp(_bad(llr, 1, np.inf)), _i8(c["lab"]), 3, _dp(thr), i64(miss), i64(fa)), "non-finite score at trial 1")):
        assert L.sr_calib_counts(*args, None) == -1 and re.search(pat, _lib.last_error()) and "HIP" not in _lib.last_error(), _lib.last_error()
    # the bound: the option's smallest value is 1 MiB; 2^17 trials of one system take 8 x 2^17 + 2^17 bytes and more
    out28 = (C.c_int64 * 28)()
    _lib.set_option("calib_scratch_mib", 1)
    try:
        big_n = 1 << 17
        Xb, lb = np.zeros((1, big_n)), np.zeros(big_n, dtype=np.int8)
        lb[0] = 1
        assert _train(L, S=1, n=big_n, X=Xb, lab=lb, state=np.zeros(30)) == -1
        assert re.search(r"calibration \(train\): the arrays resident on the device take \d+ bytes .1 system.s. x 131072 trials., the bound is 1048576 "
                         "bytes; raise the option calib_scratch_mib or calibrate on fewer trials at a time", _lib.last_error()) and "HIP" not in _lib.last_error()
        assert L.sr_calib_apply(1, big_n, _dp(Xb), _dp(np.array([1.0, 0.0])), _dp(np.zeros(big_n))) == -1 and "calib_scratch_mib" in _lib.last_error()
        assert L.sr_calib_counts(big_n, _dp(Xb), _i8(lb), 3, _dp(thr), i64(miss), i64(fa), None) == -1 and "calib_scratch_mib" in _lib.last_error()
        with pytest.raises(_lib.SRError, match="calib_scratch_mib"):
            cal.Calibrator().fit(Xb[0], lb)
    finally:
        _lib.set_option("calib_scratch_mib", 8192)
    for args, pat in (((0, 4, 0, 0, 0, 256), "up to 8 systems"), ((1, 4, 17, 0, 0, 256), "17 thresholds"), ((1, 4, 0, 3, 0, 256), "call is 0"),
                      ((1, 1 << 20, 0, 0, 1 << 20, 256), "raise the option calib_scratch_mib")):
        assert L.sr_calib_plan(*args, out28, 28) == -1 and re.search(pat, _lib.last_error()) and "HIP" not in _lib.last_error(), _lib.last_error()
    assert L.sr_calib_plan(1, 4, 0, 0, 0, 256, out28, 27) == -1 and "28 fields" in _lib.last_error()
    assert L.sr_calib_plan(1, 4, 0, 0, 0, 256, None, 28) == -1 and "null argument" in _lib.last_error()
    assert L.sr_calib_plan(1, 4097, 0, 0, 0, 256, out28, 28) == 28 and out28[2] == 2 and out28[4] == 27
    # the Python layer
    with pytest.raises(_lib.SRError, match="up to 8 systems"):
        cal.Calibrator().fit(np.zeros((9, 4)), [1, 0, 1, 0])
    with pytest.raises(ValueError, match="expected scores of the labels' shape"):
        cal.Calibrator().fit(np.zeros((2, 5)), [1, 0, 1, 0])
    with pytest.raises(ValueError, match="every system's scores in one shape"):
        cal.Calibrator().fit([np.zeros((2, 3)), np.zeros((3, 2))], np.zeros((2, 3)))
    with pytest.raises(ValueError, match="theta0 as 2 weights and the offset"):
        cal.Calibrator().fit(c["X"], c["lab"], theta0=[0.0, 0.0])
    with pytest.raises(ValueError, match="resume needs an earlier fit"):
        cal.Calibrator().fit(c["X"], c["lab"], resume=True)
    with pytest.raises(ValueError, match="needs a fitted calibrator"):
        cal.Calibrator().transform(c["X"])
    with pytest.raises(ValueError, match="one label per llr"):
        cal.cllr([0.0, 1.0], [1, 0, 1])
    with pytest.raises(ValueError, match="labels are whole numbers"):
        cal.cllr([0.0, 1.0], [0.5, 1.0])
    with pytest.raises(_lib.SRError, match="the prior is 1.5"):
        cal.Calibrator(prior=1.5).fit(c["X"], c["lab"])
    with pytest.raises(_lib.SRError, match="non-finite score at trial 1"):
        cal.cllr([0.0, np.nan, 1.0], [1, 0, 1])
    with pytest.raises(_lib.SRError, match="label 1 is 2"):
        cal.cllr([0.0, 0.5, 1.0], [1, 5, 0])
    if _lib.device_count() == 0:                       # and a call that needs the device says what is missing: no CPU path
        assert _train(L) == -1 and "no HIP device" in _lib.last_error()
        assert _train(L, X=skipped_nan) == -1 and "no HIP device" in _lib.last_error()
        assert ev() == -1 and "no HIP device" in _lib.last_error()
        assert L.sr_calib_apply(2, 4, _dp(c["X"]), _dp(th), _dp(out)) == -1 and "no HIP device" in _lib.last_error()
        assert L.sr_calib_counts(4, _dp(llr), _i8(c["lab"]), 3, _dp(thr), i64(miss), i64(fa), None) == -1 and "no HIP device" in _lib.last_error()
        assert L.sr_calib_plan(1, 4, 0, 0, 0, 0, out28, 28) == -1 and "no HIP device" in _lib.last_error()
        with pytest.raises(_lib.SRError, match="no HIP device"):
            cal.act_dcf([1.0, -1.0], [1, 0])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_calib_plan_under_asan_ubsan(tmp_path):
    """csrc/calib_plan.cpp -- every refusal's text, the block counts at n = 1, 4095, 4096, 4097, the bytes, the state length, the
    bound's refusal with its remedy, n near 2^62 -- by a stand-alone program (tests/host/calib_checks.cpp) built with AddressSanitizer
    + UBSan: host code only, no GPU, nothing loaded into Python."""
    exe = str(tmp_path / "calib_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "host", "calib_checks.cpp"), os.path.join(CSRC, "calib_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "calib checks ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_calib_kernels_keep_nothing_in_scratch(built_lib):
    import test_abi_cpu
    res = test_abi_cpu._kernel_resources("calib")
    names = " ".join(res)
    for S in range(1, 9):
        for kernel in ("17calib_pass_kernelILi%dE", "17calib_step_kernelILi%dE", "18calib_apply_kernelILi%dE"):
            assert kernel % S in names, kernel % S
    assert "calib_counts_kernel" in names and len(res) == 25
    for name, r in res.items():
        assert r["scratch"] == 0, (name, r)


def test_refused_in_a_process_forked_after_runtime_use(built_lib):
    """In a child forked after its parent touched the GPU runtime the four calls say so and name the remedy; the argument refusals
    and the plan still work there."""
    import test_fork
    from speaker_recognition_amd import _lib
    L = built_lib
    L.sr_device_count()                                # (this call is what initialises the runtime in the parent)

    def child():
        c = _case()
        th, out = np.array([1.0, 0.5, 0.0]), np.zeros(4)
        f = C.c_double()
        miss, fa = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
        i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))          # noqa: E731
        res = {"lost": L.sr_gpu_runtime_lost()}
        res["train"] = _train(L)
        res["train_error"] = _lib.last_error()
        res["eval"] = L.sr_calib_eval(2, 4, _dp(c["X"]), _i8(c["lab"]), 0.5, 0.0, _dp(th), C.byref(f), None, None, None)
        res["eval_error"] = _lib.last_error()
        res["apply"] = L.sr_calib_apply(2, 4, _dp(c["X"]), _dp(th), _dp(out))
        res["apply_error"] = _lib.last_error()
        res["counts"] = L.sr_calib_counts(4, _dp(c["X"]), _i8(c["lab"]), 1, _dp(np.array([0.0])), i64(miss), i64(fa), None)
        res["counts_error"] = _lib.last_error()
        res["refusal"] = _train(L, S=9)
        res["refusal_error"] = _lib.last_error()
        res["plan"] = _lib.calib_plan(2, 4097)["n_blocks"]
        return res

    out = test_fork._in_forked_child(child)
    assert out["lost"] == 1 and out["train"] == out["eval"] == out["apply"] == out["counts"] == out["refusal"] == -1 and out["plan"] == 2
    for call in ("train", "eval", "apply", "counts"):
        assert "forked after its parent" in out[call + "_error"] and "sr_calib_" + call in out[call + "_error"], out[call + "_error"]
    assert "up to 8 systems" in out["refusal_error"]
    assert L.sr_gpu_runtime_lost() == 0                # the parent is untouched
