"""Score calibration on the device (csrc/calib.hip through calibration.Calibrator / evaluate / cllr / error_counts / act_dcf) against
the float64 numpy restatement written from the definitions (tests/calib_cases.py, which states the generator, the mutants and derives
the gate).  Every parity case prints its worst figure as a PARITY line before asserting.  A fitted theta is never compared with the
restatement's -- that comparison is as ill-conditioned as H; the restatement evaluates g and H at the device's theta instead."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calib_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _options(built_lib):
    from speaker_recognition_amd import _lib
    yield
    _lib.set_option("calib_scratch_mib", 8192)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _fit(X, lab, P=0.5, lam=0.0, theta0=None, **kw):
    from speaker_recognition_amd import calibration as cal
    return cal.Calibrator(prior=P, ridge=lam, **kw).fit(X, lab, theta0=theta0)


# ---- one pass ----

@pytest.mark.parametrize("case", cc.PARITY_CASES)
def test_eval_parity(built_lib, case):
    """f, g and H of one device pass within the gate of the np.longdouble statement: S = 1, 2, 8; n around a wave, a workgroup's
    stride, a block, two blocks and 257 blocks + 1 (the step kernel's lane loop wraps); P = 0.5 and 0.01; a tenth of the labels
    skipped; a ridge, so that its place shows."""
    from speaker_recognition_amd import calibration as cal
    S, n, P = case
    X, lab = cc.inputs(S, n)
    ref, g = cc.parity_reference(*case)
    f, gd, H, counts = cal.evaluate(X, lab, cc.parity_theta(S), prior=P, ridge=cc.PARITY_LAM)
    ratio = cc.worst_ratio((f, gd, H), ref, g)
    print("PARITY calib eval S=%d n=%d P=%g: difference / gate = %.3g" % (S, n, P, ratio))
    assert counts == {"targets": int((lab > 0).sum()), "non_targets": int((lab == 0).sum()), "skipped": int((lab < 0).sum())}
    assert np.array_equal(H, H.T)
    assert ratio <= 1


def test_eval_parity_at_large_scores(built_lib):
    """|z| up to 1e4 with theta at scale 1e3: everything finite, inside the gate."""
    from speaker_recognition_amd import calibration as cal
    X, lab, th, P = cc.big_inputs()
    f, g, H, _ = cal.evaluate(X, lab, th, prior=P)
    assert np.isfinite(f) and np.all(np.isfinite(g)) and np.all(np.isfinite(H))
    ratio = cc.worst_ratio((f, g, H), cc.evaluate(X, lab, th, P, 0.0, dtype=np.longdouble)[:3], cc.gate(X, lab, th, P, 0.0))
    print("PARITY calib eval large scores: difference / gate = %.3g" % ratio)
    assert ratio <= 1


def test_cllr_of_zero_and_of_hand_values(built_lib):
    from speaker_recognition_amd import calibration as cal
    lab = np.array([1, 1, 0, 0, -1])
    assert cal.cllr(np.zeros(5), lab) == 1.0
    assert abs(cal.cllr([np.log(3), np.log(3), -np.log(3), -np.log(3), np.nan], lab) - np.log2(4 / 3)) < 4 * cc.EPS


def test_skipped_entries_never_enter_the_arithmetic(built_lib):
    """NaN and inf at skipped positions give the same bits as 0.0 there; a block made only of skipped entries; a class of one."""
    from speaker_recognition_amd import calibration as cal
    S, n = 2, 3 * cc.BLOCK + 5
    X, lab = cc.inputs(S, n)
    X, lab = X.copy(), lab.copy()
    lab[cc.BLOCK:2 * cc.BLOCK] = -1                    # the second block holds no trial
    th = cc.parity_theta(S)
    clean = np.where(lab[None, :] < 0, 0.0, X)
    dirty = clean.copy()
    dirty[0, lab < 0] = np.nan
    dirty[1, np.flatnonzero(lab < 0)[::2]] = np.inf
    dirty[1, np.flatnonzero(lab < 0)[1::2]] = -np.inf
    a, b = cal.evaluate(clean, lab, th, prior=0.01), cal.evaluate(dirty, lab, th, prior=0.01)
    for u, v in zip(a[:3], b[:3]):
        assert np.array_equal(_bits(u), _bits(v))
    assert a[3]["skipped"] == int((lab < 0).sum()) >= cc.BLOCK
    ref = cc.evaluate(clean, lab, th, 0.01, 0.0, dtype=np.longdouble)[:3]
    assert cc.worst_ratio(a[:3], ref, cc.gate(clean, lab, th, 0.01, 0.0)) <= 1
    fa, fb = _fit(clean, lab), _fit(dirty, lab)
    assert np.array_equal(_bits(fa.theta), _bits(fb.theta)) and fa.passes == fb.passes and fa.stop == fb.stop == "CONVERGED"
    # a class with a single member
    one = np.zeros(n, dtype=np.int8)
    one[cc.BLOCK + 7] = 1
    r = cal.evaluate(clean, one, th, prior=0.3)
    assert r[3] == {"targets": 1, "non_targets": n - 1, "skipped": 0}
    assert cc.worst_ratio(r[:3], cc.evaluate(clean, one, th, 0.3, 0.0, dtype=np.longdouble)[:3], cc.gate(clean, one, th, 0.3, 0.0)) <= 1


# ---- the fit ----

def _assert_optimal(X, lab, P, lam, c, tol=1e-16):
    crit, bound = cc.optimality(X, lab, c.theta, P, lam, tol)
    print("PARITY calib fit: g^T H^-1 g = %.3g (bound %.3g), %s after %d passes, %d halvings" % (crit, bound, c.stop, c.passes, c.halvings))
    assert np.all(np.isfinite(c.theta)) and crit <= bound


@pytest.mark.parametrize("name", list(cc.FIT_CASES))
def test_fit_is_optimal_and_takes_the_restatements_passes(built_lib, name):
    """The optimality criterion at the device's theta, and passes, halvings and the stop code equal to the restatement's (the CPU
    suite asserts for each of these inputs that no decision of the loop is within rounding of going the other way)."""
    X, lab, P, lam, th0 = cc.fit_inputs(name)
    c = _fit(X, lab, P, lam, th0)
    r = cc.fit(X, lab, P, lam, th0)
    _assert_optimal(X, lab, P, lam, c)
    assert (c.stop, c.passes, c.halvings, c.accepted) == (r["stop"], r["passes"], r["halvings"], r["accepted"])
    assert c.counts["targets"] == int((lab > 0).sum())
    assert abs(float(c.objective - cc.evaluate(X, lab, c.theta, P, lam, dtype=np.longdouble)[0])) <= cc.gate(X, lab, c.theta, P, lam)["f"]
    if name == "halving":
        assert c.halvings >= 1


def test_fit_on_separable_data(built_lib):
    X, lab = cc.inputs(2, 257, separable=True)
    c = _fit(X, lab, 0.5, 1e-3)
    assert c.stop == "CONVERGED"
    _assert_optimal(X, lab, 0.5, 1e-3, c)
    c0 = _fit(X, lab, 0.5, 0.0)                        # no finite optimum: whichever code it reaches, finite weights, no exception
    assert c0.stop in cc.STOPS and np.all(np.isfinite(c0.theta)) and 1 <= c0.passes <= 100


def test_fit_of_two_identical_systems(built_lib):
    X1, lab = cc.inputs(1, 257)
    XX = np.vstack([X1, X1])
    th0 = np.array([0.25, -0.5, 0.125])
    c = _fit(XX, lab, 0.5, 0.0, th0)
    assert c.stop == "SINGULAR" and c.passes == 1 and np.array_equal(c.theta, th0)
    c = _fit(XX, lab, 0.5, 0.0)
    assert c.stop == "SINGULAR" and c.passes == 1 and np.array_equal(c.theta, np.zeros(3))
    c = _fit(XX, lab, 0.5, 1e-6)
    assert c.stop == "CONVERGED"
    _assert_optimal(XX, lab, 0.5, 1e-6, c)
    assert abs(c.weights[0] - c.weights[1]) <= cc.equal_weights_bound(XX, lab, c.theta, 0.5, 1e-6)


# ---- bit identity ----

def test_bits_do_not_depend_on_the_run_the_bound_or_a_resume(built_lib):
    from speaker_recognition_amd import _lib, calibration as cal
    S, n, P = 2, 2 * cc.BLOCK + 1, 0.01
    X, lab = cc.inputs(S, n)
    a, b = _fit(X, lab, P), _fit(X, lab, P)
    assert a.stop == "CONVERGED" and a.passes > 4
    assert np.array_equal(_bits(a._state), _bits(b._state))
    need = _lib.calib_plan(S, n)["resident_train"]
    _lib.set_option("calib_scratch_mib", -(-need // (1 << 20)))          # the smallest value that fits
    c = _fit(X, lab, P)
    _lib.set_option("calib_scratch_mib", 8192)
    assert np.array_equal(_bits(a._state), _bits(c._state))
    # max_pass = 2, then a resume with 98, equals max_pass = 100
    r = cal.Calibrator(prior=P, max_pass=2).fit(X, lab)
    assert r.stop == "CAP" and r.passes == 2
    r.max_pass = 98
    r.fit(X, lab, resume=True)
    assert r.stop == "CONVERGED" and r.passes == a.passes
    assert np.array_equal(_bits(r._state), _bits(a._state))          # the whole state, the cap (2 + 98 = 100) included
    with pytest.raises(_lib.SRError, match="ended by CAP"):
        r.fit(X, lab, resume=True)                     # a converged state cannot be resumed


def test_transform_alone_and_in_a_batch(built_lib):
    """One trial alone equals the same trial inside a batch, bit for bit; apply lies within (S + 1) eps sum |w x|."""
    from speaker_recognition_amd import calibration as cal
    for S, n in ((1, 257), (8, cc.BLOCK + 1), (3, 2 * cc.BLOCK + 77)):
        X, lab = cc.inputs(S, n)
        c = cal.Calibrator()
        c.weights, c.offset, c._stacked = cc.parity_theta(S)[:-1].copy(), 0.3, True
        z = c.transform(X)
        want, bound = cc.apply(X, c.theta)
        assert z.shape == (n,) and np.all(np.abs(z - want) <= bound)
        for i in (0, 255, 256, n - 1):
            assert np.array_equal(_bits(c.transform(X[:, i:i + 1])), _bits(z[i:i + 1]))


# ---- counts ----

def test_counts_are_exact(built_lib):
    from speaker_recognition_amd import calibration as cal
    llr, lab, thr = cc.counts_inputs()
    llr = llr.copy()
    llr[lab < 0] = np.nan                              # a skipped entry's score is never looked at
    miss, fa, counts = cal.error_counts(llr, lab, thr, return_counts=True)
    wm, wf = cc.counts(np.where(lab < 0, 0.0, llr), lab, thr)
    assert miss.dtype == np.int64 and np.array_equal(miss, wm) and np.array_equal(fa, wf)
    assert counts == {"targets": int((lab > 0).sum()), "non_targets": int((lab == 0).sum()), "skipped": int((lab < 0).sum())}
    assert miss[0] == 0 and fa[0] == counts["non_targets"] and miss[-1] == counts["targets"] and fa[-1] == 0
    m3, f3 = cal.error_counts(llr, lab, np.r_[thr, thr[:3]])          # more than 16 thresholds: two calls
    assert np.array_equal(m3, np.r_[wm, wm[:3]]) and np.array_equal(f3, np.r_[wf, wf[:3]])
    clean = np.where(lab < 0, 0.0, llr)
    assert cal.act_dcf(llr, lab, 0.5) == cc.act_dcf(clean, lab, 0.5) and cal.act_dcf(llr, lab) == cc.act_dcf(clean, lab)
    # a score exactly on the threshold is accepted
    assert [int(v[0]) for v in cal.error_counts([0.0, -1.0, 0.0, 1.0], [1, 1, 0, 0], [0.0])] == [1, 2]
    assert cal.act_dcf([0.0, -1.0, 0.0, 1.0], [1, 1, 0, 0], 0.5) == 1.5


# ---- the Python surface ----

def test_score_matrices_round_trip_their_shape(built_lib):
    from speaker_recognition_amd import _lib, calibration as cal
    rng = np.random.default_rng(11)
    key = (rng.random((5, 7)) < 0.4).astype(int)
    key[0, 0], key[4, 6], key[2, 3] = 1, 0, -1
    A = np.where(key > 0, 1.0, -1.0) + rng.standard_normal((5, 7))
    B = np.where(key > 0, 0.5, -0.5) + rng.standard_normal((5, 7))
    c = cal.Calibrator(ridge=1e-3).fit([A, B], key)
    assert c.stop == "CONVERGED" and c.weights.shape == (2,) and c.counts["skipped"] == 1
    out = c.transform([A, B])
    assert out.shape == (5, 7)
    assert np.array_equal(_bits(out), _bits(c.transform(np.stack([A, B]))))
    want, bound = cc.apply(np.stack([A.reshape(-1), B.reshape(-1)]), c.theta)
    assert np.all(np.abs(out.reshape(-1) - want) <= bound)
    one = cal.Calibrator().fit(A, key)                 # one matrix: one system
    assert one.weights.shape == (1,) and one.transform(A).shape == (5, 7)
    vec = cal.Calibrator().fit(A.reshape(-1), key.reshape(-1))
    assert np.array_equal(_bits(vec.theta), _bits(one.theta)) and vec.transform(A.reshape(-1)).shape == (35,)
    with pytest.raises(_lib.SRError, match="up to 8 systems .* S is 9"):
        cal.Calibrator().fit([A] * 9, key)
    _lib.set_option("calib_scratch_mib", 1)
    n = 1 << 17
    lab = np.zeros(n, dtype=np.int8)
    lab[::2] = 1
    with pytest.raises(_lib.SRError, match="calib_scratch_mib"):
        cal.Calibrator().fit(np.zeros(n), lab)
