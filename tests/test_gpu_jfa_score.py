"""JFA trial scoring on the device (csrc/jfa_score.hip: sr_jfa_score_integrated / _linear through jfa.score_trials, jfa.kscore_famous_19
and jfa.score_integrated) against the loop-for-loop transliterations of the reference's kscore_famous_19.m and linear_scoring.m
(tests/jfa_score_cases.py, which states the generator and derives the gates).  Every parity test asserts kappa_L <= 1e6 on the
transliteration first and prints the observed ratio (largest absolute difference / gate)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfa_cases as jc  # noqa: E402
import jfa_score_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _options(built_lib):
    from speaker_recognition_amd import _lib
    yield
    _lib.set_option("jfa_lds_rows", 0)
    _lib.set_option("jfa_scratch_mib", 1024)
    _lib.set_option("debug_verify_clean_counters", 0)


def _check_integrated(shape, path):
    from speaker_recognition_amd import _lib, jfa
    T, J, K, D, Ry, Ru = shape
    c = sc.inputs(*shape)
    assert c["ref"]["kappa"].max() <= 1e6
    assert _lib.jfa_score_plan(T, J, K, D, Ry, Ru, lds_rows=1 if path == "forced" else 0)["path"] == ("lds" if path == "lds" else "global")
    got, counts = jfa.score_trials(*sc.args(c), return_counts=True)
    assert got.shape == (J, T) and counts == {"empty_segments": 0, "bad_segments": 0}
    gate = sc.gate_integrated(shape, c["ref"])
    r = float(np.abs(got - c["ref"]["scores"]).max()) / gate
    print("jfa score integrated %s %s: difference / gate = %.3g (gate %.3g, kappa %.3g)" % (shape, path, r, gate, c["ref"]["kappa"].max()))
    assert r <= 1


@pytest.mark.parametrize("shape", sc.SHAPES[:7])
def test_integrated_parity(built_lib, shape):
    _check_integrated(shape, "lds")


def test_integrated_parity_rank_130_automatic_global_path(built_lib):
    _check_integrated(sc.SHAPES[7], "global")


@pytest.mark.parametrize("shape", [sc.SHAPES[3], sc.SHAPES[5]])          # Ru = 17 and Ru = 65
def test_integrated_parity_forced_global_memory_path(built_lib, shape):
    from speaker_recognition_amd import _lib
    _lib.set_option("jfa_lds_rows", 1)
    _check_integrated(shape, "forced")


@pytest.mark.parametrize("shape", sc.LINEAR_SHAPES)
def test_linear_parity(built_lib, shape):
    from speaker_recognition_amd import jfa
    T, J, K, D, Ry, Ru = shape
    c = sc.inputs(*shape)
    got = jfa.score_trials(*sc.args(c), x=c["x"], mode="linear")
    gate = sc.gate_linear(shape, c["linear_mag"])
    host = jfa.linear_scoring(c["F"], c["N"], None, c["m"], c["E"], c["d"], c["v"], c["u"], c["z"], c["y"], c["x"])
    r, rh = float(np.abs(got - c["linear"]).max()) / gate, float(np.abs(got - host).max()) / gate
    print("jfa score linear %s: difference / gate = %.3g against linear_scoring.m, %.3g against jfa.linear_scoring (gate %.3g)" % (shape, r, rh, gate))
    assert got.shape == (J, T) and r <= 1 and rh <= 1


def test_bit_identity_across_bounds_runs_batches_and_model_sets(built_lib):
    from speaker_recognition_amd import _lib, jfa
    shape = sc.BIG
    T, J, K, D, Ry, Ru = shape
    c = sc.inputs(*shape)
    a = sc.args(c)
    seg = (Ru * Ru + (J + 1) * Ru) * 8
    assert seg * 12 < (1 << 20) and _lib.jfa_score_plan(*shape)["n_chunks"] == 1
    first = jfa.score_trials(*a)
    assert np.array_equal(jfa.score_trials(*a), first)                               # from run to run
    # the option's smallest bound is 1 MiB, which holds all 33 segments of this shape: more models widen a segment's h block until
    # 1 MiB holds 11 segments (3 chunks); the first 17 models' scores are the same bits inside that larger set under that bound
    more = 5000
    rng = np.random.default_rng(3)
    y2, z2 = np.vstack([c["y"], rng.standard_normal((more, Ry))]), np.vstack([c["z"], 0.1 * rng.standard_normal((more, K * D))])
    _lib.set_option("jfa_scratch_mib", 1)
    assert _lib.jfa_score_plan(T, J + more, K, D, Ry, Ru, scratch_bytes=1 << 20)["n_chunks"] >= 3
    tight = jfa.score_trials(*a[:7], z2, y2)
    _lib.set_option("jfa_scratch_mib", 1024)
    wide = jfa.score_trials(*a[:7], z2, y2)
    assert np.array_equal(tight, wide) and np.array_equal(tight[:J], first)
    seg7 = jfa.score_trials(c["F"][7:8], c["N"][7:8], *a[2:])                        # segment 7 alone
    assert np.array_equal(seg7[:, 0], first[:, 7])
    pick = [3, 11]
    two = jfa.score_trials(*a[:7], c["z"][pick], c["y"][pick])                       # models {3, 11} alone
    assert np.array_equal(two, first[pick])
    _lib.set_option("jfa_lds_rows", 1)                                               # and on the global-memory factorisation's side
    g_all = jfa.score_trials(*a)
    _lib.set_option("jfa_scratch_mib", 1)
    assert np.array_equal(jfa.score_trials(*a[:7], z2, y2)[:J], g_all)
    assert np.array_equal(jfa.score_trials(c["F"][7:8], c["N"][7:8], *a[2:])[:, 0], g_all[:, 7])
    assert float(np.abs(g_all - c["ref"]["scores"]).max()) <= sc.gate_integrated(shape, c["ref"])


def test_mask_zeros_land_where_asked(built_lib):
    from speaker_recognition_amd import jfa
    shape = sc.SHAPES[2]
    T, J, K, D, Ry, Ru = shape
    c = sc.inputs(*shape)
    mask = np.random.default_rng(5).random((J, T)) < 0.6
    for kw in (dict(), dict(x=c["x"], mode="linear")):
        dense = jfa.score_trials(*sc.args(c), **kw)
        got = jfa.score_trials(*sc.args(c), mask=mask, **kw)
        assert (dense != 0.0).all()
        assert np.array_equal(got == 0.0, ~mask) and np.array_equal(got[mask], dense[mask])


def test_empty_segment_scores_zero_and_is_counted(built_lib):
    from speaker_recognition_amd import jfa
    shape = sc.SHAPES[1]
    c = sc.inputs(*shape)
    a = sc.args(c)
    F0, N0 = np.vstack([c["F"][:1], np.zeros((1, c["F"].shape[1])), c["F"][1:]]), np.vstack([c["N"][:1], np.zeros((1, c["N"].shape[1])), c["N"][1:]])
    x0 = np.vstack([c["x"][:1], np.ones((1, c["x"].shape[1])), c["x"][1:]])
    for kw, kw0 in ((dict(), dict()), (dict(x=c["x"], mode="linear"), dict(x=x0, mode="linear"))):
        dense = jfa.score_trials(*a, **kw)
        got, counts = jfa.score_trials(F0, N0, *a[2:], return_counts=True, **kw0)
        assert counts == {"empty_segments": 1, "bad_segments": 0}
        assert np.all(got[:, 1] == 0.0) and np.array_equal(np.delete(got, 1, axis=1), dense)


def test_reference_orientation_equals_score_trials(built_lib):
    from speaker_recognition_amd import jfa
    shape = sc.SHAPES[1]
    T, J, K, D, Ry, Ru = shape
    c = sc.inputs(*shape)
    F, N, m, E, d, v, u, z, y = sc.args(c)
    rows = jfa.score_trials(F, N, m, E, d, v, u, z, y)
    cols = jfa.kscore_famous_19(F.T, N.T, None, m[:, None], E[:, None], d[:, None], v.T, u.T, z.T, y.T, 0, np.ones((J, T)))
    assert np.array_equal(cols, rows)
    mask = np.array([[1, 0, 1], [0, 1, 1]])
    assert np.array_equal(jfa.kscore_famous_19(F.T, N.T, None, m, E, d, v.T, u.T, z.T, y.T, 0, mask), np.where(mask == 1, rows, 0.0))
    # absent z and d mean zeros
    zeros = jfa.score_trials(F, N, m, E, np.zeros(K * D), v, u, np.zeros((J, K * D)), y)
    assert np.array_equal(jfa.score_trials(F, N, m, E, None, v, u, None, y), zeros)
    assert np.array_equal(jfa.kscore_famous_19(F.T, N.T, None, m, E, 0, v.T, u.T, 0, y.T), zeros)


def test_score_integrated_end_to_end(built_lib):
    """train_v / train_u / train_d on (12 speakers x 3 sessions, 8 x 5, Ry 7, Ru 5), enrolment on the first sessions, the second
    sessions as test segments: score_integrated within 5 x the gate of the restated chain on the SAME trained v, u, d (the chain's
    estimators are the device's on one side and numpy's on the other, then the scorer's own error).  Observed: see DESIGN 3.5.2."""
    from speaker_recognition_amd import jfa
    G, K, D, Ry, Ru = 12, 8, 5, 7, 5
    c = jc.case(G, K, D, Ry)
    F, N, ids, m, E = c["F"], c["N"], c["spk_ids"], c["m"], c["E"]
    ubm = (np.full(K, 1.0 / K), m.reshape(K, D), E.reshape(K, D))
    v = jfa.train_v(F, N, ids, ubm, ny=Ry, niter=3)
    u = jfa.train_u(F, N, ids, ubm, v, nx=Ru, niter=2, seed=1)
    d = jfa.train_d(F, N, ids, ubm, v, u, niter=2, seed=2)
    trn, tst = (F[0::3], N[0::3]), (F[1::3], N[1::3])
    got = jfa.score_integrated(trn, {"F": tst[0], "N": tst[1]}, ubm, v, u, d)
    want, ref = sc.score_integrated(trn, tst, m, E, v, u, d)
    assert ref["kappa"].max() <= 1e6
    gate = sc.gate_integrated((G, G, K, D, Ry, Ru), ref)
    r = float(np.abs(got - want).max()) / gate
    print("jfa score_integrated end to end: difference / gate = %.3g (gate %.3g, kappa %.3g)" % (r, gate, ref["kappa"].max()))
    assert got.shape == (G, G) and r <= 5
    assert np.array_equal(got.argmax(axis=0), want.argmax(axis=0))


def test_interleaved_with_training_and_scoring_paths(built_lib):
    from speaker_recognition_amd import _lib, jfa, synth
    from speaker_recognition_amd.core import Batch, MfccExtractor, ModelSet
    from speaker_recognition_amd.pygmm import GMM
    _lib.set_option("debug_verify_clean_counters", 1)
    ex = MfccExtractor(16000, win_length_ms=25, win_shift_ms=10)
    pb = Batch.from_pcm([synth.synth_speech(s, 0.5) for s in range(3)])
    ms = ModelSet([GMM.from_arrays(*synth.synth_gmm(32, 13, 7 + s)) for s in range(4)])
    feats = ex.extract_batch(pb)
    want_score = ms.score(feats)
    fc = jc.case(12, 8, 5, 7)
    sk = sc.inputs(*sc.SHAPES[1])
    want_trials = jfa.score_trials(*sc.args(sk))
    want_linear = jfa.score_trials(*sc.args(sk), x=sk["x"], mode="linear")
    with jfa.FactorEstimator(fc["Ns"], fc["Fs"], fc["E"]) as est:
        first = est.train(fc["W0"], 2)
        assert np.array_equal(jfa.score_trials(*sc.args(sk)), want_trials)
        assert all(np.array_equal(a, b) for a, b in zip(ms.score(feats), want_score))
        assert np.array_equal(jfa.score_trials(*sc.args(sk), x=sk["x"], mode="linear"), want_linear)
        assert all(np.array_equal(a, b) for a, b in zip(est.train(fc["W0"], 2), first))
        assert np.array_equal(jfa.score_trials(*sc.args(sk)), want_trials)
        assert all(np.array_equal(a, b) for a, b in zip(ms.score(feats), want_score))
