"""The JFA factor estimation on the device (csrc/jfa.hip: sr_jfa_open / _factors / _update / _train through jfa.FactorEstimator,
jfa.update_loadings and the reference-shaped entry points of jfa.py) against the float64 restatement of tests/jfa_cases.py.

Gates, with eps = 2^-52, every difference relative to the largest magnitude of the restated array, kappa_L and kappa_A the largest
2-norm condition numbers of the restatement's L_g and A_c:
  g_y = 8 (R + K D) eps kappa_L   -- the forward error of a backward-stable solve plus the K- and K D-term sums that form L and b
                                     in another order;
  y within g_y;  A and C within 4 g_y;  the update on the restatement's own A and C within 8 R eps kappa_A;
  one full step's W within kappa_A 4 g_y + 8 R eps kappa_A;  five iterations of train within 5 x that.
Every test asserts kappa_L, kappa_A <= 1e6 on the restatement first and prints the observed ratio (difference / gate)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfa_cases as jc  # noqa: E402

pytestmark = pytest.mark.gpu

STEP_SHAPES = jc.SHAPES[:3]


@pytest.fixture(autouse=True)
def _options(built_lib):
    from speaker_recognition_amd import _lib
    yield
    _lib.set_option("jfa_lds_rows", 0)
    _lib.set_option("jfa_scratch_mib", 1024)
    _lib.set_option("debug_verify_clean_counters", 0)


def _ratio(what, got, want, gate):
    r = jc.rel(got, want) / gate
    print("jfa %s: difference / gate = %.3g (gate %.3g)" % (what, r, gate))
    return r


def _conditioned(*kappas):
    assert all(k <= 1e6 for k in kappas), kappas


def _check_factors(shape, path):
    from speaker_recognition_amd import _lib, jfa
    G, K, D, R = shape
    c = jc.case(*shape)
    _conditioned(c["kL"], c["kA"])
    assert _lib.jfa_plan(G, K, D, R, lds_rows=_LDS.get(path, 0))["path"] == ("lds" if path == "lds" else "global")
    with jfa.FactorEstimator(c["Ns"], c["Fs"], c["E"]) as est:
        y_only = est.factors(c["W0"])
        y, A, C = est.factors(c["W0"], accumulate=True)
        assert est.bad_groups == 0
    assert y.shape == (G, R) and A.shape == (K, R, R) and C.shape == (R, K * D)
    assert np.array_equal(y, y_only)                                   # the accumulators do not change y
    assert np.array_equal(A, np.swapaxes(A, 1, 2))                     # symmetric to the bit
    gy = jc.gate_y(R, K, D, c["kL"])
    tag = "%s %s" % (shape, path)
    assert _ratio("y " + tag, y, c["y"], gy) <= 1
    assert _ratio("A " + tag, A, c["A"], 4 * gy) <= 1
    assert _ratio("C " + tag, C, c["C"], 4 * gy) <= 1


_LDS = {"lds": 0, "global": 1}


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 4, 13, 3), (5, 5, 1, 16), (33, 17, 39, 17), (2, 65, 13, 16), (5, 4, 13, 65),
                                   (33, 65, 39, 65)])
def test_factors_parity(built_lib, shape):
    _check_factors(shape, "lds")


@pytest.mark.parametrize("shape", [(33, 17, 39, 17), (5, 4, 13, 65)])
def test_factors_parity_global_memory_path(built_lib, shape):
    from speaker_recognition_amd import _lib
    _lib.set_option("jfa_lds_rows", 1)
    _check_factors(shape, "global")


def test_factors_parity_rank_130_automatic_path(built_lib):
    _check_factors((5, 3, 13, 130), "auto")


@pytest.mark.parametrize("shape", STEP_SHAPES)
def test_update_alone(built_lib, shape):
    from speaker_recognition_amd import jfa
    G, K, D, R = shape
    c = jc.case(*shape)
    _conditioned(c["kL"], c["kA"])
    W, skipped = jfa.update_loadings(c["A"], c["C"], c["W0"], return_skipped=True)
    assert skipped == 0
    assert _ratio("update %s" % (shape,), W, c["W1"], jc.gate_update(R, c["kA"])) <= 1


@pytest.mark.parametrize("shape", STEP_SHAPES)
def test_one_full_step(built_lib, shape):
    from speaker_recognition_amd import jfa
    G, K, D, R = shape
    c = jc.case(*shape)
    _conditioned(c["kL"], c["kA"])
    with jfa.FactorEstimator(c["Ns"], c["Fs"], c["E"]) as est:
        y, A, C = est.factors(c["W0"], accumulate=True)
        W_train, y_train = est.train(c["W0"], 1)
    W = jfa.update_loadings(A, C, c["W0"])
    assert _ratio("step %s" % (shape,), W, c["W1"], jc.gate_step(R, K, D, c["kL"], c["kA"])) <= 1
    assert np.array_equal(W, W_train) and np.array_equal(y, y_train)


@pytest.mark.parametrize("shape", STEP_SHAPES)
def test_train_five_iterations(built_lib, shape):
    from speaker_recognition_amd import jfa
    G, K, D, R = shape
    c = jc.case(*shape, n_iter=5)
    _conditioned(c["kL_train"], c["kA_train"])
    Ns, Fs, E = c["Ns"], c["Fs"], c["E"]
    with jfa.FactorEstimator(Ns, Fs, E) as est:
        W, y = est.train(c["W0"], 5)
        assert est.skipped == 0
        # the same bits as five chained factors + update calls
        Wc, Js = np.array(c["W0"]), [jc.objective(Ns, Fs, E, c["W0"])]
        for _ in range(5):
            yc, A, C = est.factors(Wc, accumulate=True)
            Wc = jfa.update_loadings(A, C, Wc)
            Js.append(jc.objective(Ns, Fs, E, Wc))
    assert np.array_equal(W, Wc) and np.array_equal(y, yc)
    gate = 5 * jc.gate_step(R, K, D, c["kL_train"], c["kA_train"])
    assert _ratio("train W %s" % (shape,), W, c["W_train"], gate) <= 1
    assert _ratio("train y %s" % (shape,), y, c["y_train"], gate) <= 1
    # the objective of the device-trained W never decreases
    steps = np.diff(Js)
    print("jfa train %s: objective %s, smallest step %.3g" % (shape, ["%.6g" % j for j in Js], steps.min()))
    assert all(s >= -1e-9 * abs(j) for s, j in zip(steps, Js[1:]))


def test_independent_of_batch_bound_and_run(built_lib):
    from speaker_recognition_amd import _lib, jfa
    shape = (70, 5, 39, 65)
    G, K, D, R = shape
    c = jc.case(*shape)
    Ns, Fs, E, W0 = c["Ns"], c["Fs"], c["E"], c["W0"]
    assert _lib.jfa_plan(G, K, D, R, 1 << 20)["n_chunks"] == 5 and _lib.jfa_plan(G, K, D, R)["n_chunks"] == 1
    with jfa.FactorEstimator(Ns, Fs, E) as est:
        first = est.factors(W0, accumulate=True)
        again = est.factors(W0, accumulate=True)
        _lib.set_option("jfa_scratch_mib", 1)
        tight = est.factors(W0, accumulate=True)
        tight_train = est.train(W0, 2)
        _lib.set_option("jfa_scratch_mib", 1024)
        wide_train = est.train(W0, 2)
    for a, b, t in zip(first, again, tight):
        assert np.array_equal(a, b) and np.array_equal(a, t)            # two runs; under a bound that forces five chunks
    assert all(np.array_equal(a, b) for a, b in zip(tight_train, wide_train))
    for g in (0, 17, 69):                                               # a group alone: the bits of its row inside the batch
        with jfa.FactorEstimator(Ns[g:g + 1], Fs[g:g + 1], E) as est:
            assert np.array_equal(est.factors(W0)[0], first[0][g])
    _lib.set_option("jfa_lds_rows", 1)                                  # and on the global-memory factorisation
    with jfa.FactorEstimator(Ns, Fs, E) as est:
        yg = est.factors(W0)
    with jfa.FactorEstimator(Ns[17:18], Fs[17:18], E) as est:
        assert np.array_equal(est.factors(W0)[0], yg[17])
    assert jc.rel(yg, c["y"]) <= jc.gate_y(R, K, D, c["kL"])


def test_all_zero_group_and_unoccupied_mixture(built_lib):
    from speaker_recognition_amd import jfa
    shape = (12, 8, 5, 7)
    G, K, D, R = shape
    c = jc.case(*shape)
    Ns, Fs, E, W0 = c["Ns"], c["Fs"], c["E"], c["W0"]
    with jfa.FactorEstimator(Ns, Fs, E) as est:
        y, A, C = est.factors(W0, accumulate=True)
    with jfa.FactorEstimator(np.vstack([Ns, np.zeros((1, K))]), np.vstack([Fs, np.zeros((1, K * D))]), E) as est:
        y0, A0, C0 = est.factors(W0, accumulate=True)
        assert est.bad_groups == 0
    assert np.all(y0[G] == 0.0) and np.array_equal(y0[:G], y)           # y = 0 exactly,
    assert np.array_equal(A0, A) and np.array_equal(C0, C)              # and A and C do not see the group
    # a mixture nobody occupies: A_c = 0 does not factor, its columns stay, the others move as the restatement's
    Nz, Fz = np.array(Ns), np.array(Fs)
    Nz[:, 3] = 0.0
    Fz[:, 3 * D:4 * D] = 0.0
    yr, Ar, Cr = jc.factors(Nz, Fz, E, W0)
    Wr, skipped_r = jc.update(Ar, Cr, W0)
    kL, kA = jc.cond_L(Nz, E, W0), jc.cond_A(Ar)
    _conditioned(kL, kA)
    assert skipped_r == 1 and not Ar[3].any()
    with jfa.FactorEstimator(Nz, Fz, E) as est:
        W, _ = est.train(W0, 1)
        assert est.skipped == 1
    assert np.array_equal(W[:, 3 * D:4 * D], W0[:, 3 * D:4 * D])
    assert _ratio("step with an unoccupied mixture", W, Wr, jc.gate_step(R, K, D, kL, kA)) <= 1
    Wu, sk = jfa.update_loadings(Ar, Cr, W0, return_skipped=True)
    assert sk == 1 and np.array_equal(Wu[:, 3 * D:4 * D], W0[:, 3 * D:4 * D])


def _sessions_case():
    """(12, 8, 5, 7) with its three sessions per speaker, and non-zero u, x, z, d."""
    G, K, D, R = 12, 8, 5, 7
    c = jc.case(G, K, D, R)
    rng = np.random.default_rng(77)
    kd, n = K * D, len(c["spk_ids"])
    extra = dict(v=c["W0"], u=jc.random_start(3, c["E"], 5), x=0.3 * rng.standard_normal((n, 3)), z=0.1 * rng.standard_normal((G, kd)),
                 d=0.05 * rng.random(kd) + 0.01, y=0.3 * rng.standard_normal((G, R)))
    return c, extra, (G, K, D, R)


def test_estimate_y_and_v_three_forms(built_lib):
    from speaker_recognition_amd import jfa
    c, e, (G, K, D, R) = _sessions_case()
    F, N, ids, m, E = c["F"], c["N"], c["spk_ids"], c["m"], c["E"]
    args = (F, N, None, m, E, e["d"], e["v"], e["u"], e["z"], 0, e["x"], ids)
    yr, Ar, Cr = jc.estimate_y_and_v(*args, nargout=3)
    _, vr = jc.estimate_y_and_v(*args, nargout=2)
    Ns = np.zeros((G, K))
    np.add.at(Ns, ids, N)
    kL, kA = jc.cond_L(Ns, E, e["v"]), jc.cond_A(Ar)
    _conditioned(kL, kA)
    gy = jc.gate_y(R, K, D, kL)
    y1 = jfa.estimate_y_and_v(*args)
    y2, v2 = jfa.estimate_y_and_v(*args, nargout=2)
    y3, A3, C3 = jfa.estimate_y_and_v(*args, nargout=3)
    assert np.array_equal(y1, y2) and np.array_equal(y1, y3)
    assert _ratio("estimate_y_and_v y", y1, yr, gy) <= 1
    assert _ratio("estimate_y_and_v A", A3, Ar, 4 * gy) <= 1 and _ratio("estimate_y_and_v C", C3, Cr, 4 * gy) <= 1
    assert _ratio("estimate_y_and_v v", v2, vr, jc.gate_step(R, K, D, kL, kA)) <= 1
    assert _ratio("estimate_y_and_v(A, C)", jfa.estimate_y_and_v(Ar, Cr), jc.update(Ar, Cr, np.zeros_like(vr))[0], jc.gate_update(R, kA)) <= 1
    # labels with a gap, scalar-0 arguments as the sc_* scripts pass them
    gap = np.where(ids >= 4, ids + 2, ids)
    yg = jfa.estimate_y_and_v(F, N, None, m, E, 0, e["v"], 0, np.zeros((G + 2, 1)), 0, np.zeros((len(ids), 1)), gap)
    yp = jc.estimate_y_and_v(F, N, None, m, E, 0, e["v"], 0, 0, 0, 0, ids)
    assert yg.shape == (G + 2, R) and not yg[4:6].any() and jc.rel(np.delete(yg, (4, 5), axis=0), yp) <= gy


def test_estimate_x_and_u_three_forms(built_lib):
    from speaker_recognition_amd import jfa
    c, e, (G, K, D, R) = _sessions_case()
    F, N, ids, m, E = c["F"], c["N"], c["spk_ids"], c["m"], c["E"]
    Rx = e["u"].shape[0]
    args = (F, N, None, m, E, e["d"], e["v"], e["u"], e["z"], e["y"], 0, ids)
    xr, Ar, Cr = jc.estimate_x_and_u(*args, nargout=3)
    _, ur = jc.estimate_x_and_u(*args, nargout=2)
    kL, kA = jc.cond_L(N, E, e["u"]), jc.cond_A(Ar)
    _conditioned(kL, kA)
    gx = jc.gate_y(Rx, K, D, kL)
    x1 = jfa.estimate_x_and_u(*args)
    x2, u2 = jfa.estimate_x_and_u(*args, nargout=2)
    x3, A3, C3 = jfa.estimate_x_and_u(*args, nargout=3)
    assert x1.shape == (len(ids), Rx) and np.array_equal(x1, x2) and np.array_equal(x1, x3)
    assert _ratio("estimate_x_and_u x", x1, xr, gx) <= 1
    assert _ratio("estimate_x_and_u A", A3, Ar, 4 * gx) <= 1 and _ratio("estimate_x_and_u C", C3, Cr, 4 * gx) <= 1
    assert _ratio("estimate_x_and_u u", u2, ur, jc.gate_step(Rx, K, D, kL, kA)) <= 1
    # z and d: host float64 on both sides
    zargs = (F, N, None, m, E, e["d"], e["v"], e["u"], 0, e["y"], e["x"], ids)
    zr, dr = jc.estimate_z_and_d(*zargs, nargout=2)
    z2, d2 = jfa.estimate_z_and_d(*zargs, nargout=2)
    print("jfa z %.3g d %.3g (relative; gate 1e-12)" % (jc.rel(z2, zr), jc.rel(d2, dr)))
    assert jc.rel(z2, zr) <= 1e-12 and jc.rel(d2, dr) <= 1e-12


def test_score_dot_product_end_to_end(built_lib):
    from speaker_recognition_amd import jfa
    c, e, (G, K, D, R) = _sessions_case()
    F, N, m, E = c["F"], c["N"], c["m"], c["E"]
    trn, tst = (F[0:18:3], N[0:18:3]), (F[1:27:3], N[1:27:3])           # 6 enrolment and 9 test segments
    ubm = (np.full(K, 1.0 / K), m.reshape(K, D), E.reshape(K, D))
    want = jc.score_dot_product(trn, tst, m, E, e["v"], e["u"], e["d"])
    got = jfa.score_dot_product(trn, tst, ubm, e["v"], e["u"], e["d"])
    print("jfa scores: %.3g relative (gate 1e-12)" % jc.rel(got, want))
    assert got.shape == (6, 9) and jc.rel(got, want) <= 1e-12
    assert np.array_equal(got.argmax(axis=0), want.argmax(axis=0))


def test_from_pcm_to_scores(built_lib):
    """PCM -> MFCC -> statistics on the device -> train_v / train_u / train_d -> score_dot_product; the restated chain runs on the
    same N and F."""
    import bw_cases as bc
    from speaker_recognition_amd import jfa, synth
    from speaker_recognition_amd.core import Batch, MfccExtractor
    ex = MfccExtractor(16000, win_length_ms=25, win_shift_ms=10)
    n_spk, K, D = 6, 8, 13
    pcm = []
    for s in range(n_spk):
        p = synth.synth_speech(s, 1.2)
        pcm += [p[:len(p) // 2], p[len(p) // 2:]]
    ids = np.repeat(np.arange(n_spk), 2)
    feats = ex.extract_batch(Batch.from_pcm(pcm))
    assert feats.dim == D
    ubm = bc.make_ubm(K, D, 23)
    ubm = (ubm[0], ubm[1] * 0.3, ubm[2])               # (CMVN features: unit variance around 0)
    N, F = jfa.compute_suf_stats(feats, ubm)
    m, E = ubm[1].reshape(-1), ubm[2].reshape(-1)
    v = jfa.train_v(F, N, ids, ubm, ny=3, niter=3)
    u = jfa.train_u(F, N, ids, ubm, v, nx=2, niter=2, seed=1)
    d = jfa.train_d(F, N, ids, ubm, v, u, niter=2, seed=2)
    scores = jfa.score_dot_product((F[0::2], N[0::2]), (F[1::2], N[1::2]), ubm, v, u, d)
    vr = jc.train_v(F, N, ids, m, E, 3, 3)
    ur = jc.train_u(F, N, ids, m, E, vr, 2, 2, seed=1)
    dr = jc.train_d(F, N, ids, m, E, vr, ur, 2, seed=2)
    want = jc.score_dot_product((F[0::2], N[0::2]), (F[1::2], N[1::2]), m, E, vr, ur, dr)
    print("jfa from PCM: v %.3g u %.3g d %.3g scores %.3g (relative)" % (jc.rel(v, vr), jc.rel(u, ur), jc.rel(d, dr), jc.rel(scores, want)))
    assert scores.shape == (n_spk, n_spk) and np.isfinite(scores).all()
    assert np.array_equal(scores.argmax(axis=0), want.argmax(axis=0))


def test_interleaved_with_scoring_paths(built_lib):
    from speaker_recognition_amd import _lib, jfa, synth
    from speaker_recognition_amd.core import Batch, MfccExtractor, ModelSet
    from speaker_recognition_amd.pygmm import GMM
    _lib.set_option("debug_verify_clean_counters", 1)
    ex = MfccExtractor(16000, win_length_ms=25, win_shift_ms=10)
    pb = Batch.from_pcm([synth.synth_speech(s, 0.5) for s in range(3)])
    ms = ModelSet([GMM.from_arrays(*synth.synth_gmm(32, 13, 7 + s)) for s in range(4)])
    feats = ex.extract_batch(pb)
    want = {"score": ms.score(feats), "fused": ex.predict_batch(ms, pb)}
    c = jc.case(12, 8, 5, 7)
    with jfa.FactorEstimator(c["Ns"], c["Fs"], c["E"]) as est:
        first = est.train(c["W0"], 2)

        def same(got, key):
            assert all(np.array_equal(a, b) for a, b in zip(got, want[key])), key

        def factor():
            assert all(np.array_equal(a, b) for a, b in zip(est.train(c["W0"], 2), first))

        same(ms.score(feats), "score")
        factor()
        same(ex.predict_batch(ms, pb), "fused")
        factor()
        same(ms.score(feats), "score")
