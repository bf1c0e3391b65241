"""The resident JFA route on the device (csrc/jfa_stats.hip through jfa.Stats, jfa.centred, FactorEstimator.z_and_d and the
scorers on a handle): statistics that stay on the device from the Baum-Welch pass to the score matrix, against the host-array
route bit for bit where the same kernels run on the same numbers, and against the float64 restatements (tests/jfa_cases.py,
tests/jfa_resident_cases.py) by their derived gates elsewhere."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bw_cases as bc  # noqa: E402
import jfa_cases as jc  # noqa: E402
import jfa_resident_cases as rc  # noqa: E402
import jfa_score_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _options(built_lib):
    from speaker_recognition_amd import _lib
    yield
    _lib.set_option("jfa_lds_rows", 0)
    _lib.set_option("jfa_scratch_mib", 1024)
    _lib.set_option("bw_scratch_mib", 1024)
    _lib.set_option("bw_range_frames", 0)
    _lib.set_option("debug_verify_clean_counters", 0)


def _ratio(what, got, want, gate):
    r = jc.rel(got, want) / gate
    print("jfa resident %s: difference / gate = %.3g (gate %.3g)" % (what, r, gate))
    return r


def _conditioned(*kappas):
    assert all(k <= 1e6 for k in kappas), kappas


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.mark.parametrize("K,D", [(17, 13), (65, 39)])
def test_resident_pass_is_the_batched_pass(built_lib, K, D):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch, ModelSet
    from speaker_recognition_amd.pygmm import GMM
    ubm = bc.make_ubm(K, D, 5)
    utts = [bc.draw(ubm, T, 40 + i) for i, T in enumerate((0, 1, 127, 129, 1025, 2100))]
    feats = Batch.from_features([u.astype(np.float32).reshape(-1, D) for u in utts])
    ms = ModelSet([GMM.from_arrays(ubm[0], ubm[1], np.sqrt(ubm[2]))])
    lengths = [len(u) for u in utts]
    _lib.set_option("bw_range_frames", 16)             # many small ranges: 1 MiB of slabs is several groups at either shape
    for mib in (1024, 1):
        _lib.set_option("bw_scratch_mib", mib)
        groups = _lib.bw_plan(K, D, lengths, 16, mib << 20)["n_groups"]
        assert (groups > 1) == (mib == 1), groups
        N, F, ll, dropped = ms.bw_stats(feats, 0, ll=True)
        stats, ll_r, dropped_r = ms.bw_stats(feats, 0, ll=True, resident=True)
        with stats:
            assert (stats.n, stats.K, stats.D) == (6, K, D)
            Nr, Fr = stats.get()
        assert np.array_equal(Nr, N) and np.array_equal(Fr, F) and np.array_equal(ll_r, ll) and np.array_equal(dropped_r, dropped)
        assert not Nr[0].any() and Nr[1:].any()


def test_from_arrays_get_take_and_the_handle_refusals(built_lib):
    from speaker_recognition_amd import _lib, jfa
    L = built_lib
    c = rc.case(*rc.CENTRING[1])
    N, F, ids, m, E = c["N"], c["F"], c["ids"], c["m"], c["E"]
    n, kd = F.shape
    with jfa.Stats.from_arrays(N, F) as st:
        assert (st.n, st.K, st.D, len(st)) == (n, c["K"], c["D"], n)
        Ng, Fg = st.get()
        assert np.array_equal(Ng, N) and np.array_equal(Fg, F)
        rows = np.array([5, 0, 5, n - 1, 3, 3, 3])
        with st.take(rows) as sub:
            a, b = sub.get()
            assert sub.n == len(rows) and np.array_equal(a, N[rows]) and np.array_equal(b, F[rows])
        with st.take(ids == ids[0]) as sub:
            assert np.array_equal(sub.get()[1], F[ids == ids[0]])
        # the refusals that need a live handle: by their texts, and none of them names the device
        h = st._handle()
        bad_rows = np.array([0, n], dtype=np.int64)
        assert L.sr_stats_take(h, bad_rows.ctypes.data_as(C.POINTER(C.c_int64)), 2) is None
        assert re.search(r"rows\[1\] is %d, the handle holds sessions 0 .. %d" % (n, n - 1), _lib.last_error())

        def refused(pat, mode=0, ids=ids, n_labels=c["n_labels"], d=None, z=None, v=None, Ry=0, y=None, u=None, Ru=0, x=None, E=E):
            opt = lambda a: _dp(a) if a is not None else None                        # noqa: E731
            got = L.sr_jfa_open_centred(h, _dp(E), _dp(m), mode, ids.ctypes.data_as(C.POINTER(C.c_int64)), n_labels, opt(d), opt(z), opt(v), Ry,
                                        opt(y), opt(u), Ru, opt(x))
            err = _lib.last_error()
            assert got is None and re.search(pat, err) and "HIP" not in err, err

        top = int(np.argmax(ids))                      # the first session of the largest label
        refused(r"ids\[%d\] is %d, outside 0 .. n_labels - 1 = %d" % (top, ids[top], ids[top] - 1), n_labels=int(ids[top]))
        refused(r"ids\[3\] is -1", ids=np.where(np.arange(n) == 3, -1, ids))
        refused("the mode is 0", mode=2)
        refused("d \\[K D\\] and z .* come together", d=np.array(c["d"]))
        refused("v .* and y .* come together", v=np.array(c["v"]), Ry=c["Ry"])
        refused("u .* and x .* come together", x=np.array(c["x"]), Ru=c["Ru"])
        refused("Ru is 513", u=np.zeros((513, kd)), x=np.zeros((n, 513)), Ru=513)
        refused("Ry is 0", v=np.array(c["v"]), y=np.array(c["y"]), Ry=0)
        refused("E must be positive, element 2", E=np.where(np.arange(kd) == 2, 0.0, E))
        refused("x holds a non-finite value at element 1", u=np.array(c["u"]), Ru=c["Ru"], x=np.where(np.arange(n * c["Ru"]) == 1, np.nan, c["x"].ravel()))
        _lib.set_option("jfa_scratch_mib", 1)
        big = np.zeros((1, 200000))                    # one row of the x u product is 1.6 MB: the bound of 1 MiB is below one chunk
        with jfa.Stats.from_arrays(np.ones((1, 1)), big) as wide:
            with pytest.raises(_lib.SRError, match="below one chunk .* raise the option jfa_scratch_mib"):
                jfa.centred(wide, np.zeros(200000), np.ones(200000), [0], u=np.ones((1, 200000)), x=np.ones((1, 1)))
        _lib.set_option("jfa_scratch_mib", 1024)
        # the Python layer: an E of another size, labels of another length
        with pytest.raises(ValueError, match="expected E of shape"):
            jfa.centred(st, m, E[:-1], ids)
        with pytest.raises(ValueError, match="0-based integer labels"):
            jfa.centred(st, m, E, ids[:-1])
        # on another device than the calling thread's
        _lib.lib().sr_set_thread_device(1)
        try:
            assert L.sr_stats_get(h, _dp(Ng), _dp(Fg)) == -1
            assert "lives on device 0, the calling thread is on device 1" in _lib.last_error() and "HIP" not in _lib.last_error()
        finally:
            _lib.lib().sr_set_thread_device(0)
    # closed: every call refuses by its text; closing again is harmless
    assert L.sr_stats_get(h, _dp(Ng), _dp(Fg)) == -1 and "the statistics handle is closed" in _lib.last_error()
    L.sr_stats_close(h)
    with pytest.raises(_lib.SRError, match="the statistics are closed"):
        st.get()
    # a NaN in what a resident pass would leave is met when the handle is made, not later: the host check has the same texts
    with pytest.raises(_lib.SRError, match="F holds a non-finite value at element 7"):
        jfa.Stats.from_arrays(N, np.where(np.arange(F.size).reshape(F.shape) == 7, np.nan, F))


@pytest.mark.parametrize("shape", rc.CENTRING)
def test_centring_parity(built_lib, shape):
    """Both groupings, every combination of the three optional terms, read back through sr_jfa_statistics."""
    from speaker_recognition_amd import jfa
    c = rc.case(*shape)
    worst = 0.0
    with jfa.Stats.from_arrays(c["N"], c["F"]) as st:
        for groups in ("speakers", "sessions"):
            for zd, yv, xu in rc.TERMS:
                kw = rc.terms(c, zd, yv, xu)
                Ng, want, S, n_g = rc.centre(c, groups, np.float64, **kw)
                with jfa.centred(st, c["m"], c["E"], c["ids"], groups, **kw) as est:
                    N_got, Fc_got = est.statistics()
                    assert est.G == len(Ng) and np.array_equal(est.present, np.unique(c["ids"]))
                assert np.array_equal(N_got, Ng), (groups, zd, yv, xu)               # plain adds in session order
                r = rc.worst_ratio(Fc_got, want, rc.gate(c, n_g, S, yv, xu))
                worst = max(worst, r)
                assert r <= 1.0, (groups, zd, yv, xu, r)
    print("jfa resident centring %s: worst difference / gate = %.3g" % (shape, worst))


def _bits_case():
    """70 speakers x 3 sessions x (17 x 39): the x u product is 1.1 MB, so a bound of 1 MiB cuts it."""
    c = jc.corpus(70, 17, 39, 5, 4242, sessions=3)
    rng = np.random.default_rng(5)
    perm = rng.permutation(210)
    return dict(F=np.ascontiguousarray(c["F"][perm]), N=np.ascontiguousarray(c["N"][perm]), ids=c["spk_ids"][perm].astype(np.int64), m=c["m"],
                E=c["E"], u=rng.normal(0.0, 0.3, (5, 17 * 39)), x=0.3 * rng.standard_normal((210, 5)), v=rng.normal(0.0, 0.3, (4, 17 * 39)),
                y=rng.standard_normal((70, 4)))


def test_bits_do_not_depend_on_bound_run_or_batch(built_lib):
    from speaker_recognition_amd import _lib, jfa
    c = _bits_case()
    assert _lib.jfa_centre_plan(210, 70, 17, 39, 4, 5, "speakers", 1 << 20)["n_chunks"] > 1
    assert _lib.jfa_centre_plan(210, 70, 17, 39, 4, 5, "speakers", 1 << 30)["n_chunks"] == 1
    kw = dict(u=c["u"], x=c["x"], v=c["v"], y=c["y"])
    with jfa.Stats.from_arrays(c["N"], c["F"]) as st:
        for groups in ("speakers", "sessions"):
            got = []
            for mib in (1024, 1024, 1):
                _lib.set_option("jfa_scratch_mib", mib)
                with jfa.centred(st, c["m"], c["E"], c["ids"], groups, **kw) as est:
                    got.append(est.statistics())
            _lib.set_option("jfa_scratch_mib", 1024)
            for N2, F2 in got[1:]:
                assert np.array_equal(N2, got[0][0]) and np.array_equal(F2, got[0][1]), groups
        # one speaker's sessions alone, taken into a handle of their own (they straddle the chunk boundary or not: the same bits)
        with jfa.centred(st, c["m"], c["E"], c["ids"], "speakers", **kw) as est:
            N_all, Fc_all = est.statistics()
        for spk in (0, 33, 69):
            rows = np.flatnonzero(c["ids"] == spk)
            with st.take(rows) as sub:
                with jfa.centred(sub, c["m"], c["E"], np.zeros(len(rows), dtype=np.int64), "speakers", u=c["u"], x=c["x"][rows], v=c["v"],
                                 y=c["y"][spk:spk + 1]) as est:
                    N1, Fc1 = est.statistics()
            assert np.array_equal(N1[0], N_all[spk]) and np.array_equal(Fc1[0], Fc_all[spk]), spk


def _sessions_case():
    """(12, 8, 5, 7) with its three sessions per speaker, and non-zero u, x, z, d (as tests/test_gpu_jfa.py)."""
    G, K, D, R = 12, 8, 5, 7
    c = jc.case(G, K, D, R)
    rng = np.random.default_rng(77)
    kd, n = K * D, len(c["spk_ids"])
    extra = dict(v=c["W0"], u=jc.random_start(3, c["E"], 5), x=0.3 * rng.standard_normal((n, 3)), z=0.1 * rng.standard_normal((G, kd)),
                 d=0.05 * rng.random(kd) + 0.01, y=0.3 * rng.standard_normal((G, R)))
    return c, extra, (G, K, D, R)


def test_factors_and_training_downstream_of_a_centred_handle(built_lib):
    from speaker_recognition_amd import jfa
    shape = (40, 17, 13, 17)
    G, K, D, R = shape
    c = jc.case(*shape, n_iter=3)
    _conditioned(c["kL"], c["kA"], c["kL_train"], c["kA_train"])
    F, N, ids, m, E = c["F"], c["N"], c["spk_ids"], c["m"], c["E"]
    ubm = (np.full(K, 1.0 / K), m.reshape(K, D), E.reshape(K, D))
    gy = jc.gate_y(R, K, D, c["kL"])
    with jfa.Stats.from_arrays(N, F) as st:
        with jfa.centred(st, m, E, ids) as est:
            y, A, Cm = est.factors(c["W0"], accumulate=True)
        assert _ratio("factors y", y, c["y"], gy) <= 1 and _ratio("factors A", A, c["A"], 4 * gy) <= 1 and _ratio("factors C", Cm, c["C"], 4 * gy) <= 1
        v = jfa.train_v(st, None, ids, ubm, ny=R, niter=3, v0=c["W0"])
        assert _ratio("train_v", v, c["W_train"], 3 * jc.gate_step(R, K, D, c["kL_train"], c["kA_train"])) <= 1
        # train_u: two iterations on the sessions, y fixed from the restated v
        vr = np.array(c["W_train"])
        yr = jc.estimate_y_and_v(F, N, None, m, E, 0, vr, 0, 0, 0, 0, ids)
        Fh = F - np.repeat(N, D, axis=1) * (m + yr @ vr)[ids]
        u0 = jc.random_start(5, E, 1)
        ur, _, trace = jc.train(N, Fh, E, u0, 2)
        kL = max(jc.cond_L(N, E, W) for W in [u0] + trace[:-1])
        kA = max(jc.cond_A(jc.factors(N, Fh, E, W)[1]) for W in [u0] + trace[:-1])
        _conditioned(kL, kA)
        u = jfa.train_u(st, None, ids, ubm, vr, nx=5, niter=2, seed=1)
        assert _ratio("train_u", u, ur, 2 * jc.gate_step(5, K, D, kL, kA)) <= 1


def test_estimate_entry_points_with_a_stats(built_lib):
    from speaker_recognition_amd import jfa
    c, e, (G, K, D, R) = _sessions_case()
    F, N, ids, m, E = c["F"], c["N"], c["spk_ids"], c["m"], c["E"]
    Ns = np.zeros((G, K))
    np.add.at(Ns, ids, N)
    with jfa.Stats.from_arrays(N, F) as st:
        args = (None, m, E, e["d"], e["v"], e["u"], e["z"], 0, e["x"], ids)
        yr, Ar, Cr = jc.estimate_y_and_v(F, N, *args, nargout=3)
        _, vr = jc.estimate_y_and_v(F, N, *args, nargout=2)
        kL, kA = jc.cond_L(Ns, E, e["v"]), jc.cond_A(Ar)
        _conditioned(kL, kA)
        gy = jc.gate_y(R, K, D, kL)
        y1 = jfa.estimate_y_and_v(st, None, *args)
        y2, v2 = jfa.estimate_y_and_v(st, None, *args, nargout=2)
        y3, A3, C3 = jfa.estimate_y_and_v(st, None, *args, nargout=3)
        assert y1.shape == yr.shape and np.array_equal(y1, y2) and np.array_equal(y1, y3)
        assert _ratio("estimate_y_and_v y", y1, yr, gy) <= 1
        assert _ratio("estimate_y_and_v A", A3, Ar, 4 * gy) <= 1 and _ratio("estimate_y_and_v C", C3, Cr, 4 * gy) <= 1
        assert _ratio("estimate_y_and_v v", v2, vr, jc.gate_step(R, K, D, kL, kA)) <= 1
        # labels with a gap, scalar-0 arguments and columns of zeros as the sc_* scripts pass them
        gap = np.where(ids >= 4, ids + 2, ids)
        yg = jfa.estimate_y_and_v(st, None, None, m, E, 0, e["v"], 0, np.zeros((G + 2, 1)), 0, np.zeros((len(ids), 1)), gap)
        yp = jc.estimate_y_and_v(F, N, None, m, E, 0, e["v"], 0, 0, 0, 0, ids)
        assert yg.shape == (G + 2, R) and not yg[4:6].any() and jc.rel(np.delete(yg, (4, 5), axis=0), yp) <= gy
        Rx = e["u"].shape[0]
        args = (None, m, E, e["d"], e["v"], e["u"], e["z"], e["y"], 0, ids)
        xr, Ar, Cr = jc.estimate_x_and_u(F, N, *args, nargout=3)
        _, ur = jc.estimate_x_and_u(F, N, *args, nargout=2)
        kL, kA = jc.cond_L(N, E, e["u"]), jc.cond_A(Ar)
        _conditioned(kL, kA)
        gx = jc.gate_y(Rx, K, D, kL)
        x1 = jfa.estimate_x_and_u(st, None, *args)
        x2, u2 = jfa.estimate_x_and_u(st, None, *args, nargout=2)
        x3, A3, C3 = jfa.estimate_x_and_u(st, None, *args, nargout=3)
        assert x1.shape == (len(ids), Rx) and np.array_equal(x1, x2) and np.array_equal(x1, x3)
        assert _ratio("estimate_x_and_u x", x1, xr, gx) <= 1
        assert _ratio("estimate_x_and_u A", A3, Ar, 4 * gx) <= 1 and _ratio("estimate_x_and_u C", C3, Cr, 4 * gx) <= 1
        assert _ratio("estimate_x_and_u u", u2, ur, jc.gate_step(Rx, K, D, kL, kA)) <= 1


def test_z_and_d_on_both_kinds_of_handle(built_lib):
    from speaker_recognition_amd import jfa
    c, e, (G, K, D, R) = _sessions_case()
    F, N, ids, m, E = c["F"], c["N"], c["spk_ids"], c["m"], c["E"]
    kd = K * D
    zargs = (None, m, E, e["d"], e["v"], e["u"], 0, e["y"], e["x"], ids)
    zr, ar, br = jc.estimate_z_and_d(F, N, *zargs, nargout=3)
    d3 = np.array(e["d"])
    for _ in range(3):
        d3 = jc.estimate_z_and_d(F, N, None, m, E, d3, e["v"], e["u"], 0, e["y"], e["x"], ids, nargout=2)[1]
    # the statistics jfa.py's host route would upload through sr_jfa_open
    Nx = np.repeat(N, D, axis=1)
    Ns, Fs = np.zeros((G, K)), np.zeros((G, kd))
    np.add.at(Ns, ids, N)
    np.add.at(Fs, ids, F - (e["x"] @ e["u"]) * Nx)
    Fs -= (m + e["y"] @ e["v"]) * np.repeat(Ns, D, axis=1)
    with jfa.Stats.from_arrays(N, F) as st:
        handles = (jfa.centred(st, m, E, ids, "speakers", v=e["v"], u=e["u"], y=e["y"], x=e["x"]), jfa.FactorEstimator(Ns, Fs, E))
        for kind, est in zip(("centred", "opened"), handles):
            with est:
                d_in = np.array(e["d"])
                z0, d0, a0, b0 = est.z_and_d(d_in, n_iter=0, want_z=True)
                assert np.array_equal(d0, e["d"]) and np.array_equal(d_in, e["d"])           # n_iter = 0 leaves d untouched
                z1, d1, a1, b1 = est.z_and_d(e["d"], n_iter=1, want_z=True)
                assert np.array_equal(z1, z0) and np.array_equal(a1, a0) and np.array_equal(b1, b0) and np.array_equal(d1, b0 / a0)
                d_3, a_3, b_3 = est.z_and_d(e["d"], n_iter=3)
                print("jfa resident z / d (%s): z %.3g a %.3g b %.3g d3 %.3g (relative; gates 1e-12, 1e-11)"
                      % (kind, jc.rel(z0, zr), jc.rel(a0, ar), jc.rel(b0, br), jc.rel(d_3, d3)))
                assert jc.rel(z0, zr) <= 1e-12 and jc.rel(a0, ar) <= 1e-12 and jc.rel(b0, br) <= 1e-12
                assert jc.rel(d_3, d3) <= 1e-11
        # and through the reference-shaped entry point and the driver
        z2, d2 = jfa.estimate_z_and_d(st, None, *zargs, nargout=2)
        assert z2.shape == zr.shape and jc.rel(z2, zr) <= 1e-12 and jc.rel(d2, br / ar) <= 1e-12


@pytest.mark.parametrize("shape", [sc.SHAPES[1], sc.SHAPES[3], sc.SHAPES[5]])
def test_scorers_on_a_handle_give_the_host_array_bits(built_lib, shape):
    from speaker_recognition_amd import _lib, jfa
    T, J, K, D, Ry, Ru = shape
    c = sc.inputs(*shape)
    N, F = np.array(c["N"]), np.array(c["F"])
    if T > 1:
        N[T // 2] = 0.0                                # a segment of no frames
        F[T // 2] = 0.0
    mask = (np.arange(J * T).reshape(J, T) % 3 != 0)
    a = sc.args(c, F=F, N=N)
    with jfa.Stats.from_arrays(N, F) as st:
        for lds_rows in ((0, 1) if shape == sc.SHAPES[1] else (0,)):
            _lib.set_option("jfa_lds_rows", lds_rows)
            for mode in ("integrated", "linear"):
                for mk in (None, mask):
                    want, wc = jfa.score_trials(*a, x=c["x"], mode=mode, mask=mk, return_counts=True)
                    got, gc = jfa.score_trials(st, None, *a[2:], x=c["x"], mode=mode, mask=mk, return_counts=True)
                    assert np.array_equal(got, want) and gc == wc, (mode, mk is not None, lds_rows)
                    assert gc["empty_segments"] == (1 if T > 1 else 0)
        _lib.set_option("jfa_lds_rows", 0)
        # kscore_famous_19 and linear_scoring take the handle too
        k = jfa.kscore_famous_19(st, None, None, c["m"], c["E"], c["d"], c["v"].T, c["u"].T, c["z"].T, c["y"].T)
        assert np.array_equal(k, jfa.score_trials(*a, mode="integrated"))
        lin = jfa.linear_scoring(st, None, None, c["m"], c["E"], c["d"], c["v"], c["u"], c["z"], c["y"], c["x"])
        assert np.array_equal(lin, jfa.score_trials(*a, x=c["x"], mode="linear"))


def test_from_pcm_to_scores_resident(built_lib, monkeypatch):
    """PCM -> MFCC -> resident statistics -> train_v / train_u / train_d -> score_dot_product and score_integrated on taken halves;
    the restated chain and the host-array route run on the same N and F.  The statistics never come home on the way."""
    from speaker_recognition_amd import _lib, jfa, synth
    from speaker_recognition_amd.core import Batch, MfccExtractor
    ex = MfccExtractor(16000, win_length_ms=25, win_shift_ms=10)
    n_spk, K, D = 6, 8, 13
    pcm = []
    for s in range(n_spk):
        p = synth.synth_speech(s, 1.2)
        pcm += [p[:len(p) // 2], p[len(p) // 2:]]
    ids = np.repeat(np.arange(n_spk), 2)
    feats = ex.extract_batch(Batch.from_pcm(pcm))
    ubm = bc.make_ubm(K, D, 23)
    ubm = (ubm[0], ubm[1] * 0.3, ubm[2])               # (CMVN features: unit variance around 0)
    m, E = ubm[1].reshape(-1), ubm[2].reshape(-1)
    N, F = jfa.compute_suf_stats(feats, ubm)
    called = []

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            called.append(name)
            return getattr(self._lib, name)

    monkeypatch.setattr(_lib, "_lib", Spy(_lib.lib()))
    with jfa.compute_suf_stats(feats, ubm, resident=True) as st:
        v = jfa.train_v(st, None, ids, ubm, ny=3, niter=3)
        u = jfa.train_u(st, None, ids, ubm, v, nx=2, niter=2, seed=1)
        d = jfa.train_d(st, None, ids, ubm, v, u, niter=2, seed=2)
        with st.take(np.arange(0, 2 * n_spk, 2)) as trn, st.take(np.arange(1, 2 * n_spk, 2)) as tst:
            dot = jfa.score_dot_product(trn, tst, ubm, v, u, d)
            integ = jfa.score_integrated(trn, tst, ubm, v, u, d)
    assert "sr_stats_get" not in called and "sr_bw_stats_resident" in called and "sr_jfa_open_centred" in called and "sr_jfa_zd" in called
    monkeypatch.undo()
    halves = ((F[0::2], N[0::2]), (F[1::2], N[1::2]))
    vh = jfa.train_v(F, N, ids, ubm, ny=3, niter=3)
    uh = jfa.train_u(F, N, ids, ubm, vh, nx=2, niter=2, seed=1)
    dh = jfa.train_d(F, N, ids, ubm, vh, uh, niter=2, seed=2)
    dot_h, integ_h = jfa.score_dot_product(*halves, ubm, vh, uh, dh), jfa.score_integrated(*halves, ubm, vh, uh, dh)
    vr = jc.train_v(F, N, ids, m, E, 3, 3)
    ur = jc.train_u(F, N, ids, m, E, vr, 2, 2, seed=1)
    dr = jc.train_d(F, N, ids, m, E, vr, ur, 2, seed=2)
    dot_r = jc.score_dot_product(*halves, m, E, vr, ur, dr)
    integ_r = sc.score_integrated(*halves, m, E, vr, ur, dr)[0]
    print("jfa resident from PCM: v %.3g u %.3g d %.3g dot %.3g integrated %.3g (relative to the restated chain)"
          % (jc.rel(v, vr), jc.rel(u, ur), jc.rel(d, dr), jc.rel(dot, dot_r), jc.rel(integ, integ_r)))
    assert dot.shape == integ.shape == (n_spk, n_spk) and np.isfinite(dot).all() and np.isfinite(integ).all()
    assert np.array_equal(dot.argmax(axis=0), dot_r.argmax(axis=0)) and np.array_equal(dot.argmax(axis=0), dot_h.argmax(axis=0))
    assert np.array_equal(integ.argmax(axis=0), integ_r.argmax(axis=0)) and np.array_equal(integ.argmax(axis=0), integ_h.argmax(axis=0))


def test_interleaved_with_scoring_and_training_and_lifetime(built_lib):
    from speaker_recognition_amd import _lib, jfa, synth
    from speaker_recognition_amd.core import Batch, MfccExtractor, ModelSet
    from speaker_recognition_amd.pygmm import GMM
    _lib.set_option("debug_verify_clean_counters", 1)
    ex = MfccExtractor(16000, win_length_ms=25, win_shift_ms=10)
    pb = Batch.from_pcm([synth.synth_speech(s, 0.5) for s in range(3)])
    ms = ModelSet([GMM.from_arrays(*synth.synth_gmm(32, 13, 7 + s)) for s in range(4)])
    feats = ex.extract_batch(pb)
    want = {"score": ms.score(feats), "fused": ex.predict_batch(ms, pb)}
    c = rc.case(*rc.CENTRING[1])
    kw = rc.terms(c, True, True, True)
    W0 = jc.random_start(4, c["E"], 3)
    st = jfa.Stats.from_arrays(c["N"], c["F"])
    est = jfa.centred(st, c["m"], c["E"], c["ids"], "speakers", **kw)
    first_stats = est.statistics()
    st.close()                                         # the centred handle owns its arrays: it lives on
    first = est.train(W0, 2)
    first_zd = est.z_and_d(c["d"], n_iter=2)

    def same(got, key):
        assert all(np.array_equal(a, b) for a, b in zip(got, want[key])), key

    def resident():
        with jfa.Stats.from_arrays(c["N"], c["F"]) as s2, jfa.centred(s2, c["m"], c["E"], c["ids"], "speakers", **kw) as e2:
            assert all(np.array_equal(a, b) for a, b in zip(e2.statistics(), first_stats))
        assert all(np.array_equal(a, b) for a, b in zip(est.statistics(), first_stats))
        assert all(np.array_equal(a, b) for a, b in zip(est.train(W0, 2), first))
        assert all(np.array_equal(a, b) for a, b in zip(est.z_and_d(c["d"], n_iter=2), first_zd))

    same(ms.score(feats), "score")
    resident()
    same(ex.predict_batch(ms, pb), "fused")
    resident()
    ubm = bc.make_ubm(8, 13, 23)
    with jfa.compute_suf_stats(feats, ubm, resident=True) as s3:
        a = s3.get()
    assert all(np.array_equal(x, y) for x, y in zip(a, jfa.compute_suf_stats(feats, ubm)))
    same(ms.score(feats), "score")
    resident()
    est.close()
