"""Score normalisation on the device (csrc/score_norm.hip through scorenorm.normalise / select_cohort, jfa.score_normalised) against
the float64 numpy restatement written from the definitions (tests/scorenorm_cases.py, which states the generator, the mutants and
derives the gate).  The selection is checked integer for integer; every parity case asserts the conditions the gate rests on (no
degenerate pair, rho and q under their ceilings) and prints its worst figure as a PARITY line before asserting."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bw_cases as bw  # noqa: E402
import jfa_cases as jc  # noqa: E402
import scorenorm_cases as nc  # noqa: E402

pytestmark = pytest.mark.gpu
LIMIT = 16384


@pytest.fixture(autouse=True)
def _options(built_lib):
    from speaker_recognition_amd import _lib
    yield
    _lib.set_option("norm_scratch_mib", 1024)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- the selection, exact ----

@pytest.mark.parametrize("C", [2, 63, 64, 65, 255, 256, 257, 1025, LIMIT])
def test_selection_indices_equal_the_restatement(built_lib, C):
    """Mixed signs, all-negative values, denormals, ties straddling the N-th place (quantised values), a constant row, -0.0 among
    +0.0, magnitudes over 600 decades and values that differ in one byte of the key only (one row per radix pass), at top_n = 2,
    C - 1, C and C + 5: the indices equal the restatement's integer for integer, the moments of the regular rows lie within the
    gate, a row the restatement calls degenerate has sigma 0.0 exactly."""
    from speaker_recognition_amd import scorenorm as sn
    names, X = nc.selection_rows(C)
    for top_n in sorted({n for n in (2, C - 1, C, C + 5) if n >= 2}):
        idx, mu, sg = sn.select_cohort(X, top_n)
        assert idx.shape == (len(names), min(top_n, C)) and idx.dtype == np.int64
        worst, worst_row = 0.0, ""
        for r, name in enumerate(names):
            want = nc.top_idx(X[r], top_n)
            assert np.array_equal(idx[r], want), (C, top_n, name)
            m, s, bad = nc.moments_shifted(X[r][want])
            if bad:
                assert sg[r] == 0.0, (C, top_n, name, sg[r])
                continue
            rho = float(np.abs(X[r][want] - X[r][want[0]]).max()) / s
            g = nc.gate(len(want), rho, 0.0)
            ratio = max(abs(mu[r] - m) / (g * s + 2 * nc.EPS * abs(m)), abs(sg[r] - s) / (g * s))
            if ratio > worst:
                worst, worst_row = ratio, name
        const = names.index("constant")
        assert sg[const] == 0.0 and mu[const] == 0.75
        print("PARITY scorenorm select C=%d top_n=%d: moments difference / gate = %.3g (row %r)" % (C, top_n, worst, worst_row))
        assert worst <= 1


def test_selection_refuses_a_cohort_above_the_built_limit(built_lib):
    from speaker_recognition_amd import _lib, scorenorm as sn
    assert _lib.score_norm_plan("z", 1, 1, LIMIT, 0)["max_C"] == LIMIT
    with pytest.raises(_lib.SRError, match="up to 16384 members .* C is 16385; thin the cohort"):
        sn.select_cohort(np.zeros((1, LIMIT + 1)), 2)
    with pytest.raises(_lib.SRError, match="Cz is 16385"):
        sn.znorm(np.zeros((1, 1)), np.zeros((1, LIMIT + 1)))


def test_a_batch_of_300_rows_equals_each_row_alone(built_lib):
    from speaker_recognition_amd import scorenorm as sn
    rng = np.random.default_rng(11)
    X = rng.standard_normal((300, 257))
    X[::3] = np.round(X[::3] * 2) / 2                                   # every third row quantised: ties at the threshold
    idx, mu, sg = sn.select_cohort(X, 40)
    again = sn.select_cohort(X, 40)
    assert np.array_equal(idx, again[0]) and np.array_equal(_bits(mu), _bits(again[1])) and np.array_equal(_bits(sg), _bits(again[2]))
    for r in range(300):
        i1, m1, s1 = sn.select_cohort(X[r:r + 1], 40)
        assert np.array_equal(i1[0], idx[r]) and _bits(m1)[0] == _bits(mu)[r] and _bits(s1)[0] == _bits(sg)[r], r
        assert np.array_equal(idx[r], nc.top_idx(X[r], 40))


# ---- every mode against the restatement ----

def _normalise(mode, c, **over):
    from speaker_recognition_amd import scorenorm as sn
    a = dict(c, **over)
    return sn.normalise(a["S"], mode, a["Ez"] if mode != "t" else None, a["Tt"] if mode != "z" else None, a["Zt"] if mode == "zt" else None,
                        top_n=a["top_n"] if mode in ("as1", "as2") else None, return_counts=True)


@pytest.mark.parametrize("case", nc.PARITY_CASES)
def test_every_mode_against_the_restatement(built_lib, case):
    J, T, Cn, off = case
    c = nc.inputs(*case)
    for mode in nc.MODES:
        r = nc.reference(J, T, Cn, off, mode)
        assert r["degenerate_enrol"] == 0 and r["degenerate_test"] == 0 and r["rho"] <= nc.RHO_MAX and r["q"] <= nc.Q_MAX
        got, counts = _normalise(mode, c)
        g = nc.gate(Cn, r["rho"], r["q"])
        ratio = float(np.abs(got - r["out"]).max()) / g
        print("PARITY scorenorm %s J=%d T=%d C=%d offset=%g: difference / gate = %.3g (gate %.3g, rho %.3g, q %.3g)"
              % (mode, J, T, Cn, off, ratio, g, r["rho"], r["q"]))
        assert got.shape == (J, T) and counts == {"degenerate_enrol": 0, "degenerate_test": 0}
        assert ratio <= 1, (mode, case)


def test_wrappers_are_normalise(built_lib):
    from speaker_recognition_amd import scorenorm as sn
    c = nc.inputs(17, 63, 37, 0.0)
    S, Ez, Tt, Zt, n = c["S"], c["Ez"], c["Tt"], c["Zt"], c["top_n"]
    for mode, got in (("z", sn.znorm(S, Ez)), ("t", sn.tnorm(S, Tt)), ("zt", sn.ztnorm(S, Ez, Tt, Zt)), ("s", sn.snorm(S, Ez, Tt)),
                      ("as1", sn.asnorm(S, Ez, Tt, n, variant=1)), ("as2", sn.asnorm(S, Ez, Tt, n))):
        assert np.array_equal(_bits(got), _bits(_normalise(mode, c)[0])), mode
    # top_n >= C selects everything: as1 is s, to the bit
    assert np.array_equal(_bits(sn.asnorm(S, Ez, Tt, 37, variant=1)), _bits(sn.snorm(S, Ez, Tt)))
    assert np.array_equal(_bits(sn.asnorm(S, Ez, Tt, 1000, variant=1)), _bits(sn.snorm(S, Ez, Tt)))


def test_as2_does_not_depend_on_the_scratch_bound(built_lib):
    """1 MiB holds the fixed 3 x 64 x 257 doubles and 79 of the 200 test segments: three chunks.  The same bits as in one chunk, and
    from run to run."""
    from speaker_recognition_amd import _lib
    J, T, Cn = 64, 200, 257
    c = nc.inputs(J, T, Cn, 300.0)
    assert _lib.score_norm_plan("as2", J, T, Cn, Cn, c["top_n"], scratch_bytes=1 << 20)["n_chunks"] >= 3
    assert _lib.score_norm_plan("as2", J, T, Cn, Cn, c["top_n"], scratch_bytes=1 << 30)["n_chunks"] == 1
    wide, wc = _normalise("as2", c)
    _lib.set_option("norm_scratch_mib", 1)
    tight, tc = _normalise("as2", c)
    again, _ = _normalise("as2", c)
    _lib.set_option("norm_scratch_mib", 1024)
    assert np.array_equal(_bits(tight), _bits(wide)) and np.array_equal(_bits(tight), _bits(again)) and tc == wc
    assert np.array_equal(_bits(_normalise("as2", c)[0]), _bits(wide))
    r = nc.restate("as2", c["S"], c["Ez"], c["Tt"], None, c["top_n"])
    ratio = float(np.abs(wide - r["out"]).max()) / nc.gate(Cn, r["rho"], r["q"])
    print("PARITY scorenorm as2 J=%d T=%d C=%d three chunks: difference / gate = %.3g" % (J, T, Cn, ratio))
    assert ratio <= 1 and r["rho"] <= nc.RHO_MAX and r["q"] <= nc.Q_MAX


@pytest.mark.parametrize("mode", nc.MODES)
def test_degenerate_pairs_give_exact_zeros_and_are_counted(built_lib, mode):
    """Model 3's cohort row is constant: its row of the result is 0.0 exactly, the counter equals the restatement's, and every other
    row is the same bits as in the run without that model.  (In t, which reads no Ez, a constant column of Tt does the same on the test side.)"""
    J, T, Cn = 17, 15, 37
    c = dict(nc.inputs(J, T, Cn, 0.0))
    Ez, Tt = np.array(c["Ez"]), np.array(c["Tt"])
    Ez[3] = 0.1                                                          # 0.1 x 37 / 37 is not 0.1 in float64: the variance must still be 0 exactly
    dense, _ = _normalise(mode, c)
    if mode == "t":
        Tt[:, 5] = -2.5
        got, counts = _normalise(mode, c, Tt=Tt)
        want = nc.restate(mode, c["S"], c["Ez"], Tt, c["Zt"], c["top_n"])
        assert counts == {"degenerate_enrol": 0, "degenerate_test": 1} == {k: want[k] for k in counts}
        assert (got[:, 5] == 0.0).all() and np.array_equal(_bits(np.delete(got, 5, axis=1)), _bits(np.delete(dense, 5, axis=1)))
        return
    got, counts = _normalise(mode, c, Ez=Ez)
    want = nc.restate(mode, c["S"], Ez, c["Tt"], c["Zt"], c["top_n"])
    assert counts == {k: want[k] for k in counts} and counts["degenerate_enrol"] == (T if mode == "as2" else 1) and counts["degenerate_test"] == 0
    assert (got[3] == 0.0).all() and not np.signbit(got[3]).any() and np.isfinite(got).all()
    assert np.array_equal(got == 0.0, want["out"] == 0.0)
    keep = np.arange(J) != 3
    alone, ac = _normalise(mode, c, S=c["S"][keep], Ez=c["Ez"][keep])
    assert ac == {"degenerate_enrol": 0, "degenerate_test": 0}
    assert np.array_equal(_bits(got[keep]), _bits(alone)) and np.array_equal(_bits(got[keep]), _bits(dense[keep]))


def test_as2_selected_set_constant_in_a_row_that_is_not(built_lib):
    """The case as2 counts pairs for: Ez[j0, I_t0] is one value while Ez[j0, :] is not, and Tt[I_j1, t1] likewise.  About the row's
    mean the four products leave fl(d^2) - d^2 for such a set, the rounding error of one multiplication, of either sign: the pair's
    moments then come from the values themselves.  Exactly those trials are 0.0, the pair counts are the restatement's, every other
    trial lies within the gate."""
    J, T, Cn = 17, 15, 37
    c = dict(nc.inputs(J, T, Cn, 300.0))
    n = c["top_n"]
    Ez, Tt = np.array(c["Ez"]), np.array(c["Tt"])
    j0, t0, j1, t1 = 4, 6, 11, 2
    Ez[j0, nc.top_idx(Tt[:, t0], n)] = 300.625
    Tt[nc.top_idx(Ez[j1], n), t1] = 298.75
    want = nc.restate("as2", c["S"], Ez, Tt, None, n)
    assert want["degenerate_enrol"] >= 1 and want["degenerate_test"] >= 1 and want["out"][j0, t0] == 0.0 and want["out"][j1, t1] == 0.0
    assert Ez[j0].max() > Ez[j0].min() and Tt[:, t1].max() > Tt[:, t1].min()
    got, counts = _normalise("as2", c, Ez=Ez, Tt=Tt)
    assert counts == {k: want[k] for k in counts}, (counts, want["degenerate_enrol"], want["degenerate_test"])
    assert np.array_equal(got == 0.0, want["out"] == 0.0) and got[j0, t0] == 0.0 and got[j1, t1] == 0.0 and np.isfinite(got).all()
    ratio = float(np.abs(got - want["out"]).max()) / nc.gate(Cn, want["rho"], want["q"])
    print("PARITY scorenorm as2 constant selected sets: difference / gate = %.3g (rho %.3g, q %.3g)" % (ratio, want["rho"], want["q"]))
    assert ratio <= 1 and want["rho"] <= nc.RHO_MAX and want["q"] <= nc.Q_MAX


@pytest.mark.parametrize("top_n", [2, 3])
def test_as2_on_quantised_cohort_scores(built_lib, top_n):
    """Floored cohort scores: ties among the few values the other side's selection picks make many selected sets constant in rows
    that are not, on both sides, at an offset of 300.  The zeros and both pair counts equal the restatement's."""
    J, T, Cn = 17, 15, 37
    rng = np.random.default_rng(77 + top_n)
    S = rng.standard_normal((J, T)) + 300.0
    Ez, Tt = np.floor(1.5 * rng.standard_normal((J, Cn))) + 300.0, np.floor(1.5 * rng.standard_normal((Cn, T))) + 300.0
    want = nc.restate("as2", S, Ez, Tt, None, top_n)
    assert want["degenerate_enrol"] >= 10 and want["degenerate_test"] >= 10 and (want["out"] != 0.0).sum() >= 100
    got, counts = _normalise("as2", dict(S=S, Ez=Ez, Tt=Tt, top_n=top_n))
    assert counts == {k: want[k] for k in counts}, (counts, want["degenerate_enrol"], want["degenerate_test"])
    assert np.array_equal(got == 0.0, want["out"] == 0.0) and np.isfinite(got).all()
    ratio = float(np.abs(got - want["out"]).max()) / nc.gate(Cn, want["rho"], want["q"])
    print("PARITY scorenorm as2 quantised top_n=%d: %d + %d degenerate pairs, difference / gate = %.3g" %
          (top_n, counts["degenerate_enrol"], counts["degenerate_test"], ratio))
    assert ratio <= 1


def test_as2_nearly_constant_selected_set_keeps_its_digits(built_lib):
    """A selected set 1e-9 wide, 1 away from its row's mean: the products' variance is rounding noise there (1e-18 of the mean
    square), so the pair goes through the values themselves and comes out as the shifted two-pass form gives it (the restatement's
    own mean-relative form is good to 1e-7 only at this width: the enrolment side's moments are taken by moments_shifted here)."""
    J, T, Cn = 17, 15, 37
    c = dict(nc.inputs(J, T, Cn, 0.0))
    n = c["top_n"]
    Ez = np.array(c["Ez"])
    j0, t0 = 4, 6
    It = nc.top_idx(c["Tt"][:, t0], n)
    Ez[j0, It] = 0.625 + 1e-9 * np.arange(n)
    got, counts = _normalise("as2", c, Ez=Ez)
    me, se, bad = nc.moments_shifted(Ez[j0, It])
    mt, st, _ = nc.moments(c["Tt"][nc.top_idx(Ez[j0], n), t0])
    s = c["S"][j0, t0]
    want = 0.5 * ((s - me) / se + (s - mt) / st)
    rho, q = float(np.abs(Ez[j0, It] - Ez[j0, It[0]]).max()) / se, abs(s - me) / se
    g = nc.gate(n, rho, q)
    print("PARITY scorenorm as2 nearly constant set: difference / gate = %.3g (value %.3g, gate %.3g)" % (abs(got[j0, t0] - want) / g, want, g))
    assert not bad and counts == {"degenerate_enrol": 0, "degenerate_test": 0} and abs(want) > 1e7
    assert abs(got[j0, t0] - want) <= g


# ---- through the scorers ----

def test_score_normalised_equals_normalise_of_the_scorers_matrices(built_lib):
    """The golden 256 x 13 UBM, 35 synthetic sessions (6 enrolment, 9 test, 20 cohort), Ry = Ru = 3: jfa.score_normalised is
    scorenorm.normalise applied to the matrices the existing scorers return, bit for bit, with either scorer, from host arrays and
    from a resident jfa.Stats."""
    from speaker_recognition_amd import jfa, scorenorm as sn
    ubm = bw.fixture_ubm()
    K, D, R = 256, 13, 3
    c = jc.corpus(35, K, D, R, 5, sessions=1, ubm=ubm)
    rng = np.random.default_rng(9)
    F, N = c["F"], c["N"]
    v, u, d = c["v_true"], rng.normal(0.0, 0.1, (R, K * D)), rng.uniform(0.05, 0.2, K * D)
    cuts = (slice(0, 6), slice(6, 15), slice(15, 35))

    def check(trn, tst, coh, what):
        for scorer, score in (("integrated", jfa.score_integrated), ("dot_product", jfa.score_dot_product)):
            S, Ez, Tt, Zt = (score(a, b, ubm, v, u, d) for a, b in ((trn, tst), (trn, coh), (coh, tst), (coh, coh)))
            assert S.shape == (6, 9) and Ez.shape == (6, 20) and Tt.shape == (20, 9) and Zt.shape == (20, 20)
            for norm, kw in (("as2", dict(top_n=5)), ("as1", dict(top_n=5)), ("zt", dict()), ("z", dict())):
                got = jfa.score_normalised(trn, tst, coh, ubm, v, u, d, norm=norm, scorer=scorer, **kw)
                want = sn.normalise(S, norm, Ez, Tt, Zt if norm == "zt" else None, **kw)
                assert got.shape == (6, 9) and np.isfinite(got).all() and (got != 0.0).all(), (what, scorer, norm)
                assert np.array_equal(_bits(got), _bits(want)), (what, scorer, norm)
            ref = nc.restate("as2", S, Ez, Tt, None, 5)
            assert np.abs(jfa.score_normalised(trn, tst, coh, ubm, v, u, d, top_n=5, scorer=scorer) - ref["out"]).max() <= nc.gate(20, ref["rho"], ref["q"])

    check(*[(F[s], N[s]) for s in cuts], "host arrays")
    with jfa.Stats.from_arrays(N, F) as st:
        with st.take(np.arange(0, 6)) as trn, st.take(np.arange(6, 15)) as tst, st.take(np.arange(15, 35)) as coh:
            check(trn, tst, coh, "resident statistics")
    with pytest.raises(ValueError, match="scorer is"):
        jfa.score_normalised((F[:2], N[:2]), (F[:2], N[:2]), (F[:4], N[:4]), ubm, v, u, d, scorer="x")


def test_llr_matrix_and_znorm_of_a_map_speaker_set(built_lib):
    """The GMM-UBM leg through the same normaliser: three MAP speakers and their UBM score five test and twelve impostor
    utterances (ModelSet.score), llr_matrix turns the sums into per-frame ratios against the UBM column, znorm normalises them."""
    from speaker_recognition_amd import scorenorm as sn, synth
    from speaker_recognition_amd.core import Batch, ModelSet
    from speaker_recognition_amd.pygmm import GMM
    ubm = synth.synth_gmm(32, 13, 7)
    spk = [synth.synth_map_speaker(ubm, 20 + s) for s in range(3)]
    ms = ModelSet([GMM.from_arrays(*m) for m in spk + [ubm]])
    test = [synth.draw_frames(spk[s % 3], 150 + 10 * s, 40 + s) for s in range(5)]
    imp = [synth.draw_frames(synth.synth_map_speaker(ubm, 60 + s), 120 + 7 * s, 80 + s) for s in range(12)]
    S = sn.llr_matrix(ms.score(Batch.from_features(test))[0], [len(x) for x in test])
    Ez = sn.llr_matrix(ms.score(Batch.from_features(imp))[0], [len(x) for x in imp])
    assert S.shape == (3, 5) and Ez.shape == (3, 12)
    got, counts = sn.znorm(S, Ez, return_counts=True)
    r = nc.restate("z", S, Ez=Ez)
    ratio = float(np.abs(got - r["out"]).max()) / nc.gate(12, r["rho"], r["q"])
    print("PARITY scorenorm llr_matrix + znorm: difference / gate = %.3g (rho %.3g, q %.3g)" % (ratio, r["rho"], r["q"]))
    assert counts == {"degenerate_enrol": 0, "degenerate_test": 0} and ratio <= 1
    assert np.array_equal(got.argmax(axis=0), np.arange(5) % 3)          # every test utterance is its speaker's
