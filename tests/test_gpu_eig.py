"""The symmetric eigen-solver (csrc/eig.hip), the generalised problem, LDA and the diagonalised PLDA scorer (csrc/backend_eig.hip)
on the device, through plda.sym_eig / gen_eig / LDA / PLDA.diagonalise / DiagPLDA, against LAPACK and the float64 numpy restatements
(tests/eig_cases.py, tests/plda_cases.py, which state the generators and derive the gates).  Every parity case prints its worst
figure as a PARITY line before asserting."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bw_cases as bw  # noqa: E402
import eig_cases as ec  # noqa: E402
import jfa_cases as jc  # noqa: E402
import plda_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _options(built_lib):
    from speaker_recognition_amd import _lib
    yield
    _lib.set_option("plda_scratch_mib", 1024)
    _lib.set_option("jfa_lds_rows", 0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _parity(what, case, diff, gate):
    ratio = diff / gate
    print("PARITY eig %s %s: difference / gate = %.3g (gate %.3g)" % (what, case, ratio, gate))
    return ratio


def _block():
    from speaker_recognition_amd import _lib
    return _lib.eig_plan(200)["b"]


# ---- the solver ----

@pytest.mark.parametrize("size", ec.SHAPES, ids=ec.SHAPE_IDS)
def test_the_solver_meets_the_gates_on_every_input(built_lib, size):
    from speaker_recognition_amd import plda
    b = _block()
    R = ec.shape(size, b)                              # (the sizes follow the plan's block width)
    worst = 0.0
    for kind in ec.KINDS:
        A = ec.matrix(kind, R)
        w, V, info = plda.sym_eig(A, return_info=True)
        sweeps = info["sweeps"]
        print("eig sweeps %s R=%d: %d" % (kind, R, sweeps))
        assert info["converged"] == 1 and sweeps <= ec.MAX_SWEEPS, (kind, info)
        if kind != "multiple" or R <= 2 * b:
            assert sweeps <= ec.SEPARATED_SWEEPS, (kind, sweeps)
        assert np.all(np.diff(w) <= 0), kind                                            # descending
        assert np.array_equal(_bits(V), _bits(ec.fix_signs(V))), kind                    # the sign convention
        ev, res, orth = ec.figures(A, w, V)
        g = ec.gate(R, sweeps)
        worst = max(worst, _parity("eigenvalues %s" % kind, R, ev, g), _parity("residual %s" % kind, R, res, g),
                    _parity("orthogonality %s" % kind, R, orth, g))
    assert worst <= 1


@pytest.mark.parametrize("R", (3, 65, 113))
def test_eigenvectors_equal_lapacks_where_the_gaps_are_prescribed(built_lib, R):
    from speaker_recognition_amd import plda
    A = ec.matrix("gapped", R)
    w, V, info = plda.sym_eig(A, return_info=True)
    w_ref, V_ref = ec.reference(A)
    assert info["converged"] == 1
    rel_gap = 1.0 / R                                  # eigenvalues R .. 1: every gap 1 of |A|_2 = R
    assert _parity("eigenvectors", R, float(np.max(np.abs(V - V_ref))), ec.gate(R, info["sweeps"]) / rel_gap) <= 1
    assert _parity("eigenvalues gapped", R, float(np.max(np.abs(w - w_ref))) / R, ec.gate(R, info["sweeps"])) <= 1


def test_the_same_bits_from_run_to_run(built_lib):
    from speaker_recognition_amd import plda
    for R in (33, 97, 200):
        A = ec.matrix("spd1e6", R)
        first = plda.sym_eig(A)
        plda.sym_eig(ec.matrix("indefinite", 65))      # (another size in between: the work arrays are shared)
        again = plda.sym_eig(A)
        assert np.array_equal(_bits(first[0]), _bits(again[0])) and np.array_equal(_bits(first[1]), _bits(again[1])), R
    up = np.triu(ec.matrix("spd10", 65), 1) * 1e-12     # the lower triangle is what is read
    assert np.array_equal(_bits(plda.sym_eig(ec.matrix("spd10", 65) + up)[0]), _bits(plda.sym_eig(ec.matrix("spd10", 65))[0]))


# ---- the generalised problem ----

@pytest.mark.parametrize("R", ec.GEN_R)
def test_gen_eig_diagonalises_both_covariances(built_lib, R):
    from speaker_recognition_amd import plda
    c = pc.score_case(R, 1, 1)                         # (the model of a scoring case: Sb and Sw of condition 10)
    Sb, Sw = c["Sb"], c["Sw"]
    kappa = float(np.linalg.cond(Sw))
    assert kappa <= pc.KAPPA_MAX
    psi, V, info = plda.gen_eig(Sb, Sw, return_info=True)
    assert info["status"] == 0 and np.all(np.diff(psi) <= 0)
    g = kappa * ec.gate(R, info["sweeps"])
    psi_ref = np.linalg.eigvalsh(ec.restated_M(Sb, Sw))[::-1]
    r1 = _parity("gen_eig V^T Sw V", R, float(np.max(np.abs(V.T @ Sw @ V - np.eye(R)))), g)
    r2 = _parity("gen_eig V^T Sb V", R, float(np.max(np.abs(V.T @ Sb @ V - np.diag(psi)))) / float(np.max(np.abs(psi_ref))), g)
    r3 = _parity("gen_eig psi", R, pc.rel(psi, psi_ref), g)
    assert max(r1, r2, r3) <= 1


def test_an_sw_that_does_not_factor_gives_status_1_and_zeros(built_lib):
    from speaker_recognition_amd import plda
    c = pc.score_case(17, 64, 65)
    Sw = np.array(c["Sw"])
    Sw[2, 2] = -1.0
    psi, V, info = plda.gen_eig(c["Sb"], Sw, return_info=True)
    assert info["status"] == 1 and not psi.any() and not V.any()
    with pytest.raises(ArithmeticError, match="Sw did not factor"):
        plda.gen_eig(c["Sb"], Sw)
    psi, V = plda.gen_eig(c["Sb"], c["Sw"])            # and the library goes on working
    assert np.isfinite(V).all() and psi[0] > 0


# ---- LDA ----

@pytest.mark.parametrize("case", ec.LDA_CASES, ids=["R%d-%dclasses" % (R, len(c)) for R, c in ec.LDA_CASES])
def test_lda_equals_the_restatement(built_lib, case):
    """P = 1, a value between and the largest allowed, on a corpus where that is classes - 1 (Sb rank-deficient) and on one where it
    is R."""
    from speaker_recognition_amd import plda
    R, counts = case
    c = pc.corpus(R, counts, 900 + R + len(counts))
    X, ids = c["X"], c["ids"]
    n, S = X.shape[0], len(counts)
    assert n - S > R
    worst = 0.0
    for P in ec.lda_dims(R, counts):
        mu, A, psi, Sw, Sb = ec.lda(X, ids, P)
        kappa = float(np.linalg.cond(Sw))
        assert kappa <= pc.KAPPA_MAX
        m = plda.LDA().fit(X, ids * 5 + 2, P)          # (any labels: they are made dense)
        assert m.A.shape == (P, R) and m.psi.shape == (P,) and np.all(np.diff(m.psi) <= 0)
        # LDA does not report its sweeps: the solver's on the restated covariances, and one more for the covariances' own rounding
        sweeps = plda.gen_eig(Sb, Sw, return_info=True)[2]["sweeps"] + 1
        g = kappa * (pc.gate_cov(R, n, 1.0) + ec.gate(R, sweeps))
        worst = max(worst, _parity("lda A Sw A^T", (R, S, P), float(np.max(np.abs(m.A @ Sw @ m.A.T - np.eye(P)))), g),
                    _parity("lda A Sb A^T", (R, S, P), float(np.max(np.abs(m.A @ Sb @ m.A.T - np.diag(m.psi)))) / float(psi[0]), g),
                    _parity("lda psi", (R, S, P), float(np.max(np.abs(m.psi - psi))) / float(psi[0]), g),
                    _parity("lda mu", (R, S, P), pc.rel(m.mu, mu), 8.0 * n * pc.EPS * float(np.abs(X).max()) / float(np.abs(mu).max())))
        # the projection: against the restatement with the device's own A (the directions themselves turn inside close values of psi)
        for ln in (False, True):
            Y, cnt = m.transform(X, length_norm=ln, return_counts=True)
            want = ec.project(X, m.mu, m.A, ln)
            amp = float(np.max(np.abs(X - m.mu) @ np.abs(m.A.T)) / np.max(np.abs((X - m.mu) @ m.A.T)))
            assert Y.shape == (n, P) and cnt["zero_rows"] == 0
            worst = max(worst, _parity("lda transform, length_norm %s" % ln, (R, S, P), pc.rel(Y, want), amp * 8.0 * 2 * R * pc.EPS * (2 if ln else 1)))
    assert worst <= 1
    Xz = np.array(X)
    Xz[4] = m.mu                                       # a zero row is counted and comes out as zeros
    Y, cnt = m.transform(Xz, return_counts=True)
    assert cnt["zero_rows"] == 1 and not Y[4].any() and np.isfinite(Y).all()


# ---- the diagonalised scorer ----

def _models(c):
    from speaker_recognition_amd import plda
    full = plda.PLDA(c["mu"], c["Sb"], c["Sw"])
    diag, info = full.diagonalise(return_info=True)
    assert info["status"] == 0
    return full, diag, info


@pytest.mark.parametrize("case", pc.SCORE_CASES)
def test_diagonalised_scores_equal_the_restatement_and_the_full_scorer(built_lib, case):
    R, J, T = case
    c = pc.score_case(R, J, T)
    f = c["factors"]
    kappa = float(np.linalg.cond(c["Sw"]))
    assert all(f[k] <= pc.KAPPA_MAX for k in ("kb", "kw", "kP", "kPc", "kP0")) and kappa <= pc.KAPPA_MAX
    full, diag, info = _models(c)
    got, counts = diag.score(c["enrol"], c["enrol_ids"], c["X"], return_counts=True)
    assert got.shape == (J, T) and counts["bad_classes"] == 0 and np.isfinite(got).all()
    g = ec.gate_diag_score(R, f, kappa, info["sweeps"])
    r1 = _parity("diag score", case, pc.rel(got, c["want"]), g)
    r2 = _parity("diag score against PLDA.score", case, pc.rel(got, full.score(c["enrol"], c["enrol_ids"], c["X"])), g + pc.gate_score(R, f))
    assert max(r1, r2) <= 1


def test_a_diagonalised_score_is_the_same_bits_alone_in_any_batch_and_under_any_bound(built_lib):
    from speaker_recognition_amd import _lib
    R, J, T = 65, 5, 1000
    c = pc.score_case(R, J, T)
    _, m, info = _models(c)
    whole = m.score(c["enrol"], c["enrol_ids"], c["X"])
    g = ec.gate_diag_score(R, c["factors"], float(np.linalg.cond(c["Sw"])), info["sweeps"])
    assert _parity("diag score", (R, J, T), pc.rel(whole, c["want"]), g) <= 1
    for j in (0, 3, 4):                                # the model alone
        rows = c["enrol_ids"] == j
        assert np.array_equal(_bits(m.score(c["enrol"][rows], c["enrol_ids"][rows], c["X"])), _bits(whole[j:j + 1]))
    for t in (0, 63, 999):                             # the segment alone
        assert np.array_equal(_bits(m.score(c["enrol"], c["enrol_ids"], c["X"][t:t + 1])), _bits(whole[:, t:t + 1]))
    assert (1 << 20) // ((2 * R + len(set(c["counts"].tolist())) + 1) * 8) < T       # a 1 MiB bound: two chunks
    _lib.set_option("plda_scratch_mib", 1)
    assert np.array_equal(_bits(m.score(c["enrol"], c["enrol_ids"], c["X"])), _bits(whole))


def test_diagonalised_average_is_by_the_book_on_the_averaged_vectors(built_lib):
    R, J, T = pc.SCORE_CASES[3]
    c = pc.score_case(R, J, T)
    _, m, info = _models(c)
    means = c["E"] / c["counts"][:, None]
    avg = m.score(c["enrol"], c["enrol_ids"], c["X"], enrol_mode="average")
    assert np.array_equal(_bits(avg), _bits(m.score(means, np.arange(J), c["X"])))
    want = pc.score(c["mu"], c["Sb"], c["Sw"], means, np.ones(J, dtype=np.int64), c["X"], want_factors=True)
    g = ec.gate_diag_score(R, want[1], float(np.linalg.cond(c["Sw"])), info["sweeps"])
    assert _parity("diag score, averaged enrolment", (R, J, T), pc.rel(avg, want[0]), g) <= 1
    assert not np.array_equal(avg, m.score(c["enrol"], c["enrol_ids"], c["X"]))


def test_a_negative_psi_zeroes_and_counts_its_classes(built_lib):
    from speaker_recognition_amd import plda
    R, J, T = pc.SCORE_CASES[3]
    c = pc.score_case(R, J, T)
    _, m, _ = _models(c)
    n_classes = len(set(c["counts"].tolist()))
    for bad in (-0.5, np.nan):
        psi = np.array(m.psi)
        psi[-1] = bad
        got, counts = plda.DiagPLDA(m.mu, m.V, psi).score(c["enrol"], c["enrol_ids"], c["X"], return_counts=True)
        assert counts["bad_classes"] == n_classes == 7 and not got.any()
    # a huge leading value lets -0.3 pass as rounding of it; then (c + 1) psi_d + 1 <= 0 from c = 3 on: those classes alone are zeroed
    psi = np.array(m.psi)
    psi[0], psi[-1] = 1e10, -0.3
    got, counts = plda.DiagPLDA(m.mu, m.V, psi).score(c["enrol"], c["enrol_ids"], c["X"], return_counts=True)
    low = c["counts"] <= 2
    assert counts["bad_classes"] == n_classes - 2 and not got[~low].any() and got[low].all() and np.isfinite(got).all()
    psi = np.array(m.psi)
    psi[-1] = -1e-12 * psi[0]                          # negative within rounding: used as it is
    got, counts = plda.DiagPLDA(m.mu, m.V, psi).score(c["enrol"], c["enrol_ids"], c["X"], return_counts=True)
    assert counts["bad_classes"] == 0 and np.isfinite(got).all() and got.any()


# ---- the pipeline ----

def test_i_vectors_through_lda_to_normalised_diagonal_plda_scores_end_to_end(built_lib):
    """Statistics against the golden UBM -> total-variability matrix -> i-vectors -> LDA and length normalisation -> PLDA ->
    diagonalise -> DiagPLDA.score -> Z-norm: finite scores, the target trials above the others."""
    from speaker_recognition_amd import ivector, plda, scorenorm
    ubm = bw.fixture_ubm()
    K, D = ubm[1].shape
    G, sessions, R, P = 12, 5, 6, 4
    c = jc.corpus(G, K, D, R, 4242, sessions=sessions, ubm=ubm)
    Tm = ivector.train_tv(c["F"], c["N"], ubm, R=R, niter=3)
    iv = ivector.extract(c["F"], c["N"], ubm, Tm)
    test = np.arange(G * sessions) % sessions == sessions - 1          # every speaker's last session is its test segment
    ids = c["spk_ids"]
    lda = plda.LDA().fit(iv[~test], ids[~test], P)
    dev, tst = lda.transform(iv[~test]), lda.transform(iv[test])
    assert dev.shape == (G * (sessions - 1), P) and np.isfinite(dev).all()
    model = plda.PLDA().fit(dev, ids[~test], n_iter=5)
    assert model.stop == 0 and model.iterations == 5
    diag = model.diagonalise()
    S = diag.score(dev, ids[~test], tst)
    Ez = diag.score(dev, ids[~test], dev)
    out, counts = scorenorm.normalise(S, "z", enrol_cohort=Ez, return_counts=True)
    assert out.shape == (G, G) and np.isfinite(out).all() and counts["degenerate_enrol"] == 0
    target = np.eye(G, dtype=bool)
    for name, M in (("raw", S), ("z-norm", out)):
        print("eig pipeline %s: targets %.3f, non-targets %.3f, EER %.3f" % (name, M[target].mean(), M[~target].mean(), scorenorm.eer(M.ravel(), target.ravel())))
        assert M[target].mean() > M[~target].mean()
