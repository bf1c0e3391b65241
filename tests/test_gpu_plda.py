"""The i-vector back end on the device (csrc/plda.hip through plda.fit_transform / transform / cosine_score / PLDA, ivector.train_tv /
extract) against the float64 numpy restatement and the joint-Gaussian form (tests/plda_cases.py, which states the generator, the
mutants and derives the gates).  Every parity case asserts the conditions its gate rests on (the condition numbers of the
restatement's own matrices under 1e6, no degenerate row) and prints its worst figure as a PARITY line before asserting."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bw_cases as bw  # noqa: E402
import jfa_cases as jc  # noqa: E402
import plda_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu
TRANSFORM_CASES = [(R, n) for R in pc.TRANSFORM_R for n in sorted(set((R + 1,) + pc.TRANSFORM_N)) if n > R]


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
    print("PARITY plda %s %s: difference / gate = %.3g (gate %.3g)" % (what, case, ratio, gate))
    return ratio


# ---- the transforms ----

@pytest.mark.parametrize("case", TRANSFORM_CASES)
def test_whitening_gives_unit_covariance_and_unit_norms(built_lib, case):
    from speaker_recognition_amd import plda
    R, n = case
    c = pc.transform_case(R, n)
    assert c["kSigma"] <= pc.KAPPA_MAX
    mu, A = plda.fit_transform(c["X"])
    assert np.array_equal(A, np.tril(A)) and np.isfinite(A).all()
    Y, counts = plda.transform(c["X"], mu, A, length_norm=False, return_counts=True)
    assert counts["zero_rows"] == 0
    r_cov = _parity("whiten covariance", case, float(np.abs(Y.T @ Y / n - np.eye(R)).max()), pc.gate_cov(R, n, c["kSigma"]))
    r_A = _parity("whiten A", case, pc.rel(A, c["A"]), pc.gate_cov(R, n, c["kSigma"]))
    Yn, counts = plda.transform(c["X"], mu, A, return_counts=True)
    assert counts["zero_rows"] == 0 and (np.abs(Y).sum(axis=1) > 0).all()              # no degenerate row
    r_norm = _parity("unit norms", case, float(np.abs(np.sqrt((Yn * Yn).sum(axis=1)) - 1.0).max()), 8.0 * R * pc.EPS)
    r_dir = _parity("directions", case, float(np.abs(Yn - Y / np.sqrt((Y * Y).sum(axis=1, keepdims=True))).max()), 8.0 * R * pc.EPS)
    assert max(r_cov, r_A, r_norm, r_dir) <= 1


@pytest.mark.parametrize("case", TRANSFORM_CASES)
def test_wccn_equals_the_restatement(built_lib, case):
    from speaker_recognition_amd import plda
    R, n = case
    c = pc.transform_case(R, n)
    assert c["kW"] is not None and c["kW"] <= pc.KAPPA_MAX
    mu, A = plda.fit_transform(c["X"], c["ids"] * 3 + 7, kind="wccn")                   # (any labels: they are made dense)
    scale = float(np.abs(c["X"]).max()) / float(np.abs(c["mu"]).max())
    r_mu = _parity("wccn mu", case, pc.rel(mu, c["mu"]), 8.0 * n * pc.EPS * scale)
    r_A = _parity("wccn A", case, pc.rel(A, c["Aw"]), pc.gate_cov(R, n, c["kW"]))
    want = pc.transform(c["X"], c["mu"], c["Aw"])
    amp = float(np.max(np.abs(c["X"] - c["mu"]) @ np.abs(c["Aw"].T)) / np.max(np.abs((c["X"] - c["mu"]) @ c["Aw"].T)))
    r_Y = _parity("wccn transform", case, pc.rel(plda.transform(c["X"], mu, A), want), amp * (pc.gate_cov(R, n, c["kW"]) + 8.0 * 2 * R * pc.EPS))
    assert max(r_mu, r_A, r_Y) <= 1


def test_a_zero_row_is_counted_and_comes_out_as_zeros(built_lib):
    from speaker_recognition_amd import plda
    c = pc.transform_case(17, 64)
    X = np.array(c["X"])
    X[5] = X[40] = c["mu"]                             # centred by the mu given: exact zeros
    Y, counts = plda.transform(X, c["mu"], c["A"], return_counts=True)
    assert counts["zero_rows"] == 2 and not Y[5].any() and not Y[40].any() and np.isfinite(Y).all()
    keep = np.ones(64, dtype=bool)
    keep[[5, 40]] = False
    assert np.array_equal(_bits(Y[keep]), _bits(plda.transform(c["X"], c["mu"], c["A"])[keep]))    # the other rows are untouched
    assert np.array_equal(_bits(plda.transform(X, c["mu"], c["A"], length_norm=False)[5]), _bits(np.zeros(17)))


@pytest.mark.parametrize("J", pc.COSINE_SIZES)
@pytest.mark.parametrize("T", pc.COSINE_SIZES)
def test_cosine_scores_equal_the_restatement(built_lib, J, T):
    from speaker_recognition_amd import plda
    R = 17
    rng = np.random.default_rng(100 * J + T)
    E, X = rng.standard_normal((J, R)), rng.standard_normal((T, R)) + 0.5
    want = pc.cosine(E, X)
    got = plda.cosine_score(E, X)
    assert got.shape == (J, T) and np.abs(got).max() <= 1.0 + 8 * R * pc.EPS
    assert _parity("cosine", (J, T), pc.rel(got, want), pc.gate_cosine(R, want)) <= 1
    if J > 1:                                          # a zero vector scores 0.0, not NaN
        E0 = np.array(E)
        E0[0] = 0.0
        got = plda.cosine_score(E0, X)
        assert not got[0].any() and np.isfinite(got).all()


# ---- training ----

def _fit(X, ids, start, n_iter, Sw0=None):
    from speaker_recognition_amd import plda
    return plda.PLDA().fit(X, ids, n_iter=n_iter, Sb0=start, Sw0=start if Sw0 is None else Sw0)


@pytest.mark.parametrize("case", pc.TRAIN_CASES)
def test_one_and_five_rounds_equal_the_restatement(built_lib, case):
    R, counts = case
    tc = pc.train_case(R, counts)
    n, S = sum(counts), len(counts)
    assert tc["kSigma"] <= pc.KAPPA_MAX and all(tc["worst"][k] <= pc.KAPPA_MAX for k in ("kb", "kw", "kP"))
    worst = 0.0
    for n_iter, f in ((1, tc["first"]), (5, tc["worst"])):
        m = _fit(tc["X"], tc["ids"], tc["start"], n_iter)
        assert (m.iterations, m.stop, m.n_classes) == (n_iter, 0, len(set(counts)))
        assert np.array_equal(m.Sb, m.Sb.T) and np.array_equal(m.Sw, m.Sw.T)            # symmetric to the bit
        gb, gw = pc.gate_em(R, n, S, f, n_iter)
        want_b, want_w = tc["trace"][n_iter - 1]
        worst = max(worst, _parity("train Sb, %d round(s)" % n_iter, (R, S, n), pc.rel(m.Sb, want_b), gb),
                    _parity("train Sw, %d round(s)" % n_iter, (R, S, n), pc.rel(m.Sw, want_w), gw))
    scale = float(np.abs(tc["X"]).max()) / float(np.abs(tc["mu"]).max())
    worst = max(worst, _parity("train mu", (R, S, n), pc.rel(m.mu, tc["mu"]), 8.0 * n * pc.EPS * scale))
    # the default start, half the total covariance formed on the device: the same round (the start's own rounding, n + 2 terms of
    # eps, lies far inside what the gate allows the two inverses of the start)
    from speaker_recognition_amd import plda
    d = plda.PLDA().fit(tc["X"], tc["ids"], n_iter=1)
    assert (d.iterations, d.stop) == (1, 0)
    gb, gw = pc.gate_em(R, n, S, tc["first"], 1)
    worst = max(worst, _parity("train Sb, default start", (R, S, n), pc.rel(d.Sb, tc["trace"][0][0]), gb),
                _parity("train Sw, default start", (R, S, n), pc.rel(d.Sw, tc["trace"][0][1]), gw))
    assert worst <= 1


@pytest.mark.parametrize("case", pc.TRAIN_CASES)
def test_five_rounds_in_one_call_are_five_calls_of_one(built_lib, case):
    R, counts = case
    tc = pc.train_case(R, counts)
    whole = _fit(tc["X"], tc["ids"], tc["start"], 5)
    Sb = Sw = tc["start"]
    for _ in range(5):
        m = _fit(tc["X"], tc["ids"], Sb, 1, Sw)
        Sb, Sw = m.Sb, m.Sw
    assert np.array_equal(_bits(whole.Sb), _bits(Sb)) and np.array_equal(_bits(whole.Sw), _bits(Sw)) and np.array_equal(_bits(whole.mu), _bits(m.mu))
    again = _fit(tc["X"], tc["ids"], tc["start"], 5)                                  # and from run to run
    assert np.array_equal(_bits(whole.Sb), _bits(again.Sb)) and np.array_equal(_bits(whole.Sw), _bits(again.Sw))


def test_the_joint_likelihood_of_the_devices_pairs_never_decreases(built_lib):
    tc = pc.train_case(5, (1, 2, 3, 2, 1, 3, 3, 2), 8)
    Sb = Sw = tc["start"]
    ll = [pc.marginal_loglik(tc["X"], tc["ids"], tc["mu"], Sb, Sw)]
    for _ in range(8):
        m = _fit(tc["X"], tc["ids"], Sb, 1, Sw)
        Sb, Sw = m.Sb, m.Sw
        ll.append(pc.marginal_loglik(tc["X"], tc["ids"], m.mu, Sb, Sw))
    print("plda joint-form marginal likelihood over 8 device rounds:", " ".join("%.6f" % v for v in ll))
    assert np.all(np.diff(ll) >= 0) and ll[-1] - ll[0] > 1.0


@pytest.mark.parametrize("case", [c for c in pc.TRAIN_CASES if c[0] in (17, 65)])
def test_the_global_memory_path_gives_the_lds_paths_bits_or_lies_in_the_gate(built_lib, case):
    from speaker_recognition_amd import _lib
    R, counts = case
    tc = pc.train_case(R, counts)
    n, S = sum(counts), len(counts)
    lds = _fit(tc["X"], tc["ids"], tc["start"], 5)
    _lib.set_option("jfa_lds_rows", 1)
    glob = _fit(tc["X"], tc["ids"], tc["start"], 5)
    same = np.array_equal(_bits(lds.Sb), _bits(glob.Sb)) and np.array_equal(_bits(lds.Sw), _bits(glob.Sw))
    gb, gw = pc.gate_em(R, n, S, tc["worst"], 5)
    ratio = max(_parity("train Sb, global-memory path", (R, S, n), pc.rel(glob.Sb, tc["trace"][4][0]), gb),
                _parity("train Sw, global-memory path", (R, S, n), pc.rel(glob.Sw, tc["trace"][4][1]), gw))
    print("plda global-memory path R=%d: the LDS path's bits: %s" % (R, same))
    assert same or ratio <= 1


def test_an_input_that_stops_factoring_returns_the_last_good_pair(built_lib):
    tc = pc.train_case(17, tuple(range(1, 18)))
    good = np.array(tc["start"])
    indefinite = np.array(good)
    indefinite[3, 3] = -1.0                            # symmetric, not positive definite
    for Sb0, Sw0, code in ((indefinite, good, 1), (good, indefinite, 2)):
        m = _fit(tc["X"], tc["ids"], Sb0, 5, Sw0)
        assert (m.iterations, m.stop) == (0, code)
        assert np.array_equal(_bits(m.Sb), _bits(Sb0)) and np.array_equal(_bits(m.Sw), _bits(Sw0))       # the pair given, untouched
        assert np.isfinite(m.mu).all()
    # vectors whose squares overflow: the first round's result is not finite, the pair given comes back with stop code 4
    m = _fit(tc["X"] * 1e160, tc["ids"], good, 3)
    assert (m.iterations, m.stop) == (0, 4) and np.array_equal(_bits(m.Sb), _bits(good)) and np.array_equal(_bits(m.Sw), _bits(good))


def test_a_covariance_that_does_not_factor_is_refused_by_fit_transform(built_lib):
    from speaker_recognition_amd import _lib, plda
    c = pc.transform_case(17, 64)
    X = np.array(c["X"])
    X[:, 5] = 1.0                                      # a constant column: its centred values, and its pivot, are exact zeros
    with pytest.raises(_lib.SRError, match="the total covariance of these 64 vectors of 17 dimensions does not factor .* pass more vectors"):
        plda.fit_transform(X)
    with pytest.raises(_lib.SRError, match="the within-class covariance .* does not factor"):
        plda.fit_transform(X, c["ids"], kind="wccn")
    with pytest.raises(_lib.SRError, match="the total covariance of these 1 vectors"):
        plda.fit_transform(c["X"][:1])                 # one vector: the covariance is zero
    mu, A = plda.fit_transform(c["X"])                 # and the library goes on working
    assert np.isfinite(A).all()


# ---- scoring ----

def _model(c):
    from speaker_recognition_amd import plda
    return plda.PLDA(c["mu"], c["Sb"], c["Sw"])


@pytest.mark.parametrize("case", pc.SCORE_CASES)
def test_scores_equal_the_restatement(built_lib, case):
    R, J, T = case
    c = pc.score_case(R, J, T)
    f = c["factors"]
    assert all(f[k] <= pc.KAPPA_MAX for k in ("kb", "kw", "kP", "kPc", "kP0"))
    got, counts = _model(c).score(c["enrol"], c["enrol_ids"], c["X"], return_counts=True)
    assert got.shape == (J, T) and counts["bad_classes"] == 0 and np.isfinite(got).all()
    assert _parity("score", case, pc.rel(got, c["want"]), pc.gate_score(R, f)) <= 1


def test_scores_equal_the_joint_form(built_lib):
    R, J, T = pc.SCORE_CASES[0]
    assert R == 5
    c = pc.score_case(R, J, T)
    got = _model(c).score(c["enrol"], c["enrol_ids"], c["X"])
    want = np.array([[pc.joint_score(c["mu"], c["Sb"], c["Sw"], c["enrol"][c["enrol_ids"] == j], x) for x in c["X"]] for j in range(J)])
    kJ = max(float(np.linalg.cond(pc.joint_cov(int(n) + 1, c["Sb"], c["Sw"]))) for n in c["counts"])
    joint = c["factors"]["amp_s"] * 8.0 * 2 * (8 * R) * pc.EPS * kJ                    # the joint form's own solves: up to 8 R unknowns
    assert _parity("score against the joint form", (R, J, T), pc.rel(got, want), pc.gate_score(R, c["factors"]) + joint) <= 1
    assert np.mean(np.diag(got)) > np.mean(got[~np.eye(J, T, dtype=bool)])              # the targets sit on the diagonal


def test_a_score_is_the_same_bits_alone_in_any_batch_and_under_any_bound(built_lib):
    from speaker_recognition_amd import _lib
    R, J, T = 65, 5, 1000
    c = pc.score_case(R, J, T)
    m = _model(c)
    whole = m.score(c["enrol"], c["enrol_ids"], c["X"])
    assert all(c["factors"][k] <= pc.KAPPA_MAX for k in ("kb", "kw", "kP", "kPc", "kP0"))
    assert _parity("score", (R, J, T), pc.rel(whole, c["want"]), pc.gate_score(R, c["factors"])) <= 1
    for j in (0, 3, 4):                                # the model alone
        rows = c["enrol_ids"] == j
        assert np.array_equal(_bits(m.score(c["enrol"][rows], c["enrol_ids"][rows], c["X"])), _bits(whole[j:j + 1]))
    for t in (0, 63, 999):                             # the segment alone
        assert np.array_equal(_bits(m.score(c["enrol"], c["enrol_ids"], c["X"][t:t + 1])), _bits(whole[:, t:t + 1]))
    rows = np.isin(c["enrol_ids"], (1, 4))             # another batch: two models, 130 segments from the middle
    assert np.array_equal(_bits(m.score(c["enrol"][rows], c["enrol_ids"][rows], c["X"][500:630])), _bits(whole[[1, 4], 500:630]))
    assert _lib.plda_plan("score", R, c["counts"], T=T, scratch_bytes=1 << 20)["n_chunks"] == 2
    _lib.set_option("plda_scratch_mib", 1)
    assert np.array_equal(_bits(m.score(c["enrol"], c["enrol_ids"], c["X"])), _bits(whole))
    _lib.set_option("jfa_lds_rows", 1)                 # the other factorisation path: its bits, or within the gate
    glob = m.score(c["enrol"], c["enrol_ids"], c["X"])
    same = np.array_equal(_bits(glob), _bits(whole))
    assert _parity("score, global-memory path", (R, J, T), pc.rel(glob, c["want"]), pc.gate_score(R, c["factors"])) <= 1 or same


def test_long_rows_of_unsorted_models_land_in_their_places(built_lib):
    """Rows of 8192 scores and more are copied from the device straight to their model's row: models in descending count, so that
    every row moves."""
    R, J, T = 2, 3, 8200
    c = pc.score_case(R, J, T)
    assert all(c["factors"][k] <= pc.KAPPA_MAX for k in ("kb", "kw", "kP", "kPc", "kP0")) and list(c["counts"]) == sorted(c["counts"])
    got = _model(c).score(c["enrol"], J - 1 - c["enrol_ids"], c["X"])
    assert _parity("score, long rows", (R, J, T), pc.rel(got, c["want"][::-1]), pc.gate_score(R, c["factors"])) <= 1
    assert np.array_equal(_bits(got[::-1]), _bits(_model(c).score(c["enrol"], c["enrol_ids"], c["X"])))


def test_average_is_by_the_book_on_the_averaged_vectors(built_lib):
    R, J, T = pc.SCORE_CASES[3]
    c = pc.score_case(R, J, T)
    m = _model(c)
    means = c["E"] / c["counts"][:, None]
    avg = m.score(c["enrol"], c["enrol_ids"], c["X"], enrol_mode="average")
    assert np.array_equal(_bits(avg), _bits(m.score(means, np.arange(J), c["X"])))
    want = pc.score(c["mu"], c["Sb"], c["Sw"], means, np.ones(J, dtype=np.int64), c["X"], want_factors=True)
    assert _parity("score, averaged enrolment", (R, J, T), pc.rel(avg, want[0]), pc.gate_score(R, want[1])) <= 1
    assert not np.array_equal(avg, m.score(c["enrol"], c["enrol_ids"], c["X"]))


def test_a_class_that_does_not_factor_gets_zeros_and_is_counted(built_lib):
    from speaker_recognition_amd import plda
    R, J, T = pc.SCORE_CASES[3]
    c = pc.score_case(R, J, T)
    Sw = np.array(c["Sw"])
    Sw[2, 2] = -1.0
    got, counts = plda.PLDA(c["mu"], c["Sb"], Sw).score(c["enrol"], c["enrol_ids"], c["X"], return_counts=True)
    assert counts["bad_classes"] == len(set(c["counts"].tolist())) == 7 and not got.any()


# ---- the pipeline ----

def test_i_vectors_to_normalised_plda_scores_end_to_end(built_lib):
    """Statistics against the golden UBM -> total-variability matrix -> i-vectors -> whitening and length normalisation -> PLDA ->
    Z-norm: finite scores, the target trials above the others."""
    from speaker_recognition_amd import ivector, plda, scorenorm
    ubm = bw.fixture_ubm()
    K, D = ubm[1].shape
    G, sessions, R = 12, 5, 6
    c = jc.corpus(G, K, D, R, 4242, sessions=sessions, ubm=ubm)
    Tm = ivector.train_tv(c["F"], c["N"], ubm, R=R, niter=3)
    iv = ivector.extract(c["F"], c["N"], ubm, Tm)
    assert Tm.shape == (R, K * D) and iv.shape == (G * sessions, R) and np.isfinite(iv).all()
    test = np.arange(G * sessions) % sessions == sessions - 1          # every speaker's last session is its test segment
    ids = c["spk_ids"]
    mu, A = plda.fit_transform(iv[~test])
    dev, tst = plda.transform(iv[~test], mu, A), plda.transform(iv[test], mu, A)
    model = plda.PLDA().fit(dev, ids[~test], n_iter=5)
    assert model.stop == 0 and model.iterations == 5
    S = model.score(dev, ids[~test], tst)
    Ez = model.score(dev, ids[~test], dev)
    out, counts = scorenorm.normalise(S, "z", enrol_cohort=Ez, return_counts=True)
    assert out.shape == (G, G) and np.isfinite(out).all() and counts["degenerate_enrol"] == 0
    target = np.eye(G, dtype=bool)
    sums = np.add.reduceat(dev, np.arange(0, dev.shape[0], sessions - 1))               # (a speaker's sessions are adjacent rows)
    for name, M in (("raw", S), ("z-norm", out), ("cosine", plda.cosine_score(sums, tst))):
        print("plda pipeline %s: targets %.3f, non-targets %.3f, EER %.3f" % (name, M[target].mean(), M[~target].mean(), scorenorm.eer(M.ravel(), target.ravel())))
        assert M[target].mean() > M[~target].mean()
