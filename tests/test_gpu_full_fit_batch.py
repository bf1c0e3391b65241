"""Full-covariance fits on the MI355X, single and batched (sr_fullgmm_fit, sr_fullgmm_fit_batch, skgmm.fit_many,
ModelInterface.train; csrc/gmm_full.hip).  Both run the one EM driver: ``skgmm.GMM.fit`` is a group of one, a batch is cut into
groups of S.  The contract is that a speaker's bits do not depend on its group: every comparison of a group of one
(``skgmm.GMM.fit``) against a group of S below is ``np.array_equal`` / ``==``, without a tolerance.  The scikit-learn goldens of
the group of one are test_gpu_full_cov.py's."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import fullcov_oracle as fo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("weights_", "means_", "covariances_", "precisions_cholesky_")
K, D = 32, 28


@pytest.fixture(scope="module")
def g():
    return fo.load_golden(os.path.join(ROOT, "tests", "golden", "fullcov_golden.npz"))


def _fit_single(kw, X):
    """-> the fitted model, or the ValueError its fit raised"""
    from speaker_recognition_amd import skgmm
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", skgmm.ConvergenceWarning)
        try:
            return skgmm.GMM(**kw).fit(X)
        except ValueError as e:
            return e


def _fit_batch(kws, Xs):
    from speaker_recognition_amd import skgmm
    gm = [skgmm.GMM(**kw) for kw in kws]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", skgmm.ConvergenceWarning)
        errors = skgmm.fit_many(gm, Xs)
    return gm, errors


def _same(single, batched, error, tag):
    """the batched model is the single fit bit for bit; a failed single fit is the same failure in the batch"""
    if isinstance(single, Exception):
        assert isinstance(error, ValueError) and str(error) == str(single), (tag, error, single)
        assert not hasattr(batched, "means_") and batched._h is None, tag
        return
    assert error is None, (tag, error)
    for attr in ARRAYS:
        assert np.array_equal(getattr(single, attr), getattr(batched, attr)), (tag, attr)
    assert single.n_iter_ == batched.n_iter_ and single.converged_ == batched.converged_, (tag, single.n_iter_, batched.n_iter_)
    assert single.lower_bound_ == batched.lower_bound_, (tag, single.lower_bound_, batched.lower_bound_)
    assert batched._h is not None


# n_chunks = min(32, ceil(n / 256)): 22, 1, 1, 1, 2, 32 (chunk 282: a ragged last chunk), 1
SIZES = [5600, K, 200, 256, 257, 9000, K]


@pytest.fixture(scope="module")
def kmeans_speakers():
    """40 speakers, k-means start, seeds of their own; ragged sizes that cycle through SIZES.  Speaker 1 has n = K frames at the
    default reg_covar, speaker 6 has n = K at reg_covar 1e-2 (every covariance is then at least 1e-2 I: that fit succeeds).
    -> (kwargs, data, the single fits)"""
    rng = np.random.default_rng(2024)
    kws, Xs = [], []
    for s in range(40):
        n = SIZES[s % len(SIZES)]
        Xs.append(fo.draw(rng, fo.random_model(rng, 8, D), n))
        kw = dict(n_components=K, random_state=100 + s)
        if s % len(SIZES) == 6:
            kw["reg_covar"] = 1e-2
        kws.append(kw)
    singles = [_fit_single(kw, X) for kw, X in zip(kws, Xs)]
    return kws, Xs, singles


@pytest.mark.parametrize("S", [1, 2, 7, 40])
def test_kmeans_start_is_bit_identical_to_single_fits(kmeans_speakers, S):
    kws, Xs, singles = kmeans_speakers
    assert not isinstance(singles[0], Exception) and not isinstance(singles[6], Exception)     # (n = 5600; n = K at reg_covar 1e-2)
    gm, errors = _fit_batch(kws[:S], Xs[:S])
    for s in range(S):
        if isinstance(singles[s], Exception):
            assert "ill-defined empirical covariance" in str(singles[s])
        _same(singles[s], gm[s], errors[s], (S, s, len(Xs[s])))


def _explicit_case(rng, K, D, n):
    """data of a random model, and a start near it: the model's weights and covariances, its means moved by 0.3 sigma
    -> (X, the three *_init arguments)"""
    w, mu, cov = fo.random_model(rng, K, D)
    X = fo.draw(rng, (w, mu, cov), n)
    return X, dict(weights_init=w, means_init=mu + 0.3 * rng.normal(size=mu.shape), precisions_init=np.linalg.inv(cov))


def test_explicit_start_mixed_stopping_is_bit_identical():
    """speakers that stop at different iterations, for different reasons, in one batch: tol = 0 runs to max_iter unconverged (3 and
    7 iterations); a tolerance above any change of the bound converges at the second iteration (the first has no bound before
    it); the default rule stops where the data lets it"""
    rng = np.random.default_rng(7)
    rules = [dict(tol=0.0, max_iter=3), dict(tol=1e6, max_iter=50), dict(), dict(tol=0.0, max_iter=7), dict(tol=1e-1, max_iter=100),
             dict(tol=1e-3, max_iter=4), dict(tol=1e6, max_iter=1)]
    kws, Xs = [], []
    for s, rule in enumerate(rules):
        X, init = _explicit_case(rng, 8, 13, [900, 300, 1500, 257, 700, 1100, 200][s])
        Xs.append(X)
        kws.append(dict(n_components=8, **rule, **init))
    singles = [_fit_single(kw, X) for kw, X in zip(kws, Xs)]
    assert not any(isinstance(m, Exception) for m in singles)
    iters = [m.n_iter_ for m in singles]
    assert len(set(iters)) >= 3, iters
    assert any(not m.converged_ and m.n_iter_ == kw.get("max_iter", 100) for m, kw in zip(singles, kws)), iters
    assert any(m.converged_ and m.n_iter_ < 5 for m in singles), iters
    gm, errors = _fit_batch(kws, Xs)
    for s in range(len(rules)):
        _same(singles[s], gm[s], errors[s], (s, rules[s]))


def test_unconverged_models_warn_each():
    from speaker_recognition_amd import skgmm
    rng = np.random.default_rng(3)
    Xs = [fo.draw(rng, fo.random_model(rng, 4, 5), 400) for _ in range(3)]
    gm = [skgmm.GMM(4, tol=0.0, max_iter=2), skgmm.GMM(4, tol=1e6), skgmm.GMM(4, tol=0.0, max_iter=3)]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert skgmm.fit_many(gm, Xs) == [None, None, None]
    assert len([x for x in w if issubclass(x.category, skgmm.ConvergenceWarning)]) == 2
    assert [m.converged_ for m in gm] == [False, True, False] and [m.n_iter_ for m in gm] == [2, 2, 3]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(1e-300, float(np.linalg.norm(b))))


def test_golden_case_inside_a_batch_matches_sklearn(g):
    """tests/golden's k32d28 fit twice (five iterations at tol 0; the default rule) among random k-means speakers: the tolerances
    of test_gpu_full_cov.py::test_fit_from_explicit_inits_matches_sklearn"""
    c = "k32d28"
    X = g["fit_%s_X" % c].astype(np.float64)
    kw = dict(weights_init=g["fit_%s_w0" % c], means_init=g["fit_%s_mu0" % c], precisions_init=g["fit_%s_prec0" % c])
    rng = np.random.default_rng(11)
    rand = [fo.draw(rng, fo.random_model(rng, 8, D), n) for n in (700, 3000, 257)]
    kws = [dict(n_components=K, random_state=1), dict(n_components=K, tol=0.0, max_iter=5, **kw), dict(n_components=K, random_state=2),
           dict(n_components=K, **kw), dict(n_components=K, random_state=3)]
    gm, errors = _fit_batch(kws, [rand[0], X, rand[1], X, rand[2]])
    assert errors == [None] * 5
    m5, mc = gm[1], gm[3]
    t = "fit5_%s_" % c
    assert m5.n_iter_ == 5 and not m5.converged_
    for attr, key in (("weights_", "w"), ("means_", "mu"), ("covariances_", "cov")):
        assert _rel(getattr(m5, attr), g[t + key]) < 1e-9, (attr, _rel(getattr(m5, attr), g[t + key]))
    cond = max(np.linalg.cond(cv) for cv in g[t + "cov"])
    assert _rel(m5.precisions_cholesky_, g[t + "P"]) < max(1e-9, 1e-13 * cond)
    t = "fitc_%s_" % c
    assert mc.n_iter_ == int(g[t + "n_iter"]) and int(mc.converged_) == int(g[t + "converged"])
    assert abs(mc.lower_bound_ - float(g[t + "lower_bound"])) < 1e-10 * max(1.0, abs(float(g[t + "lower_bound"])))
    assert _rel(mc.means_, g[t + "mu"]) < 1e-9


def test_a_failing_speaker_fails_alone(g):
    from speaker_recognition_amd import skgmm
    Dc = g["collapsed_X"].shape[1]
    rng = np.random.default_rng(13)
    Xs = [fo.draw(rng, fo.random_model(rng, 2, Dc), n) for n in (300, 40, 1000, 257)]
    kws = [dict(n_components=2, random_state=s) for s in range(4)]
    bad = dict(n_components=2, reg_covar=0.0, weights_init=g["collapsed_w0"], means_init=g["collapsed_mu0"],
               precisions_init=g["collapsed_prec0"])
    Xs.insert(2, g["collapsed_X"])
    kws.insert(2, bad)
    singles = [_fit_single(kw, X) for kw, X in zip(kws, Xs)]
    assert isinstance(singles[2], ValueError) and not any(isinstance(m, Exception) for m in singles[:2] + singles[3:])
    gm, errors = _fit_batch(kws, Xs)
    assert isinstance(errors[2], ValueError) and "ill-defined empirical covariance" in str(errors[2])
    assert gm[2]._h is None and not hasattr(gm[2], "means_")
    with pytest.raises(ValueError, match="not fitted"):
        gm[2].handle()
    for s in range(5):
        _same(singles[s], gm[s], errors[s], s)
    # the process goes on: an ordinary fit and a scoring call
    m = skgmm.GMM(2, **{k: v for k, v in bad.items() if k.endswith("_init")}).fit(g["collapsed_X"])
    assert np.all(np.isfinite(m.means_))
    assert np.all(np.isfinite(gm[0].score_samples(Xs[0])))


def test_group_cuts_do_not_show():
    from speaker_recognition_amd import _lib
    rng = np.random.default_rng(17)
    ns = [600, 64, 2000, 257, 900]
    Xs = [fo.draw(rng, fo.random_model(rng, 4, 13), n) for n in ns]
    kws = [dict(n_components=8, random_state=s, max_iter=40 + s) for s in range(5)]
    it0 = _lib.full_fit_batch_stats()[2]
    whole, e0 = _fit_batch(kws, Xs)
    it1 = _lib.full_fit_batch_stats()[2]
    default = _lib.full_fit_batch_bytes()
    try:
        _lib.set_option("full_fit_batch_bytes", 1)             # every speaker is a group of its own
        cut, e1 = _fit_batch(kws, Xs)
    finally:
        _lib.set_option("full_fit_batch_bytes", default)
    it2 = _lib.full_fit_batch_stats()[2]
    assert e0 == [None] * 5 and e1 == [None] * 5
    for s in range(5):
        _same(whole[s], cut[s], None, s)
    # one group runs as long as its slowest speaker; five groups run each speaker's own iterations
    assert it1 - it0 == max(m.n_iter_ for m in whole)
    assert it2 - it1 == sum(m.n_iter_ for m in whole)


def _two_points(rng, D, each=20):
    """two points, each repeated: with K 2 both components collapse onto a point, and at reg_covar 0 no covariance has a factor
    -- a k-means-start fit that fails at its first M-step"""
    return np.repeat(rng.normal(size=(2, D)), each, axis=0)


def test_kmeans_start_failure_among_explicit_and_kmeans_starts():
    """one batch with both kinds of start, in which a k-means speaker fails at its first M-step: the same failure and message
    as its single fit, everybody else bit-identical"""
    rng = np.random.default_rng(23)
    kws, Xs = [], []
    for s in range(6):
        if s in (1, 4):
            X, init = _explicit_case(rng, 2, 5, 300 + 50 * s)
            kws.append(dict(n_components=2, **init))
        elif s == 2:
            X = _two_points(rng, 5)
            kws.append(dict(n_components=2, reg_covar=0.0, random_state=s))
        else:
            X = fo.draw(rng, fo.random_model(rng, 2, 5), 200 + 100 * s)
            kws.append(dict(n_components=2, random_state=s))
        Xs.append(X)
    singles = [_fit_single(kw, X) for kw, X in zip(kws, Xs)]
    assert [isinstance(m, Exception) for m in singles] == [False, False, True, False, False, False]
    assert "ill-defined empirical covariance" in str(singles[2])
    gm, errors = _fit_batch(kws, Xs)
    for s in range(6):
        _same(singles[s], gm[s], errors[s], s)


def test_a_batch_whose_speakers_all_fail_at_the_start_launches_no_iteration():
    from speaker_recognition_amd import _lib
    rng = np.random.default_rng(29)
    Xs = [_two_points(rng, 5), _two_points(rng, 5, each=33)]
    kws = [dict(n_components=2, reg_covar=0.0, random_state=s) for s in range(2)]
    before = _lib.full_fit_batch_stats()
    gm, errors = _fit_batch(kws, Xs)
    after = _lib.full_fit_batch_stats()
    assert all(isinstance(e, ValueError) and "ill-defined empirical covariance" in str(e) for e in errors)
    assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (1, 2, 0)


def test_default_bound_holds_the_documented_set_in_one_group():
    """100 speakers x K 32 x D 28 x 5600 frames (scripts/time_full_enrol.py) at the default full_fit_batch_bytes:
    one group, so the batch launches as many iterations as its slowest speaker needs, not a second group's on top"""
    from speaker_recognition_amd import _lib
    rng = np.random.default_rng(31)
    Xs = [fo.draw(rng, fo.random_model(rng, 8, D), 5600) for _ in range(100)]
    kws = [dict(n_components=K, random_state=s) for s in range(100)]
    before = _lib.full_fit_batch_stats()
    gm, errors = _fit_batch(kws, Xs)
    after = _lib.full_fit_batch_stats()
    assert errors == [None] * 100
    assert after[2] - before[2] == max(m.n_iter_ for m in gm)
    for s in (0, 57, 99):
        _same(_fit_single(kws[s], Xs[s]), gm[s], None, s)


def _speakers(n_spk=10):
    from speaker_recognition_amd import synth
    # (test_gpu_full_cov.py's synthetic speakers: 9 apart in the family, 8 s of training audio each)
    return [synth.synth_speech(9 * s, 8.0, seed=1000 + s) for s in range(n_spk)]


def test_model_interface_trains_in_one_batched_call():
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.interface import ModelInterface
    m = ModelInterface(covariance_type="full", verbose=False, gmm_kwargs=dict(seed=5, max_iter=60))
    for s, sig in enumerate(_speakers()):
        m.enroll("spk%d" % s, 16000, sig)
    before = _lib.full_fit_batch_stats()
    m.train()
    after = _lib.full_fit_batch_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 10)
    assert m.gmmset.y == ["spk%d" % s for s in range(10)] and len(m.gmmset.gmms) == 10
    for s in range(10):
        single = _fit_single(dict(n_components=32, random_state=5, max_iter=60), np.asarray(m.features["spk%d" % s]))
        _same(single, m.gmmset.gmms[s], None, s)


def test_model_interface_failure_leaves_the_earlier_labels():
    from speaker_recognition_amd.interface import ModelInterface
    rng = np.random.default_rng(19)
    m = ModelInterface(covariance_type="full", verbose=False, gmm_order=2, gmm_kwargs=dict(reg_covar=0.0))
    m.features["a"] = list(fo.draw(rng, fo.random_model(rng, 2, 5), 300))
    m.features["bad"] = list(_two_points(rng, 5))
    m.features["c"] = list(fo.draw(rng, fo.random_model(rng, 2, 5), 300))
    assert isinstance(_fit_single(dict(n_components=2, reg_covar=0.0), np.asarray(m.features["bad"])), ValueError)
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        m.train()
    assert m.gmmset.y == ["a", "bad"] and len(m.gmmset.gmms) == 1
    _same(_fit_single(dict(n_components=2, reg_covar=0.0), np.asarray(m.features["a"])), m.gmmset.gmms[0], None, "a")


# ---- the single fit as a group of one: what it must not share with a batch (counters, the option, message prefixes), and the one
# workspace it does share
def test_a_single_fit_moves_no_batch_counter():
    from speaker_recognition_amd import _lib
    rng = np.random.default_rng(37)
    X, init = _explicit_case(rng, 2, 5, 300)
    before = _lib.full_fit_batch_stats()
    for kw in (dict(n_components=2, random_state=1), dict(n_components=2, **init)):
        m = _fit_single(kw, X)
        assert not isinstance(m, Exception) and m.n_iter_ >= 1
    assert _lib.full_fit_batch_stats() == before


def _raw_fit(h, X, reg_covar, init_given):
    """sr_fullgmm_fit on a handle -> (return value, sr_last_error())"""
    from speaker_recognition_amd import _lib
    X = np.ascontiguousarray(X, dtype=np.float64)
    prm, st = _lib.FullFitParams(1e-3, reg_covar, 100, init_given, 0), _lib.FullFitStats()
    rc = _lib.lib().sr_fullgmm_fit(h, _lib.as_dp(X), X.shape[0], X.shape[1], C.byref(prm), C.byref(st))
    return rc, _lib.last_error()


def test_single_fit_failing_at_the_kmeans_start_says_so_without_a_speaker_prefix():
    from speaker_recognition_amd import _lib, skgmm
    rng = np.random.default_rng(41)
    X = _two_points(rng, 5)
    h = C.c_void_p(_lib.lib().sr_fullgmm_create(2, 5, None, None, None))
    assert h
    try:
        rc, msg = _raw_fit(h, X, 0.0, 0)
        assert rc == -1 and msg.startswith(skgmm._ILL_DEFINED) and "ill-defined empirical covariance" in msg, msg
        assert "speaker" not in msg, msg
        assert _lib.lib().sr_fullgmm_info(h, None, None) == 0                # still without parameters
        rc, msg = _raw_fit(h, fo.draw(rng, fo.random_model(rng, 2, 5), 200), 1e-6, 0)        # the device goes on
        assert rc == 0 and _lib.lib().sr_fullgmm_info(h, None, None) == 1, msg
    finally:
        _lib.lib().sr_fullgmm_free(h)


def test_single_fit_failing_from_an_explicit_start_leaves_the_handle_as_given(g):
    from speaker_recognition_amd import _lib, skgmm
    X = np.ascontiguousarray(g["collapsed_X"], dtype=np.float64)
    Dc = X.shape[1]
    w0 = np.ascontiguousarray(g["collapsed_w0"], dtype=np.float64)
    mu0 = np.ascontiguousarray(g["collapsed_mu0"], dtype=np.float64)
    P0 = np.ascontiguousarray(skgmm._precision_cholesky_from_precisions(g["collapsed_prec0"]))

    def get():
        w, mu, cov, P = np.empty(2), np.empty((2, Dc)), np.empty((2, Dc, Dc)), np.empty((2, Dc, Dc))
        assert _lib.lib().sr_fullgmm_get(h, _lib.as_dp(w), _lib.as_dp(mu), _lib.as_dp(cov), _lib.as_dp(P)) == 0
        return w, mu, cov, P

    h = C.c_void_p(_lib.lib().sr_fullgmm_create(2, Dc, _lib.as_dp(w0), _lib.as_dp(mu0), _lib.as_dp(P0)))
    assert h
    try:
        rc, msg = _raw_fit(h, X, 0.0, 1)
        assert rc == -1 and msg.startswith(skgmm._ILL_DEFINED) and "speaker" not in msg, msg
        w, mu, cov, P = get()
        assert np.array_equal(w, w0) and np.array_equal(mu, mu0) and np.array_equal(P, P0)
        assert not cov.any()                                                 # (a handle built from arrays has no covariances)
        rc, msg = _raw_fit(h, X, 1e-6, 1)                                    # the device goes on: the same start, regularised
        assert rc == 0, msg
        assert all(np.all(np.isfinite(a)) for a in get()) and get()[2].any()
    finally:
        _lib.lib().sr_fullgmm_free(h)


def _mixed_sizes():
    """K 8 x D 13 speakers of 600, 64, 2000 and 257 frames (3, 1, 8 and 2 covariance chunks), the first four of
    test_group_cuts_do_not_show -> (kwargs, data)"""
    rng = np.random.default_rng(17)
    Xs = [fo.draw(rng, fo.random_model(rng, 4, 13), n) for n in (600, 64, 2000, 257)]
    return [dict(n_components=8, random_state=s, max_iter=40 + s) for s in range(4)], Xs


def test_the_group_bound_does_not_bear_on_a_single_fit():
    from speaker_recognition_amd import _lib
    kws, Xs = _mixed_sizes()
    at_default = _fit_single(kws[0], Xs[0])
    default = _lib.full_fit_batch_bytes()
    try:
        _lib.set_option("full_fit_batch_bytes", 1)             # far below the speaker's own workspace
        at_one = _fit_single(kws[0], Xs[0])
    finally:
        _lib.set_option("full_fit_batch_bytes", default)
    assert not isinstance(at_default, Exception)
    _same(at_default, at_one, None, "full_fit_batch_bytes = 1")
    _same(at_default, _fit_single(kws[0], Xs[0]), None, "restored")


def test_single_fits_and_a_batch_alternate_on_the_one_workspace():
    """600 frames alone, then {64, 2000} as a batch, then 257 alone: every call leaves longer tables and work lists behind than
    the next one writes.  Each result is the speaker's fit in another sequence (alone, shortest first)."""
    kws, Xs = _mixed_sizes()
    alone = [_fit_single(kws[s], Xs[s]) for s in (1, 3, 0, 2)]
    alone = dict(zip((1, 3, 0, 2), alone))
    assert not any(isinstance(m, Exception) for m in alone.values())
    first = _fit_single(kws[0], Xs[0])
    gm, errors = _fit_batch(kws[1:3], Xs[1:3])
    last = _fit_single(kws[3], Xs[3])
    _same(alone[0], first, None, 600)
    _same(alone[1], gm[0], errors[0], 64)
    _same(alone[2], gm[1], errors[1], 2000)
    _same(alone[3], last, None, 257)
