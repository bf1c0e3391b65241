"""EM and MAP training on degenerate data, through every statistics path that takes the shape: the whole fit in one launch
(em_small.hip, engine 4: K <= 32), float64 iterations (em_f64.hip, engine 5: K >= 33), an iteration per launch (em.hip:
1 vector ALU, 2 fp64 matrix-core sums, 3 split-bf16 responsibilities).  The cases are where the M-step's restatement of the
reference (gmm.cc:388-437, :502-509; gmmubm.cc:53-74) can differ from it without well-separated data noticing: a mixture that
no frame reaches (raw N_k == 0: the reference recomputes E_k[x] = sum g x / 1e-6 = 0, so an EM mean goes to the origin with
sigma sqrt(min_covar) and a MAP mean to (1 - alpha) ubm_mean), a weight of 0, frames that reach no mixture at all, a
collapsed feature column, min_covar other than 1e-3, fewer frames than mixtures.  Each fit is checked against the float64
oracle (oracle/gmm_oracle.c) applied the same number of times, and exactly where a closed form exists."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R6 = np.vectorize(lambda v: float("%g" % v))
ALPHA = 1e-6 / (1e-6 + 16.0)                 # a dead mixture's MAP weight on its (zero) data mean, relevance 16 (gmm.hh:118-120)


def _data(rng, n, cent, noise=0.7):
    return (cent[rng.integers(0, cent.shape[0], n)] + rng.normal(0, noise, (n, cent.shape[1]))).astype(np.float32)


def _paths(K, split=False):
    """(em_stats_engine option, the engine that must report) for every path that takes K mixtures: option 0 is the whole fit
    (K <= 32) or the float64 iterations (K >= 33); option 3 falls to 2 where the model is outside the split-bf16 layout's
    range (a mixture tens of sigmas from the others, or mostly padding tiles) -- `split` says the case is built to stay in it."""
    return [(0, 4 if K <= 32 else 5), (1, 1), (2, 2), (3, 3 if split else 2)]


def _fit(opt, X, start, iters, threshold=0.0, min_covar=1e-3, verbosity=0):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.pygmm import GMM
    _lib.set_option("em_stats_engine", opt)
    try:
        g = GMM.from_arrays(*start)
        g.nr_iteration, g.init_with_kmeans, g.threshold, g.min_covar, g.verbosity = iters, -1, threshold, min_covar, verbosity
        it = g.fit(X)
        return it, g.params(), _lib.last_em_stats_engine()
    finally:
        _lib.set_option("em_stats_engine", 0)


def _map(opt, X, ubm, iters):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.pygmm import GMM
    _lib.set_option("em_stats_engine", opt)
    try:
        g = GMM(ubm[1].shape[0], nr_iteration=iters, threshold=0.0)
        it = g.fit(X, ubm=GMM.from_arrays(*ubm))
        return it, g.params(), _lib.last_em_stats_engine()
    finally:
        _lib.set_option("em_stats_engine", 0)


def _oracle(go, start, X, N, min_covar=1e-3, ubm=None):
    want = go.GMMParams(*start)
    for _ in range(N):
        if ubm is None:
            want = go.em_iteration(want, X.astype(np.float64), min_covar=min_covar)
        else:
            want = go.em_iteration(want, X.astype(np.float64), map_relevance=16.0, ubm=go.GMMParams(*ubm))
    return want


def _gates(p, want, eng, tag):
    """engines 4 and 5 (float64): test_whole_fit_vs_oracle_iterated's gates; 1 to 3 (fp32 E-step):
    test_em_statistics_engines_vs_oracle's"""
    gw, gm, gs = (1e-7, 1e-6, 1e-6) if eng in (4, 5) else (1e-5, 1e-4, 1e-3)
    err = (np.max(np.abs(p[0] - want.weights)), np.max(np.abs(p[1] - want.mean)), np.max(np.abs(p[2] - want.sigma) / want.sigma))
    assert err[0] < gw and err[1] < gm and err[2] < gs, (tag, eng, err)


def _dead_em(p, want, dead, min_covar, eng, tag):
    """the closed forms of an EM mixture without responsibility: mean 0, sigma the floor, weight (1e-6 / n) / sum"""
    assert np.all(p[1][dead] == 0.0) and np.all(want.mean[dead] == 0.0), (tag, eng, p[1][dead])
    assert np.all(p[2][dead] == np.sqrt(min_covar)) and np.all(want.sigma[dead] == np.sqrt(min_covar)), (tag, eng, p[2][dead])
    # (the live N_k add up to the frame count in float64 on 4 / 5; in fp32 responsibilities, to ~1e-7 of it, on 1 to 3)
    rel = np.max(np.abs(p[0][dead] - want.weights[dead]) / want.weights[dead])
    assert rel < (1e-12 if eng in (4, 5) else 1e-6), (tag, eng, rel)


def _far_em_case(rng, K, D, n, dead):
    """data around 30 in every dimension (so the origin, where a dead mixture goes, is out of reach too), the mixtures in
    `dead` 1000 units from every frame"""
    cent = 30.0 + rng.normal(0, 2, (K, D))
    live = [k for k in range(K) if k not in dead]
    X = _data(rng, n, cent[live])
    mean = R6(cent + 0.2 * rng.standard_normal(cent.shape))
    mean[dead] += 1000.0
    return X, (np.full(K, 1.0 / K), mean, np.full((K, D), 0.9))


def test_em_unreachable_mixture(built_lib, oracle_built):
    """Case 1: one or two mixtures ~1000 units from every frame, 1, 2 and 5 iterations on every path.  After the first
    iteration a dead mixture sits at the origin with sigma sqrt(min_covar), still out of reach of data around 30."""
    go = oracle_built
    rng = np.random.default_rng(101)
    for K, D, n, dead in ((16, 13, 1500, [3]), (32, 20, 900, [0, 17]), (40, 13, 1500, [5, 39])):
        X, start = _far_em_case(rng, K, D, n, dead)
        for N in (1, 2, 5):
            want = _oracle(go, start, X, N)
            for opt, eng_want in _paths(K):
                it, p, eng = _fit(opt, X, start, N)
                tag = (K, D, n, N, opt)
                assert it == N and eng == eng_want, (tag, it, eng)
                _dead_em(p, want, dead, 1e-3, eng, tag)
                _gates(p, want, eng, tag)


def test_em_unreachable_mixture_split_responsibilities(built_lib, oracle_built):
    """Case 1 on the split-bf16 path (engine 3): 32 mixtures (no padding tile), the two dead ones 42 sigmas beyond the
    others' centre along one axis -- out of reach of every frame in float64 (a term below exp(-708)), inside the layout's
    range (max_k sum_d ((mu - centre) / sigma)^2 <= 2000).  One iteration: after it the dead mixtures sit at the origin with
    sigma sqrt(1e-3), which no layout of 16-bit parts covers (the following iterations take engine 2; case 1 checks those)."""
    go = oracle_built
    rng = np.random.default_rng(102)
    K, D, n, dead = 32, 13, 1500, [7, 21]
    live = [k for k in range(K) if k not in dead]
    cent = 30.0 + rng.normal(0, 1.0, (K, D))
    X = _data(rng, n, cent[live], noise=0.5)
    mean = R6(cent + 0.1 * rng.standard_normal(cent.shape))
    mean[dead] = R6(np.mean(mean[live], axis=0))
    mean[dead, 0] += 42 * 0.9
    start = (np.full(K, 1.0 / K), mean, np.full((K, D), 0.9))
    want = _oracle(go, start, X, 1)
    for opt, eng_want in ((3, 3), (0, 4)):
        it, p, eng = _fit(opt, X, start, 1)
        assert it == 1 and eng == eng_want, (opt, it, eng)
        _dead_em(p, want, dead, 1e-3, eng, opt)
        _gates(p, want, eng, opt)


def test_em_dead_mixture_revives_at_the_origin(built_lib, oracle_built):
    """Case 2: D = 2, data around the origin, one mixture out of reach.  The reference moves it to the origin with sigma
    sqrt(1e-3), where the frames nearest the origin give it responsibility again: its weight grows from ~1e-9 by orders of
    magnitude over 30 iterations.  Engines 4 and 5 follow the oracle all the way; 1 to 3 for 5 iterations."""
    go = oracle_built
    rng = np.random.default_rng(103)
    for K, n in ((8, 1500), (40, 1500)):
        cent = rng.normal(0, 2, (K, 2))
        cent -= cent.mean(axis=0)
        X = _data(rng, n, cent[1:])
        mean = R6(cent + 0.2 * rng.standard_normal(cent.shape))
        mean[0] += 1000.0
        start = (np.full(K, 1.0 / K), mean, np.full((K, 2), 0.9))
        for N, paths in ((30, [q for q in _paths(K) if q[0] == 0]), (5, [q for q in _paths(K) if q[0] != 0])):
            want = _oracle(go, start, X, N)
            assert want.weights[0] > 10 * 1e-6 / n and np.all(want.mean[0] != 0.0), (K, N, want.weights[0])   # (it does revive)
            for opt, eng_want in paths:
                it, p, eng = _fit(opt, X, start, N)
                tag = (K, n, N, opt)
                assert it == N and eng == eng_want, (tag, it, eng)
                _gates(p, want, eng, tag)
                rel = abs(p[0][0] - want.weights[0]) / want.weights[0]
                assert eng not in (4, 5) or rel < 1e-6, (tag, rel)


def test_em_zero_weight_in_the_warm_start(built_lib, oracle_built):
    """Case 3: w_k = 0.0 exactly (the rest renormalised): w p = 0 in the reference, the dead path of case 1 -- and nothing
    that is not finite anywhere in the model (log 0 is -inf in every engine's constant)."""
    go = oracle_built
    rng = np.random.default_rng(104)
    for K, D, n, zero in ((16, 13, 1200, [5]), (40, 13, 1200, [0, 22])):
        X, (w, mean, sigma) = _far_em_case(rng, K, D, n, [])
        w = np.full(K, 1.0 / (K - len(zero)))
        w[zero] = 0.0
        start = (w, mean, sigma)
        for N in (1, 3):
            want = _oracle(go, start, X, N)
            for opt, eng_want in _paths(K):
                it, p, eng = _fit(opt, X, start, N)
                tag = (K, N, opt)
                assert it == N and eng == eng_want, (tag, it, eng)
                assert all(np.all(np.isfinite(a)) for a in p), tag
                _dead_em(p, want, zero, 1e-3, eng, tag)
                _gates(p, want, eng, tag)


def test_em_no_frame_reaches_any_mixture(built_lib, oracle_built, capfd):
    """Case 4: every frame ~1000 units from every mixture.  Every N_k is 0: every mean 0, every sigma sqrt(min_covar), every
    weight 1/K, every total n ln 1e-15.  Under threshold 0.01 (gmm.cc:622-650) the first check, after iteration 1, compares
    with -DBL_MAX and goes on; the one after iteration 3 sees equal totals and stops: 4 iterations, on every path."""
    go = oracle_built
    rng = np.random.default_rng(105)
    for K, D, n in ((8, 13, 200), (40, 13, 200)):
        cent = rng.normal(0, 2, (K, D))
        X = _data(rng, n, 1000.0 + cent)
        start = (np.full(K, 1.0 / K), R6(cent), np.full((K, D), 0.9))
        want = _oracle(go, start, X, 4)
        for mc in (1e-3, 0.25):
            for opt, eng_want in _paths(K):
                capfd.readouterr()
                it, p, eng = _fit(opt, X, start, 50, threshold=0.01, min_covar=mc, verbosity=1)
                C.CDLL(None).fflush(None)             # (the library prints through C stdio, as the reference does)
                out = capfd.readouterr().out
                tag = (K, mc, opt)
                assert it == 4 and eng == eng_want, (tag, it, eng)
                assert np.all(p[1] == 0.0) and np.all(p[2] == np.sqrt(mc)), tag
                assert np.max(np.abs(p[0] * K - 1.0)) < 1e-14 and np.max(np.abs(want.weights * K - 1.0)) < 1e-14, (tag, p[0])
                lls = [(int(l.split()[1].rstrip(":")), float(l.split()[3])) for l in out.splitlines() if l.startswith("iter ")]
                total = n * np.log(1e-15)
                assert [i for i, _ in lls] == [1, 3], (tag, out)
                assert all(abs(v - total) <= (1e-9 if eng in (4, 5) else 1e-6) * abs(total) for _, v in lls), (tag, lls, total)


def _map_case(rng, K, D, n, dead):
    """a UBM around 1000 (where keeping the old mean is off by alpha ubm ~ 6e-5), the mixtures in `dead` 46 sigmas beyond the
    others' centre along one axis; the speaker's frames around the other mixtures"""
    cent = 1000.0 + rng.normal(0, 1.5, (K, D))
    live = [k for k in range(K) if k not in dead]
    mean = R6(cent)
    mean[dead] = R6(np.mean(mean[live], axis=0))
    mean[dead, 0] += 46 * 0.9
    X = _data(rng, n, mean[live])
    return X, (np.full(K, 1.0 / K), mean, np.full((K, D), 0.9))


def _check_map(p, want, ubm, dead, eng, tag):
    live = [k for k in range(ubm[1].shape[0]) if k not in dead]
    assert np.array_equal(p[0], ubm[0]) and np.array_equal(p[2], ubm[2]), tag      # means only, gmmubm.cc:29-38
    target = (1 - ALPHA) * ubm[1][dead]
    assert np.array_equal(want.mean[dead], target), tag
    rel = np.max(np.abs(p[1][dead] - target) / np.abs(target))
    assert rel < 1e-12, (tag, eng, rel)
    err = np.max(np.abs(p[1][live] - want.mean[live]))
    assert err < (1e-6 if eng in (4, 5) else 1e-4), (tag, eng, err)


def test_map_with_dead_mixtures(built_lib, oracle_built):
    """Case 5: MAP from a UBM whose means are near 1000, a few of its mixtures out of reach of the speaker's frames, 1 and 2
    iterations.  Dead means equal (1 - alpha) ubm_mean; weights and sigmas are the UBM's bits; live means meet the gates.  32
    mixtures keep the split-bf16 layout in range (engine 3); 40 go to the float64 iterations (engine 5)."""
    go = oracle_built
    rng = np.random.default_rng(106)
    for K, D, n, dead, split in ((32, 13, 300, [2, 9, 30], True), (40, 13, 300, [1, 20, 33, 39], False)):
        X, ubm = _map_case(rng, K, D, n, dead)
        for N in (1, 2):
            want = _oracle(go, ubm, X, N, ubm=ubm)
            for opt, eng_want in _paths(K, split):
                it, p, eng = _map(opt, X, ubm, N)
                tag = (K, N, opt)
                assert it == N and eng == eng_want, (tag, it, eng)
                _check_map(p, want, ubm, dead, eng, tag)


def test_em_collapsed_dimension_and_min_covar(built_lib, oracle_built):
    """Case 6: one feature column constant over all frames, min_covar 0.01 and 0.25: that column's sigma is the floor
    sqrt(min_covar) in every mixture, exactly; the rest against the oracle.  And one mixture on identical frames: every sigma
    the floor."""
    go = oracle_built
    rng = np.random.default_rng(107)
    for K, D, n in ((16, 13, 1500), (40, 13, 1500)):
        cent = 3.0 + rng.normal(0, 2, (K, D))
        cent[:, 4] = 2.5 + 0.2 * rng.standard_normal(K)
        X = _data(rng, n, cent)
        X[:, 4] = 2.5
        start = (np.full(K, 1.0 / K), R6(cent + 0.2 * rng.standard_normal(cent.shape)), np.full((K, D), 0.9))
        for mc in (0.01, 0.25):
            want = _oracle(go, start, X, 3, min_covar=mc)
            for opt, eng_want in _paths(K):
                it, p, eng = _fit(opt, X, start, 3, min_covar=mc)
                tag = (K, mc, opt)
                assert it == 3 and eng == eng_want, (tag, it, eng)
                assert np.all(p[2][:, 4] == np.sqrt(mc)) and np.all(want.sigma[:, 4] == np.sqrt(mc)), (tag, p[2][:, 4])
                assert np.all(p[2] >= np.sqrt(mc)), tag
                _gates(p, want, eng, tag)
    x0 = (3.0 + rng.normal(0, 2, 13)).astype(np.float32)
    X = np.tile(x0, (100, 1))
    start = (np.ones(1), R6(x0 + 0.1).reshape(1, 13), np.full((1, 13), 0.9))
    for mc in (1e-3, 0.01, 0.25):
        want = _oracle(go, start, X, 2, min_covar=mc)
        for opt, eng_want in _paths(1):
            it, p, eng = _fit(opt, X, start, 2, min_covar=mc)
            tag = (1, mc, opt)
            assert it == 2 and eng == eng_want, (tag, it, eng)
            assert p[0][0] == 1.0 and np.all(p[2] == np.sqrt(mc)) and np.all(want.sigma == np.sqrt(mc)), (tag, p)
            _gates(p, want, eng, tag)


def test_whole_fit_fewer_frames_than_mixtures(built_lib, oracle_built):
    """Case 7: 32 mixtures on 20 frames, 12 of the starting centres out of reach."""
    go = oracle_built
    rng = np.random.default_rng(108)
    K, D = 32, 13
    dead = list(range(20, 32))
    cent = 30.0 + rng.normal(0, 2, (K, D))
    X = (cent[:20] + rng.normal(0, 0.7, (20, D))).astype(np.float32)
    mean = R6(cent + 0.2 * rng.standard_normal(cent.shape))
    mean[dead] += 1000.0
    start = (np.full(K, 1.0 / K), mean, np.full((K, D), 0.9))
    for N in (1, 3):
        want = _oracle(go, start, X, N)
        for opt, eng_want in _paths(K):
            it, p, eng = _fit(opt, X, start, N)
            tag = (N, opt)
            assert it == N and eng == eng_want, (tag, it, eng)
            _dead_em(p, want, dead, 1e-3, eng, tag)
            _gates(p, want, eng, tag)


def test_legacy_symbols_with_dead_mixtures(built_lib, oracle_built):
    """Case 8: cases 1 and 5 through train_model / train_model_from_ubm (double** rows, pygmm.hh:33-34), as the reference's
    binding calls them."""
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd._lib import Parameter
    from speaker_recognition_amd.pygmm import GMM
    go, L = oracle_built, built_lib
    rng = np.random.default_rng(109)

    def rows(X):
        X = np.ascontiguousarray(X, dtype=np.float64)
        return X, (C.POINTER(C.c_double) * X.shape[0])(*[C.cast(X[i].ctypes.data, C.POINTER(C.c_double)) for i in range(X.shape[0])])

    K, D, n, dead = 16, 13, 1500, [3, 11]
    X, start = _far_em_case(rng, K, D, n, dead)
    Xd, r = rows(X)
    for N in (1, 2):
        g = GMM.from_arrays(*start)
        p = Parameter(nr_instance=n, nr_dim=D, nr_mixture=K, min_covar=1e-3, threshold=0.0, nr_iteration=N, init_with_kmeans=-1,
                      concurrency=4, verbosity=0)
        L.train_model(g.gmm, r, C.byref(p))
        assert _lib.last_em_stats_engine() == 4
        want = _oracle(go, start, X, N)
        _dead_em(g.params(), want, dead, 1e-3, 4, N)
        _gates(g.params(), want, 4, N)
    K, dead = 32, [2, 9, 30]
    X, ubm = _map_case(rng, K, D, 300, dead)
    Xd, r = rows(X)
    u = GMM.from_arrays(*ubm)
    for N in (1, 2):
        spk = GMM(K)
        p = Parameter(nr_instance=300, nr_dim=D, nr_mixture=K, min_covar=1e-3, threshold=0.0, nr_iteration=N, init_with_kmeans=0,
                      concurrency=4, verbosity=0)
        L.train_model_from_ubm(spk.gmm, u.gmm, r, C.byref(p))
        assert _lib.last_em_stats_engine() == 4
        _check_map(spk.params(), _oracle(go, ubm, X, N, ubm=ubm), ubm, dead, 4, N)
