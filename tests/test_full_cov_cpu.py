"""Full-covariance GMMs without a GPU: the float64 restatement against scikit-learn's answers, the new C symbols, argument checks,
pickling, and the kernels' scratch (tests/golden/make_fullcov_golden.py, csrc/gmm_full.hip, skgmm.py)."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

import fullcov_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE_CASES = ["k1d1", "k4d13", "k32d28", "k4d39"]
FIT_CASES = ["k1d1", "k4d13", "k32d28", "k4d39"]
NEW_SYMBOLS = ["sr_fullgmm_create", "sr_fullgmm_fit", "sr_fullgmm_info", "sr_fullgmm_get", "sr_fullgmm_free", "sr_fullset_create",
               "sr_fullset_score_batch", "sr_fullset_free"]


@pytest.fixture(scope="module")
def g():
    return fo.load_golden(os.path.join(ROOT, "tests", "golden", "fullcov_golden.npz"))


def test_golden_fixture_is_small():
    """the fixture is stored compactly (make_fullcov_golden.py): int16 frames on a 1/256 grid, upper triangles"""
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "fullcov_golden.npz")) < 512 * 1024


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


@pytest.mark.parametrize("c", SCORE_CASES)
def test_oracle_scores_match_sklearn(g, c):
    p = "score_%s_" % c
    ll = fo.score_samples(g[p + "X"], g[p + "w"], g[p + "mu"], g[p + "P"])
    assert _rel(ll, g[p + "ll"]) < 1e-12


@pytest.mark.parametrize("c", FIT_CASES)
def test_oracle_fits_match_sklearn(g, c):
    X = g["fit_%s_X" % c]
    P0 = fo.precisions_to_cholesky(g["fit_%s_prec0" % c])
    for tag, tol, it in (("fit5_%s_" % c, 0.0, 5), ("fitc_%s_" % c, 1e-3, 100)):
        r = fo.fit(X, g["fit_%s_w0" % c], g["fit_%s_mu0" % c], P0, tol=tol, max_iter=it)
        assert r["n_iter"] == int(g[tag + "n_iter"]) and int(r["converged"]) == int(g[tag + "converged"])
        assert abs(r["lower_bound"] - float(g[tag + "lower_bound"])) < 1e-12 * max(1.0, abs(float(g[tag + "lower_bound"])))
        for key, ref in (("weights", "w"), ("means", "mu"), ("covariances", "cov"), ("prec_chol", "P")):
            if tag + ref not in g:                   # (the fixture keeps covariances of the 5-iteration fits only)
                continue
            tol = 1e-12
            if key == "prec_chol":
                # scikit-learn's factor of the RECORDED covariances: the inverse factor moves by ~eps x the condition number
                # (1e8 in one component of k32d28) under the last-bit differences of a differently rounded E-step
                tol = max(tol, 1e-16 * max(np.linalg.cond(cv) for cv in g[tag + "cov"]))
            assert _rel(r[key], g[tag + ref]) < tol, (tag, key, _rel(r[key], g[tag + ref]))


def test_oracle_collapsed_case_fails(g):
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        fo.fit(g["collapsed_X"], g["collapsed_w0"], g["collapsed_mu0"],
               fo.precisions_to_cholesky(g["collapsed_prec0"]), reg_covar=0.0)


def test_new_symbols_exported(built_lib):
    from speaker_recognition_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in _lib.EXT_SYMBOLS
        assert hasattr(built_lib, name)


def test_create_rejects_wide_models(built_lib):
    assert not built_lib.sr_fullgmm_create(1, 65, None, None, None)
    assert b"64" in built_lib.sr_last_error()
    h = built_lib.sr_fullgmm_create(2, 3, None, None, None)
    assert h
    K, D = C.c_int(0), C.c_int(0)
    assert built_lib.sr_fullgmm_info(h, C.byref(K), C.byref(D)) == 0 and (K.value, D.value) == (2, 3)
    built_lib.sr_fullgmm_free(h)


def test_compute_calls_need_a_gpu(built_lib):
    """No CPU path: fitting, packing and scoring raise 'no HIP device' without a GPU."""
    from speaker_recognition_amd import _lib, skgmm
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    rng = np.random.default_rng(0)
    X = rng.normal(size=(50, 3))
    with pytest.raises(_lib.SRError, match="no HIP device"):
        skgmm.GMM(2).fit(X)
    m = skgmm.GMM.from_arrays(*fo.random_model(rng, 2, 3))
    with pytest.raises(_lib.SRError, match="no HIP device"):
        skgmm.FullSet([m])
    with pytest.raises(_lib.SRError, match="no HIP device"):
        m.score_samples(X)
    with pytest.raises(_lib.SRError, match="no HIP device"):
        s = skgmm.GMMSet(2)
        s.gmms, s.y = [m], ["a"]
        s.predict([X])


def test_argument_checks(built_lib):
    from speaker_recognition_amd import skgmm
    with pytest.raises(ValueError, match="pygmm"):
        skgmm.GMM(4, covariance_type="tied")
    with pytest.raises(ValueError, match="pygmm"):
        skgmm.GMM(4, covariance_type="diag")
    with pytest.raises(ValueError, match="n_init"):
        skgmm.GMM(4, n_init=2)
    with pytest.raises(ValueError, match="init_params"):
        skgmm.GMM(4, init_params="random")
    with pytest.raises(ValueError, match="64"):
        skgmm.GMM(2).fit(np.zeros((100, 65)))
    bad = np.array([np.eye(3), np.diag([1.0, -1.0, 1.0])])
    with pytest.raises(ValueError, match="positive-definite"):
        skgmm.GMM(2, weights_init=[0.5, 0.5], means_init=np.zeros((2, 3)), precisions_init=bad).fit(np.ones((10, 3)))
    with pytest.raises(ValueError, match="together"):
        skgmm.GMM(2, weights_init=[0.5, 0.5])


def test_from_arrays_pickles_without_the_device(built_lib):
    from speaker_recognition_amd import skgmm
    model = fo.random_model(np.random.default_rng(3), 4, 5)
    m = skgmm.GMM.from_arrays(*model)
    assert m._h is None
    r = pickle.loads(pickle.dumps(m))
    assert r._h is None
    assert np.array_equal(r.weights_, model[0]) and np.array_equal(r.covariances_, model[2])
    assert np.allclose(r.precisions_, np.linalg.inv(model[2]), rtol=1e-9, atol=1e-12)
    s = skgmm.GMMSet(4)
    s.gmms, s.y = [m, r], ["a", "b"]
    s2 = pickle.loads(pickle.dumps(s))
    assert s2.y == ["a", "b"] and s2._set is None


def test_interface_and_cli_take_the_covariance_option():
    from speaker_recognition_amd import cli, skgmm
    from speaker_recognition_amd.interface import ModelInterface
    assert isinstance(ModelInterface(covariance_type="full", verbose=False).gmmset, skgmm.GMMSet)
    assert not isinstance(ModelInterface(verbose=False).gmmset, skgmm.GMMSet)
    with pytest.raises(ValueError):
        ModelInterface(covariance_type="tied")
    assert cli.get_args(["-t", "enroll", "-i", "x", "-m", "y", "--covariance", "full"]).covariance == "full"
    assert cli.get_args(["-t", "enroll", "-i", "x", "-m", "y"]).covariance == "diag"


def test_gmm_full_kernels_do_not_spill(built_lib):
    import test_abi_cpu
    res = dict(test_abi_cpu._kernel_resources("gmm_full"), **test_abi_cpu._kernel_resources("gmm_full_fit"))
    names = [n for n in res if "fullcov_score_kernel" in n or "fe_" in n]
    assert len([n for n in names if "fullcov_score_kernel" in n]) == 2 and len([n for n in names if "fe_" in n]) == 10
    for name, r in res.items():
        assert r["scratch"] == 0, (name, r)
