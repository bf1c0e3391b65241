"""The full-covariance EM edge table without a GPU (tests/fullfit_cases.py, tests/golden/fullfit_edge_golden.npz): the float64
restatement against scikit-learn's recorded answers on every row, and the conditions that make the table a fair yardstick for the
device (tests/test_gpu_fullfit_cases.py): the restatement's own noise floor under a permutation of the frames, the condition
numbers behind the precision-factor tolerance, the edges the rows claim to reach."""
import os

import numpy as np
import pytest

import fullcov_oracle as fo
import fullfit_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fullfit_edge_golden.npz")


@pytest.fixture(scope="module")
def g():
    return fc.load_golden(GOLDEN)


def test_fixture_is_small():
    assert os.path.getsize(GOLDEN) < 512 * 1024


def _max_cond(cov):
    return max(np.linalg.cond(cv) for cv in cov)


@pytest.mark.parametrize("name", fc.NAMES)
def test_restatement_matches_sklearn(g, name):
    """test_full_cov_cpu.py::test_oracle_fits_match_sklearn's tolerances: 1e-12 norm-wise, the precision factor of the recorded
    covariances at max(1e-12, 1e-16 x condition number)"""
    c, r, ref = fc.BY_NAME[name], fc.restated(name), g[name]
    assert r["n_iter"] == ref["n_iter"] and bool(r["converged"]) == ref["converged"]
    if c.tol == 0:
        assert r["n_iter"] == c.max_iter and not r["converged"]
    else:
        assert r["converged"]
    assert abs(r["lower_bound"] - ref["lower_bound"]) < 1e-12 * max(1.0, abs(ref["lower_bound"]))
    figures = []
    for key in ("weights", "means", "covariances", "prec_chol"):
        if ref[key] is None:
            continue
        tol = 1e-12
        if key == "prec_chol":
            tol = max(tol, 1e-16 * _max_cond(ref["covariances"]))
        figures.append((key, fc.rel(r[key], ref[key]), tol))
    print(name, " ".join("%s %.1e" % f[:2] for f in figures))
    for key, d, tol in figures:
        assert d < tol, (name, key, d)
    assert (ref["covariances"] is not None) == c.cov and (ref["score"] is not None) == (not c.cov)
    if ref["score"] is not None:
        # scikit-learn's score(X) of its fitted model: the bound a further E-step would find, through every final covariance
        X, _ = fc.build(name)
        score = fo.e_step(X, r["weights"], r["means"], r["prec_chol"])[0]
        assert abs(score - ref["score"]) < 1e-12 * max(1.0, abs(ref["score"])), (name, score, ref["score"])


@pytest.mark.parametrize("name", fc.NAMES)
def test_table_conditions(name):
    """the restatement's result does not hang on the order of the frames (so a device sum in another order has room inside 1e-9),
    and no covariance is so ill-conditioned that the precision-factor tolerance 1e-13 x cond leaves 1e-7"""
    c, r = fc.BY_NAME[name], fc.restated(name)
    X, init = fc.build(name)
    assert np.array_equal(X, np.round(X * 256.0) / 256.0) and X.shape == (c.n, c.D) and len(init[0]) == c.K
    assert np.all(np.isfinite(r["covariances"])) and np.all(np.isfinite(r["bounds"]))
    perm = fc.permutation(c.n, c.seed)
    assert np.array_equal(np.sort(perm), np.arange(c.n))
    rp = fc.oracle_fit(X[perm], init, c.reg, c.tol, c.max_iter)
    assert rp["n_iter"] == r["n_iter"] and rp["converged"] == r["converged"]
    d = [fc.rel(rp[key], r[key]) for key in ("weights", "means", "covariances")]
    cond = _max_cond(r["covariances"])
    print(name, "permuted: w %.1e mu %.1e cov %.1e; cond %.1e" % (d[0], d[1], d[2], cond))
    assert max(d) < fc.PERMUTATION_FLOOR, (name, d)
    assert cond <= fc.MAX_CONDITION, (name, cond)
    if c.tol > 0:
        changes = np.abs(np.diff(np.concatenate([[-np.inf], r["bounds"]])))
        assert np.min(np.abs(changes - c.tol)) > 1e-6 and r["n_iter"] > 2, (name, changes)


def test_table_reaches_the_edges_it_names():
    Ds = sorted(set(c.D for c in fc.CASES if c.name.startswith("slots")))
    assert Ds == [22, 23, 32, 39, 45, 50, 51, 55, 59, 60, 63, 64]
    # covariance pair slots: pairs D (D + 1) / 2 over 256 threads, at most FE_PQ = 9 (gmm_full.hip); every count once at least
    assert sorted(set((D * (D + 1) // 2 + 255) // 256 for D in Ds)) == list(range(1, 10))
    assert all((D * (D + 1) // 2 + 255) // 256 == fc.slots(D) for D in range(1, 65)) and fc.slots(64) == 9
    pairs = {D: D * (D + 1) // 2 for D in Ds}
    assert pairs[22] < 256 < pairs[23] and pairs[51] < 1536 < pairs[55] and pairs[63] < 2048 < pairs[64]
    series = sorted(c.n for c in fc.CASES if c.D == 64 and c.name.startswith("n"))
    assert series == [2, 31, 32, 33, 64, 255, 256, 257, 8192, 8193]
    assert all(c.K == (1 if c.n == 2 else 2) for c in fc.CASES if c.D == 64 and c.name.startswith("n"))
    shapes = set((c.K, c.D, c.n) for c in fc.CASES)
    assert {(7, 2, 16385), (3, 45, 8225), (1, 64, 64), (64, 3, 640), (65, 3, 650), (5, 58, 5)} <= shapes
    assert any(c.n < c.D and c.K > 1 and c.name.startswith("rank") for c in fc.CASES)
    # chunks: min(32, ceil(n / 256)) of ceil(n / chunks) frames
    chunk = {n: -(-n // min(32, -(-n // 256))) for n in (8192, 8193, 8225, 16385)}
    assert chunk == {8192: 256, 8193: 257, 8225: 258, 16385: 513}
    stops = [c for c in fc.CASES if c.tol > 0]
    assert len(stops) == 2 and all((c.tol, c.max_iter) == (1e-3, 100) for c in stops)
    assert any(c.D == 64 for c in stops) and any(c.n > 8192 for c in stops)
    assert all((c.tol, c.max_iter) == (0.0, 3) for c in fc.CASES if c not in stops)


def test_empty_component_stays_empty_and_finite():
    """no frame gives the third component any responsibility: nk = 10 eps exactly, mean 0 / nk, covariance reg_covar I -- the state
    scikit-learn carries on from -- in every one of the three iterations"""
    c = fc.BY_NAME["empty_k3_d48"]
    X, (w, mu, prec) = fc.build(c.name)
    assert (c.K, c.D, c.n) == (3, 48, 600) and np.all(mu[2] == 1000.0) and np.array_equal(prec[2], np.eye(48))
    assert np.any(np.all(X == mu[0], axis=1)) and np.any(np.all(X == mu[1], axis=1))
    P = fo.precisions_to_cholesky(prec)
    for _ in range(c.max_iter):
        _, log_resp = fo.e_step(X, w, mu, P)
        resp = np.exp(log_resp)
        assert np.all(resp[:, 2] == 0.0)
        w, mu, cov, P = fo.m_step(X, resp, c.reg)
        assert resp.sum(axis=0)[2] + 10 * np.finfo(np.float64).eps == 10 * np.finfo(np.float64).eps and abs(w[2] - 3.7e-18) < 1e-19
        assert np.all(mu[2] == 0.0) and np.array_equal(cov[2], c.reg * np.eye(48))
    r = fc.restated(c.name)
    assert np.array_equal(r["covariances"], cov) and np.all(np.isfinite(r["bounds"]))

