"""Full-covariance GMMs on the MI355X (csrc/gmm_full.hip, skgmm.py): scoring against scikit-learn's answers and the float64
restatement, bit-stable sums, EM from explicit and k-means initialisations, the collapsed case, and the speaker-ID path end to end."""
import os
import pickle
import subprocess
import sys
import warnings

import numpy as np
import pytest

import fullcov_oracle as fo
from conftest import ll_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    return fo.load_golden(os.path.join(ROOT, "tests", "golden", "fullcov_golden.npz"))


def _model(rng, K, D):
    from speaker_recognition_amd import skgmm
    return skgmm.GMM.from_arrays(*fo.random_model(rng, K, D))


def _rel(a, b):
    """norm-wise relative difference ||a - b|| / ||b|| (EM carries float64 rounding of a different summation order forward)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(1e-300, float(np.linalg.norm(b))))


@pytest.mark.parametrize("c", ["k1d1", "k4d13", "k32d28", "k4d39"])
def test_scores_match_sklearn_golden(g, c):
    from speaker_recognition_amd import skgmm
    p = "score_%s_" % c
    m = skgmm.GMM(len(g[p + "w"]))
    m._set_params(g[p + "w"], g[p + "mu"], np.zeros_like(g[p + "P"]), g[p + "P"])
    ll = m.score_samples(g[p + "X"])
    assert ll_close(ll, g[p + "ll"], 1e-4) <= 1.0


@pytest.mark.parametrize("D", [1, 2, 13, 28, 31, 32, 33, 39, 63, 64])      # 32 | 33: the two built kernels; 2: one MFMA step
def test_scores_ragged_batches_against_the_restatement(D):
    from speaker_recognition_amd import skgmm
    from speaker_recognition_amd.core import Batch
    rng = np.random.default_rng(D)
    Ks = [1, 32, 33, 100, 7, 32, 1]
    models = [fo.random_model(rng, K, D) for K in Ks]
    gmms = [skgmm.GMM.from_arrays(*m) for m in models]
    lens = [1, 300, 17, 64, 1, 129, 250]
    utts = []
    for u, n in enumerate(lens):
        x = fo.draw(rng, models[u % len(models)], n)
        if u == 3:
            x[::5] += 60.0                           # outlier frames
        utts.append(x.astype(np.float32))
    fs = skgmm.FullSet(gmms)
    sums, arg, fll = fs.score(Batch.from_features(utts), frame_ll=True)
    X = np.concatenate(utts).astype(np.float64)
    off = np.concatenate([[0], np.cumsum(lens)])
    ref_sums = np.zeros((len(lens), len(gmms)))
    for s, (w, mu, cov) in enumerate(models):
        want = fo.score_samples(X, w, mu, fo.precision_cholesky(cov))
        assert ll_close(fll[s], want, 1e-4) <= 1.0, (D, s, ll_close(fll[s], want, 1e-4))
        for u in range(len(lens)):
            ref_sums[u, s] = want[off[u]:off[u + 1]].sum()
            assert abs(sums[u, s] - ref_sums[u, s]) <= 1e-4 * max(1.0, np.abs(want[off[u]:off[u + 1]]).sum())
    # (restatement's argmax wherever its winner is clear of fp32 rounding)
    for u in range(len(lens)):
        srt = np.sort(ref_sums[u])[::-1]
        if len(srt) < 2 or srt[0] - srt[1] > 1e-3 * abs(srt[0]):
            assert arg[u] == int(np.argmax(ref_sums[u]))


@pytest.mark.parametrize("S", [1, 7, 64])
def test_sets_of_many_models(S):
    from speaker_recognition_amd import skgmm
    from speaker_recognition_amd.core import Batch
    rng = np.random.default_rng(100 + S)
    models = [fo.random_model(rng, 8, 28) for _ in range(S)]
    utts = [fo.draw(rng, models[u % S], 120).astype(np.float32) for u in range(5)]
    sums, arg, _ = skgmm.FullSet([skgmm.GMM.from_arrays(*m) for m in models]).score(Batch.from_features(utts))
    X = np.concatenate(utts).astype(np.float64)
    for u in range(5):
        ref = [fo.score_samples(X[120 * u:120 * (u + 1)], m[0], m[1], fo.precision_cholesky(m[2])).sum() for m in models]
        assert ll_close(sums[u], ref, 1e-4) <= 1.0
        assert arg[u] == int(np.argmax(ref))


def test_identical_models_give_the_lower_index():
    from speaker_recognition_amd import skgmm
    from speaker_recognition_amd.core import Batch
    rng = np.random.default_rng(5)
    model = fo.random_model(rng, 4, 13)
    other = fo.random_model(rng, 4, 13)
    gm = [skgmm.GMM.from_arrays(*other), skgmm.GMM.from_arrays(*model), skgmm.GMM.from_arrays(*model)]
    x = fo.draw(rng, model, 200).astype(np.float32)
    sums, arg, _ = skgmm.FullSet(gm).score(Batch.from_features([x]))
    assert sums[0, 1] == sums[0, 2] and arg[0] == 1


def test_sums_are_bit_stable_across_calls_and_batches():
    from speaker_recognition_amd import skgmm
    from speaker_recognition_amd.core import Batch
    rng = np.random.default_rng(9)
    models = [fo.random_model(rng, 32, 28) for _ in range(3)]
    fs = skgmm.FullSet([skgmm.GMM.from_arrays(*m) for m in models])
    target = fo.draw(rng, models[1], 777).astype(np.float32)
    other = [fo.draw(rng, models[0], n).astype(np.float32) for n in (5, 1000, 33)]
    a, _, _ = fs.score(Batch.from_features([target]))
    b, _, _ = fs.score(Batch.from_features([target]))
    c, _, _ = fs.score(Batch.from_features([other[0], other[1], target, other[2]]))
    d, _, _ = fs.score(Batch.from_features([other[2], target]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[2]) and np.array_equal(a[0], d[1])


@pytest.mark.parametrize("c", ["k1d1", "k4d13", "k32d28", "k4d39"])
def test_fit_from_explicit_inits_matches_sklearn(g, c):
    from speaker_recognition_amd import skgmm
    X = g["fit_%s_X" % c].astype(np.float64)
    K = len(g["fit_%s_w0" % c])
    kw = dict(weights_init=g["fit_%s_w0" % c], means_init=g["fit_%s_mu0" % c], precisions_init=g["fit_%s_prec0" % c])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", skgmm.ConvergenceWarning)
        m5 = skgmm.GMM(K, tol=0.0, max_iter=5, **kw).fit(X)
    t = "fit5_%s_" % c
    assert m5.n_iter_ == 5 and not m5.converged_
    for attr, key in (("weights_", "w"), ("means_", "mu"), ("covariances_", "cov")):
        assert _rel(getattr(m5, attr), g[t + key]) < 1e-9, (attr, _rel(getattr(m5, attr), g[t + key]))
    # the inverse Cholesky factor inherits its covariance's condition number: k32d28 has a component near 1e5, where merely
    # reordering the frames moves scikit-learn's own factor by 1.3e-9 (the covariances agree to 1e-13 all the same)
    cond = max(np.linalg.cond(c) for c in g[t + "cov"])
    assert _rel(m5.precisions_cholesky_, g[t + "P"]) < max(1e-9, 1e-13 * cond)
    mc = skgmm.GMM(K, **kw).fit(X)
    t = "fitc_%s_" % c
    assert mc.n_iter_ == int(g[t + "n_iter"]) and int(mc.converged_) == int(g[t + "converged"])
    assert abs(mc.lower_bound_ - float(g[t + "lower_bound"])) < 1e-10 * max(1.0, abs(float(g[t + "lower_bound"])))
    assert _rel(mc.means_, g[t + "mu"]) < 1e-9


def test_kmeans_init_fit_is_reproducible_and_converged():
    from speaker_recognition_amd import skgmm
    rng = np.random.default_rng(21)
    X = fo.draw(rng, fo.random_model(rng, 8, 28), 5600)
    a = skgmm.GMM(32, random_state=7).fit(X)
    b = skgmm.GMM(32, random_state=7).fit(X)
    for attr in ("weights_", "means_", "covariances_", "precisions_cholesky_"):
        assert np.array_equal(getattr(a, attr), getattr(b, attr))
    assert a.n_iter_ == b.n_iter_ and a.lower_bound_ == b.lower_bound_
    assert a.converged_
    b0, b1, _ = fo.em_iteration(X, a.weights_, a.means_, a.precisions_cholesky_)
    assert abs(b0 - a.lower_bound_) < a.tol and abs(b1 - b0) < a.tol
    c = skgmm.GMM(32).fit(X)                          # random_state=None: the library's fixed seed
    d = skgmm.GMM(32, random_state=skgmm.DEFAULT_SEED).fit(X)
    assert np.array_equal(c.means_, d.means_)


def test_collapsed_component_raises_and_the_process_stays_usable(g):
    from speaker_recognition_amd import skgmm
    kw = dict(weights_init=g["collapsed_w0"], means_init=g["collapsed_mu0"], precisions_init=g["collapsed_prec0"])
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        skgmm.GMM(2, reg_covar=0.0, **kw).fit(g["collapsed_X"])
    m = skgmm.GMM(2, **kw).fit(g["collapsed_X"])
    assert np.all(np.isfinite(m.means_))
    assert np.all(np.isfinite(m.score_samples(g["collapsed_X"])))


def _speakers(n_spk=10):
    from speaker_recognition_amd import synth
    # (speakers 9 apart, as test_gpu_pipeline's round trip: neighbours of the synthetic family differ by 12 Hz of f0 only)
    train = [synth.synth_speech(9 * s, 8.0, seed=1000 + s) for s in range(n_spk)]
    test = [synth.synth_speech(9 * s, 4.0, seed=2000 + s) for s in range(n_spk)]
    return train, test


def test_model_interface_full_end_to_end(tmp_path):
    from speaker_recognition_amd.feature import mix_feature
    from speaker_recognition_amd.interface import ModelInterface
    train, test = _speakers()
    m = ModelInterface(covariance_type="full", verbose=False)
    for s, sig in enumerate(train):
        m.enroll("spk%d" % s, 16000, sig)
    m.train()
    labels = [m.predict(16000, sig) for sig in test]
    assert labels == ["spk%d" % s for s in range(len(test))]
    # the restatement on the trained parameters picks the same speakers
    for s, sig in enumerate(test):
        x = np.asarray(mix_feature((16000, sig)), np.float32).astype(np.float64)
        ref = [fo.score_samples(x, gm.weights_, gm.means_, gm.precisions_cholesky_).sum() for gm in m.gmmset.gmms]
        assert m.gmmset.y[int(np.argmax(ref))] == labels[s]
    p = str(tmp_path / "full.model")
    m.dump(p)
    r = ModelInterface.load(p)
    assert [r.predict(16000, sig) for sig in test] == labels
    assert r.predict_many([(16000, sig) for sig in test], gpus=2) == labels
    feats = [m._features(16000, sig) for sig in test]
    assert m.gmmset.predict(feats) == [m.gmmset.predict_one(f) for f in feats]
    assert pickle.loads(pickle.dumps(m.gmmset.gmms[0])).score(feats[0]) == m.gmmset.gmms[0].score(feats[0])


def test_cli_full_covariance(tmp_path):
    from scipy.io import wavfile
    train, test = _speakers(3)
    for s in range(3):
        d = tmp_path / ("spk%d" % s)
        d.mkdir()
        wavfile.write(str(d / "a.wav"), 16000, train[s])
        wavfile.write(str(tmp_path / ("t%d.wav" % s)), 16000, test[s])
    model = str(tmp_path / "m.out")
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "speaker-recognition.py")]
    r = subprocess.run(cmd + ["-t", "enroll", "-i", str(tmp_path / "spk*"), "-m", model, "--covariance", "full"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run(cmd + ["-t", "predict", "-i", str(tmp_path / "t*.wav"), "-m", model], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    for s in range(3):
        assert "t%d.wav -> spk%d" % (s, s) in r.stdout, r.stdout
