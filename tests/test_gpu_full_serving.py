"""Serving full-covariance speaker sets from PCM on the MI355X: the fused call (FullSet.predict_pcm), the serving stream and the
multi-GPU predictor over skgmm models, the routing of ModelInterface.predict_many / the CLI's --gpus, and diagonal objects next
to full ones (csrc/gmm_full.hip's fullcov_finalize_kernel, stream.cpp, multi.cpp)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fullcov_oracle as fo
from multi_cases import long_utterances
from conftest import ll_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (D, LPC order, delta orders): mix_feature's 13 MFCC + LPC-15 (one row block), the MFCC alone, MFCC + deltas (two row blocks)
SETUPS = [(28, 15, 0), (13, 0, 0), (39, 0, 2)]


def _models_from(rng, X, S, K):
    """S models around real feature frames: K frames of X as means, half the frames' covariance (kept well conditioned)."""
    from speaker_recognition_amd import skgmm
    D = X.shape[1]
    cov0 = np.cov(X.T) + 1e-3 * np.eye(D)
    cov = 0.5 * cov0 + 0.05 * np.diag(np.diag(cov0))
    out = []
    for _ in range(S):
        mu = X[rng.choice(len(X), K, replace=False)] + 0.1 * rng.standard_normal((K, D))
        w = rng.uniform(0.5, 1.5, K)
        out.append(skgmm.GMM.from_arrays(w / w.sum(), mu, np.repeat(cov[None], K, axis=0)))
    return out


def _setup(fs, D, n_lpc, nd, S, K=8, seed=0):
    from speaker_recognition_amd import skgmm, synth
    from speaker_recognition_amd.core import MfccExtractor
    ex = MfccExtractor(fs, n_lpc=n_lpc)
    X = np.concatenate([ex.extract(synth.synth_speech(9 * s, 2.0, fs, seed=500 + s), nd=nd) for s in range(S)])
    assert X.shape[1] == D
    gmms = _models_from(np.random.default_rng(seed), X, S, K)
    return ex, gmms, skgmm.FullSet(gmms)


@pytest.mark.parametrize("D,n_lpc,nd", SETUPS)
def test_fused_matches_extract_then_score_bit_for_bit(D, n_lpc, nd):
    from speaker_recognition_amd import _lib, synth
    from speaker_recognition_amd.core import Batch
    S = {28: 8, 13: 3, 39: 5}[D]
    ex, gmms, fset = _setup(16000, D, n_lpc, nd, S, seed=D)
    rng = np.random.default_rng(D)
    secs = [1.3, 0.5, 0.01, 2.2, 0.9, 1.7, 0.35]                 # 0.01 s: no frame at all
    sigs = [synth.synth_speech(int(rng.integers(0, 40)), s, 16000, seed=700 + i) for i, s in enumerate(secs)]
    sums, arg = fset.predict_pcm(ex, Batch.from_pcm(sigs), nd=nd)
    assert sums.shape == (len(sigs), S) and arg.dtype == np.int32
    for u, sig in enumerate(sigs):
        if ex.num_frames(len(sig)) - nd <= 0:
            assert arg[u] == -1 and np.all(sums[u] == 0.0)
            continue
        f = ex.extract(sig, nd=nd)
        s1, _, fll = fset.score(Batch.from_features([f]), frame_ll=True)
        assert np.array_equal(sums[u], s1[0]), (D, u)
        assert arg[u] == int(np.argmax(sums[u] / len(f)))
        for s, g in enumerate(gmms):
            want = fo.score_samples(f.astype(np.float32).astype(np.float64), g.weights_, g.means_, g.precisions_cholesky_)
            assert ll_close(fll[s], want, 1e-4) <= 1.0, (D, u, s)
    # the caller's buffers; the same bits again
    out = (np.empty((len(sigs), S)), np.empty(len(sigs), np.int32))
    s2, a2 = fset.predict_pcm(ex, Batch.from_pcm(sigs), nd=nd, out=out)
    assert s2 is out[0] and a2 is out[1]
    assert np.array_equal(s2, sums) and np.array_equal(a2, arg)
    # an extractor of another width is refused (with LPC columns, any deltas are)
    with pytest.raises(_lib.SRError, match="columns|without deltas"):
        fset.predict_pcm(ex, Batch.from_pcm(sigs[:2]), nd=1 if nd == 0 else 0)


def test_identical_models_give_the_lower_index_on_every_path():
    from speaker_recognition_amd import skgmm, synth
    from speaker_recognition_amd.core import Batch, MfccExtractor, MultiPredictor, ServingStream
    ex = MfccExtractor(8000)
    x = ex.extract(synth.synth_speech(4, 3.0, 8000, seed=41))
    best = _models_from(np.random.default_rng(1), x, 1, 4)[0]
    far = skgmm.GMM.from_arrays(best.weights_, best.means_ + 4.0, best.covariances_)
    gm = [far, best, skgmm.GMM.from_arrays(best.weights_, best.means_, best.covariances_)]
    fset = skgmm.FullSet(gm)
    win = np.stack([synth.synth_speech(4, 1.0, 8000, seed=42 + w)[:8000] for w in range(2)])
    sums, arg = fset.predict_pcm(ex, Batch.from_pcm(list(win)))
    assert np.array_equal(sums[:, 1], sums[:, 2]) and np.all(sums[:, 1] > sums[:, 0])
    assert arg.tolist() == [1, 1]
    st = ServingStream(ex, fset, 2, 8000, graph=True)
    st.submit(win)
    s_st, a_st, _ = st.collect()
    assert a_st.tolist() == [1, 1] and np.array_equal(s_st, sums)
    mp = MultiPredictor.from_full(gm, 8000, n_slots=2, n_lpc=0)
    s_mp, a_mp = mp.predict(list(win))
    assert a_mp.tolist() == [1, 1] and np.array_equal(s_mp, sums)


def test_stream_matches_the_fused_call_plain_and_graph():
    from speaker_recognition_amd import _lib, synth
    from speaker_recognition_amd.core import Batch, ServingStream
    n_win, win, n_ticks = 6, 8000, 5
    ex, gmms, fset = _setup(8000, 28, 15, 0, 6, seed=3)
    rng = np.random.default_rng(3)
    ticks = [np.stack([synth.synth_speech(int(rng.integers(0, 40)), 1.0, 8000, seed=900 + 10 * t + w)[:win] for w in range(n_win)])
             for t in range(n_ticks)]
    want = [fset.predict_pcm(ex, Batch.from_pcm(list(t))) for t in ticks]
    big = np.concatenate([ex.extract(synth.synth_speech(s, 30.0, 8000, seed=s)) for s in range(4)])      # ~7500 frames
    for graph in (False, True):
        st = ServingStream(ex, fset, n_win, win, nd=0, graph=graph)
        with pytest.raises(_lib.SRError, match="nothing in flight"):
            st.collect()
        st.submit(ticks[0])
        st.submit(ticks[1])
        for t in range(n_ticks):
            s, a, ms = st.collect()
            assert np.array_equal(s, want[t][0]) and np.array_equal(a, want[t][1]), (graph, t)
            assert ms > 0
            if t == 1:
                # between two ticks: a larger batch on the same set reallocates its per-frame workspace under the captured
                # graphs; the next tick must be captured again, not replayed
                fset.score(Batch.from_features([big]))
            if t + 2 < n_ticks:
                st.submit(ticks[t + 2])
        del st
    raw = _lib.lib()
    assert not raw.sr_stream_create_full(ex._h, fset._h, n_win, win, 0, _lib.SR_CLAMP_COMPAT)
    assert b"SR_STREAM_GRAPH only" in raw.sr_last_error()
    assert not raw.sr_stream_create_full(ex._h, fset._h, n_win, win, 1, 0)       # LPC columns and deltas
    assert b"without deltas" in raw.sr_last_error()


def test_multi_predictor_matches_the_fused_call_for_any_slot_count():
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch, MultiPredictor
    ex, gmms, fset = _setup(16000, 28, 15, 0, 7, seed=4)
    rng = np.random.default_rng(4)
    sigs = long_utterances(16000, 160, rng)
    assert sum(len(s) for s in sigs) > 3 * 2.2e6                   # several pieces per slot, also with three slots
    want_s, want_a = fset.predict_pcm(ex, Batch.from_pcm(sigs))
    assert want_a[80] == -1 and np.all(want_s[80] == 0.0)
    try:
        for merge in (0, 1):
            _lib.set_option("multi_merge_same_device", merge)
            for n_slots in (1, 2, 3):
                mp = MultiPredictor.from_full(gmms, 16000, n_slots=n_slots)
                assert mp.n_slots == n_slots and all(0 <= d < _lib.device_count() for d in mp.slot_devices())
                for _ in range(2):                                   # (the second call reuses every piece's buffers)
                    s, a = mp.predict(sigs)
                    assert np.array_equal(s, want_s) and np.array_equal(a, want_a), (merge, n_slots)
                few_s, few_a = mp.predict(sigs[:2])
                assert np.array_equal(few_s, want_s[:2]) and np.array_equal(few_a, want_a[:2])
                none_s, none_a = mp.predict([])
                assert none_s.shape == (0, len(gmms)) and none_a.shape == (0,)
    finally:
        _lib.set_option("multi_merge_same_device", 1)
    # page-locked PCM: the slots read the caller's buffer in place
    cat = np.concatenate(sigs)
    off = np.zeros(len(sigs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in sigs])
    _lib.host_register(cat)
    try:
        s, a = MultiPredictor.from_full(gmms, 16000, n_slots=2).predict_concat(cat, off)
    finally:
        _lib.host_unregister(cat)
    assert np.array_equal(s, want_s) and np.array_equal(a, want_a)
    # deltas instead of LPC columns (two row blocks)
    ex39, gm39, fs39 = _setup(16000, 39, 0, 2, 3, seed=5)
    w39 = fs39.predict_pcm(ex39, Batch.from_pcm(sigs[:40]), nd=2)
    s, a = MultiPredictor.from_full(gm39, 16000, n_slots=2, n_lpc=0).predict(sigs[:40], nd=2)
    assert np.array_equal(s, w39[0]) and np.array_equal(a, w39[1])
    with pytest.raises(_lib.SRError, match="columns"):
        MultiPredictor.from_full(gm39, 16000, n_slots=1, n_lpc=0).predict(sigs[:3], nd=1)


def _speakers(n_spk, train_s=8.0, test_s=4.0):
    from speaker_recognition_amd import synth
    train = [synth.synth_speech(9 * s, train_s, seed=1000 + s) for s in range(n_spk)]
    test = [synth.synth_speech(9 * s, test_s, seed=2000 + s) for s in range(n_spk)]
    return train, test


def test_model_interface_full_predict_many_shards():
    from speaker_recognition_amd.core import MultiPredictor
    from speaker_recognition_amd.interface import ModelInterface
    train, test = _speakers(4)
    m = ModelInterface(covariance_type="full", verbose=False)
    for s, sig in enumerate(train):
        m.enroll("spk%d" % s, 16000, sig)
    m.train()
    items = [(16000, sig) for sig in test] + [(16000, np.zeros(50, np.int16))]
    labels = [m.predict(fs, sig) for fs, sig in items]
    assert labels[:4] == ["spk%d" % s for s in range(4)] and labels[4] is None
    assert getattr(m, "_multi", None) is None
    assert m.predict_many(items, gpus=2) == labels
    assert m._multi is not None and isinstance(m._multi[1], MultiPredictor)
    first = m._multi[1]
    assert m.predict_many(items[:2], gpus=2) == labels[:2]
    assert m._multi[1] is first                                   # cached until the models change
    assert m.predict_many(items[:4], gpus=1) == labels[:4]          # (the one-GPU path refuses the empty one: "Signal too short!")


def test_cli_predict_gpus_on_a_full_model(tmp_path):
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
    outs = []
    for gpus in ("1", "2"):
        r = subprocess.run(cmd + ["-t", "predict", "-i", str(tmp_path / "t*.wav"), "-m", model, "--gpus", gpus], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append([line for line in r.stdout.splitlines() if " -> " in line])
    assert outs[0] == outs[1] and len(outs[0]) == 3
    for s in range(3):
        assert "t%d.wav -> spk%d" % (s, s) in outs[1][s]


def test_diagonal_stream_and_multi_unchanged_next_to_full_ones():
    from speaker_recognition_amd import synth
    from speaker_recognition_amd.core import Batch, MfccExtractor, ModelSet, MultiPredictor, ServingStream
    from speaker_recognition_amd.pygmm import GMM
    n_win, win = 6, 8000
    ex = MfccExtractor(8000)
    diag = [GMM.from_arrays(*synth.synth_gmm(16, 13, 60 + s)) for s in range(4)]
    ms = ModelSet(diag)
    pcm = np.stack([synth.synth_speech(5 * w, 1.0, 8000, seed=80 + w)[:win] for w in range(n_win)])
    want = ex.predict_batch(ms, Batch.from_pcm(list(pcm)))

    def check(st, mp):
        st.submit(pcm)
        s, a, _ = st.collect()
        assert np.array_equal(s, want[0]) and np.array_equal(a, want[1])
        s, a = mp.predict(list(pcm))
        assert np.array_equal(s, want[0]) and np.array_equal(a, want[1])

    before = (ServingStream(ex, ms, n_win, win, graph=True), MultiPredictor(diag, 8000, n_slots=2))
    check(*before)
    exf, gmms, fset = _setup(8000, 13, 0, 0, 3, seed=6)
    want_f = fset.predict_pcm(exf, Batch.from_pcm(list(pcm)))
    full = (ServingStream(exf, fset, n_win, win, graph=True), MultiPredictor.from_full(gmms, 8000, n_slots=2, n_lpc=0))
    full[0].submit(pcm)
    s, a, _ = full[0].collect()
    assert np.array_equal(s, want_f[0]) and np.array_equal(a, want_f[1])
    s, a = full[1].predict(list(pcm))
    assert np.array_equal(s, want_f[0]) and np.array_equal(a, want_f[1])
    check(*before)
    check(ServingStream(ex, ms, n_win, win, graph=True), MultiPredictor(diag, 8000, n_slots=2))
