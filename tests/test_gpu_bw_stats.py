"""The batched Baum-Welch statistics on the device (csrc/bw_stats.hip: sr_bw_stats_batch through core.ModelSet.bw_stats,
pygmm.GMM.bw_stats and jfa.py) against the float64 restatement of tests/bw_cases.py, within the project's E-step gates:
  |N - N*| <= 1e-5 T_u,  |F - F*| <= 1e-4 max(N*[u, k], 1),  |sum_k N[u, k] - (T_u - dropped[u])| <= 1e-5 T_u,
  |ll - ll*| <= 1e-4 sum_t max(1, |ll_t*|)
(tests/test_gpu_pipeline.py::test_em_statistics_engines_vs_oracle gates the same arithmetic at 1e-5 on weights and 1e-4 on
means), plus determinism, independence of the batch and of the scratch bound, the dropped-frame rule, a cross-check through the
MAP trainer, interleaving with the scoring paths, and PCM -> features -> statistics without a download."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bw_cases as bc  # noqa: E402

pytestmark = pytest.mark.gpu

R = 128
RAGGED = (0, 1, 3, 63, 64, 65, R - 1, R, R + 1, 2 * R + 3)


@pytest.fixture(autouse=True)
def _options(built_lib):
    from speaker_recognition_amd import _lib
    yield
    _lib.set_option("bw_range_frames", 0)
    _lib.set_option("bw_scratch_mib", 1024)
    _lib.set_option("debug_verify_clean_counters", 0)


def _gmm(ubm):
    from speaker_recognition_amd.pygmm import GMM
    w, mu, var = ubm
    return GMM.from_arrays(w, mu, np.sqrt(var))


def _check(ubm, utts, what):
    """bw_stats of the utterances against the restatement: prints every figure, then asserts the four gates."""
    N, F, ll, dropped = _gmm(ubm).bw_stats(utts, ll=True)
    K, D = ubm[1].shape
    assert N.shape == (len(utts), K) and F.shape == (len(utts), K * D) and ll.shape == dropped.shape == (len(utts),)
    g = bc.gates(N, F, ll, dropped, bc.batch_stats(utts, ubm), [len(x) for x in utts])
    print("bw_stats %s: gates N %.3g F %.3g sum %.3g ll %.3g (<= 1 passes)" % (what, g["N"], g["F"], g["sum"], g["ll"]))
    assert bc.passes(g), (what, g)
    return N, F, ll, dropped


@pytest.mark.parametrize("D", [1, 13, 39, 40])
@pytest.mark.parametrize("K", [1, 17, 64, 65, 256])
def test_parity_ragged_batches(built_lib, K, D):
    from speaker_recognition_amd import _lib
    _lib.set_option("bw_range_frames", R)              # several ranges at tiny sizes
    ubm = bc.make_ubm(K, D, 100 * K + D)
    utts = [bc.draw(ubm, T, 7 * K + D + i) for i, T in enumerate(RAGGED)]
    N, F, ll, dropped = _check(ubm, utts, "K=%d D=%d" % (K, D))
    assert not N[0].any() and not F[0].any() and ll[0] == 0.0 and not dropped.any()          # the empty utterance: zeros


def test_parity_default_ranges(built_lib):
    ubm = bc.make_ubm(65, 13, 5)
    utts = [bc.draw(ubm, T, 50 + T) for T in (2500, 1024, 1025, 7)]                          # 3 + 1 + 2 + 1 ranges of 1024
    _check(ubm, utts, "default ranges")


def test_parity_fixture_ubm(built_lib):
    ubm = bc.fixture_ubm()
    utts = [bc.draw(ubm, T, s) for T, s in ((37, 11), (300, 12), (3000, 13))]
    _check(ubm, utts, "fixture UBM 256 x 13")
    # the reference-shaped entry points give the same arrays
    from speaker_recognition_amd import jfa
    N, F = jfa.compute_suf_stats(utts, {"weights": ubm[0], "means": ubm[1], "variances": ubm[2]})
    N0, F0 = _gmm(ubm).bw_stats(utts)
    assert np.array_equal(N, N0) and np.array_equal(F, F0)
    n1, f1 = jfa.collect_suf_stats(utts[1].T, ubm[1].T, ubm[2].T, ubm[0].reshape(-1, 1))
    assert n1.shape == (256,) and f1.shape == (256 * 13,) and np.array_equal(n1, N0[1]) and np.array_equal(f1, F0[1])


def test_parity_far_from_the_origin(built_lib):
    """Data and model at +30 in every dimension, where sums about the origin cancel most (as the EM engine test)."""
    from speaker_recognition_amd import _lib
    _lib.set_option("bw_range_frames", R)
    ubm = bc.make_ubm(64, 13, 9, shift=30.0)
    utts = [bc.draw(ubm, T, 90 + T) for T in (500, 65, 1)]
    _check(ubm, utts, "+30")


def test_deterministic_and_independent_of_batch_and_bound(built_lib):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch, ModelSet
    _lib.set_option("bw_range_frames", R)
    K, D = 512, 39
    ubm = bc.make_ubm(K, D, 21)
    ms = ModelSet([_gmm(ubm)])
    x = bc.draw(ubm, 2 * R + 3, 22)
    others = [bc.draw(ubm, T, 30 + T) for T in (5, 0, R, 300, 64, R + 1, 1)]
    alone = ms.bw_stats(Batch.from_features([x]), ll=True)
    again = ms.bw_stats(Batch.from_features([x]), ll=True)
    assert all(np.array_equal(a, b) for a, b in zip(alone, again))                            # the same call twice
    mixed = others[:3] + [x] + others[3:]
    inside = ms.bw_stats(Batch.from_features(mixed), ll=True)
    assert all(np.array_equal(a[0], b[3]) for a, b in zip(alone, inside))                     # alone == inside a batch of 7 others
    lengths = [len(m) for m in mixed]
    assert _lib.bw_plan(K, D, lengths, R, 1 << 20)["n_groups"] >= 2 and _lib.bw_plan(K, D, lengths, R)["n_groups"] == 1
    _lib.set_option("bw_scratch_mib", 1)
    tight = ms.bw_stats(Batch.from_features(mixed), ll=True)
    assert all(np.array_equal(a, b) for a, b in zip(inside, tight))                           # 1 MiB (several groups) == the default


def test_dropped_frames(built_lib):
    from speaker_recognition_amd import _lib
    _lib.set_option("bw_range_frames", R)
    ubm = bc.make_ubm(17, 13, 31)
    clean = bc.draw(ubm, 200, 32)
    dirty = np.insert(clean, (40, 150), 0.0, axis=0)
    dirty[40, 5] = np.nan
    dirty[151] = 1e30
    N, F, ll, dropped = _check(ubm, [dirty, clean], "dropped frames")
    assert dropped.tolist() == [2, 0]
    g = bc.gates(N[:1], F[:1], ll[:1], np.zeros(1, np.int64), bc.batch_stats([clean], ubm), [200])
    print("bw_stats without the two rows: gates N %.3g F %.3g sum %.3g ll %.3g" % (g["N"], g["F"], g["sum"], g["ll"]))
    assert bc.passes(g), g
    assert np.isfinite(N).all() and np.isfinite(F).all() and np.isfinite(ll).all()
    # only empty utterances, and an empty batch
    N, F, ll, dropped = _gmm(ubm).bw_stats([np.zeros((0, 13))] * 3, ll=True)
    assert N.shape == (3, 17) and not N.any() and not F.any() and not ll.any() and not dropped.any()
    N, F = _gmm(ubm).bw_stats([])
    assert N.shape == (0, 17) and F.shape == (0, 17 * 13)


def test_refusals_through_the_entry_point(built_lib):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch, ModelSet
    ms = ModelSet([_gmm(bc.make_ubm(4, 13, 1)), _gmm(bc.make_ubm(4, 13, 2))])
    feats = Batch.from_features([np.zeros((5, 13), np.float32)])
    for call, pat in ((lambda: ms.bw_stats(feats, 2), r"model index 2 outside \[0, 2\)"),
                      (lambda: ms.bw_stats(Batch.from_pcm([np.zeros(100, np.int16)])), "take a feature batch"),
                      (lambda: ms.bw_stats(Batch.from_features([np.zeros((5, 12), np.float32)])), "feature dim 12 != model dim 13"),
                      (lambda: _gmm(bc.make_ubm(4, 41, 3)).bw_stats([np.zeros((5, 41))]), "up to 40 dimensions")):
        with pytest.raises(_lib.SRError, match=pat):
            call()
    assert ms.bw_stats(feats, 1)[0].shape == (1, 4)


def test_map_supervector_equals_one_map_iteration(built_lib):
    """map_supervectors(N, F, ubm) is the MAP trainer's means after one iteration from the same UBM (gmmubm.cc:53-74), within the
    project's mean gate of 1e-4 absolute."""
    from speaker_recognition_amd import jfa
    from speaker_recognition_amd.pygmm import GMM
    ubm = bc.make_ubm(64, 13, 41)
    g = _gmm(ubm)
    x = bc.draw(ubm, 500, 42)
    N, F = g.bw_stats([x])
    sv = jfa.map_supervectors(N, F, g).reshape(64, 13)
    spk = GMM(nr_mixture=64, nr_iteration=1, seed=1)
    spk.fit(x, ubm=g)
    err = float(np.max(np.abs(sv - spk.params()[1])))
    print("map_supervectors vs one MAP iteration: max |diff| %.3g (gate 1e-4)" % err)
    assert err <= 1e-4


def test_interleaved_with_scoring_paths(built_lib):
    from speaker_recognition_amd import _lib, synth
    from speaker_recognition_amd.core import Batch, MfccExtractor, ModelSet, ServingStream
    from speaker_recognition_amd.pygmm import GMM
    _lib.set_option("debug_verify_clean_counters", 1)
    ex = MfccExtractor(16000, win_length_ms=25, win_shift_ms=10)
    pcm = [synth.synth_speech(s, 0.5) for s in range(3)]
    pb = Batch.from_pcm(pcm)
    ms = ModelSet([GMM.from_arrays(*synth.synth_gmm(32, 13, 7 + s)) for s in range(4)])
    feats = ex.extract_batch(pb)
    win = 8000
    tick = np.concatenate([p[:win] for p in pcm]).astype(np.int16)
    plain, graph = ServingStream(ex, ms, 3, win), ServingStream(ex, ms, 3, win, graph=True)

    def ticks(st):
        st.submit(tick)
        return st.collect()[:2]

    # every scoring path on its own first (the second graph tick replays the capture)
    want = {"score": ms.score(feats), "fused": ex.predict_batch(ms, pb), "plain": ticks(plain), "graph": [ticks(graph), ticks(graph)][1]}
    first = ms.bw_stats(feats, 1, ll=True)

    def same(got, key):
        assert all(np.array_equal(a, b) for a, b in zip(got, want[key])), key

    def bw():
        assert all(np.array_equal(a, b) for a, b in zip(ms.bw_stats(feats, 1, ll=True), first))

    same(ms.score(feats), "score")
    bw()
    same(ex.predict_batch(ms, pb), "fused")
    bw()
    same(ticks(plain), "plain")
    same(ticks(graph), "graph")
    bw()
    same(ticks(graph), "graph")
    same(ms.score(feats), "score")


def test_pcm_to_statistics_without_a_download(built_lib):
    from speaker_recognition_amd import synth
    from speaker_recognition_amd.core import Batch, MfccExtractor, ModelSet
    ex = MfccExtractor(16000, win_length_ms=25, win_shift_ms=10)
    feats = ex.extract_batch(Batch.from_pcm([synth.synth_speech(s, 0.6) for s in range(3)]), nd=2)
    assert feats.dim == 39
    X, off = feats.download(), feats.offsets()
    ubm = bc.make_ubm(65, 39, 51)
    ubm = (ubm[0], ubm[1] * 0.3, ubm[2])               # (CMVN features: unit variance around 0)
    ms = ModelSet([_gmm(ubm)])
    direct = ms.bw_stats(feats, ll=True)
    again = ms.bw_stats(Batch.from_features([X[off[u]:off[u + 1]] for u in range(3)]), ll=True)
    assert all(np.array_equal(a, b) for a, b in zip(direct, again))
    g = bc.gates(*direct, bc.batch_stats([X[off[u]:off[u + 1]].astype(np.float64) for u in range(3)], ubm), np.diff(off))
    print("bw_stats on MFCC features: gates N %.3g F %.3g sum %.3g ll %.3g" % (g["N"], g["F"], g["sum"], g["ll"]))
    assert bc.passes(g), g
