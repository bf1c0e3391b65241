"""GPU: top-C Gaussian selection (csrc/gmm_topc.hip) against the float64 numpy restatement of its semantics (tests/topc_cases.py).

Two checks per case.  Selection: every selected index distinct and in range, its float64 term no more than the gate below the
float64 C-th largest (fp32 and float64 orderings may differ where two terms are closer than fp32 resolves: the band is for
safety, and device and float64 selections must agree as sets on at least 99 % of the frames).  Values: the per-frame values
and the sums against the restatement evaluated WITH the selection the device returned, by the project's gate, on every frame.
A sum is a sum of per-frame values that each meet the gate, so it is held to the sum of its frames' gates."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topc_cases as tc  # noqa: E402
from conftest import ll_close  # noqa: E402

pytestmark = pytest.mark.gpu


def build_set(models):
    from speaker_recognition_amd.core import ModelSet
    from speaker_recognition_amd.pygmm import GMM
    gmms = [GMM.from_arrays(*m) for m in models]
    return gmms, ModelSet(gmms)


def check_selection(sel, t_bg, C):
    n, K = t_bg.shape
    assert sel.shape == (n, C) and sel.min(initial=0) >= 0 and sel.max(initial=0) < K
    srt = np.sort(sel, axis=1)
    assert np.all(srt[:, 1:] != srt[:, :-1]), "a frame selected a component twice"
    kth = -np.sort(-t_bg, axis=1)[:, C - 1]                                        # the float64 C-th largest term
    got = np.take_along_axis(t_bg, sel.astype(np.int64), axis=1)
    assert np.all(got >= (kth - tc.GATE * np.maximum(1.0, np.abs(kth)))[:, None])
    want = np.sort(tc.select(t_bg, C), axis=1)
    differ = int(np.sum(np.any(srt != want, axis=1)))
    assert differ <= 0.01 * n, "device and float64 selections differ on %d of %d frames" % (differ, n)
    assert np.all(got[:, 1:] <= got[:, :-1] + tc.GATE * np.maximum(1.0, np.abs(got[:, :-1]))), "rows are in descending term order"


def check_values(fll, sums, arg, X, off, models, bg, C, sel, clamp=True):
    ref, _ = tc.frame_ll(X, models, bg, C, selection=sel, clamp_compat=clamp)
    assert fll.shape == ref.shape
    worst = ll_close(fll, ref)
    assert worst <= tc.GATE, worst                                                 # every frame, every model
    want = tc.sums(ref, off)
    gate = tc.sums(tc.GATE * np.maximum(1.0, np.abs(ref)), off)                    # the sum of the frames' gates
    assert np.all(np.abs(sums - want) <= gate + 1e-9), float(np.max(np.abs(sums - want) - gate))
    # the sums are the float64 sums of the per-frame values the call returned
    own = tc.sums(fll.astype(np.float64), off)
    assert np.allclose(sums, own, rtol=1e-12, atol=1e-9)
    assert np.array_equal(arg, tc.argmax_first(sums, np.diff(off)))                # first maximum over ALL columns, -1 when empty


@pytest.mark.parametrize("K,C,D,S,bg", tc.GRID)
def test_grid_of_small_shapes(built_lib, K, C, D, S, bg):
    from speaker_recognition_amd.core import Batch
    seed = tc.case_seed(K, C, D, S, bg)
    models = tc.make_models(K, D, S, bg, seed)
    utts = tc.make_utts(models, bg, tc.LENGTHS, seed)
    X, off = np.concatenate(utts), tc.offsets_of(utts)
    _, ms = build_set(models)
    sums, arg, fll, sel = ms.score_topc(Batch.from_features(utts), bg, C, frame_ll=True, selection=True)
    check_selection(sel, tc.terms(X, models[bg]), C)
    check_values(fll, sums, arg, X, off, models, bg, C, sel)
    assert arg[0] == -1 and np.all(sums[0] == 0.0)                                 # the empty utterance


def test_refusals_through_the_entry_points(built_lib):
    from speaker_recognition_amd import _lib, synth
    from speaker_recognition_amd.core import Batch, MfccExtractor
    models = tc.make_models(8, 13, 3, 0, 5)
    _, ms = build_set(models)
    feats = Batch.from_features([np.zeros((5, 13), np.float32)])
    for bg, C, pat in ((-1, 2, r"background column -1 outside \[0, 3\)"), (3, 2, "outside"), (0, 0, r"top_c 0 outside \[1, 8\]"),
                       (0, 9, r"top_c 9 outside \[1, 8\]")):
        with pytest.raises(_lib.SRError, match=pat):
            ms.score_topc(feats, bg, C)
    pcm = Batch.from_pcm([synth.synth_speech(0, 0.5)])
    with pytest.raises(_lib.SRError, match="takes a feature batch.*sr_predict_pcm_batch_topc"):
        ms.score_topc(pcm, 0, 2)
    untied = [synth.synth_gmm(8, 13, s) for s in range(3)]
    _, loose = build_set(untied)
    with pytest.raises(_lib.SRError, match="share sigma and weights.*sr_score_batch_set"):
        loose.score_topc(feats, 0, 2)
    ex = MfccExtractor(16000, win_length_ms=25, win_shift_ms=10)
    with pytest.raises(_lib.SRError, match="share sigma and weights"):
        ex.predict_batch_topc(loose, pcm, 0, 2)
    with pytest.raises(_lib.SRError, match="takes a PCM batch"):
        ex.predict_batch_topc(ms, feats, 0, 2)
    ms.score(feats)                                                                # and the exact path is as it was
    loose.score(feats)


def test_tie_rule(built_lib):
    """Two components identical in mu, sigma and w, frames near them: the lower index first, in every run."""
    from speaker_recognition_amd import synth
    from speaker_recognition_amd.core import Batch
    w, mean, sigma = synth.synth_gmm(6, 13, 77)
    for a, b in ((1, 4), (0, 5)):
        mean2, sigma2, w2 = mean.copy(), sigma.copy(), w.copy()
        mean2[b], sigma2[b], w2[b] = mean2[a], sigma2[a], w2[a]
        ubm = (w2, mean2, sigma2)
        models = [ubm, synth.synth_map_speaker(ubm, 3)]
        rng = np.random.default_rng(a)
        X = (mean2[a] + 0.05 * sigma2[a] * rng.standard_normal((200, 13))).astype(np.float32)
        t = tc.terms(X, ubm)
        assert np.all(np.argmax(t, axis=1) == a) and np.all(t[:, a] == t[:, b])    # the twins lead, exactly equal in float64
        _, ms = build_set(models)
        feats = Batch.from_features([X])
        first = None
        for _ in range(2):
            sel1 = ms.score_topc(feats, 0, 1, selection=True)[2]
            sel2 = ms.score_topc(feats, 0, 2, selection=True)[2]
            assert np.all(sel1[:, 0] == a), "the lower index is chosen first"
            assert np.all(sel2[:, 0] == a) and np.all(sel2[:, 1] == b)
            sel3 = ms.score_topc(feats, 0, 6, selection=True)[2]
            check_selection(sel3, t, 6)
            if first is None:
                first = (sel1, sel2, sel3)
            assert all(np.array_equal(x, y) for x, y in zip(first, (sel1, sel2, sel3)))


@pytest.mark.parametrize("K,D,S,bg", [(5, 39, 65, 32), (33, 1, 2, 1), (64, 13, 4, 0), (512, 39, 2, 0), (8, 40, 3, 2), (16, 64, 3, 1)])
def test_all_components_reproduce_the_exact_path(built_lib, K, D, S, bg):
    from speaker_recognition_amd.core import Batch
    seed = tc.case_seed(K, K, D, S, bg)
    models = tc.make_models(K, D, S, bg, seed)
    utts = tc.make_utts(models, bg, tc.LENGTHS, seed)
    _, ms = build_set(models)
    feats = Batch.from_features(utts)
    e_sums, e_arg, e_fll = ms.score(feats, frame_ll=True)
    sums, arg, fll = ms.score_topc(feats, bg, K, frame_ll=True)
    worst = ll_close(fll, e_fll)
    assert worst <= tc.GATE, worst
    assert np.array_equal(arg, e_arg)
    gate = tc.sums(tc.GATE * np.maximum(1.0, np.abs(e_fll.astype(np.float64))), tc.offsets_of(utts))
    assert np.all(np.abs(sums - e_sums) <= gate + 1e-9)


def test_routing_edges(built_lib):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    # every frame the same: one list holds all of a slot's entries, K - C lists hold none
    K, C, D, S = 33, 3, 13, 5
    models = tc.make_models(K, D, S, 0, 900)
    _, ms = build_set(models)
    one = tc.make_utts(models, 0, (1,), 900)[0]
    X = np.repeat(one, 700, axis=0)
    utts = [X[:300], X[300:]]
    off = tc.offsets_of(utts)
    sums, arg, fll, sel = ms.score_topc(Batch.from_features(utts), 0, C, frame_ll=True, selection=True)
    assert np.all(sel == sel[0]) and len(set(sel[0].tolist())) == C
    assert np.all(fll == fll[:, :1])                                               # bit-identical for identical frames
    check_values(fll, sums, arg, X, off, models, 0, C, sel)
    # K = 512 with 40 frames: most lists are empty
    models = tc.make_models(512, 39, 3, 1, 901)
    _, ms = build_set(models)
    utts = tc.make_utts(models, 1, (40,), 901)
    sums, arg, fll, sel = ms.score_topc(Batch.from_features(utts), 1, 5, frame_ll=True, selection=True)
    assert len(np.unique(sel)) <= 200
    check_selection(sel, tc.terms(utts[0], models[1]), 5)
    check_values(fll, sums, arg, utts[0], tc.offsets_of(utts), models, 1, 5, sel)
    # ~1000 frames in >= 3 chunks: a scratch bound of 1 MiB against 4 * 5 * 201 bytes per frame (260 frames per chunk)
    models = tc.make_models(64, 39, 201, 0, 902)
    _, ms = build_set(models)
    utts = tc.make_utts(models, 0, (300, 0, 129, 1, 571), 902)
    n = sum(len(u) for u in utts)
    feats = Batch.from_features(utts)
    assert _lib.topc_plan(64, 39, 201, 5, n, 1 << 20)["n_chunks"] >= 3 and _lib.topc_plan(64, 39, 201, 5, n)["n_chunks"] == 1
    whole = ms.score_topc(feats, 0, 5, frame_ll=True, selection=True)
    again = ms.score_topc(feats, 0, 5, frame_ll=True, selection=True)
    for a, b in zip(whole, again):
        assert np.array_equal(a, b), "two identical calls are bit-identical"
    try:
        _lib.set_option("topc_scratch_mib", 1)
        cut = ms.score_topc(feats, 0, 5, frame_ll=True, selection=True)
        cut2 = ms.score_topc(feats, 0, 5, frame_ll=True, selection=True)
    finally:
        _lib.set_option("topc_scratch_mib", 1024)
    assert np.array_equal(cut[3], whole[3]) and np.array_equal(cut[2], whole[2])    # selections and per-frame values: equal
    assert np.allclose(cut[0], whole[0], rtol=1e-10, atol=0.0) and np.array_equal(cut[1], whole[1])
    for a, b in zip(cut, cut2):
        assert np.array_equal(a, b)
    check_values(cut[2], cut[0], cut[1], np.concatenate(utts), tc.offsets_of(utts), models, 0, 5, cut[3])


def test_clamp_and_non_finite(built_lib):
    from speaker_recognition_amd.core import Batch
    K, C, D, S, bg = 33, 5, 13, 4, 1
    models = tc.make_models(K, D, S, bg, 910)
    _, ms = build_set(models)
    utts = tc.make_utts(models, bg, (50, 65, 20), 910)
    utts[1][::3] += 60.0                                                           # a third of one utterance beyond the clamp
    X, off = np.concatenate(utts), tc.offsets_of(utts)
    for clamp in (True, False):
        sums, arg, fll, sel = ms.score_topc(Batch.from_features(utts), bg, C, frame_ll=True, selection=True, clamp_compat=clamp)
        check_selection(sel, tc.terms(X, models[bg]), C)
        check_values(fll, sums, arg, X, off, models, bg, C, sel, clamp=clamp)
        shifted = fll[:, 50:115:3]
        assert np.all(shifted == np.float32(tc.LN_1E_15)) if clamp else np.all(shifted < tc.LN_DBL_MIN)
    # one frame holding a NaN: its utterance's sums are NaN, its selection in range and distinct, the others untouched
    clean = ms.score_topc(Batch.from_features(utts), bg, C, frame_ll=True, selection=True)
    bad = [u.copy() for u in utts]
    bad[2][7, 3] = np.nan
    sums, arg, fll, sel = ms.score_topc(Batch.from_features(bad), bg, C, frame_ll=True, selection=True)
    assert np.all(np.isnan(sums[2])) and arg[2] == -1
    row = sel[115 + 7]
    assert len(set(row.tolist())) == C and row.min() >= 0 and row.max() < K
    assert np.all(np.isnan(fll[:, 115 + 7]))
    assert np.array_equal(sums[:2], clean[0][:2]) and np.array_equal(arg[:2], clean[1][:2])
    keep = np.ones(len(X), bool)
    keep[115 + 7] = False
    assert np.array_equal(fll[:, keep], clean[2][:, keep]) and np.array_equal(sel[keep], clean[3][keep])


def test_predict_from_pcm_equals_extract_then_score(built_lib):
    from speaker_recognition_amd import synth
    from speaker_recognition_amd.core import Batch, MfccExtractor
    models = tc.make_models(64, 39, 5, 0, 920)
    _, ms = build_set(models)
    ex = MfccExtractor(16000, win_length_ms=25, win_shift_ms=10)
    pcm = Batch.from_pcm([synth.synth_speech(s, 0.4 + 0.3 * s) for s in range(3)])
    sums, arg = ex.predict_batch_topc(ms, pcm, 0, 5, nd=2)
    feats = ex.extract_batch(pcm, nd=2)
    want_sums, want_arg = ms.score_topc(feats, 0, 5)
    assert np.array_equal(sums, want_sums) and np.array_equal(arg, want_arg)        # bit for bit
    assert np.all(np.isfinite(sums)) and sums.shape == (3, 5)


def test_gmmset_layers(built_lib):
    """A small MAP-enrolled set (UBM 16 x 13, 4 speakers): labels equal the restatement's, the reject decision equals
    open_set_decide on the sums the top-C pass returns, and top_c=None is today's result."""
    from speaker_recognition_amd import synth
    from speaker_recognition_amd.core import Batch, open_set_decide
    from speaker_recognition_amd.gmmset import GMMSet
    from speaker_recognition_amd.pygmm import GMM
    ubm_p = synth.synth_gmm(16, 13, 930)
    ubm = GMM.from_arrays(*ubm_p)
    gs = GMMSet(ubm=ubm, reject_threshold=0.05)
    truth = [synth.synth_map_speaker(ubm_p, 940 + s, n_frames_per_mix=400.0) for s in range(4)]
    for s, m in enumerate(truth):
        gs.fit_new(synth.draw_frames(m, 600, 950 + s).astype(np.float64), "spk%d" % s)
    utts = [synth.draw_frames(truth[i % 4], n, 960 + i) for i, n in enumerate((120, 64, 65, 200, 33, 90))]
    utts.append(synth.draw_frames(synth.synth_gmm(16, 13, 999), 80, 970))          # somebody else
    models = [ubm_p] + [tuple(np.asarray(a) for a in g.params()) for g in gs.gmms]
    X, off = np.concatenate(utts), tc.offsets_of(utts)
    n = np.diff(off)
    # the restatement's labels, with its own (float64) selection -- and they are not a coin toss: the winner leads by far more
    # than the gate can move a sum
    ref, _ = tc.frame_ll(X, models, 0, 5)
    want = tc.sums(ref, off)
    order = np.sort(want[:, 1:], axis=1)                                          # (two sums each within GATE |sum| of the restatement's)
    assert np.all(order[:, -1] - order[:, -2] > 4 * tc.GATE * np.abs(want).max(axis=1))
    want_labels = ["spk%d" % int(np.argmax(r[1:])) for r in want]
    assert gs.predict(utts, top_c=5) == want_labels
    sums, _ = gs._open_model_set().score_topc(Batch.from_features(utts), 0, 5)
    for thr in (0.05, float(np.median((want[:, 1:].max(axis=1) - want[:, 0]) / n))):
        lab, _ = open_set_decide(sums, n, 0, thr)
        got = gs.predict_with_reject_batch(utts, threshold=thr, top_c=5)
        assert got == [None if w < 0 else gs.y[w - 1] for w in lab]
    assert None in got and any(g is not None for g in got)
    # top_c=None: exactly what the calls return today
    assert gs.predict(utts, top_c=None) == gs.predict(utts) == [gs.predict_one(u.astype(np.float64)) for u in utts]
    assert gs.predict_with_reject_batch(utts, top_c=None) == gs.predict_with_reject_batch(utts)
    # a set that does not qualify raises
    from speaker_recognition_amd import _lib
    loose = GMMSet(ubm=ubm)
    for s in range(2):
        loose._append("x%d" % s, GMM.from_arrays(*synth.synth_gmm(16, 13, 980 + s)))
    with pytest.raises(_lib.SRError, match="share sigma and weights"):
        loose.predict(utts, top_c=5)
