"""GPU: the timeline (csrc/timeline.hip: sr_timeline_decide, sr_timeline_batch, sr_fullset_timeline_batch, sr_timeline_pcm_batch,
ModelSet.timeline, ModelInterface.timeline) against the numpy restatement of its definitions (tests/timeline_oracle.py).

The gate is equality to the bit: window sums are in-order float64 sums of fp32 values, quotients one float64 division, every step
of the recurrence one float64 add or compare -- the oracle performs the same operations in the same order, so labels, sums and
path scores have no tolerance."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timeline_oracle as to  # noqa: E402

pytestmark = pytest.mark.gpu

STATES = (1, 2, 63, 64, 65, 202, 1024, 1025)
MIN_DURS = (1, 2, 3, 16)
BETAS = (0.0, 0.5, 1e300)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def window_lengths(S, m):
    from speaker_recognition_amd import _lib
    tile = _lib.timeline_plan(S, m)["tile"]
    return [0, 1, m - 1, m, m + 1, tile - 1, tile, tile + 1, 2 * tile + 3]


def synthetic(S, lengths, seed, scale=None):
    """Window sums of recordings of `lengths` windows: integer-valued doubles over counts of 1, 2 or 4, so that quotients are exact
    and ties occur in every window; `scale`: values of that magnitude instead (roundings in every add)."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(off[-1])
    counts = rng.choice([1, 2, 4], n).astype(np.int32)
    if scale is None:
        sums = (rng.integers(-3, 4, (n, S)) * counts[:, None]).astype(np.float64)
    else:
        sums = np.round(rng.normal(0.0, scale, (n, S))) * 0.5
    return sums, counts, off


def oracle_all(sums, counts, off, **kw):
    labs, paths, bads = [], [], []
    for u in range(len(off) - 1):
        lab, path, bad = to.decide(sums[off[u]:off[u + 1]], counts[off[u]:off[u + 1]], **kw)
        labs.append(lab)
        paths.append(path)
        bads.append(bad)
    return (np.concatenate(labs) if labs else np.zeros(0, np.int32)), np.array(paths), np.array(bads)


@pytest.mark.parametrize("S", STATES)
def test_decide_on_synthetic_sums(built_lib, S):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import open_set_decide
    for bg in (-1, S // 2):
        for m in MIN_DURS:
            lengths = window_lengths(S, m)
            sums, counts, off = synthetic(S, lengths, 100 * S + m)
            if m == MIN_DURS[0]:
                for mode in (0, 1):
                    lab, path, bad = _lib.timeline_decide(sums, counts, off, bg=bg, threshold=0.0, mode=mode)
                    want, _, wbad = oracle_all(sums, counts, off, bg=bg, threshold=0.0, mode=mode)
                    assert np.array_equal(lab, want) and np.isnan(path).all() and np.array_equal(bad, wbad)
                    if mode == 0 and bg >= 0:
                        open_lab, _ = open_set_decide(sums, counts, bg, 0.0)
                        assert np.array_equal(lab, open_lab)
            for beta in BETAS:
                for thr in (0.0, 1.0):
                    lab, path, bad = _lib.timeline_decide(sums, counts, off, bg=bg, threshold=thr, mode=2, beta=beta, min_dur=m)
                    want, wpath, wbad = oracle_all(sums, counts, off, bg=bg, threshold=thr, mode=2, beta=beta, m=m)
                    assert np.array_equal(lab, want), (S, bg, m, beta, thr)
                    assert np.array_equal(bits(path), bits(wpath)), (S, bg, m, beta, thr, path, wpath)
                    assert np.array_equal(bad, wbad)
    # magnitude 1e6: every add rounds
    sums, counts, off = synthetic(S, window_lengths(S, 3), 7 * S, scale=1e6)
    for m, beta in ((1, 0.5), (3, 1e5), (16, 0.0)):
        lab, path, _ = _lib.timeline_decide(sums, counts, off, bg=S - 1, threshold=-3.0, mode=2, beta=beta, min_dur=m)
        want, wpath, _ = oracle_all(sums, counts, off, bg=S - 1, threshold=-3.0, mode=2, beta=beta, m=m)
        assert np.array_equal(lab, want) and np.array_equal(bits(path), bits(wpath))


def test_decide_hold_long_alternation_and_nan(built_lib):
    from speaker_recognition_amd import _lib
    # an alternating stretch longer than 2048 windows, -1 gaps (nobody wins), in a batch with a short and an empty recording
    raw = np.array([2] + [0, 1] * 1100 + [1, 1, 3, 0, 0, 3, 3, 1] + [0, 1] * 200, dtype=np.int64)
    lengths = [len(raw), 0, 5, 300]
    rng = np.random.default_rng(4)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    sums = rng.integers(-5, 0, (int(off[-1]), 4)).astype(np.float64)
    sums[np.arange(len(raw)), raw] = 1.0                                 # column 3 is the nobody state
    counts = np.ones(len(sums), np.int32)
    lab, _, bad = _lib.timeline_decide(sums, counts, off, bg=3, mode=1)
    want, _, _ = oracle_all(sums, counts, off, bg=3, mode=1)
    assert np.array_equal(lab, want) and (lab[1:2201] == 2).all() and (lab[:len(raw)] == -1).sum() == 3 and not bad.any()
    # NaN sums: -inf, counted per recording; a window of NaN everywhere gets -1
    sums[3, :] = np.nan
    sums[10, 1] = np.nan
    sums[off[2] + 1, 0] = np.nan
    for mode, kw, okw in ((0, {}, {}), (1, {}, {}), (2, dict(beta=0.5, min_dur=2), dict(beta=0.5, m=2))):
        lab, path, bad = _lib.timeline_decide(sums, counts, off, bg=3, mode=mode, **kw)
        want, wpath, wbad = oracle_all(sums, counts, off, bg=3, mode=mode, **okw)
        assert np.array_equal(lab, want) and bad.tolist() == wbad.tolist() == [2, 0, 1, 0]
        if mode == 2:
            assert np.array_equal(bits(path), bits(wpath)) and path[0] == -np.inf and path[1] == 0.0


def test_decide_batch_equals_alone(built_lib):
    from speaker_recognition_amd import _lib
    S = 70
    lengths = [11, 0, 1, 40, 7]
    sums, counts, off = synthetic(S, lengths, 21)
    for mode, kw in ((0, {}), (1, {}), (2, dict(beta=0.5, min_dur=3))):
        lab, path, bad = _lib.timeline_decide(sums, counts, off, bg=5, threshold=0.5, mode=mode, **kw)
        for u in range(5):
            a, b = off[u], off[u + 1]
            l1, p1, b1 = _lib.timeline_decide(sums[a:b], counts[a:b], np.array([0, b - a]), bg=5, threshold=0.5, mode=mode, **kw)
            assert np.array_equal(l1, lab[a:b]) and np.array_equal(bits(p1), bits(path[u:u + 1])) and b1[0] == bad[u]
    lab, path, bad = _lib.timeline_decide(np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros(1, np.int64), mode=2, beta=1.0)
    assert len(lab) == 0 and len(path) == 0


def check_against_frames(timeline, fll, offsets, S, W, H, bg):
    """`timeline(mode, **kw)` -> (labels per recording, path scores, sums per recording) against the oracle on the frame matrix."""
    U = len(offsets) - 1
    ref = [to.window_sums(fll[:, offsets[u]:offsets[u + 1]], W, H) for u in range(U)]
    for smooth, kw, okw in (("none", {}, dict(mode=0)), ("hold", {}, dict(mode=1)),
                            ("viterbi", dict(switch_penalty=2.0, min_windows=2), dict(mode=2, beta=2.0, m=2)),
                            ("viterbi", dict(switch_penalty=0.25, min_windows=3), dict(mode=2, beta=0.25, m=3))):
        labels, path, sums = timeline(smooth=smooth, **kw)
        again = timeline(smooth=smooth, **kw)
        for u in range(U):
            wsum, wcnt = ref[u]
            assert sums[u].shape == wsum.shape and np.array_equal(bits(sums[u]), bits(wsum)), (W, H, u)
            wlab, wpath, _ = to.decide(wsum, wcnt, bg=-1 if bg is None else bg, threshold=0.25, **okw)
            assert np.array_equal(labels[u], wlab), (W, H, u, smooth)
            if smooth == "viterbi":
                assert bits(path[u]) == bits(wpath), (W, H, u, path[u], wpath)
            assert np.array_equal(again[0][u], labels[u]) and np.array_equal(bits(again[2][u]), bits(sums[u]))
        assert np.array_equal(bits(again[1]), bits(path))


WINDOWINGS = ((1, 1), (10, 5), (10, 10), (5, 8), (300, 7))


@pytest.fixture(scope="module")
def diag_case(built_lib):
    from speaker_recognition_amd import synth
    from speaker_recognition_amd.core import Batch, ModelSet
    from speaker_recognition_amd.pygmm import GMM
    models = [synth.synth_gmm(8, 13, 40 + s) for s in range(4)]
    ms = ModelSet([GMM.from_arrays(*m) for m in models])
    out = {}
    for name, frac in (("plain", 0.0), ("outliers", 0.01)):
        recs = [synth.draw_frames(models[u % 4], n, 60 + u, outlier_frac=frac) for u, n in enumerate((1, 37, 240))]
        feats = Batch.from_features(recs)
        _, _, fll = ms.score(feats, frame_ll=True)
        out[name] = (feats, fll, feats.offsets())
    return ms, out


@pytest.mark.parametrize("W,H", WINDOWINGS)
def test_batch_against_a_diagonal_set(diag_case, W, H):
    ms, cases = diag_case
    for name in ("plain", "outliers"):                                   # outliers: the clamp's patched per-frame values are the ones summed
        feats, fll, off = cases[name]
        for bg in (None, 0):
            check_against_frames(lambda **kw: ms.timeline(feats, W, H, bg=bg, threshold=0.25, scores=True, **kw), fll, off, 4, W, H, bg)


def test_fullset_timeline(built_lib):
    from speaker_recognition_amd import skgmm
    from speaker_recognition_amd.core import Batch
    rng = np.random.default_rng(9)
    D, K = 5, 2
    gmms = []
    for s in range(3):
        A = rng.normal(0, 1, (K, D, D))
        cov = A @ A.transpose(0, 2, 1) + 0.5 * np.eye(D)
        gmms.append(skgmm.GMM.from_arrays(np.full(K, 1.0 / K), rng.normal(0, 2, (K, D)), cov))
    fs = skgmm.FullSet(gmms)
    recs = [(g.means_[rng.integers(0, K, n)] + rng.normal(0, 1, (n, D))).astype(np.float32) for g, n in zip(gmms, (90, 1, 33))]
    feats = Batch.from_features(recs)
    _, _, fll = fs.score(feats, frame_ll=True)
    for W, H in ((10, 5), (5, 8), (300, 7)):
        check_against_frames(lambda **kw: fs.timeline(feats, W, H, threshold=0.25, scores=True, **kw), fll, feats.offsets(), 3, W, H, None)


def test_pcm_timeline_equals_extract_then_timeline(built_lib):
    from speaker_recognition_amd import synth
    from speaker_recognition_amd.core import Batch, MfccExtractor, ModelSet
    from speaker_recognition_amd.pygmm import GMM
    ex = MfccExtractor(16000, win_length_ms=25, win_shift_ms=10)
    pcm = Batch.from_pcm([synth.synth_speech(s, sec) for s, sec in ((0, 1.0), (1, 0.4), (2, 0.7))])
    ms = ModelSet([GMM.from_arrays(*synth.synth_gmm(8, 39, 80 + s)) for s in range(3)])
    feats = ex.extract_batch(pcm, nd=2)
    for smooth, kw in (("hold", {}), ("viterbi", dict(switch_penalty=1.0, min_windows=2))):
        want = ms.timeline(feats, 20, 8, bg=0, threshold=0.1, smooth=smooth, scores=True, **kw)
        got = ex.timeline_batch(ms, pcm, 20, 8, nd=2, bg=0, threshold=0.1, smooth=smooth, scores=True, **kw)
        for u in range(3):
            assert len(got[0][u]) == to.windows(int(np.diff(feats.offsets())[u]), 20, 8) > 0
            assert np.array_equal(got[0][u], want[0][u]) and np.array_equal(bits(got[2][u]), bits(want[2][u]))
        assert np.array_equal(bits(got[1]), bits(want[1]))


@pytest.mark.parametrize("base", (100, 200, 300))
def test_made_conversation(built_lib, base):
    """Column 0 plays the background; turns [1, 2, 3, 1, 3, 2] of 40 frames drawn from the speakers' own models.  Every window
    that lies wholly inside one turn carries that turn's speaker in modes none and viterbi (beta = 2, m = 2), and under hold
    from the turn's second such window on.  Confirmed beforehand with the oracle on a float64 CPU scorer at all three seeds."""
    from speaker_recognition_amd import synth
    from speaker_recognition_amd.core import Batch, ModelSet
    from speaker_recognition_amd.pygmm import GMM
    models = [synth.synth_gmm(8, 13, base + s) for s in range(4)]
    turns = [1, 2, 3, 1, 3, 2]
    X = np.concatenate([synth.draw_frames(models[s], 40, base + 50 + i) for i, s in enumerate(turns)])
    ms = ModelSet([GMM.from_arrays(*m) for m in models])
    feats = Batch.from_features([X])
    W, H = 10, 5
    _, _, fll = ms.score(feats, frame_ll=True)
    wsum, wcnt = to.window_sums(fll, W, H)
    inside = [(j, turns[(j * H) // 40]) for j in range(len(wsum)) if (j * H) // 40 == (j * H + W - 1) // 40]
    assert len(inside) == 6 * 7
    for smooth, kw, okw in (("none", {}, dict(mode=0)), ("hold", {}, dict(mode=1)),
                            ("viterbi", dict(switch_penalty=2.0, min_windows=2), dict(mode=2, beta=2.0, m=2))):
        lab = ms.timeline(feats, W, H, bg=0, threshold=0.0, smooth=smooth, **kw)[0]
        assert np.array_equal(lab, to.decide(wsum, wcnt, bg=0, threshold=0.0, **okw)[0])
        # hold shows a new label once two windows in a row agree: where the window astride the boundary still went to the old
        # speaker, the turn's first inside window shows the old label (the oracle on a float64 scorer: 4, 3 and 1 such windows
        # at the three seeds) -- the rule's delay, so hold is held to the windows from a turn's second inside window on
        held = [(j, s) for j, s in inside if smooth != "hold" or (j - 1, s) in inside]
        assert len(held) == (36 if smooth == "hold" else 42)
        wrong = [(j, s, int(lab[j])) for j, s in held if lab[j] != s]
        assert not wrong, (smooth, wrong)


def test_python_surface(built_lib):
    from speaker_recognition_amd import _lib, synth
    from speaker_recognition_amd.core import Batch, ModelSet
    from speaker_recognition_amd.interface import ModelInterface
    from speaker_recognition_amd.pygmm import GMM
    ms = ModelSet([GMM.from_arrays(*synth.synth_gmm(4, 13, 5 + s)) for s in range(2)])
    feats = Batch.from_features([synth.draw_frames(synth.synth_gmm(4, 13, 5), 50, 1), np.zeros((0, 13), np.float32)])
    labels = ms.timeline(feats, 10, 5)
    assert [len(x) for x in labels] == [9, 0] and labels[0].dtype == np.int32
    labels, path, sums = ms.timeline(feats, 10, 5, smooth="none", scores=True)
    assert np.isnan(path).all() and sums[0].shape == (9, 2) and sums[1].shape == (0, 2)
    for kw, exc in ((dict(window=0), _lib.SRError), (dict(hop=0), _lib.SRError), (dict(bg=2), _lib.SRError), (dict(threshold=float("nan")), _lib.SRError),
                    (dict(smooth="viterbi", switch_penalty=-1.0), _lib.SRError), (dict(smooth="viterbi", switch_penalty=1.0, min_windows=17), _lib.SRError),
                    (dict(smooth="viterbi"), ValueError), (dict(smooth="median"), ValueError)):
        with pytest.raises(exc):
            ms.timeline(feats, **dict(dict(window=10, hop=5), **kw))
    with pytest.raises(_lib.SRError, match="feature batch"):
        ms.timeline(Batch.from_pcm([np.zeros(4000, np.int16)]), 10, 5)
    # the interface: two enrolled speakers, a recording of both; the segments tile [0, duration of the features]
    m = ModelInterface(verbose=False, gmm_order=4, lpc=False, gmm_kwargs=dict(seed=3))
    clips = {name: synth.synth_speech(s, 2.0) for name, s in (("ann", 0), ("bob", 7))}
    for name, clip in clips.items():
        m.enroll(name, 16000, clip)
    m.train()
    signal = np.concatenate([clips["ann"], clips["bob"]])
    n_frames = len(m._features_of(16000, signal))
    for kw in (dict(), dict(smooth="none"), dict(smooth="viterbi", switch_penalty=1.0, min_duration_s=0.8)):
        segs = m.timeline(16000, signal, window_s=0.5, hop_s=0.25, **kw)
        assert segs[0][0] == 0.0 and abs(segs[-1][1] - n_frames * 0.016) < 1e-9
        assert all(a[1] == b[0] and a[2] != b[2] for a, b in zip(segs, segs[1:])) and all(b > a for a, b, _ in segs)
        assert {name for _, _, name in segs} <= {"ann", "bob"}
    # the names are the ones `predict` gives the same windows cut out of the recording's features
    from speaker_recognition_amd import timeline as tl
    feat = np.asarray(m._features_of(16000, signal))
    W, H = 31, 16
    cut = [feat[j * H:j * H + W] for j in range(tl.windows(n_frames, W, H))]
    want = [m.gmmset.y.index(name) for name in m.gmmset.predict(cut)]
    segs = m.timeline(16000, signal, window_s=0.5, hop_s=0.25, smooth="none")
    assert [(a, b, m.gmmset.y[lab]) for a, b, lab in tl.segments(want, n_frames, W, H, 0.016)] == segs
