"""The open-set decision on the device (csrc/open_set.hip; sr_open_set_decide, sr_score_batch_set_open, sr_predict_pcm_batch_open,
sr_stream_set_open / sr_stream_collect_open, sr_multi_predict_pcm_open): the reference's GMMSet.predict_one_with_rejection
(src/testbench/gmmset.py:69-81), restated in float64 numpy in tests/open_set_cases.py, is the yardstick.  Labels must be equal
and margins equal bit for bit (NaN where the rule gives NaN) wherever the rule is applied to the sums a call returned itself."""
import ctypes as C

import numpy as np
import pytest

import open_set_cases as oc
from conftest import ll_close

pytestmark = pytest.mark.gpu
FS, WIN = 8000, 8000


def same(got, want):
    (gl, gm), (wl, wm) = got, want
    return np.array_equal(np.asarray(gl), wl) and np.array_equal(np.asarray(gm), wm, equal_nan=True)


# ---------------------------------------------------------------- 1. the rule, bit for bit, on crafted sums

def ulp_pair():
    """(x, y, n): y is the float64 right above x, and x / n == y / n"""
    rng = np.random.default_rng(1)
    for _ in range(10000):
        x = np.float64(-rng.uniform(100, 5000))
        y = np.nextafter(x, np.inf)
        n = int(rng.integers(3, 400))
        if x / np.float64(n) == y / np.float64(n):
            return x, y, n
    raise AssertionError("no such pair found")


@pytest.mark.parametrize("S", [1, 2, 3, 64, 65, 257, 1002])
def test_rule_bit_for_bit_on_crafted_sums(built_lib, S):
    from speaker_recognition_amd.core import open_set_decide
    rng = np.random.default_rng(100 + S)
    x, y, n_ulp = ulp_pair()
    assert y > x and x / np.float64(n_ulp) == y / np.float64(n_ulp)              # the premise of the one-ulp case
    for U in (1, 4, 5, 33):
        for bg in sorted({0, S - 1, S // 2}):
            n = rng.integers(1, 700, U).astype(np.int64)
            sums = -rng.uniform(20, 90, (U, S)) * n[:, None]
            others = [s for s in range(S) if s != bg]
            if len(others) >= 2:
                a, b = others[0], others[-1]
                mid = others[len(others) // 2]
                # equal maxima at two indices (the second in another lane, or another trip of the same lane)
                u = 0
                sums[u, a] = sums[u, b] = sums[u].max() + 3.0
                if U > 1:          # two sums one ulp apart with equal quotients, the larger at the higher index
                    sums[1] = 2 * x
                    sums[1, a], sums[1, b], n[1] = x, y, n_ulp
                if U > 2:          # the background column holds the largest sum
                    sums[2, bg] = sums[2].max() + 50.0
                if U > 3:          # integers over a power of two: margin exactly 2.0
                    n[3] = 64
                    sums[3] = -64.0 * 9
                    sums[3, mid], sums[3, bg] = -64.0 * 3, -64.0 * 5
                if U > 4:
                    n[4] = 0       # no frames
                if U > 7:          # NaN sums, as the reference's max(enumerate(...)) takes them
                    sums[5, a] = np.nan          # in the first column besides bg: never replaced, accepted with margin NaN
                    sums[6, b] = np.nan          # elsewhere: never wins
                    sums[6, mid] = np.nan
                    sums[7] = np.nan             # everywhere
                    sums[8, bg] = np.nan         # in the background column: margin NaN, the best column accepted
            free = oc.rule(sums, n, bg, -np.inf)[1]
            mid_thr = float(np.nanmedian(free)) if np.any(~np.isnan(free)) else 0.0
            for thr in (2.0, np.nextafter(2.0, np.inf), -1e9, mid_thr):
                want = oc.rule(sums, n, bg, thr)
                got = open_set_decide(sums, n, bg, thr)
                assert same(got, want), (S, U, bg, thr, got, want)
            if len(others) >= 2:
                lab, mar = open_set_decide(sums, n, bg, -1e9)
                assert lab[0] == a                                               # equal maxima: the lowest index
                if U > 1:
                    assert lab[1] == a and mar[1] == x / np.float64(n_ulp) - 2 * x / np.float64(n_ulp)
                if U > 3:
                    assert mar[3] == 2.0 and open_set_decide(sums, n, bg, 2.0)[0][3] == mid                      # equal: accepted
                    assert open_set_decide(sums, n, bg, np.nextafter(2.0, np.inf))[0][3] == -1                   # just below
                if U > 4:
                    assert lab[4] == -1 and np.isnan(mar[4])
                if U > 7:
                    hi = open_set_decide(sums, n, bg, 1e9)                       # `NaN < threshold` is false at any threshold
                    for got_nan in ((lab, mar), hi):
                        assert got_nan[0][5] == a and np.isnan(got_nan[1][5])
                        assert got_nan[0][7] == a and np.isnan(got_nan[1][7])
                        assert got_nan[0][8] >= 0 and got_nan[0][8] != bg and np.isnan(got_nan[1][8])
                    assert lab[6] not in (-1, bg) and (lab[6] != b or a == b) and not np.isnan(mar[6])
            elif not others:
                lab, mar = open_set_decide(sums, n, bg, -1e9)
                assert np.all(lab == -1) and np.all(np.isnan(mar))               # S == 1: nobody besides the background


def test_bad_arguments_fail_with_a_message(built_lib):
    from speaker_recognition_amd import _lib, synth
    from speaker_recognition_amd.core import Batch, MfccExtractor, ModelSet, ServingStream, open_set_decide
    from speaker_recognition_amd.pygmm import GMM
    sums, n = np.zeros((2, 3)), np.array([5, 5])
    for bg, thr, pat in ((-1, 0.0, "outside"), (3, 0.0, "outside"), (0, np.nan, "NaN")):
        with pytest.raises(_lib.SRError, match=pat):
            open_set_decide(sums, n, bg, thr)
    ms = ModelSet([GMM.from_arrays(*synth.synth_gmm(8, 13, s)) for s in range(3)])
    feats = Batch.from_features([np.zeros((5, 13), np.float32)])
    with pytest.raises(_lib.SRError, match="outside"):
        ms.score_open(feats, 3, 0.0)
    with pytest.raises(_lib.SRError, match="NaN"):
        ms.score_open(feats, 0, np.nan)
    L = _lib.lib()
    out = np.zeros(1)
    assert L.sr_score_batch_set_open(ms._h, feats._h, 0, 0.0, _lib.as_dp(out), None, None, 0) == -1 and "null output" in _lib.last_error()
    ex = MfccExtractor(FS)
    st = ServingStream(ex, ms, 1, WIN)
    with pytest.raises(_lib.SRError, match="no open-set decision"):
        st.collect_open()
    st.submit(np.zeros(WIN, np.int16))
    st.collect()
    assert L.sr_stream_set_open(st._h, 0, 0.0) == -1 and "before the first submit" in _lib.last_error()      # the threshold is fixed


def test_refusals_on_live_handles(built_lib):
    """a live stream or predictor refuses a bad rule, and a full-covariance one any rule, with a message; it stays usable"""
    from speaker_recognition_amd import _lib, skgmm, synth
    from speaker_recognition_amd.core import MfccExtractor, MultiPredictor, ServingStream
    ex = MfccExtractor(FS)
    gmms, ms = small_set()
    S = len(gmms)
    L = _lib.lib()
    st = ServingStream(ex, ms, 1, WIN)
    for bg, thr, pat in ((-1, 0.0, "outside"), (S, 0.0, "outside"), (0, float("nan"), "NaN")):
        assert L.sr_stream_set_open(st._h, bg, thr) == -1 and pat in _lib.last_error(), (bg, thr, _lib.last_error())
        with pytest.raises(_lib.SRError, match=pat):
            ServingStream(ex, ms, 1, WIN, open_set=(bg, thr))
    assert L.sr_stream_set_open(st._h, S - 1, 0.5) == 0                           # the refused calls left the session as it was
    pcm = synth.synth_speech(1, 1.0, FS)[:WIN]
    st.submit(pcm)
    sums, lab, mar, _ = st.collect_open()
    assert same((lab, mar), oc.rule(sums, [ex.num_frames(WIN)], S - 1, 0.5))
    mp = MultiPredictor(gmms, FS, n_slots=2)
    for bg, thr, pat in ((-1, 0.0, "outside"), (S, 0.0, "outside"), (0, float("nan"), "NaN")):
        with pytest.raises(_lib.SRError, match=pat):
            mp.predict_open([pcm], bg, thr)
    out = np.zeros(S)
    cat = np.ascontiguousarray(pcm, dtype=np.int16)
    off = np.array([0, len(cat)], dtype=np.int64)
    assert L.sr_multi_predict_pcm_open(mp._h, cat.ctypes.data_as(C.POINTER(C.c_int16)), _lib.as_i64p(off), 1, 0, 0, 0.0, _lib.as_dp(out),
                                       None, None, None, 0) == -1 and "null output" in _lib.last_error()
    m_sums, m_lab, m_mar = mp.predict_open([pcm], S - 1, 0.5)                     # and the predictor still serves
    assert same((m_lab, m_mar), oc.rule(m_sums, [ex.num_frames(WIN)], S - 1, 0.5)) and np.array_equal(m_lab, lab)
    # full-covariance sets have no UBM column: any rule is refused
    rng = np.random.default_rng(3)
    full = [skgmm.GMM.from_arrays(np.full(2, 0.5), rng.standard_normal((2, 13)), np.repeat(np.eye(13)[None], 2, axis=0)) for _ in range(2)]
    fst = ServingStream(ex, skgmm.FullSet(full), 1, WIN)
    assert L.sr_stream_set_open(fst._h, 0, 0.0) == -1 and "full-covariance session" in _lib.last_error()
    with pytest.raises(_lib.SRError, match="full-covariance session"):
        ServingStream(ex, skgmm.FullSet(full), 1, WIN, open_set=(0, 0.0))
    fst.submit(pcm)
    assert fst.collect()[0].shape == (1, 2)
    with pytest.raises(_lib.SRError, match="full-covariance predictor"):
        MultiPredictor.from_full(full, FS, n_slots=1, n_lpc=0).predict_open([pcm], 0, 0.0)


# ---------------------------------------------------------------- 2. the features path

_ORACLE = {}


def features_reference(go, name):
    """models, utterances, the oracle's sums and the threshold they give -- computed once per case, read-only afterwards"""
    if name not in _ORACLE:
        models, utts = oc.features_case(getattr(oc, name))
        n = np.array([len(u) for u in utts])
        want = oc.oracle_sums(go, models, utts)
        thr, gap, per_frame = oc.threshold_from(want, n)
        want.setflags(write=False)
        _ORACLE[name] = (models, utts, n, want, thr, gap, per_frame)
    return _ORACLE[name]


@pytest.mark.parametrize("name", ["SMALL", "HEADLINE"])
def test_features_path_against_the_oracle_and_the_loop(built_lib, oracle_built, name):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch, ModelSet
    from speaker_recognition_amd.gmmset import GMMSet
    from speaker_recognition_amd.pygmm import GMM
    models, utts, n, want, thr, gap, per_frame = features_reference(oracle_built, name)
    assert gap > 100 * per_frame, (gap, per_frame)                               # every decision is unambiguous
    want_lab, want_mar = oc.rule(want, n, 0, thr)
    assert (want_lab >= 0).any() and (want_lab < 0).any()
    gmms = [GMM.from_arrays(*m) for m in models]
    ms = ModelSet(gmms)
    try:
        for eng in (0, 1, 3, 5):
            _lib.set_option("score_engine", eng)
            sums, lab, mar = ms.score_open(Batch.from_features(utts), 0, thr)
            print(name, "engine", eng, _lib.last_score_kernel()[:40], "sums worst ratio %.3g" % ll_close(sums, want), "margins",
                  np.round(mar, 3).tolist())
            assert same((lab, mar), oc.rule(sums, n, 0, thr)), eng               # the rule on the call's own sums, bit for bit
            assert ll_close(sums, want) < oc.GATE, (eng, ll_close(sums, want))
            assert np.array_equal(lab, want_lab), (eng, lab, want_lab)           # every utterance, the oracle's decision
        _lib.set_option("score_engine", 0)
        gs = GMMSet(ubm=gmms[0], reject_threshold=thr)
        for i, g in enumerate(gmms[1:]):
            gs._append("spk%d" % i, g)
        loop = gs.predict_with_reject([u.astype(np.float64) for u in utts])
        batch = gs.predict_with_reject_batch(utts)
        want_names = [None if w < 0 else "spk%d" % (w - 1) for w in want_lab]
        assert loop == want_names and batch == want_names
        assert gs._open_set is gs._open_model_set()                              # packed once, kept
        assert gs.predict_with_reject_batch(utts, threshold=np.inf) == [None] * len(utts)
        assert gs.reject_threshold == thr                                        # a call's own threshold leaves the model's alone
        assert np.array_equal(gs.reject_margins(utts), ms.score_open(Batch.from_features(utts), 0, thr)[2])
    finally:
        _lib.set_option("score_engine", 0)


# ---------------------------------------------------------------- 3. the partial-product band

def test_decision_is_taken_behind_the_flush_patch(built_lib, flush_golden):
    from conftest import flush_models
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch, ModelSet
    from speaker_recognition_amd.pygmm import GMM
    g, c = flush_golden, "d39_ubm64"
    X = g[c + "_X"]
    ms = ModelSet([GMM.from_arrays(*m) for m in flush_models(g, c)])
    utts = [X[:50], X[50:51], X[51:]]
    n = np.array([len(u) for u in utts])
    try:
        for eng in (1, 0):
            for cap in (0, 1):                                                   # (1: the list overflows, the pass runs twice)
                _lib.set_option("score_engine", eng)
                _lib.set_option("flush_list_cap", cap)
                closed, _ = ms.score(Batch.from_features(utts))
                pairs0 = _lib.flush_stats()[1]
                probe = ms.score_open(Batch.from_features(utts), 0, -np.inf)[2]
                thr = float(np.sort(probe)[1])                                   # one utterance below, two at or above
                pairs1 = _lib.flush_stats()[1]
                sums, lab, mar = ms.score_open(Batch.from_features(utts), 0, thr)
                assert pairs1 > pairs0 and _lib.flush_stats()[1] > pairs1, (eng, cap)      # both calls went through gmm_flush.hip
                assert np.array_equal(sums, closed), (eng, cap)                  # the patched sums the closed-set call returns
                assert same((lab, mar), oc.rule(sums, n, 0, thr)), (eng, cap, lab, mar)
                assert (lab >= 0).any() and (lab < 0).any()
    finally:
        _lib.set_option("score_engine", 0)
        _lib.set_option("flush_list_cap", 0)


# ---------------------------------------------------------------- 4. from PCM

def small_set(S=5, K=32, seed=7):
    from speaker_recognition_amd import synth
    from speaker_recognition_amd.core import ModelSet
    from speaker_recognition_amd.pygmm import GMM
    ubm = synth.synth_gmm(K, 13, seed)
    raw = [ubm] + [synth.synth_map_speaker(ubm, seed + 100 + s) for s in range(S)]
    gmms = [GMM.from_arrays(*m) for m in raw]
    return gmms, ModelSet(gmms)


def test_from_pcm(built_lib):
    from speaker_recognition_amd import synth
    from speaker_recognition_amd.core import Batch, MfccExtractor
    ex = MfccExtractor(FS)
    _, ms = small_set()
    pcm = [synth.synth_speech(s, d, FS) for s, d in ((1, 1.0), (2, 0.37), (3, 2.1), (4, 0.1))]      # (the last: too short for a frame)
    n = np.array([ex.num_frames(len(p)) for p in pcm])
    assert n[-1] == 0 and np.all(n[:-1] > 0)
    b = Batch.from_pcm(pcm)
    probe = ex.predict_batch_open(ms, b, 0, -np.inf)[2]
    thr = float(np.sort(probe[:-1])[1])
    sums, lab, mar = ex.predict_batch_open(ms, b, 0, thr)
    assert same((lab, mar), oc.rule(sums, n, 0, thr))
    assert lab[-1] == -1 and np.isnan(mar[-1]) and (lab[:-1] >= 0).any() and (lab[:-1] < 0).any()
    feats = ex.extract_batch(b)
    assert np.array_equal(feats.offsets(), np.concatenate([[0], np.cumsum(n)]))
    sums2, lab2, mar2 = ms.score_open(feats, 0, thr)
    assert np.array_equal(lab2, lab)
    closed, arg = ex.predict_batch(ms, b)
    assert np.array_equal(closed, sums)                                          # the sibling's sums, the sibling untouched


# ---------------------------------------------------------------- 5. the serving stream

def stream_ticks(st, ticks, opened=True):
    out = []
    for t in ticks:
        st.submit(t)
        out.append(st.collect_open() if opened else st.collect())
    return out


@pytest.mark.parametrize("n_win", [2, 6])
def test_stream_plain_and_graph(built_lib, n_win):
    from speaker_recognition_amd import synth
    from speaker_recognition_amd.core import MfccExtractor, ServingStream
    ex = MfccExtractor(FS)
    _, ms = small_set()
    ticks = [np.stack([synth.synth_speech(3 * t + w, 1.0, FS) for w in range(n_win)]) for t in range(3)]
    n = np.full(n_win, ex.num_frames(WIN))
    closed = stream_ticks(ServingStream(ex, ms, n_win, WIN), ticks, opened=False)
    thr = float(np.median(np.concatenate([oc.rule(c[0], n, 0, -np.inf)[1] for c in closed])))
    plain = stream_ticks(ServingStream(ex, ms, n_win, WIN, open_set=(0, thr)), ticks)
    graph = stream_ticks(ServingStream(ex, ms, n_win, WIN, graph=True, open_set=(0, thr)), ticks)
    labels = np.concatenate([p[1] for p in plain])
    assert (labels >= 0).any() and (labels < 0).any()
    for t in range(3):
        sums, lab, mar, _ = plain[t]
        assert same((lab, mar), oc.rule(sums, n, 0, thr)), t
        assert np.array_equal(sums, closed[t][0])
        for a, b in zip(plain[t][:3], graph[t][:3]):                             # graph ticks equal plain ticks, bit for bit
            assert np.array_equal(a, b, equal_nan=True), t
    # sr_stream_collect on an open-set session still returns the closed-set argmax
    st = ServingStream(ex, ms, n_win, WIN, graph=True, open_set=(0, thr))
    for t in range(3):
        st.submit(ticks[t])
        sums, arg, _ = st.collect()
        assert np.array_equal(sums, closed[t][0]) and np.array_equal(arg, closed[t][1])


@pytest.mark.parametrize("graph", [False, True])
def test_stream_vad_session(built_lib, graph):
    from speaker_recognition_amd.core import MfccExtractor, ServingStream
    ex = MfccExtractor(FS)
    _, ms = small_set()
    windows, noise = oc.vad_scene()
    vad = oc.make_vad(noise)
    n_win = 6
    ticks = [windows[6 * t:6 * t + 6] for t in range(3)]
    closed = []
    st = ServingStream(ex, ms, n_win, WIN, graph=graph, vad=vad)
    for t in ticks:
        st.submit(t)
        closed.append(st.collect_vad())
    voiced = np.concatenate([c[2] for c in closed])
    frames = np.array([ex.num_frames(int(v)) if 3 * v > WIN else 0 for v in voiced])
    assert (frames > 0).sum() >= 3 and np.any(voiced == 0) | np.any((voiced > 0) & (frames == 0)), (voiced, frames)
    all_sums = np.concatenate([c[0] for c in closed])
    scored = frames > 0
    thr = float(np.median(oc.rule(all_sums[scored], frames[scored], 0, -np.inf)[1]))
    st = ServingStream(ex, ms, n_win, WIN, graph=graph, vad=vad, open_set=(0, thr))
    for t in range(3):
        st.submit(ticks[t])
        sums, lab, mar, _ = st.collect_open()
        fr = frames[6 * t:6 * t + 6]
        assert np.array_equal(st.last_voiced, closed[t][2])
        assert np.array_equal(sums, closed[t][0])
        assert same((lab, mar), oc.rule(sums, fr, 0, thr)), (t, lab, mar)
        assert np.all(lab[fr == 0] == -1) and np.all(np.isnan(mar[fr == 0]))     # not voiced, or under a third: nobody


# ---------------------------------------------------------------- 6. several slots

def test_multi_equals_the_fused_call(built_lib):
    from speaker_recognition_amd import _lib, synth
    from speaker_recognition_amd.core import Batch, MfccExtractor, MultiPredictor
    ex = MfccExtractor(FS)
    gmms, ms = small_set()
    pcm = [synth.synth_speech(s, 0.4 + 0.23 * s, FS) for s in range(7)] + [synth.synth_speech(9, 0.1, FS)]
    probe = ex.predict_batch_open(ms, Batch.from_pcm(pcm), 0, -np.inf)[2]
    thr = float(np.nanmedian(probe))
    want = ex.predict_batch_open(ms, Batch.from_pcm(pcm), 0, thr)
    assert (want[1] >= 0).any() and (want[1] < 0).any()
    try:
        for slots, merge in ((1, 1), (2, 1), (2, 0)):
            _lib.set_option("multi_merge_same_device", merge)
            got = MultiPredictor(gmms, FS, n_slots=slots).predict_open(pcm, 0, thr)
            for a, b in zip(got, want):
                assert np.array_equal(a, b, equal_nan=True), (slots, merge)
    finally:
        _lib.set_option("multi_merge_same_device", 1)


# ---------------------------------------------------------------- 7. the partial-product band on the stream and multi paths
# A tick or a piece with pairs in the band is first decided on sums WITHOUT the noted pairs (the decision kernel behind finalize);
# collect / the slot's gather score it again and must hand out the decision taken behind gmm_flush.hip's patch.  Every case
# checks that pairs went through gmm_flush.hip, and that labels and margins are the rule's on the returned (patched) sums, bit
# for bit -- a pre-patch margin differs from it by the band frames' log-likelihoods, some -650 each.

def band_set():
    from speaker_recognition_amd.core import ModelSet
    from speaker_recognition_amd.pygmm import GMM
    gmms = [GMM.from_arrays(*m) for m in oc.band_models()]
    return gmms, ModelSet(gmms)


@pytest.mark.parametrize("graph,delay,cap", [(False, 0, 0), (False, 0, 1), (True, 0, 0), (True, 20, 0)])
def test_band_frames_through_the_open_set_stream(built_lib, graph, delay, cap):
    """(delay: the host held back in front of the capture until the plain pass before it has finished -- the order in which the
    tick's band flag was once lost, csrc/stream.cpp; cap 1: the band list overflows and the pass runs twice)"""
    from speaker_recognition_amd import _lib, synth
    from speaker_recognition_amd.core import MfccExtractor, ServingStream
    ex = MfccExtractor(FS)
    _, ms = band_set()
    n_win = 4
    ticks = [np.stack([synth.synth_speech(3 + 4 * t + w, 1.0, FS)[:WIN] for w in range(n_win)]) for t in range(2)]
    n = np.full(n_win, ex.num_frames(WIN))
    pairs0 = _lib.flush_stats()[1]
    closed = stream_ticks(ServingStream(ex, ms, n_win, WIN), ticks, opened=False)
    pairs1 = _lib.flush_stats()[1]
    assert pairs1 > pairs0                                                       # the scene has frames in the band
    thr = float(np.median(np.concatenate([oc.rule(c[0], n, 0, -np.inf)[1] for c in closed])))
    _lib.set_option("flush_list_cap", cap)
    _lib.set_option("debug_capture_delay_ms", delay)
    try:
        st = ServingStream(ex, ms, n_win, WIN, graph=graph, open_set=(0, thr))
        labels = []
        for rnd in range(2):                                                     # (graph: the capturing ticks, then the replayed ones)
            for t in ticks:
                st.submit(t)
            for t in range(2):
                before = _lib.flush_stats()[1]
                sums, lab, mar, _ = st.collect_open()
                print("graph", graph, "delay", delay, "cap", cap, "round", rnd, "tick", t, "pairs", _lib.flush_stats()[1] - before,
                      "margins", np.round(mar, 3).tolist())
                assert _lib.flush_stats()[1] > before, (rnd, t)                  # this tick was patched at collect
                assert same((lab, mar), oc.rule(sums, n, 0, thr)), (rnd, t, lab, mar)
                assert ll_close(sums, closed[t][0]) < oc.GATE, (rnd, t)
                labels.append(lab)
        labels = np.concatenate(labels)
        assert (labels >= 0).any() and (labels < 0).any()
    finally:
        _lib.set_option("flush_list_cap", 0)
        _lib.set_option("debug_capture_delay_ms", 0)


@pytest.mark.parametrize("graph", [False, True])
def test_band_frames_through_an_open_set_vad_session(built_lib, graph):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import MfccExtractor, ServingStream
    ex = MfccExtractor(FS)
    _, ms = band_set()
    windows, noise = oc.vad_scene()
    vad = oc.make_vad(noise)
    n_win = 6
    ticks = [windows[6 * t:6 * t + 6] for t in range(3)]
    closed = []
    st = ServingStream(ex, ms, n_win, WIN, graph=graph, vad=vad)
    for t in ticks:
        st.submit(t)
        closed.append(st.collect_vad())
    voiced = np.concatenate([c[2] for c in closed])
    frames = np.array([ex.num_frames(int(v)) if 3 * v > WIN else 0 for v in voiced])
    scored = frames > 0
    assert scored.sum() >= 3
    thr = float(np.median(oc.rule(np.concatenate([c[0] for c in closed])[scored], frames[scored], 0, -np.inf)[1]))
    st = ServingStream(ex, ms, n_win, WIN, graph=graph, vad=vad, open_set=(0, thr))
    labels, patched = [], 0
    for t in range(3):
        before = _lib.flush_stats()[1]
        st.submit(ticks[t])
        sums, lab, mar, _ = st.collect_open()
        fr = frames[6 * t:6 * t + 6]
        grew = _lib.flush_stats()[1] - before
        print("graph", graph, "tick", t, "pairs", grew, "frames", fr.tolist(), "margins", np.round(mar, 3).tolist())
        patched += grew > 0
        assert np.array_equal(st.last_voiced, closed[t][2])
        assert same((lab, mar), oc.rule(sums, fr, 0, thr)), (t, lab, mar)
        assert ll_close(sums, closed[t][0]) < oc.GATE, t
        labels.append(lab[fr > 0])
    labels = np.concatenate(labels)
    assert patched >= 2                                                          # ticks decided again behind the patch
    assert (labels >= 0).any() and (labels < 0).any()


def test_band_frames_through_multi_predict_open(built_lib):
    from speaker_recognition_amd import _lib, synth
    from speaker_recognition_amd.core import Batch, MfccExtractor, MultiPredictor
    ex = MfccExtractor(FS)
    gmms, ms = band_set()
    pcm = [synth.synth_speech(3 + s, 0.6 + 0.2 * s, FS) for s in range(6)]
    n = np.array([ex.num_frames(len(p)) for p in pcm])
    pairs0 = _lib.flush_stats()[1]
    probe = ex.predict_batch_open(ms, Batch.from_pcm(pcm), 0, -np.inf)[2]
    assert _lib.flush_stats()[1] > pairs0                                        # the utterances have frames in the band
    thr = float(np.median(probe))
    want = ex.predict_batch_open(ms, Batch.from_pcm(pcm), 0, thr)
    assert same(want[1:], oc.rule(want[0], n, 0, thr)) and (want[1] >= 0).any() and (want[1] < 0).any()
    try:
        for slots, merge, cap in ((1, 1, 0), (2, 1, 0), (2, 0, 0), (2, 0, 1)):
            _lib.set_option("multi_merge_same_device", merge)
            _lib.set_option("flush_list_cap", cap)
            before = _lib.flush_stats()[1]
            sums, lab, mar = MultiPredictor(gmms, FS, n_slots=slots).predict_open(pcm, 0, thr)
            assert _lib.flush_stats()[1] > before, (slots, merge, cap)
            assert same((lab, mar), oc.rule(sums, n, 0, thr)), (slots, merge, cap, lab, mar)
            for a, b in zip((sums, lab, mar), want):                             # and the single-device fused call's, bit for bit
                assert np.array_equal(a, b, equal_nan=True), (slots, merge, cap)
    finally:
        _lib.set_option("multi_merge_same_device", 1)
        _lib.set_option("flush_list_cap", 0)
