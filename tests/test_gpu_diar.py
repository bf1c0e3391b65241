"""GPU: the diarisation of unknown speakers (csrc/diar.hip: sr_diar_stats_batch, sr_diar_bic_matrix, sr_diar_cluster_batch,
sr_diar_cluster_pcm_batch, sr_ahc_matrix, Batch.diarize, ModelInterface.diarize) against the numpy restatement of its definitions
(tests/diar_oracle.py).

Three kinds of gate.  The statistics and the matrix mode are equal to the oracle to the bit: the same float64 operations in the same
order.  A delta-BIC goes through a Cholesky factorisation the oracle takes from LAPACK, so it is held to Cholesky's backward-error
bound carried through the log-determinant, 8 (N_a + N_b) D^2 eps kappa.  A merge sequence (and a set of kept boundaries) is a chain
of comparisons of such values: it must equal the oracle's whenever every comparison the oracle made was decided by more than four
of those bounds -- which every case asserts of the oracle first; the seeds below were chosen so that it holds."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diar_oracle as do  # noqa: E402

pytestmark = pytest.mark.gpu

INIT_COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 256, 257)      # {1, 2, 3, 63, 64, 65, 257} and both sides of every edge of _lib.diar_plan
CLUSTER_SEEDS = {13: 1300, 39: 3900}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def planted(seed, D, turns, L, n_speakers=3):
    """Frames of a recording whose turn t (turns[t] base segments of L frames) is drawn from speaker t mod n_speakers: Gaussians of
    different means and scales."""
    rng = np.random.default_rng(seed)
    means = rng.normal(0.0, 1.5, (n_speakers, D))
    scales = rng.uniform(0.7, 1.4, (n_speakers, D))
    parts = [means[t % n_speakers] + scales[t % n_speakers] * rng.normal(0.0, 1.0, (k * L, D)) for t, k in enumerate(turns)]
    return np.concatenate(parts).astype(np.float32) if parts else np.zeros((0, D), np.float32)


def seg_len(D):
    return max(3 * D, 40)


@functools.lru_cache(maxsize=None)
def uniform_case(count, D):
    """`count` initial clusters (uniform mode) of three planted speakers in turns of one to three segments, the stop rule and the
    oracle's run.  At 13 dimensions every count runs under the default rule down to the speakers.  At 39 the two largest counts take
    48 forced steps instead: the oracle's eigenvalues of every pair of every step are what such a case costs on the host (8 s for
    the whole run), and the wrap of the argmin kernel's lanes is in the first steps."""
    rng = np.random.default_rng(CLUSTER_SEEDS[D] + count)
    turns, left = [], count
    while left > 0:
        k = int(min(left, rng.integers(1, 4)))
        turns.append(k)
        left -= k
    L = seg_len(D)
    X = planted(CLUSTER_SEEDS[D] + 7 * count, D, turns, L)
    kw = dict(threshold=float("-inf"), k_max=count - 48) if count >= 256 and D == 39 else dict()
    want = do.cluster(X, L, change="uniform", **kw)
    return X, L, want, kw


def assert_log_equals(res, want):
    """The steps, labels and runs are the oracle's; every merged distance lies within that pair's own bound."""
    assert res["labels"].tolist() == want["labels"].tolist()
    assert res["merge_i"].tolist() == want["merge_i"].tolist() and res["merge_j"].tolist() == want["merge_j"].tolist()
    assert res["n_clusters"] == want["n_clusters"] and res["failed"] == want["failed"]
    for t, (got, ref) in enumerate(zip(res["merge_d"], want["merge_d"])):
        assert abs(got - ref) <= want["steps"][t][3], (t, got, ref, want["steps"][t])
    assert res["init_off"].tolist() == want["init_off"].tolist()


# ---- statistics: bit-equal ----

@pytest.mark.parametrize("D", (1, 2, 13, 39, 63, 64))
def test_segment_statistics_equal_the_oracle_to_the_bit(built_lib, D):
    from speaker_recognition_amd.core import Batch
    rng = np.random.default_rng(40 + D)
    for L in sorted({1, D, D + 1, 100}):
        lengths = [0, 1, L - 1, L, L + 1, 2 * L + L // 2]
        mats = [(rng.normal(0.0, 3.0, (n, D)) * rng.choice([1.0, 1e3], (n, 1))).astype(np.float32) for n in lengths]     # a ragged batch
        seg_off, stats = Batch.from_features(mats).segment_stats(L)
        assert np.diff(seg_off).tolist() == [do.segments(n, L) for n in lengths]
        for u, x in enumerate(mats):
            want = do.seg_stats(x, L)
            assert np.array_equal(bits(stats[seg_off[u]:seg_off[u + 1]]), bits(want)), (D, L, lengths[u])
        _, alone = Batch.from_features([mats[-1]]).segment_stats(L)                      # the same bits alone and batched
        assert np.array_equal(bits(alone), bits(stats[seg_off[-2]:]))


# ---- delta-BIC of given statistics: Cholesky's bound ----

@pytest.mark.parametrize("D", (1, 13, 39, 64))
def test_bic_matrix_within_the_cholesky_bound(built_lib, D):
    from speaker_recognition_amd import _lib
    rng = np.random.default_rng(90 + D)
    ridge = 0.5                                                          # keeps a cluster of 10 frames in 64 dimensions conditioned
    sizes = [10, 17, 40, 64, 65, 130, 257, 400]
    stats = np.array([do.stats_of((rng.normal(0.0, 0.3, D) + rng.normal(0.0, 1.0, (n, D))).astype(np.float32)) for n in sizes])
    want, bnd, ld, failed = do.bic_matrix(stats, D, 1.0, ridge)
    N = stats[:, 0][:, None] + stats[:, 0][None, :]
    off = ~np.eye(8, dtype=bool)
    kappa = bnd[off] / (8.0 * N[off] * D * D * do.EPS)
    assert failed == 0 and kappa.max() <= 100.0, kappa.max()            # the inputs are as conditioned as the bound supposes
    got, gld, gfailed = _lib.diar_bic_matrix(stats, D, 1.0, ridge)
    assert gfailed == 0 and np.array_equal(got, got.T) and (np.diag(got) == 0).all()
    err = np.abs(got - want)
    print("D=%d max err %.3g, smallest bound %.3g, max err / bound %.3g" % (D, err[off].max(), bnd[off].min(), (err[off] / bnd[off]).max()))
    assert (err[off] <= bnd[off]).all()
    assert np.abs(gld - ld).max() <= bnd[off].max()


def test_bic_matrix_rank_deficient_cluster_is_inf_and_counted(built_lib):
    from speaker_recognition_amd import _lib
    rng = np.random.default_rng(17)
    D = 13
    stats = np.array([do.stats_of(rng.normal(0.0, 1.0, (n, D)).astype(np.float32)) for n in (60, 1, 90)])    # N = 1 <= D, ridge 0
    got, ld, failed = _lib.diar_bic_matrix(stats, D, 1.0, 0.0)
    want, bnd, wld, wfailed = do.bic_matrix(stats, D, 1.0, 0.0)
    assert failed == wfailed == 1 and np.isnan(ld[1]) and not np.isnan(ld[[0, 2]]).any()
    assert np.isposinf(got[1, [0, 2]]).all() and np.isposinf(got[[0, 2], 1]).all()
    assert np.isfinite(got[0, 2]) and abs(got[0, 2] - want[0, 2]) <= bnd[0, 2]
    one, ld1, f1 = _lib.diar_bic_matrix(stats[:1], D)
    assert one.tolist() == [[0.0]] and f1 == 0
    assert _lib.diar_bic_matrix(np.zeros((0, do.stat_len(D))), D)[0].shape == (0, 0)


# ---- clustering on features ----

@pytest.mark.parametrize("D", (13, 39))
@pytest.mark.parametrize("count", INIT_COUNTS)
def test_clustering_takes_the_oracles_steps(built_lib, count, D):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    edges = _lib.diar_plan(D)["edges"]
    assert all(e in INIT_COUNTS and e + 1 in INIT_COUNTS for e in edges)
    X, L, want, kw = uniform_case(count, D)
    assert want["n_seg"] == count and do.fair(want["steps"], kw.get("threshold", 0.0))       # every decision of the oracle is clear of four bounds
    res = Batch.from_features([X]).diarize(L=L, change="uniform", **kw)[0]
    assert_log_equals(res, want)
    assert len(res["merge_d"]) == len(want["merge_d"]) == (48 if kw else max(0, count - want["n_clusters"])) and res["n_seg"] == count


def test_k_min_and_k_max_and_all_inf(built_lib):
    from speaker_recognition_amd.core import Batch
    X, L, _, _ = uniform_case(65, 13)
    feats = Batch.from_features([X])
    for kw in (dict(k_max=2), dict(k_min=7), dict(threshold=float("inf")), dict(threshold=float("inf"), k_min=3, k_max=3),
               dict(threshold=-50.0), dict(threshold=float("-inf")), dict(threshold=float("-inf"), k_max=64)):
        want = do.cluster(X, L, change="uniform", **kw)
        assert do.fair(want["steps"], kw.get("threshold", 0.0)), kw
        res = feats.diarize(L=L, change="uniform", **kw)[0]
        assert_log_equals(res, want)
    assert feats.diarize(L=L, change="uniform", k_max=2)[0]["n_clusters"] == 2           # merges forced past the threshold
    assert feats.diarize(L=L, change="uniform", k_min=7)[0]["n_clusters"] == 7           # stopped before it
    # every distance +inf: segments of one frame without a ridge have no covariance; k_max cannot force a step
    lone = Batch.from_features([X[:9]]).diarize(L=1, change="uniform", ridge=0.0, k_max=1)[0]
    assert lone["n_clusters"] == 9 and lone["failed"] == 9 and len(lone["merge_d"]) == 0 and lone["labels"].tolist() == list(range(9))
    empty = Batch.from_features([X[:0], X[:5]]).diarize(L=L)
    assert empty[0]["n_clusters"] == 0 and empty[0]["labels"].tolist() == [] and empty[0]["init_off"].tolist() == [0]
    assert empty[1]["n_clusters"] == 1 and empty[1]["init_off"].tolist() == [0, 1] and empty[1]["n_seg"] == 1


# ---- change detection ----

@pytest.mark.parametrize("m", (1, 2, 5))
def test_change_detection_keeps_the_oracles_boundaries(built_lib, m):
    from speaker_recognition_amd.core import Batch
    D, L = 13, 150
    turns = [1, 6, 4, 7, 5, 1]                                           # a boundary behind the first and before the last segment
    X = planted(500 + m, D, turns, L)
    want = do.cluster(X, L, change="bic", m=m, threshold=float("-inf"))
    c, cb = want["change"], want["change_bound"]
    for b in range(len(c)):                                              # every comparison of the peak rule is clear of four bounds
        assert abs(c[b]) > 4 * cb[b]
        for k in range(max(0, b - (m - 1)), min(len(c) - 1, b + (m - 1)) + 1):
            assert k == b or abs(c[b] - c[k]) > 4 * max(cb[b], cb[k])
    kept = np.flatnonzero(want["kept"]) + 1
    assert 1 in kept and len(c) in kept and len(kept) >= 4
    res = Batch.from_features([X]).diarize(L=L, change="bic", half_width=m, threshold=float("-inf"))[0]
    assert res["init_off"].tolist() == want["init_off"].tolist() and res["n_clusters"] == len(kept) + 1
    full = do.cluster(X, L, change="bic", m=m)                           # and the clustering of those runs
    assert do.fair(full["steps"], 0.0)
    assert_log_equals(Batch.from_features([X]).diarize(L=L, change="bic", half_width=m)[0], full)


# ---- matrix mode: bit-equal ----

@pytest.mark.parametrize("linkage", (0, 1, 2))
@pytest.mark.parametrize("n", (1, 2, 3, 64, 65, 257))
def test_matrix_mode_equals_the_oracle_to_the_bit(built_lib, n, linkage):
    from speaker_recognition_amd import _lib
    rng = np.random.default_rng(1000 + 10 * n + linkage)
    small = rng.integers(1, 5, (n, n)).astype(np.float64)                # ties at every step: the tie order
    large = rng.uniform(1e6, 2e6, (n, n))                                # every operation rounds
    for d0, thresholds in ((small, (float("inf"), 2.5)), (large, (float("inf"), 1.2e6))):
        d0 = np.triu(d0, 1) + np.triu(d0, 1).T
        for thr in thresholds:
            for kw in (dict(), dict(k_min=2, k_max=max(2, n // 3))):
                want = do.ahc(d0, linkage, threshold=thr, **kw)
                lab, mi, mj, md = _lib.ahc_matrix(d0, linkage, thr, **kw)
                assert mi.tolist() == want["merge_i"].tolist() and mj.tolist() == want["merge_j"].tolist()
                assert np.array_equal(bits(md), bits(want["merge_d"])) and lab.tolist() == want["labels"].tolist()
    if n == 3:
        inf = float("inf")
        d0 = np.array([[0, inf, 1.0], [inf, 0, inf], [1.0, inf, 0]])
        lab, mi, mj, md = _lib.ahc_matrix(d0, linkage, inf, k_max=1)     # (0, 2) merges; what is left is +inf in every linkage
        assert (mi.tolist(), mj.tolist(), lab.tolist()) == ([0], [2], [0, 1, 0])


def test_python_ahc_and_cut(built_lib):
    from speaker_recognition_amd import diarize as dz
    rng = np.random.default_rng(77)
    pts = np.concatenate([rng.normal(c, 0.1, (6, 2)) for c in ((0, 0), (5, 5), (0, 5))])
    d0 = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    d0 = (d0 + d0.T) / 2
    for linkage in ("average", "complete", "single"):
        lab, log = dz.ahc(d0, linkage=linkage, threshold=1.0)
        assert lab.tolist() == [0] * 6 + [1] * 6 + [2] * 6 and len(log[2]) == 15
        whole_lab, whole = dz.ahc(d0, linkage=linkage, threshold=float("inf"))
        assert set(whole_lab.tolist()) == {0} and len(whole[2]) == 17
        assert dz.cut(whole, 18, threshold=1.0).tolist() == lab.tolist() and dz.cut(whole, 18, k=3).tolist() == lab.tolist()
        assert dz.ahc(d0, linkage=linkage, k=2)[0].max() == 1 and dz.ahc(d0, linkage=linkage, threshold=1.0, k_max=2)[0].max() == 1


# ---- determinism ----

def test_same_bits_alone_batched_and_in_groups(built_lib):
    from speaker_recognition_amd import _lib, diarize as dz
    from speaker_recognition_amd.core import Batch
    D, L = 13, 40
    recs = [planted(900 + u, D, turns, L) for u, turns in enumerate(([30, 40, 30, 40, 30, 30], [3, 2], [100, 50, 50], [1], [90, 110]))]
    recs.insert(2, np.zeros((0, D), np.float32))
    kw = dict(L=L, change="uniform")

    def run(mats):
        return Batch.from_features(mats).diarize(**kw)

    def same(a, b):
        assert a["labels"].tolist() == b["labels"].tolist() and a["init_off"].tolist() == b["init_off"].tolist()
        assert a["merge_i"].tolist() == b["merge_i"].tolist() and a["merge_j"].tolist() == b["merge_j"].tolist()
        assert np.array_equal(bits(a["merge_d"]), bits(b["merge_d"])) and (a["n_clusters"], a["failed"]) == (b["n_clusters"], b["failed"])

    whole = run(recs)
    assert len(whole[0]["merge_d"]) > 0 and whole[0]["n_clusters"] < 200
    for a, b in zip(whole, run(recs)):                                   # run to run
        same(a, b)
    for u, x in enumerate(recs):                                         # alone
        same(whole[u], run([x])[0])
    plan = _lib.diar_plan(D, [len(x) for x in recs], L=L, change="uniform", scratch_bytes=1 << 20)
    assert plan["groups"] >= 3 and max(plan["rec_bytes"]) <= 1 << 20     # the smallest bound cuts this batch
    _lib.set_option("diar_scratch_mib", 1)
    try:
        for a, b in zip(whole, run(recs)):
            same(a, b)
        seg_off, stats = Batch.from_features(recs).segment_stats(L)
    finally:
        _lib.set_option("diar_scratch_mib", 1024)
    seg_off2, stats2 = Batch.from_features(recs).segment_stats(L)
    assert seg_off.tolist() == seg_off2.tolist() and np.array_equal(bits(stats), bits(stats2))
    # the same three comparisons with the change detector in front
    kw = dict(L=L, change="bic", half_width=5)
    whole = run(recs)
    assert len(whole[0]["labels"]) > 1 and len(whole[0]["merge_d"]) > 0
    for a, b in zip(whole, run(recs)):
        same(a, b)
    for u, x in enumerate(recs):
        same(whole[u], run([x])[0])
    _lib.set_option("diar_scratch_mib", 1)
    try:
        for a, b in zip(whole, run(recs)):
            same(a, b)
    finally:
        _lib.set_option("diar_scratch_mib", 1024)
    # the two calls on host data, run to run
    first = _lib.diar_bic_matrix(stats[:40], D, 1.0, 1e-3)
    again = _lib.diar_bic_matrix(stats[:40], D, 1.0, 1e-3)
    assert np.array_equal(bits(first[0]), bits(again[0])) and np.array_equal(bits(first[1]), bits(again[1])) and first[2] == again[2] == 0
    d0 = first[0] - first[0].min()
    for linkage in (0, 1, 2):
        one, two = _lib.ahc_matrix(d0, linkage, float("inf")), _lib.ahc_matrix(d0, linkage, float("inf"))
        assert len(one[3]) == 39 and all(np.array_equal(a, b) for a, b in zip(one[:3], two[:3])) and np.array_equal(bits(one[3]), bits(two[3]))
    kw = dict(L=L, change="uniform")
    whole = run(recs)
    lab, ranges, log = dz.cluster(recs[1], **kw)                         # the module's surface: one matrix in, one tuple out
    assert lab.tolist() == whole[1]["labels"].tolist() and ranges.tolist() == [[k * L, (k + 1) * L] for k in range(5)]
    assert np.array_equal(bits(log[2]), bits(whole[1]["merge_d"]))


def test_pcm_call_equals_extract_then_cluster(built_lib):
    from speaker_recognition_amd import synth
    from speaker_recognition_amd.core import Batch, MfccExtractor
    ex = MfccExtractor(16000, win_length_ms=25, win_shift_ms=10)
    pcm = Batch.from_pcm([np.concatenate([synth.synth_speech(s, 1.0) for s in voices]) for voices in ((0, 7), (3,), (5, 1, 5))])
    kw = dict(L=25, change="bic", half_width=2, penalty=1.0)
    want = ex.extract_batch(pcm, nd=0).diarize(**kw)
    got = ex.diarize_batch(pcm, nd=0, **kw)
    assert len(got) == 3
    for a, b in zip(got, want):
        assert a["labels"].tolist() == b["labels"].tolist() and a["init_off"].tolist() == b["init_off"].tolist()
        assert np.array_equal(bits(a["merge_d"]), bits(b["merge_d"])) and a["n_seg"] == b["n_seg"] > 0
    # the plan's refusals come from the frame counts, before the feature stage runs: 198 frames, a segment each, fit; 5000 do not
    from speaker_recognition_amd import _lib
    long_pcm = Batch.from_pcm([np.concatenate([synth.synth_speech(s, 10.0) for s in range(6)])])
    with pytest.raises(_lib.SRError, match="4096"):
        ex.diarize_batch(long_pcm, nd=0, L=1, change="uniform")
    _lib.set_option("diar_scratch_mib", 1)
    try:
        with pytest.raises(_lib.SRError, match="larger L"):
            ex.diarize_batch(long_pcm, nd=0, L=2, change="bic")
    finally:
        _lib.set_option("diar_scratch_mib", 1024)


# ---- the interface ----

def test_interface_diarize_on_three_voices(built_lib):
    from speaker_recognition_amd import diarize as dz, synth
    from speaker_recognition_amd.interface import ModelInterface
    voices = (0, 7, 3, 0, 3, 7)
    signal = np.concatenate([synth.synth_speech(s, 2.0) for s in voices])
    m = ModelInterface(verbose=False, lpc=False, gmm_kwargs=dict(seed=3))
    feat = np.asarray(m._features_of(16000, signal))
    n = len(feat)
    shift, L, _, _ = m._diarize_args(0.5, "bic", 1.0, None, None, 4)
    # the clustering is the oracle's on the features the device extracted
    want = do.cluster(feat.astype(np.float32), L, change="bic", m=2, k_max=3)
    c, cb = want["change"], want["change_bound"]
    clear = all(abs(c[b]) > 4 * cb[b] and all(k == b or abs(c[b] - c[k]) > 4 * max(cb[b], cb[k]) for k in (b - 1, b + 1) if 0 <= k < len(c))
                for b in range(len(c)))
    assert clear and do.fair(want["steps"], 0.0)
    from speaker_recognition_amd.core import Batch
    assert_log_equals(Batch.from_features([feat]).diarize(L=L, change="bic", k_max=3)[0], want)
    plain = m.diarize(16000, signal, segment_s=0.5, max_speakers=3, resegment=False)
    assert plain == [(a, b, "spk%d" % lab) for a, b, lab in dz.frame_segments(want["init_off"], want["labels"], n, L, shift)]
    assert 2 <= want["n_clusters"] <= 3

    def tiles(segs):
        assert segs[0][0] == 0.0 and abs(segs[-1][1] - n * shift) < 1e-9
        assert all(a[1] == b[0] and a[2] != b[2] for a, b in zip(segs, segs[1:])) and all(b > a for a, b, _ in segs)
        assert {name for _, _, name in segs} <= {"spk%d" % k for k in range(want["n_clusters"])}

    tiles(plain)
    # with resegment: the hand composition of the existing fit and timeline calls on the same clusters
    for covariance in ("diag", "full"):
        mi = ModelInterface(verbose=False, lpc=False, gmm_kwargs=dict(seed=3), covariance_type=covariance)
        tkw = dict(window_s=0.5, hop_s=0.25, switch_penalty=1.0, min_duration_s=0.5)
        segs = mi.diarize(16000, signal, segment_s=0.5, max_speakers=3, gmm_order=2, **tkw)
        tiles(segs)
        hand = ModelInterface(verbose=False, lpc=False, gmm_kwargs=dict(seed=3), covariance_type=covariance, gmm_order=2)
        ranges = dz.frame_ranges(want["init_off"], n, L)
        for k in range(want["n_clusters"]):
            hand.features["spk%d" % k] = list(np.concatenate([feat[a:b] for (a, b), lab in zip(ranges.tolist(), want["labels"]) if lab == k]))
        hand.train()
        assert segs == hand.timeline(16000, signal, smooth="viterbi", **tkw)
    one = m.diarize(16000, signal, segment_s=0.5, n_speakers=1)          # one cluster: the resegmentation is skipped
    assert one == [(0.0, n * shift, "spk0")]
