"""The pipelined shared-sigma kernel on its COMPACT image (csrc/score_shapes.hpp: h2c_map; score_engine 6, score_h2s_shape 3 at
D = 37 .. 39) against the float64 oracle, against the same kernel on the flat image (score_h2s_shape 5), where the form does not
apply (D = 40), and built on first use in either order of a small and a large batch.
Gates: per frame |dLL| <= 1e-4 * max(1, |LL|), utterance sums within 1e-5 relative, argmax equal.

Set sizes: 12 (a partial block), 16 (exactly one block of 15 + 1), 17 and 22 (a last block of 7: its phantom stages are skipped).
The engine refuses sets of fewer than 12 models (SHARED_MIN_MODELS), so 12 is the smallest partial block it can be given; a
2-model set is checked to be refused."""
import numpy as np
import pytest

from conftest import ll_close

pytestmark = pytest.mark.gpu
TOL = 1e-4
SUM_TOL = 1e-5
MARK = "pipelined in the wave>/compact"
LENS = [1, 31, 32, 33, 100, 8, 8, 8, 8, 385]          # packed tails (1, 31, 1, 4, 8 x 4, 1), 17 full tiles: more than one workgroup


@pytest.fixture(autouse=True)
def _reset_options(built_lib):
    from speaker_recognition_amd import _lib
    yield
    for k in ("score_engine", "score_h2s_force_exc", "score_h2s_shape"):
        _lib.set_option(k, 0)


_CASES = {}


def _case(go, D, K, S, lens=LENS, rogue=None):
    """models, utterances and the oracle's per-frame values of one set shape: computed once, shared, left unchanged"""
    key = (D, K, S, tuple(lens), rogue)
    if key not in _CASES:
        from speaker_recognition_amd import synth
        ubm = synth.synth_gmm(K, D, 1000 + 13 * D + K)
        models = [ubm] + [synth.synth_map_speaker(ubm, 7000 + s) for s in range(S - 1)]
        utts = [synth.draw_frames(models[1 + u % (S - 1)], n, 500 + u) for u, n in enumerate(lens)]
        if rogue is not None:
            utts[rogue] = utts[rogue].copy()
            utts[rogue][-2] += 60.0
        X = np.concatenate(utts).astype(np.float64)
        want = np.stack([go.score_batch(go.GMMParams(*m), X) for m in models])
        for a in utts:
            a.setflags(write=False)
        want.setflags(write=False)
        _CASES[key] = (models, utts, want)
    return _CASES[key]


def _check(out, want, lens, what):
    sums, arg, fll = out
    worst = ll_close(fll, want)
    off = np.concatenate([[0], np.cumsum(lens)])
    worst_sum = 0.0
    for u in range(len(lens)):
        w = want[:, off[u]:off[u + 1]].sum(axis=1)
        worst_sum = max(worst_sum, float(np.max(np.abs(sums[u] - w) / np.maximum(1.0, np.abs(w)))))
        assert arg[u] == int(np.argmax(w)), (what, u)
    print("%s: per frame %.3e, sums %.3e" % (what, worst, worst_sum))
    assert worst < TOL, (what, worst)
    assert worst_sum < SUM_TOL, (what, worst_sum)


def _set(models):
    from speaker_recognition_amd.core import ModelSet
    from speaker_recognition_amd.pygmm import GMM
    return ModelSet([GMM.from_arrays(*m) for m in models])


@pytest.mark.parametrize("K", [32, 50, 96])            # one mixture tile, a ragged last tile, three tiles
@pytest.mark.parametrize("D", [37, 38, 39])
def test_compact_against_oracle(built_lib, oracle_built, D, K):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    for S in (12, 16, 17, 22):
        models, utts, want = _case(oracle_built, D, K, S)
        ms = _set(models)
        _lib.set_option("score_engine", 6)
        _lib.set_option("score_h2s_shape", 3)
        for force in (0, 1):                           # ... and every tile through the exception pass (which reads the flat image)
            _lib.set_option("score_h2s_force_exc", force)
            out = ms.score(Batch.from_features(utts), frame_ll=True)
            name = _lib.last_score_kernel()
            assert "gmm_score_h2p_kernel<8,8,waves=12, pipelined in the wave>/compact" in name, name
            _check(out, want, LENS, "D=%d K=%d S=%d force_exc=%d" % (D, K, S, force))
        _lib.set_option("score_h2s_force_exc", 0)


def test_two_models_are_refused(built_lib):
    """why the smallest set above has 12 models: the shared-sigma engines take no fewer"""
    from speaker_recognition_amd import _lib, synth
    from speaker_recognition_amd.core import Batch
    ubm = synth.synth_gmm(32, 39, 5)
    ms = _set([ubm, synth.synth_map_speaker(ubm, 6)])
    _lib.set_option("score_engine", 6)
    with pytest.raises(Exception, match="does not qualify"):
        ms.score(Batch.from_features([synth.draw_frames(ubm, 40, 1)]))


@pytest.mark.parametrize("D", [37, 38, 39])
def test_rogue_frame_leaves_pack_mates_bits(built_lib, oracle_built, D):
    """One utterance of 8 frames with a frame at +60 on every dimension (the offset form refuses it: its tile's column goes to the
    exception pass): the utterances its tail is packed with keep their bits, and everything stays inside the gates."""
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    K, S, rogue = 50, 17, 6
    models, utts, want = _case(oracle_built, D, K, S)
    _, utts_r, want_r = _case(oracle_built, D, K, S, rogue=rogue)
    ms = _set(models)
    _lib.set_option("score_engine", 6)
    _lib.set_option("score_h2s_shape", 3)
    clean = ms.score(Batch.from_features(utts), frame_ll=True)
    dirty = ms.score(Batch.from_features(utts_r), frame_ll=True)
    assert MARK in _lib.last_score_kernel()
    _check(dirty, want_r, LENS, "D=%d rogue" % D)
    off = np.concatenate([[0], np.cumsum(LENS)])
    for u in range(len(LENS)):
        if u != rogue:
            assert np.array_equal(clean[0][u], dirty[0][u]) and clean[1][u] == dirty[1][u], u
            assert np.array_equal(clean[2][:, off[u]:off[u + 1]], dirty[2][:, off[u]:off[u + 1]]), u
    assert not np.array_equal(clean[0][rogue], dirty[0][rogue])


@pytest.mark.parametrize("D", [37, 38, 39])
def test_flat_image_against_compact(built_lib, oracle_built, D):
    """score_h2s_shape 5 (the same kernel on the flat image) against 3 on the same inputs: no marker, argmax equal, and the sums apart
    by no more than the two oracle gates allow (each within 1e-5 of the oracle's)."""
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    K, S = 96, 22
    models, utts, want = _case(oracle_built, D, K, S)
    ms = _set(models)
    _lib.set_option("score_engine", 6)
    out = {}
    for shape in (5, 3, 5):
        _lib.set_option("score_h2s_shape", shape)
        got = ms.score(Batch.from_features(utts), frame_ll=True)
        name = _lib.last_score_kernel()
        assert "pipelined in the wave>" in name and ("/compact" in name) == (shape == 3), name
        _check(got, want, LENS, "D=%d shape=%d" % (D, shape))
        if shape in out:
            assert all(np.array_equal(a, b) for a, b in zip(out[shape], got))       # the flat form's bits do not depend on what ran between
        out[shape] = got
    assert np.array_equal(out[3][1], out[5][1])
    off = np.concatenate([[0], np.cumsum(LENS)])
    w = np.stack([want[:, off[u]:off[u + 1]].sum(axis=1) for u in range(len(LENS))])
    rel = np.abs(out[3][0] - out[5][0]) / np.maximum(1.0, np.abs(w))
    print("D=%d: largest relative difference of a sum between the flat and the compact image %.3e" % (D, rel.max()))
    assert rel.max() <= 2 * SUM_TOL


def test_d40_keeps_the_flat_image(built_lib, oracle_built):
    """D = 40 runs the same <8,8> chains, but its parts are six half-steps: no compact form, no marker."""
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    models, utts, want = _case(oracle_built, 40, 50, 17)
    ms = _set(models)
    _lib.set_option("score_engine", 6)
    _lib.set_option("score_h2s_shape", 3)
    out = ms.score(Batch.from_features(utts), frame_ll=True)
    name = _lib.last_score_kernel()
    assert "gmm_score_h2p_kernel<8,8,waves=12, pipelined in the wave>" in name and "/compact" not in name, name
    _check(out, want, LENS, "D=40")


@pytest.mark.parametrize("small_first", [True, False])
def test_compact_image_is_built_on_first_use(built_lib, oracle_built, small_first):
    """A fresh set scored by a small batch (a 4-wave kernel: the flat image) and by a large one (the pipelined kernel: the compact
    image, made by that call), in either order, with the shape left to the dispatcher: both right."""
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    D, K, S = 39, 32, 16
    big_lens, small_lens = [9000, 40], [40]          # (two model blocks: the dispatcher goes wide above 256 tiles)
    models, big, want_big = _case(oracle_built, D, K, S, lens=big_lens)
    _, small, want_small = _case(oracle_built, D, K, S, lens=small_lens)
    ms = _set(models)
    _lib.set_option("score_engine", 6)
    for is_small in ((True, False) if small_first else (False, True)):
        out = ms.score(Batch.from_features(small if is_small else big), frame_ll=True)
        name = _lib.last_score_kernel()
        if is_small:
            assert "gmm_score_h2p_kernel" not in name and "gmm_score_h2" in name, name
            _check(out, want_small, small_lens, "small batch")
        else:
            assert MARK in name, name
            _check(out, want_big, big_lens, "large batch")
