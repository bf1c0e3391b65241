"""The compact pipelined shared-sigma kernel with its blocks taken in PAIRS behind one quadratic-half image (csrc/score_shapes.hpp:
h2q_*; score_engine 6, score_h2s_shape 3 at D = 37 .. 39) against the float64 oracle, against the same kernel block by block
(score_h2s_shape 6), under other group boundaries, and with a frame the offset form refuses.
Gates as tests/test_gpu_h2c.py: per frame |dLL| <= 1e-4 * max(1, |LL|), utterance sums within 1e-5 relative, argmax equal.

Set sizes (blocks of 15 models):
    16  15 + 1             a pair whose second block's stages are nearly all skipped
    30  15 + 15            the full 31-image pair: the last executed image an even one
    31  pair + lone 1
    37  15 + 15 + 7
    45  pair + full lone block
    52  15 + 15 + 15 + 7   the second pair short
K = 32 is one mixture tile (the last image's epilogue goes straight to the drain), K = 96 three (it rides the next tile's
quadratic-half image, out of either accumulator).

Which bits may move.  Every block's quadratic-half image holds the same values and a model's products, their order and its order
over the mixture tiles do not change with pairing -- except for the model whose image is the last one executed in a mixture tile:
its per-tile contributions are summed apart and added at the close.  Block by block that is model 4 ceil((1 + m) / 4) - 2 of a
block of m models (when there is such a model); in a pair (15, m) it is the second block's model min(31, 4 ceil((16 + m) / 4)) - 17."""
import numpy as np
import pytest

from conftest import ll_close

pytestmark = pytest.mark.gpu
TOL = 1e-4
SUM_TOL = 1e-5
SB = 15
NAME = "gmm_score_h2p_kernel<8,8,waves=12, pipelined in the wave>/compact"
LENS = [1, 31, 32, 33, 100, 8, 8, 8, 8, 385]          # packed tails (1, 31, 1, 4, 8 x 4, 1), 17 full tiles: more than one workgroup
SIZES = (16, 30, 31, 37, 45, 52)


@pytest.fixture(autouse=True)
def _reset_options(built_lib):
    from speaker_recognition_amd import _lib
    yield
    for k in ("score_engine", "score_h2s_force_exc", "score_h2s_shape", "score_model_groups"):
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


def _apart_models(S, paired, n_groups=1):
    """The models whose per-tile contributions are summed apart (module docstring), as indices into the set, for a set of S
    models scored in `n_groups` model groups -- group g takes blocks g * B // G .. (g + 1) * B // G (plan_groups), and a group
    walks its blocks two at a time where `paired`, a lone last one where their number is odd."""
    n_blocks = (S + SB - 1) // SB
    sizes = [min(SB, S - SB * b) for b in range(n_blocks)]
    out = set()
    for g in range(n_groups):
        b, end = g * n_blocks // n_groups, (g + 1) * n_blocks // n_groups
        while b < end:
            if paired and b + 1 < end and sizes[b] == SB:
                m = sizes[b + 1]
                last = min(31, 4 * ((16 + m + 3) // 4)) - 17
                if last < m:
                    out.add(SB * (b + 1) + last)
                b += 2
            else:
                m = sizes[b]
                last = 4 * ((1 + m + 3) // 4) - 2
                if last < m:
                    out.add(SB * b + last)
                b += 1
    return out


def test_apart_models_of_the_cases():
    """the rule above on the shapes this file uses, written out by hand (no GPU needed, but it is what the GPU tests lean on)"""
    assert _apart_models(30, False) == {14, 29} and _apart_models(30, True) == {29}
    assert _apart_models(37, False) == {14, 29, 36} and _apart_models(37, True) == {29, 36}
    assert _apart_models(52, False) == {14, 29, 44, 51} and _apart_models(52, True) == {29}      # (15, 7): image 23 is a phantom's
    assert _apart_models(16, True) == set() and _apart_models(31, True) == {29}
    assert _apart_models(52, True, 2) == {29} and _apart_models(52, True, 3) == {14, 29}         # groups of blocks [0,1) [1,2) [2,4)


@pytest.mark.parametrize("K", [32, 96])                # one mixture tile, three
@pytest.mark.parametrize("D", [37, 39])
def test_pairs_against_oracle(built_lib, oracle_built, D, K):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    for S in SIZES:
        models, utts, want = _case(oracle_built, D, K, S)
        ms = _set(models)
        _lib.set_option("score_engine", 6)
        _lib.set_option("score_h2s_shape", 3)
        _lib.set_option("score_model_groups", 1)       # (left to itself a batch this small gets a group per block: no pairs)
        for force in (0, 1):                           # ... and every tile through the exception pass
            _lib.set_option("score_h2s_force_exc", force)
            out = ms.score(Batch.from_features(utts), frame_ll=True)
            name = _lib.last_score_kernel()
            assert NAME in name and "once per 30 models" in name, name
            _check(out, want, LENS, "D=%d K=%d S=%d force_exc=%d" % (D, K, S, force))
        _lib.set_option("score_h2s_force_exc", 0)


def _same_bits_outside(a, b, apart, want, what):
    """two runs' (sums, argmax, frame_ll): bit-identical for every model outside `apart`, within 2 SUM_TOL inside, argmax equal"""
    S = a[2].shape[0]
    keep = np.array([s not in apart for s in range(S)])
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(a[0][:, keep], b[0][:, keep]), what
    assert np.array_equal(a[2][keep], b[2][keep]), what
    off = np.concatenate([[0], np.cumsum(LENS)])
    w = np.stack([want[:, off[u]:off[u + 1]].sum(axis=1) for u in range(len(LENS))])
    rel_sum = float(np.max(np.abs(a[0] - b[0]) / np.maximum(1.0, np.abs(w))))
    rel_ll = float(np.max(np.abs(a[2].astype(np.float64) - b[2]) / np.maximum(1.0, np.abs(want))))
    print("%s: models summed apart %s: sums differ by %.3e, frames by %.3e (relative)" % (what, sorted(apart), rel_sum, rel_ll))
    assert rel_sum <= 2 * SUM_TOL and rel_ll <= 2 * SUM_TOL, (what, rel_sum, rel_ll)


@pytest.mark.parametrize("S", [30, 37, 52])
@pytest.mark.parametrize("D", [37, 39])
def test_paired_against_block_by_block(built_lib, oracle_built, D, S):
    """score_h2s_shape 3 against 6 (one quadratic half per block) on the same inputs"""
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    K = 96
    models, utts, want = _case(oracle_built, D, K, S)
    ms = _set(models)
    _lib.set_option("score_engine", 6)
    _lib.set_option("score_model_groups", 1)           # one group: the blocks go (0, 1), (2, 3), a lone last one
    out = {}
    for shape in (6, 3):
        _lib.set_option("score_h2s_shape", shape)
        out[shape] = ms.score(Batch.from_features(utts), frame_ll=True)
        name = _lib.last_score_kernel()
        assert NAME in name and ("once per 30 models" if shape == 3 else "once per 15 models") in name, name
        _check(out[shape], want, LENS, "D=%d S=%d shape=%d" % (D, S, shape))
    _same_bits_outside(out[3], out[6], _apart_models(S, True) | _apart_models(S, False), want, "D=%d S=%d: 3 against 6" % (D, S))


@pytest.mark.parametrize("D", [37, 39])
def test_group_boundaries(built_lib, oracle_built, D):
    """S = 52 (four blocks) in 2 and 3 model groups: pairs and lone blocks in other places, a group that starts at an odd block"""
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    K, S = 96, 52
    models, utts, want = _case(oracle_built, D, K, S)
    ms = _set(models)
    _lib.set_option("score_engine", 6)
    _lib.set_option("score_h2s_shape", 3)
    out = {}
    for groups in (1, 2, 3):
        _lib.set_option("score_model_groups", groups)
        out[groups] = ms.score(Batch.from_features(utts), frame_ll=True)
        name = _lib.last_score_kernel()
        assert NAME in name and "once per 30 models" in name, name
        _check(out[groups], want, LENS, "D=%d groups=%d" % (D, groups))
    for groups in (2, 3):
        apart = _apart_models(S, True, 1) | _apart_models(S, True, groups)
        _same_bits_outside(out[groups], out[1], apart, want, "D=%d: %d groups against one" % (D, groups))


@pytest.mark.parametrize("D", [37, 39])
def test_rogue_frame_leaves_the_others_bits(built_lib, oracle_built, D):
    """tests/test_gpu_h2c.py's rogue frame at S = 37 (a pair and a lone block): a frame at +60 on every dimension goes to the exception
    pass, block by block; the utterances its tail is packed with keep their bits in every block -- both blocks of the pair
    included -- and so do the other frames of its own utterance; everything stays inside the gates."""
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    K, S, rogue = 96, 37, 6
    models, utts, want = _case(oracle_built, D, K, S)
    _, utts_r, want_r = _case(oracle_built, D, K, S, rogue=rogue)
    ms = _set(models)
    _lib.set_option("score_engine", 6)
    _lib.set_option("score_h2s_shape", 3)
    _lib.set_option("score_model_groups", 1)
    clean = ms.score(Batch.from_features(utts), frame_ll=True)
    dirty = ms.score(Batch.from_features(utts_r), frame_ll=True)
    assert NAME in _lib.last_score_kernel() and "once per 30 models" in _lib.last_score_kernel()
    _check(dirty, want_r, LENS, "D=%d rogue" % D)
    off = np.concatenate([[0], np.cumsum(LENS)])
    for u in range(len(LENS)):
        if u != rogue:
            assert np.array_equal(clean[0][u], dirty[0][u]) and clean[1][u] == dirty[1][u], u
            assert np.array_equal(clean[2][:, off[u]:off[u + 1]], dirty[2][:, off[u]:off[u + 1]]), u
    assert not np.array_equal(clean[0][rogue], dirty[0][rogue])
    others = [f for f in range(off[rogue], off[rogue + 1]) if f != off[rogue + 1] - 2]
    assert np.array_equal(clean[2][:, others], dirty[2][:, others])
