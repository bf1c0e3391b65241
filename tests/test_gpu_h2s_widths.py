"""The shared-sigma scoring engines at every chain length they are built for (tests/h2s_width_cases.py), against the float64 oracle:
the split-fp16 engine (score_engine 6) as the 4-wave, the 12-wave, the pipelined and the model-split kernel, through its online
exception kernel (score_h2s_force_exc), with one and with several model groups, on 15 (KQF, KLF) pairs -- the smallest and the largest
D of each -- and the split-bf16 engine (score_engine 4) on its six.
Gates, the project's own: per frame |dLL| <= 1e-4 max(1, |LL|), utterance sums within 1e-5 relative, argmax equal on every utterance
(tests/test_h2s_width_cases_cpu.py shows the oracle's argmax is decided by more than the sums gate leaves open).  A kernel name is
checked on every call: a shape that silently became another one would pass the gates and test nothing."""
import numpy as np
import pytest

import h2s_width_cases as wc
from conftest import ll_close

pytestmark = pytest.mark.gpu
OPTIONS = ("score_engine", "score_h2s_shape", "score_h2s_force_exc", "score_model_groups")


@pytest.fixture(autouse=True)
def _reset_options(built_lib):
    from speaker_recognition_amd import _lib
    yield
    for k in OPTIONS:
        _lib.set_option(k, 0)


_SETS = {}


def _set(D, K, S):
    """the device's model set of a row, packed once (the rogue rows share their clean row's models)"""
    if (D, K, S) not in _SETS:
        from speaker_recognition_amd.core import ModelSet
        from speaker_recognition_amd.pygmm import GMM
        _SETS[(D, K, S)] = ModelSet([GMM.from_arrays(*m) for m in wc.make_case(D, K, S)[0]])
    return _SETS[(D, K, S)]


def _score(ms, utts, engine=6, shape=0, force=0, groups=0, expect=None, **kw):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    for k, v in zip(OPTIONS, (engine, shape, force, groups)):
        _lib.set_option(k, v)
    out = ms.score(Batch.from_features(list(utts)), frame_ll=True, **kw)
    name = _lib.last_score_kernel()
    assert expect is None or name.startswith(expect), (name, expect)
    return out


class Worst:
    """the worst ratios of a test, printed as they stand when it ends (also when it fails)"""

    def __init__(self, test, pair):
        self.head, self.frame, self.sum = "%s[%s]" % (test, wc.pair_id(pair)), 0.0, 0.0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        print("h2s widths %s: worst per frame %.3e of %.0e, worst sum %.3e of %.0e" % (self.head, self.frame, wc.TOL, self.sum, wc.SUM_TOL))

    def check(self, out, want, what):
        sums, arg, fll = out
        worst = ll_close(fll, want)
        w = wc.utterance_sums(want)
        worst_sum = float(np.max(np.abs(sums - w) / np.maximum(1.0, np.abs(w))))
        self.frame, self.sum = max(self.frame, worst), max(self.sum, worst_sum)
        if not (worst < wc.TOL and worst_sum < wc.SUM_TOL):
            print("%s %s: per frame %.3e, sums %.3e" % (self.head, what, worst, worst_sum))
        assert worst < wc.TOL, (what, worst)
        assert worst_sum < wc.SUM_TOL, (what, worst_sum)
        assert np.array_equal(arg, np.argmax(w, axis=1)), (what, arg, np.argmax(w, axis=1))


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("pair", wc.PAIRS, ids=wc.pair_id)
def test_every_shape_against_oracle(built_lib, oracle_built, pair):
    """every kernel form of the pair x the exception kernel alone x one group / two, at (50, 17): name, gates, the same bits on a
    second call, and the 100-frame utterance scored alone keeps its bits of the batch"""
    K, S = wc.BASE
    with Worst("every_shape", pair) as worst:
        for D in wc.DIMS[pair]:
            _, utts = wc.make_case(D, K, S)
            want = wc.oracle_values(oracle_built, D, K, S)
            ms = _set(D, K, S)
            for shape in (1, 2, 3, 4):
                for force in (0, 1):
                    for groups in (0, 2):
                        what = "D=%d shape=%d force_exc=%d groups=%d" % (D, shape, force, groups)
                        kw = dict(shape=shape, force=force, groups=groups, expect=wc.expected_kernel(D, shape))
                        out = _score(ms, utts, **kw)
                        worst.check(out, want, what)
                        assert _same(out, _score(ms, utts, **kw)), what
                        alone = _score(ms, [utts[wc.ALONE]], **kw)
                        assert np.array_equal(alone[0][0], out[0][wc.ALONE]) and alone[1][0] == out[1][wc.ALONE], what


@pytest.mark.parametrize("pair", wc.PAIRS, ids=wc.pair_id)
def test_model_split_leaves_the_four_wave_bits(built_lib, pair):
    """DESIGN states it of the model-split shape (gmm_score_h2m_kernel; the LDS form at KLF = 10): sums and per-frame values are those of the
    plain 4-wave kernel, bit for bit, with the reference's underflow rule and without"""
    K, S = wc.BASE
    for D in wc.DIMS[pair]:
        _, utts = wc.make_case(D, K, S)
        ms = _set(D, K, S)
        for compat in (True, False):
            four = _score(ms, utts, shape=1, expect=wc.expected_kernel(D, 1), clamp_compat=compat)
            split = _score(ms, utts, shape=4, expect=wc.expected_kernel(D, 4), clamp_compat=compat)
            assert np.array_equal(four[2], split[2]), (D, compat, float(np.max(np.abs(four[2] - split[2]))))
            assert np.array_equal(four[0], split[0]) and np.array_equal(four[1], split[1]), (D, compat)


@pytest.mark.parametrize("pair", wc.PAIRS, ids=wc.pair_id)
def test_set_sizes_at_the_widest_dim(built_lib, oracle_built, pair):
    """(32, 12): one mixture tile, one partial block, the smallest set the engine takes; (96, 31): three tiles, blocks of 15 + 15 + 1 (the
    last block's phantom stages are skipped).  At D = 38 and 42 also the pipelined kernel on the flat image and with one quadratic half
    per block (score_h2s_shape 5, 6)."""
    D = wc.DIMS[pair][-1]
    with Worst("set_sizes", pair) as worst:
        for K, S in wc.SIZES:
            _, utts = wc.make_case(D, K, S)
            want = wc.oracle_values(oracle_built, D, K, S)
            ms = _set(D, K, S)
            for shape in (1, 2, 3, 4) + ((5, 6) if D in (38, 42) else ()):
                for groups in (1, 3):
                    for force in (0, 1):
                        out = _score(ms, utts, shape=shape, force=force, groups=groups, expect=wc.expected_kernel(D, shape))
                        worst.check(out, want, "D=%d K=%d S=%d shape=%d groups=%d force_exc=%d" % (D, K, S, shape, groups, force))


@pytest.mark.parametrize("pair", wc.PAIRS, ids=wc.pair_id)
def test_rogue_frame(built_lib, oracle_built, pair):
    """One frame of an 8-frame utterance at +60 on every dimension: the offset form refuses it and its tile's column goes to the
    exception pass.  Everything stays inside the gates, and every other utterance -- those its tail is packed with in the pipelined
    kernel among them -- keeps the bits of the clean run."""
    D, (K, S) = wc.DIMS[pair][-1], wc.BASE
    _, utts = wc.make_case(D, K, S)
    _, utts_r = wc.make_case(D, K, S, rogue=wc.ROGUE)
    want_r = wc.oracle_values(oracle_built, D, K, S, rogue=wc.ROGUE)
    ms = _set(D, K, S)
    off = wc.offsets()
    with Worst("rogue_frame", pair) as worst:
        for shape in (1, 2, 3, 4):
            clean = _score(ms, utts, shape=shape, expect=wc.expected_kernel(D, shape))
            dirty = _score(ms, utts_r, shape=shape, expect=wc.expected_kernel(D, shape))
            worst.check(dirty, want_r, "D=%d shape=%d rogue" % (D, shape))
            for u in range(len(wc.LENS)):
                if u != wc.ROGUE:
                    assert np.array_equal(clean[0][u], dirty[0][u]) and clean[1][u] == dirty[1][u], (shape, u)
                    assert np.array_equal(clean[2][:, off[u]:off[u + 1]], dirty[2][:, off[u]:off[u + 1]]), (shape, u)
            assert not np.array_equal(clean[0][wc.ROGUE], dirty[0][wc.ROGUE]), shape


@pytest.mark.parametrize("D", wc.BX3_DIMS, ids=lambda D: wc.pair_id(wc.bx3_pair_of(D)))
def test_bf16_shared_engine(built_lib, oracle_built, D):
    """the fp32-grade fallback gmm_score_bx3_shared_kernel<KQ,KL> on its six pairs: name, gates, and per frame within 1e-5 max(1, |LL|)
    of the split-fp16 engine on the same inputs"""
    K, S = wc.BASE
    _, utts = wc.make_case(D, K, S)
    want = wc.oracle_values(oracle_built, D, K, S)
    ms = _set(D, K, S)
    f16 = _score(ms, utts, engine=6, expect="gmm_score_h2")
    with Worst("bf16_shared", wc.bx3_pair_of(D)) as worst:
        for groups in (1, 2):
            out = _score(ms, utts, engine=4, groups=groups, expect=wc.expected_bx3_kernel(D))
            worst.check(out, want, "D=%d engine 4 groups=%d" % (D, groups))
            apart = float(np.max(np.abs(out[2] - f16[2]) / np.maximum(1.0, np.abs(want))))
            print("D=%d groups=%d: engine 4 against engine 6 per frame %.3e of %.0e" % (D, groups, apart, wc.ENGINE_TOL))
            assert apart < wc.ENGINE_TOL, (D, groups, apart)
            assert np.array_equal(out[1], f16[1])
