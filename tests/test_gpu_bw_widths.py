"""The Baum-Welch statistics kernels of csrc/bw_stats.hip at the padded row widths tests/test_gpu_bw_stats.py does not reach: its
test_parity_ragged_batches runs D = 1, 13, 39, 40 (DP 8, 13, 39, 40); here, by the same recipe and the same four gates of
tests/bw_cases.py, the smallest and the largest dim of every other width -- DP 16 and 32, whose mixed block is the count alone, and
DP 16, 24, 26, the only ones with a single full block -- and D = 8, 9, 14, 35, the ends of the four widths it enters from one side.
At D = 16, 24 and 32 also with the default range length and with one range of nine tiles; at D = 16 and 34 the resident entry point
returns the batch entry point's bits.  tests/test_em_width_cases_cpu.py shows that neighbouring dimensions of every mixture's F differ
by more than a hundred F gates in these rows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bw_cases as bc  # noqa: E402
import em_width_cases as wc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _options(built_lib):
    from speaker_recognition_amd import _lib
    yield
    _lib.set_option("bw_range_frames", 0)


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
    print("bw width %s: gates N %.3g F %.3g sum %.3g ll %.3g (<= 1 passes)" % (what, g["N"], g["F"], g["sum"], g["ll"]))
    assert bc.passes(g), (what, g)
    return N, F, ll, dropped


@pytest.mark.parametrize("D", wc.BW_DIMS)
@pytest.mark.parametrize("K", wc.BW_KS)
def test_parity_ragged_batches_at_every_width(built_lib, K, D):
    from speaker_recognition_amd import _lib
    _lib.set_option("bw_range_frames", wc.BW_R)        # several ranges at tiny sizes
    ubm, utts = wc.bw_case(bc, K, D)
    N, F, ll, dropped = _check(ubm, utts, "K=%d D=%d" % (K, D))
    assert not N[0].any() and not F[0].any() and ll[0] == 0.0 and not dropped.any()          # the empty utterance: zeros


@pytest.mark.parametrize("D", wc.BW_LONG_DIMS)
def test_parity_long_ranges(built_lib, D):
    """The default range length cuts the utterance of 1100 frames into a range of eight full tiles and one of 76 frames; a range
    length of 1100 makes it one range of nine tiles, the last ragged."""
    from speaker_recognition_amd import _lib
    ubm, utts = wc.bw_long_case(bc, D)
    lengths = [len(u) for u in utts]
    assert _lib.bw_plan(wc.BW_LONG_K, D, lengths, 0)["n_ranges"] == 2 + 9 and _lib.bw_plan(wc.BW_LONG_K, D, lengths, wc.BW_LONG_T)["n_ranges"] == 1 + 9
    _check(ubm, utts, "K=%d D=%d default ranges" % (wc.BW_LONG_K, D))
    _lib.set_option("bw_range_frames", wc.BW_LONG_T)
    _check(ubm, utts, "K=%d D=%d one range of nine tiles" % (wc.BW_LONG_K, D))


@pytest.mark.parametrize("D", wc.BW_RESIDENT_DIMS)
def test_resident_pass_is_the_batched_pass(built_lib, D):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch, ModelSet
    _lib.set_option("bw_range_frames", wc.BW_R)
    K = 65
    ubm, utts = wc.bw_case(bc, K, D)
    feats = Batch.from_features([u.astype(np.float32).reshape(-1, D) for u in utts])
    ms = ModelSet([_gmm(ubm)])
    N, F, ll, dropped = ms.bw_stats(feats, 0, ll=True)
    stats, ll_r, dropped_r = ms.bw_stats(feats, 0, ll=True, resident=True)
    with stats:
        assert (stats.n, stats.K, stats.D) == (len(utts), K, D)
        Nr, Fr = stats.get()
    assert np.array_equal(Nr, N) and np.array_equal(Fr, F) and np.array_equal(ll_r, ll) and np.array_equal(dropped_r, dropped)
    assert not Nr[0].any() and Nr[1:].any()
    g = bc.gates(N, F, ll, dropped, bc.batch_stats(utts, ubm), [len(x) for x in utts])
    assert bc.passes(g), (D, g)
