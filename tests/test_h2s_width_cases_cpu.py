"""The width table of the shared-sigma scoring engines (tests/h2s_width_cases.py) without a GPU: the conditions that make it a
fair yardstick for tests/test_gpu_h2s_widths.py.  Every chain length the two kernel files are built for is reached by a row (so a
new one cannot be added without a row), the expected kernel names agree with csrc/score_shapes.hpp, the oracle's argmax is decided
by more than the sums gate allows the device to be off, the sets lie inside the range the dispatcher offers the split-fp16 engine,
and the rogue rows need the exception path."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import h2s_width_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")


def _built_pairs(source, macro):
    """the (q, l) of every `macro(q, l)` in a kernel file, its definition apart"""
    with open(os.path.join(CSRC, source)) as f:
        text = f.read()
    return [(int(q), int(l)) for q, l in re.findall(macro + r"\((\d+), *(\d+)\)", text)]


def test_table_is_the_one_written_down():
    assert wc.DIMS == {(1, 1): [1, 4], (1, 2): [5], (2, 2): [6, 10], (3, 3): [11, 15], (3, 4): [16], (4, 4): [17, 20], (4, 5): [21],
                       (5, 5): [22, 26], (6, 6): [27, 31], (6, 7): [32], (7, 7): [33, 36], (7, 8): [37], (8, 8): [38, 42],
                       (9, 9): [43, 47], (9, 10): [48]}
    assert len(wc.PAIRS) == 15 and len(wc.ALL_DIMS) == 24
    assert wc.BX3_PAIRS == [(1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (3, 4)]
    assert sum(wc.LENS) == 614 and wc.LENS[wc.ALONE] == 100 and wc.LENS[wc.ROGUE] == 8
    # 24 base rows; the widest D of each of the 15 pairs: two more set sizes and a rogue row
    assert len(wc.rows()) == 24 + 3 * 15 and len(set(wc.rows())) == len(wc.rows())
    # D = 10, 26, 42 fill the linear half's last step exactly, D = 16, 32, 48 the quadratic half's
    assert all((3 * D + 2) % 16 == 0 for D in (10, 26, 42)) and all(3 * D % 16 == 0 for D in (16, 32, 48))
    assert {10, 26, 42, 16, 32, 48} <= set(wc.ALL_DIMS)


def test_every_built_pair_is_reachable():
    h2s = _built_pairs("gmm_score_h2_shared.hip", "SR_H2S_CASE")
    bx3 = _built_pairs("gmm_score_bx3_shared.hip", "SR_SH_CASE")
    assert len(set(h2s)) == len(h2s) and len(set(bx3)) == len(bx3)
    assert set(h2s) == {wc.pair_of(D) for D in range(1, wc.MAX_DIM + 1)}, sorted(h2s)
    assert set(bx3) == {wc.bx3_pair_of(D) for D in range(1, wc.MAX_DIM + 1)}, sorted(bx3)
    assert {wc.pair_of(D) for D in wc.ALL_DIMS} == set(h2s)
    assert {wc.bx3_pair_of(D) for D in wc.BX3_DIMS} == set(bx3)
    assert all(wc.pair_of(D) == p for p, ds in wc.DIMS.items() for D in ds)
    # the widest set either engine is offered (score_plan.cpp: shared_ok)
    with open(os.path.join(CSRC, "score_plan.cpp")) as f:
        assert "models[0]->dim <= %d" % wc.MAX_DIM in f.read()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_expected_kernel_agrees_with_the_header(tmp_path):
    exe = str(tmp_path / "h2s_width_checks")
    b = subprocess.run(["g++", "-O1", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tests", "host", "h2s_width_checks.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-1000:]
    header = {}
    for line in r.stdout.split("\n"):
        if line.strip():
            D, q, l, fits, cpt, direct = (int(v) for v in line.split())
            header[D] = ((q, l), bool(fits), bool(cpt), bool(direct))
    assert sorted(header) == list(range(1, wc.MAX_DIM + 1))
    for D in range(1, wc.MAX_DIM + 1):
        (q, l), fits, cpt, direct = header[D]
        assert wc.pair_of(D) == (q, l) and wc.h2p_fits(q, l) == fits == (2 <= l <= 8) and wc.compact(D) == cpt == (37 <= D <= 39), D
        assert direct == (l <= 9), D
        assert wc.expected_kernel(D, 1) == "gmm_score_h2s_kernel<%d,%d,waves=4> " % (q, l)
        assert wc.expected_kernel(D, 2) == "gmm_score_h2s_kernel<%d,%d,waves=12> " % (q, l)
        pipelined = "gmm_score_h2p_kernel<%d,%d,waves=12, pipelined in the wave> " % (q, l)
        assert wc.expected_kernel(D, 3) == ("gmm_score_h2p_kernel<8,8,waves=12, pipelined in the wave>/compact" if cpt else pipelined if fits
                                            else wc.expected_kernel(D, 2)), D
        assert wc.expected_kernel(D, 5) == (pipelined if fits else wc.expected_kernel(D, 2)), D
        assert wc.expected_kernel(D, 6) == wc.expected_kernel(D, 3), D
        assert wc.expected_kernel(D, 4) == "gmm_score_%s_kernel<%d,%d,waves=4 on one tile, models split> " % ("h2m" if direct else "h2s", q, l)
    # every form of the issue's list is met by a D of the table
    names = [wc.expected_kernel(D, s) for D in wc.ALL_DIMS for s in (1, 2, 3, 4)]
    met = {(n.split("<")[0], n.endswith("/compact")) for n in names}
    assert met == {("gmm_score_h2s_kernel", False), ("gmm_score_h2p_kernel", False), ("gmm_score_h2p_kernel", True), ("gmm_score_h2m_kernel", False)}
    assert [D for D in wc.ALL_DIMS if not header[D][3]] == [48]                      # the one length on the LDS form of the model-split shape
    assert sorted({wc.pair_of(D)[1] for D in wc.ALL_DIMS if header[D][1]}) == [2, 3, 4, 5, 6, 7, 8]


@pytest.mark.parametrize("pair", wc.PAIRS, ids=wc.pair_id)
def test_argmax_is_decided_and_sets_are_in_range(oracle_built, pair):
    """A device inside the sums gate is at most SUM_TOL max(1, |sum|) off on either of two sums: with the oracle's best and
    second-best 2 SUM_TOL max(1, |best|) apart it returns the oracle's argmax, on every utterance of every row."""
    for D, K, S, rogue in wc.rows():
        if wc.pair_of(D) != pair:
            continue
        models, utts = wc.make_case(D, K, S, rogue=rogue)
        assert len(models) == S and all(m[0] is models[0][0] and m[2] is models[0][2] for m in models)       # sigma and weights shared
        assert [len(u) for u in utts] == wc.LENS and all(u.shape[1] == D and u.dtype == np.float32 for u in utts)
        amp, ratio = wc.conditioning(models)
        sums = wc.utterance_sums(wc.oracle_values(oracle_built, D, K, S, rogue=rogue))
        top = np.sort(sums, axis=1)
        gap = (top[:, -1] - top[:, -2]) / np.maximum(1.0, np.abs(top[:, -1]))
        print("D=%d K=%d S=%d rogue=%s: amp %.0f, sigma ratio %.1f, smallest relative gap of the two best sums %.2e (utterance %d)"
              % (D, K, S, rogue, amp, ratio, gap.min(), int(np.argmin(gap))))
        assert amp < wc.F16_MAX_AMP and ratio < wc.F16_MAX_SIGMA_RATIO, (D, K, S, amp, ratio)
        assert np.all(gap >= 2 * wc.SUM_TOL), (D, K, S, rogue, gap)


@pytest.mark.parametrize("pair", wc.PAIRS, ids=wc.pair_id)
def test_rogue_row_is_genuine(oracle_built, pair):
    """The moved frame is a frame the reference's underflow rule decides: every model's density underflows there, so the oracle gives
    ln 1e-15 for it where the plain log-sum-exp lies far below -- the offset form cannot carry it, the exception pass must.  Nothing
    else of the row moves."""
    go = oracle_built
    D, (K, S) = wc.DIMS[pair][-1], wc.BASE
    models, utts = wc.make_case(D, K, S)
    _, utts_r = wc.make_case(D, K, S, rogue=wc.ROGUE)
    want, want_r = wc.oracle_values(go, D, K, S), wc.oracle_values(go, D, K, S, rogue=wc.ROGUE)
    f = int(wc.offsets()[wc.ROGUE + 1]) - 2
    assert all(np.array_equal(a, b) == (u != wc.ROGUE) for u, (a, b) in enumerate(zip(utts, utts_r)))
    same = np.ones(want.shape[1], dtype=bool)
    same[f] = False
    assert np.array_equal(want[:, same], want_r[:, same])
    x = np.concatenate(utts_r).astype(np.float64)[f:f + 1]
    plain = np.array([go.score_batch(go.GMMParams(*m), x, go.MODE_LOGSUMEXP, clamp_compat=False)[0] for m in models])
    print("D=%d: the rogue frame's plain log-likelihoods %.0f .. %.0f" % (D, plain.min(), plain.max()))
    assert np.all(plain < go.MINLOG) and go.MINLOG < go.LN_1E_15
    assert np.all(want_r[:, f] == go.LN_1E_15) and np.all(np.abs(want[:, f] - go.LN_1E_15) > 2 * wc.TOL * abs(go.LN_1E_15))
    s, s_r = wc.utterance_sums(want), wc.utterance_sums(want_r)
    assert np.all(s[wc.ROGUE] != s_r[wc.ROGUE]) and np.array_equal(np.delete(s, wc.ROGUE, 0), np.delete(s_r, wc.ROGUE, 0))
