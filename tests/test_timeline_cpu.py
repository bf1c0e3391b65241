"""CPU: the timeline's checker checks itself (tests/timeline_oracle.py: the Viterbi recurrence against brute-force enumeration,
the hold rule against a transliteration of the reference GUI's lines, ties, NaN), the window count and the launch decisions
(sr_timeline_windows, sr_timeline_plan, csrc/timeline_plan.cpp -- also under the host sanitizers, tests/host/timeline_checks.cpp),
the refusals every entry point makes before it touches the device, the kernels' scratch, and the Python surface that needs no
device: segments, RTTM, the interface's and the command line's arguments."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timeline_oracle as to  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")


def test_viterbi_against_brute_force():
    """240 cases: T in {1,2,3,5,7} x S in {1,2,3} x m in {1..4} x beta in {0, 0.3, 2, 1e300}.  The recurrence adds in another
    order than the enumerator, so the two best scores agree to rounding (a few ulps of the largest partial sum); the decoded
    path keeps the run-length constraint and its own score, recomputed in window order, is the brute force's best."""
    rng = np.random.default_rng(11)
    cases = 0
    for T in (1, 2, 3, 5, 7):
        for S in (1, 2, 3):
            for m in (1, 2, 3, 4):
                for beta in (0.0, 0.3, 2.0, 1e300):
                    e = rng.normal(0.0, 1.0, (T, S))
                    lab, score = to.viterbi(e, -1, beta, m)
                    best = to.brute_force(e, beta, m)
                    tol = 64 * np.finfo(np.float64).eps * max(1.0, abs(best), beta if beta < 1e299 else 1.0)
                    if beta >= 1e299 and T > 1 and S > 1:
                        tol = 64 * np.finfo(np.float64).eps * max(1.0, abs(best))
                    assert to.runs_ok(list(lab), m), (T, S, m, beta, lab)
                    assert abs(to.path_score(e, lab, beta) - best) <= tol, (T, S, m, beta)
                    assert abs(score - best) <= tol, (T, S, m, beta, score, best)
                    cases += 1
    assert cases == 240


def test_beta_zero_is_raw_and_huge_beta_is_one_label():
    rng = np.random.default_rng(3)
    for S, bg in ((1, -1), (4, -1), (5, 2), (7, 0)):
        # (untied draws: with a tie inside a window, "staying wins equality" may keep the later window's state where raw takes
        # the first maximum -- the path score is the same)
        x = rng.normal(0.0, 1.0, (60, S))
        lab, score = to.viterbi(x, bg, 0.0, 1)
        assert np.array_equal(lab, to.raw(x, bg))
        assert score == float(np.add.accumulate(x.max(axis=1))[-1])
        e = rng.integers(-4, 5, (60, S)).astype(np.float64)           # ties occur
        assert to.viterbi(e, bg, 0.0, 1)[1] == float(e.max(axis=1).sum())
        for m in (1, 2, 5):
            lab, score = to.viterbi(e, bg, 1e300, m)
            totals = np.add.accumulate(e, axis=0)[-1]                 # in window order, as the recurrence adds a state that stays
            best = to.first_max(totals, to.order(S, bg))
            assert np.all(lab == (-1 if best == bg else best)) and score == totals[best]


def _gui_hold(labels):
    """gui.py:195-204 line by line: `label` is a name or None, conv_result_list the raw labels so far."""
    conv_result_list = []
    last_label_to_show = None
    shown = []
    for label in labels:
        label_to_show = label
        if label and conv_result_list:
            last_label = conv_result_list[-1]
            if last_label and last_label != label:
                label_to_show = last_label_to_show
        conv_result_list.append(label)
        last_label_to_show = label_to_show
        shown.append(label_to_show)
    return shown


def test_hold_is_the_gui_rule():
    rng = np.random.default_rng(8)
    rows = [np.array([0, 1] * 1500, dtype=np.int32),                   # an alternating stretch longer than 2048 windows
            np.array([2] + [0, 1] * 1100 + [1, 1, -1, 0, 0, 1], dtype=np.int32),
            np.array([-1, -1, 0, -1, 1, 1, -1, -1, 2, 0, -1], dtype=np.int32),
            np.zeros(0, dtype=np.int32), np.array([3], dtype=np.int32)]
    rows += [rng.integers(-1, 3, n).astype(np.int32) for n in (2, 17, 255, 256, 257, 1000)]
    for r in rows:
        names = [None if x < 0 else "s%d" % x for x in r]
        want = [-1 if x is None else int(x[1:]) for x in _gui_hold(names)]
        assert to.hold(r).tolist() == want
    assert to.hold(rows[0]).tolist() == [0] * 3000                     # nothing ever agrees twice: the first label stays


def test_ties_and_nan():
    # a duplicated column: the lower index wins; a speaker equal to the nobody emission: the speaker wins
    sums = np.array([[3.0, 5.0, 5.0, 1.0], [4.0, 4.0, 2.0, 4.0]])
    counts = np.array([1, 2], dtype=np.int32)
    lab, _, bad = to.decide(sums, counts)
    assert lab.tolist() == [1, 0] and bad == 0
    lab, _, _ = to.decide(sums, counts, bg=1)                          # nobody (column 1) ties with speaker 2, then with speakers 0 and 3
    assert lab.tolist() == [2, 0]
    lab, _, _ = to.decide(sums, counts, bg=1, threshold=0.5)
    assert lab.tolist() == [-1, -1]
    lab, _, _ = to.decide(sums, counts, bg=0, threshold=1.0)           # window 0: 3 + 1 < 5; window 1: 2 + 1 > 2
    assert lab.tolist() == [1, -1]
    assert to.decide(sums, counts, bg=1, mode=1)[0].tolist() == [2, 2]          # hold: 2 then 0 do not agree, 2 stays
    assert to.decide(sums, counts, bg=1, mode=2, beta=0.0, m=1)[0].tolist() == [2, 0]
    # NaN: -inf before any comparison, the window counted once however many columns
    sums = np.array([[np.nan, 1.0, np.nan], [2.0, np.nan, 0.0], [np.nan, np.nan, np.nan], [1.0, 2.0, 3.0], [-np.inf, -np.inf, -np.inf]])
    lab, _, bad = to.decide(sums, np.ones(5, dtype=np.int32))
    assert lab.tolist() == [1, 0, -1, 2, -1] and bad == 3
    e, _ = to.emissions(sums, np.ones(5, dtype=np.int32))
    assert not np.isnan(e).any()
    lab, score, bad = to.decide(sums[:4], np.ones(4, dtype=np.int32), mode=2, beta=0.0, m=1)
    assert bad == 3 and score == float("-inf")                         # a window of -inf everywhere: no finite path
    # in-order sums: a sequential accumulate, not a pairwise tree
    x = np.array([[1e8, 1.0, -1e8, 1.0] * 8], dtype=np.float32)
    s, c = to.window_sums(x, 32, 32)
    acc = 0.0
    for v in x[0]:
        acc += float(v)
    assert s[0, 0] == acc and c.tolist() == [32]


def test_window_count(built_lib):
    from speaker_recognition_amd import _lib, timeline as tl
    for W, H in ((3, 7), (5, 5), (10, 4), (1, 1), (150, 40)):
        for n in (0, 1, W - 1, W, W + 1, W + H, W + H + 1):
            want = to.windows(n, W, H)
            assert _lib.timeline_windows(n, W, H) == want == tl.windows(n, W, H)
            if n > 0:
                starts = list(range(0, n, H))                          # a window starts inside the recording
                k = next((j for j, a in enumerate(starts) if a + W >= n), len(starts) - 1)
                assert want == k + 1                                   # the first window that reaches the end is the last
                if W >= H:
                    assert want == 1 + -(-max(0, n - W) // H)
            s, c = to.window_sums(np.ones((2, n), np.float32), W, H)
            assert len(s) == want and (want == 0 or (c[:-1] == W).all() and c[-1] == min(W, n - (want - 1) * H))
    assert _lib.timeline_windows(10, 0, 1) == 0 and _lib.timeline_windows(10, 1, 0) == 0 and _lib.timeline_windows(-1, 1, 1) == 0
    with pytest.raises(ValueError):
        tl.windows(10, 0, 1)


def test_plan_sweep_and_refusals(built_lib):
    from speaker_recognition_amd import _lib
    for S in (1, 2, 63, 64, 65, 1024, 1025, 4096):
        for m in (1, 2, 16):
            tile = _lib.timeline_plan(S, m)["tile"]
            for nw in (0, 1, tile - 1, tile, tile + 1, 2 * tile + 3):
                n = 0 if nw == 0 else 150 + 40 * (nw - 1)
                p = _lib.timeline_plan(S, m, n, 150, 40)
                assert p["windows"] == nw
                variant = 0 if S <= 64 else 1 if S <= 1024 else 2
                assert (p["variant"], p["states_per_lane"], p["tile"]) == (variant, 4 if variant == 2 else 1, 2 if variant == 2 else 8)
                assert p["lanes"] == (64 if variant == 0 else -(-S // 64) * 64 if variant == 1 else 1024)
                assert p["lanes"] * p["states_per_lane"] >= S
                assert p["chain_slots"] == (m - 1 if m > 2 else 0)
                ring = p["chain_slots"] * p["lanes"] * p["states_per_lane"] * 8
                assert p["chain_lds"] == int(0 < ring <= 48 * 1024)
                assert p["fwd_lds"] == 384 + (ring if p["chain_lds"] else 0) <= 65536
                assert (p["sum_span"], p["sum_chunk"], p["sum_lds"]) == (270, 64, 64 * 65 * 4)
                assert (p["sum_grid_x"], p["sum_grid_y"]) == (-(-nw // 4), -(-S // 64))
                assert p["bp_bytes"] == 8 * -(-S // 64) + 4 and (p["max_states"], p["max_min_dur"]) == (4096, 16)
    for kw, pat in ((dict(S=0), "columns"), (dict(S=4097), "4096"), (dict(min_dur=0), "min_dur"), (dict(min_dur=17), "min_dur"),
                    (dict(window=0), "window"), (dict(hop=0), "hop"), (dict(n_frames=-1), "frame")):
        with pytest.raises(_lib.SRError, match=pat):
            _lib.timeline_plan(**dict(dict(S=4), **kw))
    v = (C.c_int32 * 16)()
    assert _lib.lib().sr_timeline_plan(4, 1, 10, 5, 5, v, 15) == -1 and "16 fields" in _lib.last_error()
    assert _lib.lib().sr_timeline_plan(4, 1, 10, 5, 5, None, 16) == -1


def test_decide_refuses_before_the_device(built_lib):
    """Every refusal of the rule comes before the device is touched: they are raised on a machine without one."""
    from speaker_recognition_amd import _lib
    sums, counts, off = np.zeros((3, 4)), np.ones(3, np.int32), np.array([0, 3])
    nan = float("nan")
    for kw, pat in ((dict(bg=4), "background"), (dict(bg=-2), "background"), (dict(threshold=nan), "threshold"), (dict(mode=3), "mode"),
                    (dict(mode=-1), "mode"), (dict(mode=2, beta=nan), "beta"), (dict(mode=2, beta=-1.0), "beta"),
                    (dict(mode=2, min_dur=0), "min_dur"), (dict(mode=2, min_dur=17), "min_dur")):
        with pytest.raises(_lib.SRError, match=pat):
            _lib.timeline_decide(sums, counts, off, **kw)
    with pytest.raises(_lib.SRError, match="4096"):
        _lib.timeline_decide(np.zeros((1, 4097)), np.ones(1, np.int32), np.array([0, 1]))
    with pytest.raises(_lib.SRError, match="at least one"):
        _lib.timeline_decide(sums, np.array([1, 0, 1], np.int32), off)
    with pytest.raises(_lib.SRError, match="negative window count"):
        _lib.timeline_decide(sums, counts, np.array([0, 5, 3]))
    L = _lib.lib()
    assert L.sr_timeline_batch(None, None, 10, 5, -1, 0.0, 0, 0.0, 1, 0, None, None, None, None, None) == -1 and "null" in _lib.last_error()
    assert L.sr_fullset_timeline_batch(None, None, 10, 5, 0.0, 0, 0.0, 1, None, None, None, None, None) == -1 and "null" in _lib.last_error()
    assert L.sr_timeline_pcm_batch(None, None, None, 0, 10, 5, -1, 0.0, 0, 0.0, 1, 0, None, None, None, None, None) == -1
    assert "null" in _lib.last_error()


def test_header_documents_the_calls(built_lib):
    header = open(os.path.join(ROOT, "include", "pygmm_hip.h")).read()
    for text in ("sr_timeline_windows", "sr_timeline_plan", "sr_timeline_decide", "sr_timeline_batch", "sr_fullset_timeline_batch",
                 "sr_timeline_pcm_batch", "gui.py:195-204", "staying wins equality"):
        assert text in header


def test_timeline_kernels_do_not_spill(built_lib):
    import test_abi_cpu
    res = test_abi_cpu._kernel_resources("timeline")
    names = " ".join(res)
    for kernel in ("timeline_sum_kernel", "timeline_raw_kernel", "timeline_hold_kernel", "timeline_trace_kernel"):
        assert kernel in names
    assert sum("timeline_forward_kernel" in n for n in res) == 3         # one wave, a lane per state, lanes looping over states
    for name, r in res.items():
        assert r["scratch"] == 0, (name, r)


def test_segments_and_rttm():
    from speaker_recognition_amd import timeline as tl
    # W = 10, H = 4: label j owns frames [4 j + 3, 4 j + 7); 30 frames -> 6 windows
    assert tl.windows(30, 10, 4) == 6
    segs = tl.segments([0, 0, 1, 1, -1, 2], 30, 10, 4, 0.5)
    assert segs == [(0.0, 5.5, 0), (5.5, 9.5, 1), (9.5, 11.5, -1), (11.5, 15.0, 2)]
    assert tl.segments([5], 3, 10, 4, 0.01) == [(0.0, 0.03, 5)]          # one short window: the whole recording
    assert tl.segments([], 0, 10, 4, 0.01) == []
    assert tl.segments([1, 1, 1], 24, 8, 8, 1.0) == [(0.0, 24.0, 1)]
    segs = tl.segments([0, 1, 0], 20, 5, 8, 1.0)                         # a hop longer than the window: the hops tile
    assert segs == [(0.0, 8.0, 0), (8.0, 16.0, 1), (16.0, 20.0, 0)]
    for n, W, H in ((240, 300, 7), (320, 300, 7), (37, 10, 5), (100, 1, 1)):
        labs = np.arange(tl.windows(n, W, H)) % 3
        segs = tl.segments(labs, n, W, H, 0.016)
        assert segs[0][0] == 0.0 and abs(segs[-1][1] - n * 0.016) < 1e-12
        assert all(a[1] == b[0] and a[1] > a[0] for a, b in zip(segs, segs[1:]))
    with pytest.raises(ValueError):
        tl.segments([0, 1], 30, 10, 4, 0.5)
    rttm = tl.to_rttm([(0.0, 5.5, 0), (5.5, 9.5, -1), (9.5, 15.0, 1), (15.0, 16.0, None)], names=["ann", "bob"], recording_id="call7")
    assert rttm == ("SPEAKER call7 1 0.000 5.500 <NA> <NA> ann <NA> <NA>\n"
                    "SPEAKER call7 1 9.500 5.500 <NA> <NA> bob <NA> <NA>\n")
    assert tl.to_rttm([(0.0, 1.0, "carol"), (1.0, 2.0, 3)]).splitlines()[1].split()[7] == "spk3"
    assert tl.to_rttm([]) == ""


def test_interface_and_cli_arguments(built_lib):
    from speaker_recognition_amd import cli
    from speaker_recognition_amd.core import _timeline_args
    from speaker_recognition_amd.interface import ModelInterface
    assert _timeline_args(150, 40, None, 0.0, "hold", None, 1) == (150, 40, -1, 0.0, 1, 0.0, 1)
    assert _timeline_args(150, 40, 0, 0.5, "viterbi", 2.0, 2) == (150, 40, 0, 0.5, 2, 2.0, 2)
    assert _timeline_args(1, 1, None, 0.0, "none", None, 1)[4] == 0
    with pytest.raises(ValueError, match="switch_penalty"):
        _timeline_args(150, 40, None, 0.0, "viterbi", None, 1)
    for bad in (dict(smooth="median"), dict(window=1.5), dict(hop=True), dict(min_windows=2.0)):
        kw = dict(dict(window=150, hop=40, bg=None, threshold=0.0, smooth="hold", switch_penalty=None, min_windows=1), **bad)
        with pytest.raises(ValueError):
            _timeline_args(**kw)
    m = ModelInterface(verbose=False)
    assert m._timeline_frames(1.5, 0.4, None) == (0.016, 94, 25, 1)
    assert m._timeline_frames(1.5, 0.4, 0.8) == (0.016, 94, 25, 2)
    assert ModelInterface(verbose=False, feature_kwargs=dict(win_shift_ms=10))._timeline_frames(1.5, 0.4, 0.4) == (0.01, 150, 40, 1)
    for bad in ((0, 0.4, None), (1.5, -1, None), (1.5, 0.4, -1), (1.5, 0.4, 100.0), ("1", 0.4, None)):
        with pytest.raises(ValueError):
            m._timeline_frames(*bad)
    with pytest.raises(ValueError, match="switch_penalty"):
        m.timeline(16000, np.zeros(16000, np.int16), smooth="viterbi")
    with pytest.raises(ValueError, match="UBM"):
        m.timeline(16000, np.zeros(16000, np.int16), reject_threshold=0.5)
    base = ["-t", "timeline", "-i", "x", "-m", "y"]
    a = cli.get_args(base)
    assert (a.task, a.window, a.hop, a.smooth, a.switch_penalty, a.min_duration, a.reject_threshold) == ("timeline", 1.5, 0.4, "hold", None, None, None)
    a = cli.get_args(base + ["--window", "2", "--hop", "0.5", "--smooth", "viterbi", "--switch-penalty", "3", "--min-duration", "1",
                             "--reject-threshold", "0.2"])
    assert (a.window, a.hop, a.smooth, a.switch_penalty, a.min_duration, a.reject_threshold) == (2.0, 0.5, "viterbi", 3.0, 1.0, 0.2)
    with pytest.raises(SystemExit):
        cli.get_args(base + ["--smooth", "median"])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_timeline_plan_under_asan_ubsan(tmp_path):
    """csrc/timeline_plan.cpp swept over column counts, minimum durations, lengths, windows and hops by a stand-alone program
    (tests/host/timeline_checks.cpp) built with AddressSanitizer + UBSan: host code only, no GPU, nothing loaded into Python."""
    exe = str(tmp_path / "timeline_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "host", "timeline_checks.cpp"), os.path.join(CSRC, "timeline_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "timeline checks ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
