"""CPU: the diarisation's checker checks itself (tests/diar_oracle.py: merged statistics against the statistics of the concatenated
frames, delta-BIC from statistics against slogdet of covariances from raw frames, Lance-Williams average linkage against the
definition, a re-cut against a rerun, the peak rule against a brute-force scan), the plan (sr_diar_plan, csrc/diar_plan.cpp -- also
under the host sanitizers, tests/host/diar_checks.cpp), the refusals every entry point makes before it touches the device, the
kernels' scratch, and the Python surface that needs no device: cut, frame_segments, RTTM, the interface's and the command line's
arguments."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diar_oracle as do  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")


def _frames(rng, n, D, mean=0.0, scale=1.0):
    return (mean + scale * rng.normal(0.0, 1.0, (n, D))).astype(np.float32)


def test_merged_statistics_are_the_statistics_of_the_concatenation():
    rng = np.random.default_rng(5)
    for D in (1, 2, 13):
        a, b = _frames(rng, 57, D, 0.5), _frames(rng, 130, D, -1.0, 2.0)
        merged = do.stats_of(a) + do.stats_of(b)
        whole = do.stats_of(np.concatenate([a, b]))
        assert merged[0] == whole[0] == 187
        # another order of the same 187 terms: a few ulps of the largest partial sum
        tol = 187 * do.EPS * np.abs(np.concatenate([a, b]).astype(np.float64)).max() ** 2 * 187
        assert np.abs(merged - whole).max() <= tol
        # in frame order, not a pairwise tree
        acc = np.zeros(D)
        for row in a.astype(np.float64):
            acc = acc + row
        assert np.array_equal(do.stats_of(a)[1:1 + D], acc)
    x = np.array([[1e8], [1.0], [-1e8], [1.0]] * 8, dtype=np.float32)
    acc = 0.0
    for v in x[:, 0].astype(np.float64):
        acc = acc + v * v
    assert do.stats_of(x)[2] == acc
    seg = do.seg_stats(_frames(rng, 25, 3), 10)
    assert len(seg) == 2 and seg[0, 0] == 10 and seg[1, 0] == 15          # the last segment reaches to n
    assert len(do.seg_stats(_frames(rng, 7, 3), 10)) == 1 and len(do.seg_stats(np.zeros((0, 3), np.float32), 10)) == 0


def test_delta_bic_from_statistics_against_slogdet_of_raw_covariances():
    rng = np.random.default_rng(6)
    for D in (1, 5, 13):
        for ridge in (0.0, 1e-3):
            a, b = _frames(rng, 90, D, 0.3), _frames(rng, 140, D, -0.2, 1.5)
            d, bnd = do.dbic_rows(do.stats_of(a), *(v[0] for v in do.logdet(do.stats_of(a), D, ridge)), do.stats_of(b)[None, :],
                                  *do.logdet(do.stats_of(b), D, ridge), D, 1.3, ridge)

            def ld(x):
                x = x.astype(np.float64)
                return np.linalg.slogdet(np.atleast_2d(np.cov(x.T, bias=True)) + ridge * np.eye(D))[1]
            ab = np.concatenate([a, b])
            want = 0.5 * (230 * ld(ab) - 90 * ld(a) - 140 * ld(b)) - 1.3 * 0.5 * (D + D * (D + 1) / 2) * np.log(230)
            assert abs(d[0] - want) <= bnd[0] and bnd[0] < 1e-6, (D, ridge, d[0], want, bnd[0])
    # a single frame has no covariance: the pivot is exactly 0
    one = do.stats_of(_frames(rng, 1, 4))
    assert not do.logdet(one, 4, 0.0)[1][0] and do.logdet(one, 4, 1e-3)[1][0]
    m, _, ld_, failed = do.bic_matrix(np.array([one, do.stats_of(_frames(rng, 50, 4)), do.stats_of(_frames(rng, 60, 4))]), 4, 1.0, 0.0)
    assert failed == 1 and np.isnan(ld_[0]) and np.isinf(m[0, 1:]).all() and np.isfinite(m[1, 2]) and m[1, 2] == m[2, 1]


def test_lance_williams_average_is_the_mean_of_the_pairwise_entries():
    rng = np.random.default_rng(7)
    n = 9
    d0 = rng.uniform(1.0, 2.0, (n, n))
    d0 = (d0 + d0.T) / 2
    r = do.ahc(d0, 0, threshold=np.inf)
    assert len(r["merge_i"]) == n - 1 and r["n_clusters"] == 1
    members = {c: [c] for c in range(n)}
    for i, j, d in zip(r["merge_i"], r["merge_j"], r["merge_d"]):
        want = np.mean([d0[a, b] for a in members[i] for b in members[j]])
        assert abs(d - want) <= 16 * do.EPS * want
        members[i] += members.pop(j)
    for link, pick in ((1, max), (2, min)):
        r = do.ahc(d0, link, threshold=np.inf)
        members = {c: [c] for c in range(n)}
        for i, j, d in zip(r["merge_i"], r["merge_j"], r["merge_d"]):
            assert d == pick(d0[a, b] for a in members[i] for b in members[j])
            members[i] += members.pop(j)
    # ties: the first pair in row-major order
    tie = np.ones((4, 4)) - np.eye(4)
    r = do.ahc(tie, 1, threshold=2.0)
    assert list(zip(r["merge_i"], r["merge_j"])) == [(0, 1), (0, 2), (0, 3)]
    assert do.ahc(tie, 0, threshold=1.0)["n_clusters"] == 4                   # d < threshold is strict
    assert do.ahc(tie, 0, threshold=1.0, k_max=2)["n_clusters"] == 2 and do.ahc(tie, 0, threshold=5.0, k_min=3)["n_clusters"] == 3
    assert do.ahc(np.full((3, 3), np.inf), 0, threshold=np.inf, k_max=1)["n_clusters"] == 3     # never a step at +inf


def test_cut_is_a_rerun(built_lib):
    from speaker_recognition_amd import diarize as dz
    rng = np.random.default_rng(8)
    d0 = rng.uniform(0.0, 10.0, (12, 12))
    d0 = (d0 + d0.T) / 2
    whole = do.ahc(d0, 0, threshold=np.inf)
    log = (whole["merge_i"], whole["merge_j"], whole["merge_d"])
    for thr in (-1.0, 2.0, 4.0, 6.0, 100.0):
        want = do.ahc(d0, 0, threshold=thr)
        assert np.array_equal(do.cut(12, *log, threshold=thr)[0], want["labels"])
        assert np.array_equal(dz.cut(log, 12, threshold=thr), want["labels"])
    for k in (1, 3, 12):
        want = do.ahc(d0, 0, threshold=-np.inf, k_min=k, k_max=k)
        assert want["n_clusters"] == k and np.array_equal(dz.cut(log, 12, k=k), want["labels"])
    assert dz.cut(([], [], []), 0, k=1).tolist() == [] and dz.cut(([], [], []), 3, threshold=0.0).tolist() == [0, 1, 2]
    with pytest.raises(ValueError):
        dz.cut(log, 12)
    from speaker_recognition_amd import _lib
    with pytest.raises(_lib.SRError, match="merge log"):
        dz.cut(([1, 1], [3, 3], [-1.0, -1.0]), 5, threshold=0.0)


def test_peak_rule_against_brute_force():
    rng = np.random.default_rng(9)
    for trial in range(200):
        nb = int(rng.integers(0, 14))
        m = int(rng.integers(1, 6))
        c = rng.integers(-2, 4, nb).astype(np.float64)                        # ties occur
        if trial % 5 == 0 and nb:
            c[rng.integers(0, nb)] = np.inf
        kept = do.peaks(c, m)
        for b in range(nb):
            near = [k for k in range(nb) if abs(k - b) < m]
            want = c[b] > 0 and c[b] == max(c[k] for k in near) and b == min(k for k in near if c[k] == c[b])
            assert kept[b] == want, (c, m, b)
        if m == 1:
            assert np.array_equal(kept, c > 0)
    seg = do.seg_stats(_frames(rng, 50, 2), 10)
    off, cl = do.init_clusters(seg, np.array([False, True, False, True]))
    assert off.tolist() == [0, 2, 4, 5] and np.array_equal(cl[0], seg[0] + seg[1]) and np.array_equal(cl[2], seg[4])


def test_plan_and_refusals(built_lib):
    from speaker_recognition_amd import _lib
    for D in range(1, 65):
        p = _lib.diar_plan(D, [1000, 37, 0])
        assert p["bucket"] == (16 if D <= 16 else 32 if D <= 32 else 48 if D <= 48 else 64) and p["stat_len"] == do.stat_len(D)
        assert p["entries_per_lane"] == -(-(p["stat_len"] - 1) // 256) <= 9 and p["n_seg"] == [10, 1, 0]
        assert (p["stats_lds"], p["change_lds"]) == (64 * D * 4, 2 * 8 * p["stat_len"])
    assert (p["max_dim"], p["max_init"], p["cadence"], p["edges"], p["bound"]) == (64, 4096, 16, [4, 64, 256], 1024 << 20)
    lengths = [3000, 100, 2500, 2900, 10, 3000]
    whole = _lib.diar_plan(39, lengths, L=10)
    assert whole["group_begin"] == [0, 6] and whole["bytes"] == sum(whole["rec_bytes"])
    big = max(whole["rec_bytes"])
    cut = _lib.diar_plan(39, lengths, L=10, scratch_bytes=big)
    assert cut["groups"] >= 3 and cut["group_begin"][0] == 0 and cut["group_begin"][-1] == 6
    for a, b in zip(cut["group_begin"], cut["group_begin"][1:]):
        assert a < b and sum(cut["rec_bytes"][a:b]) <= big
    with pytest.raises(_lib.SRError, match=r"\d+ bytes.*larger L"):
        _lib.diar_plan(39, lengths, L=10, scratch_bytes=big - 1)
    with pytest.raises(_lib.SRError, match="4096"):
        _lib.diar_plan(13, [5000], L=1, change="uniform")
    assert _lib.diar_plan(13, [5000], L=1, change="bic")["n_init_bound"] == [4096]
    for kw, pat in ((dict(D=65), "64"), (dict(D=0), "64"), (dict(L=0), "L >= 1"), (dict(change="peaks"), "change mode")):
        with pytest.raises(_lib.SRError, match=pat):
            _lib.diar_plan(**dict(dict(D=13, lengths=[100]), **kw))
    v = (C.c_int64 * 16)()
    assert _lib.lib().sr_diar_plan(13, 10, 1, None, 0, 0, v, 15, None, None) == -1 and "16 fields" in _lib.last_error()
    assert _lib.lib().sr_diar_plan(13, 10, 1, None, 0, 0, v, 16, None, None) == 0
    for n, L in ((0, 5), (1, 5), (4, 5), (5, 5), (6, 5), (12, 5), (10, 1)):
        assert _lib.diar_segments(n, L) == do.segments(n, L)
    # the options table: the same range as its siblings
    _lib.set_option("diar_scratch_mib", 1)
    _lib.set_option("diar_scratch_mib", 1 << 20)
    _lib.set_option("diar_scratch_mib", 1024)
    for bad in (0, (1 << 20) + 1):
        with pytest.raises(_lib.SRError, match="diar_scratch_mib"):
            _lib.set_option("diar_scratch_mib", bad)


def test_calls_refuse_before_the_device(built_lib):
    """Every refusal comes before the device is touched: they are raised on a machine without one."""
    from speaker_recognition_amd import _lib
    L = _lib.lib()
    nan, inf = float("nan"), float("inf")
    st = np.zeros((3, do.stat_len(2)))
    st[:, 0] = 5
    for kw, pat in ((dict(D=65), "64"), (dict(penalty=0.0), "lambda"), (dict(penalty=-1.0), "lambda"), (dict(penalty=nan), "lambda"),
                    (dict(penalty=inf), "lambda"), (dict(ridge=-1.0), "ridge"), (dict(ridge=nan), "ridge"), (dict(ridge=inf), "ridge")):
        args = dict(dict(stats=st, D=2, penalty=1.0, ridge=1e-3), **kw)
        if args["D"] == 65:
            args["stats"] = np.zeros((3, do.stat_len(65)))
        with pytest.raises(_lib.SRError, match=pat):
            _lib.diar_bic_matrix(**args)
    bad = st.copy()
    bad[1, 0] = 0
    with pytest.raises(_lib.SRError, match="at least one"):
        _lib.diar_bic_matrix(bad, 2)
    bad = st.copy()
    bad[2, 3] = nan
    with pytest.raises(_lib.SRError, match="non-finite"):
        _lib.diar_bic_matrix(bad, 2)
    d = np.ones((3, 3)) - np.eye(3)
    for kw, pat in ((dict(linkage=3), "linkage"), (dict(linkage=-1), "linkage"), (dict(threshold=nan), "threshold"), (dict(k_min=0), "k_min"),
                    (dict(k_min=3, k_max=2), "k_max"), (dict(k_max=-1), "k_max")):
        with pytest.raises(_lib.SRError, match=pat):
            _lib.ahc_matrix(d, **kw)
    for i, j, v, pat in ((0, 1, nan, "NaN"), (1, 0, nan, "NaN"), (0, 2, -inf, "-inf"), (1, 2, 0.5, "symmetric")):
        m = d.copy()
        m[i, j] = v
        with pytest.raises(_lib.SRError, match=pat):
            _lib.ahc_matrix(m)
    with pytest.raises(_lib.SRError, match="4096"):
        _lib.ahc_matrix(np.zeros((4097, 4097)))
    with pytest.raises(ValueError):
        _lib.ahc_matrix(np.zeros((3, 4)))
    z = None
    assert L.sr_diar_stats_batch(None, 10, 0, None, None) == -1 and "null" in _lib.last_error()
    assert L.sr_diar_cluster_batch(None, 10, 1, 2, 1.0, 1e-3, 0.0, 1, 0, 0, z, z, z, z, z, z, z, z, z) == -1 and "null" in _lib.last_error()
    assert L.sr_diar_cluster_pcm_batch(None, None, 0, 10, 1, 2, 1.0, 1e-3, 0.0, 1, 0, 0, z, z, z, z, z, z, z, z, z) == -1
    assert "null" in _lib.last_error()
    assert L.sr_ahc_matrix(3, None, 0, 0.0, 1, 0, z, z, z, z, z, z) == -1 and "null" in _lib.last_error()
    from speaker_recognition_amd.core import _diar_args
    assert _diar_args(100, "bic", 2, 1.0, 1e-3, 0.0, 1, 0) == (100, 1, 2, 1.0, 1e-3, 0.0, 1, 0)
    assert _diar_args(50, "uniform", 1, 2, 0, -1, 2, 4) == (50, 0, 1, 2.0, 0.0, -1.0, 2, 4)
    for bad in (dict(change="peaks"), dict(L=1.5), dict(half_width=True), dict(k_min=1.0), dict(k_max=None)):
        with pytest.raises(ValueError):
            _diar_args(**dict(dict(L=100, change="bic", half_width=2, penalty=1.0, ridge=1e-3, threshold=0.0, k_min=1, k_max=0), **bad))


def test_header_documents_the_calls(built_lib):
    header = open(os.path.join(ROOT, "include", "pygmm_hip.h")).read()
    for text in ("Who spoke when, nobody enrolled", "sr_diar_segments", "sr_diar_plan", "sr_diar_stats_batch", "sr_diar_bic_matrix",
                 "sr_diar_cluster_batch", "sr_diar_cluster_pcm_batch", "sr_ahc_matrix", "sr_diar_cut", "first in row-major order",
                 "diar_scratch_mib"):
        assert text in header
    from speaker_recognition_amd import _lib
    for name in ("sr_diar_plan", "sr_diar_stats_batch", "sr_diar_bic_matrix", "sr_diar_cluster_batch", "sr_diar_cluster_pcm_batch", "sr_ahc_matrix"):
        assert name in _lib.EXT_SYMBOLS


def test_diar_kernels_do_not_spill(built_lib):
    import test_abi_cpu
    res = test_abi_cpu._kernel_resources("diar")
    names = " ".join(res)
    for kernel in ("diar_stats_kernel", "diar_peak_kernel", "diar_gather_kernel", "ahc_argmin_kernel", "ahc_row_matrix_kernel",
                   "ahc_all_stopped_kernel"):
        assert kernel in names
    for kernel, count in (("diar_change_kernel", 4), ("diar_ld_kernel", 4), ("diar_pairs_kernel", 4), ("diar_row_kernel", 4),
                          ("ahc_merge_kernel", 5)):
        assert sum(kernel in n for n in res) == count, kernel           # a bucket each: 16, 32, 48, 64 (+ the matrix mode's merge)
    for name, r in res.items():
        assert r["scratch"] == 0, (name, r)


def test_frame_segments_and_rttm():
    from speaker_recognition_amd import diarize as dz, timeline as tl
    # 5 base segments of 10 frames, the last reaching to frame 57; runs [0, 2), [2, 3), [3, 5)
    assert dz.frame_ranges([0, 2, 3, 5], 57, 10).tolist() == [[0, 20], [20, 30], [30, 57]]
    segs = dz.frame_segments([0, 2, 3, 5], [0, 1, 0], 57, 10, 0.5)
    assert segs == [(0.0, 10.0, 0), (10.0, 15.0, 1), (15.0, 28.5, 0)]
    assert dz.frame_segments([0, 2, 3, 5], [0, 0, 1], 57, 10, 0.5) == [(0.0, 15.0, 0), (15.0, 28.5, 1)]      # runs merge
    assert dz.frame_segments([0, 1], [0], 7, 10, 0.01) == [(0.0, 0.07, 0)]                                    # one short segment
    assert dz.frame_segments([0], [], 0, 10, 0.01) == []
    for n, L in ((240, 7), (100, 1), (37, 10)):
        ns = max(n // L, 1)
        off = list(range(ns + 1))
        segs = dz.frame_segments(off, np.arange(ns) % 3, n, L, 0.016)
        assert segs[0][0] == 0.0 and abs(segs[-1][1] - n * 0.016) < 1e-12
        assert all(a[1] == b[0] and a[1] > a[0] for a, b in zip(segs, segs[1:]))
    with pytest.raises(ValueError):
        dz.frame_segments([0, 2, 3, 5], [0, 1], 57, 10, 0.5)
    with pytest.raises(ValueError):
        dz.frame_segments([0, 2, 2, 5], [0, 1, 0], 57, 10, 0.5)
    named = [(a, b, "spk%d" % lab) for a, b, lab in dz.frame_segments([0, 2, 3, 5], [0, 1, 0], 57, 10, 0.5)]
    assert tl.to_rttm(named, recording_id="mtg") == ("SPEAKER mtg 1 0.000 10.000 <NA> <NA> spk0 <NA> <NA>\n"
                                                      "SPEAKER mtg 1 10.000 5.000 <NA> <NA> spk1 <NA> <NA>\n"
                                                      "SPEAKER mtg 1 15.000 13.500 <NA> <NA> spk0 <NA> <NA>\n")
    for bad in (dict(k=0), dict(k=2, k_max=3), dict(k=1.5), dict(k_max=True)):
        with pytest.raises(ValueError):
            dz._stop_args(**dict(dict(k=None, k_max=None), **bad))
    assert dz._stop_args(None, None) == (1, 0) and dz._stop_args(3, None) == (3, 3) and dz._stop_args(None, 4) == (1, 4)
    with pytest.raises(ValueError, match="linkage"):
        dz.ahc(np.zeros((2, 2)), linkage="ward")


def test_interface_and_cli_arguments(built_lib):
    from speaker_recognition_amd import cli
    from speaker_recognition_amd.interface import ModelInterface
    m = ModelInterface(verbose=False)
    assert m._diarize_args(1.0, "bic", 1.0, None, None, 8) == (0.016, 62, 1, 0)
    assert m._diarize_args(0.5, "uniform", 2, 3, None, 4) == (0.016, 31, 3, 3)
    assert ModelInterface(verbose=False, feature_kwargs=dict(win_shift_ms=10))._diarize_args(1.0, "bic", 1.0, None, 5, 8) == (0.01, 100, 1, 5)
    for bad in (dict(segment_s=0), dict(segment_s="1"), dict(change="peaks"), dict(penalty=0), dict(penalty=float("nan")), dict(n_speakers=0),
                dict(max_speakers=1.5), dict(n_speakers=2, max_speakers=3), dict(gmm_order=0)):
        kw = dict(dict(segment_s=1.0, change="bic", penalty=1.0, n_speakers=None, max_speakers=None, gmm_order=8), **bad)
        with pytest.raises(ValueError):
            m._diarize_args(**kw)
    pcm = np.zeros(16000, np.int16)
    with pytest.raises(ValueError, match="segment_s"):
        m.diarize(16000, pcm, segment_s=-1)
    with pytest.raises(ValueError, match="timeline"):
        m.diarize(16000, pcm, smooth="hold")
    with pytest.raises(ValueError, match="hop_s"):
        m.diarize(16000, pcm, hop_s=0)
    a = cli.get_args(["-t", "diarize", "-i", "x"])
    assert (a.task, a.model, a.rttm, a.speakers, a.max_speakers, a.penalty) == ("diarize", None, None, None, None, 1.0)
    a = cli.get_args(["-t", "diarize", "-i", "x", "--rttm", "o.rttm", "--speakers", "3", "--penalty", "2.5"])
    assert (a.rttm, a.speakers, a.penalty) == ("o.rttm", 3, 2.5)
    assert cli.get_args(["-t", "diarize", "-i", "x", "--max-speakers", "4"]).max_speakers == 4
    for bad in (["--speakers", "2", "--max-speakers", "3"], ["--speakers", "0"], ["--penalty", "0"]):
        with pytest.raises(SystemExit):
            cli.get_args(["-t", "diarize", "-i", "x"] + bad)
    with pytest.raises(SystemExit):
        cli.get_args(["-t", "predict", "-i", "x"])                          # every other task still needs -m
    assert cli.get_args(["-t", "predict", "-i", "x", "-m", "y"]).model == "y"


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_diar_plan_under_asan_ubsan(tmp_path):
    """csrc/diar_plan.cpp swept over dimensions, segment lengths, batches and bounds by a stand-alone program
    (tests/host/diar_checks.cpp) built with AddressSanitizer + UBSan: host code only, no GPU, nothing loaded into Python."""
    exe = str(tmp_path / "diar_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "host", "diar_checks.cpp"), os.path.join(CSRC, "diar_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "diar checks ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
