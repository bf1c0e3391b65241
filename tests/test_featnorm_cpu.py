"""CPU: the short-time feature normalisation's checker checks itself (tests/featnorm_oracle.py against the properties of feature
warping and sliding CMN), the host instance of the quantile function (sr_norm_quantile), the launch decisions (sr_feature_norm_plan,
csrc/featnorm_plan.cpp -- also under the host sanitizers, tests/host/featnorm_checks.cpp), the kernels' register budgets, and the
Python surface that needs no device: the interface's setting, pickles, the command line."""
import os
import shutil
import subprocess
import sys
from statistics import NormalDist

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import featnorm_oracle as fo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")


def _bits(a):
    return (np.ascontiguousarray(a, np.float32) + np.float32(0.0)).view(np.int32)        # (the middle rank's zero carries no sign)


def test_oracle_properties():
    rng = np.random.default_rng(5)
    for T, W in ((700, 301), (200, 8), (40, 301), (97, 3), (64, 2)):
        X = rng.normal(3.0, 2.0, (T, 3)).astype(np.float32)
        X[T // 3:T // 3 + 5, 1] = X[T // 3, 1]                      # ties
        out, r, n = fo.warp(X, W)
        assert n == 0 and r.min() >= 0 and r.max() <= 2 * min(W, T) - 2
        neg, rn, _ = fo.warp(-X, W)
        assert np.array_equal(_bits(neg), _bits(-out))              # antisymmetry, to the bit
        assert np.array_equal(rn, 2 * min(W, T) - 2 - r)
        mono, rm, _ = fo.warp(np.exp(X.astype(np.float64) / 4).astype(np.float32)[:, [0, 2]], W)       # a strictly increasing map
        assert np.array_equal(rm, r[:, [0, 2]]) and np.array_equal(_bits(mono), _bits(out[:, [0, 2]]))
    # an untied utterance no longer than the window: a permutation of the quantile grid
    T = 50
    X = rng.permutation(T).astype(np.float32)[:, None]
    out, r, _ = fo.warp(X, 301)
    grid = np.array([NormalDist().inv_cdf((2 * k + 1) / (2 * T)) for k in range(T)])
    assert np.array_equal(np.sort(r[:, 0]), 2 * np.arange(T))
    assert np.max(np.abs(np.sort(out[:, 0].astype(np.float64)) - grid)) <= 2.0 ** -23 * np.abs(grid).max()
    # a constant stretch longer than the window: exactly 0 in its interior (the strictly-less rule would give a large negative value)
    X = rng.normal(0, 1, (60, 1)).astype(np.float32)
    X[10:40] = 1.25
    out, r, _ = fo.warp(X, 8)
    assert np.all(out[14:36] == 0.0) and np.all(r[14:36] == 7)
    cm, deg = fo.sliding(X, 8, True)
    assert np.all(cm[14:36] == 0.0) and deg == 30 - 8 + 1           # every window inside the stretch, counted
    # cmn of an untied window sums to about 0
    X = rng.normal(1000.0, 0.5, (9, 2)).astype(np.float32)
    cmn, deg = fo.sliding(X, 301, False)
    assert deg == 0 and np.all(np.abs(cmn.astype(np.float64).sum(axis=0)) < 9 * 2.0 ** -24 * 4)
    # NaN: rank -1, NaN out, counted; a NaN neighbour is neither less nor equal
    X = np.arange(10, dtype=np.float32)[:, None].copy()
    X[4] = np.nan
    out, r, n = fo.warp(X, 301)
    assert n == 1 and r[4, 0] == -1 and np.isnan(out[4, 0]) and r[3, 0] == 6 and r[5, 0] == 8
    assert fo.warp(np.zeros((0, 2), np.float32), 5)[0].shape == (0, 2)
    assert np.array_equal(fo.window_starts(10, 4)[0], [0, 0, 0, 1, 2, 3, 4, 5, 6, 6])
    assert np.array_equal(fo.window_starts(5, 3)[0], [0, 0, 1, 2, 2])


def test_norm_quantile_matches_the_standard_library(built_lib):
    from speaker_recognition_amd import _lib
    q = NormalDist().inv_cdf
    assert _lib.norm_quantile(0.5) == 0.0
    worst = 0.0
    for N in (1, 2, 3, 301, 1024):
        for k in range(2 * N - 1):
            p = (k + 1) / (2 * N)
            got, want = _lib.norm_quantile(p), q(p)
            if want == 0.0:
                assert got == 0.0
            else:
                worst = max(worst, abs(got - want) / abs(want))
            mirror = _lib.norm_quantile((2 * N - 1 - k) / (2 * N))
            # odd symmetry.  The two arguments are each rounded to float64 (half an ulp of a value below 1: 2^-54), and the
            # quantile's slope is sqrt(2 pi) exp(q^2 / 2): that much of the difference is the arguments', the rest the function's
            slack = 2.0 ** -53 * (2 * np.pi) ** 0.5 * np.exp(got * got / 2)
            assert abs(mirror + got) <= 4e-15 * abs(got) + slack
            if N == 1024:
                assert mirror == -got                               # p and 1 - p both exact: to the bit
    print("sr_norm_quantile against NormalDist().inv_cdf: worst relative difference %.3g" % worst)
    assert worst <= 4e-15
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert np.isnan(_lib.norm_quantile(bad))


def test_plan_sweep_and_refusals(built_lib):
    from speaker_recognition_amd import _lib
    try:
        for tile in (0, 64):
            _lib.set_option("norm_tile", tile)
            F = tile or 256
            for mode in _lib.FEATURE_NORM_MODES:
                for W in (2, 3, 8, 301, 1024):
                    for dim in (1, 13, 39, 65):
                        for T in (0, 1, W - 1, W, W + 1, F - 1, F, F + 1, 2 * F + W + 3, 10 ** 7):
                            p = _lib.feature_norm_plan(mode, W, dim, T)
                            span = max(1, min(F + min(W, T) - 1, T))
                            assert (p["F"], p["span"], p["tiles"], p["workgroup"], p["max_window"]) == (F, span, -(-T // F), 256, 1024)
                            assert p["stride"] >= span and p["stride"] % 8 == 4 and p["stride"] < span + 8
                            assert p["cols"] * p["stride"] * 4 == p["lds"] <= 65536 and p["cols"] <= min(dim, 64)
                            assert p["passes"] == -(-dim // p["cols"]) == -(-dim // min(dim, 64, 16384 // p["stride"]))
                            assert p["grid"] == max(1, min(p["tiles"], 256 * 32))
                            assert p["table"] == int(mode == "warp" and T >= W and T * dim >= 4 * (2 * W - 1))
                            assert p["table_len"] == (2 * W - 1 if p["table"] else 0)
        _lib.set_option("norm_tile", 0)
        assert _lib.feature_norm_plan("warp", 301, 39, 10000)["cols"] == 20          # 39 columns: two even passes
        for kw, pat in ((dict(mode="median"), "mode"), (dict(mode=2), "mode"), (dict(window=1), "window"), (dict(window=1025), "window"),
                        (dict(dim=0), "dim"), (dict(dim=-3), "dim"), (dict(max_frames=-1), "frame")):
            with pytest.raises(_lib.SRError, match=pat):
                _lib.feature_norm_plan(**kw)
        for bad in (-1, -64, 1, 63, 100, 1088):
            with pytest.raises(_lib.SRError, match="norm_tile"):
                _lib.set_option("norm_tile", bad)
        import ctypes as C
        v = (C.c_int32 * 12)()
        assert _lib.lib().sr_feature_norm_plan(0, 301, 39, 100, 256, v, 11) == -1 and "12 fields" in _lib.last_error()
        assert _lib.lib().sr_feature_norm_plan(0, 301, 39, 100, 256, None, 12) == -1
        assert _lib.lib().sr_feature_norm_batch(None, 0, 301, None, None) is None and "null" in _lib.last_error()
    finally:
        _lib.set_option("norm_tile", 0)


def test_header_documents_the_stage(built_lib):
    header = open(os.path.join(ROOT, "include", "pygmm_hip.h")).read()
    for text in ("sr_feature_norm_batch", "sr_feature_norm_plan", "sr_norm_quantile", '"norm_tile"'):
        assert text in header


def test_featnorm_kernels_do_not_spill(built_lib):
    import test_abi_cpu
    res = test_abi_cpu._kernel_resources("featnorm")
    names = " ".join(res)
    assert sum("featnorm_kernel" in n for n in res) == 3                # warp, cmn, cmvn
    for kernel in ("featnorm_table_kernel", "featnorm_count_kernel"):
        assert kernel in names
    for name, r in res.items():
        assert r["scratch"] == 0, (name, r)
        if "featnorm_kernel" in name:
            assert r["occupancy"] >= 3, (name, r)                       # what 44 KiB of LDS per workgroup admit at the headline shape


def test_interface_setting_and_old_pickles(built_lib, tmp_path):
    from speaker_recognition_amd.interface import ModelInterface
    assert ModelInterface(verbose=False)._norm_setting() is None
    assert ModelInterface(verbose=False, feature_norm="warp")._norm_setting() == ("warp", 301)
    assert ModelInterface(verbose=False, feature_norm="cmn")._norm_setting() == ("cmn", 301)
    assert ModelInterface(verbose=False, feature_norm=dict(mode="cmvn", window=150))._norm_setting() == ("cmvn", 150)
    assert ModelInterface(verbose=False, feature_norm=dict(mode="warp"))._norm_setting() == ("warp", 301)
    for bad in ("median", True, 3, dict(window=100), dict(mode="warp", width=3), dict(mode="warp", window=1), dict(mode="warp", window=1025),
                dict(mode="warp", window=2.5), ("warp", 301)):
        with pytest.raises(ValueError):
            ModelInterface(verbose=False, feature_norm=bad)
    # a model pickled before the setting existed: no such attribute -- it loads and behaves as feature_norm=None
    m = ModelInterface(verbose=False)
    del m.__dict__["feature_norm"]
    f = str(tmp_path / "old.out")
    m.dump(f)
    old = ModelInterface.load(f)
    assert "feature_norm" not in old.__dict__ and old._norm_setting() is None
    f2 = str(tmp_path / "new.out")
    ModelInterface(verbose=False, feature_norm=dict(mode="cmvn", window=200)).dump(f2)
    new = ModelInterface.load(f2)
    assert new.feature_norm == dict(mode="cmvn", window=200) and new._norm_setting() == ("cmvn", 200)


def test_python_layer_refuses_without_a_device(built_lib):
    from speaker_recognition_amd.core import MfccExtractor
    from speaker_recognition_amd.feature import norm
    assert norm.normalise_many([], "warp") == []
    for bad in (dict(mode="median"), dict(window=1), dict(window=1025), dict(window=3.0)):
        with pytest.raises(ValueError):
            norm.normalise_many([np.zeros((5, 2))], **bad)
    with pytest.raises(ValueError):
        norm.feature_warp(np.zeros(5))
    with pytest.raises(ValueError):
        norm.normalise_many([np.zeros((5, 2)), np.zeros((5, 3))])
    with pytest.raises(ValueError):
        MfccExtractor(16000).extract_batch(None, norm="median")


def test_cli_parses_feature_norm(built_lib):
    from speaker_recognition_amd import cli
    base = ["-i", "x", "-m", "y"]
    for task in ("enroll", "predict"):
        a = cli.get_args(["-t", task] + base)
        assert a.feature_norm is None and a.norm_window is None and cli._feature_norm_setting(a) is None
        a = cli.get_args(["-t", task] + base + ["--feature-norm", "warp"])
        assert cli._feature_norm_setting(a) == "warp"
        a = cli.get_args(["-t", task] + base + ["--feature-norm", "cmvn", "--norm-window", "150"])
        assert cli._feature_norm_setting(a) == dict(mode="cmvn", window=150)
        assert cli._feature_norm_setting(cli.get_args(["-t", task] + base + ["--norm-window", "150"])) is None
    with pytest.raises(SystemExit):
        cli.get_args(["-t", "enroll"] + base + ["--feature-norm", "median"])
    m = cli._make_interface(cli.get_args(["-t", "enroll"] + base + ["--feature-norm", "cmn", "--norm-window", "64"]))
    assert m._norm_setting() == ("cmn", 64)
    assert cli._make_interface(cli.get_args(["-t", "enroll"] + base))._norm_setting() is None
    assert cli._make_interface(None)._norm_setting() is None
    with pytest.raises(ValueError):
        cli._make_interface(cli.get_args(["-t", "enroll"] + base + ["--feature-norm", "cmn", "--norm-window", "1"]))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_featnorm_plan_under_asan_ubsan(tmp_path):
    """csrc/featnorm_plan.cpp swept over modes, windows, widths, lengths and tile options by a stand-alone program
    (tests/host/featnorm_checks.cpp) built with AddressSanitizer + UBSan: host code only, no GPU, nothing loaded into Python."""
    exe = str(tmp_path / "featnorm_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "host", "featnorm_checks.cpp"), os.path.join(CSRC, "featnorm_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "featnorm checks ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
