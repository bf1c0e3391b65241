"""CPU side of top-C Gaussian selection (csrc/gmm_topc.hip, csrc/topc_plan.cpp): the numpy restatement (tests/topc_cases.py)
against plain loops, the launch decisions (sr_topc_plan -- also under the host sanitizers, tests/host/topc_checks.cpp), the symbols,
the refusals that must not need a device, the kernels' resource records, and the Python surface's defaults."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topc_cases as tc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")
NEW = ["sr_score_batch_set_topc", "sr_predict_pcm_batch_topc", "sr_topc_plan"]


def test_restatement_agrees_with_plain_loops():
    models = tc.make_models(5, 3, 3, 1, 42)
    utts = tc.make_utts(models, 1, (4, 0, 3), 42)
    X = np.concatenate(utts)
    X[2] += 60.0                                        # one frame beyond the clamp
    for C_ in (1, 2, 5):
        for clamp in (True, False):
            ll, sel = tc.frame_ll(X, models, 1, C_, clamp_compat=clamp)
            want, picks = tc.brute_force(X, models, 1, C_, clamp_compat=clamp)
            assert np.array_equal(sel, picks)
            assert np.allclose(ll, want, rtol=1e-12, atol=1e-12)
    assert tc.frame_ll(X, models, 1, 2)[0][0, 2] == tc.LN_1E_15 and tc.frame_ll(X, models, 1, 2, clamp_compat=False)[0][0, 2] < tc.LN_DBL_MIN
    # ties go to the lower index, whatever their position; the order is descending
    t = np.array([[1.0, 3.0, 3.0, 2.0, 3.0], [0.0, 0.0, 0.0, 0.0, 0.0]])
    assert tc.select(t, 3).tolist() == [[1, 2, 4], [0, 1, 2]] and tc.select(t, 5)[0].tolist() == [1, 2, 4, 3, 0]
    off = tc.offsets_of(utts)
    s = tc.sums(tc.frame_ll(X, models, 1, 2)[0], off)
    assert s.shape == (3, 3) and np.all(s[1] == 0.0)
    assert tc.argmax_first(s, np.diff(off)).tolist()[1] == -1
    # C = K is the full log-sum-exp of every model
    full = np.stack([tc.lse(tc.terms(X, m)) for m in models])
    assert np.allclose(tc.frame_ll(X, models, 1, 5, clamp_compat=False)[0], full, rtol=1e-12, atol=1e-12)


def test_symbols_exported_and_declared(built_lib):
    from speaker_recognition_amd import _lib
    header = open(os.path.join(ROOT, "include", "pygmm_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), "lib/pygmm.so does not export %s" % name
        assert re.search(r"\bint %s\(" % name, header), "%s is not declared in include/pygmm_hip.h" % name
        assert name in _lib.EXT_SYMBOLS
    assert "partial-product re-evaluation" in header and "topc_scratch_mib" in header
    for name in ("sr_score_batch_set", "sr_predict_pcm_batch", "sr_score_batch_set_open", "sr_open_set_decide"):
        assert hasattr(raw, name)                      # the siblings stay


def test_plan_chunks_respect_the_bound_and_cover_every_frame(built_lib):
    from speaker_recognition_amd import _lib
    for S in (1, 64, 65, 1001):
        for K, D, C_ in ((512, 39, 5), (2048, 39, 5), (33, 13, 1), (64, 40, 9), (64, 64, 64)):
            row = C_ * S * 4 + C_ * 8 + 4 + (K * 4 if C_ > 8 else 0)
            for n in (0, 1, 1000, 19200, 1000000, 12500000):
                for bound in (row, 3 * row + 1, 1 << 20, 1 << 30):
                    p = _lib.topc_plan(K, D, S, C_, n, bound, 256)
                    assert p["row_bytes"] == row and p["tp"] == (16 if D <= 16 else 40 if D <= 40 else 64)
                    assert p["cr"] == (1 if C_ == 1 else 5 if C_ <= 5 else 8 if C_ <= 8 else 0)
                    assert p["eval_waves"] == min(4, -(-S // 64)) and p["eval_grid_y"] == -(-S // (64 * p["eval_waves"]))
                    if n == 0:
                        assert p["chunk"] == 0 and p["n_chunks"] == 0
                        continue
                    assert 1 <= p["chunk"] <= n and p["chunk"] * row <= bound                    # the bound holds
                    assert p["chunk"] == min(n, bound // row, ((1 << 31) - 1 - 256) // C_)
                    assert (p["n_chunks"] - 1) * p["chunk"] < n <= p["n_chunks"] * p["chunk"]    # every frame exactly once
                    assert p["eval_grid_x"] == -(-p["chunk"] * C_ // p["run"]) + K and p["run"] in (64, 256)
                    assert p["select_grid"] == -(-p["chunk"] // 256) and p["route_grid"] == -(-p["chunk"] * C_ // 256)
            with pytest.raises(_lib.SRError, match="below one frame's row"):                    # less than one frame's row: refused
                _lib.topc_plan(512, 39, S, 5, 1000, 5 * S * 4 + 43, 256)
    p = _lib.topc_plan(512, 39, 201, 5, 10_000_000)                                             # the headline shape, default bound
    assert p["chunk"] == (1 << 30) // (5 * 201 * 4 + 44) and p["n_chunks"] == -(-10_000_000 // p["chunk"]) and p["run"] == 256
    assert _lib.topc_plan(512, 39, 201, 5, 19200)["run"] == 64                                  # a small batch is cut finer
    for bad in (0, (1 << 20) + 1):
        with pytest.raises(_lib.SRError, match="topc_scratch_mib"):
            _lib.set_option("topc_scratch_mib", bad)
    _lib.set_option("topc_scratch_mib", 1024)


def test_refusals_need_no_device(built_lib):
    """The checks fail on their arguments alone: the message names the argument and the remedy, never the device -- on a machine
    without a GPU a call that had reached the device would say "no HIP device" instead.  (A set or a batch cannot exist without
    a device: the entry points apply csrc/topc_plan.cpp's topc_check, which tests/host/topc_checks.cpp drives case by case, and
    tests/test_gpu_topc.py sees the same texts through the entry points.)"""
    from speaker_recognition_amd import _lib
    L = built_lib
    assert L.sr_score_batch_set_topc(None, None, 0, 1, None, None, None, None, 0) == -1
    assert "null argument" in _lib.last_error() and "HIP" not in _lib.last_error()
    assert L.sr_predict_pcm_batch_topc(None, None, None, 0, 0, 1, None, None, 0) == -1
    assert "null argument" in _lib.last_error() and "HIP" not in _lib.last_error()
    for kw, pat in ((dict(top_c=0), r"top_c 0 outside \[1, 8\]"), (dict(top_c=9), r"top_c 9 outside \[1, 8\]"), (dict(D=65), "64 dimensions"),
                    (dict(S=0), "empty model set"), (dict(n_frames=-1), "negative frame count"),
                    (dict(K=8193, top_c=9), "at most 8192 mixtures")):
        args = dict(K=8, D=13, S=3, top_c=2, n_frames=100)
        args.update(kw)
        with pytest.raises(_lib.SRError, match=pat) as e:
            _lib.topc_plan(**args)
        assert "HIP" not in str(e.value)
    out = (C.c_int32 * 16)()
    assert L.sr_topc_plan(8, 13, 3, 2, 100, 1 << 20, 256, out, 15) == -1 and "16 fields" in _lib.last_error()
    assert L.sr_topc_plan(8, 13, 3, 2, 100, 1 << 20, 256, None, 16) == -1 and "null argument" in _lib.last_error()
    if _lib.device_count() == 0:                       # and a call that needs the device says what is missing: no CPU path
        assert L.sr_topc_plan(8, 13, 3, 2, 100, 1 << 20, 0, out, 16) == -1 and "no HIP device" in _lib.last_error()
        from speaker_recognition_amd import synth
        from speaker_recognition_amd.core import ModelSet
        from speaker_recognition_amd.pygmm import GMM
        with pytest.raises(_lib.SRError, match="no HIP device"):
            ModelSet([GMM.from_arrays(*synth.synth_gmm(4, 3, 1))]).score_topc(None, 0, 1)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_topc_plan_under_asan_ubsan(tmp_path):
    """csrc/topc_plan.cpp -- every refusal's text and the plan swept over shapes, lengths, bounds and device sizes -- by a
    stand-alone program (tests/host/topc_checks.cpp) built with AddressSanitizer + UBSan: host code only, no GPU, nothing loaded
    into Python."""
    exe = str(tmp_path / "topc_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "host", "topc_checks.cpp"), os.path.join(CSRC, "topc_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "topc checks ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_topc_kernels_do_not_spill(built_lib):
    import test_abi_cpu
    res = test_abi_cpu._kernel_resources("gmm_topc")
    names = " ".join(res)
    for kernel in ("topc_gather_bg_kernel", "topc_select_kernel", "topc_rank_kernel", "topc_hist_kernel", "topc_scan_kernel",
                   "topc_scatter_kernel", "topc_eval_kernel", "topc_combine_kernel"):
        assert kernel in names
    assert sum("topc_select_kernel" in n for n in res) == 12 and sum("topc_eval_kernel" in n for n in res) == 3
    for name, r in res.items():
        assert r["scratch"] == 0, (name, r)


class _Recorder:
    def __init__(self):
        self.calls = []

    def score(self, batch):
        self.calls.append("score")
        return np.zeros((2, 2)), np.array([1, 0], np.int32)

    def score_open(self, batch, bg, thr):
        self.calls.append("score_open")
        return np.zeros((2, 3)), np.array([2, -1], np.int32), np.zeros(2)

    def score_topc(self, *a, **k):
        raise AssertionError("top_c=None reached the top-C entry point")


def test_python_defaults_do_not_touch_the_new_entry_points(built_lib, monkeypatch):
    from speaker_recognition_amd import cli, gmmset
    from speaker_recognition_amd.interface import ModelInterface
    monkeypatch.setattr(gmmset.Batch, "from_features", staticmethod(lambda utts: object()))
    monkeypatch.setattr(gmmset._lib, "gpu_runtime_lost", lambda: False)
    rec = _Recorder()
    gs = gmmset.GMMSet(reject_threshold=0.5)
    gs.ubm = object()
    gs.gmms, gs.y = [object(), object()], ["a", "b"]
    monkeypatch.setattr(gs, "_model_set", lambda: rec)
    monkeypatch.setattr(gs, "_open_model_set", lambda: rec)
    X = [np.zeros((3, 2)), np.zeros((4, 2))]
    assert gs.predict(X) == ["b", "a"] and gs.predict(X, top_c=None) == ["b", "a"]
    assert gs.predict_with_reject_batch(X) == ["b", None] and gs.predict_with_reject_batch(X, top_c=None) == ["b", None]
    assert rec.calls == ["score", "score", "score_open", "score_open"]
    with pytest.raises(AssertionError, match="top_c=None reached"):
        gs.predict(X, top_c=5)                                                    # (the recorder does see a top_c call)
    # without a UBM: the reference's own assertion text
    bare = gmmset.GMMSet()
    for call in (bare.predict, bare.predict_with_reject_batch):
        with pytest.raises(AssertionError, match="UBM must be given prior to conduct reject prediction."):
            call(X, top_c=5)
    # the interface and the command line: off by default, refused for full covariance and without a UBM
    assert cli.get_args(["-t", "predict", "-i", "x", "-m", "y"]).top_c is None
    assert cli.get_args(["-t", "predict", "-i", "x", "-m", "y", "--top-c", "5"]).top_c == 5
    m = ModelInterface(verbose=False)
    with pytest.raises(ValueError, match="enrolled from a UBM"):
        m.predict(8000, np.zeros(8000, np.int16), top_c=5)
    with pytest.raises(ValueError, match="full-covariance"):
        ModelInterface(verbose=False, covariance_type="full").predict_many_topc([(8000, np.zeros(8000, np.int16))], 5)


def test_cli_refuses_top_c_without_a_ubm(built_lib, tmp_path, capsys):
    from speaker_recognition_amd import cli
    from speaker_recognition_amd.interface import ModelInterface
    for kind, pat in (("diag", "enrolled from a UBM"), ("full", "full-covariance")):
        model = str(tmp_path / ("m_%s.out" % kind))
        ModelInterface(verbose=False, covariance_type=kind).dump(model)
        with pytest.raises(SystemExit):
            cli.task_predict(str(tmp_path / "*.wav"), model, 1, None, False, 5)
        assert pat in capsys.readouterr().out
