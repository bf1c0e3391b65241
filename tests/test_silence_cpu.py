"""CPU: the silence removal's checker checks itself (tests/silence_oracle.py against the properties of the reference's
src/filters/silence.py:11-50), the launch decisions (sr_silence_plan, csrc/silence_plan.cpp -- also under the host sanitizers,
tests/host/silence_checks.cpp), and the Python surface that needs no device: types, pickles, the command line."""
import math
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import silence_oracle as so  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")


def test_oracle_properties():
    z = np.zeros(1234, np.int16)
    assert np.array_equal(so.remove_silence(8000, z), z)                    # A = 0: nothing is below 0
    t = so.tie_signal()
    assert len(t) == 2400 and len(so.remove_silence(8000, t, perc=0.5)) == 2400       # 30 frames, the quiet ones ON the threshold
    assert len(so.remove_silence(8000, t, perc=0.5000001)) == 800
    assert len(so.remove_silence(8000, np.full(999, 7, np.int16), perc=2.0)) == 0
    # unsigned input: 128 on the way in, 127 on the way out (Python 2's integer division in the reference)
    flat = np.full(500, 200, np.uint8)
    out = so.remove_silence(8000, flat)
    assert out.dtype == np.uint8 and np.array_equal(out, flat - 1)
    u = np.array([128, 127, 129, 0, 255] * 64, np.uint8)
    assert np.array_equal(so.remove_silence(8000, u, perc=0.0), (u.astype(np.int64) - 1).astype(np.uint8))
    for bad in (np.zeros(10, np.float32), np.zeros(10)):
        with pytest.raises(ValueError):
            so.remove_silence(8000, bad)                                    # np.iinfo refuses floats, as in the reference
    # both branches of the walk on the envelope signal, at the three rates of the device tests
    for fs in (8000, 16000, 22050):
        x = so.envelope_noise(20011, 0)
        kept = so.remove_silence(fs, x)
        assert kept.dtype == np.int16 and 0 < len(kept) < len(x)
    # every visited frame start is a multiple of gcd(L, S): the kept samples come in runs cut from such starts
    L, S = so.frame_params(22050)
    assert (L, S, math.gcd(L, S)) == (441, 220, 1)


DEFAULTS = {8000: (160, 80, 80), 11025: (220, 110, 110), 16000: (320, 160, 160), 22050: (441, 220, 1), 44100: (882, 441, 441)}


def test_plan_at_the_defaults(built_lib):
    from speaker_recognition_amd import _lib
    try:
        for block in (0, 8, 1000):
            _lib.set_option("silence_block", block)
            for fs, (L, S, g) in DEFAULTS.items():
                for n in (1, 20011, 30 * fs):
                    p = _lib.silence_plan(fs, max_samples=n)
                    assert (p["L"], p["S"], p["g"]) == (L, S, g)
                    positions = -(-n // g)
                    assert p["positions"] == positions
                    assert p["E"] == min(max(L, S) // g, positions)
                    assert p["B"] == (block or max(256, 4 * p["E"], -(-positions // 2048)))
                    assert p["blocks"] == -(-positions // p["B"])
                    assert p["variant"] == (1 if p["E"] > 256 else 0)
                    assert p["blocks_per_wg"] == (1 if p["variant"] else 256 // p["E"])
                    assert p["list_cap"] == -(-p["B"] // (S // g))
                    assert p["grid"] == -(-p["blocks"] // p["blocks_per_wg"])
        _lib.set_option("silence_block", 0)
        assert _lib.silence_plan(22050, max_samples=30 * 22050)["E"] == 441           # g = 1 is a default-parameter case
        hour = _lib.silence_plan(16000, max_samples=10 * 3600 * 16000)                # a long recording: its chain stays short
        assert hour["B"] == -(-hour["positions"] // 2048) > 256 and hour["blocks"] <= 2048
        assert _lib.silence_plan(1000, 1.0, 0.007, 20011)["E"] == 1000                # above a workgroup: variant 1
        assert _lib.silence_plan(1000, 1.0, 0.007, 20011)["variant"] == 1
        with pytest.raises(_lib.SRError, match="frame_shift"):
            _lib.silence_plan(16000, 0.02, 0.00001, 1000)                             # S = 0
        with pytest.raises(_lib.SRError, match="frame_duration"):
            _lib.silence_plan(16000, 0.00001, 0.01, 1000)                             # L = 0
        with pytest.raises(_lib.SRError):
            _lib.silence_plan(16000, max_samples=0)
        for bad in (-1, (1 << 30) + 1):
            with pytest.raises(_lib.SRError, match="silence_block"):
                _lib.set_option("silence_block", bad)
    finally:
        _lib.set_option("silence_block", 0)


def test_silence_kernels_do_not_spill(built_lib):
    import test_abi_cpu
    res = test_abi_cpu._kernel_resources("silence")
    names = " ".join(res)
    for kernel in ("silence_chunk_kernel", "silence_scan_tiles_kernel", "silence_scan_totals_kernel", "silence_scan_add_kernel",
                   "silence_maps_kernel", "silence_chain_kernel", "silence_mark_kernel", "silence_offsets_kernel", "silence_copy_kernel"):
        assert kernel in names
    for name, r in res.items():
        assert r["scratch"] == 0, (name, r)


def test_python_layer_refuses_other_types_without_a_device(built_lib):
    from speaker_recognition_amd import filters
    assert filters.remove_silence is filters.silence.remove_silence and "remove_silence_many" in filters.__all__
    for bad in (np.zeros(100, np.float32), np.zeros(100), np.zeros(100, np.int32), np.zeros(100, np.uint16), np.zeros(100, np.int64)):
        with pytest.raises(TypeError):
            filters.remove_silence(16000, bad)
    with pytest.raises(ValueError):
        filters.remove_silence(16000, np.zeros((100, 2), np.int16))
    with pytest.raises(ValueError):
        filters.remove_silence(16000, np.zeros(0, np.int16))
    assert filters.remove_silence_many(16000, []) == []


def test_interface_setting_and_old_pickles(built_lib, tmp_path):
    from speaker_recognition_amd.interface import ModelInterface
    assert ModelInterface(verbose=False)._silence_kwargs() is None
    assert ModelInterface(verbose=False, remove_silence=True)._silence_kwargs() == {}
    assert ModelInterface(verbose=False, remove_silence=dict(perc=0.2, frame_shift=0.005))._silence_kwargs() == dict(perc=0.2, frame_shift=0.005)
    for bad in ("yes", 1.5, dict(percent=0.2)):
        with pytest.raises(ValueError):
            ModelInterface(verbose=False, remove_silence=bad)
    # a model pickled before the setting existed: no such attribute -- it loads and behaves as remove_silence=False
    m = ModelInterface(verbose=False)
    del m.__dict__["remove_silence"]
    f = str(tmp_path / "old.out")
    m.dump(f)
    old = ModelInterface.load(f)
    assert "remove_silence" not in old.__dict__ and old._silence_kwargs() is None
    items = [(16000, np.arange(10, dtype=np.int16))]
    assert old._desilenced(items) == items                     # untouched, no device call
    # and the setting travels with a new one
    f2 = str(tmp_path / "new.out")
    ModelInterface(verbose=False, remove_silence=dict(perc=0.3)).dump(f2)
    assert ModelInterface.load(f2).remove_silence == dict(perc=0.3)
    assert pickle.loads(pickle.dumps(dict(perc=0.3))) == dict(perc=0.3)


def test_cli_parses_remove_silence():
    from speaker_recognition_amd import cli
    base = ["-i", "x", "-m", "y"]
    for task in ("enroll", "predict"):
        assert cli.get_args(["-t", task] + base + ["--remove-silence"]).remove_silence is True
        assert cli.get_args(["-t", task] + base).remove_silence is False
    args = cli.get_args(["-t", "enroll"] + base + ["--remove-silence"])
    assert cli._make_interface(args).remove_silence is True
    assert cli._make_interface(cli.get_args(["-t", "enroll"] + base)).remove_silence is False
    assert cli._make_interface(None)._silence_kwargs() is None


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_silence_plan_under_asan_ubsan(tmp_path):
    """csrc/silence_plan.cpp swept over rates, frame shapes, lengths and block options by a stand-alone program
    (tests/host/silence_checks.cpp) built with AddressSanitizer + UBSan: host code only, no GPU, nothing loaded into Python."""
    exe = str(tmp_path / "silence_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "host", "silence_checks.cpp"), os.path.join(CSRC, "silence_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "silence checks ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
