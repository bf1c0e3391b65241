"""CPU side of the open-set decision (csrc/open_set.hip and the sr_*_open calls): the symbols, the argument checks that must not
need a device, the kernel's resource record, the Python surface, and the numpy restatement of the reference's rule
(tests/open_set_cases.py) on cases worked out by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import open_set_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sr_open_set_decide", "sr_score_batch_set_open", "sr_predict_pcm_batch_open", "sr_stream_set_open", "sr_stream_collect_open",
       "sr_multi_predict_pcm_open"]


def test_symbols_exported_and_declared(built_lib):
    from speaker_recognition_amd import _lib
    header = open(os.path.join(ROOT, "include", "pygmm_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), "lib/pygmm.so does not export %s" % name
        assert re.search(r"\bint %s\(" % name, header), "%s is not declared in include/pygmm_hip.h" % name
        assert name in _lib.EXT_SYMBOLS
    for name in ("sr_stream_collect", "sr_stream_collect_vad", "sr_score_batch_set", "sr_predict_pcm_batch", "sr_multi_predict_pcm"):
        assert hasattr(raw, name)                      # the siblings stay


def test_kernel_resources_no_scratch_no_lds(built_lib):
    path = os.path.join(ROOT, "speaker-recognition_amd", "build", "open_set.resources")
    assert os.path.exists(path), "the build did not leave %s" % path
    text = open(path).read()
    blocks = re.split(r"Function Name: ", text)[1:]
    mine = [b for b in blocks if "open_set_decision_kernel" in b.split()[0]]
    assert len(mine) == 1, [b.split()[0] for b in blocks]
    assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", mine[0]).group(1)) == 0
    assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", mine[0]).group(1)) == 0


def test_argument_errors_fail_before_any_device_work(built_lib):
    """Every check below fails on its arguments alone: the message names the argument, never the device -- on a machine without
    a GPU a call that had reached the device would say "no HIP device" instead."""
    from speaker_recognition_amd import _lib
    L = built_lib
    sums = np.zeros((2, 3))
    n = np.array([4, 5], dtype=np.int64)
    lab = np.zeros(2, dtype=np.int32)
    mar = np.zeros(2)

    def decide(sums_p, bg, thr, n_p, lab_p, mar_p, U=2, S=3):
        return L.sr_open_set_decide(sums_p, U, S, bg, n_p, thr, lab_p, mar_p)

    ok = (_lib.as_dp(sums), _lib.as_i64p(n), _lib.as_i32p(lab), _lib.as_dp(mar))
    for args, pat in (((ok[0], -1, 0.0, ok[1], ok[2], ok[3]), "outside"),
                      ((ok[0], 3, 0.0, ok[1], ok[2], ok[3]), "outside"),
                      ((ok[0], 0, float("nan"), ok[1], ok[2], ok[3]), "NaN"),
                      ((ok[0], 0, 0.0, ok[1], None, ok[3]), "null output"),
                      ((ok[0], 0, 0.0, ok[1], ok[2], None), "null output"),
                      ((None, 0, 0.0, ok[1], ok[2], ok[3]), "null argument"),
                      ((ok[0], 0, 0.0, None, ok[2], ok[3]), "null argument")):
        assert decide(*args) == -1
        assert pat in _lib.last_error() and "HIP" not in _lib.last_error(), (pat, _lib.last_error())
    bad_n = np.array([4, -1], dtype=np.int64)
    assert decide(ok[0], 0, 0.0, _lib.as_i64p(bad_n), ok[2], ok[3]) == -1 and "negative frame count" in _lib.last_error()
    assert decide(ok[0], 0, 0.0, ok[1], ok[2], ok[3], S=0) == -1 and "bad shape" in _lib.last_error()
    assert L.sr_score_batch_set_open(None, None, 0, 0.0, None, ok[2], ok[3], 0) == -1 and "null argument" in _lib.last_error()
    assert L.sr_predict_pcm_batch_open(None, None, None, 0, 0, 0.0, None, ok[2], ok[3], 0) == -1 and "null argument" in _lib.last_error()
    assert L.sr_stream_set_open(None, 0, 0.0) == -1 and "null stream" in _lib.last_error()
    assert L.sr_stream_collect_open(None, None, ok[2], ok[3], None, None) == -1 and "null stream" in _lib.last_error()
    off = np.zeros(1, dtype=np.int64)
    assert L.sr_multi_predict_pcm_open(None, None, _lib.as_i64p(off), 0, 0, 0, 0.0, None, ok[2], ok[3], None, 0) == -1
    assert "bad arguments" in _lib.last_error()
    if _lib.device_count() == 0:                       # and a well-formed call says what is missing: no CPU path
        assert decide(*ok[:1], 0, 0.0, *ok[1:]) == -1 and "no HIP device" in _lib.last_error()


def test_gmmset_batched_rejection_needs_a_ubm(built_lib):
    from speaker_recognition_amd.gmmset import GMMSet
    gs = GMMSet()
    for call in (gs.predict_with_reject_batch, gs.reject_margins, gs.predict_one_with_rejection):
        with pytest.raises(AssertionError, match="UBM must be given prior to conduct reject prediction."):
            call([np.zeros((3, 2))] if call is not gs.predict_one_with_rejection else np.zeros((3, 2)))


def test_interface_and_cli_refuse_a_threshold_without_a_ubm(built_lib, tmp_path):
    from speaker_recognition_amd import cli
    from speaker_recognition_amd.interface import ModelInterface
    m = ModelInterface(verbose=False)
    with pytest.raises(ValueError, match="enrolled from a UBM"):
        m.predict(8000, np.zeros(8000, np.int16), reject_threshold=0.5)
    assert cli.get_args(["-t", "predict", "-i", "x", "-m", "y"]).reject_threshold is None
    assert cli.get_args(["-t", "predict", "-i", "x", "-m", "y", "--reject-threshold", "0.25"]).reject_threshold == 0.25
    model = str(tmp_path / "m.out")
    m.dump(model)
    with pytest.raises(SystemExit):
        cli.task_predict(str(tmp_path / "*.wav"), model, 1, 0.5)
    with pytest.raises(ValueError, match="enrolled from a UBM"):
        m.predict_many_with_reject([(8000, np.zeros(8000, np.int16))], 0.5)


def test_rule_restatement_on_hand_computed_cases():
    nan = float("nan")
    # bg = 0; 4 frames: quotients -2.5, -1.5, -2; best column 2, margin -1.5 - (-3) = 1.5
    assert oc.rule_one([-12.0, -10.0, -6.0, -8.0], 4, 0, 1.5) == (2, 1.5)               # equal to the threshold: accepted
    assert oc.rule_one([-12.0, -10.0, -6.0, -8.0], 4, 0, 1.5000001) == (-1, 1.5)
    # equal maxima: the lower index; the background in the middle is skipped even when it is the largest
    assert oc.rule_one([-6.0, -1.0, -6.0], 2, 1, -100.0) == (0, -2.5)
    assert oc.rule_one([-8.0, -4.0], 4, 1, 0.0) == (-1, -1.0)
    assert oc.rule_one([-8.0, -4.0], 4, 0, 0.0) == (1, 1.0)
    # no frames / nobody besides the background
    for row, n, bg in (([-1.0, -2.0], 0, 0), ([-1.0], 5, 0)):
        lab, mar = oc.rule_one(row, n, bg, 0.0)
        assert lab == -1 and np.isnan(mar)
    # two sums one ulp apart whose quotients are equal: the lower index, although the higher holds the larger sum
    x = np.float64(-1000.3)
    y = np.nextafter(x, np.inf)
    n = next(k for k in range(3, 1000) if x / np.float64(k) == y / np.float64(k))
    assert y > x and oc.rule_one([2 * x, x, y], n, 0, -1e9)[0] == 1
    assert int(np.argmax([x, y])) == 1                                                 # (comparing the sums would pick the other)
    labels, margins = oc.rule(np.array([[-12.0, -10.0, -6.0, -8.0], [0.0, 0.0, 0.0, 0.0]]), [4, 0], 0, 1.5)
    assert labels.tolist() == [2, -1] and margins[0] == 1.5 and np.isnan(margins[1]) and nan != margins[1]
