"""The plan of a full-covariance fit without a GPU (csrc/full_plan.cpp): tests/host/full_checks.cpp -- the cut, the tables, the work
lists, every buffer's size and every narrowing, swept over K, D, frame counts, ragged sets and bounds in a stand-alone program under
AddressSanitizer + UBSan (host code only, nothing loaded into Python) -- and, through sr_full_fit_plan, the cuts DESIGN 3.8 records."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_full_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "full_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "host", "full_checks.cpp"), os.path.join(CSRC, "full_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    print(r.stdout)
    assert r.returncode == 0 and "full checks ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def closed_form_bytes(n, K, D):
    """the workspace of a lone speaker, term by term: X, lp, lpn, the chunk sums, prec and cov, mu, w logw logdet nk, head (float64);
    the three work lists (8 bytes a row); the labels; the table entry (72) and the record (16)"""
    n_chunks = min(32, (n + 255) // 256)
    doubles = n * D + n * K + n + n_chunks * K * (D * (D + 1) // 2) + 2 * K * D * D + K * D + 4 * K + 2
    return 8 * doubles + 8 * ((n + 31) // 32 + (n + 255) // 256 + n_chunks) + 4 * n + 72 + 16


def test_symbol_exported_bound_and_declared(built_lib):
    from speaker_recognition_amd import _lib
    assert "sr_full_fit_plan" in _lib.EXT_SYMBOLS and hasattr(C.CDLL(_lib.LIB_PATH), "sr_full_fit_plan")
    text = " ".join(open(os.path.join(ROOT, "include", "pygmm_hip.h")).read().split())
    assert ("int sr_full_fit_plan(int K, int D, const int64_t *lengths, const int *init_given, const int *max_iter, int S, "
            "int64_t bound_bytes, int64_t *speakers_out, int64_t *groups_out, int64_t group_cap, int64_t *out, int n_out);") in text


def test_the_documented_set_is_one_group_at_the_default_bound(built_lib):
    """100 speakers x 5600 frames x K 32 x D 28: 5.5 MB a speaker, one group under 1 GiB, 98 + 2 under 512 MiB"""
    from speaker_recognition_amd import _lib
    assert _lib.full_fit_batch_bytes() == 1 << 30
    p = _lib.full_fit_plan(32, 28, [5600] * 100)                   # (bound 0: the current full_fit_batch_bytes)
    assert closed_form_bytes(5600, 32, 28) == 5453248
    assert p["lone_bytes"] == 5453248 and p["speakers"][:, 5].tolist() == [5453248] * 100
    assert p["n_groups"] == 1 and p["groups"][0, :3].tolist() == [0, 100, 560000]
    assert p["max_group_bytes"] == 100 * 5453248 == int(p["groups"][0, 9])
    assert (p["n_lp"], p["n_lse"], p["n_cov"]) == (100 * 175, 100 * 22, 100 * 22)
    assert p["lds_logprob"] == 8 * (28 * 28 + 28 + 32 * 29 + 256)
    assert p["speakers"][:, 1].tolist() == [5600 * s for s in range(100)]           # row0
    assert p["speakers"][:, 2:4].tolist() == [[22, 255]] * 100                      # 22 chunks of 255 frames
    p = _lib.full_fit_plan(32, 28, [5600] * 100, bound_bytes=512 << 20)
    assert p["n_groups"] == 2 and p["groups"][:, :2].tolist() == [[0, 98], [98, 2]]
    assert p["speakers"][:, 6].tolist() == [0] * 98 + [1] * 2 and p["speakers"][98:, 7].tolist() == [0, 1]
    assert p["speakers"][98:, 1].tolist() == [0, 5600]                              # rows start again in a group


def test_a_bound_of_one_byte_gives_a_group_per_speaker(built_lib):
    from speaker_recognition_amd import _lib
    ns = [5600, 32, 200, 256, 257, 9000, 32]
    p = _lib.full_fit_plan(32, 28, ns, bound_bytes=1)
    assert p["n_groups"] == len(ns) and p["groups"][:, :2].tolist() == [[s, 1] for s in range(len(ns))]
    assert p["groups"][:, 9].tolist() == [closed_form_bytes(n, 32, 28) for n in ns]
    assert p["speakers"][:, 2].tolist() == [22, 1, 1, 1, 2, 32, 1] and p["speakers"][5, 3] == 282


def test_the_d64_batch_is_one_group_by_default_and_three_under_one_mib(built_lib):
    """test_gpu_fullfit_cases.py's BATCH_N at K 2, D 64: the first three speakers, 8193 frames alone, the last alone"""
    from speaker_recognition_amd import _lib
    BATCH_N = (4, 33, 257, 8193, 300)
    p = _lib.full_fit_plan(2, 64, BATCH_N, init_given=[1] * 5, max_iter=[3] * 5)
    assert p["n_groups"] == 1 and p["groups"][0, 6:9].tolist() == [3, 0, 1]          # max_iter 3, no k-means start, a given one
    p = _lib.full_fit_plan(2, 64, BATCH_N, init_given=[1] * 5, max_iter=[3] * 5, bound_bytes=1 << 20)
    assert p["n_groups"] == 3 and p["groups"][:, :2].tolist() == [[0, 3], [3, 1], [4, 1]]
    assert closed_form_bytes(8193, 2, 64) > 1 << 20                                 # (above the bound: a group of its own)
    for g in p["groups"]:
        counts = g[10:]
        assert g[9] == 8 * counts[:12].sum() + 72 * counts[12] + 16 * counts[13] + 8 * counts[14:17].sum() + 4 * counts[17]
        assert g[9] == sum(closed_form_bytes(n, 2, 64) for n in BATCH_N[g[0]:g[0] + g[1]])


def test_refusals_come_with_a_reason_and_touch_no_device(built_lib):
    from speaker_recognition_amd import _lib
    for args, word in (((65536, 3, [100]), "65536 components"), ((2, 65, [100]), "D 65"), ((2, 3, [0]), "0 frames"),
                       ((2, 3, [32 * (2 ** 31 - 1) + 1]), "frames")):
        with pytest.raises(_lib.SRError, match=word):
            _lib.full_fit_plan(*args)
    with pytest.raises(_lib.SRError, match="full_fit_batch_bytes must be >= 1"):
        _lib.full_fit_plan(2, 3, [100], bound_bytes=-1)
    with pytest.raises(_lib.SRError, match="at least one speaker"):
        _lib.full_fit_plan(2, 3, [])
