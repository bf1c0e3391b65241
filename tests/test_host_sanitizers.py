"""csrc/model_text.cpp (text format, number conversions), csrc/fp_parts.cpp and csrc/model_pack*.cpp (every packer), csrc/score_plan.cpp (the
dispatcher) and csrc/mfcc_plan.cpp (the MFCC stage's table layout and launch decisions) under AddressSanitizer + UBSan, and the threaded
packers under ThreadSanitizer: tests/host/host_checks.cpp, built here with g++ (host code only, no GPU, no HIP runtime).  The
same for csrc/multi_plan.cpp (the multi-GPU predictor's sharding plan), by a program of its own: tests/host/multi_checks.cpp."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")


HOST_CHECKS_SOURCES = ("model_text.cpp", "fp_parts.cpp", "model_pack.cpp", "model_pack_shared.cpp", "score_plan.cpp", "mfcc_plan.cpp")


def _build_and_run(tmp_path, flags, args, env=None, program="host_checks", sources=HOST_CHECKS_SOURCES, ok="host checks ok"):
    exe = str(tmp_path / program)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", *flags, "-I", CSRC, "-I", "/opt/rocm/include",
           "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "host", program + ".cpp"), *[os.path.join(CSRC, s) for s in sources],
           "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0 and ok in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_model_host_code_under_asan_ubsan(tmp_path):
    _build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], [],
                   env={"ASAN_OPTIONS": "detect_leaks=1"})


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_score_plan_under_asan_ubsan(tmp_path):
    """The dispatcher's decisions (engine, shapes, model groups) on sets packed by the library's own pack_model_set, against the
    values recorded from the commit before the plan became a function of its own (tests/host/host_checks.cpp, mode "plan")."""
    _build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], ["plan"],
                   env={"ASAN_OPTIONS": "detect_leaks=1"})


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_packed_images_under_asan_ubsan(tmp_path):
    """Every packer's image of small sets -- each layout, shared and independent sets, dead, negative-weight and zero-sigma mixtures --
    and the packers' error texts, against the hashes and figures recorded from the commit before the packers were first touched
    (tests/host/pack_table.inc; tests/host/host_checks.cpp, mode "pack")."""
    _build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], ["pack"],
                   env={"ASAN_OPTIONS": "detect_leaks=1"})


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_mfcc_plan_under_asan_ubsan(tmp_path):
    """The MFCC stage's mel-table layout and launch decisions (kernel, template arguments, workgroup shape, LDS, frames per wave)
    against the values its launchers computed inline before, and the layout's invariants over every FFT size and bank width
    (tests/host/host_checks.cpp, mode "mfcc")."""
    _build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], ["mfcc"],
                   env={"ASAN_OPTIONS": "detect_leaks=1"})


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_multi_plan_under_asan_ubsan(tmp_path):
    """The multi-GPU predictor's plan (active slots, utterances per slot, a slot's pieces, its schedule across calls), built from
    csrc/multi_plan.cpp alone: the decisions recorded from the commit before the plan became a file of its own
    (tests/host/multi_table.inc) and its invariants over the table and seeded random batches (tests/host/multi_checks.cpp)."""
    _build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], [],
                   env={"ASAN_OPTIONS": "detect_leaks=1"}, program="multi_checks", sources=("multi_plan.cpp",), ok="multi checks ok")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_threaded_packers_under_tsan(tmp_path):
    _build_and_run(tmp_path, ["-fsanitize=thread"], ["threads"])
