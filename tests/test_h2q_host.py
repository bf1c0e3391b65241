"""Pairs of blocks in the compact pipelined shared-sigma kernel on the host (tests/host/h2q_checks.cpp): csrc/score_shapes.hpp's
pair arithmetic -- stages per pair, images executed, index and parity of the last executed image, source image of every stage --
for every (15, m), m = 0 .. 15; csrc/model_pack_shared.cpp's pack_h2_compact holds the same bytes in every block's quadratic-half image of
a mixture tile (what pairing rests on); 201 models execute 210 images per mixture tile instead of 216.  A stand-alone program under
AddressSanitizer + UBSan: host code only, no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pair_arithmetic_and_shared_q_images_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "h2q_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "host", "h2q_checks.cpp"),
           *[os.path.join(CSRC, f) for f in ("fp_parts.cpp", "model_pack.cpp", "model_pack_shared.cpp")], "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "h2q checks ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
