"""The compact order of the pipelined shared-sigma kernel on the host (tests/host/h2c_checks.cpp): csrc/score_shapes.hpp's map --
which stored fragment and frame register every MFMA step multiplies, when the next image's fragments are read, the lgkmcnt counts --
replayed on an in-order queue for every part length, and csrc/model_pack_shared.cpp's pack_h2_compact against the flat
pack_models_h2_shared at D = 37, 38, 39 (the same multiset of products per mixture row) and D = 40 (no compact form).  A stand-alone
program under AddressSanitizer + UBSan: host code only, no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_compact_map_and_pack_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "h2c_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "host", "h2c_checks.cpp"),
           *[os.path.join(CSRC, f) for f in ("fp_parts.cpp", "model_pack.cpp", "model_pack_shared.cpp")], "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "h2c checks ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
