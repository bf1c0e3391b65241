"""The host half of the iteration-at-a-time trainer without a GPU (tests/host/em_checks.cpp): csrc/em_plan.cpp -- the route of a fit
and the statistics launch of an iteration, swept over shapes, device sizes and options -- and csrc/em_mstep.cpp -- re-centring, the
float64 redo of unsupported mixtures on 1, 2 and 16 threads, the M-step's rules, the stop rule, one full iteration against the
parameters formed directly.  A stand-alone program under AddressSanitizer + UBSan: host code only, nothing loaded into Python.
And the lists of built kernels in csrc/em_shapes.hpp against what csrc/em.hip compiled to."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")


@pytest.fixture(scope="module")
def em_checks(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("em_host") / "em_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "host", "em_checks.cpp")] + \
          [os.path.join(CSRC, f) for f in ("em_plan.cpp", "em_mstep.cpp", "map_plan.cpp")] + ["-o", exe, "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_em_plan_and_mstep_under_asan_ubsan(em_checks):
    r = subprocess.run([em_checks], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    print(r.stdout)
    assert r.returncode == 0 and "em checks ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_built_kernels_are_the_listed_ones(em_checks, built_lib):
    """em_shapes.hpp's three lists -- which the dispatch and the *_available predicates are generated from -- name exactly the
    statistics kernels in em.hip's object (build/em.resources, written by the Makefile)."""
    r = subprocess.run([em_checks, "--table"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    table = dict(line.split(":") for line in r.stdout.strip().splitlines())
    listed = {k: sorted(tuple(int(x) for x in e.split(",")) for e in v.split()) for k, v in table.items()}
    text = open(os.path.join(ROOT, "speaker-recognition_amd", "build", "em.resources")).read()
    built = {"vector": sorted(set((int(d),) for d in re.findall(r"Function Name: _ZN2sr15em_stats_kernelILi(\d+)EE", text))),
             "mfma": sorted(set((int(d),) for d in re.findall(r"Function Name: _ZN2sr20em_stats_mfma_kernelILi(\d+)EE", text))),
             "split": sorted(set((int(d), int(k)) for d, k in re.findall(r"Function Name: _ZN2sr21em_stats_split_kernelILi(\d+)ELi(\d+)EE", text)))}
    assert built == listed and all(len(v) > 0 for v in built.values()), (built, listed)
    # the float64 reduction exists for every padded dim of the two matrix-core forms
    reduce64 = sorted(set((int(d),) for d in re.findall(r"Function Name: _ZN2sr18em_reduce64_kernelILi(\d+)EE", text)))
    assert reduce64 == listed["mfma"] and set(d for d, _ in listed["split"]) <= set(d for d, in listed["mfma"])
