"""The iteration-at-a-time trainer (csrc/em.hip: train_em, the host M-step of csrc/em_mstep.cpp, the launches planned by
csrc/em_plan.cpp) reproduces, bit for bit, what it computed before it was split into those parts: tests/golden/em_parent_bits.npz
was recorded by tests/golden/make_em_parent_bits.py at the commit before the split, twice, and holds the cases whose two recordings
agreed -- iteration counts, the engine reported, weights, means and sigmas of the fits of tests/em_parent_cases.py.  The order of the
device's sums is a function of the launch geometry and that of the compute-unit count: on a device with another count than the
recorded one the comparison says nothing and the tests skip."""
import os
import re

import numpy as np
import pytest

import em_parent_cases as ec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def parent_bits(built_lib):
    from speaker_recognition_amd import _lib
    g = np.load(os.path.join(ROOT, "tests", "golden", "em_parent_bits.npz"))
    n_cu = int(re.search(r"(\d+) CUs", _lib.device_name()).group(1))
    if n_cu != int(g["n_cu"]):
        pytest.skip("recorded on a device of %d compute units, this one has %d: another launch geometry, another order of the sums"
                    % (int(g["n_cu"]), n_cu))
    return g


def test_every_case_was_kept(parent_bits):
    assert sorted(parent_bits["cases"].tolist()) == sorted(c[0] for c in ec.CASES)


@pytest.mark.parametrize("case", ec.CASES, ids=[c[0] for c in ec.CASES])
def test_fit_has_the_parent_commits_bits(parent_bits, case):
    assert case[0] in parent_bits["cases"].tolist()
    got = ec.run_case(case)
    keys = sorted(k for k in parent_bits.files if k.startswith(case[0] + "/"))
    assert keys == sorted(case[0] + "/" + k for k in got)
    assert got["iterations"].tolist() == parent_bits[case[0] + "/iterations"].tolist()
    assert got["engine"].tolist() == parent_bits[case[0] + "/engine"].tolist()
    for k in keys:
        want, have = parent_bits[k], got[k[len(case[0]) + 1:]]
        assert want.dtype == have.dtype and np.array_equal(want, have), (k, float(np.max(np.abs(want - have))))
