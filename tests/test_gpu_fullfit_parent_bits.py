"""The float64 full-covariance EM driver (csrc/gmm_full_fit.hip: fe_fit_group over a plan of csrc/full_plan.cpp) reproduces, bit for
bit, what it computed before it was split out of csrc/gmm_full.hip and given a plan: tests/golden/fullfit_parent_bits.npz was
recorded by tests/golden/make_fullfit_parent_bits.py at the commit before the split, twice, and holds the cases whose two recordings
agreed -- per fit of tests/fullfit_parent_cases.py n_iter, converged, lower_bound, weights, means and the SHA-256 of the precision
factors and of the covariances; per batch the three sr_full_fit_batch_stats deltas.  The tests of one build against itself
(a group of one against a group of S) pass when both move; these do not.  The k-means start's launch geometry is a function of
the compute-unit count: on a device with another count than the recorded one the comparison says nothing and the tests skip."""
import os
import re

import numpy as np
import pytest

import fullfit_parent_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def parent_bits(built_lib):
    from speaker_recognition_amd import _lib
    g = np.load(os.path.join(ROOT, "tests", "golden", "fullfit_parent_bits.npz"))
    n_cu = int(re.search(r"(\d+) CUs", _lib.device_name()).group(1))
    if n_cu != int(g["n_cu"]):
        pytest.skip("recorded on a device of %d compute units, this one has %d" % (int(g["n_cu"]), n_cu))
    return g


def test_every_case_was_kept(parent_bits):
    assert sorted(parent_bits["cases"].tolist()) == sorted(pc.CASES)


@pytest.mark.parametrize("name", pc.CASES)
def test_fit_has_the_parent_commits_bits(parent_bits, name):
    assert name in parent_bits["cases"].tolist()
    got = pc.run_case(name)
    keys = sorted(k for k in parent_bits.files if k.startswith(name + "/"))
    assert keys == sorted(name + "/" + k for k in got)
    for k in keys:
        want, have = parent_bits[k], got[k[len(name) + 1:]]
        assert want.dtype == have.dtype and np.array_equal(want, have), (k, want, have)
