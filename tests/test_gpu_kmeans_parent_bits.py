"""The start in front of EM (csrc/kmeans_host.cpp on the device back end of csrc/kmeans_init.hip, planned by csrc/kmeans_plan.cpp)
reproduces, bit for bit, what csrc/kmeans_init.hip computed when deciding, sizing, host arithmetic and launching still shared that
one file: tests/golden/kmeans_parent_bits.npz was recorded by tests/golden/make_kmeans_parent_bits.py at the commit before the split,
twice, and kept because the two recordings agreed in every bit -- per fit of tests/kmeans_parent_cases.py the weights, means and
sigmas (or the message of the refusal) and the deltas of the two kmeans_fast_stats() counters."""
import os

import numpy as np
import pytest

import kmeans_parent_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def parent_bits(built_lib):
    return np.load(os.path.join(ROOT, "tests", "golden", "kmeans_parent_bits.npz"))


def test_every_case_was_recorded(parent_bits):
    assert sorted({k.split("/")[0] for k in parent_bits.files}) == sorted(pc.NAMES)


@pytest.mark.parametrize("name", pc.NAMES)
def test_start_has_the_parent_commits_bits(parent_bits, name):
    got = pc.run_case(pc.BY_NAME[name])
    keys = sorted(k for k in parent_bits.files if k.startswith(name + "/"))
    assert keys == sorted(name + "/" + k for k in got)
    for k in keys:
        want, have = parent_bits[k], got[k[len(name) + 1:]]
        assert want.dtype == have.dtype and np.array_equal(want, have), (k, want, have)


def test_the_cases_reach_every_instantiation_and_both_counters(parent_bits):
    """what the recording itself must show: fast passes exactly where D <= 40 and the engine option is 0, and points rechecked where
    centres coincide"""
    for name, _n, _K, D, _conc, _seed, km, eng, _kind in pc.CASES:
        passes, rechecked = parent_bits[name + "/fast_stats"].tolist()
        assert (passes > 0) == (km > 0 and D <= 40 and eng == 0), name
        assert rechecked == 0 or passes > 0
    assert parent_bits["ties_k48/fast_stats"][1] > 0
