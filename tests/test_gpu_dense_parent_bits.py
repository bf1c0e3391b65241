"""The calls built on the float64 dense layer (csrc/dense64.hip's strided GEMM, csrc/dense64_dev.hpp's panel Cholesky and inverse
routines, csrc/dense64_plan.hpp's grids and LDS sizes) reproduce, bit for bit, what they computed when the layer still lived inside
JFA's files under JFA's names: tests/golden/dense_parent_bits.npz was recorded by tests/golden/make_dense_parent_bits.py at the
commit before the move, twice, and kept because the two recordings agreed in every bit -- per case of tests/dense_parent_cases.py
every array the calls return and the counts beside them (blocks that did not factor, mixtures skipped, stop codes)."""
import os

import numpy as np
import pytest

import dense_parent_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def parent_bits(built_lib):
    return np.load(os.path.join(ROOT, "tests", "golden", "dense_parent_bits.npz"))


def test_every_case_was_recorded(parent_bits):
    assert sorted({k.split("/")[0] for k in parent_bits.files}) == sorted(pc.NAMES)


@pytest.mark.parametrize("name", pc.NAMES)
def test_dense_layer_has_the_parent_commits_bits(parent_bits, name):
    got = pc.run_case(name)
    keys = sorted(k for k in parent_bits.files if k.startswith(name + "/"))
    assert keys == sorted(name + "/" + k for k in got)
    for k in keys:
        want, have = parent_bits[k], got[k[len(name) + 1:]]
        assert want.dtype == have.dtype and want.shape == have.shape and want.tobytes() == have.tobytes(), (k, want, have)


def test_the_recording_shows_what_the_cases_are_for(parent_bits):
    """the blocks that must not factor did not, and are counted; every other case factored everything; the chunked sums ran"""
    for name in pc.NAMES:
        if name.startswith(("jfa_r", "kscore_r")):
            assert not parent_bits[name + "/counts"].any(), name
    for name in pc.NAMES:
        if name.startswith("plda_r"):
            it, nc, stop, bad = parent_bits[name + "/counts"].tolist()
            assert (it, nc, stop, bad) == (2, 2, 0, 0), name
    bad, skipped = parent_bits["jfa_blocks_that_do_not_factor/counts"].tolist()
    assert (bad, skipped) == (5, 1)
    for k in ("y", "A", "C"):
        assert not parent_bits["jfa_blocks_that_do_not_factor/" + k].any()
    it, nc, stop, bad = parent_bits["plda_blocks_that_do_not_factor/counts"].tolist()
    assert (it, stop, bad) == (0, 1, nc) and nc == 2 and not parent_bits["plda_blocks_that_do_not_factor/out"].any()
    assert parent_bits["backend_lds0/status"].tolist() == [0] and parent_bits["backend_lds1/status"].tolist() == [0]
