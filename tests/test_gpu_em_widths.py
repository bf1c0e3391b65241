"""The EM statistics kernels of csrc/em.hip at every padded row width they are built for (tests/em_width_cases.py): one warm-start
iteration under the forced engine against the float64 oracle, at the project's gates on an EM iteration -- weights 1e-5 and means
1e-4 absolute, sigmas 1e-3 relative (tests/test_gpu_pipeline.py::test_em_statistics_engines_vs_oracle).  One test per
(engine, width): em_stats_kernel<DP> and em_stats_wide_kernel (engine 1), em_stats_mfma_kernel<DP> (2), em_stats_split_kernel<DP, KS>
(3), the latter two through em_reduce64_kernel<DP>; the smallest and the largest dim of the width, at the largest also a model of
one mostly dead workgroup, one with a nearly empty last workgroup, a means-only MAP iteration on the UBM's own packed set, the same
fit twice, and the engines against each other.  Then the long rows: more than one tile per workgroup with an uneven last chunk,
record ranges of two records with workgroups that return, the tile loop's stride.  tests/test_em_width_cases_cpu.py holds the
table's own conditions."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import em_width_cases as wc  # noqa: E402

pytestmark = pytest.mark.gpu

GROUPS = wc.groups()
_FITS = {}


def _run(row):
    """the row's iteration on the device under its forced option -> (weights, means, sigmas)"""
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.pygmm import GMM
    _, X, start = wc.make_data(row.dim, row.K, row.n)
    _lib.set_option("em_stats_engine", row.option)
    try:
        if row.kind == "map":
            ubm = GMM.from_arrays(*start)
            g = GMM(row.K, nr_iteration=1)
            assert g.fit(X, ubm=ubm) == 1
        else:
            g = GMM.from_arrays(*start)
            g.nr_iteration, g.init_with_kmeans = 1, -1            # -1: warm start (extension)
            assert g.fit(X) == 1
        assert _lib.last_em_stats_engine() == row.engine, (row, _lib.last_em_stats_engine())
        return g.params()
    finally:
        _lib.set_option("em_stats_engine", 0)


def _fit(row):
    if row not in _FITS:
        _FITS[row] = _run(row)
    return _FITS[row]


def _against_the_oracle(go, row):
    """the row's errors in gates, asserted"""
    want = wc.oracle_iteration(go, row)
    got = _fit(row)
    e = wc.errors(got, want)
    print("    %s: weights %.3g means %.3g sigmas %.3g of their gates" % (row, e[0], e[1], e[2]))
    if row.kind == "map":
        start = wc.make_data(row.dim, row.K, row.n)[2]
        assert np.array_equal(got[0], start[0]) and np.array_equal(got[2], start[2]), row       # the UBM's, bit for bit
        assert e[1] < 1.0, (row, e)
    else:
        assert e[0] < 1.0 and e[1] < 1.0 and e[2] < 1.0, (row, e)
    return e


@pytest.mark.parametrize("gid,rows", GROUPS, ids=[g for g, _ in GROUPS])
def test_width_against_the_oracle(built_lib, oracle_built, gid, rows):
    go = oracle_built
    errs = [_against_the_oracle(go, row) for row in rows]
    worst = [max(e[i] for e, r in zip(errs, rows) if r.kind == "em" or i == 1) for i in range(3)]
    print("em width %s: worst weights %.3g means %.3g sigmas %.3g of their gates over %d rows" % (gid, worst[0], worst[1], worst[2], len(rows)))
    # ---- at the largest dim of the width, on its base shape
    top = max((r for r in rows if r.kind == "em"), key=lambda r: (r.dim, r.K in (wc.BASE_K, wc.SPLIT_K)))
    again = _run(top)
    assert all(np.array_equal(a, b) for a, b in zip(again, _fit(top))), top                    # the same fit twice: the same bits
    if top in wc.LONG_ROWS or top.option != top.engine:
        return
    if top.engine == 3:
        # the two matrix-core engines differ in the rounding of the log densities only
        twin = top._replace(option=2, engine=2)
        assert twin in wc.twin_rows()
        _against_the_oracle(go, twin)
        (_, mu3, sg3), (_, mu2, sg2) = _fit(top), _fit(twin)
        d_mu, d_sg = float(np.max(np.abs(mu3 - mu2))), float(np.max(np.abs(sg3 - sg2) / sg2))
        print("    engines 2 and 3 at D = %d: means %.3g sigmas %.3g apart (gate %.0e)" % (top.dim, d_mu, d_sg, wc.ENGINES_AGREE))
        assert d_mu < wc.ENGINES_AGREE and d_sg < wc.ENGINES_AGREE, (top, d_mu, d_sg)
    if top.engine == 2:
        # float64 sums about the origin are at least as close to the oracle as the fp32 ones about each mean
        e2, e1 = errs[rows.index(top)], _against_the_oracle(go, top._replace(option=1, engine=1))
        assert e2[2] * wc.GATE_SG <= e1[2] * wc.GATE_SG + wc.NO_WORSE and e2[1] * wc.GATE_MU <= e1[1] * wc.GATE_MU + wc.NO_WORSE, (top, e2, e1)
