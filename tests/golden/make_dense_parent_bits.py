#!/usr/bin/env python3
"""What the calls built on the float64 dense layer (the strided GEMM, the panel Cholesky of one block and the two inverse routines:
JFA estimation and scoring, centring, PLDA, the eigen back end, score normalisation) compute, to the bit, at the commit BEFORE a
change that must not move them: run on an MI355X at that commit, twice,

    python tests/golden/make_dense_parent_bits.py /tmp/a.npz && python tests/golden/make_dense_parent_bits.py /tmp/b.npz
    python tests/golden/make_dense_parent_bits.py --merge /tmp/a.npz /tmp/b.npz

The merge requires the two recordings to agree in every bit of every case and only then writes
tests/golden/dense_parent_bits.npz: per case of tests/dense_parent_cases.py every array the calls return -- factors, accumulators,
loadings, covariances, score matrices -- and the counts beside them (groups and classes that did not factor, mixtures skipped, stop
codes)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dense_parent_cases as pc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "dense_parent_bits.npz")


def record(path):
    out = {}
    for name in pc.NAMES:
        got = pc.run_case(name)
        print("%-32s %s" % (name, ", ".join("%s %s" % (k, v.tolist() if k in ("counts", "status") else "%.17g" % np.abs(v).sum())
                                              for k, v in sorted(got.items()))))
        for k, v in got.items():
            out[name + "/" + k] = v
    np.savez_compressed(path, **out)


def merge(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files)
    differ = [k for k in a.files if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
    assert not differ, "the two recordings differ: %s" % differ
    np.savez_compressed(OUT, **{k: a[k] for k in a.files})
    print("kept %d cases, %d bytes" % (len(pc.NAMES), os.path.getsize(OUT)))


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(sys.argv[2], sys.argv[3])
    else:
        record(sys.argv[1])
