#!/usr/bin/env python3
"""What the start in front of EM (k-means|| + weighted k-means++ + the two Lloyd stages, or K random frames) computes, to the bit,
at the commit BEFORE a change that must not move it: run on an MI355X at that commit, twice,

    python tests/golden/make_kmeans_parent_bits.py /tmp/a.npz && python tests/golden/make_kmeans_parent_bits.py /tmp/b.npz
    python tests/golden/make_kmeans_parent_bits.py --merge /tmp/a.npz /tmp/b.npz

The merge requires the two recordings to agree in every bit of every case and only then writes
tests/golden/kmeans_parent_bits.npz: per case of tests/kmeans_parent_cases.py the weights, means and sigmas as float64 (or the
message of the refusal) and the deltas of kmeans_fast_stats() -- passes taken the fast way, points left to the exact pass (the SET
of those points is a function of the data; only the order of the list is not)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kmeans_parent_cases as pc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "kmeans_parent_bits.npz")


def record(path):
    out = {}
    for case in pc.CASES:
        got = pc.run_case(case)
        print("%-16s fast passes %d, rechecked %d, %s" % (case[0], got["fast_stats"][0], got["fast_stats"][1],
                                                          got["error"] if "error" in got else "means sum %.17g" % got["means"].sum()))
        for k, v in got.items():
            out[case[0] + "/" + k] = v
    np.savez_compressed(path, **out)


def merge(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files)
    differ = [k for k in a.files if a[k].dtype != b[k].dtype or not np.array_equal(a[k], b[k])]
    assert not differ, "the two recordings differ: %s" % differ
    np.savez_compressed(OUT, **{k: a[k] for k in a.files})
    print("kept %d cases, %d bytes" % (len(pc.CASES), os.path.getsize(OUT)))


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(sys.argv[2], sys.argv[3])
    else:
        record(sys.argv[1])
