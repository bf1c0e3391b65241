#!/usr/bin/env python3
"""What the float64 full-covariance EM driver (fe_fit_group) computes, to the bit, at the commit BEFORE a change that must not
move it: run on an MI355X at that commit, twice,

    python tests/golden/make_fullfit_parent_bits.py /tmp/a.npz && python tests/golden/make_fullfit_parent_bits.py /tmp/b.npz
    python tests/golden/make_fullfit_parent_bits.py --merge /tmp/a.npz /tmp/b.npz

The merge keeps the cases whose two recordings agree in every bit (and names the others) and writes
tests/golden/fullfit_parent_bits.npz: per case of tests/fullfit_parent_cases.py and per fitted model n_iter, converged,
lower_bound, weights and means as float64 and a SHA-256 each of precisions_cholesky_ and covariances_ (the arrays at D = 64 would
not fit a committed fixture); per batch the three sr_full_fit_batch_stats deltas; once, the device's compute-unit count (the fit's
own launch geometry does not depend on it, the k-means start's may).  The fit has no device atomics: every case is expected to be
kept, and tests/test_gpu_fullfit_parent_bits.py asserts that it was."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fullfit_parent_cases as pc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fullfit_parent_bits.npz")


def record(path):
    from speaker_recognition_amd import _lib
    out = {"n_cu": np.array(int(re.search(r"(\d+) CUs", _lib.device_name()).group(1)), np.int64)}
    for name in pc.CASES:
        got = pc.run_case(name)
        if name.startswith("row/"):
            print("%-28s n_iter %d converged %d bound %.17g" % (name, got["n_iter"], got["converged"], got["lower_bound"]))
        else:
            print("%-28s stats %s, failed %s" % (name, got["stats"].tolist(), [k for k in got if k.endswith("/error")]))
        for k, v in got.items():
            out[name + "/" + k] = v
    np.savez_compressed(path, **out)


def merge(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files) and int(a["n_cu"]) == int(b["n_cu"])
    out, kept = {"n_cu": a["n_cu"]}, []
    for name in pc.CASES:
        keys = [k for k in a.files if k.startswith(name + "/")]
        if all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in keys):
            kept.append(name)
            out.update({k: a[k] for k in keys})
        else:
            print("DROPPED (the two recordings differ):", name, [k for k in keys if not np.array_equal(a[k], b[k])])
    out["cases"] = np.array(kept)
    np.savez_compressed(OUT, **out)
    print("kept %d of %d cases, %d CUs, %d bytes" % (len(kept), len(pc.CASES), int(a["n_cu"]), os.path.getsize(OUT)))


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(sys.argv[2], sys.argv[3])
    else:
        record(sys.argv[1])
