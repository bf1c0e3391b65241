#!/usr/bin/env python3
"""What the iteration-at-a-time trainer (csrc/em.hip: train_em) computes, to the bit, at the commit BEFORE a change that must
not move it: run on an MI355X at that commit, twice,

    python tests/golden/make_em_parent_bits.py /tmp/a.npz && python tests/golden/make_em_parent_bits.py /tmp/b.npz
    python tests/golden/make_em_parent_bits.py --merge /tmp/a.npz /tmp/b.npz

The merge keeps the cases whose two recordings agree in every bit (and names the others) and writes
tests/golden/em_parent_bits.npz: per case of tests/em_parent_cases.py the iteration count(s), what sr_last_em_stats_engine()
reported, weights, means and sigmas as float64; once, the device's compute-unit count -- the launch geometry, and with it the
order of the sums, is a function of it, so tests/test_gpu_em_parent_bits.py compares on a device with that count only."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import em_parent_cases as ec  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "em_parent_bits.npz")


def record(path):
    from speaker_recognition_amd import _lib
    out = {"n_cu": np.array(int(re.search(r"(\d+) CUs", _lib.device_name()).group(1)), np.int64)}
    for case in ec.CASES:
        name, opt, kind, args, iters, threshold, _min_covar, eng = case
        got = ec.run_case(case)
        print("%-20s option %d: iterations %s, engine %s" % (name, opt, got["iterations"].tolist(), got["engine"].tolist()))
        assert eng is None or got["engine"].tolist() == [eng] * len(got["engine"]), (name, got["engine"])
        if name.startswith("split_stop"):
            assert got["iterations"].tolist() == [4], got["iterations"]        # stopped by the rule, at the check after iteration 3
        if kind == "map_far":
            X, ubm = ec._map_far_case(*args)
            n_weak = ec.unsupported(X, ubm)
            print("%-20s %d of %d mixtures without fp32 support under the UBM" % ("", n_weak, args[1]))
            assert n_weak > 0
        for k, v in got.items():
            out[name + "/" + k] = v
    np.savez_compressed(path, **out)


def merge(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files) and int(a["n_cu"]) == int(b["n_cu"])
    out, kept = {"n_cu": a["n_cu"]}, []
    for case in ec.CASES:
        keys = [k for k in a.files if k.startswith(case[0] + "/")]
        if all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in keys):
            kept.append(case[0])
            out.update({k: a[k] for k in keys})
        else:
            print("DROPPED (the two recordings differ):", case[0], [k for k in keys if not np.array_equal(a[k], b[k])])
    out["cases"] = np.array(kept)
    np.savez_compressed(OUT, **out)
    print("kept %d of %d cases, %d CUs, %d bytes" % (len(kept), len(ec.CASES), int(a["n_cu"]), os.path.getsize(OUT)))


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(sys.argv[2], sys.argv[3])
    else:
        record(sys.argv[1])
