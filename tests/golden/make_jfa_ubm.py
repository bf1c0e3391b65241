#!/usr/bin/env python3
"""The UBM the reference's JFA leg ships (src/jfa/models/ubm_means, ubm_variances, ubm_weights: 256 diagonal Gaussians in 13
dimensions, each table one line of text, the means and variances as supervectors -- sc_compute_suf_stats.m reshapes them to
dim x gaussians column by column, i.e. mixture-major) as float64 arrays in tests/golden/jfa_ubm.npz: ``means`` [256, 13],
``variances`` [256, 13] (VARIANCES, not standard deviations), ``weights`` [256].  Parameters only; the tests of the batched
Baum-Welch statistics (tests/test_bw_cpu.py, tests/test_gpu_bw_stats.py) draw their sessions from it.

    python tests/golden/make_jfa_ubm.py [directory of the three tables]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SRC = "/root/reference/src/jfa/models"


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else SRC
    w = np.loadtxt(os.path.join(src, "ubm_weights"), dtype=np.float64).reshape(-1)
    K = w.size
    m = np.loadtxt(os.path.join(src, "ubm_means"), dtype=np.float64).reshape(K, -1)
    v = np.loadtxt(os.path.join(src, "ubm_variances"), dtype=np.float64).reshape(K, -1)
    assert m.shape == v.shape == (256, 13) and np.all(v > 0) and np.all(w > 0) and abs(w.sum() - 1.0) < 1e-6
    out = os.path.join(ROOT, "tests", "golden", "jfa_ubm.npz")
    np.savez_compressed(out, means=m, variances=v, weights=w)
    print("wrote %s: %d x %d, %d bytes" % (out, m.shape[0], m.shape[1], os.path.getsize(out)))


if __name__ == "__main__":
    main()
