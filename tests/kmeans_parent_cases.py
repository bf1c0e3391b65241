"""The fits of tests/test_gpu_kmeans_parent_bits.py, of its recorder (tests/golden/make_kmeans_parent_bits.py) and of the host
check program's driver run (tests/test_kmeans_host_cpu.py): the smallest shapes that reach every branch of the start in front of
EM (csrc/kmeans_host.cpp over the device back end of csrc/kmeans_init.hip, planned by csrc/kmeans_plan.cpp) -- every instantiation
of the two nearest-centre kernels, the centre tail, the point tail, the worker blocks of the reference's sums, ties between
duplicate centres, the engine option and the random-frames start.  Each is a ``fit`` with ``nr_iteration = 0`` and a seed, a few
milliseconds; the data come from the integer hash of tests/em_parent_cases.py: the same bits under any numpy.  Plain module."""
import numpy as np

import em_parent_cases as ec

# name, n, K, D, concurrency, seed, init_with_kmeans, kmeans_assign_engine, kind of data
CASES = (
    # every instantiation: fast + exact <16>; <40>; exact <64> alone; <128>; two passes of the d0 loop.  700 points: two workgroups
    ("d16", 700, 5, 16, 3, 21, 1, 0, "blobs"),
    ("d13", 700, 5, 13, 3, 22, 1, 0, "blobs"),
    ("d17", 700, 5, 17, 3, 23, 1, 0, "blobs"),
    ("d40", 700, 5, 40, 3, 24, 1, 0, "blobs"),
    ("d41", 700, 5, 41, 3, 25, 1, 0, "blobs"),
    ("d64", 700, 5, 64, 3, 26, 1, 0, "blobs"),
    ("d65", 700, 5, 65, 3, 27, 1, 0, "blobs"),
    ("d128", 700, 5, 128, 3, 28, 1, 0, "blobs"),
    ("d130", 700, 5, 130, 3, 29, 1, 0, "blobs"),
    # the centre tail: one full chunk; a second chunk with one live centre; an odd chunk count; a single centre
    ("k16", 600, 16, 13, 4, 31, 1, 0, "blobs"),
    ("k17", 600, 17, 13, 4, 32, 1, 0, "blobs"),
    ("k33", 900, 33, 13, 4, 33, 1, 0, "blobs"),
    ("k1", 600, 1, 13, 4, 34, 1, 0, "blobs"),
    # the point tail: one workgroup's KM_PP * 256 points, one fewer, one more
    ("n511", 511, 4, 13, 2, 41, 1, 0, "blobs"),
    ("n512", 512, 4, 13, 2, 42, 1, 0, "blobs"),
    ("n513", 513, 4, 13, 2, 43, 1, 0, "blobs"),
    # worker blocks: one; many of odd sizes with clusters empty in most; a block above KM_BS_CHUNK; more workers than points
    ("conc1", 600, 6, 13, 1, 51, 1, 0, "blobs"),
    ("conc37_n3001", 3001, 20, 13, 37, 52, 1, 0, "blobs"),
    ("conc2_n9001", 9001, 8, 20, 2, 53, 1, 0, "blobs"),
    ("conc_above_n", 50, 3, 13, 64, 54, 1, 0, "blobs"),
    # 40 distinct rows, 50 times each, 48 centres: duplicate centres are certain (a model or the empty-cluster message)
    ("ties_k48", 2000, 48, 13, 5, 61, 1, 0, "ties"),
    # the exact pass alone on a shape the fast search would take
    ("d13_engine1", 700, 5, 13, 3, 22, 1, 1, "blobs"),
    # K random frames
    ("random_frames", 700, 7, 13, 3, 71, 0, 0, "blobs"),
)
NAMES = [c[0] for c in CASES]
BY_NAME = {c[0]: c for c in CASES}
HOST_NAMES = [c[0] for c in CASES if c[3] <= 64]             # what the host back end of tests/host/kmeans_checks.cpp runs


def frames(case):
    """-> float32 [n][D]"""
    _name, n, K, D, _conc, seed, _km, _eng, kind = case
    if kind == "ties":
        base = (2.0 * ec.noise(seed, (40, D))).astype(np.float32)
        return np.ascontiguousarray(np.repeat(base, n // 40, axis=0)[(np.arange(n) * 37 + 11) % n])     # 37 is coprime to 2000
    cent = 3.0 * ec.noise(seed, (K, D))
    own = (np.arange(n) * 7 + seed) % K
    return (cent[own] + ec.noise(seed + 1, (n, D))).astype(np.float32)


def run_case(case):
    """-> {suffix: array}: the model after the start alone (or the message of its refusal) and the deltas of the two counters"""
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.pygmm import GMM
    _name, _n, K, _D, conc, seed, km, eng, _kind = case
    X = frames(case)
    out = {}
    before = _lib.kmeans_fast_stats()
    try:
        _lib.set_option("kmeans_assign_engine", eng)
        g = GMM(nr_mixture=K, nr_iteration=0, init_with_kmeans=km, seed=seed, concurrency=conc)
        try:
            g.fit(X)
            out["weights"], out["means"], out["sigmas"] = g.params()
        except _lib.SRError as e:
            out["error"] = np.array(str(e))
    finally:
        _lib.set_option("kmeans_assign_engine", 0)
    after = _lib.kmeans_fast_stats()
    out["fast_stats"] = np.array([a - b for a, b in zip(after, before)], np.int64)       # passes, points rechecked
    return out
