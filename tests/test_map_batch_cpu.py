"""Batched MAP enrolment without a GPU (sr_map_fit_batch, GMMSet.fit_many; csrc/map_batch.hip, csrc/map_plan.cpp): the symbols and
their binding, every argument refusal (all made before the device is touched, so they answer here), the loud failure without a
device, the plan -- routes, groups, tile tables, grids -- against a restatement in this file and under the host sanitizers
(tests/host/map_checks.cpp), the host-side checks of GMMSet.fit_many, and the batched kernels' scratch."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")
K, D = 40, 5


def _ubm(lib, K=K, D=D):
    rng = np.random.default_rng(3)
    w, mu, sg = np.full(K, 1.0 / K), rng.normal(size=(K, D)), np.full((K, D), 0.9)
    from speaker_recognition_amd import _lib
    h = lib.sr_gmm_from_arrays(K, D, _lib.as_dp(w), _lib.as_dp(np.ascontiguousarray(mu)), _lib.as_dp(sg))
    assert h
    return C.c_void_p(h)


def _call(lib, handles, ns, ubm, X=None, D=D, offsets=None, S=None, param=True, iters=True, status=True, models=True):
    """sr_map_fit_batch on `handles` with ns[s] rows per speaker -> (return value, message, status)"""
    from speaker_recognition_amd import _lib
    n_spk = len(handles)
    off = np.zeros(len(ns) + 1, dtype=np.int64)
    off[1:] = np.cumsum(ns)
    if offsets is not None:
        off = np.asarray(offsets, dtype=np.int64)
    if X is None:
        X = np.random.default_rng(0).normal(size=(max(1, int(max(off))), D))
    X = np.ascontiguousarray(X, dtype=np.float32)
    p = _lib.Parameter()
    p.nr_iteration, p.threshold, p.min_covar = 5, 0.01, 1e-3
    it = np.zeros(max(1, n_spk), dtype=np.int32)
    st = np.full(max(1, n_spk), 77, dtype=np.int32)
    arr = (C.c_void_p * max(1, n_spk))(*[h.value for h in handles])
    rc = lib.sr_map_fit_batch(arr if models else None, n_spk if S is None else S, ubm, _lib.as_fp(X), _lib.as_i64p(off), D,
                              C.byref(p) if param else None, 7, _lib.as_i32p(it) if iters else None, _lib.as_i32p(st) if status else None)
    return rc, lib.sr_last_error().decode(), st


def test_symbols_exported_and_bound(built_lib):
    from speaker_recognition_amd import _lib
    for name in ("sr_map_fit_batch", "sr_map_fit_batch_error", "sr_map_fit_batch_stats", "sr_map_fit_batch_bytes", "sr_map_fit_plan"):
        assert name in _lib.EXT_SYMBOLS
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    fn = _lib.lib().sr_map_fit_batch
    assert fn.restype is C.c_int
    # GMM *const *models, int S, GMM *ubm, const float *X, const int64_t *row_offsets, int dim, param *, long seed, int *, int *
    assert list(fn.argtypes) == [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int64), C.c_int,
                                 C.POINTER(_lib.Parameter), C.c_long, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    assert _lib.lib().sr_map_fit_batch_error.restype is C.c_char_p
    assert _lib.lib().sr_map_fit_batch_bytes.restype is C.c_long


def test_declared_signatures_in_the_header():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "pygmm_hip.h")).read())
    assert ("int sr_map_fit_batch(GMM *const *models, int S, GMM *ubm, const float *X, const int64_t *row_offsets, int dim, "
            "const struct Parameter *param, long seed, int *iterations_out, int *status);") in text
    assert "const char *sr_map_fit_batch_error(int s);" in text
    assert ("void sr_map_fit_batch_stats(long *calls, long *speakers_batched, long *speakers_single, long *speakers_handed_over, "
            "long *passes);") in text
    assert "long sr_map_fit_batch_bytes(void);" in text
    assert "map_fit_batch_bytes" in text and "int sr_map_fit_plan(" in text


def test_counters_take_null_pointers(built_lib):
    from speaker_recognition_amd import _lib
    built_lib.sr_map_fit_batch_stats(None, None, None, None, None)
    assert all(v >= 0 for v in _lib.map_fit_batch_stats()) and len(_lib.map_fit_batch_stats()) == 5


def test_bad_arguments_fail_before_the_device(built_lib):
    """every case returns -1 with a message naming the problem; none needs a GPU (the checks precede the first device call)"""
    from speaker_recognition_amd import _lib
    before = _lib.map_fit_batch_stats()
    ubm = _ubm(built_lib)
    hs = [C.c_void_p(built_lib.new_gmm(K, 1)) for _ in range(3)]
    untrained = C.c_void_p(built_lib.new_gmm(K, 1))
    try:
        for kw in (dict(models=False), dict(param=False), dict(iters=False), dict(status=False)):
            rc, msg, _ = _call(built_lib, hs, [10, 10, 10], ubm, **kw)
            assert rc == -1 and "null argument" in msg, (kw, msg)
        rc, msg, _ = _call(built_lib, hs, [10, 10, 10], None)
        assert rc == -1 and "null argument" in msg, msg
        rc, msg, _ = _call(built_lib, [hs[0], C.c_void_p(None), hs[1]], [10, 10, 10], ubm)
        assert rc == -1 and "null GMM handle" in msg and "speaker 1" in msg, msg
        rc, msg, _ = _call(built_lib, [], [], ubm, S=0)
        assert rc == -1 and "at least one speaker" in msg, msg
        rc, msg, _ = _call(built_lib, hs, [10, 10, 10], ubm, offsets=[0, 20, 10, 30])
        assert rc == -1 and "must not decrease" in msg and "speaker 1" in msg, msg
        rc, msg, _ = _call(built_lib, hs, [10, 10, 10], ubm, offsets=[5, 15, 25, 35])
        assert rc == -1 and "must start at 0" in msg, msg
        rc, msg, _ = _call(built_lib, hs, [10, 10, 10], untrained)
        assert rc == -1 and "UBM has no parameters" in msg, msg
        rc, msg, _ = _call(built_lib, hs, [10, 10, 10], ubm, D=D + 1)
        assert rc == -1 and "UBM dim %d != data dim %d" % (D, D + 1) in msg, msg
        rc, msg, _ = _call(built_lib, [hs[0], hs[1], hs[0]], [10, 10, 10], ubm)
        assert rc == -1 and "twice" in msg, msg
        rc, msg, _ = _call(built_lib, [hs[0], ubm], [10, 10], ubm)
        assert rc == -1 and "is the UBM's" in msg, msg
    finally:
        for h in hs + [untrained, ubm]:
            built_lib.sr_free_gmm(h)
    # none of them counted: the counters move only once the arguments have passed and the device is there
    assert _lib.map_fit_batch_stats() == before


def test_valid_batch_fails_loudly_without_a_gpu(built_lib):
    """No CPU path: the contract of test_abi_cpu.py::test_compute_fails_loudly_without_gpu."""
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.gmmset import GMMSet
    from speaker_recognition_amd.pygmm import GMM
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    before = _lib.map_fit_batch_stats()
    ubm = _ubm(built_lib)
    hs = [C.c_void_p(built_lib.new_gmm(K, 1)) for _ in range(2)]
    try:
        rc, msg, _ = _call(built_lib, hs, [200, 300], ubm)
        assert rc == -1 and "no HIP device" in msg, msg
        assert built_lib.get_dim(hs[0]) == 0                                              # still without parameters
    finally:
        for h in hs + [ubm]:
            built_lib.sr_free_gmm(h)
    rng = np.random.default_rng(0)
    gs = GMMSet(ubm=GMM.from_arrays(np.full(K, 1.0 / K), rng.normal(size=(K, D)), np.full((K, D), 0.9)))
    with pytest.raises(_lib.SRError, match="no HIP device"):
        gs.fit_many([rng.normal(size=(200, D)), rng.normal(size=(100, D))], ["a", "b"])
    assert gs.gmms == [] and gs.y == []
    assert _lib.map_fit_batch_stats() == before


def test_option_is_checked(built_lib):
    from speaker_recognition_amd import _lib
    assert built_lib.sr_set_option(b"map_fit_batch_bytes", 0) == -1
    assert b"map_fit_batch_bytes" in built_lib.sr_last_error()
    default = _lib.map_fit_batch_bytes()
    assert default == 1 << 30                                                             # (include/pygmm_hip.h)
    try:
        assert built_lib.sr_set_option(b"map_fit_batch_bytes", 12345) == 0 and _lib.map_fit_batch_bytes() == 12345
    finally:
        assert built_lib.sr_set_option(b"map_fit_batch_bytes", default) == 0


# ---- the plan against a restatement: train_em's engine choice and train_em_f64's shapes, written out again ----

def _small_grid(K, D, n):
    R = K * (D + 1)
    for fr in (128, 64):
        if fr > 64 and -(-n // (fr // 2)) == -(-n // fr):
            continue
        seg = 1
        while seg * 2 <= fr // 64 and R * seg * 2 <= 1024:
            seg *= 2
        lds = (3 * K + 3 * K * D + K * fr + 1024 + fr + K * (2 * D + 1) + 2 + 2 * R * seg) * 8 + fr * (D + 1) * 4
        if lds > 150 * 1024:
            continue
        return -(-n // fr)
    return 0


def _route(K, D, n, n_cu=256, nit=200, verbosity=0):
    if n == 0:
        return -1
    small = (1 <= K <= 32 and 1 <= D <= 40 and 1 <= n <= 8192 and 1 <= _small_grid(K, D, n) <= n_cu // 2 and nit >= 1 and verbosity < 2)
    f64 = (K >= 1 and 1 <= D <= 64 and 1 <= n <= 8192 and nit >= 1 and verbosity < 2
           and (-(-K // 64) * 64) * (-(-n // 128) * 128) <= 32 << 20)
    return 0 if f64 and not small else 1


def _scratch(K, D, n):
    n_kb, n_pad = -(-K // 64), -(-n // 128) * 128
    n_chunks = n_pad // 64
    return 8 * (n_kb * 64 * n_pad + 2 * n_kb * n_pad + n_chunks * K * (2 * D + 1) + n_pad + 2 * n_chunks + 4 + K * D)


def _groups(K, D, lengths, bound, n_cu=256):
    """[(first speaker, speakers)] of the batched speakers in call order"""
    out, cur, used = [], [], 0
    for s, n in enumerate(lengths):
        if _route(K, D, n, n_cu) != 0:
            continue
        b = _scratch(K, D, n)
        if cur and used + b > bound:
            out.append((cur[0], len(cur)))
            cur, used = [], 0
        cur.append(s)
        used += b
    if cur:
        out.append((cur[0], len(cur)))
    return out


def test_routes_equal_the_restatement(built_lib):
    from speaker_recognition_amd import _lib
    ns = [0, 1, 64, 128, 129, 8192, 8193]
    for Kx in (1, 32, 33, 64, 65, 2048):
        for Dx in (1, 40, 41, 64, 65):
            for n_cu in (256, 8):
                p = _lib.map_fit_plan(Kx, Dx, ns, n_cu=n_cu)
                want = [_route(Kx, Dx, n, n_cu) for n in ns]
                assert p["routes"].tolist() == want, (Kx, Dx, n_cu, p["routes"].tolist(), want)
                assert (p["n_batched"], p["n_single"], p["n_error"]) == (want.count(0), want.count(1), want.count(-1))
    # what the routes are at the shapes that matter: a speaker-sized model is the whole-fit kernel's, a large UBM's speaker the batch's
    assert _route(32, 40, 3000) == 1 and _route(33, 40, 3000) == 0 and _route(512, 39, 3000) == 0 and _route(2048, 39, 8193) == 1
    assert _route(2048, 65, 3000) == 1 and _route(8, 13, 300) == 1
    # the trace of verbosity 2 is the iteration-at-a-time path's
    assert _lib.map_fit_plan(512, 39, [3000, 100], verbosity=2)["routes"].tolist() == [1, 1]


def test_groups_and_scratch_equal_the_restatement(built_lib):
    from speaker_recognition_amd import _lib
    Kx, Dx = 130, 13
    lengths = [300, 1, 63, 64, 65, 0, 127, 128, 129, 300, 8193, 300]
    one = _scratch(Kx, Dx, 300)
    for bound in (1, one, one - 1, 2 * one, 1 << 30):
        p = _lib.map_fit_plan(Kx, Dx, lengths, scratch_bytes=bound)
        assert [(int(g[0]), int(g[1])) for g in p["groups"]] == _groups(Kx, Dx, lengths, bound), bound
        for s, n in enumerate(lengths):
            if p["routes"][s] == 0:
                assert p["scratch"][s] == _scratch(Kx, Dx, n) and p["n_pad"][s] == -(-n // 128) * 128
                assert p["n_chunks_of"][s] == p["n_pad"][s] // 64
            else:
                assert p["group"][s] == -1 and p["scratch"][s] == 0
        for g in p["groups"]:
            members = [s for s in range(len(lengths)) if p["group"][s] == len([h for h in p["groups"] if h[0] < g[0]])]
            assert g[4] == sum(_scratch(Kx, Dx, lengths[s]) for s in members)
            assert g[4] <= bound or g[1] == 1                       # a speaker above the bound is a group of its own
        assert p["max_group_bytes"] == max(int(g[4]) for g in p["groups"])
    assert _lib.map_fit_plan(Kx, Dx, lengths, scratch_bytes=1)["n_groups"] == 10
    assert _lib.map_fit_plan(Kx, Dx, lengths, scratch_bytes=1 << 30)["n_groups"] == 1
    with pytest.raises(_lib.SRError, match="map_fit_batch_bytes must be >= 1"):
        _lib.map_fit_plan(Kx, Dx, lengths, scratch_bytes=0)
    with pytest.raises(_lib.SRError, match="negative length"):
        _lib.map_fit_plan(Kx, Dx, [5, -2])


def test_tile_tables_of_ragged_lengths(built_lib):
    """one row per 128-frame density tile and per 64-frame chunk, counted from the speaker's own first frame, the padding after its
    own last frame: train_em_f64's n_pad and n_chunks per speaker, so every sum has the single fit's order"""
    from speaker_recognition_amd import _lib
    Kx, Dx = 65, 13
    lengths = [1, 63, 0, 64, 65, 127, 128, 129, 300, 8193, 5]
    first = np.concatenate([[0], np.cumsum(lengths)])
    for bound in (1, 1 << 30):
        p = _lib.map_fit_plan(Kx, Dx, lengths, scratch_bytes=bound)
        want_t, want_c = [], []
        for s, n in enumerate(lengths):
            if _route(Kx, Dx, n) != 0:
                continue
            n_pad = -(-n // 128) * 128
            want_t += [(s, first[s], t) for t in range(n_pad // 128)]
            want_c += [(s, first[s], c) for c in range(n_pad // 64)]
        assert [tuple(r) for r in p["tiles"].tolist()] == want_t
        assert [tuple(r) for r in p["chunks"].tolist()] == want_c
        assert p["n_kb"] == 2 and p["n_tiles"] == len(want_t) and p["n_chunks"] == len(want_c)
        # grids: x = the group's rows, y = the mixture blocks
        assert sum(int(g[2]) for g in p["groups"]) == len(want_t) and sum(int(g[3]) for g in p["groups"]) == len(want_c)
        assert all(1 <= g[3] < 2 ** 31 for g in p["groups"]) and p["n_kb"] <= 65535
    assert p["lds_density"] == (2 * 64 * Dx + 64 + 4 * 128) * 8 + 128 * (Dx + 1) * 4
    assert p["lds_stats"] == (64 * 64 + 64 * Dx) * 8 + 64 * (Dx + 1) * 4


def test_documented_sets(built_lib):
    """under the default bound of 1 GiB the 200 speakers of configs[2] (512 x 39, 3000 frames) are 6 groups, the 1000
    speakers of configs[3] (2048 x 39) are 112"""
    from speaker_recognition_amd import _lib
    p = _lib.map_fit_plan(512, 39, [3000] * 200)
    assert (1 << 30) // _scratch(512, 39, 3000) == 37 and p["n_groups"] == 6 and p["n_batched"] == 200
    assert [int(g[1]) for g in p["groups"]] == [37] * 5 + [15]
    assert int(p["groups"][0][2]) == 37 * 24 and p["n_kb"] == 8          # 888 x 8 density workgroups a launch instead of 24 x 8
    p = _lib.map_fit_plan(2048, 39, [3000] * 1000)
    assert (1 << 30) // _scratch(2048, 39, 3000) == 9 and p["n_groups"] == 112 and p["n_kb"] == 32
    assert int(p["groups"][0][2]) == 9 * 24


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_map_plan_under_asan_ubsan(tmp_path):
    """The plan -- routes, groups, slices, tables, refusals -- swept over shapes, ragged sets, bounds and device sizes by a
    stand-alone program (tests/host/map_checks.cpp) built with AddressSanitizer + UBSan: host code only, no GPU, nothing loaded
    into Python."""
    exe = str(tmp_path / "map_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "host", "map_checks.cpp"), os.path.join(CSRC, "map_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "map checks ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_fit_many_checks_its_lists_on_the_host(built_lib, monkeypatch):
    from speaker_recognition_amd.gmmset import GMMSet
    rng = np.random.default_rng(0)
    X = rng.normal(size=(50, 3))
    with pytest.raises(ValueError, match="1 matrices but 2 labels"):
        GMMSet(2).fit_many([X], ["a", "b"])
    # without a UBM: the loop of fit_new, in order (no device)
    gs = GMMSet(2)
    seen = []
    monkeypatch.setattr(gs, "fit_new", lambda x, label: seen.append((label, np.asarray(x).shape)))
    gs.fit_many([X, X[:20]], ["a", "b"])
    assert seen == [("a", (50, 3)), ("b", (20, 3))]
    # GMMSet.fit pools by label first, then fit_many
    seen.clear()
    gs.fit([X[:10], X[10:30], X[30:]], ["a", "b", "a"])
    assert seen == [("a", (30, 3)), ("b", (20, 3))]
    gs.fit_many([], [])
    assert len(seen) == 2


def _kernel_resources(name):
    path = os.path.join(ROOT, "speaker-recognition_amd", "build", name + ".resources")
    assert os.path.exists(path), "the build did not leave %s" % path
    out, cur = {}, None
    for line in open(path):
        m = re.search(r" Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur is not None:
            cur["scratch"] = int(m.group(1))
    return out


def test_batched_kernels_have_no_scratch(built_lib):
    res = _kernel_resources("map_batch")
    for stem in ("mapb_derive", "mapb_init", "mapb_density", "mapb_lse", "mapb_stats", "mapb_head", "mapb_mstep"):
        names = [n for n in res if stem + "_kernel" in n]
        assert len(names) == 1 and res[names[0]]["scratch"] == 0, (stem, names, res)
    # the single fit's kernels run the same bodies (csrc/em_f64_dev.hpp) and did not start spilling either
    single = _kernel_resources("em_f64")
    assert len(single) >= 7 and all(v["scratch"] == 0 for v in single.values()), single
