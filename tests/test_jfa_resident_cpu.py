"""CPU side of the resident JFA route (csrc/jfa_stats.hip, the centring plan of csrc/jfa_plan.cpp, jfa.Stats / jfa.centred): the
symbols, the refusals that need no device, the centring plan (sr_jfa_centre_plan -- also under the host sanitizers,
tests/host/jfa_centre_checks.cpp), the kernels' resource records, that the host-array routes reach nothing new, the refusal in a
forked child, and that the centring gate of tests/jfa_resident_cases.py fits its float64 reference.

The refusals that need a live statistics handle (labels outside 0 .. n_labels - 1, an E or m of another size, half of a pair, rows
outside the handle) are in tests/test_gpu_jfa_resident.py: without a device no handle can be made."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfa_cases as jc  # noqa: E402
import jfa_resident_cases as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")
NEW = ["sr_bw_stats_resident", "sr_stats_from_host", "sr_stats_info", "sr_stats_get", "sr_stats_take", "sr_stats_close",
       "sr_jfa_open_centred", "sr_jfa_statistics", "sr_jfa_centre_plan", "sr_jfa_zd", "sr_jfa_score_integrated_stats",
       "sr_jfa_score_linear_stats"]


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def test_symbols_exported_declared_and_listed(built_lib):
    from speaker_recognition_amd import _lib
    header = open(os.path.join(ROOT, "include", "pygmm_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), "lib/pygmm.so does not export %s" % name
        assert re.search(r"\b(int|void|SRJfa \*|SRStats \*)\s?%s\(" % name, header), "%s is not declared in include/pygmm_hip.h" % name
        assert name in _lib.EXT_SYMBOLS
    assert "typedef struct SRStats SRStats;" in header and "SR_T_COUNT 20" in header


def test_refusals_need_no_device(built_lib):
    """Every refusal that can be reached without a live handle fails on its arguments alone, by a text that names the argument --
    never the device."""
    from speaker_recognition_amd import _lib, jfa
    L = built_lib
    n, K, D = 3, 2, 2
    N, F = np.ones((n, K)), np.zeros((n, K * D))
    E, m = np.ones(K * D), np.zeros(K * D)
    ids = np.zeros(n, dtype=np.int64)

    def bad(arr, idx, value):
        out = np.array(arr)
        out.flat[idx] = value
        return out

    def refused(status, pat):
        err = _lib.last_error()
        assert status in (None, -1) and re.search(pat, err) and "HIP" not in err, (status, err)

    # the statistics, validated before the device is touched, by the texts of sr_jfa_open
    for args, pat in (((0, K, D, _dp(N), _dp(F)), "G, K, D >= 1"), ((n, 0, D, _dp(N), _dp(F)), "G, K, D >= 1"),
                      ((n, K, D, None, _dp(F)), "null argument"), ((n, K, D, _dp(N), None), "null argument"),
                      ((n, K, D, _dp(bad(N, 3, np.nan)), _dp(F)), "N holds a non-finite value at element 3"),
                      ((n, K, D, _dp(N), _dp(bad(F, 5, -np.inf))), "F holds a non-finite value at element 5"),
                      ((n, K, D, _dp(bad(N, 4, -0.5)), _dp(F)), "negative occupancy at group 2, mixture 0")):
        refused(L.sr_stats_from_host(*args), pat)
    # a NULL handle and a closed one (the registry of live handles is asked; the pointer is never followed)
    info = (C.c_int64 * 4)()
    rows = np.zeros(1, dtype=np.int64)
    out = np.zeros((1, n))
    y, v = np.zeros((1, 1)), np.zeros((1, K * D))
    for h, pat in ((None, "null statistics handle"), (C.c_void_p(0x1000), "the statistics handle is closed")):
        refused(L.sr_stats_info(h, info, 4), "sr_stats_info: " + pat)
        refused(L.sr_stats_get(h, _dp(N), _dp(F)), "sr_stats_get: " + pat)
        refused(L.sr_stats_take(h, _ip(rows), 1), "sr_stats_take: " + pat)
        refused(L.sr_jfa_open_centred(h, _dp(E), _dp(m), 0, _ip(ids), 1, None, None, None, 0, None, None, 0, None), "sr_jfa_open_centred: " + pat)
        refused(L.sr_jfa_score_integrated_stats(h, 1, 1, 1, _dp(m), _dp(E), None, _dp(v), _dp(v), None, _dp(y), None, 0, 0, _dp(out), None, None),
                "sr_jfa_score_integrated_stats: " + pat)
        refused(L.sr_jfa_score_linear_stats(h, 1, 1, 1, _dp(m), _dp(E), None, _dp(v), _dp(v), None, _dp(y), _dp(y), None, 0, 0, _dp(out), None),
                "sr_jfa_score_linear_stats: " + pat)
    L.sr_stats_close(None)                                           # harmless, both
    L.sr_stats_close(C.c_void_p(0x1000))
    refused(L.sr_jfa_statistics(None, _dp(N), _dp(F)), "sr_jfa_statistics: null argument")
    refused(L.sr_jfa_zd(None, _dp(E), 1, None, None, None), "sr_jfa_zd: null argument")
    # the shape, the ranks and the bound, through the plan
    plan = (C.c_int64 * 16)()
    for args, pat in (((0, 1, K, D, 0, 0, 0, 1 << 30), "G, K, D >= 1"), ((n, 0, K, D, 0, 0, 0, 1 << 30), "n_labels is 0"),
                      ((n, 1, K, D, 0, 0, 2, 1 << 30), "the mode is 0"), ((n, 1, K, D, 513, 0, 0, 1 << 30), "1 .. 512 factors, Ry is 513"),
                      ((n, 1, K, D, 0, 513, 1, 1 << 30), "1 .. 512 factors, Ru is 513"), ((n, 1, K, D, -1, 0, 0, 1 << 30), "Ry is -1"),
                      ((210, 70, 17, 39, 17, 5, 0, 64 * 17 * 39 * 8 - 1), "below one chunk of .* raise the option jfa_scratch_mib")):
        refused(L.sr_jfa_centre_plan(*args, plan, 16), pat)
    assert L.sr_jfa_centre_plan(n, 1, K, D, 0, 0, 0, 1 << 30, plan, 15) == -1 and "16 fields" in _lib.last_error()
    assert L.sr_jfa_centre_plan(n, 1, K, D, 0, 0, 0, 1 << 30, None, 16) == -1 and "null argument" in _lib.last_error()
    assert L.sr_jfa_centre_plan(n, 1, K, D, 512, 512, 1, 1 << 30, plan, 16) == 16
    # the Python layer
    with pytest.raises(ValueError, match=r"expected N \[n, K\] and F \[n, K \* D\]"):
        jfa.Stats.from_arrays(N, F[:, :3])
    with pytest.raises(TypeError, match="centred takes a Stats"):
        jfa.centred((F, N), m, E, ids)
    if _lib.device_count() == 0:                       # and a valid call says what is missing: no CPU path
        assert L.sr_stats_from_host(n, K, D, _dp(N), _dp(F)) is None and "no HIP device" in _lib.last_error()
        with pytest.raises(_lib.SRError, match="no HIP device"):
            jfa.Stats.from_arrays(N, F)
        with pytest.raises(_lib.SRError, match="no HIP device"):
            jfa.compute_suf_stats([np.zeros((5, 2))], (np.array([0.5, 0.5]), np.zeros((2, 2)), np.ones((2, 2))), resident=True)


def test_centre_plan_chunks_and_bytes(built_lib):
    from speaker_recognition_amd import _lib
    for n in (1, 63, 64, 65, 210, 1000):
        for K, D in ((3, 3), (5, 39), (17, 13), (17, 39), (512, 39)):
            row = K * D * 8
            for Ru in (0, 5, 16):
                for bound in (min(n, 64) * row, 64 * row + 1, 1 << 20, 1 << 30):
                    if Ru and bound // row < min(n, 64):
                        continue
                    chunks = set()
                    for groups in ("speakers", "sessions"):
                        for n_labels, Ry in ((1, 0), (n, 17), (3 * n, 65)):
                            p = _lib.jfa_centre_plan(n, n_labels, K, D, Ry, Ru, groups, bound)
                            chunk, nc = p["chunk"], p["n_chunks"]
                            assert 1 <= chunk <= n and nc == -(-n // chunk) and (nc - 1) * chunk < n <= nc * chunk        # every session once
                            assert p["bytes_scratch"] == (chunk * row if Ru else 0) and p["bytes_scratch"] <= bound      # the bound holds
                            assert nc == 1 or chunk % p["row_tile"] == 0
                            assert p["vec"] == (2 if (K * D) % 2 == 0 else 1) and p["centre_y"] == -(-(K * D // p["vec"]) // 256)
                            assert p["bytes_Fc"] == (n if groups == "sessions" else min(n, n_labels)) * row
                            chunks.add(chunk)
                    assert len(chunks) == 1                   # a function of n, K D and the bound only
    # the shape of the bit-identity test: 210 sessions x (17 x 39), a product of 1.1 MB
    assert _lib.jfa_centre_plan(210, 70, 17, 39, 0, 5, "speakers", 1 << 20)["n_chunks"] == 2
    assert _lib.jfa_centre_plan(210, 70, 17, 39, 0, 5, "speakers", 1 << 30)["n_chunks"] == 1
    assert _lib.jfa_centre_plan(210, 70, 17, 39, 0, 0, "speakers", 1 << 20)["n_chunks"] == 1


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_centre_plan_under_asan_ubsan(tmp_path):
    """The same sweep and the refusals' texts by a stand-alone program (tests/host/jfa_centre_checks.cpp) built with
    AddressSanitizer + UBSan: host code only, no GPU, nothing loaded into Python."""
    exe = str(tmp_path / "jfa_centre_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "host", "jfa_centre_checks.cpp"), os.path.join(CSRC, "jfa_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "jfa centre checks ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_jfa_stats_kernels_do_not_spill(built_lib):
    import test_abi_cpu
    res = test_abi_cpu._kernel_resources("jfa_stats")
    names = " ".join(res)
    for kernel in ("jfa_stats_check_kernel", "jfa_take_kernel", "jfa_group_counts_kernel", "jfa_centre_kernelILi1E", "jfa_centre_kernelILi2E",
                   "jfa_zd_kernel", "jfa_segment_totals_kernel"):
        assert kernel in names
    for name, r in res.items():
        assert r["scratch"] == 0, (name, r)


class _HostEstimator:
    """jfa.FactorEstimator with the device replaced by the restatement (as tests/test_jfa_cpu.py's, without its record of calls)."""

    def __init__(self, N, Fc, E):
        self.N, self.Fc, self.E = np.array(N), np.array(Fc), np.array(E)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def factors(self, W, accumulate=False):
        y, A, Cm = jc.factors(self.N, self.Fc, self.E, np.asarray(W, dtype=np.float64))
        return (y, A, Cm) if accumulate else y

    def train(self, W, n_iter):
        W, y, _ = jc.train(self.N, self.Fc, self.E, np.asarray(W, dtype=np.float64), n_iter)
        return W, y


def test_host_array_routes_reach_nothing_new(built_lib, monkeypatch):
    """train_v / train_u / train_d, estimate_* and score_* with host arrays call no sr_stats_*, sr_jfa_open_centred, sr_jfa_zd,
    sr_jfa_statistics or *_stats scorer (the device work of the factor handle is replaced by the restatement, as in
    test_python_layer_centring_labels_and_scalars, so that the whole chain runs without a device)."""
    from speaker_recognition_amd import _lib, jfa
    called = []

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            called.append(name)
            return getattr(self._lib, name)

    monkeypatch.setattr(_lib, "_lib", Spy(_lib.lib()))
    monkeypatch.setattr(jfa, "FactorEstimator", _HostEstimator)
    monkeypatch.setattr(jfa, "update_loadings", lambda A, Cm, W, return_skipped=False: jc.update(A, Cm, np.broadcast_to(W, Cm.shape))[0])
    G, K, D, R = 6, 4, 3, 5
    c = jc.corpus(G, K, D, R, 9)
    F, N, ids, m, E = c["F"], c["N"], c["spk_ids"], c["m"], c["E"]
    ubm = (np.full(K, 1.0 / K), m.reshape(K, D), E.reshape(K, D))
    v = jfa.train_v(F, N, ids, ubm, ny=3, niter=1)
    u = jfa.train_u(F, N, ids, ubm, v, nx=2, niter=1, seed=1)
    d = jfa.train_d(F, N, ids, ubm, v, u, niter=1, seed=2)
    y = jfa.estimate_y_and_v(F, N, None, m, E, d, v, u, 0, 0, 0, ids, nargout=3)[0]
    x = jfa.estimate_x_and_u(F, N, None, m, E, d, v, u, 0, y, 0, ids, nargout=2)[0]
    z = jfa.estimate_z_and_d(F, N, None, m, E, d, v, u, 0, y, x, ids, nargout=3)[0]
    jfa.linear_scoring(F, N, None, m, E, d, v, u, z, y, x)
    jfa.score_dot_product({"F": F[0::3], "N": N[0::3]}, (F[1::3], N[1::3]), ubm, v, u, d)
    for call in (lambda: jfa.score_integrated((F[0::3], N[0::3]), (F[1::3], N[1::3]), ubm, v, u, d),
                 lambda: jfa.score_trials(F, N, m, E, d, v, u, z, y, x, mode="linear"),
                 lambda: jfa.kscore_famous_19(F.T, N.T, None, m, E, d, v.T, u.T, z.T, y.T)):
        if _lib.device_count() == 0:
            with pytest.raises(_lib.SRError, match="no HIP device"):
                call()
        else:
            call()
    new = [n for n in called if n in NEW or n.startswith("sr_stats")]
    assert new == [] and "sr_jfa_score_integrated" in called and "sr_jfa_score_linear" in called          # (the spy sees what it should)
    # and the package keeps the names where the text checks of the other tests allow them
    pkg = os.path.join(ROOT, "speaker-recognition_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py") and f not in ("jfa.py", "_lib.py", "core.py"):
                assert "sr_stats" not in open(os.path.join(dirpath, f)).read(), f


def test_refused_in_a_process_forked_after_runtime_use(built_lib):
    """As the other JFA calls: in a child forked after its parent touched the GPU runtime, a call that needs the device says so and
    names the remedy; the argument refusals and the plan still work there."""
    import test_fork
    from speaker_recognition_amd import _lib
    L = built_lib
    L.sr_device_count()                                # (this call is what initialises the runtime in the parent)
    n, K, D = 3, 2, 2
    N, F = np.ones((n, K)), np.zeros((n, K * D))

    def child():
        out = {"lost": L.sr_gpu_runtime_lost()}
        out["open"] = L.sr_stats_from_host(n, K, D, _dp(N), _dp(F))
        out["open_error"] = _lib.last_error()
        out["refusal"] = L.sr_stats_from_host(0, K, D, _dp(N), _dp(F))
        out["refusal_error"] = _lib.last_error()
        out["closed"] = L.sr_stats_get(C.c_void_p(0x1000), _dp(N), _dp(F))
        out["closed_error"] = _lib.last_error()
        out["plan"] = _lib.jfa_centre_plan(n, 2, K, D, 1, 1)["n_chunks"]
        return out

    out = test_fork._in_forked_child(child)
    assert out["lost"] == 1 and out["open"] is None and out["refusal"] is None and out["closed"] == -1 and out["plan"] == 1
    assert "forked after its parent" in out["open_error"] and "sr_stats_from_host" in out["open_error"]
    assert "G, K, D >= 1" in out["refusal_error"] and "handle is closed" in out["closed_error"]
    assert L.sr_gpu_runtime_lost() == 0                # the parent is untouched


@pytest.mark.parametrize("shape", rc.CENTRING)
def test_the_centring_gate_fits_its_reference(shape):
    """The float64 numpy restatement against the same formula in extended precision stays at or below 0.1 of the gate, for every
    combination of terms and both groupings; dropping the x u term or evaluating in float32 is far outside it (measured on an
    x86-64 host: 0.04 .. 0.06; 1e12 .. 1e13; 1e6 .. 1e7), so the gate separates a correct float64 result from a wrong one."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 here")
    c = rc.case(*shape)
    worst = 0.0
    for groups in ("speakers", "sessions"):
        for zd, yv, xu in rc.TERMS:
            kw = rc.terms(c, zd, yv, xu)
            _, got, _, _ = rc.centre(c, groups, np.float64, **kw)
            Ng, want, S, n_g = rc.centre(c, groups, np.longdouble, **kw)
            r = rc.worst_ratio(got, want, rc.gate(c, n_g, S, yv, xu))
            worst = max(worst, r)
            assert r <= 0.1, (groups, zd, yv, xu, r)
    kw = rc.terms(c, True, True, True)
    Ng, want, S, n_g = rc.centre(c, "speakers", np.longdouble, **kw)
    bound = rc.gate(c, n_g, S, True, True)
    dropped = rc.worst_ratio(rc.centre(c, "speakers", np.float64, **rc.terms(c, True, True, False))[1], want, bound)
    single = rc.worst_ratio(rc.centre(c, "speakers", np.float32, **kw)[1], want, bound)
    print("centring gate %s: float64 / gate %.3g; without x u %.3g; float32 %.3g" % (shape, worst, dropped, single))
    assert dropped > 1e3 and single > 1e3
