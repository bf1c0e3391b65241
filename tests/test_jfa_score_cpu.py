"""CPU side of JFA trial scoring (csrc/jfa_score.hip, csrc/jfa_plan.cpp, jfa.score_trials / kscore_famous_19 / score_integrated): the
transliteration of kscore_famous_19.m (tests/jfa_score_cases.py) against a hand case and against the device's restated chain in
numpy, the reference-orientation wrapper with the device call replaced, the symbols, the plan (sr_jfa_score_plan -- also under the
host sanitizers, tests/host/jfa_score_checks.cpp), every refusal without a device, the forked-process refusal, and the kernels'
resource records."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfa_score_cases as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")
NEW = ["sr_jfa_score_integrated", "sr_jfa_score_linear", "sr_jfa_score_plan"]


def test_hand_case_without_channel_factors():
    """K = 2, D = 1, one segment N = (2, 4), F = (3, 10), m = (1, 2), E = (1, 4), u = 0, J = 1 with M_1 = m + z d = (2, 4):
    L = 1 and a - h = 0, so quad2 = 0 and s = (lin - quad / 2) / n with n = 6.  UBM: lin = 3 + 5 = 8, quad = 2 + 4 = 6, s_0 = 5 / 6.
    Model: lin = 6 + 10 = 16, quad = 8 + 16 = 24, s_1 = 4 / 6.  Score = -1 / 6.  With u = (1, 2): P = (1, 1), L = 1 + 2 + 4 = 7,
    a = 3 + 5 = 8; UBM: h = 2 + 4 = 6, quad2 = 4 / 7; model: h = 4 + 8 = 12, quad2 = 16 / 7; the score gains (12 / 7) / 2 / 6 = 1 / 7."""
    F, N, m, E = np.array([[3.0, 10.0]]), np.array([[2.0, 4.0]]), np.array([1.0, 2.0]), np.array([1.0, 4.0])
    d, z, v, y = np.array([1.0, 2.0]), np.array([[1.0, 1.0]]), np.zeros((1, 2)), np.zeros((1, 1))
    for u, want in ((np.zeros((1, 2)), -1.0 / 6), (np.array([[1.0, 2.0]]), -1.0 / 6 + 1.0 / 7)):
        ref = sc.kscore_m(F.T, N.T, m, E, d, v.T, u.T, z.T, y.T)
        assert ref["scores"].shape == (1, 1) and abs(ref["scores"][0, 0] - want) < 1e-15
        assert abs(sc.restated(F, N, m, E, d, v, u, z, y)[0, 0] - want) < 1e-15
    assert np.array_equal(ref["lin"][:, 0], [8.0, 16.0]) and np.array_equal(ref["quad"][:, 0], [6.0, 24.0])
    assert np.allclose(ref["quad2"][:, 0], [4.0 / 7, 16.0 / 7], rtol=1e-15)


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_restated_chain_is_the_reference_computation(shape):
    """G once per call and h as one product over K (what the device does) against the transliterated loop, within the gate."""
    c = sc.inputs(*shape)
    assert c["ref"]["kappa"].max() <= 1e6
    gate = sc.gate_integrated(shape, c["ref"])
    r = np.abs(sc.restated(*sc.args(c)) - c["ref"]["scores"]).max() / gate
    print("restated chain %s: difference / gate = %.3g (kappa %.3g)" % (shape, r, c["ref"]["kappa"].max()))
    assert r <= 1


def test_mask_and_zero_quirk_of_the_transliteration():
    c = sc.inputs(*sc.SHAPES[1])
    F, N, m, E, d, v, u, z, y = sc.args(c)
    mask = np.array([[1, 0, 1], [0, 1, 1]])
    got = sc.kscore_m(F.T, N.T, m, E, d, v.T, u.T, z.T, y.T, mask)["scores"]
    assert np.array_equal(got == 0.0, mask == 0) and np.array_equal(got[mask == 1], c["ref"]["scores"][mask == 1])


def test_reference_orientation_wrapper(monkeypatch):
    """kscore_famous_19 takes the .m file's columns and hands score_trials rows; score_integrated hands it the enrolment factors of
    score_dot_product's chain.  The device call is replaced by the restatement."""
    from speaker_recognition_amd import jfa
    seen = []

    def fake(F, N, m, E, d, v, u, z, y, x=None, mode="integrated", mask=None, return_counts=False):
        seen.append(dict(F=F, N=N, d=d, z=z, mask=mask, mode=mode))
        dd = np.zeros(F.shape[1]) if d is None else np.asarray(d)
        zz = np.zeros((np.atleast_2d(y).shape[0], F.shape[1])) if z is None else np.asarray(z)
        out = sc.restated(np.asarray(F), np.asarray(N), np.asarray(m), np.asarray(E), dd, np.asarray(v), np.asarray(u), zz, np.asarray(y))
        return out if mask is None else np.where(mask, out, 0.0)

    monkeypatch.setattr(jfa, "score_trials", fake)
    shape = sc.SHAPES[1]
    T, J, K, D, Ry, Ru = shape
    c = sc.inputs(*shape)
    F, N, m, E, d, v, u, z, y = sc.args(c)
    want = sc.restated(F, N, m, E, d, v, u, z, y)
    got = jfa.kscore_famous_19(F.T, N.T, None, m[:, None], E[:, None], d[:, None], v.T, u.T, z.T, y.T, 0, np.ones((J, T)))
    assert got.shape == (J, T) and np.array_equal(got, want)
    assert seen[-1]["F"].shape == (T, K * D) and seen[-1]["N"].shape == (T, K) and seen[-1]["z"].shape == (J, K * D) and seen[-1]["mode"] == "integrated"
    mask = np.array([[1, 0, 1], [0, 1, 2]])                              # a score where the mask is 1, as the .m file's `== 1`
    got = jfa.kscore_famous_19(F.T, N.T, [], m, E, d, v.T, u.T, z.T, y.T, 0, mask)
    assert np.array_equal(got, np.where(mask == 1, want, 0.0))
    got = jfa.kscore_famous_19(F.T, N.T, None, m, E, 0, v.T, u.T, 0, y.T)                 # scalar 0 for d and z, no mask
    assert seen[-1]["d"] is None and seen[-1]["z"] is None and seen[-1]["mask"] is None
    assert np.array_equal(got, sc.restated(F, N, m, E, np.zeros(K * D), v, u, np.zeros((J, K * D)), y))
    # score_integrated: the enrolment chain on the host restatement of the estimators
    import jfa_cases as jc

    class HostEstimator:
        def __init__(self, N, Fc, E):
            self.a = (np.array(N), np.array(Fc), np.array(E))

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            pass

        def factors(self, W, accumulate=False):
            return jc.factors(*self.a, np.asarray(W, dtype=np.float64))[0]

    monkeypatch.setattr(jfa, "FactorEstimator", HostEstimator)
    trn, tst = (F[:2], N[:2]), (F[1:], N[1:])
    ubm = (np.full(K, 1.0 / K), m.reshape(K, D), E.reshape(K, D))
    got = jfa.score_integrated({"F": trn[0], "N": trn[1]}, tst, ubm, v, u, d)
    want, ref = sc.score_integrated(trn, tst, m, E, v, u, d)
    assert got.shape == (2, 2) and np.abs(got - want).max() <= sc.gate_integrated((2, 2, K, D, Ry, Ru), ref)
    assert jc.rel(seen[-1]["z"], jc.estimate_z_and_d(trn[0], trn[1], None, m, E, d, np.vstack([v, u]), 0, 0,
                                                      jc.estimate_y_and_v(trn[0], trn[1], None, m, E, d, np.vstack([v, u]), 0, 0, 0, 0, np.arange(2)),
                                                      0, np.arange(2))) < 1e-12


def test_symbols_exported_and_declared(built_lib):
    from speaker_recognition_amd import _lib
    header = open(os.path.join(ROOT, "include", "pygmm_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), "lib/pygmm.so does not export %s" % name
        assert re.search(r"\bint %s\(" % name, header), "%s is not declared in include/pygmm_hip.h" % name
        assert name in _lib.EXT_SYMBOLS
    assert "SR_T_COUNT 20" in header and "kscore_famous_19.m" in header          # no timer kind is added


def test_plan_chunks_paths_and_bytes(built_lib):
    from speaker_recognition_amd import _lib
    for T in (1, 5, 33, 2000):
        for J in (1, 17, 260):
            for K, D in ((1, 1), (17, 39), (512, 39)):
                for Ru in (1, 17, 65, 112, 113, 130):
                    Ry, J1, kd = 7, J + 1, K * D
                    seg = (Ru * Ru + J1 * Ru) * 8
                    for bound in (seg, 3 * seg + 5, 1 << 20, 1 << 30):
                        if bound < seg:
                            continue
                        p = _lib.jfa_score_plan(T, J, K, D, Ry, Ru, "integrated", bound)
                        chunk, n = p["chunk"], p["n_chunks"]
                        assert chunk == min(T, bound // seg) and p["seg_bytes"] == seg and p["bytes_scratch"] == chunk * seg <= bound
                        assert n == -(-T // chunk) and (n - 1) * chunk < T <= n * chunk                             # every segment once
                        assert (p["bytes_M"], p["bytes_ME"], p["bytes_P"], p["bytes_q"]) == (J1 * kd * 8, J1 * kd * 8, K * Ru * Ru * 8, J1 * K * 8)
                        assert (p["bytes_G"], p["bytes_N"], p["bytes_F"]) == (K * Ru * J1 * 8, T * K * 8, T * kd * 8)
                        assert (p["bytes_lin"], p["bytes_quad"], p["bytes_a"], p["bytes_out"], p["bytes_comp"]) == (T * J1 * 8, T * J1 * 8, T * Ru * 8, J * T * 8, 0)
                        assert p["path"] == ("lds" if Ru <= 112 else "global") and p["kscore_lds"] <= 160 * 1024
                        assert p["gemm_L_x"] == -(-Ru * Ru // 64) and p["gemm_L_y"] == -(-chunk // 64) == p["gemm_h_y"]
                        assert p["gemm_h_x"] == -(-Ru * J1 // 64) and p["gemm_lin_x"] == -(-J1 // 64) == p["gemm_quad_x"] and p["gemm_a_x"] == -(-Ru // 64)
                        assert (p["cross_grid_x"], p["cross_grid_y"], p["cross_grid_z"]) == (K, -(-J1 // 16), -(-Ru // 16))
                        assert p["gram_grid_x"] == K and p["gram_grid_y"] == (-(-Ru // 16)) ** 2 and p["kscore_grid"] == chunk
                        assert p["gemm_yv_x"] == -(-kd // 64) and p["gemm_yv_y"] == -(-J // 64)
                        for n_cu in (1, 64):                           # the device's size moves nothing but the rounds
                            o = _lib.jfa_score_plan(T, J, K, D, Ry, Ru, "integrated", bound, n_cu=n_cu)
                            assert o["kscore_rounds"] == -(-chunk // n_cu)
                            assert {k: v for k, v in o.items() if k != "kscore_rounds"} == {k: v for k, v in p.items() if k != "kscore_rounds"}
                    lin = _lib.jfa_score_plan(T, J, K, D, Ry, Ru, "linear", 1)
                    assert lin["mode"] == "linear" and lin["chunk"] == T and lin["n_chunks"] == 1 and lin["bytes_scratch"] == 0
                    assert lin["bytes_comp"] == T * kd * 8 and lin["bytes_M"] == J * kd * 8
                    assert (lin["gemm_xu_x"], lin["gemm_xu_y"], lin["gemm_out_x"], lin["gemm_out_y"]) == (-(-kd // 64), -(-T // 64), -(-T // 64), -(-J // 64))
    for lds_rows, Ru, want in ((0, 112, "lds"), (0, 113, "global"), (17, 17, "lds"), (17, 18, "global"), (1, 17, "global"), (1, 1, "lds")):
        assert _lib.jfa_score_plan(33, 17, 17, 39, 17, Ru, lds_rows=lds_rows)["path"] == want
    # the bit-identity test's bound: (17^2 + 18 x 17) x 8 = 4760 B a segment, 1 MiB holds 220: the issue's >= 3 chunks need less
    assert _lib.jfa_score_plan(33, 17, 17, 39, 17, 17, scratch_bytes=12 * 4760)["n_chunks"] == 3


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _case():
    T, J, K, D, Ry, Ru = 3, 2, 2, 2, 2, 3
    kd = K * D
    return dict(T=T, J=J, K=K, D=D, Ry=Ry, Ru=Ru, N=np.ones((T, K)), F=np.full((T, kd), 0.5), m=np.full(kd, 0.1), E=np.full(kd, 2.0),
                d=np.full(kd, 0.2), v=np.full((Ry, kd), 0.3), u=np.full((Ru, kd), 0.4), z=np.full((J, kd), 0.1), y=np.ones((J, Ry)),
                x=np.full((T, Ru), 0.5), mask=np.ones((J, T), dtype=np.uint8), mask_shape=None)


def _call(L, mode, **over):
    a = dict(_case(), **over)
    out = np.zeros((a["J"], a["T"]))
    head = (a["T"], a["J"], a["K"], a["D"], a["Ry"], a["Ru"]) + tuple(_dp(a[k]) for k in ("N", "F", "m", "E", "d", "v", "u", "z", "y"))
    mask = a["mask"]
    mr, mc = a["mask_shape"] or ((a["J"], a["T"]) if mask is not None else (0, 0))
    mk = (mask.ctypes.data_as(C.POINTER(C.c_uint8)) if mask is not None else None, mr, mc)
    if mode == "integrated":
        return L.sr_jfa_score_integrated(*head, *mk, _dp(out), None, None)
    return L.sr_jfa_score_linear(*head, _dp(a["x"]), *mk, _dp(out), None)


def _bad(arr, idx, value):
    out = np.array(arr)
    out.flat[idx] = value
    return out


REFUSALS = [(dict(T=0), "T, J, K, D, Ry, Ru >= 1"), (dict(J=0), "T, J, K, D, Ry, Ru >= 1"), (dict(K=0), "T, J, K, D, Ry, Ru >= 1"),
            (dict(D=0), "T, J, K, D, Ry, Ru >= 1"), (dict(Ry=0), "T, J, K, D, Ry, Ru >= 1"), (dict(Ru=0), "T, J, K, D, Ry, Ru >= 1"),
            (dict(Ry=513), "up to 512 factors, v or u has 513 rows; score with fewer factors"), (dict(Ru=513), "up to 512 factors"),
            (dict(N=None), "null argument"), (dict(y=None), "null argument"),
            (dict(mask_shape=(3, 2)), r"the mask is \[3\]\[2\], the score matrix \[2\]\[3\]")]
REFUSALS += [(dict([(k, _bad(_case()[k], 1, bad))]), "%s holds a non-finite value at element 1" % k)
             for k, bad in (("N", np.nan), ("F", np.inf), ("m", np.nan), ("E", np.nan), ("d", -np.inf), ("v", np.nan), ("u", np.inf), ("z", np.nan),
                            ("y", np.nan))]
REFUSALS += [(dict(N=_bad(_case()["N"], 4, -0.5)), "negative occupancy at segment 2, mixture 0"), (dict(E=_bad(_case()["E"], 1, 0.0)), "E must be positive, element 1")]


def test_refusals_need_no_device(built_lib):
    """Every refusal fails on its arguments alone, with a text that names the argument and the remedy -- never the device."""
    from speaker_recognition_amd import _lib, jfa
    L = built_lib
    for mode in ("integrated", "linear"):
        for over, pat in REFUSALS:
            assert _call(L, mode, **over) == -1, (mode, over)
            assert re.search(pat, _lib.last_error()) and "HIP" not in _lib.last_error(), (mode, over, _lib.last_error())
    assert _call(L, "linear", x=None) == -1 and "linear mode needs the test segments' channel factors x" in _lib.last_error()
    assert _call(L, "linear", x=_bad(_case()["x"], 2, np.nan)) == -1 and "x holds a non-finite value at element 2" in _lib.last_error()
    # the bound: one segment's blocks are (3^2 + 3 x 3) x 8 = 144 B; the option's smallest value is 1 MiB, so through the plan
    out = (C.c_int64 * 56)()
    for args, pat in (((3, 2, 2, 2, 2, 3, 0, 143, 0, 256), "raise the option jfa_scratch_mib"), ((3, 2, 2, 2, 2, 3, 2, 1 << 30, 0, 256), "the mode is 0"),
                      ((3, 2, 2, 2, 2, 3, 0, 1 << 30, 113, 256), "jfa_lds_rows"), ((0, 2, 2, 2, 2, 3, 1, 1 << 30, 0, 256), "T, J, K, D, Ry, Ru >= 1")):
        assert L.sr_jfa_score_plan(*args, out, 56) == -1 and re.search(pat, _lib.last_error()) and "HIP" not in _lib.last_error(), _lib.last_error()
    assert L.sr_jfa_score_plan(3, 2, 2, 2, 2, 3, 0, 144, 0, 256, out, 55) == -1 and "56 fields" in _lib.last_error()
    assert L.sr_jfa_score_plan(3, 2, 2, 2, 2, 3, 0, 144, 0, 256, None, 56) == -1 and "null argument" in _lib.last_error()
    assert L.sr_jfa_score_plan(3, 2, 2, 2, 2, 3, 0, 144, 0, 256, out, 56) == 56 and out[1] == 1 and out[2] == 3
    # the Python layer: shapes, the mode, the mask
    c = _case()
    a = (c["F"], c["N"], c["m"], c["E"], c["d"], c["v"], c["u"], c["z"], c["y"])
    with pytest.raises(ValueError, match="a mask of shape"):
        jfa.score_trials(*a, mask=np.ones((3, 2)))
    with pytest.raises(ValueError, match="mode is 'integrated' or 'linear'"):
        jfa.score_trials(*a, mode="dot")
    with pytest.raises(ValueError, match=r"expected v \[Ry, 4\]"):
        jfa.score_trials(*a[:5], c["v"][:, :3], *a[6:])
    with pytest.raises(_lib.SRError, match="linear mode needs"):
        jfa.score_trials(*a, mode="linear")
    with pytest.raises(_lib.SRError, match="F holds a non-finite value"):
        jfa.score_trials(_bad(c["F"], 0, np.nan), *a[1:])
    if _lib.device_count() == 0:                       # and a call that needs the device says what is missing: no CPU path
        for mode in ("integrated", "linear"):
            assert _call(L, mode) == -1 and "no HIP device" in _lib.last_error()
            with pytest.raises(_lib.SRError, match="no HIP device"):
                jfa.score_trials(*a, x=c["x"], mode=mode)
        assert L.sr_jfa_score_plan(3, 2, 2, 2, 2, 3, 0, 144, 0, 0, out, 56) == -1 and "no HIP device" in _lib.last_error()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_jfa_score_plan_under_asan_ubsan(tmp_path):
    """csrc/jfa_plan.cpp's scoring half -- every refusal's text and the plan swept over counts, shapes, ranks, modes, bounds, the
    jfa_lds_rows option and device sizes -- by a stand-alone program (tests/host/jfa_score_checks.cpp) built with AddressSanitizer +
    UBSan: host code only, no GPU, nothing loaded into Python."""
    exe = str(tmp_path / "jfa_score_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "host", "jfa_score_checks.cpp"), os.path.join(CSRC, "jfa_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "jfa score checks ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_jfa_score_kernels_do_not_spill(built_lib):
    import test_abi_cpu
    res = test_abi_cpu._kernel_resources("jfa_score")
    names = " ".join(res)
    for kernel in ("jfa_synth_kernel", "jfa_cross_kernel", "jfa_kscore_kernel", "jfa_compensate_kernel"):
        assert kernel in names
    assert len(res) == 4
    for name, r in res.items():
        assert r["scratch"] == 0, (name, r)


def test_refused_in_a_process_forked_after_runtime_use(built_lib):
    """In a child forked after its parent touched the GPU runtime both scoring calls say so and name the remedy; the argument
    refusals and the plan still work there."""
    import test_fork
    from speaker_recognition_amd import _lib
    L = built_lib
    L.sr_device_count()                                # (this call is what initialises the runtime in the parent)

    def child():
        out = {"lost": L.sr_gpu_runtime_lost()}
        for mode in ("integrated", "linear"):
            out[mode] = _call(L, mode)
            out[mode + "_error"] = _lib.last_error()
        out["refusal"] = _call(L, "integrated", T=0)
        out["refusal_error"] = _lib.last_error()
        out["plan"] = _lib.jfa_score_plan(3, 2, 2, 2, 2, 3)["n_chunks"]
        return out

    out = test_fork._in_forked_child(child)
    assert out["lost"] == 1 and out["integrated"] == -1 and out["linear"] == -1 and out["refusal"] == -1 and out["plan"] == 1
    assert "forked after its parent" in out["integrated_error"] and "sr_jfa_score_integrated" in out["integrated_error"]
    assert "forked after its parent" in out["linear_error"] and "sr_jfa_score_linear" in out["linear_error"]
    assert "T, J, K, D, Ry, Ru >= 1" in out["refusal_error"]
    assert L.sr_gpu_runtime_lost() == 0                # the parent is untouched
