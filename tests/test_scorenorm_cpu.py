"""CPU side of score normalisation (csrc/score_norm.hip, csrc/norm_plan.cpp, speaker_recognition_amd/scorenorm.py): the numpy
restatement (tests/scorenorm_cases.py) on hand cases, against its second statement in the device's product form and against the named
mutants on the GPU tests' own inputs; EER and minDCF on cases worked by hand; the symbols, the plan (sr_score_norm_plan -- also under
the host sanitizers, tests/host/norm_checks.cpp), every refusal without a device, the forked-process refusal and the kernels'
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
import scorenorm_cases as nc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")
NEW = ["sr_score_norm", "sr_score_norm_select", "sr_score_norm_plan"]


def test_restatement_on_hand_cases():
    """Ez row (0, 2): mu 1, sigma 1 -> z of (1, 2) is (0, 1).  Tt column (1, 3): mu 2, sigma 1 -> t of 2 is 0; column (0, 4): mu 2,
    sigma 2 -> t of 1 is -1/2.  s is their mean.  as1 with N = 2 over Ez row (5, 0, 2, 2): the top two are 5 and the FIRST 2."""
    S = np.array([[1.0, 2.0]])
    Ez, Tt = np.array([[0.0, 2.0]]), np.array([[0.0, 1.0], [4.0, 3.0]])
    assert np.array_equal(nc.restate("z", S, Ez=Ez)["out"], [[0.0, 1.0]])
    assert np.array_equal(nc.restate("t", S, Tt=Tt)["out"], [[-0.5, 0.0]])
    assert np.array_equal(nc.restate("s", S, Ez, Tt)["out"], [[-0.25, 0.5]])
    assert np.array_equal(nc.top_idx([5.0, 0.0, 2.0, 2.0], 2), [0, 2]) and np.array_equal(nc.top_idx([5.0, 0.0, 2.0, 2.0], 2, ties="high"), [0, 3])
    assert np.array_equal(nc.top_idx([-0.0, 0.0, -1.0], 1), [0]) and np.array_equal(nc.top_idx([0.0, -0.0, -1.0], 1), [0])      # -0.0 is +0.0
    assert np.array_equal(nc.top_idx([3.0, 1.0], 7), [0, 1])
    r = nc.restate("as1", np.array([[3.5]]), np.array([[5.0, 0.0, 2.0, 2.0]]), np.array([[1.0], [9.0], [3.0], [0.0]]), top_n=2)
    assert r["out"][0, 0] == 0.5 * ((3.5 - 3.5) / 1.5 + (3.5 - 6.0) / 3.0)
    # as2: I_t = the top two of Tt's column = {1, 2}, I_j = the top two of Ez's row = {0, 2}
    r = nc.restate("as2", np.array([[3.5]]), np.array([[5.0, 0.0, 2.0, 2.0]]), np.array([[1.0], [9.0], [3.0], [0.0]]), top_n=2)
    assert r["out"][0, 0] == 0.5 * ((3.5 - 1.0) / 1.0 + (3.5 - 2.0) / 1.0)
    # a constant row is degenerate: zeros, counted; zt's order matters
    r = nc.restate("z", np.array([[1.0, 2.0], [3.0, 4.0]]), Ez=np.array([[0.1, 0.1, 0.1], [0.0, 1.0, 2.0]]))
    assert np.array_equal(r["out"][0], [0.0, 0.0]) and r["degenerate_enrol"] == 1 and r["degenerate_test"] == 0 and r["out"][1, 0] != 0.0
    Zt = np.array([[0.0, 2.0], [1.0, 5.0]])
    zt = nc.restate("zt", S, Ez, Tt, Zt)["out"]
    Tn = np.array([[(0.0 - 1.0) / 1.0, 0.0], [(4.0 - 3.0) / 2.0, 0.0]])
    assert zt[0, 0] == (0.0 - Tn[:, 0].mean()) / Tn[:, 0].std()
    assert not np.allclose(zt, nc.restate("zt", S, Ez, Tt, Zt, zt_order="tz")["out"])


@pytest.mark.parametrize("case", nc.PARITY_CASES)
def test_inputs_meet_the_gates_conditions_and_the_two_restatements_agree(case):
    """On every input set of the GPU parity test: no degenerate pair, rho and q under their stated ceilings; and as2 written with
    np.partition and the four shifted products equals the gather-per-trial restatement within the gate."""
    J, T, Cn, off = case
    c = nc.inputs(*case)
    for mode in nc.MODES:
        r = nc.reference(J, T, Cn, off, mode)
        assert r["degenerate_enrol"] == 0 and r["degenerate_test"] == 0
        assert r["rho"] <= nc.RHO_MAX and r["q"] <= nc.Q_MAX, (mode, r["rho"], r["q"])
        assert np.isfinite(r["out"]).all() and (r["out"] != 0.0).all()
    r = nc.reference(J, T, Cn, off, "as2")
    g = nc.gate(Cn, r["rho"], r["q"])
    ratio = float(np.abs(nc.as2_gemm(c["S"], c["Ez"], c["Tt"], c["top_n"]) - r["out"]).max()) / g
    print("scorenorm two restatements %s: difference / gate = %.3g (gate %.3g)" % (case, ratio, g))
    assert ratio <= 1


@pytest.mark.parametrize("case", nc.PARITY_CASES)
def test_the_inputs_distinguish_every_mutant(case):
    """Each named mutant lies at least 20 gates from the restatement on the GPU parity test's own inputs, in every mode it can show
    in.  The shift mutant (as2's products on unshifted operands) is held to "outside the gate" only, at the offset of 300 sigma and
    the cohort of 37: the gate grows with C, the cancellation it loses does not (at C = 257 it reaches 0.4 .. 4 gates: printed)."""
    J, T, Cn, off = case
    c = nc.inputs(*case)
    for name, (modes, kw) in nc.MUTANTS.items():
        for mode in modes:
            r = nc.reference(J, T, Cn, off, mode)
            g = nc.gate(Cn, r["rho"], r["q"])
            m = nc.restate(mode, c["S"], c["Ez"], c["Tt"], c["Zt"], c["top_n"], **kw)
            assert float(np.abs(m["out"] - r["out"]).max()) >= 20 * g, (name, mode)
    if off > 0:
        r = nc.reference(J, T, Cn, off, "as2")
        ratio = float(np.abs(nc.as2_gemm(c["S"], c["Ez"], c["Tt"], c["top_n"], shift=False) - r["out"]).max()) / nc.gate(Cn, r["rho"], r["q"])
        print("scorenorm shift mutant %s: difference / gate = %.3g" % (case, ratio))
        if Cn == 37:
            assert ratio > 1


def test_eer_and_min_dcf_on_hand_cases():
    from speaker_recognition_amd import scorenorm as sn
    tar, imp = [0.9, 0.8, 0.6, 0.3], [0.7, 0.4, 0.2, 0.1]
    lab = [1] * 4 + [0] * 4
    assert sn.eer(tar + imp, lab) == 0.25                               # the docstring's example: (.25, .25) is an operating point
    assert sn.min_dcf(tar + imp, lab) == 0.5                            # (0, .5): 0.01 x 0.5 / 0.01
    assert sn.min_dcf(tar + imp, lab, p_target=0.5) == 0.5              # P_miss + P_fa: (.25, .25) and (0, .5) both give 0.5
    assert sn.min_dcf(tar + imp, lab, p_target=0.5, c_fa=3.0) == 0.5    # (.5 P_miss + 1.5 P_fa) / .5: (0, .5) -> 0.5
    assert sn.eer([3, 4, 1, 2], [1, 1, 0, 0]) == 0.0 and sn.min_dcf([3, 4, 1, 2], [1, 1, 0, 0]) == 0.0          # perfectly separated
    assert sn.eer([1, 2, 3, 4], [1, 1, 0, 0]) == 1.0                    # fully swapped
    assert sn.min_dcf([1, 2, 3, 4], [1, 1, 0, 0]) == 1.0                # rejecting everything is the best there is
    # ties move together: targets (1, .5), impostors (.5, 0): (0, 1) (0, .5) (.5, 0) (1, 0); the line (0, .5) - (.5, 0) crosses at .25
    assert sn.eer([1.0, 0.5, 0.5, 0.0], [1, 1, 0, 0]) == 0.25
    assert sn.min_dcf([1.0, 0.5, 0.5, 0.0], [1, 1, 0, 0], p_target=0.5) == 0.5
    assert sn.eer([2.0, 2.0, 2.0, 2.0], [1, 0, 1, 0]) == 0.5            # one score: (0, 1) and (1, 0)
    order = np.random.default_rng(0).permutation(8)                     # the order of the trials does not matter
    assert sn.eer(np.array(tar + imp)[order], np.array(lab)[order]) == 0.25
    for bad in (([1.0, 2.0], [1, 1]), ([1.0, 2.0], [0, 0]), ([1.0, np.nan], [1, 0]), ([1.0], [1, 0])):
        with pytest.raises(ValueError):
            sn.eer(*bad)
    with pytest.raises(ValueError):
        sn.min_dcf(tar + imp, lab, p_target=1.0)


def test_llr_matrix():
    from speaker_recognition_amd import scorenorm as sn
    sums = np.array([[10.0, 20.0, 4.0], [3.0, 5.0, 9.0], [1.0, 2.0, 3.0]])
    got = sn.llr_matrix(sums, [2, 4, 0])
    assert np.array_equal(got, [[3.0, -1.5, 0.0], [8.0, -1.0, 0.0]])    # background: the last column; no frames: zeros
    assert np.array_equal(sn.llr_matrix(sums, [2, 4, 0], background=0), [[5.0, 0.5, 0.0], [-3.0, 1.5, 0.0]])
    with pytest.raises(ValueError):
        sn.llr_matrix(sums, [2, 4])


def test_symbols_exported_and_declared(built_lib):
    import speaker_recognition_amd as pkg
    from speaker_recognition_amd import _lib, jfa
    header = open(os.path.join(ROOT, "include", "pygmm_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), "lib/pygmm.so does not export %s" % name
        assert re.search(r"\bint %s\(" % name, header), "%s is not declared in include/pygmm_hip.h" % name
        assert name in _lib.EXT_SYMBOLS
    assert "SR_T_COUNT 20" in header and "norm_scratch_mib" in header and "16384 members" in header          # no timer kind is added
    for name in ("normalise", "znorm", "tnorm", "ztnorm", "snorm", "asnorm", "select_cohort", "llr_matrix", "eer", "min_dcf"):
        assert callable(getattr(pkg, name))
    assert callable(jfa.score_normalised)
    for key, bad in (("norm_scratch_mib", 0), ("norm_scratch_mib", (1 << 20) + 1)):
        with pytest.raises(_lib.SRError, match="norm_scratch_mib must be within"):
            _lib.set_option(key, bad)
    _lib.set_option("norm_scratch_mib", 1024)


def test_plan_chunks_and_bytes(built_lib):
    from speaker_recognition_amd import _lib
    for J, T, Cn in ((1, 1, 2), (17, 63, 37), (200, 2000, 2000), (1000, 1000, 1000)):
        fixed, seg = 3 * J * Cn * 8, (3 * Cn + 4 * J) * 8
        for bound in (fixed + seg, fixed + 3 * seg + 5, 1 << 30):
            p = _lib.score_norm_plan("as2", J, T, Cn, Cn, 40, bound)
            chunk = min(T, (bound - fixed) // seg)
            assert (p["chunk"], p["n_chunks"], p["fixed_bytes"], p["seg_bytes"]) == (chunk, -(-T // chunk), fixed, seg)
            assert p["bytes_scratch"] == fixed + chunk * seg <= bound and p["n_sel"] == p["n_sel_test"] == min(40, Cn)
            assert (p["gemm_enrol_x"], p["gemm_enrol_y"], p["apply_x"], p["apply_y"]) == (-(-chunk // 64), -(-J // 64), J, -(-chunk // 256))
            assert p["select_lds_enrol"] == Cn * 8 + 1024 + 96 <= 160 * 1024 and p["select_test_grid"] == chunk
            for n_cu in (1, 64):                   # the device's size moves nothing but the rounds
                o = _lib.score_norm_plan("as2", J, T, Cn, Cn, 40, bound, n_cu=n_cu)
                assert o["select_rounds"] == -(-max(J, chunk) // n_cu)
                assert {k: v for k, v in o.items() if k != "select_rounds"} == {k: v for k, v in p.items() if k != "select_rounds"}
        for mode in ("z", "t", "zt", "s", "as1"):
            p = _lib.score_norm_plan(mode, J, T, Cn, Cn, 40, 1)
            assert p["mode"] == mode and p["chunk"] == T and p["n_chunks"] == 1 and p["bytes_scratch"] == 0
            assert p["n_sel"] == (0 if mode == "t" else min(40, Cn) if mode == "as1" else Cn)
            assert p["bytes_tnorm"] == (Cn * T * 8 if mode == "zt" else 0) and p["bytes_out"] == J * T * 8
    assert _lib.score_norm_plan("as2", 1, 1, 16384, 16384, 2)["max_C"] == 16384
    # the bit-identity test's bound: 1 MiB (the option's smallest) holds 3 x 64 x 257 x 8 fixed bytes and 79 segments of 8216 B
    assert _lib.score_norm_plan("as2", 64, 200, 257, 257, 40, scratch_bytes=1 << 20)["n_chunks"] == 3


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _case():
    J, T, Cn = 2, 3, 4
    rng = np.random.default_rng(1)
    return dict(mode=5, J=J, T=T, Cz=Cn, Ct=Cn, top_n=2, S=rng.standard_normal((J, T)), Ez=rng.standard_normal((J, Cn)),
                Tt=rng.standard_normal((Cn, T)), Zt=rng.standard_normal((Cn, Cn)))


def _call(L, **over):
    a = dict(_case(), **over)
    out = np.zeros((max(a["J"], 1), max(a["T"], 1)))
    return L.sr_score_norm(a["mode"], a["J"], a["T"], a["Cz"], a["Ct"], a["top_n"], _dp(a["S"]), _dp(a["Ez"]), _dp(a["Tt"]), _dp(a["Zt"]),
                           _dp(out), None)


def _bad(arr, idx, value):
    out = np.array(arr)
    out.flat[idx] = value
    return out


REFUSALS = [(dict(mode=6), "the mode is 0"), (dict(mode=-1), "the mode is 0"), (dict(J=0), "J, T >= 1"), (dict(T=0), "J, T >= 1"),
            (dict(Cz=0), "Cz is 0; a cohort needs at least one member"), (dict(Ct=0, mode=4), "Ct is 0"),
            (dict(top_n=1), r"top_n is 1; an adaptive mode takes the moments of the top_n >= 2"), (dict(top_n=0, mode=4), "top_n >= 2"),
            (dict(Cz=16385, Ct=16385), "up to 16384 members .* Cz is 16385; thin the cohort"), (dict(Ct=16385, mode=1), "Ct is 16385"),
            (dict(Cz=3), "as2 needs one cohort .* Cz = 3 and Ct = 4; score the same cohort on both sides or use as1"),
            (dict(S=None), r"null argument \(S"), (dict(Ez=None), r"mode as2 needs Ez \[J\]\[Cz\]"), (dict(Tt=None), r"mode as2 needs Tt \[Ct\]\[T\]"),
            (dict(Ez=None, mode=0), "mode z needs Ez"), (dict(Tt=None, mode=1), "mode t needs Tt"), (dict(Zt=None, mode=2), r"mode zt needs Zt \[Ct\]\[Cz\]"),
            (dict(Tt=None, mode=3), "mode s needs Tt"), (dict(Ez=None, mode=4), "mode as1 needs Ez")]
REFUSALS += [(dict([(k, _bad(_case()[k], 1, bad))], mode=2), "%s holds a non-finite value at element 1; drop that trial or cohort member" % k)
             for k, bad in (("S", np.nan), ("Ez", np.inf), ("Tt", -np.inf), ("Zt", np.nan))]


def test_refusals_need_no_device(built_lib):
    """Every refusal fails on its arguments alone, with a text that names the argument and the remedy -- never the device."""
    from speaker_recognition_amd import _lib, scorenorm as sn
    L = built_lib
    for over, pat in REFUSALS:
        assert _call(L, **over) == -1, over
        assert re.search(pat, _lib.last_error()) and "HIP" not in _lib.last_error(), (over, _lib.last_error())
    # a matrix the mode does not read may hold anything, and its size is ignored: these get as far as the device
    X = _case()["Ez"]
    idx, mu, sg = np.zeros((2, 2), dtype=np.int64), np.zeros(2), np.zeros(2)
    sel = lambda rows, Cn, n, a: L.sr_score_norm_select(rows, Cn, n, _dp(a), idx.ctypes.data_as(C.POINTER(C.c_int64)), _dp(mu), _dp(sg))      # noqa: E731
    for args, pat in (((0, 4, 2, X), "rows is 0"), ((2, 0, 2, X), "C is 0"), ((2, 16385, 2, X), "up to 16384 members"), ((2, 4, 1, X), "top_n >= 2"),
                      ((2, 4, 2, None), r"null argument \(X"), ((2, 4, 2, _bad(X, 6, np.nan)), "X holds a non-finite value at element 6")):
        assert sel(*args) == -1 and re.search(pat, _lib.last_error()) and "HIP" not in _lib.last_error(), (args[:3], _lib.last_error())
    # the bound: 3 x 2 x 4 x 8 fixed bytes and (12 + 8) x 8 a segment; the option's smallest value is 1 MiB, so through the plan
    out = (C.c_int64 * 40)()
    for args, pat in (((5, 2, 3, 4, 4, 2, 192 + 159, 256), "below one chunk of 352 bytes .* raise the option norm_scratch_mib"),
                      ((7, 2, 3, 4, 4, 2, 1 << 30, 256), "the mode is 0"), ((5, 2, 3, 4, 5, 2, 1 << 30, 256), "Cz = Ct"),
                      ((0, 0, 3, 4, 4, 2, 1 << 30, 256), "J, T >= 1")):
        assert L.sr_score_norm_plan(*args, out, 40) == -1 and re.search(pat, _lib.last_error()) and "HIP" not in _lib.last_error(), _lib.last_error()
    assert L.sr_score_norm_plan(5, 2, 3, 4, 4, 2, 352, 256, out, 39) == -1 and "40 fields" in _lib.last_error()
    assert L.sr_score_norm_plan(5, 2, 3, 4, 4, 2, 352, 256, None, 40) == -1 and "null argument" in _lib.last_error()
    assert L.sr_score_norm_plan(5, 2, 3, 4, 4, 2, 352, 256, out, 40) == 40 and out[3] == 1 and out[4] == 3
    # the Python layer: shapes, the mode, top_n
    c = _case()
    with pytest.raises(ValueError, match="mode is one of"):
        sn.normalise(c["S"], "x", c["Ez"], c["Tt"])
    with pytest.raises(ValueError, match=r"expected enrol_cohort as \[2, \?\]"):
        sn.normalise(c["S"], "z", c["Ez"][:1])
    with pytest.raises(ValueError, match=r"expected cohort_test as \[\?, 3\]"):
        sn.normalise(c["S"], "t", cohort_test=c["Tt"][:, :2])
    with pytest.raises(ValueError, match=r"expected cohort_cohort as \[4, 4\]"):
        sn.normalise(c["S"], "zt", c["Ez"], c["Tt"], c["Zt"][:3])
    if _lib.device_count() == 0:                       # a matrix the mode does not read is not looked at, whatever its shape
        for call in (lambda: sn.normalise(c["S"], "t", c["Ez"][:1], c["Tt"]), lambda: sn.normalise(c["S"], "z", c["Ez"], c["Tt"][:, :2]),
                     lambda: sn.normalise(c["S"], "s", c["Ez"], c["Tt"], c["Zt"][:3])):
            with pytest.raises(_lib.SRError, match="no HIP device"):
                call()
    with pytest.raises(ValueError, match="needs top_n"):
        sn.normalise(c["S"], "as2", c["Ez"], c["Tt"])
    with pytest.raises(ValueError, match="variant is 1 or 2"):
        sn.asnorm(c["S"], c["Ez"], c["Tt"], 2, variant=3)
    with pytest.raises(_lib.SRError, match="mode z needs Ez"):
        sn.normalise(c["S"], "z")
    with pytest.raises(_lib.SRError, match="Tt holds a non-finite value"):
        sn.tnorm(c["S"], _bad(c["Tt"], 0, np.nan))
    with pytest.raises(_lib.SRError, match="top_n is 1"):
        sn.asnorm(c["S"], c["Ez"], c["Tt"], 1)
    with pytest.raises(_lib.SRError, match="top_n >= 2"):
        sn.select_cohort(c["Ez"], 1)
    if _lib.device_count() == 0:                       # and a call that needs the device says what is missing: no CPU path
        for mode in range(6):
            assert _call(L, mode=mode) == -1 and "no HIP device" in _lib.last_error()
        assert sel(2, 4, 2, X) == -1 and "no HIP device" in _lib.last_error()
        with pytest.raises(_lib.SRError, match="no HIP device"):
            sn.asnorm(c["S"], c["Ez"], c["Tt"], 2)
        assert L.sr_score_norm_plan(5, 2, 3, 4, 4, 2, 352, 0, out, 40) == -1 and "no HIP device" in _lib.last_error()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_norm_plan_under_asan_ubsan(tmp_path):
    """csrc/norm_plan.cpp -- every refusal's text and the plan swept over modes, shapes, cohorts, top_n, bounds and device sizes --
    by a stand-alone program (tests/host/norm_checks.cpp) built with AddressSanitizer + UBSan: host code only, no GPU, nothing
    loaded into Python."""
    exe = str(tmp_path / "norm_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "host", "norm_checks.cpp"), os.path.join(CSRC, "norm_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "norm checks ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_score_norm_kernels_do_not_spill(built_lib):
    import test_abi_cpu
    res = test_abi_cpu._kernel_resources("score_norm")
    names = " ".join(res)
    for kernel in ("norm_select_moments_kernel", "norm_shift_kernel", "norm_apply_kernel"):
        assert kernel in names
    assert len(res) == 3
    for name, r in res.items():
        assert r["scratch"] == 0, (name, r)


def test_refused_in_a_process_forked_after_runtime_use(built_lib):
    """In a child forked after its parent touched the GPU runtime both calls say so and name the remedy; the argument refusals and
    the plan still work there."""
    import test_fork
    from speaker_recognition_amd import _lib
    L = built_lib
    L.sr_device_count()                                # (this call is what initialises the runtime in the parent)

    def child():
        out = {"lost": L.sr_gpu_runtime_lost()}
        out["norm"] = _call(L)
        out["norm_error"] = _lib.last_error()
        X = _case()["Ez"]
        out["select"] = L.sr_score_norm_select(2, 4, 2, _dp(X), None, None, None)
        out["select_error"] = _lib.last_error()
        out["refusal"] = _call(L, J=0)
        out["refusal_error"] = _lib.last_error()
        out["plan"] = _lib.score_norm_plan("as2", 2, 3, 4, 4, 2)["n_chunks"]
        return out

    out = test_fork._in_forked_child(child)
    assert out["lost"] == 1 and out["norm"] == -1 and out["select"] == -1 and out["refusal"] == -1 and out["plan"] == 1
    assert "forked after its parent" in out["norm_error"] and "sr_score_norm" in out["norm_error"]
    assert "forked after its parent" in out["select_error"] and "sr_score_norm_select" in out["select_error"]
    assert "J, T >= 1" in out["refusal_error"]
    assert L.sr_gpu_runtime_lost() == 0                # the parent is untouched
