"""CPU side of the i-vector back end (csrc/plda.hip, csrc/plda_plan.cpp, speaker_recognition_amd/plda.py, ivector.py): the numpy
restatement (tests/plda_cases.py) against the joint-Gaussian form, the gates' conditions and the named mutants on the GPU tests' own
inputs; the symbols, the plan (sr_plda_plan -- also under the host sanitizers, tests/host/plda_checks.cpp), every refusal without a
device, the forked-process refusal and the kernels' resource records."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plda_cases as pc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")
NEW = ["sr_backend_fit", "sr_backend_apply", "sr_cosine_score", "sr_plda_train", "sr_plda_score", "sr_plda_plan"]


def test_restated_score_equals_the_joint_form():
    """R = 5, the models' counts 1 .. 3: the score by Phi_c, P_c and P_0 is  ln p(enrolment, x) - ln p(enrolment) - ln p(x)  of the
    Gaussian with covariance I (x) Sw + 1 1^T (x) Sb."""
    rng = np.random.default_rng(5)
    R = 5
    Sb, Sw, mu = 2.0 * pc.spd(R, 10.0, rng), pc.spd(R, 10.0, rng), rng.standard_normal(R)
    counts = np.array([1, 2, 3, 2, 1, 3])
    ids = np.repeat(np.arange(6), counts)
    enrol = mu + rng.standard_normal((ids.size, R)) * 1.5
    X = mu + rng.standard_normal((4, R)) * 1.5
    E = np.zeros((6, R))
    np.add.at(E, ids, enrol)
    got, f = pc.score(mu, Sb, Sw, E, counts, X, want_factors=True)
    want = np.array([[pc.joint_score(mu, Sb, Sw, enrol[ids == j], x) for x in X] for j in range(6)])
    ratio = pc.rel(got, want) / pc.gate_score(R, f)
    print("plda restated score against the joint form: difference %.3g, difference / gate = %.3g" % (pc.rel(got, want), ratio))
    assert ratio <= 1 and pc.rel(got, want) < 1e-12


def test_restated_em_never_decreases_the_joint_likelihood():
    tc = pc.train_case(5, (1, 2, 3, 2, 1, 3, 3, 2), 8)
    ll = [pc.marginal_loglik(tc["X"], tc["ids"], tc["mu"], tc["start"], tc["start"])]
    ll += [pc.marginal_loglik(tc["X"], tc["ids"], tc["mu"], Sb, Sw) for Sb, Sw in tc["trace"]]
    assert len(ll) == 9 and np.all(np.diff(ll) >= 0), ll
    assert ll[-1] - ll[0] > 1.0                        # and it moves


@pytest.mark.parametrize("case", pc.TRAIN_CASES)
def test_training_inputs_meet_the_conditions_and_distinguish_the_mutants(case):
    """On every input set of the GPU training tests: every condition number of the restatement's rounds under the ceiling; and each
    mutant that can show on the case lies outside the five-round gate of BOTH covariances' worst factors -- applied to the second
    round, where Sb and Sw no longer commute (the start is Sb = Sw)."""
    R, counts = case
    tc = pc.train_case(R, counts)
    n, S = sum(counts), len(counts)
    assert tc["kSigma"] <= pc.KAPPA_MAX and all(tc["worst"][k] <= pc.KAPPA_MAX for k in ("kb", "kw", "kP")), tc["worst"]
    gb, gw = pc.gate_em(R, n, S, tc["worst"], 5)
    assert gb < 1e-2 and gw < 1e-2                     # a gate that lets a percent through tests nothing
    for name in pc.MUTANTS:
        if not pc.mutant_shows(name, "train", R, counts):
            continue
        Sb, Sw = pc.em_step(tc["X"], tc["ids"], tc["mu"], *tc["trace"][0], mutant=name)
        rb, rw = pc.rel(Sb, tc["trace"][1][0]) / gb, pc.rel(Sw, tc["trace"][1][1]) / gw
        print("plda mutant %s, training R = %d, S = %d: difference / gate = %.3g (Sb), %.3g (Sw)" % (name, R, S, rb, rw))
        assert max(rb, rw) > 1, (name, rb, rw)


@pytest.mark.parametrize("case", pc.SCORE_CASES)
def test_scoring_inputs_meet_the_conditions_and_distinguish_the_mutants(case):
    R, J, T = case
    c = pc.score_case(R, J, T)
    f = c["factors"]
    assert all(f[k] <= pc.KAPPA_MAX for k in ("kb", "kw", "kP", "kPc", "kP0")), f
    assert np.isfinite(c["want"]).all() and set(c["counts"]) <= set(range(1, 8))
    g = pc.gate_score(R, f)
    assert g < 1e-6
    for name in pc.MUTANTS:
        if not pc.mutant_shows(name, "score", R, c["counts"], T):
            continue
        ratio = pc.rel(pc.score(c["mu"], c["Sb"], c["Sw"], c["E"], c["counts"], c["X"], mutant=name), c["want"]) / g
        print("plda mutant %s, scoring %s: difference / gate = %.3g" % (name, case, ratio))
        assert ratio > 1, (name, ratio)


def test_transform_inputs_meet_the_conditions_and_the_transposed_mutant_shows():
    for R in pc.TRANSFORM_R:
        for n in sorted(set((R + 1,) + pc.TRANSFORM_N)):
            if n <= R:
                continue
            c = pc.transform_case(R, n)
            assert c["kSigma"] <= pc.KAPPA_MAX and c["kW"] is not None and c["kW"] <= pc.KAPPA_MAX, (R, n, c["kSigma"], c["kW"])
            Y = pc.transform(c["X"], c["mu"], c["A"], length_norm=False)
            assert np.abs(Y.T @ Y / n - np.eye(R)).max() <= pc.gate_cov(R, n, c["kSigma"])         # the restatement whitens
            if R > 1:
                bad = pc.transform(c["X"], c["mu"], c["A"], length_norm=False, mutant="transposed")
                assert np.abs(bad.T @ bad / n - np.eye(R)).max() > pc.gate_cov(R, n, c["kSigma"])


def test_symbols_exported_and_declared(built_lib):
    from speaker_recognition_amd import _lib, ivector, plda
    header = open(os.path.join(ROOT, "include", "pygmm_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), "lib/pygmm.so does not export %s" % name
        assert re.search(r"\bint %s\(" % name, header), "%s is not declared in include/pygmm_hip.h" % name
        assert name in _lib.EXT_SYMBOLS
    assert "SR_T_COUNT 20" in header and "plda_scratch_mib" in header                                          # no timer kind is added
    plan_text = re.search(r"\* sr_plda_plan: what a call decides.*?\n \* Refused", header, re.S)
    assert plan_text and "Writes 36 fields (n_out >= 36) and returns 36" in plan_text.group(0)
    assert header.count("Writes 36 fields") == 1                       # (and no other plan's text says so)
    for name in ("fit_transform", "transform", "cosine_score", "PLDA"):
        assert callable(getattr(plda, name))
    assert callable(ivector.train_tv) and callable(ivector.extract) and callable(_lib.plda_plan)
    for bad in (0, (1 << 20) + 1):
        with pytest.raises(_lib.SRError, match="plda_scratch_mib must be within"):
            _lib.set_option("plda_scratch_mib", bad)
    _lib.set_option("plda_scratch_mib", 1024)


def test_plan_classes_permutation_chunks_and_paths(built_lib):
    from speaker_recognition_amd import _lib
    # training: the labels' counts 3 1 2 1 3 -> classes (1: labels 1, 3), (2: label 2), (3: labels 0, 4)
    ids = [0, 1, 4, 2, 0, 3, 4, 2, 0, 4]
    p = _lib.plda_plan("train", 7, ids)
    assert p["classes"] == [(1, 0, 2), (2, 2, 1), (3, 3, 2)] and p["perm"].tolist() == [1, 3, 2, 0, 4]
    assert (p["rows"], p["groups"], p["n_classes"], p["path"], p["lds_rows"]) == (10, 5, 3, 0, 112)
    assert (p["sum_chunk"], p["sum_chunks"], p["grp_chunk"], p["grp_chunks"]) == (10, 1, 5, 1)
    assert p["factor_lds"] == (7 * 17 + 7 + 49) * 8 and p["invert_grid"] == 3 and p["class_sums_x"] == 5
    for R, lds_rows, path in ((112, 0, 0), (113, 0, 1), (17, 1, 1), (65, 64, 1), (64, 64, 0), (1, 1, 0)):
        q = _lib.plda_plan("train", R, ids, lds_rows=lds_rows)
        assert q["path"] == path and q["tri_inverse_y"] == (-(-R // 4) if path else 0)      # the factor's inverse: a wave per column
    big = np.arange(70000) % 69999                     # more vectors than one launch of a sum takes: whole reduction tiles, in order
    p = _lib.plda_plan("train", 3, big)
    assert (p["sum_chunk"], p["sum_chunks"], p["grp_chunk"], p["grp_chunks"]) == (65536, 2, 65536, 2) and p["sum_chunk"] % 16 == 0
    assert p["classes"] == [(1, 0, 69998), (2, 69998, 1)] and p["perm"][-1] == 0
    # scoring: the models sorted by count, stable; the chunks under the bound
    en = [2, 1, 7, 1, 2, 2]
    for R, T in ((5, 9), (65, 1000), (400, 100000)):
        seg = (2 * R + 2) * 8
        for bound in (seg, 3 * seg + 5, 1 << 20, 1 << 30):
            p = _lib.plda_plan("score", R, en, T=T, scratch_bytes=bound)
            chunk = min(T, bound // seg)
            assert (p["chunk"], p["n_chunks"], p["seg_bytes"], p["bytes_scratch"]) == (chunk, -(-T // chunk), seg, chunk * seg)
            assert p["classes"] == [(1, 0, 2), (2, 2, 3), (7, 5, 1)] and p["perm"].tolist() == [1, 3, 0, 4, 5, 2]
            assert (p["gemm_cross_x"], p["gemm_cross_y"], p["assemble_grid"]) == (-(-chunk // 64), 1, -(-3 * chunk // 256))
            for n_cu in (1, 64):                       # the device's size moves nothing but the rounds
                o = _lib.plda_plan("score", R, en, T=T, scratch_bytes=bound, n_cu=n_cu)
                assert o["invert_rounds"] == -(-4 // n_cu)
                assert all(np.array_equal(o[k], p[k]) for k in p if k != "invert_rounds")
    # the bit-identity test's bound: 1 MiB (the option's smallest) holds 992 segments of 65 dimensions
    assert _lib.plda_plan("score", 65, en, T=1000, scratch_bytes=1 << 20)["n_chunks"] == 2
    assert _lib.plda_plan("score", 512, [1], T=1)["max_R"] == 512


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None


def _case():
    rng = np.random.default_rng(2)
    R = 3
    return dict(R=R, n=6, X=rng.standard_normal((6, R)), ids=np.array([0, 1, 1, 0, 2, 1], dtype=np.int64), S=3, n_iter=1, mu=rng.standard_normal(R),
                Sb=np.eye(R) * 2.0, Sw=np.eye(R), start=0, J=2, T=4, E=rng.standard_normal((2, R)), en=np.array([1, 3], dtype=np.int64),
                Xt=rng.standard_normal((4, R)), A=np.eye(R), kind=1)


def _train(L, **over):
    a = dict(_case(), **over)
    Sb, Sw = (None if a[k] is None else np.array(a[k]) for k in ("Sb", "Sw"))
    return L.sr_plda_train(a["n"], a["R"], _dp(a["X"]), _ip(a["ids"]), a["S"], a["n_iter"], a["start"], None, _dp(Sb), _dp(Sw), None, None, None)


def _score(L, **over):
    a = dict(_case(), **over)
    out = np.zeros((max(a["J"], 1), max(a["T"], 1)))
    return L.sr_plda_score(a["J"], a["T"], a["R"], _dp(a["mu"]), _dp(a["Sb"]), _dp(a["Sw"]), _dp(a["E"]), _ip(a["en"]), _dp(a["Xt"]), _dp(out), None)


def _fit(L, **over):
    a = dict(_case(), **over)
    mu, A = np.zeros(max(a["R"], 1)), np.zeros((max(a["R"], 1),) * 2)
    return L.sr_backend_fit(a["kind"], a["n"], a["R"], _dp(a["X"]), _ip(a["ids"]), a["S"], _dp(mu), _dp(A))


def _apply(L, **over):
    a = dict(_case(), **over)
    Y = np.zeros((max(a["n"], 1), max(a["R"], 1)))
    return L.sr_backend_apply(a["n"], a["R"], _dp(a["X"]), _dp(a["mu"]), _dp(a["A"]), 1, _dp(Y), None)


def _cosine(L, **over):
    a = dict(_case(), **over)
    out = np.zeros((max(a["J"], 1), max(a["T"], 1)))
    return L.sr_cosine_score(a["J"], a["T"], a["R"], _dp(a["E"]), _dp(a["Xt"]), _dp(out))


def _bad(arr, idx, value):
    out = np.array(arr)
    out.flat[idx] = value
    return out


_C = _case()
_SKEW = np.array([[2.0, 0.5, 0.0], [0.1, 2.0, 0.0], [0.0, 0.0, 2.0]])
REFUSALS = [
    (_train, dict(R=0), "R >= 1"), (_train, dict(R=513), "up to 512 dimensions, these have 513; extract fewer factors"),
    (_train, dict(n=0), "n, the number of training vectors is 0; pass at least one row"), (_train, dict(X=None), r"null argument \(X"),
    (_train, dict(ids=None), r"null argument \(ids"), (_train, dict(S=2), "row 4 has label 2, outside 0 .. 1; renumber the speakers"),
    (_train, dict(S=4), "label 3 of 0 .. 3 has no row; renumber"), (_train, dict(ids=_C["ids"] - 1, S=3), "row 0 has label -1"),
    (_train, dict(S=0), "1 <= S <= n"), (_train, dict(n_iter=0), "n_iter is 0; run at least one iteration"),
    (_train, dict(X=_bad(_C["X"], 5, np.nan)), "X, the training vectors .* non-finite value at element 5; drop that vector"),
    (_train, dict(Sb=None), r"null argument \(Sb and Sw"), (_train, dict(Sw=None, start=1), r"null argument \(Sb and Sw"),
    (_train, dict(start=2), r"default_start is 0 \(Sb and Sw hold the start\) or 1"), (_train, dict(start=-1), "default_start is 0"), (_train, dict(Sb=_SKEW), r"Sb is not symmetric .*\[1\]\[0\].* pass \(Sb \+ Sb\^T\) / 2"),
    (_train, dict(Sw=_SKEW), "Sw is not symmetric"), (_train, dict(Sw=_bad(_C["Sw"], 4, np.inf)), "Sw holds a non-finite value at element 4"),
    (_score, dict(R=0), "R >= 1"), (_score, dict(R=600), "up to 512 dimensions"), (_score, dict(J=0), "J, the number of models is 0"),
    (_score, dict(T=0), "T, the number of test segments is 0"), (_score, dict(E=None), r"null argument \(E"), (_score, dict(Xt=None), r"null argument \(X"),
    (_score, dict(mu=None), r"null argument \(mu"), (_score, dict(en=None), r"null argument \(enrol_n"),
    (_score, dict(en=np.array([1, 0], dtype=np.int64)), "enrol_n of model 1 is 0; a model is enrolled from at least one vector"),
    (_score, dict(en=np.array([-2, 1], dtype=np.int64)), "enrol_n of model 0 is -2"),
    (_score, dict(E=_bad(_C["E"], 1, np.inf)), "E, the models' enrolment sums .* element 1"), (_score, dict(Xt=_bad(_C["Xt"], 2, np.nan)), "X, the test vectors .* element 2"),
    (_score, dict(mu=_bad(_C["mu"], 0, np.nan)), "mu holds a non-finite value at element 0"), (_score, dict(Sb=_SKEW), "Sb is not symmetric"),
    (_score, dict(Sw=_SKEW.T), "Sw is not symmetric"),
    (_fit, dict(kind=2), r"the kind is 0 \(whiten\) or 1 \(wccn\)"), (_fit, dict(R=0), "R >= 1"), (_fit, dict(n=0), "pass at least one row"),
    (_fit, dict(X=None), r"null argument \(X"), (_fit, dict(ids=None), r"null argument \(ids"), (_fit, dict(S=4), "label 3 of 0 .. 3 has no row"),
    (_fit, dict(X=_bad(_C["X"], 0, -np.inf)), "non-finite value at element 0"),
    (_apply, dict(R=513), "up to 512 dimensions"), (_apply, dict(n=0), "n, the number of vectors is 0"), (_apply, dict(mu=None), r"null argument \(mu"),
    (_apply, dict(A=_bad(_C["A"], 8, np.nan)), "A holds a non-finite value at element 8"), (_apply, dict(X=_bad(_C["X"], 3, np.nan)), "X, the vectors .* element 3"),
    (_cosine, dict(J=0), "J, the number of models is 0"), (_cosine, dict(T=0), "T, the number of test segments is 0"), (_cosine, dict(R=0), "R >= 1"),
    (_cosine, dict(E=None), r"null argument \(E"), (_cosine, dict(Xt=_bad(_C["Xt"], 11, np.nan)), "X, the test vectors .* element 11"),
]


def test_refusals_need_no_device(built_lib):
    """Every refusal fails on its arguments alone, with a text that names the argument and the remedy -- never the device."""
    from speaker_recognition_amd import _lib, plda
    L = built_lib
    for call, over, pat in REFUSALS:
        assert call(L, **over) == -1, (call.__name__, over)
        assert re.search(pat, _lib.last_error()) and "HIP" not in _lib.last_error(), (call.__name__, over, _lib.last_error())
    # the bound: the option's smallest value is 1 MiB, so through the plan
    out = (C.c_int64 * 36)()
    en = np.array([1, 3], dtype=np.int64)
    plan = lambda *a, n_out=36, o=out: L.sr_plda_plan(*a, o, n_out, None, None)                    # noqa: E731
    for args, pat in (((1, 3, 2, 2, 4, _ip(en), 63, 0, 256), "below one chunk of 64 bytes .* raise the option plda_scratch_mib"),
                      ((2, 3, 2, 2, 4, _ip(en), 1 << 30, 0, 256), "the kind is 0"), ((1, 3, 2, 2, 0, _ip(en), 1 << 30, 0, 256), "T, the number of test segments is 0"),
                      ((1, 3, 2, 2, 4, _ip(en), 1 << 30, 113, 256), "jfa_lds_rows must be 0"), ((0, 3, 2, 3, 0, _ip(en), 0, 0, 256), "1 <= S <= n")):
        assert plan(*args) == -1 and re.search(pat, _lib.last_error()) and "HIP" not in _lib.last_error(), _lib.last_error()
    assert plan(1, 3, 2, 2, 4, _ip(en), 64, 0, 256, n_out=35) == -1 and "36 fields" in _lib.last_error()
    assert plan(1, 3, 2, 2, 4, _ip(en), 64, 0, 256, o=None) == -1 and "null argument" in _lib.last_error()
    assert plan(1, 3, 2, 2, 4, _ip(en), 64, 0, 256) == 36 and out[10] == 1 and out[11] == 4
    # the Python layer: shapes, kinds, modes
    c = _case()
    with pytest.raises(ValueError, match="kind is one of"):
        plda.fit_transform(c["X"], kind="lda")
    with pytest.raises(ValueError, match="needs ids"):
        plda.fit_transform(c["X"], kind="wccn")
    with pytest.raises(ValueError, match=r"one label per row as ids \(6\), got 5"):
        plda.fit_transform(c["X"], c["ids"][:5], kind="wccn")
    with pytest.raises(ValueError, match=r"expected mu \[3\] and A \[3, 3\]"):
        plda.transform(c["X"], c["mu"][:2], c["A"])
    with pytest.raises(ValueError, match=r"expected X as \[rows, 3\]"):
        plda.cosine_score(c["E"], c["Xt"][:, :2])
    with pytest.raises(ValueError, match="enrol_mode is"):
        plda.PLDA(c["mu"], c["Sb"], c["Sw"]).score(c["E"], [0, 1], c["Xt"], enrol_mode="mean")
    with pytest.raises(ValueError, match="no parameters yet"):
        plda.PLDA().score(c["E"], [0, 1], c["Xt"])
    with pytest.raises(ValueError, match=r"expected Sb0 and Sw0 as \[3, 3\]"):
        plda.PLDA().fit(c["X"], c["ids"], Sb0=np.eye(2), Sw0=np.eye(3))
    with pytest.raises(ValueError, match="give Sb0 and Sw0 together, or neither"):
        plda.PLDA().fit(c["X"], c["ids"], Sb0=np.eye(3))
    with pytest.raises(_lib.SRError, match="Sb is not symmetric"):
        plda.PLDA().fit(c["X"], c["ids"], Sb0=_SKEW, Sw0=np.eye(3))
    with pytest.raises(_lib.SRError, match="non-finite value at element 5"):
        plda.PLDA().fit(_bad(c["X"], 5, np.nan), c["ids"], Sb0=np.eye(3), Sw0=np.eye(3))
    if _lib.device_count() == 0:                       # and a call that needs the device says what is missing: no CPU path
        for call in (_train, _score, _fit, _apply, _cosine):
            assert call(L) == -1 and "no HIP device" in _lib.last_error(), call.__name__
        with pytest.raises(_lib.SRError, match="no HIP device"):
            plda.PLDA().fit(c["X"], c["ids"])
        assert plan(1, 3, 2, 2, 4, _ip(en), 64, 0, 0) == -1 and "no HIP device" in _lib.last_error()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_plda_plan_under_asan_ubsan(tmp_path):
    """csrc/plda_plan.cpp -- every refusal's text and the two plans swept over dimensions, label patterns, counts, bounds, the LDS
    option and device sizes -- by a stand-alone program (tests/host/plda_checks.cpp) built with AddressSanitizer + UBSan: host code
    only, no GPU, nothing loaded into Python."""
    exe = str(tmp_path / "plda_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "host", "plda_checks.cpp"), os.path.join(CSRC, "plda_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "plda checks ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_plda_kernels_do_not_spill(built_lib):
    import test_abi_cpu
    res = test_abi_cpu._kernel_resources("plda")
    names = " ".join(res)
    kernels = ("plda_centre_kernel", "plda_class_sums_kernel", "plda_combine_kernel", "plda_invert_kernel", "plda_tri_inverse_kernel", "plda_scale_rows_kernel",
               "plda_update_kernel", "plda_rowdot_kernel", "plda_rownorm_kernel", "plda_assemble_kernel")
    for kernel in kernels:
        assert kernel in names
    assert len(res) == len(kernels)
    for name, r in res.items():
        assert r["scratch"] == 0, (name, r)


def test_refused_in_a_process_forked_after_runtime_use(built_lib):
    """In a child forked after its parent touched the GPU runtime every call says so and names the remedy; the argument refusals and
    the plan still work there."""
    import test_fork
    from speaker_recognition_amd import _lib
    L = built_lib
    L.sr_device_count()                                # (this call is what initialises the runtime in the parent)

    def child():
        out = {"lost": L.sr_gpu_runtime_lost()}
        for name, call in (("train", _train), ("score", _score), ("fit", _fit), ("apply", _apply), ("cosine", _cosine)):
            out[name] = call(L)
            out[name + "_error"] = _lib.last_error()
        out["refusal"] = _train(L, n_iter=0)
        out["refusal_error"] = _lib.last_error()
        out["plan"] = _lib.plda_plan("score", 3, [1, 3], T=4)["n_classes"]
        return out

    out = test_fork._in_forked_child(child)
    assert out["lost"] == 1 and out["refusal"] == -1 and out["plan"] == 2
    for name, symbol in (("train", "sr_plda_train"), ("score", "sr_plda_score"), ("fit", "sr_backend_fit"), ("apply", "sr_backend_apply"),
                         ("cosine", "sr_cosine_score")):
        assert out[name] == -1 and "forked after its parent" in out[name + "_error"] and symbol in out[name + "_error"], out[name + "_error"]
    assert "n_iter is 0" in out["refusal_error"]
    assert L.sr_gpu_runtime_lost() == 0                # the parent is untouched
