"""CPU side of the symmetric eigen-solver, LDA and the diagonalised PLDA scorer (csrc/eig.hip, csrc/eig_plan.cpp, csrc/backend_eig.hip,
speaker_recognition_amd/plda.py): the symbols, the plan and its round-robin schedule (sr_eig_plan -- also under the host sanitizers,
tests/host/eig_checks.cpp), every refusal without a device, the forked-process refusal, the kernels' resource records, the numpy
restatements (tests/eig_cases.py) against each other and the named mutants on the GPU tests' own inputs."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eig_cases as ec  # noqa: E402
import plda_cases as pc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")
NEW = ["sr_sym_eig", "sr_gen_eig", "sr_lda_fit", "sr_backend_project", "sr_plda_score_diag", "sr_eig_plan"]


# ---- the restatements against each other ----

def test_restated_diagonal_score_equals_the_joint_form():
    """R = 5: the score of the model diagonalised by LAPACK is  ln p(enrolment, x) - ln p(enrolment) - ln p(x)  of the Gaussian with
    covariance I (x) Sw + 1 1^T (x) Sb."""
    rng = np.random.default_rng(5)
    R = 5
    Sb, Sw, mu = 2.0 * pc.spd(R, 10.0, rng), pc.spd(R, 10.0, rng), rng.standard_normal(R)
    counts = np.array([1, 2, 3, 2, 1, 3])
    ids = np.repeat(np.arange(6), counts)
    enrol = mu + rng.standard_normal((ids.size, R)) * 1.5
    X = mu + rng.standard_normal((4, R)) * 1.5
    E = np.zeros((6, R))
    np.add.at(E, ids, enrol)
    psi, V = ec.gen_eig(Sb, Sw)
    got = ec.diag_score(mu, V, psi, E, counts, X)
    want = np.array([[pc.joint_score(mu, Sb, Sw, enrol[ids == j], x) for x in X] for j in range(6)])
    f = pc.score(mu, Sb, Sw, E, counts, X, want_factors=True)[1]
    ratio = pc.rel(got, want) / pc.gate_score(R, f)
    print("eig restated diagonal score against the joint form: difference %.3g, difference / gate = %.3g" % (pc.rel(got, want), ratio))
    assert ratio <= 1 and pc.rel(got, want) < 1e-12


@pytest.mark.parametrize("case", pc.SCORE_CASES)
def test_diagonal_form_lies_inside_the_score_gate_and_the_mutants_outside(case):
    """The precondition of the device's gate: the numpy restatement of the diagonal form within 1e-2 of gate_score alone on every
    case; and every mutant that can show on the case outside the whole gate (at the solver's cap: the widest it can be)."""
    R, J, T = case
    c = pc.score_case(R, J, T)
    kappa = float(np.linalg.cond(c["Sw"]))
    assert kappa <= pc.KAPPA_MAX
    psi, V = ec.gen_eig(c["Sb"], c["Sw"])
    got = ec.diag_score(c["mu"], V, psi, c["E"], c["counts"], c["X"])
    ratio = pc.rel(got, c["want"]) / pc.gate_score(R, c["factors"])
    print("eig restated diagonal score %s: difference / gate_score = %.3g" % (case, ratio))
    assert ratio <= 1e-2
    g = ec.gate_diag_score(R, c["factors"], kappa, ec.MAX_SWEEPS)
    assert g < 1e-4
    for name in ec.DIAG_MUTANTS:
        if not ec.diag_mutant_shows(name, R, c["counts"]):
            continue
        bad = pc.rel(ec.diag_score(c["mu"], V, psi, c["E"], c["counts"], c["X"], mutant=name), c["want"]) / g
        print("eig mutant %s, scoring %s: difference / gate = %.3g" % (name, case, bad))
        assert bad > 1, (name, bad)


@pytest.mark.parametrize("case", ec.LDA_CASES, ids=["R%d-%dclasses" % (R, len(c)) for R, c in ec.LDA_CASES])
def test_restated_lda_whitens_within_and_diagonalises_between(case):
    R, counts = case                                   # the GPU test's corpora
    c = pc.corpus(R, counts, 900 + R + len(counts))
    n, S = c["X"].shape[0], len(counts)
    dims = ec.lda_dims(R, counts)
    assert dims[-1] == min(R, S - 1) and n - S > R
    for P in dims:
        mu, A, psi, Sw, Sb = ec.lda(c["X"], c["ids"], P)
        kappa = float(np.linalg.cond(Sw))
        g = kappa * (pc.gate_cov(R, n, 1.0) + ec.gate(R, 1))
        assert kappa <= pc.KAPPA_MAX and A.shape == (P, R) and np.all(np.diff(psi) <= 0)
        assert np.abs(A @ Sw @ A.T - np.eye(P)).max() <= g
        assert np.abs(A @ Sb @ A.T - np.diag(psi)).max() / psi[0] <= g
        assert pc.rel(Sw + Sb, pc.total_cov(c["X"])) <= pc.gate_cov(R, n, 1.0)           # Sb + Sw is the total covariance
    all_psi = ec.gen_eig(Sb, Sw)[0]
    if S - 1 < R:                                      # Sb has rank classes - 1: the values past it are rounding, the last kept is not
        assert np.abs(all_psi[S - 1:]).max() <= g * all_psi[0] < all_psi[S - 2]
    # V not transposed in the projection: the within-class covariance of what comes out is no identity
    _, A, _, Sw, _ = ec.lda(c["X"], c["ids"], R)
    W = pc.within_cov(ec.project(c["X"], mu, A, False, mutant="transposed"), c["ids"])
    assert np.abs(W - np.eye(R)).max() > g
    W = pc.within_cov(ec.project(c["X"], mu, A, False), c["ids"])
    assert np.abs(W - np.eye(R)).max() <= g


@pytest.mark.parametrize("R", (3, 33, 65, 97))
def test_the_model_of_the_block_sweep_meets_the_gates_and_the_row_mutant_does_not(R):
    """The numpy model of csrc/eig.hip's sweep (blocks of 32, the same round robin, rotations from the identity with the inner
    angle) on the GPU tests' inputs: converged, inside the gates; with Q for Q^T in the row stage it is not a similarity any more."""
    for kind in ec.KINDS:
        A = ec.matrix(kind, R)
        w, V, sweeps, converged = ec.block_jacobi(A, 32)
        assert converged == 1 and sweeps <= ec.SEPARATED_SWEEPS, (kind, sweeps)
        g = ec.gate(R, sweeps)
        assert max(ec.figures(A, w, V)) <= g, (kind, ec.figures(A, w, V), g)
        assert np.array_equal(V, ec.fix_signs(V)) and np.all(np.diff(w) <= 0)
    if R > 64:
        A = ec.matrix("spd10", R)
        w, V, sweeps, converged = ec.block_jacobi(A, 32, mutant="row_q", cap=6)
        ev, res, orth = ec.figures(A, w, V)
        print("eig mutant row_q R=%d: eigenvalues / gate = %.3g" % (R, ev / ec.gate(R, sweeps)))
        assert max(ev, res) > ec.gate(R, sweeps)
    # psi ascending where descending is read: the sorted diagonal input comes back reversed
    w, V, _, _ = ec.block_jacobi(ec.matrix("sorted_diag", R), 32)
    assert np.array_equal(w, np.arange(R, 0, -1.0)) and (R == 1 or not np.array_equal(w, w[::-1]))


# ---- the library without a device ----

def test_symbols_exported_declared_and_prototyped(built_lib):
    from speaker_recognition_amd import _lib, plda
    header = open(os.path.join(ROOT, "include", "pygmm_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), "lib/pygmm.so does not export %s" % name
        assert re.search(r"\bint %s\(" % name, header), "%s is not declared in include/pygmm_hip.h" % name
        assert name in _lib.EXT_SYMBOLS and getattr(built_lib, name).argtypes is not None
    assert "SR_T_COUNT 20" in header                   # no timer kind is added
    assert header.count("Writes 24 fields") == 1 and header.count("Writes 36 fields") == 1
    for name in ("sym_eig", "gen_eig", "LDA", "DiagPLDA"):
        assert callable(getattr(plda, name))
    assert callable(plda.PLDA.diagonalise) and callable(_lib.eig_plan) and plda.KINDS == ("whiten", "wccn")
    assert "no eigen-solver" not in plda.__doc__ and "needs no\neigen-solver" not in plda.__doc__


def test_plan_blocks_phantom_rounds_and_schedule(built_lib):
    from speaker_recognition_amd import _lib
    b = _lib.eig_plan(1)["b"]
    assert b == 32 and _lib.eig_plan(512)["max_R"] == 512
    for R in sorted(set(ec.shapes(b) + [5 * b, 400, 512])):
        p = _lib.eig_plan(R)
        blocks = -(-R // b)
        assert (p["R"], p["blocks"], p["phantom"], p["single"]) == (R, blocks, blocks % 2, int(R <= 2 * b))
        assert p["max_sweeps"] == 40 and p["sub_problem"] == 2 * b and p["solve_lds"] <= 160 * 1024 and p["update_lds"] <= 160 * 1024
        if p["single"]:
            assert p["rounds"] == 0 and p["schedule"] == [] and p["solve_grid"] == 1
            continue
        players = blocks + blocks % 2
        assert (p["rounds"], p["pairs"], p["solve_grid"]) == (players - 1, players // 2, players // 2 - blocks % 2)
        assert (p["cols_x"], p["cols_y"], p["cols_z"], p["rows_x"], p["rows_y"]) == (p["solve_grid"], -(-R // 64), 2, p["solve_grid"], -(-R // 64))
        assert p["launches_per_sweep"] == 3 * p["rounds"] + 2
        met = {}
        for rnd in p["schedule"]:
            flat = [x for pair in rnd for x in pair]
            assert len(flat) == len(set(flat)) == players                               # no block twice in a round: everyone plays
            assert sum(q >= blocks for _, q in rnd) == blocks % 2                        # one phantom pair a round, and it does no work:
            assert all(p_ < blocks for p_, _ in rnd)                                     # it is left out of the solve stage's grid
            for pair in rnd:
                assert pair[0] < pair[1]
                met[pair] = met.get(pair, 0) + 1
        assert len(met) == players * (players - 1) // 2 and set(met.values()) == {1}    # every pair exactly once per sweep
        for n_cu in (1, 64):                           # the device's size moves nothing but the rounds over the chip
            o = _lib.eig_plan(R, n_cu=n_cu)
            assert o["pair_rounds"] == -(-(p["cols_x"] * p["cols_y"] * 2) // n_cu)
            assert all(o[k] == p[k] for k in p if k != "pair_rounds")
    assert ec.block_jacobi(ec.matrix("spd10", 97), b, schedule=_lib.eig_plan(97)["schedule"])[3] == 1      # the plan's own table drives the model


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None


def _case():
    rng = np.random.default_rng(2)
    R = 3
    return dict(R=R, n=8, X=rng.standard_normal((8, R)), ids=np.array([0, 1, 1, 0, 2, 1, 2, 0], dtype=np.int64), S=3, P=2, mu=rng.standard_normal(R),
                A=np.eye(3) * 2.0, Sb=np.eye(R) * 2.0, Sw=np.eye(R), V=np.eye(R), psi=np.array([2.0, 1.0, 0.5]), J=2, T=4,
                E=rng.standard_normal((2, R)), en=np.array([1, 3], dtype=np.int64), Xt=rng.standard_normal((4, R)), Ap=np.eye(R)[:2])


def _sym(L, **over):
    a = dict(_case(), **over)
    w, V = np.zeros(max(a["R"], 1)), np.zeros((max(a["R"], 1),) * 2)
    return L.sr_sym_eig(a["R"], _dp(a["A"]), _dp(w) if a.get("w", 1) is not None else None, _dp(V), None, None)


def _gen(L, **over):
    a = dict(_case(), **over)
    psi, V = np.zeros(max(a["R"], 1)), np.zeros((max(a["R"], 1),) * 2)
    return L.sr_gen_eig(a["R"], _dp(a["Sb"]), _dp(a["Sw"]), _dp(psi), _dp(V) if a.get("out", 1) is not None else None, None, None)


def _lda(L, **over):
    a = dict(_case(), **over)
    mu, A, psi = np.zeros(max(a["R"], 1)), np.zeros((max(a["P"], 1), max(a["R"], 1))), np.zeros(max(a["P"], 1))
    return L.sr_lda_fit(a["n"], a["R"], _dp(a["X"]), _ip(a["ids"]), a["S"], a["P"], _dp(mu), _dp(A) if a.get("out", 1) is not None else None, _dp(psi))


def _project(L, **over):
    a = dict(_case(), **over)
    Y = np.zeros((max(a["n"], 1), max(a["P"], 1)))
    return L.sr_backend_project(a["n"], a["R"], a["P"], _dp(a["X"]), _dp(a["mu"]), _dp(a["Ap"]), 1, _dp(Y), None)


def _score(L, **over):
    a = dict(_case(), **over)
    out = np.zeros((max(a["J"], 1), max(a["T"], 1)))
    return L.sr_plda_score_diag(a["J"], a["T"], a["R"], _dp(a["mu"]), _dp(a["V"]), _dp(a["psi"]), _dp(a["E"]), _ip(a["en"]), _dp(a["Xt"]), _dp(out), None)


def _bad(arr, idx, value):
    out = np.array(arr, dtype=np.float64)
    out.flat[idx] = value
    return out


_C = _case()
_SKEW = np.array([[2.0, 0.5, 0.0], [0.1, 2.0, 0.0], [0.0, 0.0, 2.0]])
REFUSALS = [
    (_sym, dict(R=0), "R >= 1"), (_sym, dict(R=513), "up to 512 rows, this one has 513; reduce the dimension"), (_sym, dict(A=None), r"null argument \(A \[R\]\[R\]\)"),
    (_sym, dict(A=_bad(_C["A"], 4, np.nan)), "A holds a non-finite value at element 4"), (_sym, dict(A=_SKEW), r"A is not symmetric .* pass \(A \+ A\^T\) / 2"),
    (_sym, dict(w=None), r"null argument \(w \[R\] and V"),
    (_gen, dict(R=0), "R >= 1"), (_gen, dict(R=600), "up to 512 rows"), (_gen, dict(Sb=None), r"null argument \(Sb"), (_gen, dict(Sw=None), r"null argument \(Sw"),
    (_gen, dict(Sb=_SKEW), "Sb is not symmetric"), (_gen, dict(Sw=_SKEW.T), "Sw is not symmetric"), (_gen, dict(Sw=_bad(_C["Sw"], 8, np.inf)), "Sw holds a non-finite value at element 8"),
    (_gen, dict(out=None), r"null argument \(psi \[R\] and V"),
    (_lda, dict(R=0), "R >= 1"), (_lda, dict(R=513), "up to 512 dimensions"), (_lda, dict(n=0), "n, the number of training vectors is 0; pass at least one row"),
    (_lda, dict(X=None), r"null argument \(X"), (_lda, dict(ids=None), r"null argument \(ids"), (_lda, dict(S=2), "row 4 has label 2, outside 0 .. 1; renumber the speakers"),
    (_lda, dict(S=4), "label 3 of 0 .. 3 has no row"), (_lda, dict(X=_bad(_C["X"], 5, np.nan)), "non-finite value at element 5; drop that vector"),
    (_lda, dict(P=0), r"P, the dimensions kept, is 0.*1 <= P <= min\(R, classes - 1\)"), (_lda, dict(P=3), "rank at most 2"), (_lda, dict(out=None), r"null argument \(mu \[R\], A \[P\]\[R\]"),
    (_project, dict(R=513), "up to 512 dimensions"), (_project, dict(n=0), "n, the number of vectors is 0"), (_project, dict(P=0), "P, the rows of A, is 0.*1 <= P <= R"),
    (_project, dict(P=4), "P, the rows of A, is 4"), (_project, dict(mu=None), r"null argument \(mu"), (_project, dict(Ap=_bad(_C["Ap"], 5, np.nan)), "A holds a non-finite value at element 5"),
    (_project, dict(X=_bad(_C["X"], 3, np.nan)), "X, the vectors .* element 3"),
    (_score, dict(R=0), "R >= 1"), (_score, dict(R=600), "up to 512 dimensions"), (_score, dict(J=0), "J, the number of models is 0"), (_score, dict(T=0), "T, the number of test segments is 0"),
    (_score, dict(E=None), r"null argument \(E"), (_score, dict(Xt=None), r"null argument \(X"), (_score, dict(mu=None), r"null argument \(mu \[R\], V"), (_score, dict(psi=None), r"null argument \(mu \[R\], V"),
    (_score, dict(en=None), r"null argument \(enrol_n"), (_score, dict(en=np.array([1, 0], dtype=np.int64)), "enrol_n of model 1 is 0"),
    (_score, dict(V=_bad(_C["V"], 7, np.nan)), "V holds a non-finite value at element 7"), (_score, dict(mu=_bad(_C["mu"], 0, np.nan)), "mu holds a non-finite value at element 0"),
    (_score, dict(Xt=_bad(_C["Xt"], 2, np.nan)), "X, the test vectors .* element 2"),
]


def test_refusals_need_no_device(built_lib):
    """Every refusal fails on its arguments alone, with a text that names the argument and the remedy -- never the device."""
    from speaker_recognition_amd import _lib, plda
    L = built_lib
    for call, over, pat in REFUSALS:
        assert call(L, **over) == -1, (call.__name__, over)
        assert re.search(pat, _lib.last_error()) and "HIP" not in _lib.last_error(), (call.__name__, over, _lib.last_error())
    out = (C.c_int64 * 24)()
    assert L.sr_eig_plan(5, 256, out, 23, None) == -1 and "24 fields" in _lib.last_error()
    assert L.sr_eig_plan(5, 256, None, 24, None) == -1 and "null argument" in _lib.last_error()
    assert L.sr_eig_plan(0, 256, out, 24, None) == -1 and "R >= 1" in _lib.last_error()
    assert L.sr_eig_plan(200, 256, out, 24, None) == 24 and (out[1], out[2], out[3], out[4]) == (32, 7, 1, 7)
    # the Python layer
    c = _case()
    with pytest.raises(ValueError, match=r"expected A as a square"):
        plda.sym_eig(np.zeros((3, 2)))
    with pytest.raises(ValueError, match=r"expected Sw as a square \[3, 3\]"):
        plda.gen_eig(c["Sb"], np.eye(2))
    with pytest.raises(ValueError, match=r"n_dims is 3; 3 classes in 3 dimensions leave 1 <= n_dims <= min\(R, classes - 1\) = 2"):
        plda.LDA().fit(c["X"], c["ids"], 3)
    with pytest.raises(ValueError, match="n_dims is 0"):
        plda.LDA().fit(c["X"], c["ids"], 0)
    with pytest.raises(ValueError, match=r"one label per row as ids \(8\), got 5"):
        plda.LDA().fit(c["X"], c["ids"][:5], 1)
    with pytest.raises(ValueError, match="no parameters yet"):
        plda.LDA().transform(c["X"])
    with pytest.raises(ValueError, match=r"expected X as \[rows, 3\]"):
        plda.LDA(c["mu"], c["Ap"]).transform(c["X"][:, :2])
    with pytest.raises(ValueError, match=r"expected A as \[n_dims <= 3, 3\]"):
        plda.LDA(c["mu"], np.eye(2)).transform(c["X"])
    with pytest.raises(ValueError, match=r"expected psi \[3\]"):
        plda.DiagPLDA(c["mu"], c["V"], c["psi"][:2])
    with pytest.raises(ValueError, match=r"expected V as a square \[3, 3\]"):
        plda.DiagPLDA(c["mu"], np.eye(2), c["psi"])
    with pytest.raises(ValueError, match="enrol_mode is"):
        plda.DiagPLDA(c["mu"], c["V"], c["psi"]).score(c["E"], [0, 1], c["Xt"], enrol_mode="mean")
    with pytest.raises(ValueError, match="no parameters yet"):
        plda.PLDA().diagonalise()
    with pytest.raises(_lib.SRError, match="A is not symmetric"):
        plda.sym_eig(_SKEW)
    if _lib.device_count() == 0:                       # and a call that needs the device says what is missing: no CPU path
        for call in (_sym, _gen, _lda, _project, _score):
            assert call(L) == -1 and "no HIP device" in _lib.last_error(), call.__name__
        with pytest.raises(_lib.SRError, match="no HIP device"):
            plda.sym_eig(np.eye(3))
        assert L.sr_eig_plan(5, 0, out, 24, None) == -1 and "no HIP device" in _lib.last_error()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_eig_plan_under_asan_ubsan(tmp_path):
    """csrc/eig_plan.cpp -- every refusal's text, the plan and its schedule at every R of 1 .. 512, the scorer's chunks -- by a
    stand-alone program (tests/host/eig_checks.cpp) built with AddressSanitizer + UBSan: host code only, no GPU, nothing loaded
    into Python."""
    exe = str(tmp_path / "eig_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "host", "eig_checks.cpp"), os.path.join(CSRC, "eig_plan.cpp"), os.path.join(CSRC, "plda_plan.cpp"),
           "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "eig checks ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_eig_kernels_do_not_spill(built_lib):
    import test_abi_cpu
    eig = test_abi_cpu._kernel_resources("eig")
    want = ("eig_single_kernel", "eig_pair_solve_kernel", "eig_update_kernel", "eig_rowmax_kernel", "eig_max_kernel", "eig_identity_kernel",
            "eig_rank_kernel", "eig_gather_kernel")
    assert len(eig) == len(want) and all(any(k in name for name in eig) for k in want), sorted(eig)
    back = test_abi_cpu._kernel_resources("backend_eig")
    want = ("beig_symmetrise_kernel", "beig_scale_rows_kernel", "beig_models_kernel", "beig_square_kernel", "beig_assemble_kernel")
    assert len(back) == len(want) and all(any(k in name for name in back) for k in want), sorted(back)
    for name, r in list(eig.items()) + list(back.items()):
        assert r["scratch"] == 0, (name, r)
    assert len(test_abi_cpu._kernel_resources("plda")) == 10                             # plda.hip's kernels are as they were


def test_refused_in_a_process_forked_after_runtime_use(built_lib):
    """In a child forked after its parent touched the GPU runtime every call says so and names the remedy; the argument refusals and
    the plan still work there."""
    import test_fork
    from speaker_recognition_amd import _lib
    L = built_lib
    L.sr_device_count()                                # (this call is what initialises the runtime in the parent)

    def child():
        out = {"lost": L.sr_gpu_runtime_lost()}
        for name, call in (("sym", _sym), ("gen", _gen), ("lda", _lda), ("project", _project), ("score", _score)):
            out[name] = call(L)
            out[name + "_error"] = _lib.last_error()
        out["refusal"] = _sym(L, A=_SKEW)
        out["refusal_error"] = _lib.last_error()
        out["plan"] = _lib.eig_plan(200)["rounds"]
        return out

    out = test_fork._in_forked_child(child)
    assert out["lost"] == 1 and out["refusal"] == -1 and out["plan"] == 7
    for name, symbol in (("sym", "sr_sym_eig"), ("gen", "sr_gen_eig"), ("lda", "sr_lda_fit"), ("project", "sr_backend_project"),
                         ("score", "sr_plda_score_diag")):
        assert out[name] == -1 and "forked after its parent" in out[name + "_error"] and symbol in out[name + "_error"], out[name + "_error"]
    assert "A is not symmetric" in out["refusal_error"]
    assert L.sr_gpu_runtime_lost() == 0                # the parent is untouched
