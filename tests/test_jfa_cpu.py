"""CPU side of the JFA factor estimation (csrc/jfa.hip, csrc/jfa_plan.cpp, jfa.py): the float64 restatement (tests/jfa_cases.py)
against itself in the reference's two shapes and against hand cases, the evidence that it is the EM step (its objective never
decreases), jfa.py's host-side centring and label handling with the device call replaced by the restatement, the plan
(sr_jfa_plan -- also under the host sanitizers, tests/host/jfa_checks.cpp), the symbols, the refusals that must not need a device,
the kernels' resource records, and that nothing of the present surface reaches the new entry points."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")
NEW = ["sr_jfa_open", "sr_jfa_factors", "sr_jfa_update", "sr_jfa_train", "sr_jfa_close", "sr_jfa_plan"]


def test_restated_entry_points_agree_with_factors():
    c = jc.corpus(9, 4, 3, 5, 3, sessions=1)
    F, N, ids, m, E = c["F"], c["N"], c["spk_ids"], c["m"], c["E"]
    W = jc.random_start(5, E, 2)
    Fc = F - m * np.repeat(N, 3, axis=1)                                # centred by hand: one session per speaker
    y, A, Cm = jc.factors(N, Fc, E, W)
    y3, A3, C3 = jc.estimate_y_and_v(F, N, None, m, E, 0, W, 0, np.zeros((9, 1)), 0, np.zeros((9, 1)), ids, nargout=3)
    assert np.allclose(y3, y, rtol=0, atol=1e-13) and np.allclose(A3, A, rtol=1e-13) and np.allclose(C3, Cm, rtol=0, atol=1e-10)
    # every session its own speaker, y = 0: estimate_x_and_u is the same computation
    x3, Ax, Cx = jc.estimate_x_and_u(F, N, None, m, E, 0, 0, W, np.zeros((9, 1)), 0, 0, ids, nargout=3)
    assert np.allclose(x3, y, rtol=0, atol=1e-13) and np.allclose(Ax, A, rtol=1e-13) and np.allclose(Cx, Cm, rtol=0, atol=1e-10)
    _, v2 = jc.estimate_y_and_v(F, N, None, m, E, 0, W, 0, 0, 0, 0, ids, nargout=2)
    assert np.allclose(v2, jc.update(A, Cm, W)[0], rtol=1e-12, atol=1e-14)
    # the inv form and the Cholesky-solve form of one step
    ys, As, Cs = jc.factors_solve(N, Fc, E, W)
    assert jc.rel(ys, y) < 1e-12 and jc.rel(As, A) < 1e-12 and jc.rel(Cs, Cm) < 1e-12


@pytest.mark.parametrize("shape", [jc.SHAPES[0], jc.SHAPES[1], jc.SHAPES[3]])
def test_objective_never_decreases(shape):
    """J(W) = sum_g (-1/2 ln det L_g + 1/2 b_g^T L_g^-1 b_g) over 8 restated iterations from the reference's random start: the
    evidence that the restatement is the EM step the reference implements.  Measured: the smallest step is +0.50 (second shape)."""
    c = jc.case(*shape)
    Ns, Fs, E, W = c["Ns"], c["Fs"], c["E"], c["W0"]
    Js = [jc.objective(Ns, Fs, E, W)]
    for _ in range(8):
        W = jc.step(Ns, Fs, E, W)[0]
        Js.append(jc.objective(Ns, Fs, E, W))
    print("objective", shape, ["%.6g" % j for j in Js])
    assert (np.diff(Js) > 0).all()
    assert c["kL"] <= 1e6 and c["kA"] <= 1e6


def test_z_and_d_and_linear_scoring_hand_case():
    """K = 2, D = 1, one speaker with one session: N = (2, 4), F = (3, 10), m = (1, 2), E = (1, 4), d = (1, 2).
    Fs = F - m N = (1, 2); L = 1 + N / E d^2 = (3, 5); z = Fs / E d / L = (1/3, 1/5); a = (1 / L + z^2) N = (8/9, 24/25);
    b = z Fs = (1/3, 2/5); d' = b / a = (3/8, 5/12).  Score of the segment against the model z d: M = z d / E = (1/3, 1/10),
    (F - m N) / sum N = (1/6, 1/3): 1/18 + 1/30 = 4/45."""
    from speaker_recognition_amd import jfa
    F, N, m, E, d = np.array([[3.0, 10.0]]), np.array([[2.0, 4.0]]), np.array([1.0, 2.0]), np.array([1.0, 4.0]), np.array([1.0, 2.0])
    for mod in (jc, jfa):
        z, a, b = mod.estimate_z_and_d(F, N, None, m, E, d, 0, 0, 0, 0, 0, np.array([0]), nargout=3)
        assert np.allclose(z, [[1 / 3, 0.2]], rtol=1e-15) and np.allclose(a, [8 / 9, 0.96], rtol=1e-15) and np.allclose(b, [1 / 3, 0.4], rtol=1e-15)
        z2, d2 = mod.estimate_z_and_d(F, N, None, m, E, d, 0, 0, 0, 0, 0, np.array([0]), nargout=2)
        assert np.allclose(d2, [0.375, 5 / 12], rtol=1e-15) and np.array_equal(z2, z)
        assert np.array_equal(mod.estimate_z_and_d(F, N, None, m, E, d, 0, 0, 0, 0, 0, np.array([0])), z)
        kw = {} if mod is jc else {"scores": 0}
        s = mod.linear_scoring(F, N, None, m, E, d, np.zeros((1, 2)), 0, z, np.zeros((1, 1)), 0, **kw)
        assert s.shape == (1, 1) and abs(s[0, 0] - 4 / 45) < 1e-16
    assert np.allclose(jfa.estimate_z_and_d(a, b), [0.375, 5 / 12], rtol=1e-15)           # d = estimate_z_and_d(a, b)


class _HostEstimator:
    """jfa.FactorEstimator with the device replaced by the restatement: what reaches it is what jfa.py's host side formed."""
    seen = []

    def __init__(self, N, Fc, E):
        self.N, self.Fc, self.E = np.array(N), np.array(Fc), np.array(E)
        _HostEstimator.seen.append(self)

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


def test_python_layer_centring_labels_and_scalars(monkeypatch):
    from speaker_recognition_amd import jfa
    monkeypatch.setattr(jfa, "FactorEstimator", _HostEstimator)
    monkeypatch.setattr(jfa, "update_loadings", lambda A, Cm, W, return_skipped=False: jc.update(A, Cm, np.broadcast_to(W, Cm.shape))[0])
    G, K, D, R = 6, 4, 3, 5
    c = jc.corpus(G, K, D, R, 9)
    F, N, ids, m, E = c["F"], c["N"], c["spk_ids"], c["m"], c["E"]
    rng = np.random.default_rng(4)
    n, kd = F.shape
    v, u = jc.random_start(R, E, 1), jc.random_start(2, E, 2)
    x, z, d, y = rng.standard_normal((n, 2)), 0.1 * rng.standard_normal((G, kd)), 0.05 + 0.1 * rng.random(kd), rng.standard_normal((G, R))
    for nargout in (1, 2, 3):
        got = jfa.estimate_y_and_v(F, N, None, m, E, d, v, u, z, 0, x, ids, nargout=nargout)
        want = jc.estimate_y_and_v(F, N, None, m, E, d, v, u, z, 0, x, ids, nargout=nargout)
        for a, b in zip(got if nargout > 1 else [got], want if nargout > 1 else [want]):
            assert a.shape == b.shape and jc.rel(a, b) < 1e-11
        got = jfa.estimate_x_and_u(F, N, None, m, E, d, v, u, z, y, 0, ids, nargout=nargout)
        want = jc.estimate_x_and_u(F, N, None, m, E, d, v, u, z, y, 0, ids, nargout=nargout)
        for a, b in zip(got if nargout > 1 else [got], want if nargout > 1 else [want]):
            assert a.shape == b.shape and jc.rel(a, b) < 1e-11
    # groups are speakers: the handle saw G rows of summed, centred statistics; then n sessions
    assert _HostEstimator.seen[0].N.shape == (G, K) and _HostEstimator.seen[1].N.shape == (n, K)
    # the sc_* scripts' call: scalars 0 and columns of zeros; labels with a gap leave rows of zeros
    gap = np.where(ids >= 2, ids + 3, ids)
    yg = jfa.estimate_y_and_v(F, N, [], m, E, 0, v, 0, np.zeros((G + 3, 1)), 0, np.zeros((n, 1)), gap)
    yp = jc.estimate_y_and_v(F, N, None, m, E, 0, v, 0, 0, 0, 0, ids)
    assert yg.shape == (G + 3, R) and not yg[2:5].any() and jc.rel(np.delete(yg, (2, 3, 4), axis=0), yp) < 1e-12
    zg = jfa.estimate_z_and_d(F, N, None, m, E, d, v, u, 0, np.insert(y, [2, 2, 2], 0.0, axis=0), x, gap)
    assert zg.shape == (G + 3, kd) and not zg[2:5].any()
    assert jc.rel(np.delete(zg, (2, 3, 4), axis=0), jc.estimate_z_and_d(F, N, None, m, E, d, v, u, 0, y, x, ids)) < 1e-12
    xs = jfa.estimate_x_and_u(F, N, None, m, E, 0, v, u, np.zeros((G, 1)), y, np.zeros((n, 1)), ids)
    assert jc.rel(xs, jc.estimate_x_and_u(F, N, None, m, E, 0, v, u, 0, y, 0, ids)) < 1e-12
    for bad in (ids[:-1], ids.astype(float), np.where(ids == 0, -1, ids)):
        with pytest.raises(ValueError, match="0-based integer labels"):
            jfa.estimate_y_and_v(F, N, None, m, E, 0, v, 0, 0, 0, 0, bad)
    # the drivers: the chain of the restatement on the same statistics
    ubm = (np.full(K, 1.0 / K), m.reshape(K, D), E.reshape(K, D))
    vt = jfa.train_v(F, N, ids, ubm, ny=3, niter=2)
    assert jc.rel(vt, jc.train_v(F, N, ids, m, E, 3, 2)) < 1e-12
    ut = jfa.train_u(F, N, ids, ubm, vt, nx=2, niter=2, seed=1)
    assert jc.rel(ut, jc.train_u(F, N, ids, m, E, vt, 2, 2, seed=1)) < 1e-11
    dt = jfa.train_d(F, N, ids, ubm, vt, ut, niter=2, seed=2)
    assert jc.rel(dt, jc.train_d(F, N, ids, m, E, vt, ut, 2, seed=2)) < 1e-11
    s = jfa.score_dot_product({"F": F[0::3], "N": N[0::3]}, (F[1::3], N[1::3]), ubm, vt, ut, dt)
    assert jc.rel(s, jc.score_dot_product((F[0::3], N[0::3]), (F[1::3], N[1::3]), m, E, vt, ut, dt)) < 1e-11
    assert np.array_equal(jfa.random_loadings(3, E, 7), jc.random_start(3, E, 7))


def test_symbols_exported_and_declared(built_lib):
    from speaker_recognition_amd import _lib
    header = open(os.path.join(ROOT, "include", "pygmm_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), "lib/pygmm.so does not export %s" % name
        assert re.search(r"\b(int|void|SRJfa \*)\s?%s\(" % name, header), "%s is not declared in include/pygmm_hip.h" % name
        assert name in _lib.EXT_SYMBOLS
    for text in ("jfa_scratch_mib", "jfa_lds_rows", "SR_T_JFA_GRAM 13", "SR_T_JFA_GEMM_L 14", "SR_T_JFA_GEMM_B 15", "SR_T_JFA_GEMM_A 16",
                 "SR_T_JFA_GEMM_C 17", "SR_T_JFA_FACTOR 18", "SR_T_JFA_UPDATE 19", "SR_T_COUNT 20", "typedef struct SRJfa SRJfa;"):
        assert text in header
    assert (_lib.T_JFA_GRAM, _lib.T_JFA_GEMM_L, _lib.T_JFA_GEMM_B, _lib.T_JFA_GEMM_A, _lib.T_JFA_GEMM_C, _lib.T_JFA_FACTOR, _lib.T_JFA_UPDATE) == tuple(range(13, 20))
    for name in ("sr_bw_stats_batch", "sr_score_batch_set", "sr_train_f32"):
        assert hasattr(raw, name)                      # the siblings stay


def test_plan_chunks_paths_and_bytes(built_lib):
    from speaker_recognition_amd import _lib
    for G in (1, 15, 16, 17, 70, 1000):
        for K, D in ((1, 1), (5, 39), (512, 39)):
            for R in (1, 17, 65, 112, 113, 300, 320):
                block = R * R * 8
                for bound in (16 * block, 33 * block + 5, 1 << 20, 1 << 30):
                    if bound // block < min(G, 16):
                        continue
                    p = _lib.jfa_plan(G, K, D, R, bound)
                    chunk, n = p["chunk"], p["n_chunks"]
                    assert 1 <= chunk <= G and chunk * block <= bound == max(bound, p["bytes_scratch"])          # the bound holds
                    assert n == -(-G // chunk) and (n - 1) * chunk < G <= n * chunk                              # every group once
                    assert n == 1 or chunk % p["k_step"] == 0                                                    # whole reduction steps
                    assert p["k_step"] == 16 and p["max_R"] >= 320
                    assert (p["bytes_N"], p["bytes_Fc"], p["bytes_P"], p["bytes_C"]) == (G * K * 8, G * K * D * 8, K * block, R * K * D * 8)
                    assert p["path"] == ("lds" if R <= 112 else "global") and p["factor_lds"] <= 160 * 1024
                    assert p["gemm_L_x"] == -(-R * R // 64) and p["gemm_L_y"] == -(-chunk // 64) and p["gemm_A_y"] == -(-K // 64)
                    assert p["gemm_b_x"] == -(-R // 64) and p["gemm_C_x"] == -(-K * D // 64) and p["gemm_C_y"] == -(-R // 64)
                    assert p["gram_grid_x"] == K and p["gram_grid_y"] == (-(-R // 16)) ** 2
    # the path switches at jfa_lds_rows; 1 forces the global-memory factorisation at any R > 1
    for lds_rows, R, want in ((0, 112, "lds"), (0, 113, "global"), (17, 17, "lds"), (17, 18, "global"), (1, 17, "global"), (1, 2, "global"),
                              (1, 1, "lds"), (112, 112, "lds"), (64, 65, "global")):
        assert _lib.jfa_plan(33, 5, 13, R, lds_rows=lds_rows)["path"] == want
    assert _lib.jfa_plan(70, 5, 39, 65, 1 << 20)["n_chunks"] == 5                  # 65^2 x 8 B = 33 KiB a group: 16 at a time under 1 MiB
    p = _lib.jfa_plan(1000, 512, 39, 320)
    assert p["path"] == "global" and p["n_chunks"] == 1 and p["bytes_scratch"] == 1000 * 320 * 320 * 8
    for key, bad in (("jfa_scratch_mib", 0), ("jfa_scratch_mib", (1 << 20) + 1), ("jfa_lds_rows", -1), ("jfa_lds_rows", 113)):
        with pytest.raises(_lib.SRError, match=key):
            _lib.set_option(key, bad)
    _lib.set_option("jfa_scratch_mib", 1024)
    _lib.set_option("jfa_lds_rows", 0)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_refusals_need_no_device(built_lib):
    """Every refusal fails on its arguments alone, with a text that names the argument -- never the device."""
    from speaker_recognition_amd import _lib, jfa
    L = built_lib
    G, K, D, R = 3, 2, 2, 2
    N, Fc, E, W = np.ones((G, K)), np.zeros((G, K * D)), np.ones(K * D), np.ones((R, K * D))
    A, Cm = np.stack([np.eye(R)] * K), np.ones((R, K * D))

    def opened(G=G, K=K, D=D, N=N, Fc=Fc, E=E):
        return L.sr_jfa_open(G, K, D, _dp(N) if N is not None else None, _dp(Fc), _dp(E))

    def bad(arr, idx, value):
        out = np.array(arr)
        out.flat[idx] = value
        return out

    for kw, pat in ((dict(G=0), "G, K, D >= 1"), (dict(K=0), "G, K, D >= 1"), (dict(D=0), "G, K, D >= 1"), (dict(N=None), "null argument"),
                    (dict(N=bad(N, 3, np.nan)), "N holds a non-finite value at element 3"), (dict(N=bad(N, 4, -0.5)), "negative occupancy at group 2, mixture 0"),
                    (dict(Fc=bad(Fc, 5, np.inf)), "Fc holds a non-finite value at element 5"), (dict(E=bad(E, 1, 0.0)), "E must be positive, element 1"),
                    (dict(E=bad(E, 2, np.nan)), "E holds a non-finite value")):
        assert opened(**kw) is None, kw
        assert re.search(pat, _lib.last_error()) and "HIP" not in _lib.last_error(), _lib.last_error()
    out = (C.c_int64 * 32)()
    for args, pat in (((G, K, D, 0, 1 << 30, 0, 256), "R >= 1"), ((G, K, D, 513, 1 << 30, 0, 256), "up to 512 factors, the loading matrix has 513"),
                      ((70, 5, 39, 65, 16 * 65 * 65 * 8 - 1, 0, 256), "raise the option jfa_scratch_mib"), ((G, K, D, R, 1 << 30, 113, 256), "jfa_lds_rows"),
                      ((0, K, D, R, 1 << 30, 0, 256), "G, K, D >= 1")):
        assert L.sr_jfa_plan(*args, out, 32) == -1 and re.search(pat, _lib.last_error()) and "HIP" not in _lib.last_error(), _lib.last_error()
    assert L.sr_jfa_plan(G, K, D, R, 1 << 30, 0, 256, out, 31) == -1 and "32 fields" in _lib.last_error()
    assert L.sr_jfa_plan(G, K, D, R, 1 << 30, 0, 256, None, 32) == -1 and "null argument" in _lib.last_error()
    assert L.sr_jfa_plan(G, K, D, 320, 1 << 30, 0, 256, out, 32) == 32                                  # R = 320 is accepted
    # the loading matrix and the accumulators, through the update (no handle needed)
    sk = C.c_int64(0)
    for args, pat in (((K, D, 0, _dp(A), _dp(Cm), _dp(W)), "R >= 1"), ((K, D, 513, _dp(A), _dp(Cm), _dp(W)), "up to 512 factors"),
                      ((0, D, R, _dp(A), _dp(Cm), _dp(W)), "G, K, D >= 1"), ((K, D, R, None, _dp(Cm), _dp(W)), "null argument"),
                      ((K, D, R, _dp(A), _dp(Cm), _dp(bad(W, 6, np.nan))), "W holds a non-finite value at element 6"),
                      ((K, D, R, _dp(bad(A, 1, np.inf)), _dp(Cm), _dp(W)), "A holds a non-finite value at element 1"),
                      ((K, D, R, _dp(A), _dp(bad(Cm, 0, np.nan)), _dp(W)), "C holds a non-finite value at element 0")):
        assert L.sr_jfa_update(*args, C.byref(sk)) == -1 and re.search(pat, _lib.last_error()) and "HIP" not in _lib.last_error(), _lib.last_error()
    assert L.sr_jfa_factors(None, _dp(W), R, _dp(W), None, None, None) == -1 and "null argument" in _lib.last_error()
    assert L.sr_jfa_train(None, _dp(W), R, 1, None, None) == -1 and "null argument" in _lib.last_error()
    L.sr_jfa_close(None)                                                                                 # harmless
    with pytest.raises(ValueError, match=r"expected N \[G, K\]"):
        jfa.FactorEstimator(N, Fc[:, :3], E)
    with pytest.raises(ValueError, match=r"expected A \[K, R, R\]"):
        jfa.update_loadings(A[:, :1], Cm, W)
    if _lib.device_count() == 0:                       # and a call that needs the device says what is missing: no CPU path
        assert opened() is None and "no HIP device" in _lib.last_error()
        with pytest.raises(_lib.SRError, match="no HIP device"):
            jfa.update_loadings(A, Cm, W)
        assert L.sr_jfa_plan(G, K, D, R, 1 << 30, 0, 0, out, 32) == -1 and "no HIP device" in _lib.last_error()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_jfa_plan_under_asan_ubsan(tmp_path):
    """csrc/jfa_plan.cpp -- every refusal's text and the plan swept over group counts, shapes, ranks, bounds, the jfa_lds_rows
    option and device sizes -- by a stand-alone program (tests/host/jfa_checks.cpp) built with AddressSanitizer + UBSan: host code
    only, no GPU, nothing loaded into Python."""
    exe = str(tmp_path / "jfa_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "host", "jfa_checks.cpp"), os.path.join(CSRC, "jfa_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "jfa checks ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_jfa_kernels_do_not_spill(built_lib):
    import test_abi_cpu
    res = test_abi_cpu._kernel_resources("jfa")
    names = " ".join(res)
    for kernel in ("jfa_scale_kernel", "jfa_gram_kernel", "jfa_factor_kernel"):
        assert kernel in names
    assert len(res) == 3
    for name, r in res.items():
        assert r["scratch"] == 0, (name, r)


def test_dense64_gemm_kernel_does_not_spill(built_lib):
    """the float64 GEMM every JFA, PLDA, eigen back end and score normalisation product goes through: present, alone in its file, no scratch"""
    import test_abi_cpu
    res = test_abi_cpu._kernel_resources("dense64")
    assert "dense_gemm_kernel" in " ".join(res)
    assert len(res) == 1
    for name, r in res.items():
        assert r["scratch"] == 0, (name, r)


def test_present_surface_does_not_reach_the_new_entry_points(built_lib, monkeypatch):
    """The package import, jfa's present entry points and every other module leave sr_jfa_* alone: they are reached from
    jfa.FactorEstimator, jfa.update_loadings and _lib.jfa_plan only."""
    from speaker_recognition_amd import _lib, jfa
    pkg = os.path.join(ROOT, "speaker-recognition_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py") and f not in ("jfa.py", "_lib.py"):
                text = open(os.path.join(dirpath, f)).read()
                assert "sr_jfa" not in text and "FactorEstimator" not in text and "jfa_plan" not in text, f
    called = []

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name.startswith("sr_jfa"):
                called.append(name)
            return getattr(self._lib, name)

    real = _lib.lib()
    monkeypatch.setattr(_lib, "_lib", Spy(real))
    ubm = (np.array([0.5, 0.5]), np.array([[0.0, 10.0], [4.0, -2.0]]), np.ones((2, 2)))
    jfa.map_supervectors(np.array([[16.0, 0.0]]), np.array([[32.0, 0.0, 0.0, 0.0]]), ubm)
    if _lib.device_count() == 0:
        with pytest.raises(_lib.SRError, match="no HIP device"):
            jfa.compute_suf_stats([np.zeros((5, 2))], ubm)
        with pytest.raises(_lib.SRError, match="no HIP device"):
            jfa.collect_suf_stats(np.zeros((2, 5)), ubm[1].T, ubm[2].T, ubm[0])
    else:
        jfa.compute_suf_stats([np.zeros((5, 2))], ubm)
        jfa.collect_suf_stats(np.zeros((2, 5)), ubm[1].T, ubm[2].T, ubm[0])
    assert called == []
    _lib.jfa_plan(3, 2, 2, 2)
    assert called == ["sr_jfa_plan"]                   # (the spy sees what it should)


def test_refused_in_a_process_forked_after_runtime_use(built_lib):
    """As the bw and top-C calls: in a child forked after its parent touched the GPU runtime, the calls that need the device say
    so and name the remedy; the argument refusals and the plan still work there."""
    import test_fork
    from speaker_recognition_amd import _lib
    L = built_lib
    L.sr_device_count()                                # (this call is what initialises the runtime in the parent)
    G, K, D, R = 3, 2, 2, 2
    N, Fc, E, W = np.ones((G, K)), np.zeros((G, K * D)), np.ones(K * D), np.ones((R, K * D))
    A, Cm = np.stack([np.eye(R)] * K), np.ones((R, K * D))

    def child():
        out = {"lost": L.sr_gpu_runtime_lost()}
        out["open"] = L.sr_jfa_open(G, K, D, _dp(N), _dp(Fc), _dp(E))
        out["open_error"] = _lib.last_error()
        out["update"] = L.sr_jfa_update(K, D, R, _dp(A), _dp(Cm), _dp(W), None)
        out["update_error"] = _lib.last_error()
        out["refusal"] = L.sr_jfa_open(0, K, D, _dp(N), _dp(Fc), _dp(E))
        out["refusal_error"] = _lib.last_error()
        out["plan"] = _lib.jfa_plan(G, K, D, R)["n_chunks"]
        return out

    out = test_fork._in_forked_child(child)
    assert out["lost"] == 1 and out["open"] is None and out["update"] == -1 and out["refusal"] is None and out["plan"] == 1
    assert "forked after its parent" in out["open_error"] and "sr_jfa_open" in out["open_error"]
    assert "forked after its parent" in out["update_error"] and "sr_jfa_update" in out["update_error"]
    assert "G, K, D >= 1" in out["refusal_error"]
    assert L.sr_gpu_runtime_lost() == 0                # the parent is untouched
