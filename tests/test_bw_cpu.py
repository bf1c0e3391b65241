"""CPU side of the batched Baum-Welch statistics (csrc/bw_stats.hip, csrc/bw_plan.cpp, jfa.py): the float64 restatement
(tests/bw_cases.py) against plain loops and against the reference's linear-domain formula, the relevance-MAP supervector, the
plan (sr_bw_plan -- also under the host sanitizers, tests/host/bw_checks.cpp), the symbols, the refusals that must not need a
device, the kernels' resource records, and the Python surface's defaults."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bw_cases as bc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")
NEW = ["sr_bw_stats_batch", "sr_bw_plan"]


def test_restatement_agrees_with_plain_loops_and_drops_frames():
    ubm = bc.make_ubm(5, 3, 1)
    X = bc.draw(ubm, 9, 2)
    clean = np.delete(X, (3, 5), axis=0)
    X[3, 1] = np.nan
    X[5] = 1e30
    for x in (X, clean, X[:0]):
        N, F, ll, dropped, llt = bc.stats(x, ubm)
        Nl, Fl, lll, dl = bc.stats_loops(x, ubm)
        assert dropped == dl and np.allclose(N, Nl, rtol=0, atol=1e-12) and np.allclose(F, Fl, rtol=0, atol=1e-12) and abs(ll - lll) < 1e-10
    N, F, ll, dropped, llt = bc.stats(X, ubm)
    Nc, Fc, llc, dc, _ = bc.stats(clean, ubm)
    # the two rows contribute nothing: the statistics are those of the utterance without them, and every other frame counts once
    assert dropped == 2 and dc == 0 and np.isnan(llt[[3, 5]]).all() and np.isfinite(np.delete(llt, (3, 5))).all()
    assert np.array_equal(N, Nc) and np.array_equal(F, Fc) and ll == llc and abs(N.sum() - 7.0) < 1e-12
    # a frame far from every mixture has a finite total in the log domain and contributes normally (the linear form has 0 / 0 there)
    far = np.full((1, 3), 300.0)
    N, F, ll, dropped, _ = bc.stats(far, ubm)
    assert dropped == 0 and abs(N.sum() - 1.0) < 1e-12 and np.isfinite(ll) and ll < -1e4
    with np.errstate(all="ignore"):
        assert np.isnan(bc.stats_linear(far.T, ubm[1].T, ubm[2].T, ubm[0])[0]).all()
    # an empty utterance gives zeros
    N, F, ll, dropped, _ = bc.stats(np.zeros((0, 3)), ubm)
    assert not N.any() and not F.any() and ll == 0.0 and dropped == 0 and F.shape == (15,)


def test_restatement_equals_the_reference_formula_on_the_fixture_ubm():
    """gaussian_posteriors.m / collect_suf_stats.m restated in numpy, in their own orientation and in the linear domain, on the
    reference's own UBM tables: the log-domain restatement agrees to 1e-10, and the reference's arithmetic is well defined on
    these inputs (its smallest per-frame sum is far above the underflow threshold)."""
    ubm = bc.fixture_ubm()
    w, mu, var = ubm
    assert mu.shape == var.shape == (256, 13) and w.shape == (256,) and abs(w.sum() - 1) < 1e-9 and (var > 0).all()
    for T, seed in ((37, 11), (300, 12), (3000, 13)):
        X = bc.draw(ubm, T, seed)
        N, F, ll, dropped, llt = bc.stats(X, ubm)
        Nr, Fr, tot = bc.stats_linear(X.T, mu.T, var.T, w.reshape(-1, 1))
        assert dropped == 0 and tot.min() > 1e-200
        assert np.max(np.abs(N - Nr)) <= 1e-10 and np.max(np.abs(F - Fr)) <= 1e-10
        assert np.max(np.abs(llt - np.log(tot))) <= 1e-10
        assert abs(N.sum() - T) < 1e-9
    # F is mixture-major, D values per mixture: the reference's reshape of the dim x gaussians matrix
    X = bc.draw(ubm, 5, 14)
    N, F, *_ = bc.stats(X, ubm)
    t = bc.log_terms(X, ubm)
    gam = np.exp(t - np.log(np.exp(t).sum(axis=1))[:, None])
    assert np.allclose(F.reshape(256, 13)[7], gam[:, 7] @ X, rtol=0, atol=1e-12)


def test_map_supervectors_hand_case_and_collect_orientation(monkeypatch):
    from speaker_recognition_amd import jfa
    mu = np.array([[0.0, 10.0], [4.0, -2.0]])
    ubm = (np.array([0.5, 0.5]), mu, np.ones((2, 2)))
    N = np.array([[16.0, 0.0], [48.0, 8.0]])
    F = np.array([[32.0, 0.0, 0.0, 0.0], [48.0, 96.0, 8.0, 16.0]])
    sv = jfa.map_supervectors(N, F, ubm)
    # session 0: alpha = (1/2, 0): mixture 0 half way from mu to E = (2, 0); mixture 1 stays.  session 1: alpha = (3/4, 1/3)
    assert np.allclose(sv, [[1.0, 5.0, 4.0, -2.0], [0.75 * 1 + 0.25 * 0, 0.75 * 2 + 0.25 * 10, (1 + 2 * 4) / 3, (2 - 2 * 2) / 3]], rtol=0, atol=1e-14)
    assert np.allclose(jfa.map_supervectors(N, F, ubm, relevance=1e-9)[1], [1.0, 2.0, 1.0, 2.0], atol=1e-8)
    assert np.allclose(jfa.map_supervectors(N[0], F[0], {"weights": ubm[0], "means": mu, "variances": ubm[2]}), sv[:1])
    with pytest.raises(ValueError, match="expected N"):
        jfa.map_supervectors(N, F[:, :3], ubm)
    with pytest.raises(ValueError, match="relevance"):
        jfa.map_supervectors(N, F, ubm, relevance=0.0)
    # collect_suf_stats: MATLAB orientation in, supervector order out -- the device call replaced by the restatement
    seen = {}

    def fake(sessions, u):
        seen["shape"] = sessions[0].shape
        w, m, v = (np.asarray(a) for a in u)
        seen["ubm"] = (w.shape, m.shape, v.shape)
        r = bc.batch_stats(sessions, (w, m, v))
        return r[0], r[1]

    monkeypatch.setattr(jfa, "compute_suf_stats", fake)
    u3 = bc.make_ubm(4, 3, 5)
    X = bc.draw(u3, 11, 6)
    Nc, Fc = jfa.collect_suf_stats(X.T, u3[1].T, u3[2].T, u3[0].reshape(-1, 1))
    Nr, Fr, _ = bc.stats_linear(X.T, u3[1].T, u3[2].T, u3[0])
    assert seen["shape"] == (11, 3) and seen["ubm"] == ((4,), (4, 3), (4, 3))
    assert Nc.shape == (4,) and Fc.shape == (12,) and np.allclose(Nc, Nr, atol=1e-12) and np.allclose(Fc, Fr, atol=1e-12)
    with pytest.raises(ValueError, match="expected data"):
        jfa.collect_suf_stats(X, u3[1].T, u3[2].T, u3[0])


def test_symbols_exported_and_declared(built_lib):
    from speaker_recognition_amd import _lib
    header = open(os.path.join(ROOT, "include", "pygmm_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), "lib/pygmm.so does not export %s" % name
        assert re.search(r"\bint %s\(" % name, header), "%s is not declared in include/pygmm_hip.h" % name
        assert name in _lib.EXT_SYMBOLS
    for text in ("bw_scratch_mib", "bw_range_frames", "SR_T_BW_LSE 10", "SR_T_BW_STATS 11", "SR_T_BW_REDUCE 12", "log domain"):
        assert text in header
    assert (_lib.T_BW_LSE, _lib.T_BW_STATS, _lib.T_BW_REDUCE) == (10, 11, 12)
    for name in ("sr_score_batch_set", "sr_score_batch_set_topc", "sr_train_f32"):
        assert hasattr(raw, name)                      # the siblings stay


def _cut(p, lengths, u):
    off = int(np.sum(lengths[:u]))
    r = p["ranges"]
    return [(int(a[1]) - off, int(a[2])) for a in r if a[0] == u]


def test_plan_ranges_cover_every_frame_and_groups_respect_the_bound(built_lib):
    from speaker_recognition_amd import _lib
    R = 128
    ragged = np.array([0, 1, 3, 63, 64, 65, R - 1, R, R + 1, 2 * R + 3], dtype=np.int64)
    for K, D in ((1, 1), (17, 13), (64, 39), (65, 40), (256, 13), (512, 39)):
        dp = next(d for d in (8, 13, 16, 24, 26, 32, 34, 39, 40) if d >= D)
        slab = -(-K // 64) * 64 * (-(-(dp + 1) // 16) * 16) * 8
        for lengths in (ragged, ragged[::-1].copy(), np.array([300] * 5), np.array([], dtype=np.int64), np.array([0, 0])):
            for rf in (0, R, 1000):
                for bound in (slab, 1 << 20, 1 << 30):
                    if bound < slab:
                        continue
                    p = _lib.bw_plan(K, D, lengths, rf, bound, 256)
                    assert p["dp"] == dp and p["slab_bytes"] == slab and p["n_mix_blocks"] == -(-K // 64) and p["ncb"] * 16 >= dp + 1
                    rows = p["ranges"]
                    off = np.concatenate([[0], np.cumsum(lengths)])
                    covered = np.zeros(int(off[-1]), dtype=np.int32)
                    for u, first, n in rows:
                        assert n >= 1 and off[u] <= first and first + n <= off[u + 1]            # never across an utterance
                        covered[first:first + n] += 1
                    assert (covered == 1).all()                                                  # every frame exactly once
                    assert [tuple(r) for r in rows] == sorted(tuple(r) for r in rows)            # in batch order
                    want = rf if rf else 1024
                    assert all(n == want or first + n == off[u + 1] for u, first, n in rows)
                    assert 1 <= p["group_ranges"] and p["group_ranges"] * slab <= bound          # the bound holds
                    assert p["n_groups"] == -(-len(rows) // p["group_ranges"]) and p["lse_grid"] == -(-int(off[-1]) // 256)
                    assert p["reduce_blocks"] == -(-K * (D + 1) // 256) and p["stats_lds"] <= 80 * 1024
    # an utterance's cut does not change with its neighbours or with the bound
    K, D = 512, 39
    alone = _lib.bw_plan(K, D, [2 * R + 3], R)
    inside = _lib.bw_plan(K, D, ragged, R)
    tight = _lib.bw_plan(K, D, ragged, R, 196608)
    assert _cut(alone, [2 * R + 3], 0) == _cut(inside, ragged, 9) == _cut(tight, ragged, 9) == [(0, R), (R, R), (2 * R, 3)]
    assert tight["group_ranges"] == 1 and tight["n_groups"] == tight["n_ranges"] == inside["n_ranges"] and inside["n_groups"] == 1
    # the automatic cut: 1024 frames, grown in whole tiles of 128 so that one utterance has at most 256 ranges
    assert _lib.bw_plan(K, D, [5000])["n_ranges"] == 5 and _lib.bw_plan(K, D, [262144])["n_ranges"] == 256
    p = _lib.bw_plan(K, D, [1000000])
    assert p["n_ranges"] == -(-1000000 // 3968) <= 256 and p["ranges"][0][2] == 3968 and p["auto_range"] == 1024
    for key, bad in (("bw_scratch_mib", 0), ("bw_scratch_mib", (1 << 20) + 1), ("bw_range_frames", -1), ("bw_range_frames", (1 << 30) + 1)):
        with pytest.raises(_lib.SRError, match=key):
            _lib.set_option(key, bad)
    _lib.set_option("bw_scratch_mib", 1024)
    _lib.set_option("bw_range_frames", 0)


def test_refusals_need_no_device(built_lib):
    """Every refusal fails on its arguments alone, with a text that names the argument -- never the device."""
    from speaker_recognition_amd import _lib
    L = built_lib
    assert L.sr_bw_stats_batch(None, 0, None, None, None, None, None) == -1
    assert "null argument" in _lib.last_error() and "HIP" not in _lib.last_error()
    for kw, pat in ((dict(D=41), r"up to 40 dimensions, the model has 41"), (dict(features=False), "take a feature batch"),
                    (dict(S=3, model=3), r"model index 3 outside \[0, 3\)"), (dict(model=-1), r"model index -1 outside \[0, 1\)"),
                    (dict(feat_dim=39), "feature dim 39 != model dim 13"), (dict(K=0), "no mixtures"), (dict(S=0), "empty model set"),
                    (dict(K=512, D=39, scratch_bytes=196607), "below one range's slab of 196608"),
                    (dict(lengths=[5, -2]), "utterance 1 has a negative length"), (dict(range_frames=-1), "bw_range_frames must be 0")):
        args = dict(K=8, D=13, lengths=[100])
        args.update(kw)
        with pytest.raises(_lib.SRError, match=pat) as e:
            _lib.bw_plan(**args)
        assert "HIP" not in str(e.value)
    out = (C.c_int64 * 12)()
    lengths = (C.c_int64 * 1)(100)
    assert L.sr_bw_plan(1, 0, 8, 13, 1, 13, lengths, 1, 0, 1 << 20, 256, None, 0, out, 11) == -1 and "12 fields" in _lib.last_error()
    assert L.sr_bw_plan(1, 0, 8, 13, 1, 13, lengths, 1, 0, 1 << 20, 256, None, 0, None, 12) == -1 and "null argument" in _lib.last_error()
    if _lib.device_count() == 0:                       # and a call that needs the device says what is missing: no CPU path
        assert L.sr_bw_plan(1, 0, 8, 13, 1, 13, lengths, 1, 0, 1 << 20, 0, None, 0, out, 12) == -1 and "no HIP device" in _lib.last_error()
        from speaker_recognition_amd import synth
        from speaker_recognition_amd.pygmm import GMM
        with pytest.raises(_lib.SRError, match="no HIP device"):
            GMM.from_arrays(*synth.synth_gmm(4, 3, 1)).bw_stats([np.zeros((5, 3))])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_bw_plan_under_asan_ubsan(tmp_path):
    """csrc/bw_plan.cpp -- every refusal's text and the plan swept over shapes, ragged batches, range lengths, bounds and device
    sizes -- by a stand-alone program (tests/host/bw_checks.cpp) built with AddressSanitizer + UBSan: host code only, no GPU,
    nothing loaded into Python."""
    exe = str(tmp_path / "bw_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "host", "bw_checks.cpp"), os.path.join(CSRC, "bw_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "bw checks ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_bw_kernels_do_not_spill(built_lib):
    import test_abi_cpu
    res = test_abi_cpu._kernel_resources("bw_stats")
    names = " ".join(res)
    for kernel in ("bw_lse_kernel", "bw_stats_kernel", "bw_ll_kernel", "bw_reduce_kernel"):
        assert kernel in names
    assert sum("bw_lse_kernel" in n for n in res) == 9 and sum("bw_stats_kernel" in n for n in res) == 9      # padded dims 8 .. 40
    for name, r in res.items():
        assert r["scratch"] == 0, (name, r)


def test_python_defaults_do_not_touch_the_new_entry_points(built_lib, monkeypatch):
    """Nothing of the existing Python surface -- the set classes, the interface, the command line -- calls bw_stats: the new
    entry points are reached from ModelSet.bw_stats, GMM.bw_stats and jfa.py only."""
    from speaker_recognition_amd import core
    pkg = os.path.join(ROOT, "speaker-recognition_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py") and f not in ("core.py", "pygmm.py", "jfa.py", "_lib.py"):
                text = open(os.path.join(dirpath, f)).read()
                assert "bw_stats" not in text and not re.search(r"import jfa|from \.jfa|\bjfa\.\w+\(", text), f      # (the package docstring names the module)
    called = []
    monkeypatch.setattr(core.ModelSet, "bw_stats", lambda *a, **k: called.append(1))
    from speaker_recognition_amd import cli, gmmset
    from speaker_recognition_amd.interface import ModelInterface
    assert not hasattr(cli.get_args(["-t", "predict", "-i", "x", "-m", "y"]), "bw_stats")
    ModelInterface(verbose=False)
    gmmset.GMMSet()
    assert called == []
