"""CPU: the C-ABI library builds for gfx950, loads, exports every symbol the header declares,
its host-side logic (text format, MFCC tables, frame counts) matches the oracle, and every
compute entry point fails LOUDLY when no GPU is present (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import mfcc_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "pygmm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"\b([a-z_][a-z0-9_]*)\s*\([^;{]*\)\s*;", text)
    return sorted(set(n for n in names if n not in ("defined",)))


def test_header_symbols_exported(built_lib):
    from speaker_recognition_amd import _lib
    names = declared_symbols()
    assert len(names) >= 45
    for legacy in _lib.LEGACY_SYMBOLS:        # src/gmm/src/pygmm.hh:28-41
        assert legacy in names
    raw = C.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), "lib/pygmm.so does not export %s" % n
    assert set(_lib.LEGACY_SYMBOLS + _lib.EXT_SYMBOLS) == set(names)


def test_parameter_struct_layout():
    from speaker_recognition_amd._lib import Parameter
    assert C.sizeof(Parameter) == 48
    assert Parameter.min_covar.offset == 16 and Parameter.nr_iteration.offset == 32


def test_text_format_host_side(built_lib, oracle_built, gmm_golden, tmp_path):
    from speaker_recognition_amd.pygmm import GMM
    go, g = oracle_built, gmm_golden
    p = go.GMMParams(g["syn16x13_w"], g["syn16x13_mean"], g["syn16x13_sigma"])
    text = go.format_model_text(p)
    f = tmp_path / "m.model"
    f.write_text(text)
    m = GMM.load(str(f))
    assert m.get_dim() == 13 and m.get_nr_mixtures() == 16
    w, mu, sg = m.params()
    assert np.array_equal(w, p.weights) and np.array_equal(mu, p.mean) and np.array_equal(sg, p.sigma)
    assert m.dumps() == text                      # byte-identical to GMM::dump (gmm.cc:655-662)
    out = tmp_path / "o.model"
    m.dump(str(out))
    assert out.read_text() == text
    m2 = GMM.loads(text)
    assert m2.get_nr_mixtures() == 16
    with pytest.raises(Exception):
        GMM.load(str(tmp_path / "missing.model"))
    with pytest.raises(Exception):
        GMM.loads("3\n0.5 0.5\n")                 # truncated


def test_text_numbers_equal_libc(built_lib):
    """The model text is written and read without printf / strtod (csrc/model_text.cpp fast_g6, fast_decimal): every number
    must still come out as `out << v` (= "%g") writes it and go in as `in >> v` reads it -- checked against Python's own
    '%g' and float(), which are libc's, over magnitudes, rounding ties at the 7th digit and odd spellings."""
    from speaker_recognition_amd.pygmm import GMM
    rng = np.random.default_rng(3)
    K, D = 512, 39
    n = K * D
    v = np.concatenate([
        (rng.random(n // 4) - 0.5) * 20,
        10.0 ** ((rng.random(n // 4) - 0.5) * 44) * rng.choice([-1.0, 1.0], n // 4),
        (np.floor(rng.random(n // 4) * 1e6) + 0.5) * 10.0 ** rng.integers(-12, 12, n // 4),      # ties at the 7th digit
        np.round(rng.random(n - 3 * (n // 4)) * 2e6) * 10.0 ** rng.integers(-15, 15, n - 3 * (n // 4)),
    ])
    v[:8] = [0.0, -0.0, 1e-310, 999999.5, 9999995.0, 0.0001, 0.00009999995, 123456.5]
    mean = v.reshape(K, D)
    sigma = np.abs(rng.permutation(v)).reshape(K, D) + 1e-300
    m = GMM.from_arrays(np.full(K, 1.0 / K), mean, sigma)
    tok = m.dumps().split("\n")
    got_mean = " ".join(tok[3 + 3 * k] for k in range(K)).split()
    got_sigma = " ".join(tok[4 + 3 * k] for k in range(K)).split()
    assert got_mean == ["%g" % x for x in mean.ravel()]
    assert got_sigma == ["%g" % x for x in sigma.ravel()]
    # reading: what "%g", "%.15g" and "%.17g" write, plus spellings strtod accepts
    for fmt in ("%g", "%.15g", "%.17g", "%.3e", "%f"):
        vals = np.where(np.abs(v) < 1e30, v, 1.0) if fmt == "%f" else v
        words = [fmt % x for x in vals]
        text = "%d\n%s\n" % (K, " ".join(["%g" % (1.0 / K)] * K))
        for k in range(K):
            text += "%d 1\n%s\n%s\n" % (D, " ".join(words[k * D:(k + 1) * D]), " ".join(["1"] * D))
        _, mu, _ = GMM.loads(text).params()
        want = np.array([float(w) for w in words]).reshape(K, D)
        assert np.array_equal(mu.view(np.int64), want.view(np.int64)), fmt
    odd = ["+1.5", "-.5", "5.", "1e5", "1E-3", "0x10", "1e", "00012.50", "1.7976931348623157e308", "4.9e-324", "nan", "inf", "-inf",
           "123456789012345678", "0.000000000000000000000000000001"]
    for w in odd:
        text = "1\n1\n1 1\n%s\n1\n" % w
        try:
            _, mu, _ = GMM.loads(text).params()
        except Exception:
            assert w in ("0x10", "1e")            # strtod stops inside the word: what follows is no number
            continue
        want = float.fromhex(w) if w.startswith("0x") else float(w)
        assert np.array_equal(np.array([mu[0, 0]]).view(np.int64), np.array([want]).view(np.int64)), w


def _kernel_resources(name):
    """{mangled kernel name: {vgpr, scratch, occupancy}} from the remarks the build keeps next to every object (csrc/Makefile)."""
    import re
    path = os.path.join(ROOT, "speaker-recognition_amd", "build", name + ".resources")
    assert os.path.exists(path), "the build did not leave %s" % path
    out, cur = {}, None
    for line in open(path):
        m = re.search(r" Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for key, pat in (("vgpr", r"\bVGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    assert out, "no kernel remarks in %s" % path
    return out


def test_no_hot_kernel_spills(built_lib):
    """Scratch (register spills) per lane of the kernels on the hot paths, as the compiler reports it for gfx950.  Parity tests
    cannot see a spill; this one caught nothing in time once: the vector engine ran 10x slower for most of a round behind a
    wave-uniform branch in its log-sum-exp (1240 B of scratch per lane at D = 39, F = 4)."""
    import re
    vec = _kernel_resources("gmm_score")
    seen = 0
    for name, r in vec.items():
        m = re.search(r"gmm_score_kernelILi(\d+)ELi(\d+)ELb(\d)", name)
        if not m:
            continue
        seen += 1
        dp, f, pk = (int(v) for v in m.groups())
        assert r["scratch"] <= (64 if (dp, f, pk) == (56, 2, 1) else 0), (dp, f, pk, r)
    assert seen >= 40
    for name, r in _kernel_resources("em").items():
        assert r["scratch"] == 0, (name, r)
    for name, r in _kernel_resources("gmm_score_split").items():
        assert r["scratch"] <= 32, (name, r)
    h2s = _kernel_resources("gmm_score_h2_shared")
    # the shared-sigma engine: NOTHING in scratch in any workgroup shape at any chain length (round 4: the 4-wave shape of the long
    # chains -- configs[2] / [3]'s <8,8,*> carried 364 bytes per lane through round 3, one reload of it inside the image loop --
    # keeps its quadratic-half frame fragments in LDS like the 12-wave shapes)
    n_main = 0
    for name, r in h2s.items():
        if re.search(r"gmm_score_h2s_kernelILi(\d+)ELi(\d+)E", name):
            n_main += 1
            assert r["scratch"] == 0 and r["occupancy"] >= 2, (name, r)
    assert n_main >= 30
    # (the single-wave exception pass: rare by construction; its two longest chains, dims 43..48, keep a bounded spill)
    for name, r in h2s.items():
        m = re.search(r"gmm_score_h2s_online_kernelILi(\d+)ELi(\d+)E", name)
        if m:
            assert r["scratch"] <= (200 if int(m.group(1)) >= 9 else 0), (name, r)
    # the pipelined 12-wave shape (the default for large batches since round 3): NOTHING in scratch -- a spill reload inside its
    # image loop waits with vmcnt(0), i.e. for the LDS-DMA stream in flight (it cost 8 % when two fragments spilled) -- and three
    # waves per SIMD
    piped = {n: r for n, r in h2s.items() if "gmm_score_h2p_kernel" in n}
    assert len(piped) >= 12
    for name, r in piped.items():
        assert r["scratch"] == 0 and r["occupancy"] >= 3, (name, r)
    # the model-split shape of a serving decision with its images straight in registers (round 6): two sets of fragments and nothing
    # in scratch (a reload in the image loop waits for the prefetches in flight), two workgroups per CU
    direct = {n: r for n, r in h2s.items() if "gmm_score_h2m_kernel" in n}
    assert len(direct) >= 12
    for name, r in direct.items():
        assert r["scratch"] == 0 and r["occupancy"] >= 2, (name, r)
    mf = _kernel_resources("mfcc")
    head = [r for n, r in mf.items() if "mfcc_frames_fft2048_kernelIsLi4ELi1ELi12ELi16E" in n]
    assert len(head) == 1 and head[0]["scratch"] == 0 and head[0]["occupancy"] >= 3, head
    # the float64-spectrum kernel (the feature stage's default since round 5): 16 float64 complex points per lane + the butterflies'
    # temporaries fill the 256 registers two waves per SIMD leave each other; the int16 variants must stay out of scratch
    f64 = {n: r for n, r in _kernel_resources("mfcc_f64").items() if "mfcc_frames_fft2048_f64_kernelIs" in n}
    assert len(f64) == 2                          # mel presets 0 and 1: every instance there is
    for name, r in f64.items():
        assert r["scratch"] == 0 and r["occupancy"] >= 2, (name, r)


def test_new_gmm_rejects_non_diagonal(built_lib):
    L = built_lib
    assert not L.new_gmm(4, 2)                    # gmm.cc:211-215 throws; here: NULL + message
    assert b"diagonal" in L.sr_last_error()
    h = L.new_gmm(4, 1)
    assert h and L.get_nr_mixtures(h) == 4 and L.get_dim(h) == 0
    L.sr_free_gmm(h)


def test_mfcc_tables_match_oracle(built_lib):
    from speaker_recognition_amd.core import MfccExtractor
    for fs, kw in ((16000, {}), (8000, {}), (16000, dict(win_length_ms=25, win_shift_ms=10, FFT_SIZE=512, n_filters=40)),
                   (8000, dict(win_length_ms=25, win_shift_ms=10, FFT_SIZE=256, n_filters=24, n_ceps=12))):
        ex = MfccExtractor(fs, **kw)
        ref = mo.get_mfcc_extractor(fs, **kw)
        assert (ex.FRAME_LEN, ex.FRAME_SHIFT) == (ref.FRAME_LEN, ref.FRAME_SHIFT)
        win, M, D = ex.tables()
        assert np.allclose(win, ref.window, rtol=0, atol=1e-15)
        assert np.array_equal(M != 0, ref.M != 0)
        assert np.allclose(M, ref.M, rtol=0, atol=1e-12)
        assert np.allclose(D, ref.D, rtol=0, atol=1e-14)
        for n in (0, 5 * ref.FRAME_LEN, 5 * ref.FRAME_LEN + 1, 16000, 480000):
            want = ref.n_frames(n) if n > 5 * ref.FRAME_LEN else 0
            assert ex.num_frames(n) == want


def test_bad_mfcc_parameters_rejected(built_lib):
    from speaker_recognition_amd._lib import SRError
    from speaker_recognition_amd.core import MfccExtractor
    with pytest.raises(SRError):
        MfccExtractor(16000, FFT_SIZE=1000)
    with pytest.raises(SRError):
        MfccExtractor(16000, win_length_ms=200)   # frame longer than the FFT


def test_verify_clean_counters_option_host_side(built_lib):
    """The test hook of tests/test_gpu_interleave.py is a host-side option: 0 and 1 are taken, anything else is refused with a
    message naming it, and none of it needs a GPU."""
    from speaker_recognition_amd import _lib
    try:
        for v in (1, 0, 1):
            _lib.set_option("debug_verify_clean_counters", v)
        for bad in (-1, 2, 7):
            with pytest.raises(_lib.SRError, match="debug_verify_clean_counters must be 0 or 1"):
                _lib.set_option("debug_verify_clean_counters", bad)
    finally:
        _lib.set_option("debug_verify_clean_counters", 0)


def test_compute_fails_loudly_without_gpu(built_lib, oracle_built, gmm_golden):
    """No silent CPU path: with no HIP device every compute call raises."""
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.pygmm import GMM
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible here")
    g = gmm_golden
    m = GMM.from_arrays(g["syn5x3_w"], g["syn5x3_mean"], g["syn5x3_sigma"])
    with pytest.raises(_lib.SRError, match="no HIP device"):
        m.score(g["syn5x3_X"])
    with pytest.raises(_lib.SRError):
        m.fit(g["syn5x3_X"])
    # legacy symbol: NaN + parked message instead of an exception across the ABI
    X = np.ascontiguousarray(g["syn5x3_X"])
    rows = (C.POINTER(C.c_double) * len(X))(*[C.cast(X[i].ctypes.data, C.POINTER(C.c_double)) for i in range(len(X))])
    v = built_lib.score_all(m.gmm, rows, len(X), X.shape[1], 1)
    assert np.isnan(v) and b"no HIP device" in built_lib.sr_last_error()


def _build_c_example(tmp_path):
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "speaker-recognition_amd", "lib")
    exe = str(tmp_path / "predict_pcm")
    cmd = [shutil.which("gcc") or "gcc", "-std=c99", "-D_DEFAULT_SOURCE", "-Wall", "-Werror", "-I" + os.path.join(root, "include"),
           os.path.join(root, "examples", "predict_pcm.c"), "-o", exe, "-L" + libdir, "-l:pygmm.so",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lm"]
    subprocess.check_call(cmd)
    return exe


def test_header_is_plain_c_and_example_links(built_lib, tmp_path):
    """include/pygmm_hip.h compiles as C99 (no C++ or HIP types at the boundary) and a plain-C host
    (examples/predict_pcm.c) links against lib/pygmm.so; without a GPU it reports so and exits 2."""
    import subprocess
    exe = _build_c_example(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    import ctypes
    if built_lib.sr_device_count() <= 0:
        assert r.returncode == 2 and "no HIP device" in r.stderr


def test_restated_glibc_rand_matches_libc(built_lib):
    """The reference seeds every random draw of its trainer from libc rand() (random.hh:22-25); the HIP runtime
    draws from the process-wide generator while it initialises, so the library carries glibc's algorithm itself
    (csrc/kmeans_init.hip).  Its stream equals rand() of a fresh process."""
    import ctypes as C
    import subprocess
    import sys
    from speaker_recognition_amd import _lib
    n = 5000
    buf = (C.c_int * n)()
    L = _lib.lib()
    L.sr_reference_rand_sample.argtypes = [C.POINTER(C.c_int), C.c_int]
    assert L.sr_reference_rand_sample(buf, n) == 0
    code = "import ctypes as C; l = C.CDLL('libc.so.6'); print(' '.join(str(l.rand()) for _ in range(%d)))" % n
    want = [int(v) for v in subprocess.check_output([sys.executable, "-c", code]).split()]
    assert list(buf) == want
    assert want[0] == 1804289383
