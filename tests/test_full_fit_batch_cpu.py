"""Batched full-covariance fits without a GPU (sr_fullgmm_fit_batch, skgmm.fit_many; csrc/gmm_full_fit.hip): the symbol and its
binding, every argument check (all made before the device is touched, so they answer here), the loud failure without a device,
the host-side checks of skgmm.fit_many, and the batched kernels' scratch."""
import ctypes as C
import re

import numpy as np
import pytest

K, D = 4, 3


def _handles(lib, shapes):
    hs = [lib.sr_fullgmm_create(k, d, None, None, None) for k, d in shapes]
    assert all(hs)
    return [C.c_void_p(h) for h in hs]


def _call(lib, handles, ns, X=None, D=D, params=None, offsets=None, S=None):
    """sr_fullgmm_fit_batch on `handles` with ns[s] rows per speaker -> (return value, message, status)"""
    from speaker_recognition_amd import _lib
    n_spk = len(handles)
    off = np.zeros(len(ns) + 1, dtype=np.int64)
    off[1:] = np.cumsum(ns)
    if offsets is not None:
        off = np.asarray(offsets, dtype=np.int64)
    if X is None:
        X = np.random.default_rng(0).normal(size=(max(1, int(max(off))), D))
    X = np.ascontiguousarray(X, dtype=np.float64)
    prm = (_lib.FullFitParams * max(1, n_spk))()
    for s in range(n_spk):
        prm[s] = params[s] if params else _lib.FullFitParams(1e-3, 1e-6, 100, 0, 0)
    st = (_lib.FullFitStats * max(1, n_spk))()
    status = np.full(max(1, n_spk), 77, dtype=np.int32)
    arr = (C.c_void_p * max(1, n_spk))(*[h.value for h in handles])
    rc = lib.sr_fullgmm_fit_batch(arr, n_spk if S is None else S, _lib.as_dp(X), _lib.as_i64p(off), D, prm, st, _lib.as_i32p(status))
    return rc, lib.sr_last_error().decode(), status


def test_symbols_exported_and_bound(built_lib):
    from speaker_recognition_amd import _lib
    for name in ("sr_fullgmm_fit_batch", "sr_fullgmm_fit_batch_error", "sr_full_fit_batch_stats", "sr_full_fit_batch_bytes"):
        assert name in _lib.EXT_SYMBOLS
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    fn = _lib.lib().sr_fullgmm_fit_batch
    assert fn.restype is C.c_int
    # SRFullGMM *const *models, int S, const double *X, const int64_t *row_offsets, int D, params *, stats *, int *status
    assert list(fn.argtypes) == [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int,
                                 C.POINTER(_lib.FullFitParams), C.POINTER(_lib.FullFitStats), C.POINTER(C.c_int)]
    assert _lib.lib().sr_fullgmm_fit_batch_error.restype is C.c_char_p


def test_declared_signature_in_the_header():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"\s+", " ", open(os.path.join(root, "include", "pygmm_hip.h")).read())
    assert ("int sr_fullgmm_fit_batch(SRFullGMM *const *models, int S, const double *X, const int64_t *row_offsets, int D, "
            "const struct SRFullFitParams *params, struct SRFullFitStats *out, int *status);") in text
    assert "const char *sr_fullgmm_fit_batch_error(int s);" in text
    assert "void sr_full_fit_batch_stats(long *calls, long *speakers, long *iterations);" in text


def test_counters_take_null_pointers(built_lib):
    from speaker_recognition_amd import _lib
    built_lib.sr_full_fit_batch_stats(None, None, None)
    calls, speakers, iterations = _lib.full_fit_batch_stats()
    assert calls >= 0 and speakers >= calls and iterations >= 0


def test_bad_arguments_fail_before_the_device(built_lib):
    """every case returns -1 with a message naming the problem; none needs a GPU (the checks precede the first device call)"""
    from speaker_recognition_amd import _lib
    before = _lib.full_fit_batch_stats()
    hs = _handles(built_lib, [(K, D)] * 3)
    try:
        rc, msg, _ = _call(built_lib, [], [], S=0)
        assert rc == -1 and "at least one speaker" in msg, msg
        rc, msg, _ = _call(built_lib, hs, [10, 10, 10], offsets=[0, 20, 10, 30])
        assert rc == -1 and "must not decrease" in msg and "speaker 1" in msg, msg
        rc, msg, _ = _call(built_lib, hs, [10, 10, 10], offsets=[5, 15, 25, 35])
        assert rc == -1 and "must start at 0" in msg, msg
        mixed_k = _handles(built_lib, [(K, D), (K + 1, D)])
        rc, msg, _ = _call(built_lib, mixed_k, [10, 10])
        assert rc == -1 and "components" in msg and "speaker 1" in msg, msg
        mixed_d = _handles(built_lib, [(K, D), (K, D + 1)])
        rc, msg, _ = _call(built_lib, mixed_d, [10, 10])
        assert rc == -1 and "dims" in msg and "speaker 1" in msg, msg
        rc, msg, _ = _call(built_lib, [hs[0], hs[1], hs[0]], [10, 10, 10])
        assert rc == -1 and "twice" in msg, msg
        rc, msg, _ = _call(built_lib, hs, [10, K - 1, 10])
        assert rc == -1 and "speaker 1" in msg and "n_samples >= n_components" in msg, msg
        X = np.random.default_rng(1).normal(size=(30, D))
        X[25, 1] = np.nan
        rc, msg, _ = _call(built_lib, hs, [10, 10, 10], X=X)
        assert rc == -1 and "speaker 2" in msg and "NaN" in msg, msg
        prm = [_lib.FullFitParams(1e-3, 1e-6, 100, 0, 0) for _ in range(3)]
        prm[1] = _lib.FullFitParams(1e-3, 1e-6, 0, 0, 0)
        rc, msg, _ = _call(built_lib, hs, [10, 10, 10], params=prm)
        assert rc == -1 and "speaker 1" in msg and "max_iter" in msg, msg
        # the single fit's other checks, per speaker
        for bad, word in ((_lib.FullFitParams(-1.0, 1e-6, 10, 0, 0), "tol"), (_lib.FullFitParams(1e-3, -1.0, 10, 0, 0), "reg_covar"),
                          (_lib.FullFitParams(1e-3, 1e-6, 10, 0, -1), "seed"), (_lib.FullFitParams(1e-3, 1e-6, 10, 1, 0), "init_given")):
            prm = [_lib.FullFitParams(1e-3, 1e-6, 100, 0, 0), _lib.FullFitParams(1e-3, 1e-6, 100, 0, 0), bad]
            rc, msg, _ = _call(built_lib, hs, [10, 10, 10], params=prm)
            assert rc == -1 and "speaker 2" in msg and word in msg, msg
        rc, msg, _ = _call(built_lib, hs, [10, 10, 10], D=D + 1)
        assert rc == -1 and "columns" in msg, msg
        for h in mixed_k + mixed_d:
            built_lib.sr_fullgmm_free(h)
    finally:
        for h in hs:
            built_lib.sr_fullgmm_free(h)
    # none of them counted as a batched call: the counters move only once the arguments have passed
    assert _lib.full_fit_batch_stats() == before


def test_valid_batch_fails_loudly_without_a_gpu(built_lib):
    """No CPU path: the contract of test_abi_cpu.py::test_compute_fails_loudly_without_gpu."""
    from speaker_recognition_amd import _lib, skgmm
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    hs = _handles(built_lib, [(K, D)] * 2)
    try:
        rc, msg, _ = _call(built_lib, hs, [20, 30])
        assert rc == -1 and "no HIP device" in msg, msg
        K_, D_ = C.c_int(0), C.c_int(0)
        assert built_lib.sr_fullgmm_info(hs[0], C.byref(K_), C.byref(D_)) == 0           # still without parameters
    finally:
        for h in hs:
            built_lib.sr_fullgmm_free(h)
    rng = np.random.default_rng(0)
    gm = [skgmm.GMM(2), skgmm.GMM(2)]
    with pytest.raises(_lib.SRError, match="no HIP device"):
        skgmm.fit_many(gm, [rng.normal(size=(50, 3)), rng.normal(size=(40, 3))])
    assert not hasattr(gm[0], "means_") and gm[0]._h is None
    s = skgmm.GMMSet(2)
    with pytest.raises(_lib.SRError, match="no HIP device"):
        s.fit_many([rng.normal(size=(50, 3))], ["a"])


def test_fit_many_checks_its_lists_on_the_host(built_lib):
    from speaker_recognition_amd import skgmm
    rng = np.random.default_rng(0)
    X = rng.normal(size=(50, 3))
    with pytest.raises(ValueError, match="2 models but 1 matrices"):
        skgmm.fit_many([skgmm.GMM(2), skgmm.GMM(2)], [X])
    with pytest.raises(ValueError, match="features"):
        skgmm.fit_many([skgmm.GMM(2), skgmm.GMM(2)], [X, rng.normal(size=(50, 4))])
    with pytest.raises(ValueError, match="components"):
        skgmm.fit_many([skgmm.GMM(2), skgmm.GMM(3)], [X, X])
    with pytest.raises(ValueError, match="n_samples >= n_components"):
        skgmm.fit_many([skgmm.GMM(8), skgmm.GMM(8)], [X, X[:5]])
    with pytest.raises(ValueError, match="64"):
        skgmm.fit_many([skgmm.GMM(2)], [np.zeros((100, 65))])
    with pytest.raises(ValueError, match="2-D"):
        skgmm.fit_many([skgmm.GMM(2)], [np.zeros(10)])
    g = skgmm.GMM(2)
    with pytest.raises(ValueError, match="twice"):
        skgmm.fit_many([g, g], [X, X])
    assert skgmm.fit_many([], []) == []
    with pytest.raises(ValueError, match="1 matrices but 2 labels"):
        skgmm.GMMSet(2).fit_many([X], ["a", "b"])


def test_option_is_checked(built_lib):
    assert built_lib.sr_set_option(b"full_fit_batch_bytes", 0) == -1
    assert b"full_fit_batch_bytes" in built_lib.sr_last_error()
    from speaker_recognition_amd import _lib
    default = _lib.full_fit_batch_bytes()
    assert default == 1 << 30                                                       # (include/pygmm_hip.h)
    try:
        assert built_lib.sr_set_option(b"full_fit_batch_bytes", 12345) == 0 and _lib.full_fit_batch_bytes() == 12345
    finally:
        assert built_lib.sr_set_option(b"full_fit_batch_bytes", default) == 0        # (the default)


# ScratchSize [bytes/lane] of the single-model training kernels (one per device body) in the build of the commit before the
# batched fit (build/gmm_full.resources there): none of them spilled.
PARENT_SCRATCH = {"fe_logprob": 0, "fe_lse": 0, "fe_bound": 0, "fe_means": 0, "fe_cov": 0, "fe_chol": 0, "fe_weights": 0,
                  "fe_derive": 0}


def _kernel_resources(name):
    """{mangled kernel name: {vgpr, scratch}} from the remarks the build keeps next to every object (csrc/Makefile)"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "speaker-recognition_amd", "build", name + ".resources")
    assert os.path.exists(path), "the build did not leave %s" % path
    out, cur = {}, None
    for line in open(path):
        m = re.search(r" Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for key, pat in (("vgpr", r"\bVGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    assert out, "no kernel remarks in %s" % path
    return out


def test_batched_kernels_have_no_scratch_and_no_single_model_kernel_is_left(built_lib):
    res = _kernel_resources("gmm_full_fit")
    for stem, parent in PARENT_SCRATCH.items():
        batch = [n for n in res if stem + "_batch_kernel" in n]
        assert len(batch) == 1, (stem, sorted(res))
        assert res[batch[0]]["scratch"] <= parent, (batch[0], res[batch[0]])
        # the single fit is a group of one in the batched driver: it has no kernels of its own
        assert not [n for n in res if stem + "_kernel" in n], (stem, sorted(res))
    for stem in ("fe_stop_batch_kernel", "fe_onehot_batch_kernel"):
        names = [n for n in res if stem in n]
        assert len(names) == 1 and res[names[0]]["scratch"] == 0, (stem, names)
