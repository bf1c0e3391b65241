"""The serving stream's voice-activity front end without a GPU: the new entry points are declared, exported and prototyped alike,
refuse bad arguments before they touch a device, the rules the device applies (csrc/ltsd.hip vad_compact_kernel) restated in numpy
agree with filters.ltsd.voiced_runs + ModelInterface.filter, and the new kernel compiles without scratch."""
import ctypes as C
import re

import numpy as np
import pytest

NEW_SYMBOLS = ["sr_stream_create_vad", "sr_stream_collect_vad"]


def test_new_symbols_exported_declared_and_prototyped(built_lib):
    import test_abi_cpu
    from speaker_recognition_amd import _lib
    declared = test_abi_cpu.declared_symbols()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXT_SYMBOLS and hasattr(raw, name), name
    # the header's parameter lists against the ctypes prototypes, type by type
    text = re.sub(r"/\*.*?\*/", "", open(test_abi_cpu.ROOT + "/include/pygmm_hip.h").read(), flags=re.S)
    ctype = {"SRMfcc *": C.c_void_p, "SRModelSet *": C.c_void_p, "SRFullSet *": C.c_void_p, "SRStream *": C.c_void_p, "int": C.c_int,
             "int64_t": C.c_int64, "double": C.c_double, "const float *": C.POINTER(C.c_float), "double *": C.POINTER(C.c_double),
             "int *": C.POINTER(C.c_int)}
    for name in NEW_SYMBOLS:
        m = re.search(r"(\w[\w \*]*?)\b%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        want = []
        for arg in m.group(2).split(","):
            t = re.sub(r"\w+$", "", " ".join(arg.split())).strip()
            want.append(ctype[t])
        fn = getattr(built_lib, name)
        assert list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype == ctype[m.group(1).strip()], name


def test_argument_checks_come_before_the_device(built_lib):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import MfccExtractor
    ex = MfccExtractor(8000)
    na = np.ones(371 // 2 + 1, np.float32)
    fake = C.c_void_p(1)                     # never dereferenced: every case fails before the set is looked at
    ok = dict(m=ex._h, set=fake, full=None, n=6, w=8000, nd=0, flags=0, N=371, order=5, na=_lib.as_fp(na), l0=5.0, l1=10.0)

    def err(**kw):
        a = dict(ok, **kw)
        h = built_lib.sr_stream_create_vad(a["m"], a["set"], a["full"], a["n"], a["w"], a["nd"], a["flags"], a["N"], a["order"], a["na"],
                                           a["l0"], a["l1"])
        assert not h
        return built_lib.sr_last_error()

    assert b"bad arguments" in err(m=None)
    assert b"bad arguments" in err(set=None)                       # neither set
    assert b"bad arguments" in err(full=fake)                      # both
    assert b"bad arguments" in err(na=None)
    assert b"bad arguments" in err(n=0)
    assert b"nd = 0 only" in err(nd=1)
    assert b"SR_STREAM_GRAPH only" in err(set=None, full=fake, flags=_lib.SR_CLAMP_COMPAT)
    assert b"SR_CLAMP_COMPAT and SR_STREAM_GRAPH" in err(flags=0x200)
    assert b"finite" in err(l0=float("nan"))
    assert b"finite" in err(l1=float("inf"))
    assert b"too short for one LTSD analysis window" in err(w=300)
    assert b"order 5 needs more than 10" in err(w=1900)            # 9 analysis windows
    assert b"outside 0..64" in err(order=-1)
    assert built_lib.sr_stream_collect_vad(None, None, None, None, None) == -1
    assert b"null stream" in built_lib.sr_last_error()


def test_serving_stream_vad_argument_is_checked_on_the_host(built_lib):
    from speaker_recognition_amd.core import MfccExtractor, ServingStream
    from speaker_recognition_amd.filters import VAD
    with pytest.raises(TypeError, match="FullSet"):
        ServingStream(MfccExtractor(8000), [1, 2], 6, 8000, vad=VAD())


def device_rule(ltsd, lam0, lam1, W, half, frame_len, frame_shift):
    """vad_compact_kernel's marks in numpy: (destination half-hop of every half-hop or -1, L, T); float32 values against float64
    thresholds"""
    v = np.asarray(ltsd, np.float32).astype(np.float64)
    above, strong = v > lam0, v > lam1
    dst, n, i = np.full(len(v), -1), 0, 0
    while i < len(v):
        if not above[i]:
            i += 1
            continue
        j = i
        while j < len(v) and above[j]:
            j += 1
        if strong[i:j].any():
            dst[i:j] = np.arange(n, n + (j - i))
            n += j - i
        i = j
    L = n * half
    T = (L - frame_len) // frame_shift + 1 if 3 * L > W and L > 5 * frame_len else 0
    return dst, L, T


def test_rules_restated_agree_with_voiced_runs_and_the_one_third_rule(built_lib):
    from speaker_recognition_amd.core import MfccExtractor, vad_thresholds
    from speaker_recognition_amd.filters.ltsd import voiced_runs
    ex = MfccExtractor(8000)
    W, half, wn = 8000, 185, 42
    rng = np.random.default_rng(21)
    lam0 = float(np.float32(7.3) * 1.1)            # a float64 that is no float32
    lam1 = 2.0 * lam0
    d0, d1 = vad_thresholds(lam0, lam1)
    kept = 0
    for case in range(400):
        l = rng.uniform(0.0, 1.4 * lam1, wn).astype(np.float32)
        l[:5] = l[-5:] = 0.0
        if case % 3 == 0:                        # long stretches above lambda0, as speech gives
            l[5:-5] = np.repeat(rng.uniform(0.0, 1.4 * lam1, 8), 4).astype(np.float32)
        # values exactly equal to a threshold as the comparison sees it, and its float32 neighbours
        for t in (d0, d1):
            f = np.float32(t)
            for x in (f, np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(1e9))):
                l[rng.integers(5, wn - 5)] = x
        sig = np.arange(W, dtype=np.int64)
        runs = voiced_runs(l, lam0, lam1)
        want = np.concatenate([sig[s * half:(f + 1) * half] for s, f in runs]) if runs else np.zeros(0, np.int64)
        dst, L, T = device_rule(l, d0, d1, W, half, ex.FRAME_LEN, ex.FRAME_SHIFT)
        got = np.full(L, -1, np.int64)
        for h in np.nonzero(dst >= 0)[0]:
            got[dst[h] * half:(dst[h] + 1) * half] = sig[h * half:(h + 1) * half]
        assert L == len(want) and np.array_equal(got, want), case
        keep = len(want) > W / 3 and ex.num_frames(len(want)) > 0          # interface.filter, then "Signal too short"
        assert (T > 0) == keep and (not keep or T == ex.num_frames(len(want))), case
        kept += keep
    assert 40 < kept < 360, kept


def test_new_kernels_do_not_spill(built_lib):
    import test_abi_cpu
    res = test_abi_cpu._kernel_resources("ltsd")
    names = [n for n in res if "vad_compact_kernel" in n]
    assert len(names) == 1, sorted(res)
    assert res[names[0]]["scratch"] == 0, res[names[0]]
    for obj, kern in (("mfcc", "cmvn_delta_kernel"), ("gmm_full", "fullcov_finalize_kernel"), ("ltsd", "ltsd_reduce_kernel")):
        r = test_abi_cpu._kernel_resources(obj)
        for n in [n for n in r if kern in n]:
            assert r[n]["scratch"] == 0, (n, r[n])
