"""CPU: the x-vector checker checks itself (tests/xvector_cases.py against torch's conv1d and against explicit loops, in float64;
every mutant outside the gate on the GPU tests' own inputs; the conditions the gates rest on), the plan (sr_xvector_plan,
csrc/xvector_plan.cpp -- also under the host sanitizers, tests/host/xvector_checks.cpp), every refusal with its message before the
device is touched, the file format, the symbols, and the layer kernel's resource record."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import xvector_cases as xc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")
NEW = ["sr_xvector_create", "sr_xvector_free", "sr_xvector_info", "sr_xvector_plan", "sr_xvector_extract_batch", "sr_xvector_extract"]


@pytest.fixture(scope="module")
def xv(built_lib):
    from speaker_recognition_amd import xvector
    return xvector


def _rel(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


# ---- the restatement against independent formulations ----

def test_bf16_rounding_on_the_bits():
    x = np.array([1.0, 1.00390625, 1.01171875, np.nextafter(np.float32(1.00390625), np.float32(2.0)), -1.00390625, 3.0e38, 0.0, -0.0, 1e-30], dtype=np.float32)
    got = xc.bf16_rne(x)
    # 1 + 2^-8 is a tie between 1 and 1 + 2^-7: to even (1); 1 + 3 2^-8 ties to 1 + 2^-6 (even); just above a tie goes up
    assert got[0] == 1.0 and got[1] == 1.0 and got[2] == np.float32(1.015625) and got[3] == np.float32(1.0078125) and got[4] == -1.0
    assert np.all((got.view(np.uint32) & 0xffff) == 0)
    rng = np.random.default_rng(0)
    v = (rng.standard_normal(200000) * 10.0 ** rng.integers(-20, 20, 200000)).astype(np.float32)
    assert np.array_equal(xc.bf16_rne(v), xc.bf16_from64(v.astype(np.float64)))           # the two routes agree on float32 inputs
    assert np.all(np.abs(xc.bf16_trunc(v)) <= np.abs(xc.bf16_rne(v)))
    try:
        import torch
    except Exception:      # noqa: BLE001
        return
    assert np.array_equal(xc.bf16_rne(v), torch.tensor(v).to(torch.bfloat16).float().numpy())


def test_restatement_equals_conv1d_for_uniform_offsets():
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    rng = np.random.default_rng(1)
    for c_in, c_out, offsets in ((30, 48, (-2, -1, 0, 1, 2)), (24, 33, (-3, 0, 3)), (7, 5, (0,)), (9, 4, (0, 4))):
        layer = xc.make_layer(rng, "tdnn", c_in, c_out, offsets, act="relu", affine=True)
        X = xc.bf16_rne(xc.features(rng, 50, c_in)).astype(np.float64)
        a, _ = xc.layer_forward(layer, X)
        m = len(offsets)
        w = xc.bf16_rne(layer["W"]).astype(np.float64).reshape(c_out, m, c_in).transpose(0, 2, 1)
        dil = offsets[1] - offsets[0] if m > 1 else 1
        z = F.conv1d(torch.tensor(X.T[None]), torch.tensor(w.copy()), torch.tensor(layer["b"].astype(np.float64)), dilation=dil)[0].numpy().T
        want = layer["scale"].astype(np.float64) * np.maximum(z, 0.0) + layer["shift"].astype(np.float64)
        assert a.shape == want.shape and _rel(a, want) < 1e-12


def test_restatement_equals_loops_for_irregular_offsets():
    rng = np.random.default_rng(2)
    for c_in, c_out, offsets, act in ((5, 4, (-1, 0, 2), "relu"), (3, 6, (-5,), "none"), (4, 3, (-4, -1, 0, 3, 7), "relu")):
        layer = xc.make_layer(rng, "tdnn", c_in, c_out, offsets, act=act, affine=True)
        X = xc.bf16_rne(xc.features(rng, 30, c_in)).astype(np.float64)
        a, S = xc.layer_forward(layer, X)
        Wq = xc.bf16_rne(layer["W"]).astype(np.float64)
        T_out = 30 - (offsets[-1] - offsets[0])
        want = np.zeros((T_out, c_out))
        mag = np.zeros((T_out, c_out))
        for u in range(T_out):
            for o in range(c_out):
                z = float(layer["b"][o])
                s = abs(z)
                for j, off in enumerate(offsets):
                    for k in range(c_in):
                        z += Wq[o, j * c_in + k] * X[u + off - offsets[0], k]
                        s += abs(Wq[o, j * c_in + k] * X[u + off - offsets[0], k])
                if act == "relu":
                    z = max(z, 0.0)
                want[u, o] = float(layer["scale"][o]) * z + float(layer["shift"][o])
                mag[u, o] = s
        assert _rel(a, want) < 1e-12 and _rel(S, mag) < 1e-12


def test_pooling_restatement_and_its_condition():
    """The pooling of the restatement against numpy's own mean / std, and the ceiling on E2 / var of every pooling input of the GPU
    tests (the gate's amplification: below POOL_AMP_MAX the standard deviation's bound stays under 1e-6 relative)."""
    layer = xc.pool_layer(33, var_floor=1e-4)
    for n in xc.POOL_N:
        for C in xc.POOL_C:
            X = xc.bf16_rne(xc.pool_input(n, C)).astype(np.float64)
            got = xc.pool_forward(dict(layer, channels=C), X)
            want_std = np.sqrt(np.maximum(X.var(axis=0), 1e-4))
            assert np.allclose(got[:C], X.mean(axis=0), rtol=1e-13, atol=1e-15) and np.allclose(got[C:], want_std, rtol=1e-9, atol=1e-12)
            ratio, amp = xc.pool_gate(dict(layer, channels=C), X, xc.rne32_from64(got))
            assert ratio <= 1.0 and amp < xc.POOL_AMP_MAX
            assert got[C] == np.sqrt(1e-4)                                  # channel 0 is constant: the floor is taken
            if n > 1:
                assert amp * n * 2.0 ** -53 < 1e-6


def test_pooling_condition_on_the_networks_test_inputs():
    """The same ceiling on the pooling inputs of the two teacher-forced networks of the GPU tests, evaluated in the restatement (the
    GPU test asserts it again on the device's own activations)."""
    for layers, frames, seed, D in ((xc.standard_network(), xc.STD_TEST_FRAMES, xc.STD_TEST_SEED, 30),
                                    (xc.irregular_network(), xc.IRR_TEST_FRAMES, xc.IRR_TEST_SEED, 24)):
        for f in xc.network_test_features(frames, seed, D):
            pool, x = xc.pooling_input(layers, f)
            ratio, amp = xc.pool_gate(pool, x, xc.rne32_from64(xc.pool_forward(pool, x)))
            assert ratio <= 1.0 and amp < xc.POOL_AMP_MAX and amp * len(x) * 2.0 ** -53 < 1e-6, (len(f), ratio, amp)


# ---- the mutants ----

def test_every_mutant_falls_outside_the_gate(built_lib):
    """On the GPU tests' own inputs: the layer mutants on the irregular single-layer case and on the row-edge layer, the store
    mutant on the same outputs, the pooling mutants on the pooling cases."""
    from speaker_recognition_amd.xvector import XVector
    TN = XVector(xc.irregular_network()).tile_cols
    net, X = xc.mutant_layer_case(TN)
    layer = net[0]
    x = xc.bf16_rne(X).astype(np.float64)
    a, S = xc.layer_forward(layer, x)
    assert xc.layer_gate_f32(layer, a, S, xc.rne32_from64(a)) <= 1.0 and xc.layer_gate_bf16(layer, a, S, xc.bf16_from64(a)) == 0
    for mutant in xc.MUTANTS_LAYER:
        bad, _ = xc.layer_forward(layer, x, mutant=mutant)
        assert xc.layer_gate_f32(layer, a, S, xc.rne32_from64(bad)) > 1.0, mutant
        assert xc.layer_gate_bf16(layer, a, S, xc.bf16_from64(bad)) > 0, mutant
    assert xc.layer_gate_bf16(layer, a, S, xc.bf16_trunc(xc.rne32_from64(a))) > 0, "store_truncated"
    # the same on the standard network's first layer (K = 150 spans three stages: the bias mutant adds it three times)
    std = xc.standard_network()
    x = xc.bf16_rne(xc.features(np.random.default_rng(3), 15, 30)).astype(np.float64)
    a, S = xc.layer_forward(std[0], x)
    for mutant in xc.MUTANTS_LAYER:
        bad, _ = xc.layer_forward(std[0], x, mutant=mutant)
        assert xc.layer_gate_f32(std[0], a, S, xc.rne32_from64(bad)) > 1.0, mutant
    pool = xc.pool_layer(33, var_floor=1e-4)
    x = xc.bf16_rne(xc.pool_input(63, 33)).astype(np.float64)
    for mutant in xc.MUTANTS_POOL:
        bad = xc.pool_forward(pool, x, mutant=mutant)
        ratio, _ = xc.pool_gate(pool, x, xc.rne32_from64(bad))
        assert ratio > 1.0, mutant
    assert set(xc.MUTANTS) == set(xc.MUTANTS_LAYER + xc.MUTANTS_POOL + ("store_truncated",)) and len(xc.MUTANTS) == 8


# ---- symbols, header, resources ----

def test_symbols_header_and_option(built_lib):
    from speaker_recognition_amd import _lib
    header = open(os.path.join(ROOT, "include", "pygmm_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header) and hasattr(raw, name) and name in _lib.EXT_SYMBOLS
    assert "SR_T_COUNT 20" in header and "xvector_scratch_mib" in header          # no timer kind is added
    for bad in (0, (1 << 20) + 1):
        with pytest.raises(_lib.SRError, match="xvector_scratch_mib must be within 1 .. 1048576 .the default is 1024."):
            _lib.set_option("xvector_scratch_mib", bad)
    _lib.set_option("xvector_scratch_mib", 1)
    _lib.set_option("xvector_scratch_mib", 1024)
    with pytest.raises(_lib.SRError, match="debug_xvector_mfma_shape must be 0"):
        _lib.set_option("debug_xvector_mfma_shape", 2)


def test_layer_kernel_has_no_scratch(built_lib):
    path = os.path.join(ROOT, "speaker-recognition_amd", "build", "xvector.resources")
    assert os.path.exists(path), "the build did not leave %s" % path
    kernels, cur = {}, None
    for line in open(path):
        m = re.search(r" Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur is not None:
            cur["scratch"] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and cur is not None:
            cur["lds"] = int(m.group(1))
    layer = {n: r for n, r in kernels.items() if "xv_layer_kernel" in n}
    assert len(layer) == 4                       # two stores x two MFMA shapes
    for n, r in kernels.items():
        if "xv_" in n:
            assert r["scratch"] == 0, n
    for n, r in layer.items():
        assert r["lds"] == 65536, n


# ---- the plan ----

def test_plan_tables_at_the_edge_shapes(xv):
    net = xv.XVector(xc.irregular_network())
    TM, TN = net.tile_rows, net.tile_cols
    ctx = net.context
    assert (TM, TN, ctx, net.embedding_dim, net.pool_index, net.input_dim) == (128, 128, 7, 17, 3, 24)
    rows = xc.row_edge_rows(TM)
    lengths = [r + ctx for r in rows]                      # the LAST frame layer's rows sit at the tile's edges
    p = net.plan(lengths, tiles_of=(2, 0))
    assert list(p["width_pad"]) == [32, 64, 224, 32, 64, 32] and p["granule"] == 32 and p["k_stage"] == 64 and p["lds_bytes"] == 65536
    assert p["n_chunks"] == 1 and p["out_shape"] == (5, 17) and list(p["chunk_begin"]) == [0, 5]
    spans = (3, 4, 0)
    for s in range(4):
        assert list(p["rows"][s]) == [n - sum(spans[:s]) for n in lengths]
    assert list(p["rows"][4]) == [1] * 5 and list(p["rows"][5]) == [1] * 5
    want_tiles = [sum(-(-(n - sum(spans[:l + 1])) // TM) for n in lengths) for l in range(3)]
    assert list(p["tile_counts"][:, 0]) == want_tiles + [0, 1]
    assert [tuple(t) for t in p["tiles"]] == [(0, 0, 1), (1, 0, TM - 1), (2, 0, TM), (3, 0, TM), (3, TM, 1), (4, 0, TM), (4, TM, TM), (4, 2 * TM, 3)]
    for l in range(3):                                      # no tile straddles a segment, every row is covered once
        t = net.plan(lengths, tiles_of=(l, 0))["tiles"]
        for s in range(5):
            mine = t[t[:, 0] == s]
            assert list(mine[:, 1]) == list(range(0, int(p["rows"][l + 1][s]), TM)) and int(mine[:, 2].sum()) == p["rows"][l + 1][s]
            assert np.all(mine[:, 1] + mine[:, 2] <= p["rows"][l + 1][s]) and mine[:, 2].max() <= TM
    # chunking under 1 MiB: whole segments, in order, every chunk within the bound; the rows do not depend on it
    lengths = [300] * 40 + [15, 900]
    q = net.plan(lengths, scratch_bytes=1 << 20)
    assert q["n_chunks"] > 1 and q["chunk_bytes"] <= 1 << 20 and q["chunk_begin"][0] == 0 and q["chunk_begin"][-1] == 42
    assert np.all(np.diff(q["chunk_begin"]) >= 1) and np.array_equal(q["rows"], net.plan(lengths)["rows"])
    assert int(q["tile_counts"][0].sum()) == int(net.plan(lengths)["tile_counts"][0].sum())
    # the standard network: 1500 is no multiple of the tile, the padded widths
    std = xv.XVector(xc.standard_network())
    sp = std.plan([15, 200, 457])
    assert std.context == 14 and list(sp["width_pad"]) == [32, 512, 512, 512, 512, 1504, 3008, 512]
    assert list(sp["rows"][5]) == [1, 186, 443] and list(sp["tile_counts"][:, 0]) == [7, 7, 7, 7, 7, 0, 1]
    # a tapped frame layer returns its rows
    assert net.plan([20, 30], tap=1)["out_shape"] == (20 - 7 + 30 - 7, 200) and net.plan([20, 30], tap=3)["out_shape"] == (2, 62)


def test_plan_under_asan_ubsan(tmp_path):
    """csrc/xvector_plan.cpp swept by a stand-alone program (tests/host/xvector_checks.cpp) built with AddressSanitizer + UBSan: host
    code only, no GPU, nothing loaded into Python."""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "xvector_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "host", "xvector_checks.cpp"), os.path.join(CSRC, "xvector_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "xvector checks ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


# ---- the refusals, each before the device ----

def _net(xv, **over):
    rng = np.random.default_rng(5)
    layers = [xc.make_layer(rng, "tdnn", 6, 8, (-1, 0, 1)), xc.pool_layer(8), xc.make_layer(rng, "affine", 16, 4, act="none", affine=False)]
    return layers


def test_model_refusals(xv):
    from speaker_recognition_amd._lib import SRError
    rng = np.random.default_rng(6)
    t = lambda ci, co, off=(0,), **kw: xc.make_layer(rng, "tdnn", ci, co, off, **kw)      # noqa: E731
    a = lambda ci, co, **kw: xc.make_layer(rng, "affine", ci, co, act=kw.pop("act", "none"), **kw)      # noqa: E731
    cases = [
        ([t(6, 8), a(8, 4)], "0 stats_pool layers; a network holds exactly one"),
        ([t(6, 8), xc.pool_layer(8), xc.pool_layer(16), a(32, 4)], "2 stats_pool layers; a network holds exactly one"),
        ([t(6, 8), xc.pool_layer(8)], "ends at its stats_pool; at least one affine layer follows"),
        ([t(6, 8), xc.pool_layer(8), a(16, 4, act="relu")], "last layer's act must be none: cut the network at the embedding layer"),
        ([t(6, 8, (0, -1)), xc.pool_layer(8), a(16, 4)], "offsets must ascend strictly .-1 follows 0.; sort them"),
        ([t(6, 8, (-17, 0)), xc.pool_layer(8), a(16, 4)], "offset -17; within -16 .. 16"),
        ([t(6, 4097), xc.pool_layer(4097), a(8194, 4)], "4097 output channels; 1 .. 4096"),
        ([t(6, 8), xc.pool_layer(9), a(18, 4)], "layer 1 takes 9 channels, layer 0 gives 8; consecutive layers must agree"),
        ([t(6, 8), xc.pool_layer(8), a(15, 4)], "layer 2 takes 15 channels, layer 1 gives 16; consecutive layers must agree"),
        ([a(6, 8), xc.pool_layer(8), a(16, 4)], "layer 0 is affine in front of the stats_pool; frame layers are tdnn"),
        ([t(6, 8), xc.pool_layer(8), t(16, 4, act="none")], "layer 2 is a tdnn behind the stats_pool; segment layers are affine"),
    ]
    for layers, message in cases:
        with pytest.raises(SRError, match=message):
            xv.XVector(layers)
    bad = _net(xv)
    bad[0]["W"] = bad[0]["W"].copy()
    bad[0]["W"][3, 5] = np.inf
    with pytest.raises(SRError, match="layer 0 holds a non-finite weight at entry 59; clean the checkpoint"):
        xv.XVector(bad)
    bad = _net(xv)
    bad[2]["b"] = bad[2]["b"].copy()
    bad[2]["b"][1] = np.nan
    with pytest.raises(SRError, match="layer 2 holds a non-finite bias, scale or shift at channel 1"):
        xv.XVector(bad)
    with pytest.raises(ValueError, match="layer 0 has 10 offsets; a descriptor row holds at most 9"):
        xv.XVector([t(6, 8, tuple(range(10))), xc.pool_layer(8), a(16, 4)])
    # the library's own refusal of an offset count its descriptor row cannot hold, through the C ABI
    from speaker_recognition_amd import _lib
    good = xv.XVector(_net(xv))
    desc = good._desc.copy()
    desc[0, 5] = 10
    out = np.zeros(16, dtype=np.int64)
    i32p = C.POINTER(C.c_int32)
    assert _lib.lib().sr_xvector_plan(3, desc.ctypes.data_as(i32p), _lib.as_dp(good._floors), None, 0, -1, 0, 0, _lib.as_i64p(out), 16, None, None, None,
                                      None, 0, 0, None, 0) == -1 and "layer 0: 10 offsets; 1 .. 9" in _lib.last_error()
    with pytest.raises(ValueError, match="scale and shift are given together"):
        xv.XVector([dict(_net(xv)[0], shift=None)] + _net(xv)[1:])
    with pytest.raises(ValueError, match="act must be 'relu' or 'none'"):
        xv.XVector([dict(_net(xv)[0], act="tanh")] + _net(xv)[1:])


def test_call_refusals_come_before_the_device(xv):
    """Every refusal of a forward pass names its remedy and is made on the host: none of these messages is the missing GPU's.  (On a
    machine with a GPU the same calls refuse the same way; the last one, a clean call, fails loudly here for want of a device.)"""
    from speaker_recognition_amd import _lib
    net = xv.XVector(_net(xv))
    assert (net.context, net.embedding_dim, net.input_dim) == (2, 4, 6)
    ok = np.zeros((10, 6), np.float32)
    cases = [
        (dict(feats=[ok, np.zeros((2, 6), np.float32)]), "segment 1 holds 2 frames; the network needs 3 .its context of 2 frames . 1.: pass longer segments"),
        (dict(feats=[ok], segments=[(0, 8, 3)]), "segment 0 covers frames 8 .. 11 of utterance 0, which holds 10; keep segments inside their utterance"),
        (dict(feats=[ok], segments=[(1, 0, 3)]), "segment 0 names utterance 1; the batch holds 1"),
        (dict(feats=[ok], segments=[(0, -1, 5)]), "keep segments inside their utterance"),
        (dict(feats=[np.zeros((10, 5), np.float32)]), "the features are 5 wide, the network's first layer takes 6"),
        (dict(feats=[ok], tap=3), None),
    ]
    for kw, message in cases:
        if message is None:
            with pytest.raises(ValueError, match="tap must be None or a layer index 0 .. 2"):
                net.extract(**kw)
            continue
        with pytest.raises(_lib.SRError, match=message) as e:
            net.extract(**kw)
        assert "HIP" not in str(e.value)
    bad = ok.copy()
    bad[7, 2] = np.nan
    with pytest.raises(_lib.SRError, match="non-finite value at row 7, column 2; clean them first"):
        net.extract([bad])
    _lib.set_option("xvector_scratch_mib", 1)
    try:
        with pytest.raises(_lib.SRError, match=r"segment 0 alone takes \d+ bytes of activations, the bound is 1048576; raise the option xvector_scratch_mib"):
            net.extract([np.zeros((200000, 6), np.float32)])
    finally:
        _lib.set_option("xvector_scratch_mib", 1024)
    with pytest.raises(_lib.SRError, match="tdnn or affine layer only"):
        net.extract([ok], tap=1, tap_bf16=True)
    with pytest.raises(ValueError, match="window must be at least the network's context . 1 = 3 frames"):
        net.extract_windows([ok], 2, 1)
    assert [tuple(r) for r in xv.window_table([10, 4, 7], 5, 3)] == [(0, 0, 5), (0, 3, 5), (2, 0, 5)]
    if _lib.device_count() == 0:
        with pytest.raises(_lib.SRError, match="no CPU path|no HIP device|GPU"):
            net.extract([ok])


def _fork_case(L, xv, with_batch):
    """What a process forked after its parent used the GPU runtime gets from the x-vector calls: the two forward passes refuse by
    name, after the argument refusals; creating a network, its info and the plan still work.  `with_batch`: also the resident-batch
    entry point, on a batch the parent made (needs a device)."""
    import test_fork
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    L.sr_device_count()                                # (this call is what initialises the runtime in the parent)
    net = xv.XVector(_net(xv))
    ok = np.zeros((10, 6), np.float32)
    batch = Batch.from_features([ok]) if with_batch else None

    def attempt(fn):
        try:
            fn()
            return "no refusal"
        except _lib.SRError as e:
            return str(e)

    def child():
        out = {"lost": L.sr_gpu_runtime_lost()}
        out["extract"] = attempt(lambda: net.extract([ok]))
        out["short"] = attempt(lambda: net.extract([ok[:2]]))                      # an argument refusal comes first
        out["outside"] = attempt(lambda: net.extract([ok], segments=[(0, 8, 3)]))
        if with_batch:
            out["extract_batch"] = attempt(lambda: net.extract(batch))
            out["batch_outside"] = attempt(lambda: net.extract(batch, segments=[(0, 8, 3)]))
        made = xv.XVector(_net(xv))                                                # create, info and the plan need no device
        out["created"] = (made.context, made.embedding_dim, made.plan([10, 40])["out_shape"])
        out["create_refusal"] = attempt(lambda: xv.XVector(_net(xv)[:2]))
        return out

    out = test_fork._in_forked_child(child)
    assert out["lost"] == 1
    assert "forked after its parent" in out["extract"] and "sr_xvector_extract" in out["extract"] and "sr_xvector_extract_batch" not in out["extract"]
    assert "segment 0 holds 2 frames; the network needs 3" in out["short"] and "forked" not in out["short"]
    assert "keep segments inside their utterance" in out["outside"] and "forked" not in out["outside"]
    if with_batch:
        assert "forked after its parent" in out["extract_batch"] and "sr_xvector_extract_batch" in out["extract_batch"]
        assert "keep segments inside their utterance" in out["batch_outside"] and "forked" not in out["batch_outside"]
    assert out["created"] == (2, 4, (2, 4)) and "at least one affine layer follows" in out["create_refusal"]
    assert L.sr_gpu_runtime_lost() == 0                # the parent is untouched


def test_refused_in_a_process_forked_after_runtime_use(built_lib, xv):
    """The host-rows entry point, with no device; where a device is present also the resident-batch one (and always in
    tests/test_gpu_xvector.py)."""
    _fork_case(built_lib, xv, with_batch=built_lib.sr_device_count() > 0)


# ---- files ----

def test_save_load_round_trips_to_the_bit(xv, tmp_path):
    layers = xc.irregular_network()
    net = xv.XVector(layers)
    path = str(tmp_path / "net.npz")
    net.save(path)
    z = np.load(path)
    assert int(z["n_layers"]) == 5 and str(z["0.kind"]) == "tdnn" and str(z["3.kind"]) == "stats_pool" and "1.scale" not in z.files
    assert list(z["0.offsets"]) == [-1, 0, 2] and z["0.W"].dtype == np.float32 and float(z["3.var_floor"]) == 1e-10
    back = xv.XVector.load(path)
    assert (back.context, back.embedding_dim, back.n_layers) == (net.context, net.embedding_dim, net.n_layers)
    for a, b in zip(net.layers, back.layers):
        assert a.keys() == b.keys()
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
            else:
                assert a[k] == b[k], k
