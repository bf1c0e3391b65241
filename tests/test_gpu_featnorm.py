"""GPU: short-time feature normalisation (csrc/featnorm.hip: Batch.normalise, feature.norm, MfccExtractor.extract_batch(norm=),
ModelInterface(feature_norm=)) against the numpy restatement of its definitions (tests/featnorm_oracle.py).

The gates.  warp: the doubled mid-ranks equal the oracle's exactly; an output lies within one fp32 ulp of the oracle's -- both are
float64-accurate values (AS241, about 1e-16 relative) rounded once to fp32, so they can differ only where the two float64 values
straddle a rounding boundary.  cmn / cmvn: |got - want| <= 2^-23 max(|want|, 1) -- one fp32 rounding; the float64 error of the
in-order two-pass sums is below 1e-12 for these inputs.  Bits are identical alone, in a batch and under either tile option."""
import functools
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import featnorm_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ("warp", "cmn", "cmvn")
WINDOWS = (2, 3, 8, 301, 1024)
TILES = (0, 64)
DIMS = (1, 13, 39, 65)
F_OF = {0: 256, 64: 64}             # frames per workgroup under each tile option (checked against the plan below)


@pytest.fixture(autouse=True)
def _tile_option():
    from speaker_recognition_amd import _lib
    yield
    _lib.set_option("norm_tile", 0)


def lengths(W):
    """1, 2, W - 1, W, W + 1, W + W // 2 and, for the frames per workgroup F of both tile options, F - 1, F, F + 1, 2 F + W + 3:
    one list for both options, so that their outputs can be compared and the oracle runs once"""
    out = {1, 2, W - 1, W, W + 1, W + W // 2}
    for F in F_OF.values():
        out |= {F - 1, F, F + 1, 2 * F + W + 3}
    return sorted(out - {0})


def contents(T, W, seed, dim=max(DIMS)):
    """gaussian columns with means up to 1e3 and sigma from 0.01 to 5; column 0 carries a tied stretch longer than W (where the
    utterance is) and, like column 1, exact duplicates of values a few frames away"""
    rng = np.random.default_rng(seed)
    mean = rng.uniform(-1e3, 1e3, dim)
    sigma = np.exp(rng.uniform(np.log(0.01), np.log(5.0), dim))
    X = (mean + sigma * rng.standard_normal((T, dim))).astype(np.float32)
    if T == 0:
        return X
    for c in (0, 1):
        for i in rng.integers(0, T, max(1, T // 8)):
            j = min(T - 1, i + int(rng.integers(1, 8)))
            X[j, c] = X[i, c]
    L = min(T, W + 3) if T > W else T // 2
    p = (T - L) // 2
    X[p:p + L, 0] = X[p, 0]
    return X


@functools.lru_cache(maxsize=None)
def reference(W):
    """{T: the utterance X [T, 65], its three outputs, its ranks and its equal-valued windows}: computed once per window for the
    widest matrix and left unchanged; a narrower case takes the leading columns (columns are independent)"""
    ref = {}
    for T in lengths(W):
        X = contents(T, W, 1000 * W + T)
        X.setflags(write=False)
        out, r, _ = fo.warp(X, W)
        cmn, cmvn, flat = fo.sliding_all(X, W)
        for a in (out, r, cmn, cmvn, flat):
            a.setflags(write=False)
        ref[T] = dict(X=X, warp=out, ranks=r, cmn=cmn, cmvn=cmvn, flat=flat)
    return ref


def run(mats, mode, W, ranks=False):
    """-> (list of outputs, counts[, list of ranks]) of ONE device call"""
    from speaker_recognition_amd.core import Batch
    b = Batch.from_features(list(mats))
    res = b.normalise(mode, W, ranks=ranks, counts=True)
    out, counts = res[0], res[-1]
    Y, off = out.download(), out.offsets()
    assert out.n_utt == len(mats) and out.dim == mats[0].shape[1] and np.array_equal(off, b.offsets()) and counts.dtype == np.int64
    cut = lambda A: [A[off[u]:off[u + 1]] for u in range(len(mats))]  # noqa: E731
    return (cut(Y), counts) + ((cut(res[1]),) if ranks else ())


def within_one_ulp(got, want):
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    g, w = got[~nan].astype(np.float64), want[~nan].astype(np.float64)
    return bool(np.all(np.abs(g - w) <= np.spacing(np.maximum(np.abs(got[~nan]), np.abs(want[~nan]))).astype(np.float64)))


def check_against_oracle(mode, got, want, label):
    if mode == "warp":
        diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
        print("%s: warp max |got - want| = %.3g" % (label, np.nanmax(diff) if diff.size else 0.0))
        assert within_one_ulp(got, want), label
    else:
        with np.errstate(invalid="ignore"):
            rel = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.maximum(np.abs(want.astype(np.float64)), 1.0)
            rel[got == want] = 0.0                                  # (an infinity that both sides hold)
        worst = np.nanmax(rel) if rel.size and not np.isnan(rel).all() else 0.0
        print("%s: %s max |got - want| / max(|want|, 1) = %.3g (gate %.3g)" % (label, mode, worst, 2.0 ** -23))
        assert np.array_equal(np.isnan(got), np.isnan(want)), label
        assert np.all(rel[~np.isnan(want)] <= 2.0 ** -23), label


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("W", WINDOWS)
def test_every_window_tile_width_and_length(built_lib, W, tile, dim):
    from speaker_recognition_amd import _lib
    ref = reference(W)
    Ts = lengths(W)
    mats = [np.ascontiguousarray(ref[T]["X"][:, :dim]) for T in Ts]
    other = [t for t in TILES if t != tile][0]
    for mode in MODES:
        _lib.set_option("norm_tile", tile)
        assert _lib.feature_norm_plan(mode, W, dim, max(Ts))["F"] == F_OF[tile]
        if mode == "warp":
            batch, counts, ranks = run(mats, mode, W, ranks=True)
        else:
            batch, counts = run(mats, mode, W)
        for u, T in enumerate(Ts):
            label = "W=%d tile=%d dim=%d T=%d" % (W, tile, dim, T)
            want = ref[T][mode][:, :dim]
            check_against_oracle(mode, batch[u], want, label)
            if mode == "warp":
                assert np.array_equal(ranks[u], ref[T]["ranks"][:, :dim]), label
                assert counts[u] == 0
            elif mode == "cmvn":
                assert counts[u] == int(ref[T]["flat"][:, :dim].sum()), label
                assert np.all(batch[u][ref[T]["flat"][:, :dim]] == 0.0)
            else:
                assert counts[u] == 0
            alone, c1 = run([mats[u]], mode, W)                 # the utterance alone: the same bits, the same count
            assert np.array_equal(bits(alone[0]), bits(batch[u])) and c1[0] == counts[u], label
        _lib.set_option("norm_tile", other)                     # the other tile option: the same bits
        again, c2 = run(mats, mode, W)
        for u in range(len(Ts)):
            assert np.array_equal(bits(again[u]), bits(batch[u])), (W, tile, dim, mode, Ts[u])
        assert np.array_equal(c2, counts)
        _lib.set_option("norm_tile", tile)
        rerun, c3 = run(mats, mode, W)                          # and from run to run
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(rerun, batch)) and np.array_equal(c3, counts)


@pytest.mark.parametrize("tile", TILES)
def test_mixed_batch_of_five(built_lib, tile):
    from speaker_recognition_amd import _lib
    _lib.set_option("norm_tile", tile)
    mats = [contents(T, 301, 77 + T, dim=39) for T in (700, 1, 0, 302, 64)]
    for mode in MODES:
        got, counts = run(mats, mode, 301)
        for u, X in enumerate(mats):
            want, n = fo.normalise(X, mode, 301)
            assert got[u].shape == X.shape
            check_against_oracle(mode, got[u], want, "mixed %s utt %d" % (mode, u))
            assert counts[u] == n, (mode, u)
        assert counts[2] == 0 and got[2].shape == (0, 39)
        if mode != "cmn":
            assert np.all(got[1] == 0.0)                        # one frame: the middle rank, an equal-valued window
        assert counts[1] == (39 if mode == "cmvn" else 0)


@pytest.mark.parametrize("tile", TILES)
def test_nan_and_inf_cells(built_lib, tile):
    from speaker_recognition_amd import _lib
    _lib.set_option("norm_tile", tile)
    W = 8
    clean = contents(200, W, 9, dim=5)
    X = clean.copy()
    X[50, 1] = np.nan
    X[120, 1] = np.inf
    X[121, 3] = -np.inf
    X[10, 3] = np.nan
    X[199, 4] = np.nan
    got, counts, ranks = run([X, clean], "warp", W, ranks=True)
    want, r, n = fo.warp(X, W)
    assert n == 3 and counts[0] == 3 and counts[1] == 0
    assert np.array_equal(ranks[0], r) and ranks[0][50, 1] == ranks[0][10, 3] == ranks[0][199, 4] == -1
    assert np.isnan(got[0][50, 1]) and np.isnan(got[0][10, 3]) and np.isnan(got[0][199, 4]) and np.isnan(got[0]).sum() == 3
    assert ranks[0][120, 1] == 2 * W - 2 and ranks[0][121, 3] == 0          # +-inf rank like any value: the largest, the smallest
    assert within_one_ulp(got[0], want)
    # rows and columns away from the cells are the clean utterance's, to the bit: other columns, and frames whose windows miss them
    ref = got[1]
    far = np.ones(X.shape, bool)
    for t, c in ((50, 1), (120, 1), (121, 3), (10, 3), (199, 4)):
        far[max(0, t - W):t + W + 1, c] = False
    assert np.array_equal(bits(got[0][far]), bits(ref[far]))
    for mode in ("cmn", "cmvn"):
        got, counts = run([X, clean], mode, W)
        want, n = fo.sliding(X, W, mode == "cmvn")
        assert np.array_equal(np.isnan(got[0]), np.isnan(want)) and np.isnan(got[0]).any()      # NaN, and inf - inf, by arithmetic
        check_against_oracle(mode, got[0], want, "nan/inf " + mode)
        assert counts[0] == n and counts[1] == fo.sliding(clean, W, mode == "cmvn")[1]
        assert np.array_equal(bits(got[0][far]), bits(got[1][far]))


def test_refusals(built_lib):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    X = contents(50, 8, 1, dim=4)
    feats = Batch.from_features([X])
    pcm = Batch.from_pcm([np.zeros(4000, np.int16)])
    for batch, kw, pat in ((pcm, {}, "PCM"), (Batch.from_pcm([np.zeros(4000, np.float32)]), {}, "PCM"), (feats, dict(window=1), "window"),
                           (feats, dict(window=1025), "window"), (feats, dict(mode="median"), "mode"), (feats, dict(mode=None), "mode")):
        with pytest.raises(_lib.SRError, match=pat) as e:
            batch.normalise(**kw)
        assert "HIP" not in str(e.value)
    with pytest.raises(_lib.SRError, match="ranks"):
        feats.normalise("cmn", 8, ranks=True)
    for bad in (-1, -64, 65, 2048):
        with pytest.raises(_lib.SRError, match="norm_tile"):
            _lib.set_option("norm_tile", bad)
    # and the device still answers
    got, _ = run([X], "warp", 8)
    assert within_one_ulp(got[0], fo.warp(X, 8)[0])


def _in_forked_child(fn, timeout=60):
    recv, send = mp.Pipe(duplex=False)
    pid = os.fork()
    if pid == 0:
        recv.close()
        try:
            send.send(("ok", fn()))
        except BaseException as e:      # noqa: BLE001 -- everything goes back to the parent
            send.send(("error", repr(e)))
        finally:
            send.close()
            os._exit(0)
    send.close()
    try:
        if not recv.poll(timeout):
            os.kill(pid, 9)
            pytest.fail("the forked child did not answer within %d s" % timeout)
        kind, value = recv.recv()
    except EOFError:
        _, status = os.waitpid(pid, 0)
        pytest.fail("the forked child died without an answer (wait status %d)" % status)
    os.waitpid(pid, 0)
    assert kind == "ok", value
    return value


def test_forked_child_is_refused(built_lib):
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    from speaker_recognition_amd.feature import norm
    X = contents(300, 8, 4, dim=3)
    feats = Batch.from_features([X])
    before, _ = run([X], "warp", 8)                 # the parent has used the device

    def child():
        out = {"lost": _lib.lib().sr_gpu_runtime_lost()}
        try:
            feats.normalise("warp", 8)
            out["normalise"] = "ran"
        except _lib.SRError as e:
            out["normalise"] = str(e)
        h = _lib.lib().sr_feature_norm_batch(feats._h, 1, 8, None, None)
        out["raw"] = "ran" if h else _lib.last_error()
        try:
            norm.normalise_many([X], "cmvn", 8)
            out["many"] = "ran"
        except _lib.SRError as e:
            out["many"] = str(e)
        return out

    out = _in_forked_child(child)
    assert out["lost"] == 1
    for key in ("normalise", "raw", "many"):
        assert "forked after its parent" in out[key] and "spawn" in out[key], (key, out[key])
    assert "sr_feature_norm_batch" in out["normalise"] and "sr_feature_norm_batch" in out["raw"]
    after, _ = run([X], "warp", 8)                  # the parent still gets its answer
    assert np.array_equal(bits(after[0]), bits(before[0])) and _lib.lib().sr_gpu_runtime_lost() == 0


def test_the_stage_in_its_chain(built_lib):
    from speaker_recognition_amd import synth
    from speaker_recognition_amd.core import Batch, MfccExtractor, ModelSet
    from speaker_recognition_amd.feature import norm
    from speaker_recognition_amd.pygmm import GMM
    pcm = [synth.synth_speech(s, 1.5 + 0.5 * s) for s in range(3)]
    ex = MfccExtractor(16000, win_length_ms=25, win_shift_ms=10)
    fused = ex.extract_batch(Batch.from_pcm(pcm), nd=2, cmvn=False, norm="warp")
    raw = ex.extract_batch(Batch.from_pcm(pcm), nd=2, cmvn=False)
    two = raw.normalise("warp")
    assert fused.dim == 39 and np.array_equal(fused.offsets(), raw.offsets())
    Y = fused.download()
    assert np.array_equal(bits(Y), bits(two.download()))
    # resident or uploaded again: the same scores, to the bit
    models = ModelSet([GMM.from_arrays(*synth.synth_gmm(16, 39, 40 + s)) for s in range(4)])
    sums_a, arg_a = models.score(fused)
    sums_b, arg_b = models.score(Batch.from_features(Y, fused.offsets()))
    assert np.array_equal(sums_a, sums_b) and np.array_equal(arg_a, arg_b) and np.isfinite(sums_a).all()
    # host matrices through feature.norm
    R, off = raw.download(), raw.offsets()
    X = R[off[1]:off[2]]
    assert within_one_ulp(norm.feature_warp(X), fo.warp(X, 301)[0])
    assert np.array_equal(bits(norm.feature_warp(X)), bits(Y[off[1]:off[2]]))
    check_against_oracle("warp", norm.feature_warp(X.astype(np.float64), window=100), fo.warp(X, 100)[0], "feature_warp")
    check_against_oracle("cmvn", norm.sliding_cmvn(X, window=100), fo.sliding(X, 100, True)[0], "sliding_cmvn")
    check_against_oracle("cmn", norm.sliding_cmvn(X, window=100, norm_vars=False), fo.sliding(X, 100, False)[0], "sliding_cmn")
    many = norm.normalise_many([R[off[u]:off[u + 1]] for u in range(3)], "warp", 301)
    assert all(np.array_equal(bits(many[u]), bits(Y[off[u]:off[u + 1]])) for u in range(3))


def test_model_interface(built_lib, tmp_path):
    from scipy.io import wavfile
    from speaker_recognition_amd import cli, synth
    from speaker_recognition_amd.feature import mix_feature
    from speaker_recognition_amd.interface import ModelInterface
    fs = 16000
    train = [synth.synth_speech(7 * s, 4.0, fs) for s in range(2)]
    test = [synth.synth_speech(7 * s, 2.0, fs)[2000:] for s in range(2)]
    kw = dict(verbose=False, gmm_order=8, lpc=False, gmm_kwargs=dict(seed=3))
    m = ModelInterface(feature_norm="warp", **kw)
    for s, x in enumerate(train):
        m.enroll("spk%d" % s, fs, x)
        want = fo.warp(np.asarray(mix_feature((fs, x), lpc=False), np.float32), 301)[0]
        got = np.asarray(m.features["spk%d" % s], np.float32)
        assert got.shape == want.shape and within_one_ulp(got, want)
    m.train()
    for s, x in enumerate(test):
        assert m.predict(fs, x) == "spk%d" % s
    assert m.predict_many([(fs, x) for x in test]) == ["spk0", "spk1"]
    assert m.predict_many([(fs, x) for x in test], gpus=0) == ["spk0", "spk1"]        # (the one-GPU path, with the setting)
    f = str(tmp_path / "m.out")
    m.dump(f)
    again = ModelInterface.load(f)
    assert again.feature_norm == "warp" and [again.predict(fs, x) for x in test] == ["spk0", "spk1"]
    # the command line: the model's own setting holds without the flag; the flag reaches the model
    for s, x in enumerate(test):
        wavfile.write(str(tmp_path / ("t%d.wav" % s)), fs, x)
    pattern = str(tmp_path / "t*.wav")
    assert [label for _, label in cli.task_predict(pattern, f)] == ["spk0", "spk1"]
    plain = ModelInterface(**kw)
    plain.gmmset = m.gmmset
    f2 = str(tmp_path / "plain.out")
    plain.dump(f2)
    assert ModelInterface.load(f2).feature_norm is None
    args = cli.get_args(["-t", "predict", "-i", pattern, "-m", f2, "--feature-norm", "warp"])
    assert [label for _, label in cli.task_predict(pattern, f2, feature_norm=cli._feature_norm_setting(args))] == ["spk0", "spk1"]
    seen = []
    orig = ModelInterface._norm_setting
    try:
        ModelInterface._norm_setting = lambda self: seen.append(self.feature_norm) or orig(self)
        cli.task_predict(pattern, f2, feature_norm=dict(mode="cmvn", window=150))
    finally:
        ModelInterface._norm_setting = orig
    assert dict(mode="cmvn", window=150) in seen
