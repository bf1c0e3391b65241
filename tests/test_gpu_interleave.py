"""Entry points interleaved in one process on one device.  They share per-device workspaces, the scoring pass's counters and
captured serving graphs that point into them, so one path's answer must not depend on what ran before it.

A delivering scoring pass (small results written straight to host memory) skips the clear of the pass counters when the last
delivering pass left them clear.  A replayed serving graph writes those counters without the library seeing it: the saturation
flag, the partial-product band count and the shared-sigma engine's exception counts.  A stale exception count indexed that
engine's exception lists out of bounds.  Every test here runs with sr_set_option("debug_verify_clean_counters", 1), so that a
library without the fix fails on the host before such a pass is launched.

Operations and their float64 references: tests/interleave_ops.py."""
import numpy as np
import pytest

import interleave_ops as io_

pytestmark = pytest.mark.gpu

MENU = ["score_rogue", "score_diag", "frame_ll", "fused", "tick_graph", "tick_plain", "tick_oor", "score_all", "gmm_score",
        "predict_one", "score_models", "em_small", "em_f64", "em_iter", "em_map", "kmeans", "full_score", "full_fit", "multi", "vad"]
SEEN = {}          # op (EM: (op, engine)) -> its first results in this process
CHECKED = set()    # ops already compared with their reference


@pytest.fixture(scope="module")
def world(built_lib, oracle_built):
    from speaker_recognition_amd import _lib
    _lib.set_option("debug_verify_clean_counters", 1)
    try:
        w = io_.World(oracle_built)
        # every workspace grown to what the ops need and every stream slot captured (graph): later ticks replay
        for _ in range(2):
            for op in MENU:
                if op not in w.streams:
                    _record(w, op, w.run(op))
        for _ in range(2):
            for name, st in w.streams.items():
                for t in range(2):
                    st.submit(w.ticks[t])
                for t in range(2):
                    _same(st.collect()[:2], w.tick_want[(name, t)], name)
        yield w
    finally:
        for k in ("debug_verify_clean_counters", "score_engine", "em_stats_engine"):
            _lib.set_option(k, 0)


@pytest.fixture(autouse=True)
def _hook(built_lib):
    from speaker_recognition_amd import _lib
    _lib.set_option("debug_verify_clean_counters", 1)
    try:
        yield
    finally:
        _lib.set_option("debug_verify_clean_counters", 0)
        _lib.set_option("score_engine", 0)
        _lib.set_option("em_stats_engine", 0)


def _same(got, want, what):
    assert len(got) == len(want), what
    for a, b in zip(got, want):
        assert np.array_equal(np.asarray(a), np.asarray(b)), (what, float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))))


def _record(w, op, res):
    """first occurrence: kept (and checked against the reference); later ones: bit-identical to it -- EM only between fits of
    the same statistics engine, else at tests/test_gpu_em_small.py's tolerances"""
    eng = w.engine(op)
    key = (op, eng) if eng is not None else op
    if op not in CHECKED:
        w.check(op, res)
        CHECKED.add(op)
    if key in SEEN:
        _same(res, SEEN[key], key)
    else:
        SEEN[key] = res
    if eng is not None:
        for k, ref in SEEN.items():
            if isinstance(k, tuple) and k[0] == op and k[1] != eng:
                it, wt, mu, sg = res
                assert np.max(np.abs(wt - ref[1])) < 2e-5 and np.max(np.abs(mu - ref[2])) < 2e-4, (op, eng, k)
                assert np.max(np.abs(sg - ref[3]) / ref[3]) < 1e-3, (op, eng, k)


def _tick(w, name, t):
    st = w.streams[name]
    st.submit(w.ticks[t])
    return st


# ---------------------------------------------------------------------------------------------------------------- targeted


def _warm_then_replay(w, name, ticks_in_flight):
    """two ticks, one per slot (re-captured if something moved a workspace since), then `ticks_in_flight` more that replay
    the captured graphs and are left in flight; returns their tick indices"""
    st = w.streams[name]
    for t in (0, 1):
        st.submit(w.ticks[t])
        _same(st.collect()[:2], w.tick_want[(name, t)], (name, "warm-up", t))
    for t in range(ticks_in_flight):
        st.submit(w.ticks[t & 1])
    return [t & 1 for t in range(ticks_in_flight)]


def _collect(w, name, ticks):
    for t in ticks:
        _same(w.streams[name].collect()[:2], w.tick_want[(name, t)], (name, t))


@pytest.mark.parametrize("call", ["score_rogue", "fused", "predict_one", "score_models", "score_all"])
def test_delivering_call_after_replayed_ticks(world, call):
    """a delivering call -> replayed ticks of the rogue shared-sigma set, collected -> the same call again -> a replayed tick
    that leaves the fp16 range, still in flight -> the same call again.  Every answer bit-identical to the first one, which is
    equal to the float64 oracle (ModelSet.score, MfccExtractor.predict_batch, GMMSet.predict_one's scores,
    sr_score_models_f32, pygmm.GMM.score_all).  The rogue ticks leave exception counts (pass counters 4 ...), the fp16 tick
    the saturation flag (counter 0).  A one-model set, as score_all scores, has no exception counters.  Against a library
    without the fix the other four variants fail with the hook's error; the score_all variant still passes there, because
    these sequences do not leave a replayed tick's counters in place in front of its pass.  For score_all this is a check of
    answers only."""
    w = world
    first = w.run(call)
    w.check(call, first)
    _collect(w, "tick_graph", _warm_then_replay(w, "tick_graph", 2))
    _same(w.run(call), first, (call, "after the rogue ticks"))
    # a fresh stream of the fp16-range set: both slots captured, then the call between submit and collect of replayed ticks
    from speaker_recognition_amd.core import Batch
    ex, ms, pcm, st = _oor_stream(io_.FS)
    want = ex.predict_batch(ms, Batch.from_pcm(list(pcm)), nd=0)
    for _ in range(2):
        st.submit(pcm)
        _same(st.collect()[:2], want, "warm-up")
    for r in range(3):
        st.submit(pcm)
        _same(w.run(call), first, (call, "while a tick that leaves the fp16 range is in flight", r))
        _same(st.collect()[:2], want, ("fp16-range tick", r))
    _same(w.run(call), first, (call, "after it"))


def _band_stream(ex_fs, go):
    """a set whose frames land in the partial-product band (test_band_frames_through_fused_pipelined_and_streaming_paths)"""
    from speaker_recognition_amd import synth
    from speaker_recognition_amd.core import Batch, MfccExtractor, ModelSet, ServingStream
    from speaker_recognition_amd.pygmm import GMM
    ex = MfccExtractor(ex_fs)
    n_win, win = 4, 2 * ex_fs
    pcm = np.stack([synth.synth_speech(3 + u, 2.0, ex_fs)[:win] for u in range(n_win)])
    feats = ex.extract_batch(Batch.from_pcm(list(pcm)), nd=0)
    X = feats.download().astype(np.float64)
    D, K = X.shape[1], 32
    rng = np.random.default_rng(2)
    models = []
    for s in range(3):
        mean = np.zeros((K, D))
        mean[:, s] = 1.84 + 0.01 * rng.standard_normal(K)
        sigma = np.full((K, D), 3.0)
        sigma[:, s] = 0.05
        models.append((np.full(K, 1.0 / K), io_.r6(mean), sigma))
    want_ll = np.stack([go.score_batch(go.GMMParams(*m), X, go.MODE_FASTEXP) for m in models])
    assert ((want_ll < -600.0) & (want_ll > -709.0)).sum() > 20
    ms = ModelSet([GMM.from_arrays(*m) for m in models])
    return ex, ms, pcm, ServingStream(ex, ms, n_win, win, nd=0, graph=True)


def _oor_stream(ex_fs):
    """a set whose every tick leaves the fp16 range and is scored again at collect (interleave_ops.oor_models)"""
    from speaker_recognition_amd import _lib, synth
    from speaker_recognition_amd.core import Batch, MfccExtractor, ModelSet, ServingStream
    from speaker_recognition_amd.pygmm import GMM
    ex = MfccExtractor(ex_fs)
    ms = ModelSet([GMM.from_arrays(*m) for m in io_.oor_models()])
    audio = synth.synth_speech(6, 3.0, ex_fs)
    pcm = np.stack([audio[j * 4000:j * 4000 + ex_fs] for j in range(3)])
    ex.predict_batch(ms, Batch.from_pcm(list(pcm)), nd=0)
    assert "bf16x3" in _lib.last_score_kernel(), _lib.last_score_kernel()      # the re-run: the fp16 pass saturated
    return ex, ms, pcm, ServingStream(ex, ms, 3, ex_fs, nd=0, graph=True)


def test_delivering_call_between_submit_and_collect(world, oracle_built):
    """ModelSet.score on the rogue set while replayed ticks are in flight and not yet collected: the rogue set's tick (exception
    counts), then one with frames in the partial-product band (band count), then one that leaves the fp16 range (saturation
    flag) -- the answer stays bit-identical and equal to the oracle; every tick equals the synchronous fused step."""
    from speaker_recognition_amd.core import Batch
    w = world
    first = w.run("score_rogue")
    w.check("score_rogue", first)
    for make in (lambda: _band_stream(io_.FS, oracle_built), lambda: _oor_stream(io_.FS)):
        ex, ms, pcm, st = make()
        want = ex.predict_batch(ms, Batch.from_pcm(list(pcm)), nd=0)
        for _ in range(2):                       # both slots captured: the ticks below replay
            st.submit(pcm)
            _same(st.collect()[:2], want, "warm-up")
        for rep in range(3):
            _tick(w, "tick_graph", rep & 1)
            st.submit(pcm)
            _same(w.run("score_rogue"), first, ("between submit and collect", rep))
            _same(w.streams["tick_graph"].collect()[:2], w.tick_want[("tick_graph", rep & 1)], ("rogue tick", rep))
            _same(st.collect()[:2], want, ("other tick", rep))
            _same(w.run("score_rogue"), first, ("after collect", rep))
        del st


# ---------------------------------------------------------------------------------------------------------------- the program


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_interleaved_program(world, seed):
    """A seeded ordering of the whole menu, every op at least three times.  A serving tick is submitted as one step and collected
    at the end of a step one to three steps later, so at least one other op runs while it is in flight; whenever the rogue
    set's graph stream has nothing in flight after a step, a tick of it is submitted there, so every step after the first runs
    with a tick pending.  Every result is bit-identical to the op's first one in this process; each op is checked once
    against its float64 reference."""
    w = world
    rng = np.random.default_rng(seed)
    prog = [op for op in MENU for _ in range(3)] + [str(op) for op in rng.choice(MENU, 8)]
    rng.shuffle(prog)
    pending = {name: [] for name in w.streams}         # (step due, tick index), oldest first
    n_sub = {name: 0 for name in w.streams}
    log = []
    ops_with_tick = ops_total = 0

    def collect(name):
        _, t = pending[name].pop(0)
        log.append("collect %s[%d]" % (name, t))
        _same(w.streams[name].collect()[:2], w.tick_want[(name, t)], (name, t))

    def submit(name, i):
        if len(pending[name]) == 2:                    # (two ticks in flight per stream at most)
            collect(name)
        t = n_sub[name] % 2
        n_sub[name] += 1
        log.append("submit %s[%d]" % (name, t))
        w.streams[name].submit(w.ticks[t])
        pending[name].append((i + int(rng.integers(1, 4)), t))

    for i, op in enumerate(prog):
        try:
            if op in w.streams:
                submit(op, i)
            else:
                ops_total += 1
                ops_with_tick += any(pending.values())
                log.append(op)
                _record(w, op, w.run(op))
            for name, q in pending.items():            # (end of the step: what is due leaves)
                while q and q[0][0] <= i:
                    collect(name)
            if not pending["tick_graph"]:
                submit("tick_graph", i)
        except Exception as e:
            pytest.fail("seed %d, step %d (%s): %s: %s\nsteps so far: %s" % (seed, i, op, type(e).__name__, e, ", ".join(log)))
    try:
        for name in pending:
            while pending[name]:
                collect(name)
    except Exception as e:
        pytest.fail("seed %d, final collects: %s: %s\nsteps: %s" % (seed, type(e).__name__, e, ", ".join(log)))
    assert CHECKED >= set(MENU) - set(w.streams)
    assert ops_with_tick >= ops_total - 1, (ops_with_tick, ops_total)       # (all but possibly the first step)
