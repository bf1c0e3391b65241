"""The operations of tests/test_gpu_interleave.py: every entry point that owns or shares per-device state (scoring workspaces,
the pass counters, cached batches and sets, captured serving graphs), on small fixed inputs, with the float64 reference each
one is checked against once.  A plain module, not a conftest: the test file imports it."""
import warnings

import numpy as np

FS = 16000
N_WIN = 3                   # windows per serving tick
TOL_H2S = 1e-5              # the split-fp16 shared-sigma engine, per frame (test_h2s_offset_engine_accuracy_and_exceptions)
TOL = 1e-4                  # every other diagonal engine, per frame (tests/test_gpu_gmm.py)


def r6(a):
    """parameters as the text format writes them (%g): the oracle and the device start from the same numbers"""
    return np.vectorize(lambda v: float("%g" % v))(a)


def rogue_models(K=64, D=39, S=13, seed=4242):
    """A UBM, S speakers MAP-adapted from it and one "rogue" speaker with the UBM's sigma and weights but means 3 sigma away:
    its likelihoods sit hundreds of nats from the reference offset, so every pass of the split-fp16 shared-sigma engine notes
    exception tiles for it (as in test_h2s_offset_engine_accuracy_and_exceptions)."""
    from speaker_recognition_amd import synth
    ubm = synth.synth_gmm(K, D, seed)
    w, mu, sg = ubm
    return [ubm] + [synth.synth_map_speaker(ubm, 600 + s) for s in range(S)] + [(w, r6(mu + 3.0 * sg), sg)]


def oor_models():
    """Three models whose split-fp16 image of every MFCC frame saturates in dimension 0 (sigma 2^-7 there, centre 2.5 away from
    the features): every pass of the fp16 engine raises its out-of-range flag, pass counter 0, and the batch is scored again
    on the fp32-grade engines (test_fp16_engine_range_fallback)."""
    from speaker_recognition_amd import synth
    models = []
    for s in range(3):
        w, mu, sg = (a.copy() for a in synth.synth_gmm(32, 13, 900 + s))
        mu[:, 0], sg[:, 0] = 2.5, 2.0 ** -7
        models.append((w, mu, sg))
    return models


def _lib_last_kernel():
    from speaker_recognition_amd import _lib
    return _lib.last_score_kernel()


def is_h2s(name):
    """the split-fp16 shared-sigma engine, in any of its workgroup shapes"""
    return any(k in name for k in ("gmm_score_h2s_kernel", "gmm_score_h2p_kernel", "gmm_score_h2m_kernel"))


def sums_bound(want_ll, off, tol):
    """|sum error| allowed per (utterance, model) when every frame may be off by tol * max(1, |LL|)"""
    a = tol * np.maximum(1.0, np.abs(want_ll))
    return np.stack([a[:, off[u]:off[u + 1]].sum(axis=1) for u in range(len(off) - 1)]) + 1e-9


def oracle_ll(go, models, X, mode=None, clamp_compat=True):
    mode = go.MODE_LOGSUMEXP if mode is None else mode
    return np.stack([go.score_batch(go.GMMParams(*m), X, mode, clamp_compat=clamp_compat) for m in models])


def check_sums(go, models, X, off, sums, arg, tol):
    """device sums and argmax against the float64 oracle's per-frame values summed per utterance"""
    want_ll = oracle_ll(go, models, X)
    want = np.stack([want_ll[:, off[u]:off[u + 1]].sum(axis=1) for u in range(len(off) - 1)])
    bound = sums_bound(want_ll, off, tol)
    assert np.all(np.abs(sums - want) <= bound), float(np.max(np.abs(sums - want) / bound))
    for u in range(len(off) - 1):
        srt = np.sort(want[u])[::-1]
        if len(srt) < 2 or srt[0] - srt[1] > 2 * bound[u].max():
            assert arg[u] == int(np.argmax(want[u])), u
    return want_ll


class World:
    """Everything the program's operations use, built once: the same objects are scored and refitted over and over."""

    def __init__(self, go):
        from speaker_recognition_amd import skgmm, synth
        from speaker_recognition_amd.core import Batch, MfccExtractor, ModelSet, MultiPredictor, ServingStream
        from speaker_recognition_amd.filters import ltsd as L
        from speaker_recognition_amd.gmmset import GMMSet
        from speaker_recognition_amd.pygmm import GMM
        from oracle import ltsd_oracle as lo
        import fullcov_oracle as fo
        self.go = go
        # ---- diagonal scoring, D = 39 (13 MFCC + two deltas): the rogue shared-sigma set and independent models
        self.rogue = rogue_models()
        self.rogue_gmms = [GMM.from_arrays(*m) for m in self.rogue]
        self.ms_rogue = ModelSet(self.rogue_gmms)
        self.diag = [synth.synth_gmm(32, 39, 900 + s) for s in range(5)]
        self.diag_gmms = [GMM.from_arrays(*m) for m in self.diag]
        self.ms_diag = ModelSet(self.diag_gmms)
        self.utts = [synth.draw_frames(self.rogue[1 + u], 120 + 13 * u, 31 + u, outlier_frac=0.01 if u % 2 else 0.0)
                     for u in range(4)]
        self.feats = Batch.from_features(self.utts)
        self.X = np.concatenate(self.utts).astype(np.float64)
        self.X32 = self.X.astype(np.float32)
        self.off = np.concatenate([[0], np.cumsum([len(u) for u in self.utts])])
        self.legacy = self.rogue_gmms[-1]                  # pygmm.GMM.score_all / score: the rogue speaker alone
        # GMMSet.predict_one in a process that owns the GPU: its own packed set and one-utterance batch, kept across calls
        self.gmmset = GMMSet()
        for i, g in enumerate(self.rogue_gmms):
            self.gmmset._append("spk%d" % i, g)
        # ---- from PCM (16 kHz, 32 / 16 ms frames, nd = 2)
        self.ex = MfccExtractor(FS)
        self.pcm = [synth.synth_speech(3 + u, 1.0 + 0.25 * u, FS) for u in range(3)]
        self.pcm_batch = Batch.from_pcm(self.pcm)
        self.ms_oor = ModelSet([GMM.from_arrays(*m) for m in oor_models()])
        audio = synth.synth_speech(4, 12.0, FS)           # (windows on which the rogue speaker lists exception tiles)
        self.ticks = [np.stack([audio[(t * N_WIN + j) * 4000:(t * N_WIN + j) * 4000 + FS] for j in range(N_WIN)])
                      for t in range(2)]
        # what every tick must return: the synchronous fused step on the same windows, bit for bit
        self.tick_want = {}
        # (tick_graph: the rogue set, whose ticks leave exception counts; tick_oor: every tick leaves the saturation flag)
        self.tick_sets = {"tick_graph": (self.ms_rogue, 2, True), "tick_plain": (self.ms_diag, 2, False), "tick_oor": (self.ms_oor, 0, True)}
        for name, (ms, nd, _) in self.tick_sets.items():
            for t, tk in enumerate(self.ticks):
                self.tick_want[(name, t)] = self.ex.predict_batch(ms, Batch.from_pcm(list(tk)), nd=nd)
                if name == "tick_oor":
                    assert "bf16x3" in _lib_last_kernel(), _lib_last_kernel()      # the re-run: the fp16 pass saturated
        self.streams = {name: ServingStream(self.ex, ms, N_WIN, FS, nd=nd, graph=graph)
                        for name, (ms, nd, graph) in self.tick_sets.items()}
        self.multi = MultiPredictor(self.diag_gmms, FS, n_slots=2)
        self.multi_want = self.ex.predict_batch(self.ms_diag, self.pcm_batch, nd=2)
        # ---- diagonal training, 13 dims
        rng = np.random.default_rng(17)
        self.em = {}
        for name, n, K in (("em_small", 1000, 8), ("em_f64", 600, 40), ("em_iter", 1500, 8)):
            cent = 3.0 + rng.normal(0, 2, (K, 13))
            X = (cent[rng.integers(0, K, n)] + rng.normal(0, 0.7, (n, 13))).astype(np.float32)
            start = go.GMMParams(np.full(K, 1.0 / K), r6(cent + 0.2 * rng.standard_normal(cent.shape)), np.full((K, 13), 0.9))
            self.em[name] = (X, start)
        self.em_iters = {"em_small": 4, "em_f64": 2, "em_iter": 1, "em_map": 3}
        X, start = self.em["em_small"]
        self.em["em_map"] = (X[:300], start)
        self.ubm8 = GMM.from_arrays(start.weights, start.mean, start.sigma)
        cent = rng.normal(0, 3, (8, 20))
        self.km_X = (cent[rng.integers(0, 8, 3000)] + rng.normal(0, 1, (3000, 20))).astype(np.float32)
        # ---- full covariance, 13 dims
        self.full = [fo.random_model(rng, 4, 13) for _ in range(3)]
        self.full_gmms = [skgmm.GMM.from_arrays(*m) for m in self.full]
        self.full_set = skgmm.FullSet(self.full_gmms)
        self.full_utts = [fo.draw(rng, self.full[u % 3], 90 + 17 * u).astype(np.float32) for u in range(4)]
        self.full_batch = Batch.from_features(self.full_utts)
        self.full_fit_X = fo.draw(rng, self.full[0], 800)
        w0, mu0, cov0 = fo.random_model(rng, 4, 13)
        prec0 = np.linalg.inv(cov0)
        self.full_init = (w0, mu0 + self.full[0][1].mean(0), 0.5 * (prec0 + np.transpose(prec0, (0, 2, 1))))
        # ---- VAD
        N = lo.window_size(FS)
        noise = np.clip(rng.normal(0, 120.0, 3 * FS), -32768, 32767).astype(np.int16)
        sig = np.clip(rng.normal(0, 120.0, 2 * FS) + np.pad(synth.synth_speech(5, 1.0, FS).astype(np.float64), (FS // 2, FS // 2)),
                      -32768, 32767).astype(np.int16)
        self.vad_N = N
        self.vad_na = lo.noise_spectrum(noise, N)
        self.vad_sigs = [sig, sig[:FS // 3].copy()]
        self._ltsd = L
        self._Batch, self._GMM, self._skgmm = Batch, GMM, skgmm

    # ------------------------------------------------------------------ the operations: name -> results (tuple of arrays)
    def run(self, name):
        from speaker_recognition_amd import _lib
        if name == "score_rogue":                         # delivers (host memory, no per-frame output)
            return self.ms_rogue.score(self.feats)
        if name == "score_diag":
            return self.ms_diag.score(self.feats)
        if name == "frame_ll":                            # does not deliver
            return self.ms_rogue.score(self.feats, frame_ll=True)
        if name == "fused":
            return self.ex.predict_batch(self.ms_rogue, self.pcm_batch, nd=2)
        if name == "score_all":
            return (np.array([self.legacy.score_all(self.X32)]),)
        if name == "gmm_score":
            return (self.legacy.score(self.X32),)
        if name == "predict_one":
            return (np.array(self.gmmset.predict_one_scores(self.X32[:self.off[1]])),)
        if name == "score_models":                        # sr_score_models_f32 in-process: the library's per-device packed-set cache
            import ctypes as C
            X = _lib.f32_matrix(self.X32[:self.off[1]])
            h = (C.c_void_p * len(self.rogue_gmms))(*[g.gmm for g in self.rogue_gmms])
            out = np.zeros(len(self.rogue_gmms))
            _lib.check(_lib.lib().sr_score_models_f32(h, len(self.rogue_gmms), _lib.as_fp(X), X.shape[0], X.shape[1], _lib.as_dp(out),
                                                      _lib.SR_CLAMP_COMPAT), "sr_score_models_f32")
            return (out,)
        if name in ("em_small", "em_f64", "em_iter"):
            X, start = self.em[name]
            if name == "em_iter":
                _lib.set_option("em_stats_engine", 3)         # an iteration per launch
            try:
                g = self._GMM.from_arrays(start.weights, start.mean, start.sigma)
                g.nr_iteration, g.init_with_kmeans, g.threshold = self.em_iters[name], -1, 0.0     # warm start, no stop rule
                it = g.fit(X)
            finally:
                _lib.set_option("em_stats_engine", 0)
            return (np.array([it]),) + g.params()
        if name == "em_map":
            X, _ = self.em[name]
            g = self._GMM(8, nr_iteration=self.em_iters[name], threshold=0.0)
            return (np.array([g.fit(X, ubm=self.ubm8)]),) + g.params()
        if name == "kmeans":
            g = self._GMM(nr_mixture=8, nr_iteration=0, init_with_kmeans=1, seed=5, concurrency=3)
            g.fit(self.km_X)
            return g.params()
        if name == "full_score":
            return self.full_set.score(self.full_batch, frame_ll=True)
        if name == "full_fit":
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", self._skgmm.ConvergenceWarning)
                w0, mu0, prec0 = self.full_init
                m = self._skgmm.GMM(4, tol=0.0, max_iter=3, weights_init=w0, means_init=mu0, precisions_init=prec0).fit(self.full_fit_X)
            return m.weights_, m.means_, m.covariances_, np.array([m.n_iter_])
        if name == "multi":
            return self.multi.predict(self.pcm, nd=2)
        if name == "vad":
            return tuple(self._ltsd.ltsd_values(self.vad_sigs, self.vad_na[:self.vad_N // 2 + 1].astype(np.float32), self.vad_N, 5))
        raise KeyError(name)

    def engine(self, name):
        """what decides whether two occurrences must agree bit for bit: the EM statistics engine that ran (em_small may hand a
        fit to another engine under contention)"""
        from speaker_recognition_amd import _lib
        return _lib.last_em_stats_engine() if name.startswith("em_") else None

    # ------------------------------------------------------------------ each operation once against its reference
    def check(self, name, res):
        from speaker_recognition_amd import _lib
        go = self.go
        # the engine each op is named for (checked on the occurrence that is compared with the reference, right after it ran)
        if name in ("score_rogue", "frame_ll", "predict_one", "score_models", "fused"):
            assert is_h2s(_lib.last_score_kernel()), (name, _lib.last_score_kernel())
        if name in ("em_small", "em_map", "em_f64", "em_iter"):
            want_eng = {"em_small": (4,), "em_map": (4,), "em_f64": (5,), "em_iter": (1, 2, 3)}[name]
            assert _lib.last_em_stats_engine() in want_eng, (name, _lib.last_em_stats_engine())
        if name == "score_rogue":
            check_sums(go, self.rogue, self.X, self.off, res[0], res[1], TOL_H2S)
        elif name == "score_diag":
            check_sums(go, self.diag, self.X, self.off, res[0], res[1], TOL)
        elif name == "frame_ll":
            want_ll = check_sums(go, self.rogue, self.X, self.off, res[0], res[1], TOL_H2S)
            rel = np.abs(res[2] - want_ll) / np.maximum(1.0, np.abs(want_ll))
            assert rel.max() < TOL_H2S, rel.max()
        elif name == "fused":
            from oracle import mfcc_oracle as mo
            feats = self.ex.extract_batch(self.pcm_batch, nd=2)
            Xd, off = feats.download().astype(np.float64), feats.offsets()
            for u, p in enumerate(self.pcm):
                ref = mo.extract(FS, p, diff=True, nd=2)
                assert np.max(np.abs(Xd[off[u]:off[u + 1]] - ref)) < 4e-5, u        # smoke()'s MFCC gate
            check_sums(go, self.rogue, Xd, off, res[0], res[1], TOL_H2S)
            for t in range(len(self.ticks)):                 # and what the rogue set's stream ticks must equal
                fb = self.ex.extract_batch(self._Batch.from_pcm(list(self.ticks[t])), nd=2)
                want = self.tick_want[("tick_graph", t)]
                check_sums(go, self.rogue, fb.download().astype(np.float64), fb.offsets(), want[0], want[1], TOL_H2S)
        elif name == "score_all":
            want = go.score_batch(go.GMMParams(*self.rogue[-1]), self.X)
            assert abs(res[0][0] - want.sum()) <= TOL * np.maximum(1.0, np.abs(want)).sum()
        elif name == "gmm_score":
            want = go.score_batch(go.GMMParams(*self.rogue[-1]), self.X)
            assert np.max(np.abs(res[0] - want) / np.maximum(1.0, np.abs(want))) < TOL
        elif name in ("predict_one", "score_models"):
            n = self.off[1]
            want_ll = oracle_ll(go, self.rogue, self.X[:n])
            assert np.all(np.abs(res[0] - want_ll.sum(axis=1)) <= TOL_H2S * np.maximum(1.0, np.abs(want_ll)).sum(axis=1))
        elif name in ("em_small", "em_f64", "em_map"):
            X, start = self.em[name]
            want = start
            for _ in range(self.em_iters[name]):
                want = go.em_iteration(want, X.astype(np.float64), **(dict(map_relevance=16.0, ubm=start) if name == "em_map" else {}))
            it, w, mu, sg = res
            assert it[0] == self.em_iters[name]
            if name == "em_map":      # means only (gmmubm.cc:29-38)
                assert np.array_equal(w, start.weights) and np.array_equal(sg, start.sigma)
                assert np.max(np.abs(mu - want.mean)) < 1e-6
            else:                     # tests/test_gpu_em_small.py, tests/test_gpu_em_f64.py
                err = (np.max(np.abs(w - want.weights)), np.max(np.abs(mu - want.mean)), np.max(np.abs(sg - want.sigma) / want.sigma))
                assert err[0] < 1e-7 and err[1] < 1e-6 and err[2] < 1e-6, err
        elif name == "em_iter":       # test_em_and_map_iteration_vs_oracle
            X, start = self.em[name]
            want = go.em_iteration(start, X.astype(np.float64))
            it, w, mu, sg = res
            assert it[0] == 1
            assert np.max(np.abs(w - want.weights)) < 1e-5 and np.max(np.abs(mu - want.mean)) < 1e-4
            assert np.max(np.abs(sg - want.sigma) / want.sigma) < 1e-3
        elif name == "kmeans":        # test_kmeans_initialiser_on_the_device_equals_its_restatement
            from oracle import init_oracle as io
            w0, mu0, sg0 = io.init_gaussians(self.km_X.astype(np.float64), 8, 1, 3, io.GlibcRand(5 + 1))
            w, mu, sg = res
            assert np.max(np.abs(mu - mu0)) < 1e-9 * max(1.0, np.max(np.abs(mu0)))
            assert np.max(np.abs(sg - sg0) / sg0) < 1e-12 and np.allclose(w, w0, atol=0)
        elif name == "full_score":    # tests/test_gpu_full_cov.py
            import fullcov_oracle as fo
            sums, arg, fll = res
            Xf = np.concatenate(self.full_utts).astype(np.float64)
            off = np.concatenate([[0], np.cumsum([len(u) for u in self.full_utts])])
            for s, (w, mu, cov) in enumerate(self.full):
                want = fo.score_samples(Xf, w, mu, fo.precision_cholesky(cov))
                assert np.max(np.abs(fll[s] - want) / np.maximum(1.0, np.abs(want))) < 1e-4, s
                for u in range(len(off) - 1):
                    assert abs(sums[u, s] - want[off[u]:off[u + 1]].sum()) <= 1e-4 * max(1.0, np.abs(want[off[u]:off[u + 1]]).sum())
        elif name == "full_fit":      # the float64 restatement, as test_fit_from_explicit_inits_matches_sklearn's gate
            import fullcov_oracle as fo
            w0, mu0, prec0 = self.full_init
            want = fo.fit(self.full_fit_X, w0, mu0, self._skgmm._precision_cholesky_from_precisions(prec0), tol=0.0, max_iter=3)
            w, mu, cov, n_iter = res
            assert n_iter[0] == 3
            for got, key in ((w, "weights"), (mu, "means"), (cov, "covariances")):
                rel = np.linalg.norm(got - want[key]) / np.linalg.norm(want[key])
                assert rel < 1e-9, (key, rel)
        elif name == "multi":         # test_multi_slot_prediction_equals_single_device; the fused step itself against the oracle
            assert np.array_equal(res[0], self.multi_want[0]) and np.array_equal(res[1], self.multi_want[1])
            feats = self.ex.extract_batch(self.pcm_batch, nd=2)
            check_sums(go, self.diag, feats.download().astype(np.float64), feats.offsets(), res[0], res[1], TOL)
        elif name == "vad":           # tests/test_gpu_vad.py
            from oracle import ltsd_oracle as lo
            for s, g in zip(self.vad_sigs, res):
                want = lo.ltsd(s, self.vad_na, self.vad_N, 5)
                assert g.shape == want.shape
                if len(want):
                    assert np.max(np.abs(g - want)) < 2e-3
        else:
            raise KeyError(name)
