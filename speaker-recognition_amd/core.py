"""Handle wrappers over the sr_* part of the C ABI: device batches, speaker sets, the MFCC
extractor object.  Thin by design -- marshalling only, all arithmetic is in lib/pygmm.so."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import SRError, check, lib


class Batch:
    """An utterance batch resident in HBM (PCM or features); frees its device memory on GC."""

    def __init__(self, handle, owner=True):
        if not handle:
            raise SRError("batch creation failed: %s" % _lib.last_error())
        self._h = C.c_void_p(handle)
        self._owner = owner

    @classmethod
    def from_pcm(cls, signals) -> "Batch":
        """``signals``: list of 1-D arrays (int16 -> stays int16 on the device; anything else is
        sent as float32), or a tuple ``(concatenated, offsets)``."""
        if isinstance(signals, tuple):
            cat, offsets = signals
            cat = np.ascontiguousarray(cat)
            offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        else:
            sigs = [np.asarray(s) for s in signals]
            for s in sigs:
                if s.ndim != 1:
                    raise ValueError("Only Support Mono Wav File!")   # gui/utils.py:12
            offsets = np.zeros(len(sigs) + 1, dtype=np.int64)
            offsets[1:] = np.cumsum([len(s) for s in sigs])
            all_i16 = all(s.dtype == np.int16 for s in sigs)
            cat = (np.concatenate(sigs) if sigs else np.zeros(0, np.int16))
            cat = np.ascontiguousarray(cat if all_i16 else cat.astype(np.float32))
        if cat.dtype == np.int16:
            h = lib().sr_batch_from_pcm(cat.ctypes.data_as(C.POINTER(C.c_int16)),
                                        _lib.as_i64p(offsets), len(offsets) - 1)
        else:
            cat = np.ascontiguousarray(cat, dtype=np.float32)
            h = lib().sr_batch_from_pcm_f32(_lib.as_fp(cat), _lib.as_i64p(offsets), len(offsets) - 1)
        return cls(h)

    @classmethod
    def from_features(cls, X, offsets=None) -> "Batch":
        """``X``: [n, dim] matrix with ``offsets`` [U+1], or a list of [T_u, dim] matrices."""
        if offsets is None and isinstance(X, (list, tuple)):
            if X and all(isinstance(x, np.ndarray) and x.ndim == 2 for x in X):
                # what feature extraction hands over -- float64 matrices (MFCC.py:69-79) -- converted WHILE they are gathered:
                # one pass over the frames instead of a float32 copy per utterance and a second pass to join them
                mats = X
                X = np.concatenate(mats, axis=0, dtype=np.float32, casting="unsafe")
            else:
                mats = [_lib.f32_matrix(x) for x in X]
                X = np.concatenate(mats, axis=0) if mats else np.zeros((0, 1), np.float32)
            offsets = np.zeros(len(mats) + 1, dtype=np.int64)
            offsets[1:] = np.cumsum([m.shape[0] for m in mats])
        X = _lib.f32_matrix(X)
        if offsets is None:
            offsets = np.array([0, X.shape[0]], dtype=np.int64)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        h = lib().sr_batch_from_features(_lib.as_fp(X), X.shape[0], X.shape[1],
                                         _lib.as_i64p(offsets), len(offsets) - 1)
        return cls(h)

    def update_pcm(self, samples) -> None:
        """Overwrite the batch's int16 samples in place (same layout): the serving loop's H2D."""
        a = np.ascontiguousarray(samples, dtype=np.int16)
        check(lib().sr_batch_update_pcm(self._h, a.ctypes.data_as(C.POINTER(C.c_int16)), a.size),
              "sr_batch_update_pcm")

    def reset_pcm(self, signals) -> None:
        """New int16 signals with a new layout into the same device buffers (they only grow)."""
        sigs = [np.ascontiguousarray(x, dtype=np.int16) for x in signals]
        offsets = np.zeros(len(sigs) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([len(x) for x in sigs])
        cat = np.ascontiguousarray(np.concatenate(sigs)) if sigs else np.zeros(0, np.int16)
        check(lib().sr_batch_reset_pcm(self._h, cat.ctypes.data_as(C.POINTER(C.c_int16)), _lib.as_i64p(offsets),
                                       len(sigs)), "sr_batch_reset_pcm")

    def reset_features(self, X) -> None:
        """One [T, dim] matrix as the batch's single utterance, into the same device buffers (they only grow): what the
        reference's per-utterance loop (gmmset.py:62-64) costs nothing but the upload with."""
        X = _lib.f32_matrix(X)
        offsets = np.array([0, X.shape[0]], dtype=np.int64)
        check(lib().sr_batch_reset_features(self._h, _lib.as_fp(X), X.shape[0], X.shape[1], _lib.as_i64p(offsets), 1),
              "sr_batch_reset_features")

    @property
    def n_utt(self) -> int:
        return lib().sr_batch_num_utterances(self._h)

    @property
    def n_rows(self) -> int:
        return int(lib().sr_batch_num_rows(self._h))

    @property
    def dim(self) -> int:
        return lib().sr_batch_dim(self._h)

    def offsets(self) -> np.ndarray:
        out = np.zeros(self.n_utt + 1, dtype=np.int64)
        check(lib().sr_batch_offsets(self._h, _lib.as_i64p(out)), "sr_batch_offsets")
        return out

    def download(self) -> np.ndarray:
        out = np.empty((self.n_rows, self.dim), dtype=np.float32)
        check(lib().sr_batch_download(self._h, _lib.as_fp(out)), "sr_batch_download")
        return out

    def download_pcm(self) -> np.ndarray:
        """The int16 samples of a PCM batch, concatenated (``offsets()`` cuts them into utterances)."""
        out = np.empty(self.n_rows, dtype=np.int16)
        check(lib().sr_batch_download_pcm16(self._h, out.ctypes.data_as(C.POINTER(C.c_int16))), "sr_batch_download_pcm16")
        return out

    def remove_silence(self, fs, frame_duration=0.02, frame_shift=0.01, perc=0.15) -> "Batch":
        """The reference's energy-threshold silence removal (src/filters/silence.py:11-50) on every utterance of an int16 PCM
        batch, on the device (sr_silence_remove_batch): -> a new device-resident PCM batch, bit-identical to the reference's
        output per utterance, usable by ``MfccExtractor.extract_batch`` / ``predict_batch`` / ``predict_batch_open`` as it is.
        An utterance may come out empty (``perc`` >= 1): it has no frames and ``predict_batch`` gives it -1."""
        h = lib().sr_silence_remove_batch(self._h, float(fs), float(frame_duration), float(frame_shift), float(perc), None)
        if not h:
            raise SRError("sr_silence_remove_batch failed: %s" % _lib.last_error())
        return Batch(h)

    def normalise(self, mode="warp", window=301, ranks=False, counts=False):
        """Short-time feature normalisation of every utterance of a feature batch, on the device (sr_feature_norm_batch): -> a
        new device-resident feature batch of the same layout.  ``mode``: "warp" (feature warping: each value mapped through its
        mid-rank in a window of ``window`` frames onto a standard normal), "cmn" or "cmvn" (the window's mean, or mean and
        variance, in float64).  The window is centred, and shifted -- not shortened -- at both ends of an utterance.
        ``counts=True`` also returns the per-utterance int64 counts of degenerate cells (warp: NaN cells; cmvn: windows of equal
        values, which give 0), ``ranks=True`` the int32 doubled mid-ranks [rows, dim] (warp only; for tests): the result is then
        the tuple (batch[, ranks][, counts])."""
        deg = np.zeros(max(1, self.n_utt), dtype=np.int64) if counts else None
        rk = np.empty((self.n_rows, self.dim), dtype=np.int32) if ranks else None
        h = lib().sr_feature_norm_batch(self._h, _lib.feature_norm_mode(mode), int(window), None if deg is None else _lib.as_i64p(deg),
                                        None if rk is None else rk.ctypes.data_as(C.POINTER(C.c_int32)))
        if not h:
            raise SRError("sr_feature_norm_batch failed: %s" % _lib.last_error())
        out = (Batch(h),) + ((rk,) if ranks else ()) + ((deg[:self.n_utt],) if counts else ())
        return out if len(out) > 1 else out[0]

    def segment_stats(self, L: int):
        """Full-covariance statistics of the base segments of ``L`` frames of every recording of a feature batch, computed on the
        device and brought home (sr_diar_stats_batch): -> (segment offsets [U + 1], statistics [n_seg, 1 + D + D (D + 1) / 2]
        float64: N, s, the lower triangle of Q by rows)."""
        lengths = np.diff(self.offsets())
        cap = int(sum(_lib.diar_segments(int(n), int(L)) for n in lengths)) if isinstance(L, (int, np.integer)) and L >= 1 else 0
        seg_off = np.zeros(self.n_utt + 1, dtype=np.int64)
        stats = np.zeros((max(cap, 1), _lib.diar_stat_len(max(self.dim, 1))), dtype=np.float64)
        check(lib().sr_diar_stats_batch(self._h, int(L), cap, _lib.as_i64p(seg_off), _lib.as_dp(stats)), "sr_diar_stats_batch")
        return seg_off, stats[:cap]

    def diarize(self, L: int = 100, change: str = "bic", half_width: int = 2, penalty: float = 1.0, ridge: float = 1e-3,
                threshold: float = 0.0, k_min: int = 1, k_max: int = 0):
        """Clusters the frames of every recording of a feature batch with nobody enrolled (sr_diar_cluster_batch; include/pygmm_hip.h
        "Who spoke when, nobody enrolled"): base segments of ``L`` frames, BIC change detection (``change`` "bic", half-width
        ``half_width`` segments) or none ("uniform"), agglomerative clustering under delta-BIC with weight ``penalty`` until no pair
        lies below ``threshold`` (never below ``k_min`` clusters; ``k_max`` > 0: down to at most that many whatever the distance).
        -> a list with one dict per recording: ``labels`` (per initial cluster), ``init_off`` (the initial clusters' runs in
        base-segment indices), ``merge_i``, ``merge_j``, ``merge_d`` (the steps taken), ``n_clusters``, ``failed``, ``n_seg``."""
        tail = _diar_args(L, change, half_width, penalty, ridge, threshold, k_min, k_max)
        return _diar_call(lib().sr_diar_cluster_batch, "sr_diar_cluster_batch", (self._h,), tail, np.diff(self.offsets()))

    def __del__(self):
        try:
            if self._owner and self._h:
                lib().sr_batch_free(self._h)
                self._h = None
        except Exception:
            pass


class ModelSet:
    """S models packed once and resident on the device (one fused scoring launch for all)."""

    def __init__(self, gmms):
        self._keep = list(gmms)
        arr = (C.c_void_p * len(self._keep))(*[g.gmm for g in self._keep])
        h = lib().sr_modelset_create(arr, len(self._keep))
        if not h:
            raise SRError("sr_modelset_create failed: %s" % _lib.last_error())
        self._h = C.c_void_p(h)

    def __len__(self):
        return lib().sr_modelset_size(self._h)

    @property
    def dim(self) -> int:
        return lib().sr_modelset_dim(self._h)

    def info(self) -> dict:
        """Conditioning of the packed set as the engine dispatcher sees it (sr_modelset_info)."""
        out = np.zeros(8)
        check(lib().sr_modelset_info(self._h, _lib.as_dp(out)), "sr_modelset_info")
        return {"amp": out[0], "pad_waste": out[1], "sigma_ratio": out[2], "coef_max": out[3],
                "shared_sigma": bool(out[4]), "models": int(out[5]), "device": int(out[6]),
                "hybrid_vector_mixtures": int(out[7])}

    def score(self, feats: Batch, frame_ll: bool = False, clamp_compat: bool = True):
        """-> (sums[U, S] float64, argmax[U] int32[, frame_ll[S, n] float32])."""
        U, S = feats.n_utt, len(self)
        sums = np.zeros((U, S), dtype=np.float64)
        arg = np.full(U, -1, dtype=np.int32)
        fll = np.empty((S, feats.n_rows), dtype=np.float32) if frame_ll else None
        check(lib().sr_score_batch_set(self._h, feats._h, _lib.as_dp(sums), _lib.as_i32p(arg),
                                       _lib.as_fp(fll) if frame_ll else None,
                                       _lib.SR_CLAMP_COMPAT if clamp_compat else 0),
              "sr_score_batch_set")
        return (sums, arg, fll) if frame_ll else (sums, arg)

    def score_open(self, feats: Batch, bg: int, threshold: float, clamp_compat: bool = True):
        """The same pass with the open-set decision taken on the device (sr_score_batch_set_open): column ``bg`` is the
        background model (the UBM); -> (sums[U, S] float64, labels[U] int32, margins[U] float64).  A label is the first maximum
        of sums / frames over the other columns, or -1 when its margin over the background's sums / frames is below
        ``threshold`` (gmmset.py:69-81); an utterance without frames has label -1 and margin NaN."""
        U, S = feats.n_utt, len(self)
        sums = np.zeros((U, S), dtype=np.float64)
        labels = np.full(U, -1, dtype=np.int32)
        margins = np.full(U, np.nan, dtype=np.float64)
        check(lib().sr_score_batch_set_open(self._h, feats._h, int(bg), float(threshold), _lib.as_dp(sums), _lib.as_i32p(labels),
                                            _lib.as_dp(margins), _lib.SR_CLAMP_COMPAT if clamp_compat else 0),
              "sr_score_batch_set_open")
        return sums, labels, margins

    def score_topc(self, feats: Batch, bg: int, top_c: int, frame_ll: bool = False, selection: bool = False, clamp_compat: bool = True):
        """Top-C Gaussian selection (sr_score_batch_set_topc; Reynolds, Quatieri & Dunn 2000) for a set whose models share sigma
        and weights with the background model in column ``bg`` (speakers MAP-adapted from one UBM): per frame the ``top_c`` best
        components of the background model are found and only those are evaluated in every other model; the background column
        stays exact.  An approximation (``top_c`` = the mixture count reproduces ``score``), so nothing else takes this path.
        -> (sums[U, S] float64, argmax[U] int32[, frame_ll[S, n] float32][, selection[n, top_c] int32]).  A set that does not
        qualify, ``bg`` or ``top_c`` out of range, or a PCM batch raise ``SRError`` before the device is touched."""
        U, S = feats.n_utt, len(self)
        sums = np.zeros((U, S), dtype=np.float64)
        arg = np.full(U, -1, dtype=np.int32)
        fll = np.empty((S, feats.n_rows), dtype=np.float32) if frame_ll else None
        sel = np.full((feats.n_rows, max(0, int(top_c))), -1, dtype=np.int32) if selection else None
        check(lib().sr_score_batch_set_topc(self._h, feats._h, int(bg), int(top_c), _lib.as_dp(sums), _lib.as_i32p(arg),
                                            _lib.as_i32p(sel) if selection else None, _lib.as_fp(fll) if frame_ll else None,
                                            _lib.SR_CLAMP_COMPAT if clamp_compat else 0), "sr_score_batch_set_topc")
        return (sums, arg) + ((fll,) if frame_ll else ()) + ((sel,) if selection else ())

    def timeline(self, feats: Batch, window: int, hop: int, bg=None, threshold: float = 0.0, smooth: str = "hold", switch_penalty=None,
                 min_windows: int = 1, scores: bool = False, clamp_compat: bool = True):
        """Who speaks when in every recording of a feature batch (sr_timeline_batch): the batch is scored once, the per-frame
        values are summed over windows of ``window`` frames every ``hop`` frames on the device, and every window gets a label: a
        column of the set, or -1 ("nobody") where column ``bg`` (the UBM) plus ``threshold`` beats every speaker.  ``smooth``:
        "none" (the first maximum per window), "hold" (the reference GUI's rule: a new label shows once two consecutive windows
        agree) or "viterbi" (the best path under ``switch_penalty`` per label change, runs of at least ``min_windows`` windows;
        ``switch_penalty`` has no default and must be given).  -> a list of int32 label arrays, one per recording; with
        ``scores`` -> (labels, path scores [U] (NaN unless viterbi), window sums [Nw, S] per recording)."""
        tail = _timeline_args(window, hop, bg, threshold, smooth, switch_penalty, min_windows)
        lengths = np.diff(feats.offsets())
        return _timeline_call(lib().sr_timeline_batch, "sr_timeline_batch", (self._h, feats._h),
                              tail + (_lib.SR_CLAMP_COMPAT if clamp_compat else 0,), lengths, len(self), scores)

    def bw_stats(self, feats: Batch, model: int = 0, ll: bool = False, resident: bool = False):
        """Baum-Welch statistics of every utterance of a feature batch against model ``model`` of the set, the UBM
        (sr_bw_stats_batch): -> (N[U, K], F[U, K * D][, ll[U], dropped[U]]), float64 (dropped: int64).  N[u, k] = sum_t gamma_k(t),
        F[u, k * D + d] = sum_t gamma_k(t) x_t[d] (mixture-major, the supervector order), ll[u] the utterance's log-likelihood;
        a frame whose log-sum-exp is not finite (a NaN row, values beyond every density's range) contributes nothing and is
        counted in ``dropped``.  A PCM batch, a model index out of range, rows wider than 40 dimensions or a dimension mismatch
        raise ``SRError`` before the device is touched.  ``resident``: N and F stay on the device in a ``jfa.Stats`` (the same
        passes, the same bits; sr_bw_stats_resident) -> stats, or (stats, ll, dropped)."""
        model = int(model)
        K = self._keep[model].get_nr_mixtures() if 0 <= model < len(self._keep) else 0
        U, D = feats.n_utt, self.dim
        if resident:
            from .jfa import Stats
            lls = np.zeros(U, dtype=np.float64)
            dropped = np.zeros(U, dtype=np.int64)
            h = check(lib().sr_bw_stats_resident(self._h, model, feats._h, _lib.as_dp(lls), _lib.as_i64p(dropped)), "sr_bw_stats_resident")
            stats = Stats(h)
            return (stats, lls, dropped) if ll else stats
        N = np.zeros((U, K), dtype=np.float64)
        F = np.zeros((U, K * D), dtype=np.float64)
        lls = np.zeros(U, dtype=np.float64)
        dropped = np.zeros(U, dtype=np.int64)
        check(lib().sr_bw_stats_batch(self._h, model, feats._h, _lib.as_dp(N), _lib.as_dp(F), _lib.as_dp(lls), _lib.as_i64p(dropped)),
              "sr_bw_stats_batch")
        return (N, F, lls, dropped) if ll else (N, F)

    def __del__(self):
        try:
            if self._h:
                lib().sr_modelset_free(self._h)
                self._h = None
        except Exception:
            pass


class MfccExtractor:
    """Device MFCC extractor; constants as MFCCExtractor.__init__ (src/feature/MFCC.py:20-41)."""

    def __init__(self, fs, win_length_ms=32, win_shift_ms=16, FFT_SIZE=2048, n_filters=50,
                 n_ceps=13, pre_emphasis_coef=0.95, n_lpc=0):
        h = lib().sr_mfcc_create(float(fs), float(win_length_ms), float(win_shift_ms),
                                 int(FFT_SIZE), int(n_filters), int(n_ceps), float(pre_emphasis_coef))
        if not h:
            raise SRError("sr_mfcc_create failed: %s" % _lib.last_error())
        self._h = C.c_void_p(h)
        self.n_lpc = int(n_lpc)        # > 0: every frame also carries LPC-n_lpc columns (mix_feature)
        if self.n_lpc:
            check(lib().sr_mfcc_set_lpc(self._h, self.n_lpc), "sr_mfcc_set_lpc")
        self.fs, self.FFT_SIZE, self.n_bands, self.coefs = fs, FFT_SIZE, n_filters, n_ceps
        self.PRE_EMPH = pre_emphasis_coef
        self.FRAME_LEN = lib().sr_mfcc_frame_len(self._h)
        self.FRAME_SHIFT = lib().sr_mfcc_frame_shift(self._h)

    def tables(self):
        """Host float64 constants (window, mel bank M, DCT rows D) -- for tests."""
        win = np.empty(self.FRAME_LEN)
        M = np.empty((self.n_bands, self.FFT_SIZE // 2 + 1))
        D = np.empty((self.coefs, self.n_bands))
        check(lib().sr_mfcc_tables(self._h, _lib.as_dp(win), _lib.as_dp(M), _lib.as_dp(D)), "sr_mfcc_tables")
        return win, M, D

    def num_frames(self, n_samples: int) -> int:
        return int(lib().sr_mfcc_num_frames(self._h, int(n_samples)))

    def extract_batch(self, pcm: Batch, nd: int = 0, cmvn: bool = True, norm=None, norm_window: int = 301) -> Batch:
        """``norm`` ("warp", "cmn" or "cmvn"; default off): the features go through ``Batch.normalise(norm, norm_window)`` before
        they are returned, both stages resident (the per-utterance ``cmvn`` is the caller's choice: usually False with it)."""
        if norm is not None and _lib.feature_norm_mode(norm) < 0:
            raise ValueError("norm must be None, 'warp', 'cmn' or 'cmvn' (got %r)" % (norm,))
        h = lib().sr_mfcc_extract_batch(self._h, pcm._h, int(nd), 1 if cmvn else 0)
        if not h:
            raise SRError("sr_mfcc_extract_batch failed: %s" % _lib.last_error())
        out = Batch(h)
        return out if norm is None else out.normalise(norm, norm_window)

    def embed_batch(self, net, pcm: Batch, nd: int = 0, cmvn: bool = True, norm=None, segments=None, norm_window: int = 301) -> np.ndarray:
        """Speaker embeddings from resident PCM: ``extract_batch`` followed by ``net.extract`` (an ``xvector.XVector``), the features
        never leaving the device; the bits of the two calls made one after the other.  ``segments``: as ``XVector.extract``, in
        feature frames.  -> float32 [n, E]."""
        return net.extract(self.extract_batch(pcm, nd, cmvn, norm, norm_window), segments=segments)

    def extract(self, signal, nd: int = 0, cmvn: bool = True) -> np.ndarray:
        """One utterance -> float64 [T - nd, n_ceps*(nd+1)] (what MFCCExtractor.extract returns,
        MFCC.py:49-79, plus optional deltas)."""
        signal = np.asarray(signal)
        if signal.ndim > 1:
            signal = np.mean(signal, axis=1)                      # MFCC.py:53-55
        assert len(signal) > 5 * self.FRAME_LEN, "Signal too short!"  # MFCC.py:56
        out = self.extract_batch(Batch.from_pcm([signal]), nd, cmvn)
        return out.download().astype(np.float64)

    def predict_batch(self, models: ModelSet, pcm: Batch, nd: int = 0, clamp_compat: bool = True, out=None):
        """Fused serving step on resident PCM: MFCC -> CMVN/deltas -> scoring -> argmax.
        ``out`` = (float64[U, S], int32[U]) C-contiguous arrays to fill instead of fresh ones: a serving loop that keeps its result
        buffers spares the page faults of 8 U S new bytes per call (and may page-lock them once with ``_lib.host_register``, so that
        the results leave the device by DMA)."""
        U, S = pcm.n_utt, len(models)
        if out is None:
            sums = np.zeros((U, S), dtype=np.float64)
            arg = np.full(U, -1, dtype=np.int32)
        else:
            sums, arg = out
            if sums.shape != (U, S) or sums.dtype != np.float64 or not sums.flags.c_contiguous or arg.shape != (U,) or \
                    arg.dtype != np.int32 or not arg.flags.c_contiguous:
                raise ValueError("out must be (float64[%d, %d], int32[%d]), C-contiguous" % (U, S, U))
        check(lib().sr_predict_pcm_batch(self._h, models._h, pcm._h, int(nd), _lib.as_dp(sums),
                                         _lib.as_i32p(arg), _lib.SR_CLAMP_COMPAT if clamp_compat else 0),
              "sr_predict_pcm_batch")
        return sums, arg

    def predict_batch_open(self, models: ModelSet, pcm: Batch, bg: int, threshold: float, nd: int = 0, clamp_compat: bool = True):
        """``predict_batch`` with the open-set decision of ``ModelSet.score_open`` (sr_predict_pcm_batch_open):
        -> (sums[U, S], labels[U] int32, margins[U] float64)."""
        U, S = pcm.n_utt, len(models)
        sums = np.zeros((U, S), dtype=np.float64)
        labels = np.full(U, -1, dtype=np.int32)
        margins = np.full(U, np.nan, dtype=np.float64)
        check(lib().sr_predict_pcm_batch_open(self._h, models._h, pcm._h, int(nd), int(bg), float(threshold), _lib.as_dp(sums),
                                              _lib.as_i32p(labels), _lib.as_dp(margins),
                                              _lib.SR_CLAMP_COMPAT if clamp_compat else 0), "sr_predict_pcm_batch_open")
        return sums, labels, margins

    def timeline_batch(self, models: ModelSet, pcm: Batch, window: int, hop: int, nd: int = 0, bg=None, threshold: float = 0.0,
                       smooth: str = "hold", switch_penalty=None, min_windows: int = 1, scores: bool = False, clamp_compat: bool = True):
        """``ModelSet.timeline`` from resident PCM in one call (sr_timeline_pcm_batch): MFCC -> CMVN / deltas -> scoring -> window
        sums -> labels; the bits of ``extract_batch`` followed by ``ModelSet.timeline``."""
        tail = _timeline_args(window, hop, bg, threshold, smooth, switch_penalty, min_windows)
        lengths = [max(0, self.num_frames(int(n)) - int(nd)) for n in np.diff(pcm.offsets())]
        return _timeline_call(lib().sr_timeline_pcm_batch, "sr_timeline_pcm_batch", (self._h, models._h, pcm._h, int(nd)),
                              tail + (_lib.SR_CLAMP_COMPAT if clamp_compat else 0,), lengths, len(models), scores)

    def diarize_batch(self, pcm: Batch, nd: int = 0, L: int = 100, change: str = "bic", half_width: int = 2, penalty: float = 1.0,
                      ridge: float = 1e-3, threshold: float = 0.0, k_min: int = 1, k_max: int = 0):
        """``Batch.diarize`` from resident PCM in one call (sr_diar_cluster_pcm_batch): MFCC -> CMVN / deltas -> statistics ->
        change detection -> clustering; the bits of ``extract_batch`` followed by ``Batch.diarize``."""
        tail = _diar_args(L, change, half_width, penalty, ridge, threshold, k_min, k_max)
        lengths = [max(0, self.num_frames(int(n)) - int(nd)) for n in np.diff(pcm.offsets())]
        return _diar_call(lib().sr_diar_cluster_pcm_batch, "sr_diar_cluster_pcm_batch", (self._h, pcm._h, int(nd)), tail, lengths)

    def predict_batch_topc(self, models: ModelSet, pcm: Batch, bg: int, top_c: int, nd: int = 0, clamp_compat: bool = True):
        """``predict_batch`` through ``ModelSet.score_topc`` (sr_predict_pcm_batch_topc): the features stay on the device;
        -> (sums[U, S], argmax[U] int32), the bits of ``extract_batch`` followed by ``score_topc``."""
        U, S = pcm.n_utt, len(models)
        sums = np.zeros((U, S), dtype=np.float64)
        arg = np.full(U, -1, dtype=np.int32)
        check(lib().sr_predict_pcm_batch_topc(self._h, models._h, pcm._h, int(nd), int(bg), int(top_c), _lib.as_dp(sums),
                                              _lib.as_i32p(arg), _lib.SR_CLAMP_COMPAT if clamp_compat else 0), "sr_predict_pcm_batch_topc")
        return sums, arg

    def __del__(self):
        try:
            if self._h:
                lib().sr_mfcc_free(self._h)
                self._h = None
        except Exception:
            pass


def _timeline_args(window, hop, bg, threshold, smooth, switch_penalty, min_windows):
    """The checked arguments of a timeline call, as the C ABI takes them: (window, hop, bg, threshold, mode, beta, min_dur)."""
    mode = _lib.timeline_mode(smooth)
    if mode < 0:
        raise ValueError("smooth must be 'none', 'hold' or 'viterbi' (got %r)" % (smooth,))
    if mode == 2 and switch_penalty is None:
        raise ValueError("smooth='viterbi' needs an explicit switch_penalty: there is no data-tuned default")
    for name, v in (("window", window), ("hop", hop), ("min_windows", min_windows)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s must be an integer number of %s (got %r)" % (name, "windows" if name == "min_windows" else "frames", v))
    return (int(window), int(hop), -1 if bg is None else int(bg), float(threshold), mode,
            0.0 if switch_penalty is None else float(switch_penalty), int(min_windows))


def _diar_args(L, change, half_width, penalty, ridge, threshold, k_min, k_max):
    """The checked arguments of a diarisation call, as the C ABI takes them: (L, change, m, lambda, ridge, threshold, k_min, k_max)."""
    mode = _lib.diar_change_mode(change)
    if mode < 0:
        raise ValueError("change must be 'bic' or 'uniform' (got %r)" % (change,))
    for name, v in (("L", L), ("half_width", half_width), ("k_min", k_min), ("k_max", k_max)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s must be an integer (got %r)" % (name, v))
    return (int(L), mode, int(half_width), float(penalty), float(ridge), float(threshold), int(k_min), int(k_max))


def _diar_call(fn, what, head, tail, lengths):
    """Runs sr_diar_cluster_batch / _pcm_batch; ``lengths``: the frames of every recording.  -> a dict per recording."""
    L = tail[0]
    U = len(lengths)
    n_seg = [_lib.diar_segments(int(n), L) if L >= 1 else 0 for n in lengths]
    cap = int(sum(n_seg))
    i32 = C.POINTER(C.c_int32)
    cl_off = np.zeros(U + 1, dtype=np.int64)
    init_off = np.zeros(cap + U + 1, dtype=np.int64)
    mi, mj, lab = (np.zeros(max(cap, 1), dtype=np.int32) for _ in range(3))
    md = np.zeros(max(cap, 1), dtype=np.float64)
    nm, nc, nf = (np.zeros(max(U, 1), dtype=np.int64) for _ in range(3))
    check(fn(*head, *tail, cap, _lib.as_i64p(cl_off), _lib.as_i64p(init_off), mi.ctypes.data_as(i32), mj.ctypes.data_as(i32), _lib.as_dp(md),
             lab.ctypes.data_as(i32), _lib.as_i64p(nm), _lib.as_i64p(nc), _lib.as_i64p(nf)), what)
    out = []
    for u in range(U):
        a, b, t = int(cl_off[u]), int(cl_off[u + 1]), int(nm[u])
        out.append(dict(labels=lab[a:b].copy(), init_off=init_off[a + u:b + u + 1].copy(), merge_i=mi[a:a + t].copy(), merge_j=mj[a:a + t].copy(),
                        merge_d=md[a:a + t].copy(), n_clusters=int(nc[u]), failed=int(nf[u]), n_seg=n_seg[u]))
    return out


def _timeline_call(fn, what, head, tail, lengths, S, scores):
    """Runs one of the sr_*timeline*_batch calls: ``head`` / ``tail`` are its arguments before / after (window ... min_dur [flags]);
    ``lengths`` the frames of every recording.  -> per-recording label arrays[, path scores[U], sums per recording]."""
    window, hop = tail[0], tail[1]
    U = len(lengths)
    nw = [_lib.timeline_windows(int(n), window, hop) if window >= 1 and hop >= 1 else 0 for n in lengths]
    total = int(sum(nw))
    win_off = np.zeros(U + 1, dtype=np.int64)
    labels = np.full(max(total, 1), -1, dtype=np.int32)
    sums = np.zeros((max(total, 1), S), dtype=np.float64) if scores else None
    path = np.zeros(max(U, 1), dtype=np.float64)
    bad = np.zeros(max(U, 1), dtype=np.int64)
    check(fn(*head, *tail, _lib.as_i64p(win_off), _lib.as_i32p(labels), _lib.as_dp(sums) if scores else None, _lib.as_dp(path),
             _lib.as_i64p(bad)), what)
    if [int(x) for x in np.diff(win_off)] != nw:
        raise SRError("%s: the library counted other windows than the caller (%r against %r)" % (what, np.diff(win_off).tolist(), nw))
    out = [labels[win_off[u]:win_off[u + 1]].copy() for u in range(U)]
    if not scores:
        return out
    return out, path[:U].copy(), [sums[win_off[u]:win_off[u + 1]].copy() for u in range(U)]


def open_set_decide(sums, n_frames, bg: int, threshold: float):
    """The open-set rule on sums the caller holds (sr_open_set_decide): ``sums`` [U, S] float64, ``n_frames`` [U];
    -> (labels[U] int32, margins[U] float64), as ``ModelSet.score_open`` gives them."""
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    if sums.ndim != 2:
        raise ValueError("expected [utterances, models] sums, got shape %r" % (sums.shape,))
    n = np.ascontiguousarray(n_frames, dtype=np.int64)
    U, S = sums.shape
    if n.shape != (U,):
        raise ValueError("expected %d frame counts, got shape %r" % (U, n.shape))
    labels = np.full(U, -1, dtype=np.int32)
    margins = np.full(U, np.nan, dtype=np.float64)
    check(lib().sr_open_set_decide(_lib.as_dp(sums), U, S, int(bg), _lib.as_i64p(n), float(threshold), _lib.as_i32p(labels),
                                   _lib.as_dp(margins)), "sr_open_set_decide")
    return labels, margins


def vad_thresholds(lambda0, lambda1):
    """The float64 thresholds the device compares a float32 LTSD value with so that it decides as ``filters.ltsd.voiced_runs``
    does under the numpy in use: ``ltsds > lambda0`` (an array against a Python float) and ``np.max(...) > lambda1`` (a float32
    scalar against one) compare in whatever type numpy promotes to -- float32 for both since NEP 50, float32 and float64 before --
    and a comparison in float32 is the comparison in float64 against the threshold rounded to float32."""
    t0 = np.result_type(np.zeros(1, np.float32), float(lambda0))
    t1 = np.result_type(np.float32(0), float(lambda1))
    return float(t0.type(lambda0)), float(t1.type(lambda1))


class ServingStream:
    """Double-buffered fixed-shape serving session (sr_stream_*): ``n_windows`` windows of
    ``window_samples`` int16 samples per tick; ``submit`` queues a tick (H2D on its own HIP stream,
    overlapping the previous tick's kernels), ``collect`` returns the oldest tick's decisions.
    ``graph=True`` replays each tick's kernels and result copies as one captured hipGraph.
    ``models`` is a diagonal ``ModelSet`` or a full-covariance ``skgmm.FullSet`` (chosen by type; ``clamp_compat`` does not
    apply to the latter, whose ticks give ``FullSet.predict_pcm``'s results).
    ``vad``: an initialised ``filters.VAD`` (or ``filters.ltsd.LTSD_VAD``) of the extractor's sampling rate puts the reference's
    voice-activity front end in front of every window, on the device (sr_stream_create_vad): a window is scored on its voiced
    samples alone, as ``ModelInterface.filter`` + the fused call would score it, and only if more than a third of it is voiced --
    otherwise its sums are 0 and its argmax -1.  ``collect`` returns what it always did; the voiced sample counts of the tick
    collected last are in ``last_voiced`` (``collect_vad`` returns them as a fourth value).  ``nd`` must be 0 then.
    ``open_set=(bg, threshold)`` (a diagonal ``ModelSet`` whose column ``bg`` is the UBM): every tick also takes the open-set
    decision of ``ModelSet.score_open`` on the device (sr_stream_set_open); ``collect_open`` returns it.  The pair is fixed for
    the session's life."""

    def __init__(self, extractor: MfccExtractor, models, n_windows: int, window_samples: int,
                 nd: int = 0, clamp_compat: bool = True, graph: bool = False, vad=None, open_set=None):
        from .skgmm import FullSet
        self._keep = (extractor, models)
        self.n_windows, self.window_samples, self.n_models = int(n_windows), int(window_samples), len(models)
        self.vad, self.last_voiced = vad is not None, None
        if vad is not None:
            if not isinstance(models, (FullSet, ModelSet)):
                raise TypeError("models must be a core.ModelSet or an skgmm.FullSet (got %s)" % type(models).__name__)
            det = getattr(vad, "ltsd", vad)             # filters.VAD wraps the detector
            if getattr(det, "noise_amp", None) is None:
                raise ValueError("vad is not initialised: init_noise / init_params_by_noise first")
            if float(det.fs) != float(extractor.fs):
                raise ValueError("the VAD was initialised at %g Hz, the extractor works at %g Hz" % (det.fs, extractor.fs))
            lam0, lam1 = vad_thresholds(det.lambda0, det.lambda1)
            na = np.ascontiguousarray(det.noise_amp, dtype=np.float32)
            full = isinstance(models, FullSet)
            flags = (_lib.SR_STREAM_GRAPH if graph else 0) | (_lib.SR_CLAMP_COMPAT if clamp_compat and not full else 0)
            h = lib().sr_stream_create_vad(extractor._h, None if full else models._h, models._h if full else None, self.n_windows,
                                           self.window_samples, int(nd), flags, int(det.window_size), int(det.order), _lib.as_fp(na),
                                           lam0, lam1)
            what = "sr_stream_create_vad"
        elif isinstance(models, FullSet):
            h = lib().sr_stream_create_full(extractor._h, models._h, self.n_windows, self.window_samples, int(nd),
                                            _lib.SR_STREAM_GRAPH if graph else 0)
            what = "sr_stream_create_full"
        elif isinstance(models, ModelSet):
            h = lib().sr_stream_create(extractor._h, models._h, self.n_windows, self.window_samples, int(nd),
                                       (_lib.SR_CLAMP_COMPAT if clamp_compat else 0) | (_lib.SR_STREAM_GRAPH if graph else 0))
            what = "sr_stream_create"
        else:
            raise TypeError("models must be a core.ModelSet or an skgmm.FullSet (got %s)" % type(models).__name__)
        if not h:
            raise SRError("%s failed: %s" % (what, _lib.last_error()))
        self._h = C.c_void_p(h)
        self.open_set = None
        if open_set is not None:
            bg, threshold = open_set
            check(lib().sr_stream_set_open(self._h, int(bg), float(threshold)), "sr_stream_set_open")
            self.open_set = (int(bg), float(threshold))

    def submit(self, pcm) -> None:
        a = np.ascontiguousarray(pcm, dtype=np.int16)
        if a.size != self.n_windows * self.window_samples:
            raise ValueError("expected %d x %d samples" % (self.n_windows, self.window_samples))
        check(lib().sr_stream_submit(self._h, a.ctypes.data_as(C.POINTER(C.c_int16))), "sr_stream_submit")

    def collect(self):
        sums = np.empty((self.n_windows, self.n_models), dtype=np.float64)
        arg = np.empty(self.n_windows, dtype=np.int32)
        ms = C.c_double(0)
        if self.vad:
            voiced = np.empty(self.n_windows, dtype=np.int32)
            check(lib().sr_stream_collect_vad(self._h, _lib.as_dp(sums), _lib.as_i32p(arg), _lib.as_i32p(voiced), C.byref(ms)),
                  "sr_stream_collect_vad")
            self.last_voiced = voiced
        else:
            check(lib().sr_stream_collect(self._h, _lib.as_dp(sums), _lib.as_i32p(arg), C.byref(ms)), "sr_stream_collect")
        return sums, arg, ms.value

    def collect_vad(self):
        """``collect`` of a session with ``vad=``: (sums, argmax, voiced samples per window, device ms)."""
        if not self.vad:
            raise SRError("not a voice-activity session: create the stream with vad=")
        sums, arg, ms = self.collect()
        return sums, arg, self.last_voiced, ms

    def collect_open(self):
        """The oldest tick of a session with ``open_set=``: (sums, labels int32, margins float64, device ms).  A window a
        voice-activity session did not score has label -1 and margin NaN; its voiced counts are in ``last_voiced``."""
        sums = np.empty((self.n_windows, self.n_models), dtype=np.float64)
        labels = np.empty(self.n_windows, dtype=np.int32)
        margins = np.empty(self.n_windows, dtype=np.float64)
        voiced = np.empty(self.n_windows, dtype=np.int32) if self.vad else None
        ms = C.c_double(0)
        check(lib().sr_stream_collect_open(self._h, _lib.as_dp(sums), _lib.as_i32p(labels), _lib.as_dp(margins),
                                           _lib.as_i32p(voiced) if self.vad else None, C.byref(ms)), "sr_stream_collect_open")
        if self.vad:
            self.last_voiced = voiced
        return sums, labels, margins, ms.value

    def __del__(self):
        try:
            if self._h:
                lib().sr_stream_free(self._h)
                self._h = None
        except Exception:
            pass


class MultiPredictor:
    """Every GPU of the node from one process: utterances are dealt to ``n_slots`` slots by length
    (slot i on device i % device_count), each slot has its own replica of the models and a host thread
    that runs MFCC -> CMVN/deltas -> all models -> sums + argmax on its GPU; rows are gathered on the
    host (``sr_multi_*``; the reference: Threadpool in gmm.cc:533-560, Pool in test-gmm.py:128-133)."""

    def __init__(self, gmms, fs, n_slots=0, win_length_ms=32, win_shift_ms=16, FFT_SIZE=2048, n_filters=50,
                 n_ceps=13, pre_emphasis_coef=0.95):
        self._keep = list(gmms)
        arr = (C.c_void_p * len(self._keep))(*[g.gmm for g in self._keep])
        h = lib().sr_multi_create(arr, len(self._keep), float(fs), float(win_length_ms), float(win_shift_ms),
                                  int(FFT_SIZE), int(n_filters), int(n_ceps), float(pre_emphasis_coef), int(n_slots))
        if not h:
            raise SRError("sr_multi_create failed: %s" % _lib.last_error())
        self._h = C.c_void_p(h)
        self.n_models = len(self._keep)
        self.slot_seconds = None

    @classmethod
    def from_full(cls, gmms, fs, n_slots=0, n_lpc=15, win_length_ms=32, win_shift_ms=16, FFT_SIZE=2048, n_filters=50,
                  n_ceps=13, pre_emphasis_coef=0.95) -> "MultiPredictor":
        """The same predictor over full-covariance models (``skgmm.GMM``): every slot packs its own ``FullSet`` replica, and
        its features are the MFCC + LPC-``n_lpc`` columns (mix_feature; ``nd`` must be 0 then) or, with ``n_lpc=0``, the MFCC
        with ``nd`` orders of deltas.  Results are ``FullSet.predict_pcm``'s, bit for bit, for any slot count; an utterance
        without frames gets argmax -1.  ``clamp_compat`` does not apply."""
        self = cls.__new__(cls)
        self._h = None
        self._keep = list(gmms)
        arr = (C.c_void_p * len(self._keep))(*[g.handle().value for g in self._keep])
        h = lib().sr_multi_create_full(arr, len(self._keep), float(fs), float(win_length_ms), float(win_shift_ms), int(FFT_SIZE),
                                       int(n_filters), int(n_ceps), float(pre_emphasis_coef), int(n_lpc), int(n_slots))
        if not h:
            raise SRError("sr_multi_create_full failed: %s" % _lib.last_error())
        self._h = C.c_void_p(h)
        self.n_models = len(self._keep)
        self.slot_seconds = None
        return self

    @property
    def n_slots(self) -> int:
        return lib().sr_multi_slots(self._h)

    def slot_devices(self):
        return [lib().sr_multi_slot_device(self._h, i) for i in range(self.n_slots)]

    def slot_numa_nodes(self):
        """NUMA node every slot's host thread pinned itself to in the last call (-1: the platform does not say)."""
        return [lib().sr_multi_slot_numa_node(self._h, i) for i in range(self.n_slots)]

    def slot_pieces(self):
        """Pieces every slot cut its utterances into in the last call (0: the slot took no work)."""
        return [lib().sr_multi_slot_pieces(self._h, i) for i in range(self.n_slots)]

    def predict(self, signals, nd=0, clamp_compat=True):
        """``signals``: list of int16 arrays.  -> (sums[U, S], argmax[U])."""
        sigs = [np.ascontiguousarray(s, dtype=np.int16) for s in signals]
        offsets = np.zeros(len(sigs) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([len(s) for s in sigs])
        cat = np.ascontiguousarray(np.concatenate(sigs)) if sigs else np.zeros(0, np.int16)
        return self.predict_concat(cat, offsets, nd, clamp_compat)

    def predict_concat(self, cat, offsets, nd=0, clamp_compat=True):
        U = len(offsets) - 1
        sums = np.zeros((U, self.n_models), dtype=np.float64)
        arg = np.full(U, -1, dtype=np.int32)
        secs = np.zeros(self.n_slots, dtype=np.float64)
        check(lib().sr_multi_predict_pcm(self._h, cat.ctypes.data_as(C.POINTER(C.c_int16)), _lib.as_i64p(offsets), U,
                                         int(nd), _lib.as_dp(sums), _lib.as_i32p(arg), _lib.as_dp(secs),
                                         _lib.SR_CLAMP_COMPAT if clamp_compat else 0), "sr_multi_predict_pcm")
        self.slot_seconds = secs
        return sums, arg

    def predict_open(self, signals, bg, threshold, nd=0, clamp_compat=True):
        """``predict`` with the open-set decision of ``ModelSet.score_open``, every slot deciding its utterances on its own
        device (sr_multi_predict_pcm_open).  -> (sums[U, S], labels[U] int32, margins[U] float64)."""
        sigs = [np.ascontiguousarray(s, dtype=np.int16) for s in signals]
        offsets = np.zeros(len(sigs) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([len(s) for s in sigs])
        cat = np.ascontiguousarray(np.concatenate(sigs)) if sigs else np.zeros(0, np.int16)
        U = len(sigs)
        sums = np.zeros((U, self.n_models), dtype=np.float64)
        labels = np.full(U, -1, dtype=np.int32)
        margins = np.full(U, np.nan, dtype=np.float64)
        secs = np.zeros(self.n_slots, dtype=np.float64)
        check(lib().sr_multi_predict_pcm_open(self._h, cat.ctypes.data_as(C.POINTER(C.c_int16)), _lib.as_i64p(offsets), U, int(nd),
                                              int(bg), float(threshold), _lib.as_dp(sums), _lib.as_i32p(labels), _lib.as_dp(margins),
                                              _lib.as_dp(secs), _lib.SR_CLAMP_COMPAT if clamp_compat else 0),
              "sr_multi_predict_pcm_open")
        self.slot_seconds = secs
        return sums, labels, margins

    def __del__(self):
        try:
            if self._h:
                lib().sr_multi_free(self._h)
                self._h = None
        except Exception:
            pass
