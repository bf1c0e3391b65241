"""Model facade -- mirrors the reference's ``src/gui/interface.py`` (ModelInterface :26-109):
enroll / train / predict / dump / load with the same meaning.  The speaker set is the
device-backed ``GMMSetPyGMM`` (the reference's C++ back-end, interface.py:19-23,63-75, is the
drop-in boundary of this repo; its scikit-learn default is third-party code).

Extensions (all keyword-only, defaults = the reference's behaviour): ``gmm_order``,
``feature_kwargs`` (forwarded to the extractor), ``lpc`` (False: MFCC half of mix_feature only),
``diff``/``nd`` (append deltas to the MFCC half; excludes the LPC columns),
``gmm_kwargs`` (forwarded to ``pygmm.GMM``), ``ubm`` (MAP-adapt speakers from a UBM),
``covariance_type`` ('diag', the default: the C++ back-end's diagonal models; 'full': the reference CLI's own speaker model,
scikit-learn's full-covariance ``GaussianMixture``, as ``skgmm.GMMSet`` -- ``UBM_MODEL_FILE`` is then ignored, as the reference
ignores it when its set is not ``GMMSetPyGMM``, interface.py:63-75; ``gmm_kwargs`` go to ``skgmm.GMM``, a ``seed`` among them
becoming its ``random_state``, -1 = the library's default).
``remove_silence`` (False; True: the reference's defaults; or a dict of ``frame_duration`` / ``frame_shift`` / ``perc``): the
energy-threshold silence removal of the reference's corpus preparation (``filters.silence``, on the device) in front of the
feature stage of ``enroll`` and every ``predict*`` -- the setting is stored with the model; int16, int8 or uint8 audio.  A signal
it leaves too short for a frame gives None from ``predict*`` and raises from ``enroll``, as a short raw signal does.  With it,
``predict_many(gpus != 1)`` takes the one-GPU path.
``feature_norm`` (None; "warp", "cmn", "cmvn", or a dict of ``mode`` / ``window``): short-time feature normalisation
(``feature.norm``, on the device: feature warping or sliding-window CMN / CMVN over ``window`` = 301 frames) of whatever
``mix_feature`` returns, in ``enroll`` and every ``predict*`` -- the setting is stored with the model.  With it,
``predict_many(gpus != 1)`` takes the one-GPU path.
VAD (``init_noise`` / ``filter``) is the LTSD detector of ``filters`` (third-party pyssp in the
reference: restated, parity unpinned).
"""
from __future__ import annotations

import pickle
import sys
import time
import traceback as tb
from collections import defaultdict

import numpy as np

from .feature import mix_feature
from .gmmset import GMMSetPyGMM as GMMSet
from .pygmm import GMM


class ModelInterface(object):

    UBM_MODEL_FILE = None

    def __init__(self, *, gmm_order=32, feature_kwargs=None, diff=False, nd=1, lpc=True, gmm_kwargs=None,
                 verbose=True, covariance_type="diag", remove_silence=False, feature_norm=None):
        if covariance_type not in ("diag", "full"):
            raise ValueError("covariance_type must be 'diag' or 'full' (got %r)" % (covariance_type,))
        self.covariance_type = covariance_type
        self.remove_silence = remove_silence
        self._silence_kwargs()          # (a bad value fails here, not at the first recording)
        self.feature_norm = feature_norm
        self._norm_setting()
        self.features = defaultdict(list)
        self.gmm_order = gmm_order
        self.feature_kwargs = dict(feature_kwargs or {})
        self.diff, self.nd, self.lpc = diff, nd, lpc
        self.gmm_kwargs = dict(gmm_kwargs or {})
        self.verbose = verbose
        self.gmmset = self._new_full_set() if covariance_type == "full" else GMMSet(gmm_order=gmm_order, **self.gmm_kwargs)

    def _new_full_set(self):
        from . import skgmm
        kw = dict(self.gmm_kwargs)
        if "seed" in kw:
            seed = kw.pop("seed")
            kw["random_state"] = None if seed is None or seed < 0 else int(seed)
        return skgmm.GMMSet(gmm_order=self.gmm_order, **kw)

    def init_noise(self, fs, signal):
        """init vad from environment noise (gui/interface.py:37-41)"""
        from .filters import VAD
        if getattr(self, "vad", None) is None:
            self.vad = VAD()
        self.vad.init_noise(fs, signal)

    def filter(self, fs, signal):
        """use VAD to filter out the silent part of a signal; empty if less than a third of it is
        voiced (gui/interface.py:43-53)"""
        if getattr(self, "vad", None) is None:
            raise RuntimeError("NoiseFilter Not Initialized")
        ret, intervals = self.vad.filter(fs, signal)
        if len(ret) > len(signal) / 3:
            return ret
        return np.array([])

    def _silence_kwargs(self):
        """None when silence removal is off (also for a model pickled before the setting existed), else its parameters."""
        rs = getattr(self, "remove_silence", False)
        if rs is False or rs is None:
            return None
        if rs is True:
            return {}
        if isinstance(rs, dict) and set(rs) <= {"frame_duration", "frame_shift", "perc"}:
            return dict(rs)
        raise ValueError("remove_silence must be False, True or a dict of frame_duration / frame_shift / perc (got %r)" % (rs,))

    def _norm_setting(self):
        """None when feature normalisation is off (also for a model pickled before the setting existed), else (mode, window)."""
        fn = getattr(self, "feature_norm", None)
        if fn is None:
            return None
        from .feature.norm import check_setting
        if isinstance(fn, str):
            return check_setting(fn)
        if isinstance(fn, dict) and "mode" in fn and set(fn) <= {"mode", "window"}:
            return check_setting(fn["mode"], fn.get("window", 301))
        raise ValueError("feature_norm must be None, 'warp', 'cmn', 'cmvn' or a dict of mode / window (got %r)" % (fn,))

    def _desilenced(self, items):
        """[(fs, signal), ...] as they reach the feature stage: unchanged, or through ``filters.silence`` -- one device call
        per sampling rate."""
        kw = self._silence_kwargs()
        items = list(items)
        if kw is None or not items:
            return items
        from .filters.silence import remove_silence_many
        out = [None] * len(items)
        for rate in sorted({fs for fs, _ in items}):
            idx = [i for i, (fs, _) in enumerate(items) if fs == rate]
            for i, sig in zip(idx, remove_silence_many(rate, [items[i][1] for i in idx], **kw)):
                out[i] = (rate, sig)
        return out

    def _features(self, fs, signal):
        fs, signal = self._desilenced([(fs, signal)])[0]
        return self._features_of(fs, signal)

    def _features_of(self, fs, signal):
        feat = mix_feature((fs, signal), lpc=self.lpc, diff=self.diff, nd=self.nd, **self.feature_kwargs)
        setting = self._norm_setting()
        if setting is None:
            return feat
        from .feature.norm import normalise_many
        return normalise_many([feat], *setting)[0].astype(np.float64)

    def _features_many(self, items):
        """The feature matrices of [(fs, signal), ...] behind the silence removal; a signal it leaves too short for a frame
        gives None in its place (``predict`` answers None there too)."""
        feats = []
        for fs, sig in self._desilenced(items):
            try:
                feats.append(self._features_of(fs, sig))
            except Exception:
                print(tb.format_exc(), file=sys.stderr)
                feats.append(None)
        return feats

    @staticmethod
    def _spread(feats, predict):
        """``predict`` over the matrices that exist, None where there is none"""
        have = [f for f in feats if f is not None]
        labels = iter(predict(have) if have else [])
        return [None if f is None else next(labels) for f in feats]

    def enroll(self, name, fs, signal):
        """add the signal to this person's training dataset"""
        feat = self._features(fs, signal)
        self.features[name].extend(feat)

    def _get_gmm_set(self):
        import os
        if getattr(self, "covariance_type", "diag") == "full":
            return self._new_full_set()
        if self.UBM_MODEL_FILE and os.path.isfile(self.UBM_MODEL_FILE):
            return GMMSet(ubm=GMM.load(self.UBM_MODEL_FILE), **self.gmm_kwargs)
        return GMMSet(gmm_order=self.gmm_order, **self.gmm_kwargs)

    def train(self):
        self.gmmset = self._get_gmm_set()
        start = time.time()
        if self.verbose:
            print("Start training...")
        # every speaker in one batched device fit -- full covariance: sr_fullgmm_fit_batch; diagonal with a UBM: sr_map_fit_batch
        # (without one GMMSet.fit_many is the loop of fit_new) -- the models of a loop of fit_new, bit for bit
        self.gmmset.fit_many([np.asarray(feats) for feats in self.features.values()], list(self.features.keys()))
        if self.verbose:
            print(time.time() - start, " seconds")

    def predict(self, fs, signal, reject_threshold=None, top_c=None):
        """return a label (name).  Extension: ``reject_threshold`` (a number) takes the open-set decision instead -- None when
        the best speaker's per-frame margin over the UBM is below it (``GMMSet.predict_with_reject_batch``: decided on the
        device); only a model enrolled from a UBM can.  ``top_c`` (an integer; default off): score through top-C Gaussian
        selection against the UBM (``GMMSet.predict(top_c=)``: an approximation, far less work per frame for large sets); only a
        model enrolled from a UBM can."""
        if top_c is not None:
            return self.predict_many_topc([(fs, signal)], top_c, reject_threshold)[0]
        if reject_threshold is not None:
            self._check_reject()
        try:
            feat = self._features(fs, signal)
        except Exception:
            print(tb.format_exc(), file=sys.stderr)
            return None
        if reject_threshold is None:
            return self.gmmset.predict_one(feat)
        return self.gmmset.predict_with_reject_batch([feat], threshold=float(reject_threshold))[0]

    def _check_reject(self):
        if getattr(self, "covariance_type", "diag") == "full" or getattr(self.gmmset, "ubm", None) is None:
            raise ValueError("a reject threshold needs a model enrolled from a UBM (ModelInterface.UBM_MODEL_FILE at training "
                             "time, diagonal models): this one has none")

    def _check_topc(self):
        if getattr(self, "covariance_type", "diag") == "full":
            raise ValueError("top-C Gaussian selection is for diagonal models enrolled from a UBM: this model is full-covariance")
        if getattr(self.gmmset, "ubm", None) is None:
            raise ValueError("top-C Gaussian selection needs a model enrolled from a UBM (ModelInterface.UBM_MODEL_FILE at training "
                             "time): this one has none")

    def predict_many_topc(self, items, top_c, reject_threshold=None):
        """Extension: [(fs, signal), ...] -> labels, every utterance scored in ONE batch through top-C Gaussian selection against
        the UBM (``GMMSet.predict(top_c=)``); with ``reject_threshold`` the open-set rule decides on those sums."""
        self._check_topc()
        if int(top_c) < 1:
            raise ValueError("top_c must be >= 1 (got %r)" % (top_c,))
        if reject_threshold is not None:
            run = lambda f: self.gmmset.predict_with_reject_batch(f, threshold=float(reject_threshold), top_c=int(top_c))  # noqa: E731
        else:
            run = lambda f: self.gmmset.predict(f, top_c=int(top_c))  # noqa: E731
        if self._silence_kwargs() is not None:
            return self._spread(self._features_many(list(items)), run)
        return run([self._features(fs, sig) for fs, sig in items])

    def predict_many_with_reject(self, items, reject_threshold):
        """Extension: [(fs, signal), ...] -> labels by the open-set decision of ``predict(reject_threshold=)``, every utterance
        scored and decided in ONE batch on one GPU (``GMMSet.predict_with_reject_batch``)."""
        self._check_reject()
        if self._silence_kwargs() is not None:
            return self._spread(self._features_many(list(items)),
                                lambda f: self.gmmset.predict_with_reject_batch(f, threshold=float(reject_threshold)))
        feats = [self._features(fs, sig) for fs, sig in items]
        return self.gmmset.predict_with_reject_batch(feats, threshold=float(reject_threshold))

    def predict_many(self, items, gpus=1):
        """Extension: [(fs, signal), ...] -> labels, every utterance scored in one batch.  ``gpus`` != 1
        (0 = every visible GPU) shards the utterances over the GPUs of the node from this one process
        (core.MultiPredictor: a host thread and a model replica per GPU, no collective) -- for diagonal models on the
        MFCC-only feature (``lpc=False``), and for full-covariance models on either feature (``MultiPredictor.from_full``),
        on int16 audio of one sampling rate; anything else takes the one-GPU path.
        One difference on the sharded full-covariance route: an utterance of 5 frames' length or less, which the one-GPU path
        refuses ("Signal too short!"), is scored when it yields at least one frame and gets ``None`` when it yields none (as on
        the diagonal sharded route)."""
        items = list(items)
        if self._silence_kwargs() is not None or self._norm_setting() is not None:
            gpus = 1                # (neither is part of the sharded route: its slots upload raw PCM and extract for themselves)
        rates = {fs for fs, _ in items}
        full = getattr(self, "covariance_type", "diag") == "full"
        pcm_ok = len(rates) == 1 and items and all(np.asarray(sig).dtype == np.int16 and np.asarray(sig).ndim == 1 for _, sig in items)
        if gpus != 1 and full and pcm_ok:
            from .core import MultiPredictor
            kw = dict(self.feature_kwargs)
            order = kw.pop("n_lpc", 15)
            fs = rates.pop()
            # mix_feature's columns: MFCC + LPC-15 when lpc and not diff, else the MFCC with deltas when diff (feature/__init__.py)
            n_lpc = order if self.lpc and not self.diff else 0
            nd = self.nd if self.diff else 0
            key = ("full", tuple((id(g), g._version) for g in self.gmmset.gmms), fs, int(gpus), n_lpc, tuple(sorted(kw.items())))
            cached = getattr(self, "_multi", None)
            if cached is None or cached[0] != key:
                cached = self._multi = (key, MultiPredictor.from_full(self.gmmset.gmms, fs, n_slots=int(gpus), n_lpc=n_lpc, **kw))
            _, winners = cached[1].predict([sig for _, sig in items], nd=nd)
            return [None if w < 0 else self.gmmset.y[w] for w in winners]
        if gpus != 1 and not full and not self.lpc and pcm_ok:
            from .core import MultiPredictor
            kw = dict(self.feature_kwargs)
            fs = rates.pop()
            # the per-GPU model replicas are packed and uploaded once and kept until the model set changes (re-training
            # replaces the GMM objects), not rebuilt on every call
            key = (tuple(id(g) for g in self.gmmset.gmms), fs, int(gpus), tuple(sorted(kw.items())))
            cached = getattr(self, "_multi", None)
            if cached is None or cached[0] != key:
                cached = self._multi = (key, MultiPredictor(self.gmmset.gmms, fs, n_slots=int(gpus), **kw))
            mp = cached[1]
            _, winners = mp.predict([sig for _, sig in items], nd=self.nd if self.diff else 0)
            return [None if w < 0 else self.gmmset.y[w] for w in winners]
        if self._silence_kwargs() is not None:
            return self._spread(self._features_many(items), self.gmmset.predict)
        feats = [self._features(fs, sig) for fs, sig in items]
        return self.gmmset.predict(feats)

    def _timeline_frames(self, window_s, hop_s, min_duration_s):
        """(frame shift in seconds, window, hop in frames, minimum turn in windows) of a timeline call."""
        shift = float(self.feature_kwargs.get("win_shift_ms", 16)) / 1000.0
        for name, v in (("window_s", window_s), ("hop_s", hop_s)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not v > 0:
                raise ValueError("%s must be a positive number of seconds (got %r)" % (name, v))
        W, H = max(1, int(round(window_s / shift))), max(1, int(round(hop_s / shift)))
        if min_duration_s is None:
            return shift, W, H, 1
        if isinstance(min_duration_s, bool) or not isinstance(min_duration_s, (int, float)) or not min_duration_s >= 0:
            raise ValueError("min_duration_s must be a number of seconds >= 0 (got %r)" % (min_duration_s,))
        m = max(1, int(np.ceil(min_duration_s / (H * shift) - 1e-9)))
        if m > 16:
            raise ValueError("min_duration_s = %r is %d hops of %g s: the decode holds a turn for at most 16 windows (use a longer hop)"
                             % (min_duration_s, m, H * shift))
        return shift, W, H, m

    def timeline(self, fs, signal, window_s=1.5, hop_s=0.4, smooth="hold", switch_penalty=None, min_duration_s=None,
                 reject_threshold=None):
        """Extension: who speaks when in a recording -> ``[(start_s, end_s, name or None)]``, intervals that tile
        [0, duration of the features] without gaps.  The features are extracted once for the whole recording (``feature_norm``
        is honoured; silence removal is not applied: it would change the time axis), scored once, and the per-frame values are
        summed over windows of ``window_s`` every ``hop_s`` on the device (``core.ModelSet.timeline``).  ``smooth``: "none",
        "hold" (the reference GUI's rule, gui.py:195-204) or "viterbi" (needs ``switch_penalty``; ``min_duration_s`` is the
        shortest turn).  ``reject_threshold`` (a number): the model's UBM becomes the "nobody" state, whose windows come back
        with the name None; only a model enrolled from a UBM can.  Unlike the GUI's loop the windows are not extracted and
        voice-activity-filtered one by one."""
        from .core import _timeline_args
        shift, W, H, m = self._timeline_frames(window_s, hop_s, min_duration_s)
        _timeline_args(W, H, None, 0.0, smooth, switch_penalty, m)
        if reject_threshold is not None:
            self._check_reject()
        return self._timeline_of(np.asarray(self._features_of(fs, signal)), shift, W, H, m, smooth, switch_penalty, reject_threshold)

    def _timeline_of(self, feat, shift, W, H, m, smooth, switch_penalty, reject_threshold):
        """``timeline`` on the recording's feature matrix, its arguments checked and in frames."""
        from . import timeline as tl
        from .core import Batch
        full = getattr(self, "covariance_type", "diag") == "full"
        batch = Batch.from_features([feat])
        kw = dict(smooth=smooth, switch_penalty=switch_penalty, min_windows=m)
        if full:
            labels = self.gmmset._full_set().timeline(batch, W, H, **kw)[0]
            names = list(self.gmmset.y)
        elif reject_threshold is not None:
            labels = self.gmmset._open_model_set().timeline(batch, W, H, bg=0, threshold=float(reject_threshold), **kw)[0]
            names = [None] + list(self.gmmset.y)
        else:
            labels = self.gmmset._model_set().timeline(batch, W, H, **kw)[0]
            names = list(self.gmmset.y)
        return [(a, b, None if lab < 0 else names[lab]) for a, b, lab in tl.segments(labels, len(feat), W, H, shift)]

    def _diarize_args(self, segment_s, change, penalty, n_speakers, max_speakers, gmm_order):
        """(frame shift in seconds, frames per base segment, k_min, k_max) of a diarize call, its arguments checked."""
        from . import _lib
        shift = float(self.feature_kwargs.get("win_shift_ms", 16)) / 1000.0
        if isinstance(segment_s, bool) or not isinstance(segment_s, (int, float)) or not segment_s > 0:
            raise ValueError("segment_s must be a positive number of seconds (got %r)" % (segment_s,))
        if _lib.diar_change_mode(change) < 0:
            raise ValueError("change must be 'bic' or 'uniform' (got %r)" % (change,))
        if isinstance(penalty, bool) or not isinstance(penalty, (int, float)) or not penalty > 0 or not np.isfinite(penalty):
            raise ValueError("penalty must be a finite number > 0 (got %r)" % (penalty,))
        for name, v in (("n_speakers", n_speakers), ("max_speakers", max_speakers)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1):
                raise ValueError("%s must be None or an integer >= 1 (got %r)" % (name, v))
        if n_speakers is not None and max_speakers is not None:
            raise ValueError("give n_speakers (exactly that many) or max_speakers (at most that many), not both")
        if isinstance(gmm_order, bool) or not isinstance(gmm_order, (int, np.integer)) or gmm_order < 1:
            raise ValueError("gmm_order must be an integer >= 1 (got %r)" % (gmm_order,))
        L = max(1, int(round(segment_s / shift)))
        if n_speakers is not None:
            return shift, L, int(n_speakers), int(n_speakers)
        return shift, L, 1, 0 if max_speakers is None else int(max_speakers)

    def diarize(self, fs, signal, segment_s=1.0, change="bic", penalty=1.0, n_speakers=None, max_speakers=None, resegment=True,
                gmm_order=8, **timeline_kw):
        """Extension: who speaks when in a recording with nobody enrolled -> ``[(start_s, end_s, "spk0"), ...]``, intervals that
        tile [0, duration of the features] without gaps.  The features are extracted as ``timeline`` extracts them and clustered
        on the device (``core.Batch.diarize``: base segments of ``segment_s``, BIC change detection or ``change="uniform"``,
        agglomerative clustering under delta-BIC with weight ``penalty``; ``n_speakers`` forces that many clusters,
        ``max_speakers`` caps them).  With ``resegment`` one model of ``gmm_order`` mixtures per cluster is fitted on that cluster's
        frames by the batched fit of this interface's ``covariance_type``, and ``timeline(smooth="viterbi")`` decodes the
        recording over those models (``timeline_kw``: window_s, hop_s, switch_penalty -- 5.0 here, not tuned on data --,
        min_duration_s).  A recording that ends with one cluster skips the resegmentation.  Speakers are named by first
        appearance: spk0, spk1, ..."""
        from . import diarize as dz
        from .core import Batch, _timeline_args
        shift, L, k_min, k_max = self._diarize_args(segment_s, change, penalty, n_speakers, max_speakers, gmm_order)
        kw = dict(dict(window_s=1.5, hop_s=0.4, switch_penalty=5.0, min_duration_s=None), **timeline_kw)
        if set(kw) - {"window_s", "hop_s", "switch_penalty", "min_duration_s"}:
            raise ValueError("diarize passes window_s, hop_s, switch_penalty and min_duration_s on to timeline (got %r)" % sorted(timeline_kw))
        _, W, H, m = self._timeline_frames(kw["window_s"], kw["hop_s"], kw["min_duration_s"])
        _timeline_args(W, H, None, 0.0, "viterbi", kw["switch_penalty"], m)
        feat = np.asarray(self._features_of(fs, signal))
        res = Batch.from_features([feat]).diarize(L=L, change=change, penalty=float(penalty), k_min=k_min, k_max=k_max)[0]
        labels, ranges = res["labels"], dz.frame_ranges(res["init_off"], len(feat), L)
        if not resegment or res["n_clusters"] <= 1:
            return [(a, b, "spk%d" % lab) for a, b, lab in dz.frame_segments(res["init_off"], labels, len(feat), L, shift)]
        sub = self._cluster_models(feat, labels, ranges, res["n_clusters"], gmm_order)
        return sub._timeline_of(feat, shift, W, H, m, "viterbi", kw["switch_penalty"], None)

    def _cluster_models(self, feat, labels, ranges, n_clusters, gmm_order):
        """An interface of this one's settings whose speakers are the clusters: one model per cluster, fitted on its frames by the
        batched fit (the features make the round trip through the host that ``train`` makes)."""
        sub = ModelInterface(gmm_order=int(gmm_order), feature_kwargs=self.feature_kwargs, diff=self.diff, nd=self.nd, lpc=self.lpc,
                             gmm_kwargs=self.gmm_kwargs, verbose=False, covariance_type=getattr(self, "covariance_type", "diag"),
                             feature_norm=getattr(self, "feature_norm", None))
        sub.UBM_MODEL_FILE = None
        for c in range(int(n_clusters)):
            rows = np.concatenate([feat[a:b] for (a, b), lab in zip(ranges.tolist(), labels) if lab == c], axis=0)
            if len(rows) < int(gmm_order):
                raise ValueError("cluster spk%d holds %d frames, fewer than gmm_order = %d mixtures: lower gmm_order, or raise penalty / "
                                 "lower max_speakers so that small clusters merge" % (c, len(rows), gmm_order))
            sub.features["spk%d" % c] = list(rows)
        sub.train()
        return sub

    def dump(self, fname):
        """ dump all models to file"""
        self.gmmset.before_pickle()
        multi, self._multi = getattr(self, "_multi", None), None        # (device handles do not pickle)
        try:
            with open(fname, "wb") as f:
                pickle.dump(self, f, -1)
        finally:
            self._multi = multi
            self.gmmset.after_pickle()

    @staticmethod
    def load(fname):
        """ load from a dumped model file"""
        with open(fname, "rb") as f:
            R = pickle.load(f)
            R.gmmset.after_pickle()
            return R
