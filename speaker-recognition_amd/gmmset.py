"""Speaker set -- API mirror of the reference's ``src/testbench/gmmset.py`` (``GMMSet`` :15-91,
``GMMSetPyGMM`` :94-105): one GMM per label, prediction = arg max over speakers of the summed
per-frame log-likelihood, optional open-set rejection against a UBM.  Same method names, arguments
and results; the implementation is this package's.

The reference scores speaker by speaker through the ABI (gmmset.py:59-64, :95-99).  Here every
speaker model sits in one device-resident ``ModelSet`` and an utterance -- or a whole list of them
-- is scored against all of them in ONE fused launch: each frame tile leaves HBM once.
"""
from __future__ import annotations

import ctypes as C
import threading
from collections import OrderedDict

import numpy as np

from . import _lib
from .core import Batch, ModelSet
from .pygmm import GMM


class GMMSet(object):
    def __init__(self, gmm_order=32, ubm=None, reject_threshold=10, **kwargs):
        self.ubm, self.reject_threshold, self.kwargs = ubm, reject_threshold, kwargs
        # speakers adapted from a UBM inherit its size (gmmset.py:24-27)
        self.gmm_order = gmm_order if ubm is None else ubm.get_nr_mixtures()
        self.gmms, self.y = [], []
        self._set = None
        self._set_key = None            # packed device copy of self.gmms, rebuilt when the list changes
        self._open_set = None
        self._open_set_key = None       # the same with the UBM in front (column 0): the batched open-set decision's set

    # ---- enrolment ----
    def _append(self, label, gmm):
        self.gmms.append(gmm)
        self.y.append(label)
        self._set = None
        self._open_set = None

    def fit_new(self, x, label):
        """Train one model on the frames ``x`` (EM, or MAP adaptation when a UBM was given)."""
        model = GMM(self.gmm_order, **self.kwargs)
        model.fit(x, self.ubm)
        self._append(label, model)

    def cluster_by_label(self, X, y):
        """Pool the frame lists of equal labels -> (tuple of frame lists, tuple of labels)."""
        pooled = OrderedDict()
        for frames, label in zip(X, y):
            pooled.setdefault(label, []).extend(frames)
        return tuple(pooled.values()), tuple(pooled.keys())

    def auto_tune_parameter(self, X, y):
        return None                  # unimplemented in the reference as well (gmmset.py:44-47)

    def fit_many(self, xs, labels):
        """Train one model per matrix ``xs[s]`` and append them under ``labels[s]``, in order: with a UBM every speaker in ONE
        batched device fit (``sr_map_fit_batch``, csrc/map_batch.hip) -- the models and iteration counts of a loop of ``fit_new``,
        bit for bit; without one, or in a process that lost its GPU runtime to fork(), that loop.  As in the loop, the speakers
        before the first failing one are appended and its error is raised."""
        xs, labels = list(xs), list(labels)
        if len(xs) != len(labels):
            raise ValueError("fit_many: %d matrices but %d labels" % (len(xs), len(labels)))
        if not xs:
            return
        if self.ubm is None or _lib.gpu_runtime_lost():
            for x, label in zip(xs, labels):
                self.fit_new(x, label)
            return
        dim = self.ubm.get_dim()
        mats, refused = [], None
        for x in xs:                          # (what the loop would refuse at speaker s is raised after the speakers before it)
            try:
                X = _lib.f32_matrix(x)
                if X.shape[0] > 0 and X.shape[1] != dim:
                    raise _lib.SRError("train failed: UBM dim %d != data dim %d" % (dim, X.shape[1]))
            except (ValueError, _lib.SRError) as e:
                refused = e
                break
            mats.append(X)
        if not mats:
            raise refused
        S = len(mats)
        models = [GMM(self.gmm_order, **self.kwargs) for _ in range(S)]
        off = np.zeros(S + 1, dtype=np.int64)
        np.cumsum([X.shape[0] for X in mats], out=off[1:])
        have = [X for X in mats if X.shape[0] > 0]
        Xall = np.ascontiguousarray(np.concatenate(have, axis=0)) if have else np.zeros((1, dim), np.float32)
        p = models[0]._gen_param(Xall)
        handles = (C.c_void_p * S)(*[m.gmm.value for m in models])
        iters = np.zeros(S, dtype=np.int32)
        status = np.zeros(S, dtype=np.int32)
        rc = _lib.lib().sr_map_fit_batch(handles, S, self.ubm.gmm, _lib.as_fp(Xall), _lib.as_i64p(off), dim, C.byref(p), int(models[0].seed),
                                         _lib.as_i32p(iters), _lib.as_i32p(status))
        _lib.check(rc, "sr_map_fit_batch")
        for s, (model, label) in enumerate(zip(models, labels)):
            if status[s] < 0:
                raise _lib.SRError("train failed: %s" % _lib.lib().sr_map_fit_batch_error(s).decode("utf-8", "replace"))
            model.nr_mixture = _lib.lib().get_nr_mixtures(model.gmm)
            model._version = getattr(model, "_version", 0) + 1      # as GMM.fit: invalidates packed copies (_model_set)
            self._append(label, model)
        if refused is not None:
            raise refused

    def fit(self, X, y):
        frames, labels = self.cluster_by_label(X, y)
        self.fit_many(frames, labels)
        self.auto_tune_parameter(frames, labels)

    def load_gmm(self, label, fname):
        model = GMM.load(fname)
        for name, value in self.kwargs.items():
            setattr(model, name, value)
        self._append(label, model)

    # ---- scoring ----
    def _model_set(self):
        # the packed device copy is valid for exactly these model objects in this state: refitting
        # a model in place, replacing an element or reloading one must not leave a stale copy
        key = tuple((id(g), getattr(g, "_version", 0)) for g in self.gmms)
        if self._set is None or self._set_key != key:
            self._set = ModelSet(self.gmms)
            self._set_key = key
        return self._set

    def gmm_score(self, gmm, x):
        return float(np.sum(gmm.score(x)))

    def predict_one_scores(self, x):
        """Summed log-likelihood of utterance ``x`` under every speaker model (one launch)."""
        if _lib.gpu_runtime_lost():
            # a worker forked after the parent used the GPU (the reference's fit-then-Pool drivers, test-nperson.py:126-139):
            # device-resident sets cannot exist here; the reference's own speaker-by-speaker loop (gmmset.py:59-64) can --
            # each call is served by this process's helper (csrc/fork_proxy.cpp)
            # -- in ONE conversation and one fused pass in the helper for the whole set (sr_score_models_f32; the per-speaker loop was
            # a conversation, a launch chain and a reply per speaker: 80 per utterance in the reference's logged run)
            X = _lib.f32_matrix(x)
            handles = (C.c_void_p * len(self.gmms))(*[g.gmm for g in self.gmms])
            sums = np.zeros(len(self.gmms))
            _lib.check(_lib.lib().sr_score_models_f32(handles, len(self.gmms), _lib.as_fp(X), X.shape[0], X.shape[1],
                                                      _lib.as_dp(sums), _lib.SR_CLAMP_COMPAT), "sr_score_models_f32")
            return sums.tolist()
        # one utterance at a time is how the reference's drivers call (gmmset.py:62-64, gui.py:179-214): the device batch is kept and
        # refilled, so such a loop allocates nothing
        # (a batch per calling thread: the calls below release the GIL)
        mine = self.__dict__.setdefault("_scratch", {})
        scratch = mine.get(threading.get_ident())
        if scratch is None:
            scratch = mine[threading.get_ident()] = Batch.from_features([x])
        else:
            scratch.reset_features(x)
        totals, _ = self._model_set().score(scratch)
        return totals[0].tolist()

    def _label_of_best(self, scores):
        return self.y[int(np.argmax(scores))]          # numpy's argmax keeps the first maximum, as
                                                        # max(enumerate(...)) does (gmmset.py:62-64)

    def predict_one(self, x):
        return self._label_of_best(self.predict_one_scores(x))

    def _topc_sums(self, utterances, top_c):
        # [UBM] + speakers through the top-C path, the UBM as background column 0 (core.ModelSet.score_topc)
        if self.ubm is None:
            raise AssertionError("UBM must be given prior to conduct reject prediction.")
        sums, _ = self._open_model_set().score_topc(Batch.from_features(utterances), 0, int(top_c))
        return sums

    def predict(self, X, top_c=None):
        """All utterances in one batch; the arg max comes back from the device.
        ``top_c``: score through top-C Gaussian selection against the UBM (speakers enrolled from it; an approximation, see
        ``ModelSet.score_topc``) -- the label is the first maximum over the speakers' columns, as the open-set route maps them."""
        utterances = list(X)
        if not utterances:
            return []
        if top_c is not None:
            sums = self._topc_sums(utterances, top_c)
            return [None if len(x) == 0 or not self.gmms else self.y[int(np.argmax(row[1:]))] for x, row in zip(utterances, sums)]
        if _lib.gpu_runtime_lost():
            return [self.predict_one(x) for x in utterances]
        _, winners = self._model_set().score(Batch.from_features(utterances))
        return [None if w < 0 else self.y[w] for w in winners]

    def _open_model_set(self):
        # [ubm] + speakers, the UBM as column 0; the same key discipline as _model_set, the UBM's state included
        models = [self.ubm] + list(self.gmms)
        key = tuple((id(g), getattr(g, "_version", 0)) for g in models)
        if self._open_set is None or self._open_set_key != key:
            self._open_set = ModelSet(models)
            self._open_set_key = key
        return self._open_set

    def _reject_batch(self, X, threshold=None):
        if self.ubm is None:
            raise AssertionError("UBM must be given prior to conduct reject prediction.")
        utterances = list(X)
        if not utterances:
            return np.zeros(0, np.int32), np.zeros(0)
        _, labels, margins = self._open_model_set().score_open(Batch.from_features(utterances), 0,
                                                                float(self.reject_threshold if threshold is None else threshold))
        return labels, margins

    def predict_with_reject_batch(self, X, threshold=None, top_c=None):
        """``predict_with_reject`` for all utterances in ONE batch, the decision taken on the device
        (``ModelSet.score_open`` over [UBM] + speakers): a list of labels, None for a rejected utterance.
        ``threshold``: decide against this value for the call instead of ``reject_threshold``, which stays as it is.
        ``top_c``: the sums come from top-C Gaussian selection (``ModelSet.score_topc``) and the same rule decides on them."""
        if top_c is not None:
            from .core import open_set_decide
            utterances = list(X)
            if self.ubm is None:
                raise AssertionError("UBM must be given prior to conduct reject prediction.")
            if not utterances:
                return []
            sums = self._topc_sums(utterances, top_c)
            labels, _ = open_set_decide(sums, [len(x) for x in utterances], 0,
                                        float(self.reject_threshold if threshold is None else threshold))
            return [None if w < 0 else self.y[w - 1] for w in labels]
        labels, _ = self._reject_batch(X, threshold)
        return [None if w < 0 else self.y[w - 1] for w in labels]

    def reject_margins(self, X):
        """The per-frame margin of every utterance's best speaker over the UBM (what ``reject_threshold`` is compared with),
        from the same batched pass; NaN for an utterance without frames."""
        return self._reject_batch(X)[1]

    def predict_one_with_rejection(self, x):
        """Open-set decision (gmmset.py:69-81): per-frame margin of the best speaker over the UBM
        below ``reject_threshold`` -> None.  (``predict_with_reject_batch`` decides a whole list in one device pass.)"""
        if self.ubm is None:
            raise AssertionError("UBM must be given prior to conduct reject prediction.")
        n = float(len(x))
        per_frame = np.asarray(self.predict_one_scores(x)) / n
        best = int(np.argmax(per_frame))
        margin = per_frame[best] - self.gmm_score(self.ubm, x) / n
        return self.y[best] if margin >= self.reject_threshold else None

    def predict_with_reject(self, X):
        """One utterance at a time, as the reference; ``predict_with_reject_batch`` is the batched form."""
        return [self.predict_one_with_rejection(x) for x in X]


class GMMSetPyGMM(GMMSet):
    def predict_one(self, x):
        # the reference divides every total by the frame count first (gmmset.py:96); same winner
        return self._label_of_best(np.asarray(self.predict_one_scores(x)) / float(len(x)))

    # models travel through pickle as their text dumps (gmmset.py:101-105)
    def before_pickle(self):
        self._set = None
        self._open_set = None
        self.__dict__.pop("_scratch", None)
        self.gmms = [m.dumps() for m in self.gmms]

    def after_pickle(self):
        self._set = None
        self._open_set = None
        self.gmms = [GMM.loads(text) for text in self.gmms]

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_set"] = None
        state["_open_set"] = None
        state.pop("_scratch", None)
        return state
