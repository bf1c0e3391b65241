"""Speaker embeddings from a network the user brings: the Python surface of csrc/xvector.hip (include/pygmm_hip.h, "Speaker
embeddings").  Inference only: an ``XVector`` is an ordered list of layers that ends at the embedding layer (a trained x-vector
network is cut there, at Kaldi's ``tdnn6.affine``), and ``extract`` runs it on the device over whole utterances or over a table of
segments.  The result feeds everything that takes one vector per segment: ``plda.fit_transform``, ``plda.cosine_score``,
``scorenorm``, ``calibration``, ``diarize.ahc``.

Layers are plain dicts (``tdnn``, ``stats_pool`` and ``affine`` below build them):

``tdnn``        frame layer.  ``offsets``: strictly ascending integers o_1 < ... < o_m (1 <= m <= 9, |o| <= 16); ``W`` [C_out, m C_in],
                offset-major (block j multiplies the frame at offset o_j); ``b`` [C_out]; ``act`` "relu" or "none"; optional per-channel
                ``scale`` and ``shift``.  Output  y = scale * act(W x_ctx + b) + shift: Kaldi's order -- affine, ReLU, batch-norm.  A
                batch-norm IN FRONT of the ReLU is folded into ``W`` and ``b`` by the user, with ``scale`` / ``shift`` left out.  Valid
                convolution only: T input frames give T - (o_m - o_1) output frames, output frame u = b + sum_j W_j x[u + o_j - o_1].
``stats_pool``  per segment and channel the mean and the standard deviation over the remaining frames, population variance:
                std = sqrt(max(sum x^2 / n - mean^2, var_floor)); output [mean | std], 2 C wide.  Exactly one per network.
``affine``      segment layer: the form of ``tdnn`` with offsets (0,) on the [n_segments, C] matrix.  The last layer's output is the
                embedding; its ``act`` must be "none".

Channel widths are 1 .. 4096, any value; the padding to the kernel's granule happens inside the library and never shows.

Arithmetic: weights are rounded once to bf16 (round to nearest even) when the network is created, features by a convert kernel; every
layer accumulates in fp32 on the bf16 matrix cores, its epilogue runs in fp32, activations are stored as bf16, the last layer as fp32;
the pooling sums in float64.  A segment's embedding is the same bits alone, in any batch, at any position, under any
``xvector_scratch_mib`` and from run to run.

File format (``save`` / ``load``): one ``.npz`` with ``n_layers`` and, per layer i, the keys ``"<i>.kind"`` ("tdnn", "stats_pool",
"affine"), ``"<i>.offsets"`` (int32), ``"<i>.W"``, ``"<i>.b"`` (float32), ``"<i>.act"`` ("relu", "none"), ``"<i>.scale"``,
``"<i>.shift"`` (float32; absent when the layer has none).  A pooling layer stores ``"<i>.kind"``, ``"<i>.var_floor"`` (float64) and
its width ``"<i>.channels"``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import SRError, check, lib

KINDS = ("tdnn", "stats_pool", "affine")
ACTS = ("none", "relu")


def tdnn(offsets, W, b, act="relu", scale=None, shift=None) -> dict:
    return {"kind": "tdnn", "offsets": tuple(int(o) for o in offsets), "W": W, "b": b, "act": act, "scale": scale, "shift": shift}


def affine(W, b, act="none", scale=None, shift=None) -> dict:
    return {"kind": "affine", "offsets": (0,), "W": W, "b": b, "act": act, "scale": scale, "shift": shift}


def stats_pool(channels: int, var_floor: float = 1e-10) -> dict:
    return {"kind": "stats_pool", "channels": int(channels), "var_floor": float(var_floor)}


def _f32(a, what):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim not in (1, 2):
        raise ValueError("%s must be a vector or a matrix" % what)
    return a


class XVector:
    """The network, resident on the device after its first ``extract``."""

    def __init__(self, layers):
        self.layers = [self._normalise(i, dict(l)) for i, l in enumerate(layers)]
        n = len(self.layers)
        desc = np.zeros((max(n, 1), 16), dtype=np.int32)
        floors = np.zeros(max(n, 1), dtype=np.float64)
        fpp = C.POINTER(C.c_float)
        W, b, sc, sh = ((fpp * max(n, 1))() for _ in range(4))
        for i, l in enumerate(self.layers):
            k = KINDS.index(l["kind"])
            if k == 1:
                desc[i, :3] = (1, l["channels"], 2 * l["channels"])
                floors[i] = l["var_floor"]
                continue
            m = len(l["offsets"])
            if m > 9:
                raise ValueError("layer %d has %d offsets; a descriptor row holds at most 9" % (i, m))
            c_out, k_in = l["W"].shape
            c_in = k_in // max(m, 1)
            if m < 1 or c_in * m != k_in or l["b"].shape != (c_out,):
                raise ValueError("layer %d: W is %r for %d offsets and b is %r; W is [C_out, m C_in], b [C_out]" % (i, l["W"].shape, m, l["b"].shape))
            desc[i, :6] = (k, c_in, c_out, ACTS.index(l["act"]), int(l["scale"] is not None), m)
            desc[i, 6:6 + m] = l["offsets"]
            W[i], b[i] = _lib.as_fp(l["W"]), _lib.as_fp(l["b"])
            if l["scale"] is not None:
                if l["scale"].shape != (c_out,) or l["shift"].shape != (c_out,):
                    raise ValueError("layer %d: scale and shift are [C_out]" % i)
                sc[i], sh[i] = _lib.as_fp(l["scale"]), _lib.as_fp(l["shift"])
        self._desc, self._floors = desc, floors
        h = lib().sr_xvector_create(n, desc.ctypes.data_as(C.POINTER(C.c_int32)), _lib.as_dp(floors), W, b, sc, sh)
        if not h:
            raise SRError("sr_xvector_create failed: %s" % _lib.last_error())
        self._h = C.c_void_p(h)
        info = np.zeros(12, dtype=np.int32)
        check(lib().sr_xvector_info(self._h, info.ctypes.data_as(C.POINTER(C.c_int32)), 12), "sr_xvector_info")
        self.n_layers, self.pool_index, self.input_dim, self.embedding_dim, self.context = (int(x) for x in info[:5])
        self.tile_rows, self.tile_cols = int(info[5]), int(info[6])

    @staticmethod
    def _normalise(i, l):
        if l.get("kind") not in KINDS:
            raise ValueError("layer %d: kind must be one of %r (got %r)" % (i, KINDS, l.get("kind")))
        if l["kind"] == "stats_pool":
            return {"kind": "stats_pool", "channels": int(l["channels"]), "var_floor": float(l.get("var_floor", 1e-10))}
        if l.get("act", "none") not in ACTS:
            raise ValueError("layer %d: act must be 'relu' or 'none' (got %r)" % (i, l.get("act")))
        if (l.get("scale") is None) != (l.get("shift") is None):
            raise ValueError("layer %d: scale and shift are given together or not at all" % i)
        out = {"kind": l["kind"], "offsets": tuple(int(o) for o in l.get("offsets", (0,))), "W": _f32(l["W"], "W"), "b": _f32(l["b"], "b"),
               "act": l.get("act", "none"), "scale": None, "shift": None}
        if out["W"].ndim != 2 or out["b"].ndim != 1:
            raise ValueError("layer %d: W is a matrix [C_out, m C_in], b a vector [C_out]" % i)
        if l.get("scale") is not None:
            out["scale"], out["shift"] = _f32(l["scale"], "scale"), _f32(l["shift"], "shift")
        return out

    # ---- files ----

    def save(self, path) -> None:
        d = {"n_layers": np.int64(len(self.layers))}
        for i, l in enumerate(self.layers):
            d["%d.kind" % i] = np.str_(l["kind"])
            if l["kind"] == "stats_pool":
                d["%d.channels" % i] = np.int64(l["channels"])
                d["%d.var_floor" % i] = np.float64(l["var_floor"])
                continue
            d["%d.offsets" % i] = np.asarray(l["offsets"], dtype=np.int32)
            d["%d.W" % i], d["%d.b" % i], d["%d.act" % i] = l["W"], l["b"], np.str_(l["act"])
            if l["scale"] is not None:
                d["%d.scale" % i], d["%d.shift" % i] = l["scale"], l["shift"]
        with open(path, "wb") as f:
            np.savez(f, **d)

    @classmethod
    def load(cls, path) -> "XVector":
        with np.load(path, allow_pickle=False) as z:
            layers = []
            for i in range(int(z["n_layers"])):
                kind = str(z["%d.kind" % i])
                if kind == "stats_pool":
                    layers.append(stats_pool(int(z["%d.channels" % i]), float(z["%d.var_floor" % i])))
                    continue
                has = "%d.scale" % i in z.files
                layers.append({"kind": kind, "offsets": tuple(int(o) for o in z["%d.offsets" % i]), "W": z["%d.W" % i], "b": z["%d.b" % i],
                               "act": str(z["%d.act" % i]), "scale": z["%d.scale" % i] if has else None,
                               "shift": z["%d.shift" % i] if has else None})
        return cls(layers)

    # ---- the plan (host only) ----

    def plan(self, lengths, tap=None, tap_bf16=False, scratch_bytes: int = 0, tiles_of=None) -> dict:
        """What a call over segments of ``lengths`` frames does (sr_xvector_plan; no device): the tile shape, the padded widths,
        every segment's rows at every stage, the chunks under the scratch bound (0: the option xvector_scratch_mib) and the tile
        counts per layer and chunk; ``tiles_of=(layer, chunk)`` adds that tile list as rows (segment in chunk, first row, rows)."""
        lengths = np.ascontiguousarray(lengths, dtype=np.int64).reshape(-1)
        n, L = len(lengths), self.n_layers
        out = np.zeros(16, dtype=np.int64)
        widths = np.zeros(L + 1, dtype=np.int32)
        rows = np.zeros((L + 1, n), dtype=np.int64)
        chunk_begin = np.zeros(n + 2, dtype=np.int64)
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)

        def call(counts, layer, chunk, tiles, cap):
            return check(lib().sr_xvector_plan(L, self._desc.ctypes.data_as(i32p), _lib.as_dp(self._floors), _lib.as_i64p(lengths), n,
                                               -1 if tap is None else int(tap), int(bool(tap_bf16)), int(scratch_bytes), _lib.as_i64p(out), 16,
                                               widths.ctypes.data_as(i32p), _lib.as_i64p(rows), _lib.as_i64p(chunk_begin),
                                               counts.ctypes.data_as(i64p) if counts is not None else None, layer, chunk,
                                               tiles.ctypes.data_as(i32p) if tiles is not None else None, cap), "sr_xvector_plan")
        n_chunks = call(None, 0, 0, None, 0)
        counts = np.zeros((L, max(n_chunks, 1)), dtype=np.int64)
        call(counts, 0, 0, None, 0)
        res = {"tile_rows": int(out[0]), "tile_cols": int(out[1]), "k_stage": int(out[2]), "granule": int(out[3]), "context": int(out[4]),
               "embedding_dim": int(out[5]), "n_chunks": int(out[6]), "lds_bytes": int(out[7]), "pool_index": int(out[8]), "last_layer": int(out[9]),
               "out_shape": (int(out[10]), int(out[11])), "buffer_bytes": (int(out[12]), int(out[13])), "chunk_bytes": int(out[14]),
               "scratch_bytes": int(out[15]), "width_pad": widths.copy(), "rows": rows, "chunk_begin": chunk_begin[:n_chunks + 1].copy(),
               "tile_counts": counts[:, :n_chunks]}
        if tiles_of is not None:
            layer, chunk = tiles_of
            cap = int(counts[layer, chunk])
            tiles = np.zeros((max(cap, 1), 3), dtype=np.int32)
            call(counts, int(layer), int(chunk), tiles, cap)
            res["tiles"] = tiles[:cap]
        return res

    # ---- the forward pass ----

    def _out_shape(self, lengths, tap):
        last = self.n_layers - 1 if tap is None else int(tap)
        if not -1 < last < self.n_layers:
            raise ValueError("tap must be None or a layer index 0 .. %d" % (self.n_layers - 1))
        l = self.layers[last]
        cols = 2 * l["channels"] if l["kind"] == "stats_pool" else l["W"].shape[0]
        if last >= self.pool_index:
            return len(lengths), cols
        used = sum(x["offsets"][-1] - x["offsets"][0] for x in self.layers[:last + 1])
        return int(sum(max(int(n) - used, 0) for n in lengths)), cols

    def extract(self, feats, segments=None, tap=None, tap_bf16=False, times=False):
        """``feats``: a ``core.Batch`` of features (they stay where they are) or a list of [T, D] arrays.  ``segments``: None (one
        segment per utterance) or an int array [n, 3] of (utterance, first frame, frames).  -> float32 [n, E].  ``tap``: a layer index
        returns that layer's output instead (fp32; ``tap_bf16``: the bf16 values the layer stores inside the network, widened):
        [sum of the segments' rows, C_out] for a frame layer, [n, 2 C] for the pooling.  ``times``: also the per-stage device times in
        ms, ``{"convert": .., "layers": [..]}``."""
        from .core import Batch
        segs = None
        if segments is not None:
            segs = np.ascontiguousarray(segments, dtype=np.int32).reshape(-1, 3)
        t = np.zeros(self.n_layers + 1, dtype=np.float64)
        i32p = C.POINTER(C.c_int32)
        segp = segs.ctypes.data_as(i32p) if segs is not None else None
        n_seg = 0 if segs is None else len(segs)
        if isinstance(feats, Batch):
            lengths = np.diff(feats.offsets()) if segs is None else segs[:, 2]
            out = np.zeros(self._out_shape(lengths, tap), dtype=np.float32)
            check(lib().sr_xvector_extract_batch(self._h, feats._h, segp, n_seg, -1 if tap is None else int(tap), int(bool(tap_bf16)),
                                                 _lib.as_fp(out), out.size, _lib.as_dp(t)), "sr_xvector_extract_batch")
        else:
            mats = [_lib.f32_matrix(x) for x in feats]
            X = np.concatenate(mats, axis=0) if mats else np.zeros((0, self.input_dim), np.float32)
            offsets = np.zeros(len(mats) + 1, dtype=np.int64)
            offsets[1:] = np.cumsum([m.shape[0] for m in mats])
            lengths = np.diff(offsets) if segs is None else segs[:, 2]
            out = np.zeros(self._out_shape(lengths, tap), dtype=np.float32)
            check(lib().sr_xvector_extract(self._h, _lib.as_fp(X), X.shape[0], X.shape[1], _lib.as_i64p(offsets), len(mats), segp, n_seg,
                                           -1 if tap is None else int(tap), int(bool(tap_bf16)), _lib.as_fp(out), out.size, _lib.as_dp(t)),
                  "sr_xvector_extract")
        if times:
            return out, {"convert": float(t[0]), "layers": [float(x) for x in t[1:]]}
        return out

    def extract_windows(self, feats, window: int, hop: int):
        """Sliding windows of ``window`` frames every ``hop`` frames over every utterance (the windows that fit whole) ->
        ``(embeddings [n, E], table [n, 3])``: the input of ``plda.cosine_score`` followed by ``diarize.ahc``."""
        from .core import Batch
        window, hop = int(window), int(hop)
        if window < self.context + 1 or hop < 1:
            raise ValueError("window must be at least the network's context + 1 = %d frames and hop >= 1" % (self.context + 1))
        lengths = np.diff(feats.offsets()) if isinstance(feats, Batch) else [np.shape(x)[0] for x in feats]
        table = window_table(lengths, window, hop)
        return self.extract(feats, segments=table), table

    def __del__(self):
        try:
            if self._h:
                lib().sr_xvector_free(self._h)
                self._h = None
        except Exception:
            pass


def window_table(lengths, window: int, hop: int) -> np.ndarray:
    """(utterance, first frame, frames) of every whole window of every utterance."""
    rows = [(u, f, window) for u, T in enumerate(lengths) for f in range(0, int(T) - window + 1, hop)]
    return np.asarray(rows, dtype=np.int32).reshape(-1, 3)
