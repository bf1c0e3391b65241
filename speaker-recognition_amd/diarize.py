"""Who spoke when with nobody enrolled: the Python surface of csrc/diar.hip (include/pygmm_hip.h "Who spoke when, nobody enrolled").

``cluster`` runs the device chain on features -- per-segment full-covariance statistics, BIC change detection, agglomerative
clustering under delta-BIC -- and ``ahc`` the same merge loop on a caller's dissimilarity matrix (a PLDA or cosine score matrix
turned into distances).  ``cut`` re-cuts a merge log on the host, ``frame_segments`` turns labelled initial clusters into time
intervals that ``timeline.to_rttm`` writes.  ``ModelInterface.diarize`` composes them with the batched fits and the Viterbi decode.
"""
from __future__ import annotations

import numpy as np

from . import _lib


def cluster(features_or_batch, L: int = 100, change: str = "bic", half_width: int = 2, penalty: float = 1.0, ridge: float = 1e-3,
            threshold: float = 0.0, k=None, k_max=None):
    """Clusters one recording: a [frames, D] matrix, or every recording of a ``core.Batch`` of features.  ``k``: exactly that many
    clusters (as far as finite distances allow); ``k_max``: at most that many, fewer when pairs still lie below ``threshold``.
    -> for a matrix ``(labels, ranges, merges)``: a label per initial cluster, the initial clusters' frame ranges [n_init, 2], and
    the merge log ``(merge_i, merge_j, merge_d)``; for a batch a list of such tuples."""
    from .core import Batch
    k_min, k_cap = _stop_args(k, k_max)
    single = not isinstance(features_or_batch, Batch)
    batch = Batch.from_features([np.asarray(features_or_batch)]) if single else features_or_batch
    lengths = np.diff(batch.offsets())
    res = batch.diarize(L=L, change=change, half_width=half_width, penalty=penalty, ridge=ridge, threshold=threshold, k_min=k_min, k_max=k_cap)
    out = [(r["labels"], frame_ranges(r["init_off"], int(n), L), (r["merge_i"], r["merge_j"], r["merge_d"])) for r, n in zip(res, lengths)]
    return out[0] if single else out


def ahc(dist, linkage: str = "average", threshold: float = 0.0, k=None, k_max=None):
    """Agglomerative clustering of a symmetric dissimilarity matrix on the device (sr_ahc_matrix): ``linkage`` "average",
    "complete" or "single"; pairs merge while their distance is below ``threshold``.  -> ``(labels, (merge_i, merge_j, merge_d))``.
    Scores turn into distances by negation: ``ahc(-PLDA.score(x, x), threshold=-t)``."""
    link = _lib.ahc_linkage(linkage)
    if link < 0:
        raise ValueError("linkage must be 'average', 'complete' or 'single' (got %r)" % (linkage,))
    k_min, k_cap = _stop_args(k, k_max)
    lab, mi, mj, md = _lib.ahc_matrix(dist, link, threshold, k_min, k_cap)
    return lab, (mi, mj, md)


def cut(merges, n: int, threshold=None, k=None):
    """Re-cuts a merge log over ``n`` initial clusters without another device call: the labels a run with that ``threshold`` and /
    or exactly ``k`` clusters would have given, as long as the log reaches that far (a log made with ``threshold=inf`` is the whole
    dendrogram).  ``merges``: ``(merge_i, merge_j, merge_d)``."""
    if threshold is None and k is None:
        raise ValueError("cut needs a threshold, a number of clusters, or both")
    k_min, k_cap = _stop_args(k, None)
    labels, _ = _lib.diar_cut(n, merges[0], merges[1], merges[2], -np.inf if threshold is None else threshold, k_min, k_cap)
    return labels


def _stop_args(k, k_max):
    for name, v in (("k", k), ("k_max", k_max)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1):
            raise ValueError("%s must be None or an integer >= 1 (got %r)" % (name, v))
    if k is not None and k_max is not None:
        raise ValueError("give k (exactly that many clusters) or k_max (at most that many), not both")
    if k is not None:
        return int(k), int(k)
    return 1, 0 if k_max is None else int(k_max)


def frame_ranges(init_off, n_frames: int, L: int) -> np.ndarray:
    """The frames [start, end) of every initial cluster from its run of base segments: segment i covers [i L, (i + 1) L), the last
    segment of the recording reaches to ``n_frames``."""
    init_off = np.asarray(init_off, dtype=np.int64).reshape(-1)
    n_init = len(init_off) - 1
    out = np.zeros((max(n_init, 0), 2), dtype=np.int64)
    for c in range(n_init):
        out[c, 0] = init_off[c] * int(L)
        out[c, 1] = int(n_frames) if c == n_init - 1 else init_off[c + 1] * int(L)
    return out


def frame_segments(init_off, labels, n_frames: int, L: int, frame_shift_s: float):
    """Labelled initial clusters -> ``[(start_s, end_s, label)]`` covering [0, n_frames * frame_shift_s] without gaps or overlaps,
    runs of equal labels merged: what ``timeline.to_rttm`` takes."""
    labels = [int(x) for x in np.asarray(labels).reshape(-1)]
    ranges = frame_ranges(init_off, n_frames, L)
    if len(labels) != len(ranges):
        raise ValueError("%d labels for %d initial clusters" % (len(labels), len(ranges)))
    if len(ranges) and (ranges[0, 0] != 0 or np.any(ranges[:, 1] <= ranges[:, 0])):
        raise ValueError("the runs of base segments must start at 0 and grow")
    out = []
    for (a, b), lab in zip(ranges.tolist(), labels):
        if out and out[-1][2] == lab:
            out[-1][1] = b
        else:
            out.append([a, b, lab])
    return [(a * float(frame_shift_s), b * float(frame_shift_s), lab) for a, b, lab in out]
