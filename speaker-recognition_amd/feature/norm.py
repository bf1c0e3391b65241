"""Short-time feature normalisation of host matrices on the device (csrc/featnorm.hip through ``Batch.normalise``): feature
warping (Pelecanos & Sridharan 2001: each coefficient mapped through its rank in a sliding window onto a standard normal) and
sliding-window mean / mean-and-variance normalisation (what Kaldi's ``apply-cmvn-sliding`` does with a centred window).

Every matrix is [frames, dim]; each utterance and each column is normalised on its own.  The window of ``window`` frames (2 ..
1024) is centred on the frame, and shifted -- not shortened -- at both ends of the utterance; an utterance shorter than the window
is its own window.  Results are float32, as the device computes them."""
from __future__ import annotations

import numpy as np

from ..core import Batch

__all__ = ["MODES", "check_setting", "feature_warp", "sliding_cmvn", "normalise_many"]

MODES = ("warp", "cmn", "cmvn")
MIN_WINDOW, MAX_WINDOW = 2, 1024


def check_setting(mode, window=301):
    """-> (mode, window) as the device takes them; ValueError for anything it would refuse (no device call)."""
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError("the normalisation mode must be one of %s (got %r)" % (", ".join(MODES), mode))
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or not MIN_WINDOW <= int(window) <= MAX_WINDOW:
        raise ValueError("the normalisation window must be an integer in %d .. %d frames (got %r)" % (MIN_WINDOW, MAX_WINDOW, window))
    return mode, int(window)


def normalise_many(matrices, mode="warp", window=301):
    """Every matrix of a list normalised in ONE device call; -> a list of float32 matrices of the same shapes."""
    mode, window = check_setting(mode, window)
    mats = [np.asarray(m) for m in matrices]
    if not mats:
        return []
    for m in mats:
        if m.ndim != 2 or m.shape[1] != mats[0].shape[1] or m.shape[1] < 1:
            raise ValueError("expected [frames, dim] matrices of one width")
    out = Batch.from_features(mats).normalise(mode, window)
    Y, off = out.download(), out.offsets()
    return [Y[off[u]:off[u + 1]] for u in range(len(mats))]


def feature_warp(X, window=301):
    """Feature warping of one [frames, dim] matrix over ``window`` frames (3 s at a 10 ms shift)."""
    return normalise_many([X], "warp", window)[0]


def sliding_cmvn(X, window=301, norm_vars=True):
    """Sliding-window mean (``norm_vars=False``) or mean-and-variance normalisation of one [frames, dim] matrix."""
    return normalise_many([X], "cmvn" if norm_vars else "cmn", window)[0]
