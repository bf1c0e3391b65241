"""The short-time feature normalisation's definitions, restated in numpy and float64 (what csrc/featnorm.hip must compute).

One utterance X [T, D] of fp32 values, a window of W frames: N = min(W, T), frame t's window is the rows [s0, s0 + N) with
s0(t) = min(max(t - W // 2, 0), T - N) -- centred in the interior, shifted (not shortened) at both ends.
  warp: less / eq = window values < / == x_t (fp32), r2 = 2 less + eq - 1, out = float32(Q((r2 + 1) / (2 N))), Q the standard normal
        quantile of ``statistics.NormalDist`` (AS241), taken through the lower half of the distribution (a = r2 + 1 above N:
        -Q((2 N - a) / (2 N)); a == N: 0) so that mirrored ranks give negated values to the bit.  NaN cell: NaN, rank -1, counted.
  cmn:  out = float32(x_t - mean), mean = (sum x) / N, summed in window order.
  cmvn: out = float32((x_t - mean) / sqrt(var)), var = (sum (x - mean)^2) / N in window order; max == min: exactly 0, counted."""
from statistics import NormalDist

import numpy as np

_Q = NormalDist().inv_cdf


def window_starts(T, W):
    N = min(W, T)
    return np.minimum(np.maximum(np.arange(T) - W // 2, 0), T - N), N


def warp_value(r2, N):
    a, M = r2 + 1, 2 * N
    if a == N:
        return 0.0
    return _Q(a / M) if a < N else -_Q((M - a) / M)


def ranks(X, W):
    """-> int32 [T, D] doubled mid-ranks (-1 for a NaN cell)"""
    X = np.asarray(X, np.float32)
    T = X.shape[0]
    s0, N = window_starts(T, W)
    less, eq = np.zeros(X.shape, np.int32), np.zeros(X.shape, np.int32)
    with np.errstate(invalid="ignore"):
        for k in range(N):
            v = X[s0 + k]
            less += v < X
            eq += v == X
    return 2 * less + eq - 1


def warp(X, W):
    """-> (float32 [T, D], ranks, count of NaN cells)"""
    r = ranks(X, W)
    N = min(W, r.shape[0])
    table = np.array([warp_value(k, N) for k in range(max(2 * N - 1, 0))] + [np.nan])          # [-1] is the NaN cell's
    return table[r].astype(np.float32), r, int((r < 0).sum())


def sliding_all(X, W):
    """-> (cmn float32 [T, D], cmvn float32 [T, D], bool [T, D]: the window holds equal values only)"""
    X32 = np.asarray(X, np.float32)
    X = X32.astype(np.float64)
    T = X.shape[0]
    s0, N = window_starts(T, W)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = np.zeros(X.shape)
        for k in range(N):
            s += X[s0 + k]                                      # in window order
        mean = s / max(N, 1)
        acc = np.zeros(X.shape)
        hi, lo = np.full(X.shape, -np.inf, np.float32), np.full(X.shape, np.inf, np.float32)
        for k in range(N):
            d = X[s0 + k] - mean
            acc += d * d
            np.maximum(hi, X32[s0 + k], out=hi)
            np.minimum(lo, X32[s0 + k], out=lo)
        flat = hi == lo
        cmn = X - mean
        cmvn = np.where(flat, 0.0, cmn / np.sqrt(acc / max(N, 1)))
    return cmn.astype(np.float32), cmvn.astype(np.float32), flat


def sliding(X, W, norm_vars):
    """-> (float32 [T, D], count of equal-valued windows (cmvn; 0 for cmn))"""
    cmn, cmvn, flat = sliding_all(X, W)
    return (cmvn, int(flat.sum())) if norm_vars else (cmn, 0)


def normalise(X, mode, W):
    """-> (float32 output, per-utterance degenerate count)"""
    if mode == "warp":
        out, _, n = warp(X, W)
        return out, n
    return sliding(X, W, mode == "cmvn")
