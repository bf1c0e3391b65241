"""The reference's energy-threshold silence removal (src/filters/silence.py:11-50), restated in numpy: exact int64 sums, float64
decisions in the reference's operation order, and its Python 2 integer divisions on the offsets of unsigned input.  The checker of
csrc/silence.hip (tests/test_gpu_silence.py) and of itself (tests/test_silence_cpu.py)."""
import numpy as np


def frame_params(fs, frame_duration=0.02, frame_shift=0.01):
    """(L, S): frame length and shift in samples, as int() truncates the float64 products."""
    return int(frame_duration * fs), int(frame_shift * fs)


def remove_silence(fs, signal, frame_duration=0.02, frame_shift=0.01, perc=0.15):
    """-> the kept samples, in ``signal``'s dtype (any numpy integer type the reference's np.iinfo takes)."""
    signal = np.asarray(signal)
    info = np.iinfo(signal.dtype)                   # raises on floats, as the reference
    unsigned = info.min >= 0
    x = signal.astype(np.int64)
    if unsigned:
        x = x - (info.max + 1) // 2                 # Python 2's `/` on ints: 128 for uint8
    n = len(x)
    L, S = frame_params(fs, frame_duration, frame_shift)
    if L < 1 or S < 1 or n < 1:
        raise ValueError("L = %d, S = %d, n = %d: the reference loops forever or raises here" % (L, S, n))
    pre = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(x * x, out=pre[1:])
    threshold = (int(pre[n]) / float(n)) * perc     # an exact integer -> float64, one division, one multiply
    out = []
    i = 0
    while i < n:
        hi = min(i + L, n)
        e = int(pre[hi] - pre[i]) / float(hi - i)
        if e < threshold:
            i += L
        else:
            out.append(x[i:min(i + S, hi)])
            i += S
    ret = np.concatenate(out) if out else np.zeros(0, np.int64)
    if unsigned:
        ret = ret + info.max // 2                   # 127 for uint8: the asymmetry is the reference's
    return ret.astype(signal.dtype)


def envelope_noise(n, seed=0):
    """Gaussian noise under a two-level envelope: sigma 30 or 3000, switching every 137 samples (seeded), int16."""
    rng = np.random.default_rng(seed)
    level = np.where(rng.integers(0, 2, (n + 136) // 137) == 1, 3000.0, 30.0)
    sigma = np.repeat(level, 137)[:n]
    return np.clip(np.rint(rng.standard_normal(n) * sigma), -32768, 32767).astype(np.int16)


def tie_signal(fs=8000, q=100, n=2400):
    """Amplitude 2q for the first third, q for the rest: with perc = 0.5 the quiet frames lie exactly on the threshold."""
    x = np.full(n, q, dtype=np.int16)
    x[:n // 3] = 2 * q
    return x
