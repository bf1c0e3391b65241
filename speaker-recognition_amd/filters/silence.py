"""Energy-threshold silence removal -- same surface as the reference's ``src/filters/silence.py`` (``remove_silence``, :11-50),
which its corpus preparation (``src/data/remove-silence.py``) applies to every recording.  The arithmetic runs on the GPU
(csrc/silence.hip: exact integer energies, the reference's float64 decisions, bit-identical output); this module recentres and
widens the sample types the device does not take and restores them afterwards.

int16, int8 and uint8 signals are accepted.  Unsigned input is recentred as the reference does it under Python 2's integer
division: ``x - (max + 1) // 2`` on the way in, ``+ max // 2`` on the way out (128 and 127 for uint8).  Anything else raises
``TypeError``: floats fail in the reference too (``np.iinfo``), and wider integers would need its wrap-around behaviour."""
from __future__ import annotations

import numpy as np

from ..core import Batch

__all__ = ["remove_silence", "remove_silence_many"]


def _to_device_type(signal):
    """-> (int16 samples, offset to add back, the caller's dtype)"""
    a = np.asarray(signal)
    if a.ndim != 1:
        raise ValueError("Only Support Mono Wav File!")
    if len(a) == 0:
        raise ValueError("remove_silence: empty signal")            # the reference: IndexError at signal[0]
    if a.dtype == np.int16:
        return np.ascontiguousarray(a), 0, a.dtype
    if a.dtype == np.int8:
        return a.astype(np.int16), 0, a.dtype
    if a.dtype == np.uint8:
        info = np.iinfo(a.dtype)
        return a.astype(np.int16) - np.int16((info.max + 1) // 2), info.max // 2, a.dtype
    raise TypeError("remove_silence takes int16, int8 or uint8 samples, not %s" % a.dtype)


def remove_silence_many(fs, signals, frame_duration=0.02, frame_shift=0.01, perc=0.15):
    """``remove_silence`` of every signal of a list, in ONE device call; -> a list of arrays, each in its signal's dtype."""
    prepared = [_to_device_type(s) for s in signals]
    if not prepared:
        return []
    out = Batch.from_pcm([p[0] for p in prepared]).remove_silence(fs, frame_duration, frame_shift, perc)
    cat, off = out.download_pcm(), out.offsets()
    ret = []
    for u, (_, back, dtype) in enumerate(prepared):
        kept = cat[off[u]:off[u + 1]]
        # (the reference adds the offset in int64 and lets astype wrap)
        ret.append((kept.astype(np.int64) + back).astype(dtype) if back or dtype != np.int16 else kept.copy())
    return ret


def remove_silence(fs, signal, frame_duration=0.02, frame_shift=0.01, perc=0.15):
    """Drop the frames whose mean energy is below ``perc`` times the signal's (silence.py:11-50); same dtype as ``signal``."""
    return remove_silence_many(fs, [signal], frame_duration, frame_shift, perc)[0]
