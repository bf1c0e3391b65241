"""Who spoke when: host-side helpers around the device timeline (``core.ModelSet.timeline``, include/pygmm_hip.h "Who spoke when").

``windows`` counts the windows of a recording, ``segments`` turns a label per window into time intervals, ``to_rttm`` writes them
in the RTTM format scoring tools read.  Pure Python: nothing here needs the device.
"""
from __future__ import annotations

import numpy as np


def windows(n: int, W: int, H: int) -> int:
    """Windows of a recording of ``n`` frames under window ``W`` and hop ``H`` (frames): 0 if empty, else
    1 + ceil(max(0, n - W) / H); window j covers frames [j H, min(j H + W, n)).  With W < H no window is formed that would start
    at or behind frame n: min(that, ceil(n / H))."""
    n, W, H = int(n), int(W), int(H)
    if W < 1 or H < 1:
        raise ValueError("window and hop must be at least 1 frame (got %d, %d)" % (W, H))
    if n <= 0:
        return 0
    return min(1 + -(-max(0, n - W) // H), -(-n // H))


def segments(labels, n_frames: int, W: int, H: int, frame_shift_s: float):
    """Labels per window -> ``[(start_s, end_s, label)]`` covering [0, n_frames * frame_shift_s] without gaps or overlaps.
    Label j owns frames [j H + c, (j + 1) H + c) with c = floor(max(0, W - H) / 2): the middle hop of its window.  The first
    window's interval reaches back to frame 0, the last one's forward to ``n_frames``; runs of equal labels are merged.  Labels
    are passed through (-1 is "nobody")."""
    labels = [int(x) for x in np.asarray(labels).reshape(-1)]
    n_frames, W, H = int(n_frames), int(W), int(H)
    if len(labels) != windows(n_frames, W, H):
        raise ValueError("%d labels for %d frames under window %d, hop %d (expected %d)" % (len(labels), n_frames, W, H, windows(n_frames, W, H)))
    c = max(0, W - H) // 2
    out = []
    for j, lab in enumerate(labels):
        a = 0 if j == 0 else min(j * H + c, n_frames)
        b = n_frames if j == len(labels) - 1 else min((j + 1) * H + c, n_frames)
        if out and out[-1][2] == lab:
            out[-1][1] = b
        elif b > a or not out:
            out.append([a, b, lab])
    return [(a * float(frame_shift_s), b * float(frame_shift_s), lab) for a, b, lab in out]


def to_rttm(segs, names=None, recording_id: str = "rec") -> str:
    """RTTM lines ("SPEAKER <id> 1 <start> <duration> <NA> <NA> <name> <NA> <NA>") of the segments that carry a speaker; "nobody"
    (label -1 or None) is silence and is left out.  ``names``: a sequence or mapping from label to name (default: "spk<label>")."""
    lines = []
    for start, end, lab in segs:
        if lab is None or (isinstance(lab, (int, np.integer)) and lab < 0):
            continue
        if isinstance(lab, (int, np.integer)):
            name = names[lab] if names is not None else "spk%d" % lab
        else:
            name = lab
        lines.append("SPEAKER %s 1 %.3f %.3f <NA> <NA> %s <NA> <NA>" % (recording_id, start, end - start, name))
    return "\n".join(lines) + ("\n" if lines else "")
