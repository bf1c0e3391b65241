"""What the tests of the multi-GPU predictor share: the recorded plan table (tests/host/multi_table.inc, read as data), the
invariants of a plan as ``_lib.multi_plan`` returns it, and the long-utterance signals that make a slot cut several pieces."""
import ast
import os
import re

import numpy as np

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "multi_table.inc")
MULTI_CHUNKS = 8


def load_table() -> dict:
    """{"PartitionCases": [...], "PiecesCases": [...], "ScheduleCases": [...]}: the rows of multi_table.inc as nested lists (a C
    initialiser list of numbers and strings is a Python literal once its braces are brackets)."""
    text = re.sub(r"^\s*//.*$", "", open(TABLE).read(), flags=re.M)
    out = {}
    for name, body in re.findall(r"static const \w+ k(\w+)\[\] = \{\n(.*?)\n\};", text, flags=re.S):
        out[name] = ast.literal_eval("[" + body.replace("{", "[").replace("}", "]") + "]")
    assert set(out) == {"PartitionCases", "PiecesCases", "ScheduleCases"}
    return out


def offsets_of(runs) -> np.ndarray:
    """Cumulative sample offsets of lengths given as runs [count, samples]."""
    lengths = np.concatenate([np.full(c, v, np.int64) for c, v in runs]) if runs else np.zeros(0, np.int64)
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def list_of(spans) -> list:
    return [first + i for first, count in spans for i in range(count)]


def check_plan(plan, offsets, devices, merge, schedules=None) -> None:
    """Every utterance in exactly one active slot, a slot's list ascending, its pieces a contiguous cover of it with u0 <= u1,
    1 <= n <= MULTI_CHUNKS (and within what the schedule, the utterance count and the 2^20-sample floor allow), and no two
    active slots on one device when they merge."""
    n_utt = len(offsets) - 1
    slots = [p["slot"] for p in plan]
    assert slots == sorted(set(slots)) and slots[0] == 0 and all(0 <= k < len(devices) for k in slots)
    if merge:
        assert len({devices[k] for k in slots}) == len(slots)
    else:
        assert slots == list(range(len(devices)))
    assert {devices[k] for k in slots} == set(devices)
    assert sorted(u for p in plan for u in p["utts"]) == list(range(n_utt))
    for p in plan:
        utts, pieces = p["utts"], p["pieces"]
        assert utts == sorted(utts)
        total = int(sum(offsets[u + 1] - offsets[u] for u in utts))
        want = 4 if (schedules is not None and schedules[p["slot"]]) else 8
        assert 1 <= len(pieces) <= min(MULTI_CHUNKS, want)
        assert len(pieces) == max(1, min(want, len(utts), total >> 20))
        assert pieces[0][0] == 0 and pieces[-1][1] == len(utts)
        assert all(u0 <= u1 for u0, u1 in pieces) and all(pieces[c][0] == pieces[c - 1][1] for c in range(1, len(pieces)))


def long_utterances(fs, n, rng):
    """n int16 utterances of 0.4-9 s cut from a few synthetic speakers (several M samples in all), plus one without a frame."""
    from speaker_recognition_amd import synth
    base = [synth.synth_speech(9 * s, 60.0, fs, seed=300 + s) for s in range(6)]
    out = []
    for i in range(n):
        b = base[i % len(base)]
        L = int(rng.uniform(0.4, 9.0) * fs)
        o = int(rng.integers(0, len(b) - L))
        out.append(np.ascontiguousarray(b[o:o + L]))
    out.insert(n // 2, np.zeros(100, np.int16))
    return out
