"""The multi-GPU predictor's sharding plan (csrc/multi_plan.cpp) through the library the device compiler built (sr_multi_plan): the
decisions recorded from the commit before the plan became a file of its own (tests/host/multi_table.inc -- the same table the g++
build reproduces under the host sanitizers, tests/host/multi_checks.cpp: both compilers cut the same pieces), its invariants over
the table and seeded random batches, and the refusals, none of which needs a device."""
import ctypes as C

import numpy as np
import pytest

import multi_cases as mc

DEVICE_SETS = [[0], [0, 0], [0, 1], [0, 1, 0], [0, 1, 2, 3, 0, 1, 2, 3], [0, 0, 0, 1]]


@pytest.fixture(scope="module")
def table():
    return mc.load_table()


def test_table_is_read_whole(table):
    assert len(table["PartitionCases"]) == 20 and len(table["PiecesCases"]) == 30 and len(table["ScheduleCases"]) == 13
    names = [c[0] for c in table["PartitionCases"]]
    assert "longest * 8 * n == total" in names and "one sample beyond the boundary" in names and "a total of 0 samples" in names


def test_partition_reproduces_the_recorded_table(built_lib, table):
    from speaker_recognition_amd import _lib
    for name, runs, n_active, slots in table["PartitionCases"]:
        off = mc.offsets_of(runs)
        plan = _lib.multi_plan(off, list(range(n_active)), merge=True)
        assert [p["slot"] for p in plan] == list(range(n_active)), name
        assert [p["utts"] for p in plan] == [mc.list_of(s) for s in slots], name
        # slots on one device each their own share without the merge, one queue with it
        same = _lib.multi_plan(off, [0] * n_active, merge=False)
        assert [p["utts"] for p in same] == [p["utts"] for p in plan], name
        one = _lib.multi_plan(off, [0] * n_active, merge=True)
        assert len(one) == 1 and one[0]["utts"] == list(range(len(off) - 1)), name
        for devices in DEVICE_SETS:
            for merge in (False, True):
                mc.check_plan(_lib.multi_plan(off, devices, merge), off, devices, merge)


def test_pieces_reproduce_the_recorded_table(built_lib, table):
    from speaker_recognition_amd import _lib
    seen = set()
    for name, runs, schedule, pieces in table["PiecesCases"]:
        off = mc.offsets_of(runs)
        plan = _lib.multi_plan(off, [0], schedules=[schedule])
        assert len(plan) == 1 and plan[0]["utts"] == list(range(len(off) - 1)), name
        assert plan[0]["pieces"] == [tuple(p) for p in pieces], (name, schedule)
        seen.add((schedule, len(pieces)))
        for devices in DEVICE_SETS:
            sched = [schedule] * len(devices)
            mc.check_plan(_lib.multi_plan(off, devices, True, sched), off, devices, True, sched)
    # one piece, two, fewer utterances than pieces, eight mild ones, four growing ones
    assert {(0, 1), (0, 2), (0, 3), (0, 7), (0, 8), (1, 1), (1, 2), (1, 3), (1, 4)} <= seen
    # a schedule is a slot's own: the second slot's growing pieces leave the first slot's alone
    off = mc.offsets_of([[400, 160000]])
    mixed = _lib.multi_plan(off, [0, 1], schedules=[0, 1])
    assert [len(p["pieces"]) for p in mixed] == [8, 4]
    assert mixed[0] == _lib.multi_plan(off, [0, 1])[0] and mixed[1] == _lib.multi_plan(off, [0, 1], schedules=[1, 1])[1]


def test_invariants_over_random_batches(built_lib):
    from speaker_recognition_amd import _lib
    rng = np.random.default_rng(14)
    for trial in range(300):
        n_utt = int(rng.integers(0, 12 if trial % 4 == 0 else 400))
        scale = 1 << int(rng.integers(4, 21))
        kind = rng.integers(0, 16, n_utt)
        lengths = np.where(kind == 0, 0, np.where(kind == 1, rng.integers(0, scale * 64, n_utt), rng.integers(0, scale, n_utt)))
        off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        devices = DEVICE_SETS[trial % len(DEVICE_SETS)]
        merge = (trial // 6) % 2 == 0
        sched = [int(s) for s in rng.integers(0, 2, len(devices))]
        mc.check_plan(_lib.multi_plan(off, devices, merge, sched), off, devices, merge, sched)


def test_refusals_need_no_device(built_lib):
    from speaker_recognition_amd import _lib
    L = built_lib
    for off, devices, pat in (([1, 5], [0], r"sample_offsets\[0\] must be 0"), ([0, 5, 3], [0], "non-decreasing"),
                              ([0, 5], [], "1 .. 64 slots"), ([0, 5], [0] * 65, "1 .. 64 slots")):
        with pytest.raises(_lib.SRError, match=pat) as e:
            _lib.multi_plan(off, devices)
        assert "HIP" not in str(e.value)
    assert L.sr_multi_plan(None, 0, None, 1, 1, None, None, None, None, None) == -1 and "bad arguments" in _lib.last_error()
    assert L.sr_multi_slot_pieces(None, 0) == -1
    # no utterances: every active slot an empty list and one empty piece
    assert _lib.multi_plan([0], [0, 1]) == [{"slot": 0, "utts": [], "pieces": [(0, 0)]}, {"slot": 1, "utts": [], "pieces": [(0, 0)]}]
    # schedules may be NULL: equal pieces for every slot
    active, counts, utts, pieces = (C.c_int * 1)(), (C.c_int * 1)(), (C.c_int * 1)(), (C.c_int * 17)()
    assert L.sr_multi_plan((C.c_int64 * 1)(0), 0, (C.c_int * 1)(3), 1, 1, None, active, counts, utts, pieces) == 1
    assert active[0] == 0 and counts[0] == 0 and list(pieces)[:3] == [1, 0, 0]
