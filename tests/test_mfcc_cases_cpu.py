"""tests/test_gpu_mfcc_cases.py runs the branches it names and can tell right from wrong -- shown without a GPU, on exactly
its cases and inputs (tests/mfcc_cases.py):

  * sr_mfcc_plan (csrc/mfcc_plan.cpp: what the launchers consume) on 256 compute units returns, for every row of the case table,
    the kernel, template arguments, workgroup shape and CMVN padding the row expects; taken over the table every value of those
    fields that the code can produce occurs, and what cannot occur is named with its reason (mfcc_cases.UNREACHABLE);
  * oracle/mfcc_oracle.py and a second float64 restatement of the chain, written differently on purpose, agree to 1e-9;
  * every named mutant -- one plausible kernel mistake each -- lies at least 20 tolerances away from the oracle on at least one
    compared value of at least one case (the separation table is printed: run with -s);
  * the bounds can be met at all: the oracle's raw cepstra rounded to float32 (what the frame kernels store), then CMVN and deltas
    in float64, stay under a quarter of every bound.
"""
import numpy as np
import pytest

import mfcc_cases as mc

N_CU = 256


@pytest.fixture(scope="module")
def plans(built_lib):
    """{case: (extractor, plan at precision 2, plan at precision 0)} on 256 compute units, 100 frames, mfcc_generic 0"""
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import MfccExtractor
    out = {}
    for c in mc.CASES:
        ex = MfccExtractor(c.fs, **mc.kw(c))
        assert (ex.FRAME_LEN, ex.FRAME_SHIFT) == (mc.frame_len(c), mc.frame_shift(c))
        out[c.name] = (ex, _lib.mfcc_plan(ex._h, 2, 0, 0, 100, N_CU), _lib.mfcc_plan(ex._h, 0, 0, 0, 100, N_CU))
    return out


def _passes(p):
    return sum(1 for n in p["pass_len"] if n > 0)


def test_frame_lengths_are_the_edges_they_name():
    L = {n: mc.frame_len(mc.CASE[n]) for n in ("default_16k", "len512", "len513", "len2048", "lds_22k", "fft32", "fft1024_len640_2f")}
    assert L == {"default_16k": 512, "len512": 512, "len513": 513, "len2048": 2048, "lds_22k": 441, "fft32": 32, "fft1024_len640_2f": 640}
    for c in mc.CASES:
        s = mc.signals(c.name)
        assert [len(x) for x in s[3:]] == [5 * mc.frame_len(c), 5 * mc.frame_len(c) + 1]
        assert all(len(x) > 5 * mc.frame_len(c) for x in s[:3])
        z = np.flatnonzero(s[1] == 0)
        assert len(z) >= 2 * mc.frame_len(c) + 2 * mc.frame_shift(c)            # whole frames of exact zeros: the floor path


def test_plan_returns_the_expected_branch(plans):
    for c in mc.CASES:
        _ex, p2, p0 = plans[c.name]
        e = c.expect
        got = dict(k2=p2["kernel"], k0=p0["kernel"], N1=p0["N1"], NZ1=p0["NZ1"], preset=p0["preset"], wpb0=p0["wpb"], wpb2=p2["wpb"],
                   cp=p0["cp"], passes=_passes(p0), past_nc=p0["max_read"] > c.fft // 2)
        for k, v in e.items():
            assert got[k] == v, (c.name, k, got[k], v)
        assert p2["cp"] == p0["cp"] and p2["pass_len"] == p0["pass_len"]
        if p2["kernel"] == mc.F64F:
            assert (p2["N1"], p2["NZ1"], p2["preset"]) == (16, 4, p0["preset"]), c.name
        assert p0["n_empty"] == 0, c.name                                       # (an empty band: ln 0 in the reference, out of scope)
        assert p0["lds"] <= 160 * 1024 and p2["lds"] <= 160 * 1024


def test_forced_generic_plans_the_generic_kernels(plans):
    from speaker_recognition_amd import _lib
    for c in mc.CASES:
        ex = plans[c.name][0]
        assert _lib.mfcc_plan(ex._h, 2, 1, 1, 100, N_CU)["kernel"] == mc.F64G
        assert _lib.mfcc_plan(ex._h, 0, 1, 1, 100, N_CU)["kernel"] == mc.F32G


def test_branch_census(plans):
    """every value of each plan field that the code can produce occurs in the table; what cannot is in mc.UNREACHABLE"""
    seen = {k: set() for k in ("kernel", "N1", "NZ1", "N1/NZ1", "preset", "wpb0", "wpb2f", "wpb2g", "cp", "passes", "preset/kernel")}
    takes_preset = {}
    for c in mc.CASES:
        _ex, p2, p0 = plans[c.name]
        seen["kernel"] |= {p2["kernel"], p0["kernel"]}
        seen["cp"].add(p0["cp"])
        if p0["kernel"] == mc.F32F:
            seen["N1"].add(p0["N1"])
            seen["NZ1"].add(p0["NZ1"])
            seen["N1/NZ1"].add((p0["N1"], p0["NZ1"]))
            seen["preset"].add(p0["preset"])
            seen["wpb0"].add(p0["wpb"])
            seen["passes"].add(_passes(p0))
            seen["preset/kernel"].add((p0["preset"], mc.F32F))
            takes_preset.setdefault(p0["preset"], c.name)
        if p2["kernel"] == mc.F64F:
            seen["wpb2f"].add(p2["wpb"])
            seen["preset/kernel"].add((p2["preset"], mc.F64F))
        else:
            seen["wpb2g"].add(p2["wpb"])
    assert seen["kernel"] == {mc.F32F, mc.F32G, mc.F64F, mc.F64G}
    assert seen["N1"] == {16, 8, 4} and seen["NZ1"] == {4, 8, 16}
    # every (N1, NZ1) the launcher's switch can name, minus the ones no frame length selects
    switch = {(16, 4), (16, 16), (8, 4), (8, 8), (4, 4)}
    assert seen["N1/NZ1"] == switch
    for n1 in (16, 8, 4):
        for nz in (4, 8, 16):
            assert ((n1, nz) in switch) != (("N1/NZ1", (n1, nz)) in mc.UNREACHABLE), (n1, nz)
    assert seen["preset"] == {0, 1} and ("preset", 2) in mc.UNREACHABLE
    assert seen["preset/kernel"] == {(0, mc.F32F), (1, mc.F32F), (0, mc.F64F), (1, mc.F64F)}
    assert seen["wpb0"] == {4, 12}
    assert seen["wpb2f"] == {8} and seen["wpb2g"] == {4, 1} and ("wpb2", 2) in mc.UNREACHABLE
    assert seen["cp"] == {16, 32, 64}
    assert seen["passes"] == {1, 2, 3, 4}
    # the configuration that takes each preset
    assert takes_preset == {1: "default_16k", 0: "default_8k"}
    # fp32 fast with 4 waves for each of its two reasons: long frames (NZ1 > 4) and a mel table too large for 12 waves (NZ1 4)
    four = {(plans[c.name][2]["NZ1"] > 4) for c in mc.CASES if plans[c.name][2]["kernel"] == mc.F32F and plans[c.name][2]["wpb"] == 4}
    assert four == {True, False}
    # f64 generic chosen for each of its reasons: FFT size, frame length, LDS (FFT 2048, frames <= 512, n_ceps <= 16), n_ceps
    lds_only = [c.name for c in mc.CASES if plans[c.name][1]["kernel"] == mc.F64G and c.fft == 2048 and mc.frame_len(c) <= 512 and c.n_ceps <= 16]
    assert set(lds_only) == {"lds_2f", "lds_3f", "lds_22k", "lds_17f"}
    for n in lds_only:                                     # the fast kernel has room for 5104 padded floats
        assert plans[n][2]["pad_floats"] > 5104
    assert all(plans[c.name][2]["pad_floats"] <= 5104 for c in mc.CASES if plans[c.name][1]["kernel"] == mc.F64F)


def test_padded_sweeps_stay_inside_the_power_spectrum_region(plans):
    past = []
    for c in mc.CASES:
        _ex, p2, p0 = plans[c.name]
        if p0["kernel"] == mc.F32F or p2["kernel"] == mc.F64F:
            assert p0["max_read"] < 1100, (c.name, p0["max_read"])
            if p0["max_read"] > c.fft // 2:
                past.append(c.fft)
    assert {512, 1024, 2048} <= set(past)                  # at least one row per fast FFT size reads beyond bin NC


def test_frames_per_wave_branches(plans):
    from speaker_recognition_amd import _lib
    ex = plans["default_16k"][0]
    fpw = lambda precision, n: _lib.mfcc_plan(ex._h, precision, 0, 0, n, N_CU)["frames_per_wave"]
    r0, r2 = N_CU * 12, N_CU * 8                                                # one round of waves: fp32 (one 12-wave workgroup per CU), float64
    got0 = [fpw(0, n) for n in (1, r0, r0 + 1, 8 * r0 + 1, 40 * r0)]
    assert got0 == [1, 1, 2, 8, 10]                                             # 1, 2, the floor of 8, and more than 8 (four rounds of 10)
    got2 = [fpw(2, n) for n in (1, r2, r2 + 1, 8 * r2 + 1, 40 * r2, 200 * r2)]
    assert got2 == [1, 1, 2, 9, 40, 50]                                         # one round up to 40 frames per wave; 200 rounds' worth: four rounds of 50
    # grid: every frame has a wave, no workgroup is idle
    for precision, wpb in ((0, 12), (2, 8)):
        for n in (1, 777, r0 + 1, 40 * r0):
            p = _lib.mfcc_plan(ex._h, precision, 0, 0, n, N_CU)
            assert p["wpb"] == wpb and p["grid"] * wpb * p["frames_per_wave"] >= n > (p["grid"] - 1) * wpb * p["frames_per_wave"]


# ---------------------------------------------------------------- the comparison itself ---------------------------------------
def _units(c, raw, feats, ref):
    """largest error in units of the precision-2 tolerance, and where"""
    worst = (0.0, None)
    for q, (err, scale) in mc.errors(c, raw, feats, ref).items():
        u = err / (mc.tolerance(2, q) * scale)
        if u > worst[0]:
            worst = (u, q)
    return worst


def test_two_restatements_agree():
    worst = 0.0
    for c in mc.CASES:
        for kind in ("int16", "float32"):
            for s, ref in zip(mc.pcm(c.name, kind), mc.reference(c.name, kind)):
                if ref is None:
                    continue
                raw, feats = mc.second(c, s)
                for q, (err, _scale) in mc.errors(c, raw, feats, ref).items():
                    worst = max(worst, err)
                    assert err < mc.AGREE, (c.name, kind, q, err)
    print("\nrestatements agree to %.1e" % worst)


def test_every_mutant_is_caught():
    rows = []
    for m in mc.MUTANTS:
        best = (0.0, None, None)
        for c in mc.CASES:
            for s, ref in zip(mc.pcm(c.name, "int16"), mc.reference(c.name, "int16")):
                if ref is None:
                    continue
                raw, feats = mc.second(c, s, mutant=m)
                u, q = _units(c, raw, feats, ref)
                if u > best[0]:
                    best = (u, c.name, q)
            if best[0] >= 1e4:          # far enough: no need to walk the rest of the table for this one
                break
        rows.append((m, best))
        assert best[0] >= mc.MUTANT_FACTOR, (m, best)
    print("\nmutant                        tolerances  case / quantity\n" +
          "\n".join("  %-26s %12.0f  %s / %s" % (m, b[0], b[1], b[2]) for m, b in rows))


def test_preemph_default_mutant_is_invisible_at_the_default():
    """why the pre-emphasis rows exist: at 0.95 a kernel with the constant baked in is the oracle itself"""
    c = mc.CASE["default_16k"]
    s, ref = mc.pcm(c.name, "int16")[0], mc.reference(c.name, "int16")[0]
    raw, feats = mc.second(c, s, mutant="preemph_default")
    assert _units(c, raw, feats, ref)[0] < 1e-3
    for name in ("pre0", "pre05", "pre097", "pre1"):
        c = mc.CASE[name]
        s, ref = mc.pcm(name, "int16")[0], mc.reference(name, "int16")[0]
        raw, feats = mc.second(c, s, mutant="preemph_default")
        assert _units(c, raw, feats, ref)[0] >= mc.MUTANT_FACTOR, name


def test_reference_rounded_to_float32_meets_a_quarter_of_each_bound():
    """the frame kernels store raw cepstra as float32: the floor of what they can reach"""
    worst = {}
    for c in mc.CASES:
        for kind in ("int16", "float32"):
            for ref in mc.reference(c.name, kind):
                if ref is None:
                    continue
                raw32 = ref["raw"].astype(np.float32).astype(np.float64)
                feats = {nd: mc.second_features(raw32, nd) for nd in (0, 1, 2)}
                for q, (err, scale) in mc.errors(c, raw32, feats, ref).items():
                    for precision in (2, 0):
                        assert err < 0.25 * mc.tolerance(precision, q) * scale, (c.name, kind, q, err)
                    key = q.split("_")[0]
                    if err / scale > worst.get(key, (0.0, None))[0]:
                        worst[key] = (err / scale, c.name)
    print("\nfloat32 rounding of the raw cepstra alone: " + ", ".join("%s %.1e (%s)" % (k, v[0], v[1]) for k, v in sorted(worst.items())))


def test_sample_frames_covers_first_last_and_boundaries():
    off = np.concatenate(([0], np.cumsum([0, 3, 0, 40, 7, 0, 90, 5, 0, 120, 30, 2, 0])))
    pick = mc.sample_frames(off, 200)
    assert pick[0] == 1 and pick[-1] == 11 and sum(off[u + 1] - off[u] for u in pick) >= 200
