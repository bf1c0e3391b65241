"""tests/test_gpu_frontend.py can tell right from wrong -- shown without a GPU, on exactly its inputs (tests/frontend_cases.py):

  * each oracle (oracle/lpc_oracle.py, oracle/ltsd_oracle.py) and its second float64 restatement, written differently on purpose,
    agree far inside the GPU tolerance;
  * every named mutant -- one subtle kernel mistake each -- lies at least 20 GPU tolerances away from the oracle on at least one
    value its test compares (the tolerances are themselves 10-30 float32 output roundings; 20 keeps a mutant's effect clear of a
    kernel that merely sits at the tolerance's edge).  The separation factors are printed (run with -s);
  * the caps the GPU tests put on what they leave unpinned hold for the restatements alone.

The float32 direct DFT at large N: the existing LTSD tolerances (2e-3 dB, 1e-4 relative on the noise spectrum) were set at
N <= 743.  frontend_cases.emulate_ltsd_f32 runs the kernels' arithmetic on the CPU (float32 window and twiddle ring, sequential
float32 FMA sums, float32 sqrt, float64 weighted sum); its error against the oracle on the raw-window inputs, order 1:

      N      371      743      1024     2048     2229     4096
      dB   1.8e-06  2.0e-06  3.5e-06  4.1e-06  8.8e-06  9.0e-06

-- 200 times under 2e-3 dB at N = 4096, so the bound stays as it is at every N (test_ltsd_f32_emulation_is_far_inside)."""
import numpy as np
import pytest

import frontend_cases as fc
from oracle import lpc_oracle, ltsd_oracle

AGREE_LPC = fc.LPC_TOL / 100            # measured: 1e-13 .. 7e-10 (resonances of radius 0.995: condition up to 1e7)
AGREE_LTSD_DB = 1e-9                    # measured: 7e-15 dB
AGREE_NOISE_REL = 1e-12                 # measured: 9e-16


def _table(title, rows):
    print("\n%s\n" % title + "\n".join("    %-18s %12.0f x tolerance   (%s)" % r for r in rows))


@pytest.fixture(scope="module")
def lpc_instances():
    """{(order, fs, win_ms, pcm type): (signal, oracle rows)} for every case of test_lpc_every_instance_vs_oracle"""
    out = {}
    for fs, win_ms, frame_len, _spl in fc.LPC_FRAMES:
        sig = fc.lpc_signal(fs, frame_len)
        for name, s in (("int16", sig), ("float32", fc.as_float_pcm(sig))):
            for order in fc.LPC_ORDERS:
                out[(order, fs, win_ms, name)] = (s, lpc_oracle.extract(fs, s, n_lpc=order, **fc.lpc_kw(win_ms)))
    return out


def test_frame_configurations_select_what_they_name():
    for fs, win_ms, frame_len, spl in fc.LPC_FRAMES:
        ex = lpc_oracle.LPCExtractor(fs, **fc.lpc_kw(win_ms))
        assert ex.FRAME_LEN == frame_len and ex.FRAME_SHIFT == frame_len // 2
        need = (frame_len + 63) // 64
        assert (8 if need <= 8 else 16 if need <= 16 else 32) == spl        # lpc_extract_into's choice
    assert {c[3] for c in fc.LPC_FRAMES} == {8, 16, 32}
    fs, win_ms, frame_len = fc.LPC_TOO_LONG
    assert lpc_oracle.LPCExtractor(fs, **fc.lpc_kw(win_ms)).FRAME_LEN == frame_len > 64 * 32
    assert [ltsd_oracle.window_size(fs) for fs in fc.LTSD_RATES] == [371, 512, 743, 1024, 1486, 2048, 2229]


def test_lpc_oracle_and_toeplitz_restatement_agree(lpc_instances):
    worst = 0.0
    for (order, fs, win_ms, _name), (sig, ref) in lpc_instances.items():
        sec = fc.lpc_second(fs, sig, n_lpc=order, **fc.lpc_kw(win_ms))
        assert sec.shape == ref.shape and len(ref) >= 20
        worst = max(worst, float(fc.lpc_metric(sec, ref).max()))
    print("\nLPC oracle vs direct lag sums + solve_toeplitz, %d cases: worst %.2e" % (len(lpc_instances), worst))
    assert worst < AGREE_LPC, worst


def test_every_lpc_mutant_is_seen(lpc_instances):
    rows = []
    for mutant in fc.LPC_MUTANTS:
        if mutant == "shift_plus_one":
            continue
        sep = {}
        for (order, fs, win_ms, name), (sig, ref) in lpc_instances.items():
            mu = fc.lpc_second(fs, sig, n_lpc=order, mutant=mutant, **fc.lpc_kw(win_ms))
            sep[(order, fs, win_ms, name)] = float(fc.lpc_metric(mu, ref).max()) / fc.LPC_TOL
        # a kernel instance with this mistake must not get through: the mutant is seen in EVERY parametrised case
        case = min(sep, key=sep.get)
        rows.append((mutant, sep[case], "weakest of %d cases: order %d, %d Hz, %g ms, %s" % ((len(sep),) + case)))
    _table("LPC mutants vs test_lpc_every_instance_vs_oracle", rows)
    for mutant, sep, _where in rows:
        assert sep >= fc.MUTANT_FACTOR, (mutant, sep)


def test_ragged_batch_has_what_its_test_needs_and_sees_the_shift_mutant():
    sigs = fc.ragged_batch()
    frames = np.array([(len(s) - 80) // 320 + 1 if len(s) > 400 else 0 for s in sigs])
    assert len(sigs) >= 40 and (frames[:4] == 0).all() and (frames[-3:] == 0).all()
    agree, sep, n_utt = 0.0, [], 0
    for u, s in enumerate(sigs):
        if frames[u] == 0:
            continue
        ref = lpc_oracle.extract(fc.RAGGED_FS, s, **fc.RAGGED_KW)
        assert len(ref) == frames[u]
        agree = max(agree, float(fc.lpc_metric(fc.lpc_second(fc.RAGGED_FS, s, **fc.RAGGED_KW), ref).max()))
        mu = fc.lpc_second(fc.RAGGED_FS, s, mutant="shift_plus_one", utt_index=u, **fc.RAGGED_KW)
        if frames[u] >= 2:
            sep.append(float(fc.lpc_metric(mu, ref).max()) / fc.LPC_TOL)
            n_utt += 1
    _table("LPC mutant vs test_lpc_ragged_batch_vs_oracle_and_alone", [("shift_plus_one", min(sep), "weakest of %d utterances with 2+ frames" % n_utt)])
    assert agree < AGREE_LPC, agree
    assert min(sep) >= fc.MUTANT_FACTOR, min(sep)


def test_degenerate_frames_are_pinned_by_the_restatements():
    sig, inside = fc.degenerate_signal()
    assert set(inside) == set(fc.DEGENERATE_CLASSES)
    for order in fc.DEGENERATE_ORDERS:
        ref = lpc_oracle.extract(fc.DEGENERATE_FS, sig, n_lpc=order, **fc.DEGENERATE_KW)
        sec = fc.lpc_second(fc.DEGENERATE_FS, sig, n_lpc=order, **fc.DEGENERATE_KW)
        d = fc.lpc_metric(sec, ref).max(axis=1)
        unpinned = d >= fc.LPC_TOL
        print("\ndegenerate frames, order %d: %d of %d unpinned; per class: %s" % (
            order, int(unpinned.sum()), len(ref), ", ".join("%s %.1e" % (n, d[f].max()) for n, f in inside.items())))
        assert np.mean(unpinned) <= fc.UNPINNED_CAP
        nan_rows = np.isnan(fc.lpc_second(fc.DEGENERATE_FS, sig, n_lpc=order, keep_nan=True, **fc.DEGENERATE_KW)).any(axis=1)
        assert nan_rows.sum() >= 2 and np.all(ref[nan_rows] == 0.0)          # the all-zero frames beside the impulse: NaN -> 0


@pytest.fixture(scope="module")
def ltsd_cases():
    """[(tag, N, order, signals, oracle noise spectrum [N], oracle values per signal)]: every int16 case of the two value tests"""
    out = []
    for fs in fc.LTSD_RATES:
        N = ltsd_oracle.window_size(fs)
        na = ltsd_oracle.noise_spectrum(fc.ltsd_noise(N), N)
        for order in fc.LTSD_ORDERS:
            sigs = fc.ltsd_batch(N, order)
            out.append(("fs=%d" % fs, N, order, sigs, na, [ltsd_oracle.ltsd(s, na, N, order) for s in sigs]))
    for N in fc.LTSD_RAW_N:
        na = ltsd_oracle.noise_spectrum(fc.raw_window_noise(N), N)
        sigs = fc.raw_window_batch(N)
        out.append(("raw", N, 1, sigs, na, [ltsd_oracle.ltsd(s, na, N, 1) for s in sigs]))
    return out


def test_ltsd_oracle_and_half_spectrum_restatement_agree(ltsd_cases):
    worst, worst_n = 0.0, 0.0
    for tag, N, order, sigs, na, want in ltsd_cases:
        NB = N // 2 + 1
        noise = fc.raw_window_noise(N) if tag == "raw" else fc.ltsd_noise(N)
        worst_n = max(worst_n, float(np.max(np.abs(fc.noise_second(noise, N) - na[:NB]) / na[:NB])))
        for s, w in zip(sigs, want):
            sec = fc.ltsd_second(s, na[:NB], N, order)
            assert sec.shape == w.shape
            if len(w):
                worst = max(worst, float(np.max(np.abs(sec - w))))
    print("\nLTSD oracle vs half spectrum with mirror weights, %d cases: worst %.2e dB, noise spectrum %.2e relative" % (
        len(ltsd_cases), worst, worst_n))
    assert worst < AGREE_LTSD_DB and worst_n < AGREE_NOISE_REL


def test_every_ltsd_mutant_is_seen(ltsd_cases):
    rows = []
    for mutant in fc.LTSD_MUTANTS:
        best, where, seen_in = 0.0, None, 0
        for tag, N, order, sigs, na, want in ltsd_cases:
            sep = 0.0
            for s, w in zip(sigs, want):
                if len(w):
                    sep = max(sep, float(np.max(np.abs(fc.ltsd_second(s, na[:N // 2 + 1], N, order, mutant=mutant) - w))) / fc.LTSD_TOL_DB)
            seen_in += sep >= fc.MUTANT_FACTOR
            if sep > best:
                best, where = sep, "%s N=%d order=%d" % (tag, N, order)
        rows.append((mutant, best, "clearest in %s; 20+ in %d of %d cases" % (where, seen_in, len(ltsd_cases))))
    _table("LTSD mutants vs test_ltsd_values_at_every_rate_and_order / test_ltsd_raw_window_sizes", rows)
    for mutant, best, _where in rows:
        assert best >= fc.MUTANT_FACTOR, (mutant, best)
    # where a mutant can be seen at all, it is: the Nyquist weight at every even N, the rounded hop at every odd N, the DC
    # weight and the envelope at every rate
    for tag, N, order, sigs, na, want in ltsd_cases:
        if tag == "raw":
            continue
        muts = ["dc_weight_2", "nyquist_weight_2" if N % 2 == 0 else "hop_rounded_up"] + (["envelope_open", "edge_rule"] if order else [])
        for mutant in muts:
            sep = max(float(np.max(np.abs(fc.ltsd_second(s, na[:N // 2 + 1], N, order, mutant=mutant) - w))) for s, w in zip(sigs, want) if len(w))
            assert sep / fc.LTSD_TOL_DB >= fc.MUTANT_FACTOR, (mutant, N, order, sep)


def test_ltsd_batches_hold_the_edge_cases(ltsd_cases):
    for tag, N, order, sigs, na, want in ltsd_cases:
        wn = [len(w) for w in want]
        if tag != "raw":
            assert 0 in wn and 2 * order in wn and 2 * order + 1 in wn
            assert max(want[0].max(), want[1].max()) > 20.0
        for w in want:
            interior = w[order:len(w) - order] if len(w) > 2 * order else w[:0]
            assert np.all(interior != 0) and np.all(np.isfinite(w))


def test_zero_noise_bins_give_all_three_classes():
    N, order = 512, 5
    sigs, zero_bins = fc.zero_bin_case(N, order)
    na = ltsd_oracle.noise_spectrum(fc.ltsd_noise(N), N)
    for k in zero_bins:
        na[k] = na[(N - k) % N] = 0.0
    with np.errstate(all="ignore"):
        want = np.concatenate([ltsd_oracle.ltsd(s, na, N, order) for s in sigs])
    assert np.isnan(want).any() and np.isposinf(want).any() and np.isfinite(want).any() and not np.isneginf(want).any()


def test_vad_scenes_keep_clear_of_the_thresholds():
    """the cap of test_vad_intervals_at_44100_vs_the_oracle, for the restatements alone: no window within the value tolerance of
    a threshold, and the second restatement decides as the oracle does"""
    from speaker_recognition_amd.filters.ltsd import voiced_runs
    scenes, noise = fc.vad_scene()
    N = ltsd_oracle.window_size(fc.VAD_FS)
    na, lam0, lam1 = ltsd_oracle.thresholds(noise, N)
    n_near = n_all = n_runs = 0
    for sc in scenes:
        l = ltsd_oracle.ltsd(sc, na, N)
        # the device's thresholds are its own (1.1 x its maximum over the noise): within 1.1 tolerances of the oracle's
        n_near += int(fc.near_threshold(l, lam0, lam1, tol=(1.0 + 2.2) * fc.LTSD_TOL_DB).sum())
        n_all += len(l)
        runs = voiced_runs(l, lam0, lam1)
        n_runs += len(runs)
        assert voiced_runs(fc.ltsd_second(sc, na[:N // 2 + 1], N), lam0, lam1) == runs
    print("\nVAD scenes at %d Hz: %d windows, %d runs, %d near a threshold (lambda0 %.3f dB)" % (fc.VAD_FS, n_all, n_runs, n_near, lam0))
    assert n_runs >= 4 and n_near <= fc.NEAR_CAP * n_all


@pytest.mark.parametrize("N", [371, 743, 1024, 2048, 2229, 4096])
def test_ltsd_f32_emulation_is_far_inside(N):
    """4 x the emulated float32 error stays under the existing bound at every N: the bound needs no widening at N > 743."""
    sig = fc.raw_window_batch(N)[0]
    na = ltsd_oracle.noise_spectrum(fc.raw_window_noise(N), N)
    want = ltsd_oracle.ltsd(sig, na, N, 1)
    err = float(np.max(np.abs(fc.emulate_ltsd_f32(sig, na[:N // 2 + 1], N, 1) - want)))
    print("\nemulated float32 LTSD, N = %d: %.2e dB" % (N, err))
    assert 4.0 * err < fc.LTSD_TOL_DB, err
