"""The two front-end kernels that had one oracle comparison each -- LPC (csrc/lpc.hip) and LTSD (csrc/ltsd.hip) -- at every
instance that is built, against the float64 oracles (oracle/lpc_oracle.py, oracle/ltsd_oracle.py, oracle/mfcc_oracle.py) on
the inputs of tests/frontend_cases.py.  tests/test_frontend_cases_cpu.py shows on the same inputs that these comparisons tell
a subtly wrong kernel from a right one (every named mutant lies 20+ tolerances away from the oracle).

Coverage, by name:
  lpc_frames_kernel<PcmT, SPL, ORDER>: PcmT int16 and float32; SPL 8 (frames of 256 / 400 / 512 samples), SPL 16 (640 / 1024),
      SPL 32 (1102 / 1764 / 2048; SPL 32 x ORDER 20 is the one instance above 64 KB of LDS); ORDER 10, 12, 15, 16, 20;
      the utterance walk of a wave over ragged batches with zero-frame utterances, and frames_per_wave > 8.
  ltsd_amp_kernel<PcmT>, ltsd_reduce_kernel: PcmT int16 and float32; N = 371, 743, 2229 (odd), 512, 1024, 1486, 2048 (even:
      the Nyquist bin's weight of 1), raw N = 4, 5, 4095, 4096; order 0, 1, 5, 12; a noise spectrum with zero bins.
  vad_compact_kernel and the stream at 16 kHz and 22.05 kHz: tests/test_gpu_stream_vad.py; LTSD_VAD.filter at 44.1 kHz here.

Tolerances are the existing tests' (frontend_cases.LPC_TOL, LTSD_TOL_DB, NOISE_TOL_REL); every test prints its worst figure
("PARITY ..." lines, run with -s) before it asserts.  The LTSD bounds were set at N <= 743; the kernels' arithmetic emulated on
the CPU (frontend_cases.emulate_ltsd_f32: float32 window, ring and sequential FMA sums) stays within 1e-5 dB of the oracle up
to N = 4096 (table in tests/test_frontend_cases_cpu.py), so 2e-3 dB holds there without change."""
import re

import numpy as np
import pytest

import frontend_cases as fc

pytestmark = pytest.mark.gpu


def _report(case, what, value, bound):
    print("PARITY %-58s %-22s %.3e  (bound %.1e)" % (case, what, value, bound))


# ------------------------------------------------------------------ (a) LPC, every instance ------------------------------------
@pytest.mark.parametrize("pcm_type", ["int16", "float32"])
@pytest.mark.parametrize("fs,win_ms,frame_len,spl", fc.LPC_FRAMES, ids=["fs%d-%dms-L%d-SPL%d" % c for c in fc.LPC_FRAMES])
@pytest.mark.parametrize("order", fc.LPC_ORDERS)
def test_lpc_every_instance_vs_oracle(built_lib, order, fs, win_ms, frame_len, spl, pcm_type):
    from oracle import lpc_oracle as lo, mfcc_oracle as mo
    from speaker_recognition_amd.feature import LPC, mix_feature
    kw = fc.lpc_kw(win_ms)
    sig = fc.lpc_signal(fs, frame_len)
    if pcm_type == "float32":
        sig = fc.as_float_pcm(sig)
    ref_l = lo.extract(fs, sig, n_lpc=order, **kw)
    ref_m = mo.extract(fs, sig, **kw)
    assert lo.LPCExtractor(fs, n_lpc=order, **kw).FRAME_LEN == frame_len and (frame_len + 63) // 64 <= spl
    assert spl == 8 or (frame_len + 63) // 64 > spl // 2                   # the case selects the SPL it names
    only = LPC.extract(fs, sig, n_lpc=order, **kw)
    mix = mix_feature((fs, sig), n_lpc=order, **kw)
    assert only.shape == ref_l.shape and mix.shape == (ref_m.shape[0], 13 + order)
    err = float(fc.lpc_metric(only, ref_l).max())
    err_m = float(np.max(np.abs(mix[:, :13] - ref_m)))
    _report("lpc order=%d fs=%d L=%d SPL=%d %s" % (order, fs, frame_len, spl, pcm_type), "lpc / mfcc cols", err, fc.LPC_TOL)
    assert np.all(np.isfinite(only))
    assert err < fc.LPC_TOL, err
    assert np.array_equal(only, mix[:, 13:])
    assert err_m < 1e-3, err_m                                             # the MFCC half of mix_feature (the existing test's bound)
    if pcm_type == "int16":
        # the same samples as float32 PCM: both instances convert a sample to float64 first, so the rows are the same bits
        assert np.array_equal(LPC.extract(fs, sig.astype(np.float32), n_lpc=order, **kw), only)


def test_lpc_refusals(built_lib):
    from speaker_recognition_amd import synth
    from speaker_recognition_amd._lib import SRError
    from speaker_recognition_amd.core import MfccExtractor
    from speaker_recognition_amd.feature import LPC, mix_feature
    for order in fc.LPC_UNBUILT_ORDERS:
        with pytest.raises(SRError, match="LPC order %d is not instantiated" % order):
            MfccExtractor(16000, n_lpc=order)
        with pytest.raises(SRError, match="LPC order %d is not instantiated" % order):
            LPC.extract(16000, synth.synth_speech(1, 0.5, 16000), n_lpc=order)
    fs, win_ms, frame_len = fc.LPC_TOO_LONG
    sig = fc.lpc_signal(fs, frame_len, n_frames=12)
    ex = MfccExtractor(fs, win_length_ms=win_ms, win_shift_ms=win_ms / 2.0, FFT_SIZE=4096, n_lpc=15)
    assert ex.FRAME_LEN == frame_len > 2048
    with pytest.raises(SRError, match="frame of %d samples is too long for the LPC kernel" % frame_len):
        ex.extract(sig)
    with pytest.raises(SRError, match="too long for the LPC kernel"):
        mix_feature((fs, sig), win_length_ms=win_ms, win_shift_ms=win_ms / 2.0, FFT_SIZE=4096)
    # the MFCC half alone takes that frame
    assert MfccExtractor(fs, win_length_ms=win_ms, win_shift_ms=win_ms / 2.0, FFT_SIZE=4096).extract(sig).shape[1] == 13
    for order, win in ((20, 2), (16, 2), (10, 1)):                          # frames of 16, 16 and 8 samples at 8 kHz
        ex = MfccExtractor(8000, win_length_ms=win, win_shift_ms=win, n_lpc=order)
        assert order >= ex.FRAME_LEN
        with pytest.raises(SRError, match="LPC order %d needs a longer frame" % order):
            ex.extract(fc.lpc_signal(8000, 256, n_frames=4))
    # and the extractor still works afterwards
    test_lpc_every_instance_vs_oracle(built_lib, 15, 8000, 32, 256, 8, "int16")


# ------------------------------------------------------------------ (b) LPC, ragged batches ------------------------------------
def _cu_count():
    from speaker_recognition_amd import _lib
    m = re.search(r"(\d+) CUs", _lib.device_name())
    assert m, _lib.device_name()
    return int(m.group(1))


def test_lpc_ragged_batch_vs_oracle_and_alone(built_lib):
    """10 ms frames every 40 ms: most utterances have 2..5 frames and runs of them have none, so the 8 consecutive frames of one
    wave cross several utterance boundaries, empty utterances included (`while (frame >= utt_f1)`, the binary search over
    repeated frame_off values)."""
    from oracle import lpc_oracle as lo
    from speaker_recognition_amd.core import Batch, MfccExtractor
    fs, kw = fc.RAGGED_FS, fc.RAGGED_KW
    sigs = fc.ragged_batch()
    ex = MfccExtractor(fs, n_lpc=15, **kw)
    assert ex.FRAME_LEN == 80 and ex.FRAME_SHIFT == 320
    out = ex.extract_batch(Batch.from_pcm(sigs), nd=0, cmvn=False)
    X, off = out.download(), out.offsets()
    want_frames = [(len(s) - 80) // 320 + 1 if len(s) > 5 * 80 else 0 for s in sigs]
    assert len(sigs) >= 40 and np.array_equal(np.diff(off), want_frames)
    empty = np.array(want_frames) == 0
    assert empty[:4].all() and empty[-3:].all() and np.any(empty[10:-10][:-1] & empty[10:-10][1:])     # runs at start, end, middle
    # a wave's range [8 w, 8 w + 8) holds frames of 3+ utterances somewhere, with an empty utterance between two of them
    utt_of = np.repeat(np.arange(len(sigs)), want_frames)
    spans = [utt_of[f:f + 8] for f in range(0, len(utt_of), 8)]
    assert max(len(set(s.tolist())) for s in spans) >= 3
    assert any(np.any(empty[s.min():s.max() + 1]) for s in spans)
    worst = 0.0
    for u, s in enumerate(sigs):
        got = X[off[u]:off[u + 1]]
        if want_frames[u] == 0:
            continue
        ref = lo.extract(fs, s, **kw)
        assert got[:, 13:].shape == ref.shape
        worst = max(worst, float(fc.lpc_metric(got[:, 13:], ref).max()))
        alone = ex.extract_batch(Batch.from_pcm([s]), nd=0, cmvn=False).download()
        assert np.array_equal(alone, got), u                                # bit-identical: rows do not depend on the batch
    _report("lpc ragged batch (%d utterances, %d frames)" % (len(sigs), len(X)), "lpc", worst, fc.LPC_TOL)
    assert worst < fc.LPC_TOL, worst
    # float32 PCM of the same samples: the same bits
    Xf = ex.extract_batch(Batch.from_pcm([s.astype(np.float32) for s in sigs]), nd=0, cmvn=False).download()
    assert np.array_equal(Xf[:, 13:], X[:, 13:])


def test_lpc_more_than_eight_frames_per_wave(built_lib):
    """The launch takes at most 32 waves per CU, so beyond 8 * 32 * n_cu frames a wave walks more than 8 (frames_per_wave);
    the first and last frame of every wave's range, and a stride through the rest, against the oracle."""
    from oracle import lpc_oracle as lo
    from speaker_recognition_amd.core import Batch, MfccExtractor
    n_cu = _cu_count()
    max_waves = n_cu * 32
    sigs, kw = fc.large_batch(int(8 * max_waves * 1.3))
    fs = fc.RAGGED_FS
    ex = MfccExtractor(fs, n_lpc=15, **kw)
    out = ex.extract_batch(Batch.from_pcm(sigs), nd=0, cmvn=False)
    X, off = out.download(), out.offsets()
    NF = len(X)
    want_frames = [(len(s) - 80) // 80 + 1 if len(s) > 400 else 0 for s in sigs]
    assert np.array_equal(np.diff(off), want_frames)
    fpw = max(8, -(-NF // max_waves))                                       # lpc_extract_into
    assert fpw > 8, (NF, n_cu, fpw)
    firsts = np.arange(0, NF, fpw)
    lasts = np.minimum(firsts + fpw, NF) - 1
    pick = np.unique(np.concatenate([firsts, lasts, np.arange(0, NF, 37), off[:-1][np.diff(off) > 0], off[1:][np.diff(off) > 0] - 1]))
    assert len(pick) >= 2000
    oex = lo.LPCExtractor(fs, **kw)
    utt = np.searchsorted(off, pick, side="right") - 1
    worst = 0.0
    for u in np.unique(utt):
        sel = pick[utt == u]
        ref = fc.lpc_frame_oracle(oex, sigs[u], sel - off[u])
        worst = max(worst, float(fc.lpc_metric(X[sel, 13:], ref).max()))
    _report("lpc large batch (%d CUs, %d frames, %d per wave, %d compared)" % (n_cu, NF, fpw, len(pick)), "lpc", worst, fc.LPC_TOL)
    assert np.all(np.isfinite(X))
    assert worst < fc.LPC_TOL, worst


# ------------------------------------------------------------------ (c) LPC, degenerate frames ---------------------------------
@pytest.mark.parametrize("order", fc.DEGENERATE_ORDERS)
def test_lpc_degenerate_frames(built_lib, order):
    """Constant, square-wave, dither, impulse and sinusoid frames inside ordinary speech.  Where the two float64 restatements
    agree within the tolerance the value is pinned and the device must agree too; elsewhere only what the reference fixes is
    asserted (NaN -> 0.0 exactly, no NaN).  The Hamming window keeps every such frame's system regular enough for the two to
    agree (measured: 3e-11 at worst), so the unpinned share is 0 of 263 frames; the cap of 5 % is asserted."""
    from oracle import lpc_oracle as lo
    from speaker_recognition_amd.feature import LPC
    fs, kw, L = fc.DEGENERATE_FS, fc.DEGENERATE_KW, fc.DEGENERATE_L
    sig, inside = fc.degenerate_signal()
    ref = lo.extract(fs, sig, n_lpc=order, **kw)
    sec = fc.lpc_second(fs, sig, n_lpc=order, **kw)
    got = LPC.extract(fs, sig, n_lpc=order, **kw)
    assert got.shape == ref.shape and not np.any(np.isnan(got))
    pinned = fc.lpc_metric(sec, ref).max(axis=1) < fc.LPC_TOL
    assert np.mean(~pinned) <= fc.UNPINNED_CAP, int(np.sum(~pinned))
    err = fc.lpc_metric(got, ref).max(axis=1)
    ordinary = np.ones(len(ref), bool)
    for name, frames in inside.items():
        assert len(frames) >= 3
        ordinary[frames] = False
        if np.any(pinned[frames]):
            _report("lpc degenerate order=%d %s" % (order, name), "lpc", float(err[frames][pinned[frames]].max()), fc.LPC_TOL)
    _report("lpc degenerate order=%d other frames (%d unpinned of %d)" % (order, int(np.sum(~pinned)), len(ref)), "lpc",
            float(err[ordinary & pinned].max()), fc.LPC_TOL)
    silent = np.array([not np.any(sig[f * (L // 2):f * (L // 2) + L]) for f in range(len(ref))])
    assert silent.sum() >= 2                                                # all-zero frames beside the impulse: NaN -> 0.0
    assert np.all(got[silent] == 0.0) and np.all(ref[silent] == 0.0)
    assert np.all(err[pinned] < fc.LPC_TOL), (float(err[pinned].max()), np.nonzero(pinned & (err >= fc.LPC_TOL))[0].tolist())


# ------------------------------------------------------------------ (d) LTSD values --------------------------------------------
def _ltsd_case(tag, N, order, sigs, noise, pcm_type):
    from oracle import ltsd_oracle as lo
    from speaker_recognition_amd.filters import ltsd as L
    NB = N // 2 + 1
    if pcm_type == "float32":
        sigs = [fc.as_float_pcm(s) for s in sigs]
        noise = fc.as_float_pcm(noise)
    na_want = lo.noise_spectrum(noise, N)
    na = L.noise_spectrum(noise, N)
    assert na.shape == (NB,)
    err_n = float(np.max(np.abs(na - na_want[:NB]) / na_want[:NB]))
    got = L.ltsd_values(sigs, na_want[:NB].astype(np.float32), N, order)
    worst, n_windows = 0.0, 0
    for s, g in zip(sigs, got):
        want = lo.ltsd(s, na_want, N, order)
        assert g.shape == want.shape == (lo.num_windows(len(s), N),)
        n_windows += len(want)
        if len(want):
            worst = max(worst, float(np.max(np.abs(g - want))))
            assert np.all(g[:order] == 0) and np.all(g[len(g) - order:] == 0)
            if len(want) <= 2 * order:
                assert np.all(g == 0)
            else:
                assert np.all(g[order:len(g) - order] != 0)
    _report("ltsd %s N=%d order=%d %s (%d windows)" % (tag, N, order, pcm_type, n_windows), "dB / noise rel", worst, fc.LTSD_TOL_DB)
    _report("ltsd %s N=%d %s noise spectrum" % (tag, N, pcm_type), "rel", err_n, fc.NOISE_TOL_REL)
    assert err_n < fc.NOISE_TOL_REL, err_n
    assert worst < fc.LTSD_TOL_DB, worst
    if pcm_type == "int16":
        # the same samples as float32 PCM: window * (float) sample either way, the same bits
        again = L.ltsd_values([s.astype(np.float32) for s in sigs], na_want[:NB].astype(np.float32), N, order)
        assert all(np.array_equal(a, g) for a, g in zip(again, got))
    return got


@pytest.mark.parametrize("pcm_type", ["int16", "float32"])
@pytest.mark.parametrize("order", fc.LTSD_ORDERS)
@pytest.mark.parametrize("fs", fc.LTSD_RATES)
def test_ltsd_values_at_every_rate_and_order(built_lib, fs, order, pcm_type):
    from oracle import ltsd_oracle as lo
    N = lo.window_size(fs)
    assert N == {8000: 371, 11025: 512, 16000: 743, 22050: 1024, 32000: 1486, 44100: 2048, 48000: 2229}[fs]
    sigs = fc.ltsd_batch(N, order)
    wn = [lo.num_windows(len(s), N) for s in sigs]
    assert 0 in wn and 2 * order in wn and 2 * order + 1 in wn
    got = _ltsd_case("fs=%d" % fs, N, order, sigs, fc.ltsd_noise(N), pcm_type)
    assert np.max(got[0]) > 20.0 and np.max(got[1]) > 20.0                   # the bursts and the alternating component are seen


@pytest.mark.parametrize("pcm_type", ["int16", "float32"])
@pytest.mark.parametrize("N", fc.LTSD_RAW_N)
def test_ltsd_raw_window_sizes(built_lib, N, pcm_type):
    _ltsd_case("raw", N, 1, fc.raw_window_batch(N), fc.raw_window_noise(N), pcm_type)


def test_ltsd_refusals(built_lib):
    from speaker_recognition_amd._lib import SRError
    from speaker_recognition_amd.filters import ltsd as L
    sig = fc.raw_window_batch(512)[0]
    for N in fc.LTSD_REFUSED_N:
        na = np.ones(N // 2 + 1, np.float32)
        with pytest.raises(SRError, match="LTSD window of %d samples is outside 4..4096" % N):
            L.ltsd_values([sig], na, N, 1)
        with pytest.raises(SRError, match="LTSD window of %d samples is outside 4..4096" % N):
            L.noise_spectrum(sig, N)
    for order in fc.LTSD_REFUSED_ORDERS:
        with pytest.raises(SRError, match="LTSD order %d is outside 0..64" % order):
            L.ltsd_values([sig], np.ones(257, np.float32), 512, order)
    with pytest.raises(SRError, match="too short for one LTSD window"):
        L.noise_spectrum(sig[:300], 512)
    assert len(L.ltsd_values([sig], np.ones(257, np.float32), 512, 64)[0]) == len(sig) // 256 - 1      # 0 and 64 are the ends


def test_ltsd_zero_noise_bins(built_lib):
    """1 / noise^2 = inf in a bin: +inf where the signal has energy there, NaN (0 * inf) where it is digital silence, as the
    division in the float64 restatement gives; the edges stay 0."""
    from oracle import ltsd_oracle as lo
    from speaker_recognition_amd.filters import ltsd as L
    N, order = 512, 5
    sigs, zero_bins = fc.zero_bin_case(N, order)
    na = lo.noise_spectrum(fc.ltsd_noise(N), N)
    for k in zero_bins:
        na[k] = na[(N - k) % N] = 0.0
    got = L.ltsd_values(sigs, na[:N // 2 + 1].astype(np.float32), N, order)
    seen = set()
    for s, g in zip(sigs, got):
        with np.errstate(all="ignore"):
            want = lo.ltsd(s, na, N, order)
        assert np.array_equal(np.isnan(g), np.isnan(want))
        assert np.array_equal(np.isposinf(g), np.isposinf(want))
        assert not np.any(np.isneginf(g)) and not np.any(np.isneginf(want))
        fin = np.isfinite(want)
        assert np.all(np.abs(g[fin] - want[fin]) < fc.LTSD_TOL_DB)
        seen |= {"nan"} if np.isnan(want).any() else set()
        seen |= {"inf"} if np.isposinf(want).any() else set()
        seen |= {"finite"} if fin.any() else set()
    assert seen == {"nan", "inf", "finite"}, seen


# ------------------------------------------------------------------ (e) the decision at 44.1 kHz -------------------------------
def test_vad_intervals_at_44100_vs_the_oracle(built_lib):
    """LTSD_VAD.filter / filter_many at 44.1 kHz (N = 2048) against voiced_runs on the oracle's LTSD values.  A window whose oracle
    value lies within the value tolerance of a threshold may go either way, and with it the run it belongs to; such windows are
    at most 1 % (asserted; none with these scenes)."""
    from oracle import ltsd_oracle as lo
    from speaker_recognition_amd.filters.ltsd import LTSD_VAD, voiced_runs
    fs = fc.VAD_FS
    scenes, noise = fc.vad_scene(fs)
    v = LTSD_VAD()
    v.init_params_by_noise(fs, noise)
    N = lo.window_size(fs)
    assert v.window_size == N == 2048
    na, lam0, lam1 = lo.thresholds(noise, N)
    _report("vad fs=%d lambda0 %.4f (oracle %.4f)" % (fs, v.lambda0, lam0), "dB", abs(v.lambda0 - lam0), 1.1 * fc.LTSD_TOL_DB)
    assert abs(v.lambda0 - lam0) < 1.1 * fc.LTSD_TOL_DB and v.lambda1 == 2.0 * v.lambda0
    half = N // 2
    n_near = n_all = n_runs = 0
    many = v.filter_many(scenes)
    for i, sc in enumerate(scenes):
        l = lo.ltsd(sc, na, N)
        runs = voiced_runs(l, v.lambda0, v.lambda1)
        n_runs += len(runs)
        affected = fc.affected_by_near(l, v.lambda0, v.lambda1)
        n_near += int(fc.near_threshold(l, v.lambda0, v.lambda1).sum())
        n_all += len(l)
        want = np.zeros(len(l), bool)
        for s, f in runs:
            want[s:f + 1] = True
        for voiced, intervals in (v.filter(sc), many[i]):
            got = np.zeros(len(l), bool)
            for s, e in intervals:
                assert s % half == 0 and e % half == 0 and s < e
                got[s // half:e // half] = True
            assert np.array_equal(got[~affected], want[~affected]), i
            assert len(voiced) == sum(e - s for s, e in intervals)
            if not affected.any():
                assert intervals == [(s * half, (f + 1) * half) for s, f in runs]
                assert np.array_equal(voiced, np.concatenate([sc[s:e] for s, e in intervals]) if intervals else np.array([]))
    _report("vad fs=%d: %d windows, %d runs, %d near a threshold" % (fs, n_all, n_runs, n_near), "share", n_near / n_all, fc.NEAR_CAP)
    assert n_runs >= 4 and len(many[-1][1]) == 0                             # bursts found; the floor alone gives nothing
    assert n_near <= fc.NEAR_CAP * n_all, (n_near, n_all)
