"""Inputs and second opinions for the two front-end kernels that sit in front of every default path: LPC (csrc/lpc.hip) and
LTSD (csrc/ltsd.hip).  Plain module (as tests/fullcov_oracle.py): tests/test_gpu_frontend.py runs the kernels on these inputs
against oracle/lpc_oracle.py and oracle/ltsd_oracle.py; tests/test_frontend_cases_cpu.py shows, without a GPU and on the same
inputs, that the comparison can tell right from wrong.

Three kinds of thing live here:

  * deterministic signal builders (numpy, scipy.signal.lfilter and synth.synth_speech only);
  * a SECOND float64 restatement of each oracle, written differently on purpose, so that the oracle itself has a check:
      LPC   autocorrelation by direct lag sums in np.longdouble (the oracle goes through the FFT), coefficients by
            scipy.linalg.solve_toeplitz (the oracle runs the Levinson-Durbin recursion in Python);
      LTSD  the half spectrum of a real FFT with explicit mirror weights -- 1 for k = 0 and for k = N/2 when N is even, else 2
            (the oracle sums all N bins of a complex FFT);
  * named MUTANTS of those restatements, each one subtle kernel mistake (LPC_MUTANTS, LTSD_MUTANTS).
"""
from __future__ import annotations

import numpy as np

# ------------------------------------------------------------------ tolerances (the existing tests' bounds) ------------------
LPC_TOL = 2e-6            # max |got - ref| / max(1, |ref|)       (tests/test_gpu_mfcc.py::test_lpc_and_mix_feature_vs_oracle)
LTSD_TOL_DB = 2e-3        # max |got - ref|, dB                   (tests/test_gpu_vad.py::test_ltsd_values_vs_oracle)
NOISE_TOL_REL = 1e-4      # noise spectrum, relative per bin      (same test)
MUTANT_FACTOR = 20.0      # a mutant must differ from the oracle by at least this many tolerances on a compared value

# ------------------------------------------------------------------ LPC: the instances ----------------------------------------
LPC_ORDERS = (10, 12, 15, 16, 20)                       # every SR_LPC_CASE(O) of csrc/lpc.hip
LPC_UNBUILT_ORDERS = (14, 21)
# (fs, win_length_ms, frame_len, SPL): every SR_LPC_SPL(S) -- samples per lane 8 (frames up to 512), 16 (..1024), 32 (..2048)
LPC_FRAMES = (
    (8000, 32, 256, 8), (16000, 25, 400, 8), (16000, 32, 512, 8),
    (16000, 40, 640, 16), (16000, 64, 1024, 16),
    (44100, 25, 1102, 32), (44100, 40, 1764, 32), (16000, 128, 2048, 32),
)
LPC_TOO_LONG = (44100, 50, 2205)                        # 2049+ samples: refused (with FFT_SIZE 4096 the MFCC half accepts it)


def lpc_kw(win_ms):
    """window and shift keywords of a frame configuration: half-overlapped frames"""
    return dict(win_length_ms=win_ms, win_shift_ms=win_ms / 2.0)


def ar_signal(n, fs, poles, seed, amplitude=9000.0):
    """AR(p) resonance: white noise through 1 / prod (1 - 2 r cos(w) z^-1 + r^2 z^-2) over (freq_hz, radius) pole pairs.
    Radii close to 1 give the ill-conditioned Toeplitz systems (cond 1e4..1e7) the float64 chain of the kernel exists for."""
    from scipy.signal import lfilter
    rng = np.random.default_rng(seed)
    y = rng.standard_normal(n + 2000)
    for f, r in poles:
        y = lfilter([1.0], [1.0, -2.0 * r * np.cos(2 * np.pi * f / fs), r * r], y)
    y = y[2000:]
    return y / np.max(np.abs(y)) * amplitude


def lpc_signal(fs, frame_len, seed=0, n_frames=26):
    """int16: speech, then an AR(2) resonance (radius 0.995), then an AR(6) one, about `n_frames` half-overlapped frames"""
    from speaker_recognition_amd import synth
    n = (n_frames + 1) * (frame_len // 2) + 7
    a = n // 3
    sp = synth.synth_speech(7 + seed, a / float(fs) + 0.01, fs, seed=300 + seed)[:a].astype(np.float64)
    ar2 = ar_signal(a, fs, [(0.11 * fs, 0.995)], 11 + seed)
    ar6 = ar_signal(n - 2 * a, fs, [(0.05 * fs, 0.99), (0.17 * fs, 0.985), (0.31 * fs, 0.98)], 23 + seed)
    return np.round(np.concatenate([sp, ar2, ar6])).astype(np.int16)


def as_float_pcm(sig):
    """the float32-PCM twin of an int16 signal: non-integer samples, so that the float instance cannot pass on integers alone"""
    return (np.asarray(sig, np.float32) * np.float32(0.37)).astype(np.float32)


# ragged batches (2b): 10 ms window, 40 ms shift at 8 kHz -> frames of 80 samples every 320; an utterance needs > 400 samples
RAGGED_FS, RAGGED_KW = 8000, dict(win_length_ms=10, win_shift_ms=40)


def ragged_batch(seed=3):
    """>= 40 int16 utterances of mixed length; runs of consecutive zero-frame ones (<= 5 frame lengths) at the start, in the
    middle and at the end; most of the others have 2..5 frames, so that a wave's 8 frames cross several boundaries."""
    rng = np.random.default_rng(seed)
    L = 80
    lens = [400, 17, 0, 399]                                              # start: four utterances without frames
    lens += [401, 720, 721, 1041, 400, 401, 1361, 405]
    lens += [int(x) for x in rng.integers(401, 1700, 10)]
    lens += [0, 1, 400, 80, 5 * L]                                        # middle: five in a row
    lens += [int(x) for x in rng.integers(401, 2400, 12)]
    lens += [6000, 401, 399, 402, 9000]
    lens += [int(x) for x in rng.integers(401, 1200, 6)]
    lens += [400, 0, 79]                                                  # end: three
    total = sum(lens)
    src = np.round(ar_signal(total, RAGGED_FS, [(700.0, 0.99), (1900.0, 0.97)], 40 + seed)).astype(np.int16)
    out, t = [], 0
    for n in lens:
        out.append(src[t:t + n].copy())
        t += n
    return out


def large_batch(n_frames_wanted, seed=5):
    """(signals, kw): utterances of mixed length at 8 kHz, 10 ms window and shift, with at least `n_frames_wanted` frames"""
    kw = dict(win_length_ms=10, win_shift_ms=10)
    rng = np.random.default_rng(seed)
    lens, frames = [], 0
    while frames < n_frames_wanted:
        n = int(rng.integers(300, 160000)) if len(lens) % 7 else int(rng.integers(0, 401))
        lens.append(n)
        frames += (n - 80) // 80 + 1 if n > 400 else 0
    src = np.round(ar_signal(sum(lens), RAGGED_FS, [(600.0, 0.992), (2100.0, 0.96)], 50 + seed, 6000.0)).astype(np.int16)
    out, t = [], 0
    for n in lens:
        out.append(src[t:t + n])
        t += n
    return out, kw


# ---- degenerate frames (2c) ----
DEGENERATE_FS, DEGENERATE_KW, DEGENERATE_L = 16000, dict(win_length_ms=32, win_shift_ms=16), 512
DEGENERATE_CLASSES = ("dc_max", "dc_min", "dc_one", "square_nyquist", "square_quarter", "dither", "impulse", "sinusoid")
DEGENERATE_ORDERS = (10, 15, 20)
UNPINNED_CAP = 0.05


def degenerate_block(name, n, seed=0):
    i = np.arange(n)
    if name == "dc_max":
        return np.full(n, 32767.0)
    if name == "dc_min":
        return np.full(n, -32767.0)
    if name == "dc_one":
        return np.full(n, 1.0)
    if name == "square_nyquist":
        return np.where(i % 2 == 0, 32767.0, -32767.0)
    if name == "square_quarter":
        return np.where((i // 2) % 2 == 0, 32767.0, -32767.0)
    if name == "dither":
        return np.random.default_rng(70 + seed).integers(0, 2, n) * 2.0 - 1.0
    if name == "impulse":
        x = np.zeros(n)
        x[n // 2 + 37] = 32767.0
        return x
    if name == "sinusoid":
        return np.round(20000.0 * np.sin(2 * np.pi * 1000.0 / DEGENERATE_FS * i))
    raise KeyError(name)


def degenerate_signal():
    """-> (int16 signal, {class: [frame indices wholly inside the degenerate block]}): ordinary speech with one block of
    3 frame lengths per class (5 half-overlapped frames wholly inside), 12 frame lengths of speech between the blocks."""
    from speaker_recognition_amd import synth
    L, S = DEGENERATE_L, DEGENERATE_L // 2
    gap, blk = 12 * L, 3 * L
    n = gap + len(DEGENERATE_CLASSES) * (blk + gap)
    sig = synth.synth_speech(5, n / float(DEGENERATE_FS) + 0.01, DEGENERATE_FS, seed=77)[:n].astype(np.float64)
    inside = {}
    for c, name in enumerate(DEGENERATE_CLASSES):
        s0 = gap + c * (blk + gap)
        sig[s0:s0 + blk] = degenerate_block(name, blk)
        f0 = -(-s0 // S)
        inside[name] = [f for f in range(f0, (s0 + blk - L) // S + 1)]
    return sig.astype(np.int16), inside


# ------------------------------------------------------------------ LPC: second restatement and mutants ------------------------
LPC_MUTANTS = ("unbiased", "preemph_first", "halo", "short_recursion", "shift_plus_one")


def _solve_lpc(r, order):
    from scipy.linalg import solve_toeplitz
    r = np.asarray(r, np.float64)
    if not np.all(np.isfinite(r)) or r[0] == 0.0:
        return np.full(order, np.nan)
    try:
        with np.errstate(all="ignore"):
            return solve_toeplitz(r[:order], -r[1:order + 1])
    except np.linalg.LinAlgError:
        return np.full(order, np.nan)


def lpc_second(fs, signal, win_length_ms=32, win_shift_ms=16, n_lpc=15, pre_emphasis_coef=0.95, mutant=None, utt_index=0,
               keep_nan=False):
    """Second float64 restatement of oracle/lpc_oracle.extract (or, with ``mutant``, one subtle mistake):
      unbiased         autocorrelation divided by L - k instead of L
      preemph_first    pre-emphasis on the samples, then the window (the chain is: window, then pre-emphasis)
      halo             the lag halo behind the frame is not zero: the last `order` values of the previous frame sit there
      short_recursion  the recursion stops at order - 1; the last coefficient stays 0
      shift_plus_one   frames of utterance 2 onwards (``utt_index`` >= 1) start every shift + 1 samples
    ``keep_nan``: leave NaN rows as they are (to tell "NaN -> 0" from a value)."""
    assert mutant is None or mutant in LPC_MUTANTS, mutant
    x = np.asarray(signal, np.float64)
    L = int(float(win_length_ms) / 1000 * fs)
    S = int(float(win_shift_ms) / 1000 * fs)
    T = (len(x) - L) // S + 1
    w = (0.54 - 0.46 * np.cos(2 * np.pi * (np.arange(L) + 0.5) / L)).astype(np.longdouble)
    step = S + 1 if (mutant == "shift_plus_one" and utt_index >= 1) else S
    out = np.zeros((max(T, 0), n_lpc))
    prev = np.zeros(L, np.longdouble)
    for f in range(T):
        fr = np.zeros(L, np.longdouble)
        seg = x[f * step:f * step + L]
        fr[:len(seg)] = seg
        if mutant == "preemph_first":
            y = fr.copy()
            y[1:] -= np.longdouble(pre_emphasis_coef) * fr[:-1]
            y *= w
        else:
            y = fr * w
            y[1:] = y[1:] - np.longdouble(pre_emphasis_coef) * y[:-1]
        ext = np.concatenate([y, prev[L - n_lpc:] if mutant == "halo" else np.zeros(n_lpc, np.longdouble)])
        r = np.array([np.sum(y * ext[k:k + L]) for k in range(n_lpc + 1)], np.longdouble)
        r = r / (L - np.arange(n_lpc + 1)) if mutant == "unbiased" else r / L
        if mutant == "short_recursion":
            out[f, :n_lpc - 1] = _solve_lpc(r, n_lpc - 1)
        else:
            out[f] = _solve_lpc(r, n_lpc)
        prev = y
    if not keep_nan:
        out[np.isnan(out)] = 0.0
    return out


def lpc_metric(got, ref):
    """the LPC tests' measure: |got - ref| / max(1, |ref|), per element"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) / np.maximum(1.0, np.abs(ref))


def lpc_frame_oracle(ex, signal, frames):
    """oracle/lpc_oracle's rows for the given frame indices only (``ex``: an lpc_oracle.LPCExtractor)"""
    from oracle import lpc_oracle as lo
    x = np.asarray(signal, np.float64)
    out = np.zeros((len(frames), ex.n_lpc))
    for i, f in enumerate(frames):
        fr = x[f * ex.FRAME_SHIFT:f * ex.FRAME_SHIFT + ex.FRAME_LEN] * ex.window
        fr[1:] -= fr[:-1] * ex.PRE_EMPH
        out[i] = lo.levinson_1d(lo.acorr_lpc(fr), ex.n_lpc)[0][1:]
    out[np.isnan(out)] = 0.0
    return out


# ------------------------------------------------------------------ LTSD: the cases ---------------------------------------------
LTSD_RATES = (8000, 11025, 16000, 22050, 32000, 44100, 48000)            # N = 371, 512, 743, 1024, 1486, 2048, 2229
LTSD_ORDERS = (0, 1, 5, 12)
LTSD_RAW_N = (4, 5, 4095, 4096)
LTSD_REFUSED_N = (3, 4097)
LTSD_REFUSED_ORDERS = (-1, 65)
NOISE_SIGMA = 120.0


def ltsd_noise(N, seed=0, windows=40):
    rng = np.random.default_rng(900 + seed)
    return np.clip(np.round(rng.normal(0.0, NOISE_SIGMA, (windows + 1) * (N // 2) + 3)), -32768, 32767).astype(np.int16)


def burst_scene(N, order, seed=0):
    """noise floor with speech-like (resonant) bursts of irregular length; long enough for interior windows at any order"""
    half = N // 2
    wn = max(60, 2 * order + 30)
    n = (wn + 1) * half + half // 3
    rng = np.random.default_rng(910 + seed)
    sig = rng.normal(0.0, NOISE_SIGMA, n)
    tone = ar_signal(n, 16000, [(700.0, 0.98), (2300.0, 0.95)], 920 + seed, 7000.0)
    t, on = int(3.5 * half), True
    while t < n:
        d = int(rng.uniform(2.0, 9.0) * half)
        if on:
            sig[t:t + d] += tone[t:t + d]
        t, on = t + d, not on
    return np.clip(np.round(sig), -32768, 32767).astype(np.int16)


def alternating_scene(N, order, seed=0):
    """noise floor; an alternating +A / -A component (the Nyquist bin of an even N) switched on for the middle third; a DC
    offset (bin 0) switched on for the last sixth"""
    half = N // 2
    wn = max(60, 2 * order + 30)
    n = (wn + 1) * half + 5
    rng = np.random.default_rng(930 + seed)
    sig = rng.normal(0.0, NOISE_SIGMA, n)
    i = np.arange(n)
    mid = (i >= n // 3) & (i < 2 * n // 3)
    sig[mid] += np.where(i[mid] % 2 == 0, 3000.0, -3000.0)
    sig[5 * n // 6:] += 2500.0
    return np.clip(np.round(sig), -32768, 32767).astype(np.int16)


def ltsd_batch(N, order, seed=0):
    """the signals of one LTSD case: bursts, the alternating / DC scene, too short for one window, exactly 2 order and
    2 order + 1 windows (all zeros / one value), a reversed copy, a mid-scene cut"""
    half = N // 2
    a, b = burst_scene(N, order, seed), alternating_scene(N, order, seed)

    def with_windows(wn):               # the shortest signal with `wn` windows: len // half - 1 == wn
        return b[len(b) // 3:len(b) // 3 + (wn + 1) * half].copy()
    sigs = [a, b, a[:max(0, 2 * half - 1)].copy(), with_windows(2 * order), with_windows(2 * order + 1), a[::-1].copy(),
            b[len(b) // 4:len(b) // 4 + (2 * order + 9) * half + half // 2].copy(), np.zeros(3, np.int16)]
    return sigs


def raw_window_batch(N, order=1):
    """short signals for the raw window sizes (a handful of windows: the direct DFT at N = 4096 is 17 Mflop per window)"""
    half = N // 2
    wn = 2 * order + 6
    rng = np.random.default_rng(940 + N)
    n = (wn + 1) * half + 1
    sig = rng.normal(0.0, NOISE_SIGMA, n)
    i = np.arange(n)
    sig[n // 3:2 * n // 3] += np.where(i[n // 3:2 * n // 3] % 2 == 0, 3000.0, -3000.0) + 800.0 * np.sin(0.9 * i[n // 3:2 * n // 3])
    sig = np.clip(np.round(sig), -32768, 32767).astype(np.int16)
    return [sig, sig[::-1].copy(), sig[:half], sig[:(2 * order + 1) * half + 1].copy()]


def raw_window_noise(N):
    rng = np.random.default_rng(950 + N)
    return np.clip(np.round(rng.normal(0.0, NOISE_SIGMA, 9 * (N // 2) + 1)), -32768, 32767).astype(np.int16)


def zero_bin_case(N=512, order=5):
    """-> (signals, zero bins): a scene whose first third is digital silence (all-zero windows: 0 * inf) for a noise spectrum
    with zero bins"""
    s = burst_scene(N, order, seed=4)
    s[:len(s) // 3] = 0
    return [s, alternating_scene(N, order, seed=4)], (7, N // 2)


# ---- VAD at 44.1 kHz (2e) ----
VAD_FS = 44100
NEAR_CAP = 0.01


def vad_scene(fs=VAD_FS, seed=0):
    """(scenes, noise): bursts 40 dB above a stationary floor with abrupt edges -- LTSD jumps from ~lambda0 / 1.1 to tens of dB
    within a window or two, so few windows can sit near a threshold"""
    from speaker_recognition_amd import synth
    rng = np.random.default_rng(960 + seed)
    noise = np.round(rng.normal(0.0, 60.0, 2 * fs)).astype(np.int16)
    scenes = []
    for k, (secs, bursts) in enumerate(((3.0, [(0.5, 1.1), (1.7, 2.0), (2.3, 2.7)]), (2.0, [(0.3, 1.5)]), (1.0, []))):
        sig = rng.normal(0.0, 60.0, int(secs * fs))
        for j, (s, e) in enumerate(bursts):
            sp = synth.synth_speech(4 + j + 3 * k, e - s, fs, seed=60 + j + 10 * k).astype(np.float64)
            sig[int(s * fs):int(s * fs) + len(sp)] += sp
        scenes.append(np.clip(np.round(sig), -32768, 32767).astype(np.int16))
    return scenes, noise


def near_threshold(l, lam0, lam1, tol=LTSD_TOL_DB):
    l = np.asarray(l, np.float64)
    return (np.abs(l - lam0) <= tol) | (np.abs(l - lam1) <= tol)


def affected_by_near(l, lam0, lam1, tol=LTSD_TOL_DB):
    """windows whose decision a value within `tol` of a threshold can change: the near windows themselves and every maximal run
    of windows above lambda0 - tol that touches one"""
    l = np.asarray(l, np.float64)
    near = near_threshold(l, lam0, lam1, tol)
    out = near.copy()
    above = l > lam0 - tol
    i, n = 0, len(l)
    while i < n:
        if not above[i]:
            i += 1
            continue
        j = i
        while j + 1 < n and above[j + 1]:
            j += 1
        if near[max(0, i - 1):j + 2].any():
            out[i:j + 1] = True
        i = j + 1
    return out


# ------------------------------------------------------------------ LTSD: second restatement and mutants -----------------------
LTSD_MUTANTS = ("nyquist_weight_2", "dc_weight_2", "envelope_open", "edge_rule", "window_periodic", "hop_rounded_up")


def ltsd_half_amplitudes(signal, N, mutant=None):
    """[windows][N/2 + 1] amplitudes of the real FFT of the Hann-windowed, zero-extended frames"""
    x = np.asarray(signal, np.float64)
    half = N // 2
    wn = max(0, len(x) // half - 1)
    hop = (N + 1) // 2 if mutant == "hop_rounded_up" else half
    i = np.arange(N)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * i / (N if mutant == "window_periodic" else N - 1))
    pad = np.concatenate([x, np.zeros(N + wn * (hop - half) + 1)])
    fr = np.stack([pad[l * hop:l * hop + N] for l in range(wn)]) if wn else np.zeros((0, N))
    return np.abs(np.fft.rfft(fr * win[None, :], axis=1))


def ltsd_second(signal, noise_amp_half, N, order=5, mutant=None):
    """Second float64 restatement of oracle/ltsd_oracle.ltsd on bins 0..N/2 (or, with ``mutant``, one subtle mistake):
      nyquist_weight_2  bin N/2 of an even N counted twice       dc_weight_2      bin 0 counted twice
      envelope_open     maximum over [-order, order)             edge_rule        zero only where l + order > windows
      window_periodic   numpy.hanning(N + 1)[:N]                 hop_rounded_up   hop (N + 1) / 2 for odd N"""
    assert mutant is None or mutant in LTSD_MUTANTS, mutant
    amp = ltsd_half_amplitudes(signal, N, mutant)
    wn, NB = amp.shape[0], N // 2 + 1
    wgt = np.full(NB, 2.0)
    wgt[0] = 2.0 if mutant == "dc_weight_2" else 1.0
    if N % 2 == 0:
        wgt[N // 2] = 2.0 if mutant == "nyquist_weight_2" else 1.0
    na = np.asarray(noise_amp_half, np.float64)[:NB]
    out = np.zeros(wn)
    with np.errstate(all="ignore"):
        for l in range(wn):
            if l < order or (l + order > wn if mutant == "edge_rule" else l + order >= wn):
                continue
            hi = l + order if mutant == "envelope_open" else l + order + 1
            if hi <= l - order:
                continue
            e = amp[l - order:min(hi, wn)].max(axis=0)
            out[l] = 10.0 * np.log10(np.dot(wgt, (e / na) ** 2) / N)
    return out


def noise_second(noise, N):
    return ltsd_half_amplitudes(noise, N).mean(axis=0)


def emulate_ltsd_f32(signal, noise_amp_half, N, order=5):
    """The kernels' arithmetic on the CPU, for a tolerance that does not come from the device: float32 window, float32
    twiddle ring, float32 products accumulated sequentially in float32 (float64 product rounded once = FMA), float32
    sqrt; maxima, then the float64 weighted sum with float32 1 / noise^2."""
    x = np.asarray(signal, np.float64)
    half, NB = N // 2, N // 2 + 1
    wn = max(0, len(x) // half - 1)
    i = np.arange(N)
    win = (0.5 - 0.5 * np.cos(2.0 * np.pi * i / (N - 1.0))).astype(np.float32)
    ang = 2.0 * np.pi * i / float(N)
    rc, rs = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
    pad = np.concatenate([x, np.zeros(N + 1)])
    amp = np.zeros((wn, NB), np.float32)
    k = np.arange(NB)
    for l in range(wn):
        xv = (win * pad[l * half:l * half + N].astype(np.float32)).astype(np.float32)
        re, im = np.zeros(NB, np.float32), np.zeros(NB, np.float32)
        idx = np.zeros(NB, np.int64)
        for n in range(N):
            re = (re.astype(np.float64) + float(xv[n]) * rc[idx].astype(np.float64)).astype(np.float32)
            im = (im.astype(np.float64) + float(xv[n]) * rs[idx].astype(np.float64)).astype(np.float32)
            idx = (idx + k) % N
        amp[l] = np.sqrt((re * re + im * im).astype(np.float32))
    inv = (1.0 / np.asarray(noise_amp_half, np.float64)[:NB] ** 2).astype(np.float32).astype(np.float64)
    wgt = np.full(NB, 2.0)
    wgt[0] = 1.0
    if N % 2 == 0:
        wgt[N // 2] = 1.0
    out = np.zeros(wn, np.float32)
    for l in range(wn):
        if l < order or l + order >= wn:
            continue
        m = amp[l - order:l + order + 1].max(axis=0).astype(np.float64)
        out[l] = np.float32(10.0 * np.log10(np.dot(wgt, m * m * inv) / N))
    return out
