"""Cases, signals and second opinions for the MFCC chain (csrc/mfcc.hip, csrc/mfcc_f64.hip: four frame kernels and
cmvn_delta_kernel, picked by csrc/mfcc_plan.cpp).  Plain module (as tests/frontend_cases.py): tests/test_gpu_mfcc_cases.py runs
the kernels on these cases against oracle/mfcc_oracle.py and checks, through sr_mfcc_plan, that each case ran the branch it
names; tests/test_mfcc_cases_cpu.py shows, without a GPU and on the same inputs, that the plan takes those branches and that
the comparison can tell right from wrong.

What lives here:

  * CASES: one row per dispatch branch and parameter edge, with the plan fields the row is expected to produce (`expect`);
  * deterministic signals per case (synth.synth_speech only), int16 and their float32 twins;
  * a SECOND float64 restatement of the chain, written differently from oracle/mfcc_oracle.py on purpose: frames by stride
    tricks, np.fft.rfft, the mel bank rebuilt bin by bin and summed as per-band slices of contiguous runs (the oracle: a dense
    product with the matrix of MFCC.py:81-105), the DCT by the cosine formula per coefficient, deltas by index arithmetic on the
    normalised rows;
  * named MUTANTS of that restatement, each one plausible kernel mistake.

Known and untested (the reference itself yields non-finite or rounding-dependent values there): a mel bank with an EMPTY band
(16 kHz / FFT 256 / 64 filters has one: ln 0), and a cepstral column that is CONSTANT over an utterance (CMVN divides by a zero or
rounding-sized deviation).  No row here has either; test_mfcc_cases_cpu.py asserts the first from the plan.
"""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import numpy as np

# ------------------------------------------------------------------ tolerances (the existing tests' bounds) ------------------
# tests/test_gpu_mfcc.py: TOL[precision] = (raw rel, feature max, feature mean, delta max, delta-delta max);
# test_fft_sizes_vs_oracle: float64 spectrum 2e-6 x max(1, max |ref|) raw, 1e-5 statics, 4e-5 delta columns
TOL = {
    2: dict(raw=2e-6, static=1e-5, d1=4e-5, d2=4e-5),
    0: dict(raw=2e-4, static=1e-3, d1=1e-3, d2=2e-3),
}
GENERIC_AGREE = {2: 4e-5, 0: 2e-3}   # mfcc_generic 0 against 1: the delta bound (test_fft_sizes_vs_oracle)
MUTANT_FACTOR = 20.0                 # a mutant must differ from the oracle by at least this many tolerances on a compared value
AGREE = 1e-9                         # the two float64 restatements

# ------------------------------------------------------------------ the case table -------------------------------------------
Case = namedtuple("Case", "name fs win_ms shift_ms fft n_filters n_ceps pre_emph expect")
F32F, F32G, F64F, F64G = "fp32-fast", "fp32-generic", "f64-fast", "f64-generic"


def _c(name, fs, win, shift, fft, nf, nc, pre=0.95, **expect):
    """expect: k0 / k2 = kernel at mfcc_precision 0 / 2 (mfcc_generic 0); N1, NZ1, preset, wpb0 (fp32 waves per workgroup),
    wpb2 (float64), cp, passes (mel passes with a nonzero length), past_nc (the padded sweep reads beyond bin FFT_SIZE / 2)"""
    return Case(name, fs, win, shift, fft, nf, nc, pre, expect)


def _small(tag, fs, win, shift, fft, **common):
    """one frame shape at FFT 1024 / 512 with 2, 24 and 64 filters"""
    past = common.pop("past_nc")
    return [_c("%s_%df" % (tag, nf), fs, win, shift, fft, nf, min(13, nf - 1), k0=F32F, k2=F64G, preset=0, cp=16,
               passes=(nf + 15) // 16, past_nc=nf in past, **common) for nf in (2, 24, 64)]


CASES = [
    # fast path, default parameters (FRAME_LEN 512 at 16 kHz: the largest frame of the NZ1 = 4 instances)
    _c("default_16k", 16000, 32, 16, 2048, 50, 13, k0=F32F, k2=F64F, N1=16, NZ1=4, preset=1, wpb0=12, wpb2=8, cp=16, passes=4,
       past_nc=True),
    _c("default_8k", 8000, 32, 16, 2048, 50, 13, k0=F32F, k2=F64F, N1=16, NZ1=4, preset=0, wpb0=12, wpb2=8, cp=16, passes=4),
    # fast path, run-time sweep lengths (preset 0) by number of mel passes
    _c("p0_16f", 16000, 25, 10, 2048, 16, 13, k0=F32F, k2=F64F, N1=16, NZ1=4, preset=0, wpb0=12, cp=16, passes=1),
    _c("p0_24f", 16000, 25, 10, 2048, 24, 13, k0=F32F, k2=F64F, N1=16, NZ1=4, preset=0, wpb0=12, cp=16, passes=2),
    _c("p0_40f", 16000, 25, 10, 2048, 40, 13, k0=F32F, k2=F64F, N1=16, NZ1=4, preset=0, wpb0=12, cp=16, passes=3),
    _c("p0_64f", 16000, 25, 10, 2048, 64, 13, k0=F32F, k2=F64F, N1=16, NZ1=4, preset=0, wpb0=12, cp=16, passes=4),
    # fast path, LDS limits: the padded mel table of a narrow bank is large (every run as long as the longest of its pass)
    _c("lds_2f", 16000, 25, 10, 2048, 2, 1, k0=F32F, k2=F64G, N1=16, NZ1=4, preset=0, wpb0=4, wpb2=4, cp=16, passes=1),
    _c("lds_3f", 16000, 25, 10, 2048, 3, 2, k0=F32F, k2=F64G, N1=16, NZ1=4, preset=0, wpb0=4, wpb2=4, cp=16, passes=1),
    _c("lds_22k", 22050, 20, 10, 2048, 50, 13, k0=F32F, k2=F64G, N1=16, NZ1=4, preset=0, wpb0=12, wpb2=4, cp=16, passes=4),
    _c("lds_17f", 16000, 25, 10, 2048, 17, 13, k0=F32F, k2=F64G, N1=16, NZ1=4, preset=0, wpb0=12, wpb2=4, cp=16, passes=2),
    # number of cepstra: cmvn_delta_kernel's column padding, and the fast kernels' limit of 16
    _c("ceps16", 16000, 32, 16, 2048, 50, 16, k0=F32F, k2=F64F, preset=1, wpb0=12, cp=16, passes=4),
    _c("ceps17", 16000, 32, 16, 2048, 50, 17, k0=F32G, k2=F64G, cp=32, wpb2=4),
    _c("ceps32", 16000, 32, 16, 2048, 50, 32, k0=F32G, k2=F64G, cp=32, wpb2=4),
    _c("ceps33", 16000, 32, 16, 2048, 50, 33, k0=F32G, k2=F64G, cp=64, wpb2=4),
    _c("ceps63", 16000, 32, 16, 2048, 64, 63, k0=F32G, k2=F64G, cp=64, wpb2=4),
    # frame length at FFT 2048
    _c("len512", 16000, 32, 16, 2048, 40, 13, k0=F32F, k2=F64F, N1=16, NZ1=4, preset=0, wpb0=12, cp=16, passes=3),
    _c("len513", 16000, 32.0625, 16, 2048, 50, 13, k0=F32F, k2=F64G, N1=16, NZ1=16, preset=1, wpb0=4, wpb2=4, cp=16, passes=4),
    _c("len2048", 16000, 128, 64, 2048, 50, 13, k0=F32F, k2=F64G, N1=16, NZ1=16, preset=1, wpb0=4, wpb2=4, cp=16, passes=4),
    # FFT 1024 and 512 (fp32: the register-resident kernel with 8 / 4 points per lane in pass 1; float64: the generic kernel)
    *_small("fft1024_len400", 16000, 25, 10, 1024, N1=8, NZ1=4, wpb0=12, past_nc=(2, 24, 64)),
    *_small("fft1024_len640", 16000, 40, 20, 1024, N1=8, NZ1=8, wpb0=4, past_nc=(2, 24, 64)),
    *_small("fft512_len400", 16000, 25, 10, 512, N1=4, NZ1=4, wpb0=12, past_nc=(2, 64)),
    # small and large transforms: both generic kernels (radix 4 with one trailing radix-2 pass where FFT_SIZE / 2 is no power of 4:
    # FFT 64, 256, 1024 and 4096)
    _c("fft32", 8000, 4, 2, 32, 4, 3, k0=F32G, k2=F64G, cp=16, wpb2=4),
    _c("fft64", 8000, 8, 4, 64, 8, 5, k0=F32G, k2=F64G, cp=16, wpb2=4),
    _c("fft128", 8000, 16, 8, 128, 16, 13, k0=F32G, k2=F64G, cp=16, wpb2=4),
    _c("fft256", 8000, 25, 10, 256, 24, 13, k0=F32G, k2=F64G, cp=16, wpb2=4),
    _c("fft4096", 16000, 25, 10, 4096, 50, 13, k0=F32G, k2=F64G, cp=16, wpb2=1),
    # pre-emphasis (a kernel with 0.95 baked in passes every other row)
    _c("pre0", 16000, 32, 16, 2048, 50, 13, 0.0, k0=F32F, k2=F64F, preset=1, cp=16),
    _c("pre05", 16000, 32, 16, 2048, 50, 13, 0.5, k0=F32F, k2=F64F, preset=1, cp=16),
    _c("pre097", 16000, 32, 16, 2048, 50, 13, 0.97, k0=F32F, k2=F64F, preset=1, cp=16),
    _c("pre1", 16000, 32, 16, 2048, 50, 13, 1.0, k0=F32F, k2=F64F, preset=1, cp=16),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)

# Values of a plan field that no parameters select, with the reason (test_mfcc_cases_cpu.py::test_branch_census):
UNREACHABLE = {
    ("preset", 2): "removed: no (fs, n_filters) has the sweep lengths 32/64/96/96 it was built for (8 kHz / 50 filters: 32/48/96/96)",
    ("wpb2", 2): "f64 generic with two waves: lds_for(4) = 9 * 8 * FFT_SIZE + 2048 fits 160 KB up to FFT 2048, lds_for(2) = "
                 "5 * 8 * FFT_SIZE + 1024 = 164864 does not at FFT 4096, the only larger size: 4 or 1, never 2",
    ("N1/NZ1", (4, 8)): "FFT 512 holds frames of at most 512 samples: 4 rows",
    ("N1/NZ1", (4, 16)): "FFT 512 holds frames of at most 512 samples: 4 rows",
    ("N1/NZ1", (8, 16)): "FFT 1024 holds frames of at most 1024 samples: 8 rows",
    ("N1/NZ1", (16, 8)): "FFT 2048: frames of more than 512 samples all take the NZ1 = 16 instance",
    ("f64-fast NZ1", 16): "the float64 fast kernel holds frames of at most 512 samples (4 rows): longer ones take the generic kernel",
    ("f64-fast N1", 8): "the float64 fast kernel is FFT 2048 only; FFT 1024 and 512 take the generic kernel",
}


def kw(case):
    """keywords of core.MfccExtractor / oracle.mfcc_oracle.get_mfcc_extractor"""
    return dict(win_length_ms=case.win_ms, win_shift_ms=case.shift_ms, FFT_SIZE=case.fft, n_filters=case.n_filters,
                n_ceps=case.n_ceps, pre_emphasis_coef=case.pre_emph)


def frame_len(case):
    return int(float(case.win_ms) / 1000 * case.fs)


def frame_shift(case):
    return int(float(case.shift_ms) / 1000 * case.fs)


# ------------------------------------------------------------------ signals ---------------------------------------------------
def as_float_pcm(sig):
    """the float32-PCM twin of an int16 signal: non-integer samples, so that the float instance cannot pass on integers alone"""
    return (np.asarray(sig, np.float32) * np.float32(0.37)).astype(np.float32)


@lru_cache(maxsize=None)
def signals(name):
    """five int16 utterances of a case: about 0.4, 0.7 and 1.2 s of synth_speech (never fewer than 9 / 14 / 23 frames; a run of
    exact zeros longer than two frames inside the second: whole frames on the floor path), then one of exactly 5 FRAME_LEN
    samples (no frames, MFCC.py:56) and one of 5 FRAME_LEN + 1 (the shortest that has any)"""
    from speaker_recognition_amd import synth
    c = CASE[name]
    L, S = frame_len(c), frame_shift(c)
    seed0 = 100 + 7 * CASES.index(c)
    out = []
    for i, (secs, min_frames) in enumerate(((0.4, 9), (0.7, 14), (1.2, 23))):
        n = max(int(secs * c.fs), 5 * L + 1, L + (min_frames - 1) * S + 3 + i)
        s = synth.synth_speech(3 + i + CASES.index(c), n / float(c.fs) + 0.01, c.fs, seed=seed0 + i)[:n].copy()
        if i == 1:
            z0 = n // 3
            s[z0:z0 + 2 * L + 2 * S + 5] = 0
        out.append(s)
    for i, n in enumerate((5 * L, 5 * L + 1)):
        out.append(synth.synth_speech(9 + i, n / float(c.fs) + 0.01, c.fs, seed=seed0 + 5 + i)[:n].copy())
    return tuple(out)


def pcm(name, kind):
    s = signals(name)
    return s if kind == "int16" else tuple(as_float_pcm(x) for x in s)


# ------------------------------------------------------------------ the oracle's answers, computed once ---------------------
@lru_cache(maxsize=None)
def reference(name, kind):
    """per utterance: None (no frames) or dict(raw=float64 [T, C], nd0=, nd1=, nd2= normalised features with deltas)"""
    from oracle import mfcc_oracle as mo
    c = CASE[name]
    ex = mo.get_mfcc_extractor(c.fs, **kw(c))
    out = []
    for s in pcm(name, kind):
        if len(s) <= 5 * ex.FRAME_LEN:
            out.append(None)
            continue
        raw = ex.raw_cepstra(np.asarray(s, np.float64))
        z = (raw - raw.mean(axis=0)) / raw.std(axis=0) if raw.shape[0] > 1 else raw
        out.append(dict(raw=raw, nd0=z, nd1=mo.diff_feature(z, 1), nd2=mo.diff_feature(z, 2)))
    return tuple(out)


def errors(c, got_raw, got, ref):
    """{quantity: (error, bound)}: got_raw [T, C] or None, got = {nd: [T - nd, C (nd + 1)]}, ref = one entry of reference();
    the bounds are those of mfcc_precision 2 -- scale by TOL[0][q] / TOL[2][q] for precision 0"""
    C = c.n_ceps
    out = {}
    if got_raw is not None:
        out["raw"] = (float(np.max(np.abs(got_raw - ref["raw"]))), max(1.0, float(np.abs(ref["raw"]).max())))
    for nd, g in got.items():
        r = ref["nd%d" % nd]
        assert g.shape == r.shape, (c.name, nd, g.shape, r.shape)
        d = np.abs(g - r)
        out["static_nd%d" % nd] = (float(d[:, :C].max()), 1.0)
        if nd >= 1:
            out["d1_nd%d" % nd] = (float(d[:, C:2 * C].max()), 1.0)
        if nd >= 2:
            out["d2_nd%d" % nd] = (float(d[:, 2 * C:].max()), 1.0)
    return out


def tolerance(precision, quantity):
    return TOL[precision][quantity.split("_")[0]]


# ------------------------------------------------------------------ the second restatement and its mutants -------------------
MUTANTS = ("window_unshifted", "preemph_first", "preemph_stream", "preemph_default", "last_bin_dropped", "c0_kept", "sample_std",
           "delta_rows_off_by_one", "stats_over_emitted_rows")


@lru_cache(maxsize=None)
def mel_runs(fs, fft, n_bands):
    """the melfb.m-style bank, bin by bin: bin k sits at pf(k) = ln(1 + k / (f0 FFT)) / lr on the band axis (band centres at
    1..B) and gives 2 (1 - frac) to the band below it and 2 frac to the band above; bins from 1 to FFT/2 - 1 below B + 1.
    -> [(first bin, weights)] per band: one contiguous run each"""
    f0 = 700.0 / fs
    lr = np.log(1 + 0.5 / f0) / (n_bands + 1)
    per_band = [dict() for _ in range(n_bands)]
    # the band edges in bins, as MFCC.py:85-89 rounds them (the comparisons on pf itself round differently at an exact integer)
    edge = lambda i: fft * f0 * (np.exp(i * lr) - 1)
    b2, b3, b4 = int(np.ceil(edge(1))), int(np.floor(edge(n_bands))), min(fft // 2, int(np.ceil(edge(n_bands + 1)))) - 1
    for k in range(1, b4 + 1):
        pf = np.log(1 + k / f0 / fft) / lr
        lo = int(np.floor(pf))
        frac = pf - lo
        if k >= b2:
            per_band[lo - 1][k] = per_band[lo - 1].get(k, 0.0) + 2 * (1 - frac)
        if k <= b3:
            per_band[lo][k] = per_band[lo].get(k, 0.0) + 2 * frac
    runs = []
    for d in per_band:
        ks = sorted(k for k, v in d.items() if v != 0.0)
        assert ks and ks == list(range(ks[0], ks[-1] + 1)), "an empty or split band"
        runs.append((ks[0], np.array([d[k] for k in ks])))
    return runs


def second_raw(c, signal, mutant=None):
    """raw cepstra, float64 [T, n_ceps]"""
    x = np.asarray(signal, np.float64)
    L, S, N, B = frame_len(c), frame_shift(c), c.fft, c.n_filters
    assert len(x) > 5 * L
    T = (len(x) - L) // S + 1
    fr = np.lib.stride_tricks.sliding_window_view(x, L)[::S][:T]
    assert fr.shape == (T, L)
    i = np.arange(L)
    w = 0.54 - 0.46 * np.cos(2 * np.pi * (i + (0.0 if mutant == "window_unshifted" else 0.5)) / L)
    pre = 0.95 if mutant == "preemph_default" else c.pre_emph
    if mutant == "preemph_first":                         # y = w (x[i] - a x[i-1]) instead of w[i] x[i] - a w[i-1] x[i-1]
        y = fr.copy()
        y[:, 1:] -= pre * fr[:, :-1]
        y = y * w
    else:
        wf = fr * w
        y = wf.copy()
        y[:, 1:] -= pre * wf[:, :-1]
        if mutant == "preemph_stream":                    # the frame's first sample also takes the sample before the frame
            prev = np.concatenate(([0.0], x[np.arange(1, T) * S - 1]))
            y[:, 0] -= pre * prev * w[0]
    Z = np.fft.rfft(y, N, axis=1)
    P = Z.real ** 2 + Z.imag ** 2
    P = np.where(P < 1e-100, 1e-100, P)
    E = np.empty((T, B))
    for b, (k0, wt) in enumerate(mel_runs(c.fs, N, B)):
        if mutant == "last_bin_dropped":
            wt = wt[:-1]
        E[:, b] = P[:, k0:k0 + len(wt)] @ wt
    lE = np.log(E)
    xs = np.arange(B)
    rows = range(c.n_ceps) if mutant == "c0_kept" else range(1, c.n_ceps + 1)
    out = np.empty((T, c.n_ceps))
    for j, yv in enumerate(rows):
        out[:, j] = np.sqrt(2.0 / B) * (lE @ np.cos(np.pi * (2 * xs + 1) * yv / (2.0 * B))) / (np.sqrt(2) if yv == 0 else 1.0)
    return out


def second_features(raw, nd, mutant=None, cmvn=True):
    """CMVN over all T rows (population deviation, no epsilon), then output row t = normalised row t + nd, its first difference
    and the difference of the last two first differences: [T - nd, C (nd + 1)]"""
    T, C = raw.shape
    z = np.asarray(raw, np.float64)
    if cmvn and T > 1:
        st = raw[nd:] if mutant == "stats_over_emitted_rows" else raw
        mu = st.sum(axis=0) / st.shape[0]
        var = ((st - mu) ** 2).sum(axis=0) / (st.shape[0] - (1 if mutant == "sample_std" else 0))
        z = (raw - mu) / np.sqrt(var)
    t = np.arange(nd, T)
    cols = [z[t]]
    if nd >= 1:
        cols.append(z[t] - z[t - 1])
    if nd >= 2:
        back = 1 if mutant == "delta_rows_off_by_one" else 2          # (z[t-1] read where z[t-2] belongs)
        cols.append((z[t] - z[t - 1]) - (z[t - 1] - z[t - back]))
    return np.concatenate(cols, axis=1)


def second(c, signal, mutant=None):
    """what errors() takes: (raw, {nd: features}) of the second restatement or one of its mutants"""
    raw = second_raw(c, signal, mutant)
    return raw, {nd: second_features(raw, nd, mutant) for nd in (0, 1, 2)}


# ------------------------------------------------------------------ large batches ---------------------------------------------
LARGE_FS = 8000
LARGE_KW = dict(win_length_ms=10, win_shift_ms=10, FFT_SIZE=2048)      # frames of 80 samples, no overlap


def sample_frames(off, n_want=200):
    """utterances whose frames a large-batch test compares with the oracle: the first and the last with frames, and those around
    evenly spaced frame indices (boundary-crossing waves); -> sorted utterance indices, at least `n_want` frames together when the
    batch has them"""
    off = np.asarray(off)
    has = np.nonzero(np.diff(off) > 0)[0]
    pick = {int(has[0]), int(has[-1])}
    total = int(off[-1])
    frames = lambda p: sum(int(off[u + 1] - off[u]) for u in p)
    k = 3
    while frames(pick) < n_want and k < 64:
        for f in np.linspace(0, total - 1, k).astype(np.int64):
            pick.add(int(np.searchsorted(off, f, side="right") - 1))
        k += 2
    return sorted(pick)
