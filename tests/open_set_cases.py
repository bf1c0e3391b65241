"""Shared by tests/test_open_set_cpu.py and tests/test_gpu_open_set.py: the reference's open-set rule restated in float64 numpy
(reference src/testbench/gmmset.py:69-81) and the synthetic UBM + MAP-speaker cases of the features path, the voice-activity scene of the stream tests and the models that
put frames into the partial-product band.  Nothing here touches the GPU."""
import operator

import numpy as np

GATE = 1e-4      # the project's parity gate on a log-likelihood: |a - ref| <= GATE * max(1, |ref|)


def rule_one(row, n, bg, threshold):
    """One utterance: (label, margin).  `row`: its sums over the S columns, float64; `n`: its frame count.
    gmmset.py:72-81 line by line -- the scores are the columns other than the UBM's, in order -- with the two cases the reference
    cannot reach (no frames: it divides by zero; no speaker: max() of nothing) giving (-1, NaN)."""
    row = np.asarray(row, dtype=np.float64)
    cols = [s for s in range(len(row)) if s != bg]
    if n == 0 or not cols:
        return -1, np.float64(np.nan)
    x_len = np.float64(n)
    with np.errstate(all="ignore"):
        scores = [row[s] / x_len for s in cols]                                    # :74
        max_tup = max(enumerate(scores), key=operator.itemgetter(1))               # :75 (the first maximum)
        ubm_score = row[bg] / x_len                                                # :76
        margin = max_tup[1] - ubm_score
    if margin < threshold:                                                         # :78
        return -1, margin
    return cols[max_tup[0]], margin


def rule(sums, n_frames, bg, threshold):
    """-> (labels int32 [U], margins float64 [U]) of sums [U, S]."""
    sums = np.asarray(sums, dtype=np.float64)
    out = [rule_one(sums[u], int(n_frames[u]), bg, threshold) for u in range(len(sums))]
    return np.array([o[0] for o in out], dtype=np.int32).reshape(-1), np.array([o[1] for o in out], dtype=np.float64).reshape(-1)


# ---- the features path: a UBM (column 0), MAP-adapted speakers, utterances from the speakers and from unrelated models ----

# (K, D, UBM seed, speakers, first speaker seed, first utterance seed): chosen on the CPU with the oracle so that the widest gap
# between the sorted margins is far above what the parity gate can move a margin by (features_case checks it again)
SMALL = dict(K=8, D=5, ubm_seed=11, n_spk=4, spk_seed=400, utt_seed=7000)
HEADLINE = dict(K=512, D=39, ubm_seed=99, n_spk=3, spk_seed=500, utt_seed=7002)
LENGTHS = (1, 31, 32, 33, 300, 257, 33, 32, 31, 200)      # even positions: a speaker's frames; odd: an unrelated model's


def features_case(spec):
    from speaker_recognition_amd import synth
    ubm = synth.synth_gmm(spec["K"], spec["D"], spec["ubm_seed"])
    spk = [synth.synth_map_speaker(ubm, spec["spk_seed"] + s) for s in range(spec["n_spk"])]
    utts = []
    for i, n in enumerate(LENGTHS):
        if i % 2 == 0:
            src = spk[(i // 2) % len(spk)]
        else:
            src = synth.synth_gmm(spec["K"], spec["D"], 9000 + spec["ubm_seed"] + i)
        utts.append(synth.draw_frames(src, n, spec["utt_seed"] + i))
    return [ubm] + spk, utts


def oracle_sums(go, models, utts):
    X = np.concatenate(utts).astype(np.float64)
    off = np.concatenate([[0], np.cumsum([len(u) for u in utts])])
    ll = np.stack([go.score_batch(go.GMMParams(*m), X) for m in models])
    return np.array([[ll[s, off[u]:off[u + 1]].sum() for s in range(len(models))] for u in range(len(utts))])


def threshold_from(want_sums, n_frames):
    """The midpoint of the widest gap between the oracle's sorted margins, that gap, and what the gate can move a margin by:
    both sums of a margin may be off by GATE * max(1, |sum|), and the margin is their difference over the frame count."""
    _, margins = rule(want_sums, n_frames, 0, -np.inf)
    m = np.sort(margins)
    gaps = np.diff(m)
    i = int(np.argmax(gaps))
    per_frame = max(2 * GATE * max(1.0, float(np.max(np.abs(want_sums[u])))) / n_frames[u] for u in range(len(n_frames)))
    return float((m[i] + m[i + 1]) / 2), float(gaps[i]), per_frame


# ---- the serving stream's voice-activity scene: speech bursts and gaps of irregular length over a noise floor ----

def vad_scene(seed=11, fs=8000, win=8000):
    """(windows [n][win] int16, half a window apart, and the noise the detector is initialised with)"""
    from speaker_recognition_amd import synth
    step = win // 2
    audio = synth.synth_speech(3, 40.0, fs)
    rng = np.random.default_rng(seed)
    gate = np.zeros(len(audio), bool)
    t, on = 0, True
    while t < len(audio):
        d = int(rng.uniform(0.15, 1.2) * fs)
        gate[t:t + d] = on
        t, on = t + d, not on
    frng = np.random.default_rng(5)
    floor = frng.normal(0, 60, len(audio)).astype(np.int16)
    sc = (np.where(gate, audio // 2, 0) + floor).astype(np.int16)
    noise = frng.normal(0, 60, 3 * fs).astype(np.int16)
    n = (len(sc) - win) // step
    return np.stack([sc[i * step:i * step + win] for i in range(n)]), noise


def make_vad(noise, fs=8000):
    from speaker_recognition_amd.filters import VAD
    vad = VAD()
    vad.init_noise(fs, noise)
    return vad


# ---- models that put frames into the band where the reference's partial-product flushes decide (gmm_flush.hip) ----

def band_models(D=13, K=32, n_models=3, seed=2):
    """Every model sits 36.8 sigma from a feature value of 0 in ONE tight dimension (its own) and is wide in the others.  The
    stream's features are mean- and variance-normalised per utterance, so a few per cent of any utterance's frames score between
    -709 and -600 against each model (the band), others beyond it (clamped) and the rest before it: the recipe of
    tests/test_gpu_pipeline.py's band test, at the stream tests' 13 dimensions."""
    rng = np.random.default_rng(seed)
    r6 = np.vectorize(lambda v: float("%g" % v))
    models = []
    for s in range(n_models):
        mean = np.zeros((K, D))
        mean[:, s] = 1.84 + 0.01 * rng.standard_normal(K)
        sigma = np.full((K, D), 3.0)
        sigma[:, s] = 0.05
        models.append((np.full(K, 1.0 / K), r6(mean), sigma))
    return models
