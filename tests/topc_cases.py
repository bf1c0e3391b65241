"""Shared by tests/test_topc_cpu.py and tests/test_gpu_topc.py: top-C Gaussian selection (csrc/gmm_topc.hip; Reynolds, Quatieri &
Dunn 2000) restated in float64 numpy -- the terms, the stable descending selection, the log-sum-exp, the clamp and the sums -- and
the synthetic UBM + MAP-speaker cases.  Models and data as SURVEY.md 8d (speaker_recognition_amd.synth): mu ~ N(0, 1),
sigma ~ U(0.2, 1.5) floored at sqrt(1e-3), w ~ Dirichlet(1), speakers = the UBM with MAP-like mean shifts, frames drawn from the
speakers, fixed seeds.  Nothing here touches the GPU."""
import numpy as np

GATE = 1e-4                                             # |a - ref| <= GATE * max(1, |ref|) per frame
LN_DBL_MIN = float(np.log(np.finfo(np.float64).tiny))   # -708.396...: below it the reference's linear-domain sum is 0
LN_1E_15 = float(np.log(1e-15))                         # ... and its safe_log returns this (gmm.cc:34-38)
LENGTHS = (0, 1, 63, 64, 65, 300)                       # ragged tiles and an empty utterance in one batch


def constants(model):
    """ln w_k - sum_d ln(sqrt(2 pi) sigma_kd), [K]"""
    w, _, sigma = model
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(w, np.float64)) - np.sum(np.log(np.sqrt(2 * np.pi) * np.asarray(sigma, np.float64)), axis=1)


def terms(X, model):
    """t_k(x) for every frame and component, float64 [n, K]"""
    _, mean, sigma = model
    X = np.asarray(X, np.float64)
    out = np.empty((len(X), len(mean)))
    inv = 1.0 / (2.0 * np.asarray(sigma, np.float64) ** 2)
    c = constants(model)
    for a in range(0, len(X), 256):                     # (blocks of frames: [256, K, D] temporaries)
        d = X[a:a + 256, None, :] - np.asarray(mean, np.float64)[None]
        out[a:a + 256] = c[None] - np.sum(d * d * inv[None], axis=2)
    return out


def terms_at(X, model, sel):
    """t_k(x) for the components sel[n, C] only, float64 [n, C]"""
    _, mean, sigma = model
    X = np.asarray(X, np.float64)
    mean, sigma = np.asarray(mean, np.float64), np.asarray(sigma, np.float64)
    c = constants(model)
    out = np.empty(sel.shape)
    for a in range(0, len(X), 256):
        s = sel[a:a + 256]
        d = X[a:a + 256, None, :] - mean[s]
        out[a:a + 256] = c[s] - np.sum(d * d / (2.0 * sigma[s] ** 2), axis=2)
    return out


def select(t, C):
    """The C indices with the largest t, descending, equal values to the lower index first: int32 [n, C]"""
    return np.argsort(-t, axis=1, kind="stable")[:, :C].astype(np.int32)


def lse(a, axis=1):
    m = np.max(a, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.squeeze(m, axis) + np.log(np.sum(np.exp(a - m), axis=axis))


def clamp(ll):
    return np.where(ll < LN_DBL_MIN, LN_1E_15, ll)


def frame_ll(X, models, bg, C, selection=None, clamp_compat=True):
    """-> (LL [S, n] float64, selection [n, C]): the background column exact over all K, every other over the selection
    (`selection`: use this one -- the device's -- instead of the restatement's own)"""
    X = np.asarray(X, np.float64)
    t_bg = terms(X, models[bg])
    sel = select(t_bg, C) if selection is None else np.asarray(selection)
    out = np.empty((len(models), len(X)))
    for s, m in enumerate(models):
        out[s] = lse(t_bg) if s == bg else lse(terms_at(X, m, sel))
    return (clamp(out) if clamp_compat else out), sel


def sums(ll, offsets):
    """[U, S] float64 per-utterance sums of LL [S, n]"""
    return np.array([[ll[s, offsets[u]:offsets[u + 1]].sum() for s in range(len(ll))] for u in range(len(offsets) - 1)]).reshape(
        len(offsets) - 1, len(ll))


def argmax_first(row_sums, n_frames):
    """the first maximum over all columns, -1 for an utterance without frames"""
    return np.array([-1 if n == 0 else int(np.argmax(r)) for r, n in zip(row_sums, n_frames)], np.int32)


def brute_force(X, models, bg, C, clamp_compat=True):
    """The semantics again as plain loops over frames, models, components and dimensions (tiny cases only)."""
    import math
    S, n = len(models), len(X)
    out = np.zeros((S, n))
    picks = np.zeros((n, C), np.int32)

    def term(x, model, k):
        w, mean, sigma = model
        t = math.log(w[k])
        for d in range(len(x)):
            t -= math.log(math.sqrt(2 * math.pi) * sigma[k][d])
        for d in range(len(x)):
            t -= (x[d] - mean[k][d]) ** 2 / (2 * sigma[k][d] ** 2)
        return t

    for i in range(n):
        x = [float(v) for v in X[i]]
        K = len(models[bg][0])
        t = [term(x, models[bg], k) for k in range(K)]
        order = sorted(range(K), key=lambda k: (-t[k], k))[:C]
        picks[i] = order
        for s in range(S):
            vals = t if s == bg else [term(x, models[s], k) for k in order]
            m = max(vals)
            ll = m + math.log(sum(math.exp(v - m) for v in vals))
            out[s, i] = LN_1E_15 if clamp_compat and ll < LN_DBL_MIN else ll
    return out, picks


# ---- cases ----

def make_models(K, D, S, bg, seed):
    """S models: the UBM at column bg, S - 1 MAP-like speakers around it; (weights, mean, sigma) float64 each"""
    from speaker_recognition_amd import synth
    ubm = synth.synth_gmm(K, D, seed)
    spk = [synth.synth_map_speaker(ubm, seed + 100 + s) for s in range(S - 1)]
    return spk[:bg] + [ubm] + spk[bg:]


def make_utts(models, bg, lengths, seed):
    """frames drawn from the speakers in turn (from the UBM when it is alone), float32"""
    from speaker_recognition_amd import synth
    src = [m for s, m in enumerate(models) if s != bg] or [models[bg]]
    D = np.asarray(models[0][1]).shape[1]
    return [synth.draw_frames(src[i % len(src)], n, seed + 1000 + i) if n else np.zeros((0, D), np.float32)
            for i, n in enumerate(lengths)]


def offsets_of(utts):
    return np.concatenate([[0], np.cumsum([len(u) for u in utts])]).astype(np.int64)


# (K, C, D, S, bg): a pruned cross of K in {1, 5, 33, 64, 512}, C in {1, 3, 5, K}, D in {1, 13, 39, 40}, S in {1, 2, 65, 201},
# bg first / middle / last -- plus the sizes at which the device code takes another path: D = 16 | 17 and 40 | 41 and 64 (the
# padded row widths 16, 40, 64), C = 6, 8 | 9 (register slots 1, 5, 8; above 8 the rank kernel), S = 257 and 300 (more than one
# block of 256 models).  Every case scores LENGTHS: 493 frames.
GRID = [
    (1, 1, 1, 1, 0),
    (5, 1, 13, 2, 0),
    (5, 3, 40, 2, 1),
    (5, 5, 39, 65, 32),
    (5, 1, 16, 2, 0),
    (5, 3, 17, 2, 1),
    (5, 3, 64, 65, 0),
    (5, 1, 13, 257, 256),
    (5, 3, 13, 300, 299),
    (33, 5, 39, 1, 0),
    (33, 3, 13, 65, 64),
    (33, 5, 39, 2, 0),
    (33, 5, 41, 3, 1),
    (33, 6, 39, 65, 3),
    (33, 8, 13, 2, 0),
    (33, 9, 13, 2, 0),
    (33, 33, 1, 2, 1),
    (64, 1, 39, 201, 0),
    (64, 5, 40, 201, 100),
    (64, 5, 39, 201, 200),
    (64, 64, 13, 2, 0),
    (512, 3, 13, 2, 1),
    (512, 5, 39, 65, 0),
    (512, 512, 39, 2, 0),
]


def case_seed(K, C, D, S, bg):
    return 1000 * K + 37 * D + 5 * S + bg + C
