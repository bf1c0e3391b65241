"""The calls of tests/test_gpu_dense_parent_bits.py and of its recorder (tests/golden/make_dense_parent_bits.py): the smallest shapes
at which a move of the float64 dense layer (csrc/dense64.hip's GEMM and its launcher, csrc/dense64_dev.hpp's panel Cholesky and the
two inverse routines, csrc/dense64_plan.hpp's grids and LDS sizes) could go wrong -- the GEMM's tile and reduction edges, the four
operand orders, the unit diagonal, accumulating launches cut into chunks, both factorisation paths at one row, one panel and a panel
with a tail, the three modes of the block inverse, and blocks that do not factor.  Every case goes through public calls only and
takes a few milliseconds; the data come from the integer hash of tests/em_parent_cases.py: the same bits under any numpy.  Plain
module."""
import numpy as np

import em_parent_cases as ec

RANKS = (1, 16, 18)                 # one row; one Cholesky panel; a panel and a tail
LDS_ROWS = (0, 1)                   # the option jfa_lds_rows: the block in LDS (automatic); in place in global memory above one row


def _options(**kw):
    from speaker_recognition_amd import _lib
    for k, v in kw.items():
        _lib.set_option(k, v)


def _jfa_stats(seed, G, K, D):
    """-> N [G][K] >= 0, Fc [G][K D], E [K D] > 0"""
    N = 10.0 * np.abs(ec.noise(seed, (G, K)))
    E = 0.3 + np.abs(ec.noise(seed + 1, (K * D,)))
    Fc = np.repeat(N, D, axis=1) * ec.noise(seed + 2, (G, K * D)) + np.sqrt(np.repeat(N, D, axis=1)) * ec.noise(seed + 3, (G, K * D))
    return N, Fc, E


def _spd(seed, R, extra=4):
    """A well-conditioned symmetric positive definite [R][R], symmetric to the bit."""
    B = ec.noise(seed, (R + extra, R))
    return B.T @ B / (R + extra) + 0.5 * np.eye(R)


def _plda_rows(seed, R, speakers=20):
    """Speakers with 2 and 3 vectors in turn -- two count classes -> X [n][R], ids [n]"""
    ids = np.concatenate([np.full(2 + s % 2, s) for s in range(speakers)])
    X = 1.5 * ec.noise(seed, (speakers, R))[ids] + ec.noise(seed + 1, (ids.size, R))
    return X, ids


# ---- the cases: each -> {suffix: array} ----

def cosine(J, T, R, seed):
    """E X^T: M = J, N = T, the reduction R; A and B both k-fast"""
    from speaker_recognition_amd import plda
    return {"out": plda.cosine_score(ec.noise(seed, (J, R)), ec.noise(seed + 1, (T, R)))}


def jfa_factors_update(R, lds_rows, seed):
    """sr_jfa_factors with accumulators (L = I + N P with the unit diagonal, b, the factorisation's mode 0, A and C: the four operand
    orders) and sr_jfa_update on them (mode 1)"""
    from speaker_recognition_amd import jfa
    G, K, D = 9, 3, 4
    N, Fc, E = _jfa_stats(seed, G, K, D)
    W = 0.3 * ec.noise(seed + 4, (R, K * D))
    try:
        _options(jfa_lds_rows=lds_rows)
        with jfa.FactorEstimator(N, Fc, E) as est:
            y, A, C = est.factors(W, accumulate=True)
            bad = est.bad_groups
        W2, skipped = jfa.update_loadings(A, C, W, return_skipped=True)
    finally:
        _options(jfa_lds_rows=0)
    return {"y": y, "A": A, "C": C, "W": W2, "counts": np.array([bad, skipped], np.int64)}


def jfa_train_chunked(seed):
    """150 groups at R = 32 under a bound of 1 MiB: chunks of 128 groups, A and C continue from what they hold"""
    from speaker_recognition_amd import _lib, jfa
    G, K, D, R = 150, 3, 4, 32
    assert _lib.jfa_plan(G, K, D, R, 1 << 20)["n_chunks"] == 2
    N, Fc, E = _jfa_stats(seed, G, K, D)
    W = 0.3 * ec.noise(seed + 4, (R, K * D))
    try:
        _options(jfa_scratch_mib=1)
        with jfa.FactorEstimator(N, Fc, E) as est:
            W2, y = est.train(W, 2)
            skipped = est.skipped
    finally:
        _options(jfa_scratch_mib=1024)
    return {"W": W2, "y": y, "counts": np.array([skipped], np.int64)}


def jfa_bad_blocks(seed):
    """A group whose L is not finite (loadings of 1e160: P overflows): y = 0, Q = 0, counted, nothing added to A and C; a mixture of
    the update whose A_c is negative definite: W_c keeps its value, counted"""
    from speaker_recognition_amd import jfa
    G, K, D, R = 5, 3, 4, 18
    N, Fc, E = _jfa_stats(seed, G, K, D)
    W = 0.3 * ec.noise(seed + 4, (R, K * D))
    with jfa.FactorEstimator(N, Fc, E) as est:
        y, A, C = est.factors(np.full_like(W, 1e160), accumulate=True)
        bad = est.bad_groups
    A2 = np.stack([_spd(seed + 5, R), -np.eye(R), _spd(seed + 6, R)])
    W2, skipped = jfa.update_loadings(A2, ec.noise(seed + 7, (R, K * D)), W, return_skipped=True)
    return {"y": y, "A": A, "C": C, "W": W2, "counts": np.array([bad, skipped], np.int64)}


def jfa_score(Ru, lds_rows, mode, seed):
    """sr_jfa_score_integrated (the kscore kernel's factorisation) / sr_jfa_score_linear"""
    from speaker_recognition_amd import jfa
    T, J, K, D, Ry = 5, 3, 3, 4, 2
    N, F, E = _jfa_stats(seed, T, K, D)
    kd = K * D
    m, d = ec.noise(seed + 4, (kd,)), 0.2 * np.abs(ec.noise(seed + 5, (kd,)))
    v, u = 0.3 * ec.noise(seed + 6, (Ry, kd)), 0.3 * ec.noise(seed + 7, (Ru, kd))
    z, y, x = ec.noise(seed + 8, (J, kd)), ec.noise(seed + 9, (J, Ry)), ec.noise(seed + 10, (T, Ru))
    try:
        _options(jfa_lds_rows=lds_rows)
        out, counts = jfa.score_trials(F + np.repeat(N, D, axis=1) * m, N, m, E, d, v, u, z, y, x=x, mode=mode, return_counts=True)
    finally:
        _options(jfa_lds_rows=0)
    return {"out": out, "counts": np.array([counts["empty_segments"], counts["bad_segments"]], np.int64)}


def jfa_centred(seed):
    """sr_jfa_open_centred with a y v and an x u term: both products of the centring"""
    from speaker_recognition_amd import jfa
    n, K, D, Ry, Ru = 11, 3, 4, 2, 3
    N, F, E = _jfa_stats(seed, n, K, D)
    kd = K * D
    ids = (np.arange(n) * 3) % 4
    m = ec.noise(seed + 4, (kd,))
    v, u = 0.3 * ec.noise(seed + 5, (Ry, kd)), 0.3 * ec.noise(seed + 6, (Ru, kd))
    y, x = ec.noise(seed + 7, (4, Ry)), ec.noise(seed + 8, (n, Ru))
    with jfa.Stats.from_arrays(N, F) as stats:
        with jfa.centred(stats, m, E, ids, "speakers", v=v, y=y, u=u, x=x) as est:
            Ng, Fc = est.statistics()
    return {"N": Ng, "Fc": Fc}


def plda_train_score(R, lds_rows, seed):
    """sr_plda_train and sr_plda_score with two count classes: the block inverse (mode 0) and its log-determinants, M X^T"""
    from speaker_recognition_amd import plda
    X, ids = _plda_rows(seed, R)
    T = ec.noise(seed + 2, (7, R))
    try:
        _options(jfa_lds_rows=lds_rows)
        p = plda.PLDA().fit(X, ids, n_iter=2)
        out, counts = p.score(X[:9], ids[:9], T, return_counts=True)
    finally:
        _options(jfa_lds_rows=0)
    return {"mu": p.mu, "Sb": p.Sb, "Sw": p.Sw, "out": out,
            "counts": np.array([p.iterations, p.n_classes, p.stop, counts["bad_classes"]], np.int64)}


def plda_bad_blocks(seed):
    """An Sb that does not factor: the training stops at once with its code, the scores are exact zeros and every class is counted"""
    from speaker_recognition_amd import plda
    R = 18
    X, ids = _plda_rows(seed, R)
    p = plda.PLDA().fit(X, ids, n_iter=2, Sb0=-np.eye(R), Sw0=np.eye(R))
    out, counts = plda.PLDA(p.mu, -np.eye(R), np.eye(R)).score(X[:9], ids[:9], ec.noise(seed + 2, (7, R)), return_counts=True)
    return {"Sb": p.Sb, "Sw": p.Sw, "out": out, "counts": np.array([p.iterations, p.n_classes, p.stop, counts["bad_classes"]], np.int64)}


def whiten_long(seed):
    """One sum over more than PLDA_SUM_CHUNK = 65536 rows at R = 3: the second launch continues from C; the block inverse's mode 1"""
    from speaker_recognition_amd import plda
    mu, A = plda.fit_transform(ec.noise(seed, (65536 + 19, 3)) * np.array([1.0, 2.0, 0.5]), kind="whiten")
    return {"mu": mu, "A": A}


def backend_modes(lds_rows, seed):
    """whitening (mode 1 of the block inverse), gen_eig and lda_fit (mode 2), the projection, the diagonalised scorer"""
    from speaker_recognition_amd import plda
    R = 18
    X, ids = _plda_rows(seed, R)
    try:
        _options(jfa_lds_rows=lds_rows)
        mu, A = plda.fit_transform(X, kind="whiten")
        psi, V, info = plda.gen_eig(_spd(seed + 2, R), _spd(seed + 3, R), return_info=True)
        lda = plda.LDA().fit(X, ids, 5)
        Y = lda.transform(X[:6])
        diag = plda.DiagPLDA(mu, V, np.abs(psi)).score(X[:9], ids[:9], ec.noise(seed + 4, (7, R)))
    finally:
        _options(jfa_lds_rows=0)
    return {"mu": mu, "A": A, "psi": psi, "V": V, "status": np.array([info["status"]], np.int64), "lda_mu": lda.mu, "lda_A": lda.A,
            "lda_psi": lda.psi, "Y": Y, "diag": diag}


def score_norm_as2(seed):
    """as2 with J, the test segments and the cohort off the tile and the reduction step: the four products of score_norm.hip"""
    from speaker_recognition_amd import scorenorm
    J, T, C = 65, 63, 37
    out, counts = scorenorm.normalise(ec.noise(seed, (J, T)), "as2", enrol_cohort=ec.noise(seed + 1, (J, C)),
                                      cohort_test=ec.noise(seed + 2, (C, T)), top_n=10, return_counts=True)
    return {"out": out, "counts": np.array([counts["degenerate_enrol"], counts["degenerate_test"]], np.int64)}


def _cases():
    c = {}
    # an output one short of, equal to and one beyond a tile of 64 in each dimension; a reduction of 3, 16 and 17
    for J, T, R in ((63, 65, 3), (64, 64, 16), (65, 63, 17), (65, 65, 16)):
        c["cosine_%dx%dx%d" % (J, T, R)] = (cosine, (J, T, R, 100 + J + R))
    for R in RANKS:
        for lds in LDS_ROWS:
            c["jfa_r%d_lds%d" % (R, lds)] = (jfa_factors_update, (R, lds, 200 + R))
            c["plda_r%d_lds%d" % (R, lds)] = (plda_train_score, (R, lds, 300 + R))
            c["kscore_r%d_lds%d" % (R, lds)] = (jfa_score, (R, lds, "integrated", 400 + R))
    c["jfa_train_two_chunks"] = (jfa_train_chunked, (500,))
    c["jfa_blocks_that_do_not_factor"] = (jfa_bad_blocks, (510,))
    c["jfa_score_linear"] = (jfa_score, (3, 0, "linear", 520))
    c["jfa_open_centred"] = (jfa_centred, (530,))
    c["plda_blocks_that_do_not_factor"] = (plda_bad_blocks, (540,))
    c["whiten_two_sum_chunks"] = (whiten_long, (550,))
    for lds in LDS_ROWS:
        c["backend_lds%d" % lds] = (backend_modes, (lds, 560))
    c["score_norm_as2"] = (score_norm_as2, (570,))
    return c


CASES = _cases()
NAMES = list(CASES)


def run_case(name):
    f, args = CASES[name]
    return {k: np.ascontiguousarray(v) for k, v in f(*args).items()}
