"""The shared-sigma scoring engines at every chain length they are built for: the table behind tests/test_gpu_h2s_widths.py (the
device against the float64 oracle) and tests/test_h2s_width_cases_cpu.py (the table's own conditions, without a GPU).

The split-fp16 engine (score_engine 6, csrc/gmm_score_h2_shared.hip) contracts KQF = ceil(3D / 16) steps for the quadratic half and
KLF = ceil((3D + 2) / 16) for a model's linear half: 15 pairs over D = 1 .. 48.  DIMS holds, for every pair, the smallest and the
largest D that maps to it: the largest fills the last contraction step (or leaves one slot of it), the smallest leaves it almost
empty, so both ends of the slot tables are walked.  The fp32-grade fallback (score_engine 4, csrc/gmm_score_bx3_shared.hip) has
KQ = ceil(D / 16), KL = ceil((D + 1) / 16): six pairs.  Everything here is computed from those formulas, not from the C++ code.

Pure Python + numpy: the package (its synthetic models) is imported inside make_case only."""
import numpy as np

TOL = 1e-4                    # per frame: |dLL| <= TOL max(1, |LL|) (conftest.ll_close)
SUM_TOL = 1e-5                # an utterance's sum, relative to the oracle's (tests/test_gpu_h2c.py)
ENGINE_TOL = 1e-5             # per frame, engine 4 against engine 6 (test_h2s_offset_engine_accuracy_and_exceptions)
F16_MAX_AMP = 1000.0          # csrc/score_plan.hpp: what the dispatcher offers the split-fp16 engines
F16_MAX_SIGMA_RATIO = 256.0
MAX_DIM = 48                  # score_plan.cpp: shared_ok
LENS = [1, 31, 32, 33, 100, 8, 8, 8, 8, 385]      # 614 frames: packed tails, 17 full tiles = more than one 12-wave workgroup
ALONE = 4                     # the utterance of 100 frames that is also scored on its own
ROGUE = 6                     # the utterance whose last-but-one frame the rogue rows move by +60


def pair_of(D):
    """(KQF, KLF) of the split-fp16 shared-sigma engine"""
    return (-(-3 * D // 16), -(-(3 * D + 2) // 16))


def bx3_pair_of(D):
    """(KQ, KL) of the split-bf16 shared-sigma engine"""
    return (-(-D // 16), -(-(D + 1) // 16))


PAIRS = sorted(set(pair_of(D) for D in range(1, MAX_DIM + 1)))
BX3_PAIRS = sorted(set(bx3_pair_of(D) for D in range(1, MAX_DIM + 1)))
# pair -> its smallest and its largest D (one entry where they coincide)
DIMS = {p: sorted(set([min(D for D in range(1, MAX_DIM + 1) if pair_of(D) == p), max(D for D in range(1, MAX_DIM + 1) if pair_of(D) == p)]))
        for p in PAIRS}
ALL_DIMS = sorted(D for ds in DIMS.values() for D in ds)
# the split-bf16 engine: D = 16 and 32 are its two odd pairs, 4 / 31 / 47 / 48 the others
BX3_DIMS = [4, 16, 31, 32, 47, 48]

BASE = (50, 17)               # a ragged second mixture tile; blocks of 15 + 2
SIZES = [(32, 12), (96, 31)]  # one tile and one partial block (the smallest set the engine takes); three tiles, blocks of 15 + 15 + 1


def pair_id(p):
    return "%d-%d" % p


def rows():
    """every (D, K, S, rogue) of the table"""
    out = []
    for p in PAIRS:
        for D in DIMS[p]:
            out.append((D,) + BASE + (None,))
        D = DIMS[p][-1]
        for K, S in SIZES:
            out.append((D, K, S, None))
        out.append((D,) + BASE + (ROGUE,))
    return out


def h2p_fits(kqf, klf):
    """the pipelined kernel's LDS: a ring of two stages of four images and the 12 waves' quadratic-half fragments, in KiB"""
    return klf >= 2 and kqf <= klf and 2 * 4 * klf + 12 * kqf <= 160


def compact(D):
    """the compact image: parts of five half-steps of 8 slots (D + 1 <= 40) whose 8 steps are the flat order's KLF"""
    return pair_of(D)[1] == 8 and -(-(D + 1) // 8) == 5


def expected_kernel(D, shape):
    """what last_score_kernel() starts with for score_engine 6 and score_h2s_shape 1 .. 6"""
    q, l = pair_of(D)
    if shape in (3, 5, 6) and h2p_fits(q, l):
        if shape != 5 and compact(D):
            return "gmm_score_h2p_kernel<8,8,waves=12, pipelined in the wave>/compact"
        return "gmm_score_h2p_kernel<%d,%d,waves=12, pipelined in the wave> " % (q, l)
    if shape in (2, 3, 5, 6):
        return "gmm_score_h2s_kernel<%d,%d,waves=12> " % (q, l)
    if shape == 4:
        return "gmm_score_%s_kernel<%d,%d,waves=4 on one tile, models split> " % ("h2m" if l <= 9 else "h2s", q, l)
    assert shape == 1, shape
    return "gmm_score_h2s_kernel<%d,%d,waves=4> " % (q, l)


def expected_bx3_kernel(D):
    return "gmm_score_bx3_shared_kernel<%d,%d> " % bx3_pair_of(D)


_CASES = {}


def make_case(D, K, S, lens=LENS, rogue=None):
    """(models, utterances) -- the recipe of tests/test_gpu_h2c.py::_case: a UBM, S - 1 MAP speakers, utterance u drawn from speaker
    u mod (S - 1); `rogue` moves the last-but-one frame of that utterance by +60 on every dimension.  Made once, read-only."""
    key = (D, K, S, tuple(lens), rogue)
    if key not in _CASES:
        from speaker_recognition_amd import synth
        ubm = synth.synth_gmm(K, D, 1000 + 13 * D + K)
        models = [ubm] + [synth.synth_map_speaker(ubm, 7000 + s) for s in range(S - 1)]
        utts = [synth.draw_frames(models[1 + u % (S - 1)], n, 500 + u) for u, n in enumerate(lens)]
        if rogue is not None:
            utts[rogue] = utts[rogue].copy()
            utts[rogue][-2] += 60.0
        for a in utts:
            a.setflags(write=False)
        _CASES[key] = (models, utts)
    return _CASES[key]


_WANT = {}


def oracle_values(go, D, K, S, lens=LENS, rogue=None):
    """the float64 oracle's per-frame values [S, frames] of a row (its default mode, the reference's underflow rule on), made once"""
    key = (D, K, S, tuple(lens), rogue)
    if key not in _WANT:
        models, utts = make_case(D, K, S, lens, rogue)
        X = np.concatenate(utts).astype(np.float64)
        want = np.stack([go.score_batch(go.GMMParams(*m), X) for m in models])
        want.setflags(write=False)
        _WANT[key] = want
    return _WANT[key]


def offsets(lens=LENS):
    return np.concatenate([[0], np.cumsum(lens)])


def utterance_sums(want, lens=LENS):
    """[utterances, S]"""
    off = offsets(lens)
    return np.stack([want[:, off[u]:off[u + 1]].sum(axis=1) for u in range(len(lens))])


def conditioning(models):
    """(amp, sigma ratio) as pack_models_h2_shared takes them: amp = max_k sum_d ((mu_kd - centre_d) / sigma_kd)^2 over every model,
    the centre the mean of all models' means rounded to float32; the largest sigma_max / sigma_min of a dimension"""
    mu = np.stack([m[1] for m in models])                       # [S, K, D]
    sg = models[0][2]
    centre = mu.reshape(-1, mu.shape[-1]).mean(axis=0).astype(np.float32).astype(np.float64)
    amp = float(np.max(np.sum(((mu - centre) / sg) ** 2, axis=-1)))
    return amp, float(np.max(sg.max(axis=0) / sg.min(axis=0)))
