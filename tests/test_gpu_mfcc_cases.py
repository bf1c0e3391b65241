"""The MFCC kernels at every dispatch branch and parameter edge (tests/mfcc_cases.py) against oracle/mfcc_oracle.py: the four frame
kernels of csrc/mfcc.hip and csrc/mfcc_f64.hip and cmvn_delta_kernel at its three column paddings.  Every test first asks
sr_mfcc_plan, on the device it runs on, which kernel the launch takes -- the link between "ran" and "ran that branch";
tests/test_mfcc_cases_cpu.py shows without a GPU that the table covers every branch and that these comparisons catch each of
nine plausible kernel mistakes.  Every figure is printed before it is asserted (run with -s)."""
import numpy as np
import pytest

import frontend_cases as fc
import mfcc_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_mfcc_options(built_lib):
    """every test starts (and leaves) with the defaults: float64 spectrum, register-resident kernel where it applies"""
    from speaker_recognition_amd import _lib
    _lib.set_option("mfcc_precision", 2)
    _lib.set_option("mfcc_generic", 0)
    yield
    _lib.set_option("mfcc_precision", 2)
    _lib.set_option("mfcc_generic", 0)


def _set(precision, generic):
    from speaker_recognition_amd import _lib
    _lib.set_option("mfcc_precision", precision)
    _lib.set_option("mfcc_generic", generic)


def _planned(ex, precision, generic, kind, n_frames):
    from speaker_recognition_amd import _lib
    return _lib.mfcc_plan(ex._h, precision, generic, 0 if kind == "int16" else 1, n_frames, 0)


def _split(batch):
    X, off = batch.download(), batch.offsets()
    return [X[off[i]:off[i + 1]].astype(np.float64) for i in range(len(off) - 1)]


@pytest.mark.parametrize("precision", [2, 0])
@pytest.mark.parametrize("kind", ["int16", "float32"])
@pytest.mark.parametrize("name", [c.name for c in mc.CASES])
def test_case_vs_oracle(built_lib, name, kind, precision):
    """raw cepstra and extract_batch at nd 0, 1, 2 per utterance against the oracle, with the kernel the row names (mfcc_generic 0)
    and with the generic one (1); the two agree within the delta bound"""
    from speaker_recognition_amd.core import Batch, MfccExtractor
    c = mc.CASE[name]
    sigs, refs = mc.pcm(name, kind), mc.reference(name, kind)
    ex = MfccExtractor(c.fs, **mc.kw(c))
    n_frames = sum(ex.num_frames(len(s)) for s in sigs)
    assert ex.num_frames(len(sigs[3])) == 0 and ex.num_frames(len(sigs[4])) > 0
    got = {}
    for generic in (0, 1):
        plan = _planned(ex, precision, generic, kind, n_frames)
        want = c.expect["k%d" % precision] if generic == 0 else (mc.F64G if precision == 2 else mc.F32G)
        assert plan["kernel"] == want, (name, precision, generic, plan)
        assert plan["cp"] == c.expect["cp"]
        _set(precision, generic)
        pcm = Batch.from_pcm(list(sigs))
        raw = _split(ex.extract_batch(pcm, nd=0, cmvn=False))
        feats = {nd: _split(ex.extract_batch(pcm, nd=nd)) for nd in (0, 1, 2)}
        got[generic] = feats
        for u, ref in enumerate(refs):
            if ref is None:
                assert raw[u].shape[0] == 0 and all(feats[nd][u].shape[0] == 0 for nd in feats), (name, u)
                continue
            assert raw[u].shape == ref["raw"].shape and np.all(np.isfinite(raw[u]))
            errs = mc.errors(c, raw[u], {nd: feats[nd][u] for nd in feats}, ref)
            for q, (err, scale) in errs.items():
                print("MFCCERR %s %s p%d g%d %s u%d %s %.3e bound %.3e" % (name, kind, precision, generic, plan["kernel"], u, q, err,
                                                                           mc.tolerance(precision, q) * scale))
            for q, (err, scale) in errs.items():
                assert err < mc.tolerance(precision, q) * scale, (name, kind, precision, generic, u, q, err)
    for nd in (0, 1, 2):
        for u in range(len(sigs)):
            if got[0][nd][u].size:
                d = float(np.max(np.abs(got[0][nd][u] - got[1][nd][u])))
                assert d < mc.GENERIC_AGREE[precision], (name, nd, u, d)


@pytest.mark.parametrize("precision", [2, 0])
@pytest.mark.parametrize("name", ["default_16k", "ceps17", "ceps33"])
def test_deltas_without_cmvn(built_lib, name, precision):
    """cmvn = 0 with nd 1 and 2 (n_ceps 13, 17, 33: 16, 32 and 64 CMVN columns): the plain differences of the raw cepstra.  Against the
    oracle's diff_feature(raw cepstra) within the raw bound t times 1, 2 and 4 (a first difference carries the error of two terms,
    a second one of four); and EXACTLY the float32 rounding of the float64 differences of the device's own raw cepstra."""
    from oracle import mfcc_oracle as mo
    from speaker_recognition_amd.core import Batch, MfccExtractor
    c = mc.CASE[name]
    sigs, refs = mc.pcm(name, "int16"), mc.reference(name, "int16")
    ex = MfccExtractor(c.fs, **mc.kw(c))
    _set(precision, 0)
    assert _planned(ex, precision, 0, "int16", 100)["cp"] == {13: 16, 17: 32, 33: 64}[c.n_ceps]
    pcm = Batch.from_pcm(list(sigs))
    raw = [r.astype(np.float32) for r in _split(ex.extract_batch(pcm, nd=0, cmvn=False))]
    C = c.n_ceps
    for nd in (1, 2):
        out = ex.extract_batch(pcm, nd=nd, cmvn=False)
        assert out.dim == C * (nd + 1)
        X, off = out.download(), out.offsets()
        for u, ref in enumerate(refs):
            g = X[off[u]:off[u + 1]]
            if ref is None:
                assert g.shape[0] == 0
                continue
            r64 = raw[u].astype(np.float64)
            t = np.arange(nd, r64.shape[0])
            own = [r64[t], r64[t] - r64[t - 1]] + ([(r64[t] - r64[t - 1]) - (r64[t - 1] - r64[t - 2])] if nd == 2 else [])
            assert np.array_equal(g, np.concatenate(own, axis=1).astype(np.float32)), (name, nd, u)
            want = mo.diff_feature(ref["raw"], nd)
            bound = mc.TOL[precision]["raw"] * max(1.0, float(np.abs(ref["raw"]).max()))
            for j, factor in enumerate((1, 2, 4)[:nd + 1]):
                err = float(np.max(np.abs(g[:, j * C:(j + 1) * C] - want[:, j * C:(j + 1) * C])))
                print("MFCCRAWD %s p%d nd%d u%d block%d %.3e bound %.3e" % (name, precision, nd, u, j, err, factor * bound))
                assert err < factor * bound, (name, nd, u, j, err)


def _large(ex, precision, sigs, min_fpw):
    """one large ragged batch: the planned kernel is the fast one with at least `min_fpw` frames per wave; every utterance's raw cepstra
    are bit-identical to the same utterance extracted alone; the sampled utterances (first, last, around evenly spaced frames) meet
    the oracle bounds, raw and after CMVN with both deltas"""
    from oracle import mfcc_oracle as mo
    from speaker_recognition_amd.core import Batch
    n_frames = sum(ex.num_frames(len(s)) for s in sigs)
    plan = _planned(ex, precision, 0, "int16", n_frames)
    print("MFCCLARGE p%d: %d utterances, %d frames, %s" % (precision, len(sigs), n_frames, plan))
    assert plan["kernel"] == (mc.F64F if precision == 2 else mc.F32F) and plan["frames_per_wave"] >= min_fpw, plan
    assert any(ex.num_frames(len(s)) == 0 for s in sigs[1:-1])             # an utterance without frames inside the batch
    _set(precision, 0)
    pcm = Batch.from_pcm(list(sigs))
    out = ex.extract_batch(pcm, nd=0, cmvn=False)
    X, off = out.download(), out.offsets()
    assert off[-1] == n_frames and np.all(np.isfinite(X))
    feats = _split(ex.extract_batch(pcm, nd=2))
    for u, s in enumerate(sigs):
        if off[u + 1] == off[u]:
            assert ex.num_frames(len(s)) == 0
            continue
        alone = ex.extract_batch(Batch.from_pcm([s]), nd=0, cmvn=False).download()
        assert np.array_equal(alone, X[off[u]:off[u + 1]]), (u, len(s))
    picked = mc.sample_frames(off, 200)
    assert sum(off[u + 1] - off[u] for u in picked) >= 200
    c = mc.Case("large", mc.LARGE_FS, 10, 10, 2048, 50, 13, 0.95, {})
    worst = {}
    for u in picked:
        ref_raw = mo.get_mfcc_extractor(mc.LARGE_FS, **mc.LARGE_KW).raw_cepstra(sigs[u].astype(np.float64))
        z = (ref_raw - ref_raw.mean(axis=0)) / ref_raw.std(axis=0) if ref_raw.shape[0] > 1 else ref_raw
        if ref_raw.shape[0] <= 2:
            errs = mc.errors(c, X[off[u]:off[u + 1]].astype(np.float64), {}, dict(raw=ref_raw))
        else:
            errs = mc.errors(c, X[off[u]:off[u + 1]].astype(np.float64), {2: feats[u]}, dict(raw=ref_raw, nd2=mo.diff_feature(z, 2)))
        for q, (err, scale) in errs.items():
            print("MFCCLARGEERR p%d u%d (%d frames) %s %.3e bound %.3e" % (precision, u, off[u + 1] - off[u], q, err, mc.tolerance(precision, q) * scale))
            worst[q] = max(worst.get(q, 0.0), err / (mc.tolerance(precision, q) * scale))
    assert all(v < 1.0 for v in worst.values()), worst


def _n_cu(ex):
    """compute units of the device, from the plan itself: one frame per wave fills one round of 8-wave workgroups, one per CU"""
    from speaker_recognition_amd import _lib
    n = 8
    while _lib.mfcc_plan(ex._h, 2, 0, 0, n, 0)["frames_per_wave"] == 1:
        n *= 2
    lo, hi = n // 2, n                      # frames_per_wave is 1 up to n_cu * 8 frames
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _lib.mfcc_plan(ex._h, 2, 0, 0, mid, 0)["frames_per_wave"] == 1 else (lo, mid)
    assert lo % 8 == 0
    return lo // 8


def test_ragged_batch_with_several_frames_per_wave(built_lib):
    """8 kHz, frames of 80 samples: a wave of either fast kernel walks a contiguous range of frames across utterance boundaries
    (utterances without frames among them), prefetching the next frame's samples -- float64 with at least 3 frames per wave, fp32
    with at least 2"""
    from speaker_recognition_amd.core import MfccExtractor
    ex = MfccExtractor(mc.LARGE_FS, **mc.LARGE_KW)
    n_cu = _n_cu(ex)
    sigs, kw = fc.large_batch(n_cu * 48 + 200)             # six rounds of n_cu * 8 float64 waves, four of n_cu * 12 fp32 ones
    assert kw == {k: mc.LARGE_KW[k] for k in kw}
    _large(ex, 2, sigs, 3)
    _large(ex, 0, sigs, 2)


def test_ragged_batch_with_more_than_eight_frames_per_wave(built_lib):
    """the fp32 fast kernel's third frames-per-wave branch: more than 8 rounds' worth of frames -- 24 rounds here, about 74,000 frames
    on 256 compute units -- go to four times as many waves as fit the chip at once, 8 frames each at the least (one round would
    give 25 per wave)"""
    from speaker_recognition_amd.core import MfccExtractor
    ex = MfccExtractor(mc.LARGE_FS, **mc.LARGE_KW)
    n_cu = _n_cu(ex)
    sigs, _kw = fc.large_batch(n_cu * 12 * 24 + 200, seed=6)
    n_frames = sum(ex.num_frames(len(s)) for s in sigs)
    assert n_frames > 8 * n_cu * 12
    assert _planned(ex, 0, 0, "int16", n_frames)["frames_per_wave"] == max(8, -(-n_frames // (4 * n_cu * 12)))
    _large(ex, 0, sigs, 8)


@pytest.mark.parametrize("precision", [2, 0])
@pytest.mark.parametrize("name", ["default_16k", "ceps17", "fft512_len400_24f", "fft32"])
def test_edge_lengths(built_lib, name, precision):
    """5 FRAME_LEN samples give no frames, 5 FRAME_LEN + 1 give frames; the utterance without frames first, last or between two
    others changes nothing about its neighbours (raw cepstra bit-identical to each utterance alone; features too)"""
    from speaker_recognition_amd.core import Batch, MfccExtractor
    c = mc.CASE[name]
    a, b, _long, z, e = mc.pcm(name, "int16")
    ex = MfccExtractor(c.fs, **mc.kw(c))
    L = ex.FRAME_LEN
    assert len(z) == 5 * L and len(e) == 5 * L + 1 and ex.num_frames(len(z)) == 0
    assert ex.num_frames(len(e)) == (4 * L + 1) // ex.FRAME_SHIFT + 1
    for generic in (0, 1):
        _set(precision, generic)
        alone = {id(s): (ex.extract_batch(Batch.from_pcm([s]), nd=0, cmvn=False).download(), ex.extract_batch(Batch.from_pcm([s]), nd=2).download())
                 for s in (a, b, e)}
        for order in ([z, a, b], [a, z, b], [a, b, z], [z, e, z], [e, z, z, a], [z, z, e]):
            pcm = Batch.from_pcm(order)
            raw, f2 = ex.extract_batch(pcm, nd=0, cmvn=False), ex.extract_batch(pcm, nd=2)
            R, off, F, foff = raw.download(), raw.offsets(), f2.download(), f2.offsets()
            for u, s in enumerate(order):
                if s is z:
                    assert off[u + 1] == off[u] and foff[u + 1] == foff[u]
                else:
                    assert off[u + 1] - off[u] == ex.num_frames(len(s)) and foff[u + 1] - foff[u] == ex.num_frames(len(s)) - 2
                    assert np.array_equal(R[off[u]:off[u + 1]], alone[id(s)][0]), (name, generic, u)
                    assert np.array_equal(F[foff[u]:foff[u + 1]], alone[id(s)][1]), (name, generic, u)
