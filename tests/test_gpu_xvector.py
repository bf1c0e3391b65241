"""GPU: the x-vector forward pass (csrc/xvector.hip) against the numpy restatement of tests/xvector_cases.py.  Every layer is checked
on the device's own input (teacher forcing through `tap`), so no tolerance compounds rounding flips; what must be equal to the bit
(the bf16 store against numpy's rounding of the fp32 store, a segment alone against the same segment anywhere in a batch, under
another scratch bound, in another run, through the other entry points) is compared with array_equal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import xvector_cases as xc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def xv(built_lib):
    from speaker_recognition_amd import _lib, xvector
    _lib.set_option("xvector_scratch_mib", 1024)
    _lib.set_option("debug_xvector_mfma_shape", 0)
    yield xvector
    _lib.set_option("xvector_scratch_mib", 1024)
    _lib.set_option("debug_xvector_mfma_shape", 0)


@pytest.fixture(scope="module")
def tile(xv):
    net = xv.XVector(xc.irregular_network())
    return net.tile_rows, net.tile_cols


def _split(rows, counts):
    out, at = [], 0
    for n in counts:
        out.append(rows[at:at + n])
        at += n
    assert at == len(rows)
    return out


def _check_layer(layer, xs, y32, y16):
    """xs: the layer's bf16-valued inputs per segment; y32 / y16: the device's fp32-store and bf16-store outputs, all segments"""
    span = layer["offsets"][-1] - layer["offsets"][0]
    counts = [len(x) - span for x in xs]
    worst, flips = 0.0, 0
    for x, a32, a16 in zip(xs, _split(y32, counts), _split(y16, counts)):
        a, S = xc.layer_forward(layer, x)
        worst = max(worst, xc.layer_gate_f32(layer, a, S, a32))
        flips += xc.layer_gate_bf16(layer, a, S, a16)
    print("layer gate: worst |y - a| / beta = %.3g, bf16 stores outside the interval: %d" % (worst, flips))
    assert worst <= 1.0 and flips == 0
    assert np.array_equal(y16, xc.bf16_rne(y32))          # the bf16 store is numpy's RNE of the same build's fp32 store


def test_layer_shapes(xv, tile):
    """A covering subset of C_in x C_out x offsets (xvector_cases.layer_cases), one layer through `tap`, both stores, two segments
    (5 and TM + 3 output frames: a short tile and a second workgroup)."""
    TM, TN = tile
    for i, (c_in, c_out, offsets, act, affine) in enumerate(xc.layer_cases(TN)):
        rng = np.random.default_rng(100 + i)
        layers = xc.single_layer_network(rng, c_in, c_out, offsets, act, affine)
        span = offsets[-1] - offsets[0]
        feats = [xc.features(rng, 5 + span, c_in), xc.features(rng, TM + 3 + span, c_in)]
        net = xv.XVector(layers)
        y32 = net.extract(feats, tap=0)
        y16 = net.extract(feats, tap=0, tap_bf16=True)
        assert y32.shape == (5 + TM + 3, c_out) and y32.dtype == np.float32
        _check_layer(layers[0], [xc.bf16_rne(f).astype(np.float64) for f in feats], y32, y16)


def test_row_edges(xv, tile):
    """Segments of 1, TM - 1, TM, TM + 1 and 2 TM + 3 output frames as windows of one ragged batch -- the first at the batch's first
    row, the last ending at its last row, the rows around every window and whole utterances between them filled with large distinct
    values -- and again each alone: inside the gate, and the same bits both ways."""
    TM, _ = tile
    rng = np.random.default_rng(7)
    offsets = (-1, 0, 2)
    layers = xc.single_layer_network(rng, 24, 33, offsets)
    net = xv.XVector(layers)
    rows = xc.row_edge_rows(TM)
    wins = [xc.features(rng, r + 3, 24) for r in rows]
    big = lambda n, k: (1.0e4 * (k + 1) + np.arange(n * 24, dtype=np.float32).reshape(n, 24))      # noqa: E731
    utts, segs = [], []
    for k, w in enumerate(wins):
        head = 0 if k == 0 else 3
        tail = 0 if k == len(wins) - 1 else 2
        utts.append(np.concatenate([big(head, k), w, big(tail, k + 10)], axis=0))
        segs.append((len(utts) - 1, head, len(w)))
        if k < len(wins) - 1:
            utts.append(big(9, k + 20))                      # an utterance no segment names
    together32 = net.extract(utts, segments=segs, tap=0)
    together16 = net.extract(utts, segments=segs, tap=0, tap_bf16=True)
    _check_layer(layers[0], [xc.bf16_rne(w).astype(np.float64) for w in wins], together32, together16)
    emb = net.extract(utts, segments=segs)
    for k, (w, part) in enumerate(zip(wins, _split(together32, rows))):
        assert np.array_equal(net.extract([w], tap=0), part), "segment %d alone" % k
        assert np.array_equal(net.extract([w]), emb[k:k + 1])


def test_pooling(xv):
    """n in {1, 2, 63, 64, 65, 1000} frames x C in {1, 33, 1500}, channel 0 constant (the floor is taken), against the pooling gate;
    the pooling reads the convert kernel's bf16 features (a network with no frame layer)."""
    for C in xc.POOL_C:
        rng = np.random.default_rng(C)
        layers = [xc.pool_layer(C, var_floor=1e-4), xc.make_layer(rng, "affine", 2 * C, 3, act="none", affine=False)]
        net = xv.XVector(layers)
        feats = [xc.pool_input(n, C) for n in xc.POOL_N]
        got = net.extract(feats, tap=0)
        assert got.shape == (len(feats), 2 * C) and got.dtype == np.float32
        for f, y in zip(feats, got):
            x = xc.bf16_rne(f).astype(np.float64)
            ratio, amp = xc.pool_gate(layers[0], x, y)
            assert ratio <= 1.0 and amp < xc.POOL_AMP_MAX, (C, len(f), ratio, amp)
            assert y[C] == np.float32(np.sqrt(1e-4))         # the constant channel's std is the floor's root


def _teacher_forced(xv, layers, feats):
    net = xv.XVector(layers)
    P = net.pool_index
    xs = [xc.bf16_rne(f).astype(np.float64) for f in feats]
    for l, layer in enumerate(layers):
        if l < P:
            y32, y16 = net.extract(feats, tap=l), net.extract(feats, tap=l, tap_bf16=True)
            _check_layer(layer, xs, y32, y16)
            span = layer["offsets"][-1] - layer["offsets"][0]
            xs = [a.astype(np.float64) for a in _split(y16, [len(x) - span for x in xs])]
        elif l == P:
            pooled = net.extract(feats, tap=l)
            for x, y in zip(xs, pooled):
                ratio, amp = xc.pool_gate(layer, x, y)
                assert ratio <= 1.0 and amp < xc.POOL_AMP_MAX, (l, ratio, amp)      # (the gate's condition, on this input too)
            xs = [xc.bf16_rne(pooled).astype(np.float64)]    # the pooled matrix, as the convert kernel rounds it
        else:
            last = l == len(layers) - 1
            y32 = net.extract(feats, tap=l)
            y16 = net.extract(feats, tap=l, tap_bf16=True)
            _check_layer(layer, xs, y32, y16)
            if last:
                emb = net.extract(feats)
                assert emb.shape == (len(feats), net.embedding_dim) and emb.dtype == np.float32
                assert np.array_equal(emb, y32)
            xs = [y16.astype(np.float64)]
    return net


def test_standard_network_teacher_forced(xv):
    """30 -> 512 (-2..2), 512 (-2,0,2), 512 (-3,0,3), 512, 1500, pooling, 512 on utterances of 15 (= context + 1), 200 and 457 frames;
    records the worst 1 - cosine against the unrounded float64 network (not gated: what bf16 costs)."""
    layers = xc.standard_network()
    feats = xc.network_test_features(xc.STD_TEST_FRAMES, xc.STD_TEST_SEED, 30)
    assert xc.context_of(layers) + 1 == 15
    net = _teacher_forced(xv, layers, feats)
    emb = net.extract(feats)
    worst = 0.0
    for f, e in zip(feats, emb):
        ref = xc.network_forward(layers, f, rounded=False)
        worst = max(worst, 1.0 - float(ref @ e.astype(np.float64)) / float(np.linalg.norm(ref) * np.linalg.norm(e.astype(np.float64))))
    print("worst 1 - cosine(device, unrounded float64 network) = %.3g" % worst)


def test_irregular_network_teacher_forced(xv):
    layers = xc.irregular_network()
    feats = xc.network_test_features(xc.IRR_TEST_FRAMES, xc.IRR_TEST_SEED, 24)
    net = _teacher_forced(xv, layers, feats)
    assert net.embedding_dim == 17 and net.context == 7


def test_bits(xv):
    """A segment's embedding: alone; first, middle and last in a batch of 70; under xvector_scratch_mib = 1 against the default; in two
    consecutive runs; through extract (host arrays) against extract_batch (resident)."""
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    layers = xc.irregular_network()
    net = xv.XVector(layers)
    rng = np.random.default_rng(11)
    lens = rng.integers(8, 400, size=70)
    feats = [xc.features(rng, int(T), 24) for T in lens]
    target = xc.features(rng, 211, 24)
    alone = net.extract([target])
    for pos in (0, 35, 69):
        batch = list(feats)
        batch[pos] = target
        got = net.extract(batch)
        assert np.array_equal(got[pos:pos + 1], alone), pos
        assert np.array_equal(net.extract(batch), got)                        # run to run
        resident = net.extract(Batch.from_features(batch))
        assert np.array_equal(resident, got)                                  # host arrays against a resident batch
        _lib.set_option("xvector_scratch_mib", 1)
        try:
            assert net.plan([len(b) for b in batch], scratch_bytes=1 << 20)["n_chunks"] > 1
            assert np.array_equal(net.extract(batch), got)
        finally:
            _lib.set_option("xvector_scratch_mib", 1024)


def test_embed_batch_matches_two_calls(xv):
    from speaker_recognition_amd import synth
    from speaker_recognition_amd.core import Batch, MfccExtractor
    rng = np.random.default_rng(12)
    layers = [xc.make_layer(rng, "tdnn", 13, 40, (-2, 0, 2)), xc.pool_layer(40), xc.make_layer(rng, "affine", 80, 16, act="none", affine=False)]
    net = xv.XVector(layers)
    ex = MfccExtractor(16000, win_length_ms=25, win_shift_ms=10)
    pcm = Batch.from_pcm([synth.synth_speech(s, 0.5) for s in range(3)])
    fused = ex.embed_batch(net, pcm)
    two = net.extract(ex.extract_batch(pcm))
    assert fused.shape == (3, 16) and np.array_equal(fused, two)
    feats = ex.extract_batch(pcm)
    assert np.array_equal(net.extract(_split(feats.download(), np.diff(feats.offsets()))), two)


def test_windows(xv):
    """extract_windows(window = context + 20, hop = 7) on one recording against the same windows cut out and submitted as separate
    utterances, to the bit (hop < window: overlapping; a second call with hop = window: abutting); a window past the end is refused."""
    from speaker_recognition_amd import _lib
    layers = xc.irregular_network()
    net = xv.XVector(layers)
    rng = np.random.default_rng(13)
    rec = xc.features(rng, 140, 24)
    w = net.context + 20
    for hop in (7, w):
        emb, table = net.extract_windows([rec], w, hop)
        assert len(table) == (140 - w) // hop + 1 and emb.shape == (len(table), 17)
        cut = net.extract([rec[f:f + n] for _, f, n in table])
        assert np.array_equal(emb, cut)
    with pytest.raises(_lib.SRError, match="segment 0 covers frames 120 .. 147 of utterance 0, which holds 140"):
        net.extract([rec], segments=[(0, 120, w)])


def test_refused_in_a_process_forked_after_runtime_use(xv, built_lib):
    """Both forward passes, the resident-batch one on a batch the parent made, in a child forked after the runtime was used."""
    import test_xvector_cpu
    test_xvector_cpu._fork_case(built_lib, xv, with_batch=True)


def test_back_end_takes_the_embeddings(xv):
    """40 segments through plda.fit_transform and plda.cosine_score against numpy's cosine of the same embeddings; the matrix goes
    into diarize.ahc.  No accuracy claim on a random network."""
    import plda_cases as pc
    from speaker_recognition_amd import diarize, plda
    layers = xc.irregular_network()
    net = xv.XVector(layers)
    rng = np.random.default_rng(14)
    emb = net.extract([xc.features(rng, 60, 24) for _ in range(40)]).astype(np.float64)
    labels = np.repeat(np.arange(8), 5)
    mu, A = plda.fit_transform(emb, labels, kind="wccn")
    proj = plda.transform(emb, mu, A)
    assert proj.shape == (40, 17) and np.isfinite(proj).all()
    S = plda.cosine_score(proj, proj)
    want = pc.cosine(proj, proj)
    assert pc.rel(S, want) <= pc.gate_cosine(17, want)
    lab, _ = diarize.ahc(1.0 - S, threshold=0.5)
    assert len(lab) == 40


def test_cli_embed(xv, tmp_path):
    from scipy.io import wavfile

    from speaker_recognition_amd import cli, synth
    from speaker_recognition_amd.core import Batch, MfccExtractor
    rng = np.random.default_rng(15)
    layers = [xc.make_layer(rng, "tdnn", 28, 48, (-1, 0, 1)), xc.pool_layer(48), xc.make_layer(rng, "affine", 96, 8, act="none", affine=False)]
    net = xv.XVector(layers)
    net.save(str(tmp_path / "net.npz"))
    sigs = [synth.synth_speech(s, 0.6) for s in (1, 2)]
    for k, s in enumerate(sigs):
        wavfile.write(str(tmp_path / ("u%d.wav" % k)), 16000, s)
    out = str(tmp_path / "emb.npz")
    cli.main(["-t", "embed", "-i", str(tmp_path / "*.wav"), "-m", str(tmp_path / "net.npz"), "--out", out])
    z = np.load(out)
    assert [os.path.basename(n) for n in z["names"]] == ["u0.wav", "u1.wav"] and z["embeddings"].shape == (2, 8)
    ex = MfccExtractor(16000, n_lpc=15)
    assert np.array_equal(z["embeddings"], ex.embed_batch(net, Batch.from_pcm(sigs)))
