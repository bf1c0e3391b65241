#!/usr/bin/env python3
"""CPU emulation (numpy) of the pipelined shared-sigma kernel's two contraction orders, to size the error of the COMPACT order
(csrc/score_shapes.hpp: h2c_map) beside the flat one BEFORE running its kernel:
  flat     [lo(A) hi(z) | hi(A) lo(z) | hi(A) hi(z)] cut into steps of 16 slots
  compact  H pairs x zl pairs | H pairs x zh pairs | (H,H) x (zl,zh) | L pairs x zh pairs | (L,0) x (zh,0)
Both hold the same part products (two fp16 parts per operand, three products); what differs is which 16 of them an MFMA step adds
up.  A step's 16 products are exact and summed exactly; the accumulator is rounded to fp32 after every step (conventions of
emulate_split.py).  Q = the quadratic chain, Q - O, then every model's linear chain on top of it, LL = O + log2 sum_k 2^value,
against the float64 log-sum-exp.
Usage: emulate_h2p_compact.py [K] [D] [S] [N]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speaker_recognition_amd import synth  # noqa: E402
from scripts.emulate_split import coeffs, lse2  # noqa: E402


def split2(v):
    v = v.astype(np.float32)
    hi = v.astype(np.float16).astype(np.float32)
    lo = (v - hi).astype(np.float16).astype(np.float32)
    return hi, lo


def flat_slots(D, linear):
    """[(a_part, b_part, index)] per slot; part 0 = hi, 1 = lo; index D = the constant; None = an empty slot."""
    s = [(1, 0, d) for d in range(D)]
    if linear:
        s.append((1, 0, D))
    s += [(0, 1, d) for d in range(D)] + [(0, 0, d) for d in range(D)]
    if linear:
        s.append((0, 0, D))
    s += [None] * (-len(s) % 16)
    return s


def compact_slots(D, linear):
    h = (D + 1 + 7) // 8
    np_, odd = h // 2, h & 1

    def half(a_part, b_part, p):
        out = []
        for j in range(8):
            d = 8 * p + j
            if d < D:
                out.append((a_part, b_part, d))
            elif linear and d == 8 * h - 1 and b_part == 0:       # the constant meets the 1 of zh only
                out.append((a_part, b_part, D))
            else:
                out.append(None)
        return out
    s = []
    for i in range(np_):
        s += half(0, 1, 2 * i) + half(0, 1, 2 * i + 1)
    for i in range(np_):
        s += half(0, 0, 2 * i) + half(0, 0, 2 * i + 1)
    if odd:
        s += half(0, 1, h - 1) + half(0, 0, h - 1)
    for i in range(np_):
        s += half(1, 0, 2 * i) + half(1, 0, 2 * i + 1)
    if odd:
        s += half(1, 0, h - 1) + [None] * 8
    return s


def chain(slots, a_parts, b_parts, init):
    """init [N, K] fp32; a_parts[p] [K, D(+1)], b_parts[p] [N, D(+1)]: the accumulator after every step of 16 slots, rounded to fp32."""
    acc = init.astype(np.float32)
    for k0 in range(0, len(slots), 16):
        step = np.zeros(acc.shape, np.float64)
        for sl in slots[k0:k0 + 16]:
            if sl is not None:
                ap, bp, d = sl
                step += np.outer(b_parts[bp][:, d].astype(np.float64), a_parts[ap][:, d].astype(np.float64))
        acc = (acc.astype(np.float64) + step).astype(np.float32)
    return acc


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    D = int(sys.argv[2]) if len(sys.argv) > 2 else 39
    S = int(sys.argv[3]) if len(sys.argv) > 3 else 17
    N = int(sys.argv[4]) if len(sys.argv) > 4 else 2000
    ubm = synth.synth_gmm(K, D, 7)
    models = [ubm] + [synth.synth_map_speaker(ubm, 100 + s) for s in range(S - 1)]
    X = np.concatenate([synth.draw_frames(models[u % S], N // 4, 42 + u, outlier_frac=0.0) for u in range(4)]).astype(np.float64)
    center = np.mean(np.concatenate([m[1] for m in models]), axis=0)
    es = np.round(np.mean(np.log2(ubm[2]), axis=0))                      # per-dimension power-of-two scale (pack_models_h2_shared)
    xp = ((X - center) / 2.0 ** es).astype(np.float32)
    for name, mk in (("flat", flat_slots), ("compact", compact_slots)):
        ms = [len([s for s in mk(D, lin) if s is not None]) for lin in (False, True)]
        assert ms == [3 * D, 3 * D + 2], ms
    same = all(sorted(s for s in flat_slots(D, lin) if s) == sorted(s for s in compact_slots(D, lin) if s) for lin in (False, True))
    print("K=%d D=%d S=%d N=%d: %d + %d products, the same multiset in both orders: %s; steps flat %d / %d, compact %d / %d" % (
        K, D, S, len(X), 3 * D, 3 * D + 2, same, len(flat_slots(D, False)) // 16, len(flat_slots(D, True)) // 16,
        len(compact_slots(D, False)) // 16, len(compact_slots(D, True)) // 16))
    bq = split2((xp.astype(np.float32) ** 2).astype(np.float32))
    one = np.ones((len(xp), 1), np.float32)
    zero = np.zeros((len(xp), 1), np.float32)
    bl = (np.concatenate([split2(xp)[0], one], axis=1), np.concatenate([split2(xp)[1], zero], axis=1))
    A2, _, _ = coeffs(ubm, center, es)
    aq = split2(A2)
    # the offset: the first model's own value (the kernel takes a pre-pass's; anything within a few nats does)
    A2r, A1r, Cr = coeffs(models[0], center, es)
    xd = xp.astype(np.float64)
    off = lse2(xd ** 2 @ A2r.T + xd @ A1r.T + Cr[None, :]).astype(np.float32)
    for name, mk in (("flat", flat_slots), ("compact", compact_slots)):
        q = chain(mk(D, False), aq, bq, np.zeros((len(xp), K), np.float32))
        q = (q - off[:, None]).astype(np.float32)
        worst, rms, cnt = 0.0, 0.0, 0
        for m in models:
            A2m, A1, C = coeffs(m, center, es)
            al = tuple(np.concatenate([p, c[:, None]], axis=1) for p, c in zip(split2(A1), split2(C)))
            v = chain(mk(D, True), al, bl, q)
            tot = np.sum(np.exp2(v.astype(np.float32)), axis=1, dtype=np.float32)
            got = off.astype(np.float64) + np.log2(tot.astype(np.float64))
            ref = lse2(xd ** 2 @ A2m.T + xd @ A1.T + C[None, :])
            ll_ref = ref * np.log(2.0)
            rel = np.abs(got - ref) * np.log(2.0) / np.maximum(1.0, np.abs(ll_ref))
            worst = max(worst, float(rel.max()))
            rms += float(np.sum(rel ** 2))
            cnt += len(rel)
        print("   %-8s per-frame error against float64 / max(1, |LL|): max %.3e  rms %.3e" % (name, worst, np.sqrt(rms / cnt)))


if __name__ == "__main__":
    main()
