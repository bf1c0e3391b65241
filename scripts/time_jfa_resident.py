#!/usr/bin/env python3
"""What the JFA leg costs with the statistics resident on the device (csrc/jfa_stats.hip, jfa.Stats) against the host-array route,
both in one process, alternating; one JSON line on stdout.

    python scripts/time_jfa_resident.py [--out profiles/r20_jfa_resident.json] [--reps 5] [--shapes a,b] [--sessions 1000]

Two shapes: (a) 1000 sessions x 1000 frames against 512 x 39 as 200 speakers x 5, R = 100; (b) 1000 sessions x 3000 frames
against the reference's own 256 x 13 JFA UBM (tests/golden/jfa_ubm.npz), same grouping and rank.  Frames are unit normal draws:
the timing does not depend on their values.  Per stage and route: the host clock around a device synchronise (min, median, max of
--reps runs after one warm-up; spread = max - min) and the device time of one run from the library's event timers (HIP events on
the library's stream, every SR_T_BW_* / SR_T_JFA_* kind summed).  Stages: the statistics; the centring in front of train_v, train_u
and train_d (host route: jfa.py's numpy centring and the upload through sr_jfa_open; resident: sr_jfa_open_centred); ten train
iterations on the handle either route made; ten z / d iterations (host route: jfa.estimate_z_and_d ten times; resident: one
sr_jfa_zd); both scorers at 200 models x the sessions; the whole chain statistics -> train_v -> train_u -> train_d ->
score_dot_product.  "resident_not_slower": the resident median is no more than the host-array median plus the larger of the two
spreads.  The centring kernel's achieved bytes per second (bytes from the shapes: F, the x u product and N read once, the
shift's rows read once, Fc written once) against the 8.0 TB/s HBM3E figure of the data sheet and the 6.29 TB/s a float4 copy
reaches."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def device_ms(fn):
    """Device time of one run: every bw / jfa timer kind, from HIP events on the library's stream."""
    from speaker_recognition_amd import _lib
    _lib.profile_enable(True)
    _lib.profile_reset()
    fn()
    kinds = {k: _lib.profile_get(k)[0] for k in range(_lib.T_BW_LSE, _lib.T_JFA_UPDATE + 1)}
    _lib.profile_enable(False)
    return float(sum(kinds.values())), kinds


def stage(name, host_fn, resident_fn, reps, out, closing=lambda r: None):
    """Both routes alternating run by run, after one warm-up of each."""
    from speaker_recognition_amd import _lib
    runs = {"host_arrays": [], "resident": []}
    for fn in (host_fn, resident_fn):                  # warm-up
        closing(fn())
        _lib.synchronize()
    for _ in range(reps):
        for key, fn in (("host_arrays", host_fn), ("resident", resident_fn)):
            t0 = time.perf_counter()
            r = fn()
            _lib.synchronize()
            runs[key].append((time.perf_counter() - t0) * 1e3)
            closing(r)
    rec = {}
    for key, fn in (("host_arrays", host_fn), ("resident", resident_fn)):
        t = runs[key]
        rec[key] = {"min_ms": float(min(t)), "median_ms": float(np.median(t)), "max_ms": float(max(t)), "spread_ms": float(max(t) - min(t))}
        keep = []
        rec[key]["device_ms"], kinds = device_ms(lambda: keep.append(fn()))
        rec[key]["device_kind_ms"] = {str(k): v for k, v in kinds.items() if v > 0}
        for r in keep:
            closing(r)
    h, r = rec["host_arrays"], rec["resident"]
    rec["resident_not_slower"] = bool(r["median_ms"] <= h["median_ms"] + max(h["spread_ms"], r["spread_ms"]))
    rec["host_over_resident"] = h["median_ms"] / r["median_ms"] if r["median_ms"] > 0 else None
    out[name] = rec
    note("  %-22s host arrays %9.2f ms (spread %.2f), resident %9.2f ms (spread %.2f), device %.2f / %.2f ms"
         % (name, h["median_ms"], h["spread_ms"], r["median_ms"], r["spread_ms"], h["device_ms"], r["device_ms"]))
    return rec


def close(r):
    if hasattr(r, "close"):
        r.close()
    elif isinstance(r, tuple):
        for a in r:
            close(a)


def shape(name, n, frames, ubm, speakers, R, J, reps):
    from speaker_recognition_amd import _lib, jfa
    from speaker_recognition_amd.core import Batch, ModelSet
    note("shape", name)
    w, mu, var = ubm
    K, D = mu.shape
    kd = K * D
    rng = np.random.default_rng(20)
    feats = Batch.from_features([rng.standard_normal((frames, D)).astype(np.float32) for _ in range(n)])
    ms = ModelSet([jfa.as_ubm(ubm)])
    ids = np.repeat(np.arange(speakers), n // speakers).astype(np.int64)
    m, E = mu.reshape(-1), var.reshape(-1)
    out = {"shape": name, "sessions": n, "frames": frames, "K": K, "D": D, "speakers": speakers, "R": R, "models": J, "reps": reps}
    stage("statistics", lambda: ms.bw_stats(feats, 0), lambda: ms.bw_stats(feats, 0, resident=True), reps, out, close)
    N, F = ms.bw_stats(feats, 0)
    st = ms.bw_stats(feats, 0, resident=True)
    v0, u0 = jfa.random_loadings(R, E, 0), jfa.random_loadings(R, E, 1)
    d0 = jfa.random_loadings(1, E, 2)[0]
    y = jfa.estimate_y_and_v(st, None, None, m, E, 0, v0, 0, 0, 0, 0, ids)
    x = jfa.estimate_x_and_u(st, None, None, m, E, 0, v0, u0, 0, y, 0, ids)

    # the host-array route's centring, as jfa.train_v / train_u / train_d (estimate_z_and_d) write it, then the upload
    def host_centre_v():
        Fh, Nh, Nx, mm, EE = jfa._stats(F, N, m, E)
        Ns = jfa._speaker_sums(Nh, ids, speakers)
        Fs = jfa._speaker_sums(Fh, ids, speakers) - mm * jfa._speaker_sums(Nx, ids, speakers)
        return jfa.FactorEstimator(Ns, Fs, EE)

    def host_centre_u():
        Fh, Nh, Nx, mm, EE = jfa._stats(F, N, m, E)
        return jfa.FactorEstimator(Nh, Fh - Nx * (mm + y @ v0)[ids], EE)

    def host_centre_d():
        Fh, Nh, Nx, mm, EE = jfa._stats(F, N, m, E)
        Ns = jfa._speaker_sums(Nx, ids, speakers)
        Fs = jfa._speaker_sums(Fh - jfa._times(x, u0, n, kd) * Nx, ids, speakers) - (mm + jfa._times(y, v0, speakers, kd)) * Ns
        return jfa.FactorEstimator(jfa._speaker_sums(Nh, ids, speakers), Fs, EE)

    stage("centring_train_v", host_centre_v, lambda: jfa.centred(st, m, E, ids, "speakers"), reps, out, close)
    stage("centring_train_u", host_centre_u, lambda: jfa.centred(st, m, E, ids, "sessions", v=v0, y=y), reps, out, close)
    rec = stage("centring_train_d", host_centre_d, lambda: jfa.centred(st, m, E, ids, "speakers", v=v0, y=y, u=u0, x=x), reps, out, close)
    # the centring kernel's rate, from the resident run's streaming kind (it also holds the group-count kernel: K / (K D) of the bytes)
    stream_ms = rec["resident"]["device_kind_ms"].get(str(_lib.T_JFA_GRAM), 0.0)
    nbytes = 8.0 * (2 * n * kd + n * K + speakers * (2 * kd + K) + kd)          # F, x u, N; y v rows, Fc, N_g; m
    out["centring_kernel"] = {"bytes": nbytes, "device_ms": stream_ms, "tb_per_s": nbytes / (stream_ms * 1e-3) / 1e12 if stream_ms > 0 else None,
                              "hbm_spec_tb_per_s": HBM_SPEC_TBS, "hbm_copy_tb_per_s": HBM_COPY_TBS, "bound": "HBM bandwidth (a stream: 1 FMA per 24 bytes)"}
    if stream_ms > 0:
        out["centring_kernel"]["share_of_copy_rate"] = out["centring_kernel"]["tb_per_s"] / HBM_COPY_TBS
    with host_centre_v() as eh, jfa.centred(st, m, E, ids, "speakers") as er:
        stage("train_10_iterations", lambda: eh.train(v0, 10), lambda: er.train(v0, 10), reps, out)
    with jfa.centred(st, m, E, ids, "speakers", v=v0, y=y, u=u0, x=x) as er:
        def host_zd():
            d = d0
            for _ in range(10):
                _, d = jfa.estimate_z_and_d(F, N, None, m, E, d, v0, u0, 0, y, x, ids, nargout=2)
            return d
        stage("zd_10_iterations", host_zd, lambda: er.z_and_d(d0, n_iter=10)[0], reps, out)
    rng = np.random.default_rng(21)
    ym, zm = rng.standard_normal((J, R)), 0.1 * rng.standard_normal((J, kd))
    stage("score_integrated", lambda: jfa.score_trials(F, N, m, E, d0, v0, u0, zm, ym), lambda: jfa.score_trials(st, None, m, E, d0, v0, u0, zm, ym),
          reps, out)
    stage("score_linear", lambda: jfa.score_trials(F, N, m, E, d0, v0, u0, zm, ym, x, mode="linear"),
          lambda: jfa.score_trials(st, None, m, E, d0, v0, u0, zm, ym, x, mode="linear"), reps, out)

    def chain(resident):
        if resident:
            s = ms.bw_stats(feats, 0, resident=True)
            a = (s, None)
        else:
            Nc, Fc = ms.bw_stats(feats, 0)
            a = (Fc, Nc)
        v = jfa.train_v(*a, ids, ubm, ny=R, niter=10)
        u = jfa.train_u(*a, ids, ubm, v, nx=R, niter=10, seed=1)
        d = jfa.train_d(*a, ids, ubm, v, u, niter=10, seed=2)
        if resident:
            with s.take(np.arange(J)) as trn:
                sc = jfa.score_dot_product(trn, s, ubm, v, u, d)
            s.close()
        else:
            sc = jfa.score_dot_product((a[0][:J], a[1][:J]), a, ubm, v, u, d)
        return sc

    stage("whole_chain", lambda: chain(False), lambda: chain(True), reps, out)
    st.close()
    out["every_stage_resident_not_slower"] = all(v["resident_not_slower"] for v in out.values() if isinstance(v, dict) and "resident_not_slower" in v)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--sessions", type=int, default=1000)
    args = ap.parse_args()
    import bw_cases as bc
    from speaker_recognition_amd import _lib
    want = args.shapes.split(",")
    n = args.sessions
    shapes = []
    if "b" in want:
        shapes.append(shape("b_%dx3000_fixture256x13" % n, n, 3000, bc.fixture_ubm(), n // 5, 100, min(200, n), args.reps))
    if "a" in want:
        shapes.append(shape("a_%dx1000_512x39" % n, n, 1000, bc.make_ubm(512, 39, 1), n // 5, 100, min(200, n), args.reps))
    out = {"device": _lib.device_name(), "shapes": shapes}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
