#!/usr/bin/env python3
"""What the x-vector forward pass costs on the device (csrc/xvector.hip), in one run; one JSON line on stdout.

    python scripts/time_xvector.py [--out profiles/r28_xvector.json] [--host-frames 300]

Network: input 30; frame layers 512 (-2..2), 512 (-2, 0, 2), 512 (-3, 0, 3), 512 (0), 1500 (0); pooling; affine 512; seeded random
weights scaled by 1 / sqrt(fan_in).  Shapes: 1000 utterances of 1000 frames, 64 of 300, one of 300, resident random features.
Per shape and per MFMA shape (the timing hook debug_xvector_mfma_shape: 0 = 32x32x16, 1 = 16x16x32):
  call_ms      host wall clock around XVector.extract of the resident batch as a user calls it (no events recorded), median of 5
               after a warm-up;
  convert_ms, layer_ms[l]   the call's own per-stage device times (HIP events around every launch), medians of 5 further calls made
               with times=True;
  per layer    FLOP = 2 rows K C_out on the unpadded widths, the achieved FLOP/s as a fraction of the dense bf16 spec peak
               (2.5 PFLOP/s) and of the LDS-fed matrix probe (csrc/probe.hip, mode 1, measured in this run); the bytes the layer moves
               (activations read once per offset and column tile as the kernel reads them, weights once per row tile, outputs
               written once) and its arithmetic intensity in FLOP per byte;
  host_numpy   the float64 restatement (tests/xvector_cases.py) of ONE utterance of --host-frames frames, extrapolated to the shape
               by frames (the stated subset: that one utterance);
  torch        the same network through torch.nn.functional.conv1d in bf16 on the same device, when torch imports there and sees
               the device: median of 5 after a warm-up, torch.cuda.synchronize around it.
No rate is fixed in advance: the JSON carries what was measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SPEC_PEAK = 2.5e15
SHAPES = ((1000, 1000), (64, 300), (1, 300))


def layer_costs(layers, n_utt, frames, plan):
    """per non-pooling layer: (rows, FLOP, bytes moved by the kernel as it reads)"""
    out, rows = [], frames
    TM, TN = plan["tile_rows"], plan["tile_cols"]
    pooled = False
    for l in layers:
        if l["kind"] == "stats_pool":
            out.append(None)
            pooled, rows = True, 1
            continue
        m = len(l["offsets"])
        c_out, K = l["W"].shape
        c_in = K // m
        if not pooled:
            rows -= l["offsets"][-1] - l["offsets"][0]
        n_rows = n_utt * rows
        col_tiles = -(-c_out // TN)
        row_tiles = n_utt * -(-rows // TM) if not pooled else -(-n_utt // TM)
        cp = -(-c_in // 32) * 32
        bytes_moved = n_rows * m * cp * 2 * col_tiles + row_tiles * col_tiles * TN * m * cp * 2 + n_rows * c_out * 2
        out.append((n_rows, 2.0 * n_rows * K * c_out, bytes_moved))
    return out


def torch_network(layers, device):
    import torch
    mods = []
    for l in layers:
        if l["kind"] == "stats_pool":
            mods.append(None)
            continue
        m = len(l["offsets"])
        c_out, K = l["W"].shape
        w = torch.tensor(l["W"].reshape(c_out, m, K // m).transpose(0, 2, 1).copy(), dtype=torch.bfloat16, device=device)
        off = l["offsets"]
        dil = off[1] - off[0] if m > 1 else 1
        assert all(off[j + 1] - off[j] == dil for j in range(m - 1))
        mods.append((w, torch.tensor(l["b"], dtype=torch.bfloat16, device=device), dil, l["act"] == "relu",
                     None if l["scale"] is None else torch.tensor(l["scale"], dtype=torch.bfloat16, device=device)[None, :, None],
                     None if l["shift"] is None else torch.tensor(l["shift"], dtype=torch.bfloat16, device=device)[None, :, None]))
    return mods


def torch_forward(mods, x):
    import torch
    import torch.nn.functional as F
    for mod in mods:
        if mod is None:
            x = torch.cat([x.float().mean(dim=2), x.float().std(dim=2, unbiased=False)], dim=1).to(torch.bfloat16)[:, :, None]
            continue
        w, b, dil, relu, sc, sh = mod
        x = F.conv1d(x, w, b, dilation=dil)
        if relu:
            x = F.relu(x)
        if sc is not None:
            x = x * sc + sh
    return x[:, :, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-frames", type=int, default=300)
    args = ap.parse_args()
    import xvector_cases as xc
    from speaker_recognition_amd import _lib
    from speaker_recognition_amd.core import Batch
    from speaker_recognition_amd.xvector import XVector

    layers = xc.standard_network()
    net = XVector(layers)
    rec = {"device": _lib.device_name(), "network": [list(x) for x in xc.STD_NETWORK] + ["stats_pool", xc.STD_EMBED],
           "spec_peak_flops": SPEC_PEAK}
    tf, mhz = _lib.mfma_streamed_probe(50.0)
    rec["lds_fed_probe_tflops"], rec["lds_fed_probe_mhz"] = tf, mhz
    rng = np.random.default_rng(28)

    # the host restatement of one utterance, once
    one = xc.features(rng, args.host_frames, 30)
    t0 = time.perf_counter()
    want = xc.network_forward(layers, one)
    host_s = time.perf_counter() - t0
    got = net.extract([one])[0]
    rec["host_numpy"] = {"frames": args.host_frames, "seconds": host_s,
                         "device_minus_restatement_max_abs": float(np.max(np.abs(got - want))), "embedding_max_abs": float(np.max(np.abs(want)))}

    torch_ok, torch_why = False, ""
    try:
        import torch
        torch_ok = torch.cuda.is_available()
        torch_why = "" if torch_ok else "torch sees no device"
    except Exception as e:      # noqa: BLE001
        torch_why = "torch does not import: %s" % e
    rec["torch_note"] = torch_why

    rec["shapes"] = []
    for n_utt, frames in SHAPES:
        X = rng.standard_normal((n_utt * frames, 30)).astype(np.float32)
        offsets = np.arange(n_utt + 1, dtype=np.int64) * frames
        batch = Batch.from_features(X, offsets)
        plan = net.plan([frames] * n_utt)
        costs = layer_costs(layers, n_utt, frames, plan)
        entry = {"utterances": n_utt, "frames": frames, "n_chunks": plan["n_chunks"], "buffer_bytes": list(plan["buffer_bytes"]),
                 "host_numpy_extrapolated_s": host_s * n_utt * frames / args.host_frames, "mfma": []}
        for shape, name in ((0, "32x32x16"), (1, "16x16x32")):
            _lib.set_option("debug_xvector_mfma_shape", shape)
            net.extract(batch)
            _lib.synchronize()
            calls, convs, lay = [], [], []
            for _ in range(5):                  # the call as a user makes it: no events recorded
                t0 = time.perf_counter()
                net.extract(batch)
                calls.append((time.perf_counter() - t0) * 1e3)
            for _ in range(5):                  # a pass of its own for the per-stage device times
                _, t = net.extract(batch, times=True)
                convs.append(t["convert"])
                lay.append(t["layers"])
            lay = np.median(np.asarray(lay), axis=0)
            per_layer = []
            for l, c in enumerate(costs):
                if c is None:
                    per_layer.append({"layer": l, "kind": "stats_pool", "device_ms": float(lay[l])})
                    continue
                rows, flop, nbytes = c
                rate = flop / (lay[l] * 1e-3) if lay[l] > 0 else 0.0
                per_layer.append({"layer": l, "kind": layers[l]["kind"], "rows": int(rows), "flop": flop, "device_ms": float(lay[l]),
                                  "flops": rate, "of_spec_peak": rate / SPEC_PEAK, "of_lds_fed_probe": rate / (tf * 1e12) if tf > 0 else None,
                                  "bytes_moved": int(nbytes), "flop_per_byte": flop / nbytes})
            frame_flop = sum(c[1] for c in costs[:net.pool_index])
            frame_ms = float(sum(lay[:net.pool_index]))
            entry["mfma"].append({"shape": name, "call_ms": float(np.median(calls)), "convert_ms": float(np.median(convs)),
                                  "device_ms_total": float(np.median(convs) + lay.sum()), "frame_layers_ms": frame_ms,
                                  "frame_layers_of_lds_fed_probe": frame_flop / (frame_ms * 1e-3) / (tf * 1e12) if frame_ms > 0 and tf > 0 else None,
                                  "frame_layers_of_spec_peak": frame_flop / (frame_ms * 1e-3) / SPEC_PEAK if frame_ms > 0 else None,
                                  "layers": per_layer})
        _lib.set_option("debug_xvector_mfma_shape", 0)
        try:
            if not torch_ok:
                raise RuntimeError(torch_why)
            import torch
            mods = torch_network(layers, "cuda")
            x = torch.tensor(X.reshape(n_utt, frames, 30).transpose(0, 2, 1).copy(), dtype=torch.bfloat16, device="cuda")
            with torch.no_grad():
                torch_forward(mods, x)
                torch.cuda.synchronize()
                ts = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    torch_forward(mods, x)
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
            entry["torch_conv1d_bf16_ms"] = float(np.median(ts))
            del x
        except Exception as e:      # noqa: BLE001  (recorded, not fatal: the library's own figures stand without it)
            entry["torch_conv1d_bf16_ms"] = None
            entry["torch_note"] = str(e)[:200]
        rec["shapes"].append(entry)
        del batch
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
