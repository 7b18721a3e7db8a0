"""Measurements of eliding fill-value chunks, on the GPU.

  python tools/bench_occupancy.py kernel [--size 1024] [--out FILE]
      The chunk-occupancy pass (occupancy.hip) over a size^3 float32 and a size^3 uint8 device
      array with cells of 32^3: an all-fill input (every byte is read) and a dense one (a wave
      stops loading where the cells are marked), alternated in one run with zarrs_info's range
      over the same array. Windows of at least --window seconds after a warm-up, medians of
      --rounds windows.
  python tools/bench_occupancy.py e2e [--size 1024] [--dir DIR] [--out FILE]
      `equal` store -> store over a size^3 uint8 volume of which about 90 % is the fill value,
      written with zstd level 1 and with bytes, and `reencode` of a dense volume with bytes;
      elision on and off alternated (off is what the store did before). Wall time, encode
      thread-seconds, device-to-host seconds and bytes written, from the call's own stats.
"""
import argparse
import json
import math
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from bench_ops import HBM_PEAK_GBS, timed  # noqa: E402


def bench_kernel(n, rounds, window_s):
    import torch
    import zarrs_tools_amd as zt
    ctx = zt.default_context(0)
    stream = torch.cuda.current_stream()
    cells = (32, 32, 32)
    res = {"op": "chunk occupancy (device-resident)",
           "config": {"shape": [n] * 3, "cells": list(cells), "rounds": rounds,
                      "window_s": window_s}, "ops": {}}
    for dt, esz in (("float32", 4), ("uint8", 1)):
        fill = torch.zeros((n, n, n), dtype=zt.torch_dtype(dt), device="cuda")
        if dt == "float32":
            dense = zt.synth_step_noise_f32((n, n, n)) + 1.0  # no element is 0.0
        else:
            dense = torch.ones((n, n, n), dtype=torch.uint8, device="cuda")
        rng_op = zt.Range()
        rstate = rng_op.new_state(fill.device, ctx)
        checks = {
            "fill": not bool(zt.chunk_occupancy(fill, cells, 0, ctx).any()),
            "dense": bool(zt.chunk_occupancy(dense, cells, 0, ctx).all()),
        }
        ops = {"range": lambda: rng_op.accumulate(fill, rstate, ctx),
               "fill": lambda: zt.chunk_occupancy(fill, cells, 0, ctx),
               "dense": lambda: zt.chunk_occupancy(dense, cells, 0, ctx)}
        reps = {}
        for k, fn in ops.items():
            r = 1
            while True:
                t = timed(fn, stream, r)
                if t * r >= window_s * 1e3:
                    break
                r = math.ceil(window_s * 1e3 / t * 1.05) + 1
            reps[k] = r
        ms = {k: [] for k in ops}
        for _ in range(rounds):
            for k, fn in ops.items():
                ms[k].append(timed(fn, stream, reps[k]))
        nbytes = n ** 3 * esz
        out = {}
        for k in ops:
            v = sorted(ms[k])
            med = v[len(v) // 2]
            out[k] = {"ms": round(med, 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                      "spread": round((v[-1] - v[0]) / med, 4), "calls_per_window": reps[k],
                      "array_bytes": nbytes, "GB/s_of_array": round(nbytes / (med / 1e3) / 1e9, 1),
                      "hbm_frac_of_array": round(nbytes / (med / 1e3) / 1e9 / HBM_PEAK_GBS, 4)}
            if k in checks:
                out[k]["exact"] = checks[k]
        for k in ops:
            out[k]["ratio_to_range"] = round(out[k]["ms"] / out["range"]["ms"], 4)
        res["ops"][dt] = out
        del fill, dense
        torch.cuda.empty_cache()
    return res


def bench_e2e(n, root, rounds):
    from zarrs_tools_amd import store as S
    chunk = (64, 64, 64)
    rng = np.random.default_rng(7)
    sparse, dense = os.path.join(root, "sparse"), os.path.join(root, "dense")
    S.create_array(sparse, "uint8", (n, n, n), chunk)
    S.create_array(dense, "uint8", (n, n, n), chunk)
    nz = max(chunk[0], n // 10 // chunk[0] * chunk[0])  # about 10 % of the planes hold data
    for z in range(0, n, chunk[0]):
        noise = rng.integers(0, 4, size=(chunk[0], n, n), dtype=np.uint8)
        S.write_array(dense, noise, (z, 0, 0))
        S.write_array(sparse, noise if z < nz else np.zeros_like(noise), (z, 0, 0))
    keys = ("wall_s", "encode_s", "d2h_s", "kernel_s", "decode_s", "bytes_written",
            "chunks_elided")
    cases = {
        "equal_90pct_fill_zstd1": (lambda d: S.equal(sparse, d, 1, encoding={
            "bytes_to_bytes_codecs": [{"name": "zstd", "configuration": {
                "level": 1, "checksum": False}}]})),
        "equal_90pct_fill_bytes": (lambda d: S.equal(sparse, d, 1)),
        "reencode_dense_bytes": (lambda d: S.reencode(dense, d)),
    }
    if not S.codec_available("zstd"):
        del cases["equal_90pct_fill_zstd1"]
    res = {"op": "store -> store with and without eliding fill-value chunks",
           "config": {"shape": [n] * 3, "chunk_shape": list(chunk), "data_planes": nz,
                      "rounds": rounds}, "cases": {}}
    for name, run in cases.items():
        runs = {"off": [], "on": []}
        dst = os.path.join(root, "out")
        for _ in range(rounds):
            for mode in ("off", "on"):
                shutil.rmtree(dst, ignore_errors=True)
                S.set_store_empty_chunks(mode == "off")
                st = run(dst)
                runs[mode].append({k: st[k] for k in keys})
        S.set_store_empty_chunks(True)
        med = {m: {k: sorted(r[k] for r in runs[m])[len(runs[m]) // 2] for k in keys}
               for m in runs}
        res["cases"][name] = {"runs": runs, "median": med,
                              "on_over_off_wall": round(med["on"]["wall_s"] / med["off"]["wall_s"], 4)}
        shutil.rmtree(dst, ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "e2e"])
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.what == "kernel":
        res = bench_kernel(a.size, a.rounds, a.window)
    else:
        root = tempfile.mkdtemp(prefix="zt_occ_", dir=a.dir)
        try:
            res = bench_e2e(a.size, root, min(a.rounds, 3))
        finally:
            shutil.rmtree(root, ignore_errors=True)
    text = json.dumps(res)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
