#!/usr/bin/env python3
"""Device-resident rates of the other rows on the path: the zarrs_ome mean
pyramid (config P per GPU: a 2048^3 uint16 octant, factor 2, 5 levels) and the Gaussian
(zarrs_filter gaussian 1.0,1.0,1.0 3,3,3 on 1024^3 f32, docs/zarrs_filter.md:107). One JSON line
per operation with its HBM roofline fraction and a CPU baseline (the oracle's C restatement,
one thread, on a bounded sample of the same workload).
`--only gradient`: the gradient magnitude (Sobel) on 1024^3 f32, alternated with the Gaussian at
kernel_half_size 1 on the same volume (its yardstick), windows of at least half a second.
`--only rank`: the rank filters (minimum, median, maximum) at kernel_half_size 1 on 1024^3 f32 and
u8, alternated with the same Gaussian yardstick; the median once more through the generic
bisection kernel.
`--only sat`: the summed-area table on 1024^3 float32 -> float32 and uint16 -> uint64, each
alternated with the reencode cast of the same type pair on the same volume (one read and one
write per voxel: the streaming yardstick).
`--only pointwise`: the per-element filters (reencode, crop, rescale, clamp, equal, replace_value)
on 1024^3, each single launch alternated with the reencode cast of the same type pair, and the
fused rescale -> clamp -> equal chain against its three single launches.
`--only info`: zarrs_info's range and histogram (info.hip) on 1024^3 uint8, uint16 and float32,
each alternated with the pointwise reencode of the same type on the same volume (the per-byte
yardstick); the histogram at 256 and 4096 bins and at 65 536 bins (above the LDS cap), on uniform
noise and on a volume that is 90 % one value.
`--only compare`: zarrs_validate's comparison (compare.hip) on two 1024^3 float32 arrays, equal,
1 % differing and all differing, alternated with the range over one float32 run of the same
bytes.
`--only arithmetic`: the two-array arithmetic filter (arithmetic.hip) on 1024^3: float32 - float32
-> float32, uint16 + uint16 -> uint16 and float32 * uint8 -> float32, alternated with Rescale on
float32 -> float32 (the per-byte yardstick).
`--only connected_components`: the labelling (connected.hip) of 1024^3 uint8 -> uint32 at
connectivity 1 and 3 on sparse noise, dense noise and a thresholded synth_u16 volume, alternated
with the Reencode uint8 -> uint32 cast of the same volume (the streaming floor); with scipy
installed, scipy.ndimage.label on the host as the CPU baseline (`--no-scipy` skips it);
`--cc-once` calls every labelling once and nothing else, for a kernel trace.
`--only label_statistics`: the per-label statistics and the label size filter (labels.hip) on
1024^3 uint32 labels (the labelling's three volumes at connectivity 1, the dense one at 3 as well),
alternated with Range on the same arrays.
`--only distance_transform`: the exact Euclidean distance transform (distance.hip) of 1024^3 uint8
-> float32 on noise of density 0.5 and 0.999 and on a solid ball, at spacing (1, 1, 1) and
(3, 1, 1), alternated with the Reencode uint8 -> float32 cast of the same volume (the streaming
floor); with scipy installed and a volume of at most 512^3, scipy.ndimage.distance_transform_edt
on the host as the CPU baseline (`--no-scipy` skips it); `--edt-once` calls every transform once
and nothing else, for a kernel trace.
`--only reconstruction`: morphological reconstruction (reconstruct.hip) on 1024^3: fill_holes at
connectivity 1 and 3 on the labelling's three uint8 volumes and h_maxima on the uint32 squared
distance map of one of them, alternated with the connected_components call on the same volume and
the Reencode uint8 -> uint32 cast; rounds, ms per call and ms per round against the streaming
floor of a round (two reads and one write per element); with scipy installed,
scipy.ndimage.binary_fill_holes on the host fills the same masks at `--rec-scipy-size`^3 (default
256; `--no-scipy` skips it); `--rec-once` calls every case once and nothing else.
`--only watershed`: the seeded watershed (watershed.hip) on 1024^3: the uint32 squared distance map
of the synth_u16 > q0.7 volume flooded from its maxima inside the foreground, seeded with its
labelled h-maxima, alternated with the Reconstruction h_maxima(1) call and the connected_components
call on the same volume; the three round counts, ms per call and the streaming floor of the phases
launched.

Algorithmic bytes: pyramid = level 0 read once + every level written once (2 B per u16
element; the fused launches never read an intermediate level back); Gaussian = 4 B read + 4 B written per voxel (the separable passes' intermediates are
not credited).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0


def timed(fn, stream, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def bench_pyramid(n, reps, levels, discrete=False, dtype="uint16"):
    import numpy as np
    import torch
    import zarrs_tools_amd as zt
    from oracle import oracle as O
    ctx = zt.default_context(0)
    x = zt.synth_u16((n, n, n))
    if dtype in ("uint8", "int8"):  # the low byte of the u16 noise: 256 values
        tt = torch.uint8 if dtype == "uint8" else torch.int8
        x = (x.view(torch.int16) & 0xFF).to(tt) if not discrete else \
            (x.view(torch.int16) & 0x7).to(tt)
    elif discrete:  # few distinct values, so the mode is not mostly a tie of eight
        x = (x.view(torch.int16) & 0x7).view(torch.uint16)
    esz = x.element_size()
    torch.cuda.synchronize()
    shapes = zt.pyramid_level_shapes((n, n, n), (2, 2, 2), levels)
    ms = timed(lambda: zt.pyramid(x, (2, 2, 2), levels, discrete=discrete, ctx=ctx),
               torch.cuda.current_stream(), reps)
    # parity (bit-exact): a 64^3 level-0 block aligned to 2^levels, its levels from the oracle
    lv = zt.pyramid(x, (2, 2, 2), levels, discrete=discrete, ctx=ctx)
    blk = x[:64, 64:128, 128:192].cpu().numpy()
    cur, exact = blk, True
    for k, t in enumerate(lv):
        cur = O.downsample(cur, dtype, (2, 2, 2), dtype, discrete=discrete)
        f = 2 ** (k + 1)
        got = t[:64 // f, 64 // f:128 // f, 128 // f:192 // f].cpu().numpy()
        exact = exact and np.array_equal(got, cur)
    del lv
    # compulsory bytes: level 0 read once + every level written once (fused launches never
    # read an intermediate level back); per_level: each level's input read + output written
    prev, nbytes, per_level = (n, n, n), esz * n ** 3, 0
    for s in shapes:
        per_level += esz * (int(np.prod(prev)) + int(np.prod(s)))
        nbytes += esz * int(np.prod(s))
        prev = s
    gbs = nbytes / (ms / 1e3) / 1e9
    # CPU: the oracle's level-1 downsample of a 256^3 sample (single thread)
    sample = O.synth_u16((256, 256, 256))
    if discrete:
        sample = (sample & 0x7).astype(np.dtype(dtype))
    elif dtype in ("uint8", "int8"):
        sample = (sample & 0xFF).astype(np.uint8).view(np.dtype(dtype))
    t0 = time.perf_counter()
    O.downsample(sample, dtype, (2, 2, 2), dtype, discrete=discrete)
    cpu_s = time.perf_counter() - t0
    return {"op": f"zarrs_ome {'mode (--discrete)' if discrete else 'mean'} pyramid "
                  "(device-resident)", "config":
            {"level0": [n] * 3, "dtype": dtype, "factor": [2, 2, 2], "levels": len(shapes)},
            "parity_bit_exact": bool(exact),
            "ms": round(ms, 4), "input_gvox_per_s": round(n ** 3 / (ms / 1e3) / 1e9, 3),
            "roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
                         "algorithmic_bytes": nbytes, "per_level_bytes": per_level},
            "cpu_baseline": {"input_gvox_per_s": round(256 ** 3 / cpu_s / 1e9, 4), "cores": 1,
                             "kind": "port", "sample": f"level 1 of a 256^3 {dtype} block, "
                             "oracle downsample (C restatement of downsample.rs:72-120)"}}


def bench_gaussian(n, reps):
    import torch
    import zarrs_tools_amd as zt
    from oracle import oracle as O
    ctx = zt.default_context(0)
    x = zt.synth_step_noise_f32((n, n, n))
    y = torch.empty_like(x)
    g = zt.Gaussian([1.0] * 3, [3] * 3)
    a_in, a_out = zt.DeviceArray(x, (256,) * 3), zt.DeviceArray(y, (256,) * 3)
    ms = timed(lambda: g.apply(a_in, a_out, ctx=ctx), torch.cuda.current_stream(), reps)
    gbs = n ** 3 * 8 / (ms / 1e3) / 1e9
    sample = O.synth_step_noise_f32((128, 128, 128))
    t0 = time.perf_counter()
    O.gaussian_apply_ndarray(sample, [1.0] * 3, [3] * 3)
    cpu_s = time.perf_counter() - t0
    return {"op": "gaussian sigma 1,1,1 half 3,3,3 (device-resident)",
            "config": {"shape": [n] * 3, "dtype": "float32", "chunk": [256] * 3},
            "ms": round(ms, 4), "gib_per_s": round(n ** 3 * 4 / 2 ** 30 / (ms / 1e3), 3),
            "roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
                         "algorithmic_bytes": n ** 3 * 8},
            "cpu_baseline": {"gib_per_s": round(128 ** 3 * 4 / 2 ** 30 / cpu_s, 4), "cores": 1,
                             "kind": "port", "sample": "128^3 f32 block, oracle Gaussian (C "
                             "restatement of gaussian.rs:110-119 / kernel.rs:17-73)"}}


def bench_gradient(n, rounds=5, window_s=0.5):
    """zarrs_filter gradient-magnitude (Sobel) on n^3 f32 -> f32 through GradientMagnitude.apply,
    alternated in one run with the Gaussian at sigma 1,1,1 / kernel_half_size 1,1,1 on the same
    volume (the same 3x3x3 footprint and algorithmic bytes: the yardstick). Each window is device
    events around enough calls for at least `window_s`, after a warm-up; `rounds` windows of each,
    alternating. Algorithmic bytes: 4 B read + 4 B written per voxel."""
    import math
    import numpy as np
    import torch
    import zarrs_tools_amd as zt
    from tests import gm_ref
    ctx = zt.default_context(0)
    x = zt.synth_step_noise_f32((n, n, n))
    y = torch.empty_like(x)
    chunk = (min(n, 256),) * 3
    a_in, a_out = zt.DeviceArray(x, chunk), zt.DeviceArray(y, chunk)
    gm = zt.GradientMagnitude("sobel")
    gs = zt.Gaussian([1.0] * 3, [1] * 3)
    stream = torch.cuda.current_stream()
    ops = {"gradient": lambda: gm.apply(a_in, a_out, ctx=ctx),
           "gaussian": lambda: gs.apply(a_in, a_out, ctx=ctx)}
    # parity (bit-exact) of the corner region whose inputs lie in the block copied back
    m = min(n - 1, 32)
    ops["gradient"]()
    torch.cuda.synchronize()
    ref = gm_ref.apply_ndarray(x[:m + 1, :m + 1, :m + 1].cpu().numpy())[:m, :m, :m]
    exact = bool(np.array_equal(y[:m, :m, :m].cpu().numpy(), ref))
    reps = {}
    for k, fn in ops.items():  # warm-up, then calls per window until a window lasts window_s
        r = 8
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

    def line(k):
        v = sorted(ms[k])
        med = v[len(v) // 2]
        gbs = n ** 3 * 8 / (med / 1e3) / 1e9
        return {"ms": round(med, 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                "spread": round((v[-1] - v[0]) / med, 4), "windows_ms": [round(t, 4) for t in ms[k]],
                "calls_per_window": reps[k],
                "gib_per_s": round(n ** 3 * 4 / 2 ** 30 / (med / 1e3), 3),
                "roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS,
                             "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
                             "algorithmic_bytes": n ** 3 * 8}}

    g, y_ = line("gradient"), line("gaussian")
    return {"op": "gradient_magnitude sobel (device-resident)",
            "config": {"shape": [n] * 3, "dtype": "float32", "chunk": list(chunk),
                       "rounds": rounds, "window_s": window_s},
            "parity_bit_exact": exact, **g,
            "yardstick": {"op": "gaussian sigma 1,1,1 half 1,1,1 (device-resident), same volume, "
                                "windows alternated with the gradient's", **y_},
            "ratio_to_yardstick": round(g["ms"] / y_["ms"], 4)}


def bench_rank(n, dtype, rounds=5, window_s=0.5):
    """The rank filters (minimum, median, maximum) at kernel_half_size 1,1,1 on n^3 `dtype`
    (float32 or uint8) through RankFilter.apply, alternated in one run with the Gaussian at sigma
    1,1,1 / kernel_half_size 1,1,1 on the same volume (the same 3x3x3 footprint and algorithmic
    bytes: the yardstick of the gradient magnitude). Windows as bench_gradient. The median is also
    timed once through the generic bisection kernel (the same volume as a 4-D array).
    Algorithmic bytes: one read and one write of every voxel."""
    import math
    import numpy as np
    import torch
    import zarrs_tools_amd as zt
    from tests import rank_ref
    ctx = zt.default_context(0)
    if dtype == "float32":
        x = zt.synth_step_noise_f32((n, n, n))
    else:  # the low byte of the u16 noise: 256 values
        x = (zt.synth_u16((n, n, n)).view(torch.int16) & 0xFF).to(torch.uint8)
    esz = x.element_size()
    y = torch.empty_like(x)
    chunk = (min(n, 256),) * 3
    a_in, a_out = zt.DeviceArray(x, chunk, dtype), zt.DeviceArray(y, chunk, dtype)
    gs = zt.Gaussian([1.0] * 3, [1] * 3)
    stream = torch.cuda.current_stream()
    filters = {k: zt.RankFilter(k, (1, 1, 1)) for k in ("minimum", "median", "maximum")}
    ops = {k: (lambda f=f: f.apply(a_in, a_out, ctx=ctx)) for k, f in filters.items()}
    ops["gaussian"] = lambda: gs.apply(a_in, a_out, ctx=ctx)
    # parity (bit-exact) of the corner region whose inputs lie in the block copied back
    m = min(n - 1, 32)
    blk = x[:m + 1, :m + 1, :m + 1].cpu().numpy()
    exact = {}
    for k in filters:
        ops[k]()
        torch.cuda.synchronize()
        ref = rank_ref.apply_ndarray(blk, k, (1, 1, 1), dtype)[:m, :m, :m]
        exact[k] = bool(np.array_equal(y[:m, :m, :m].cpu().numpy(), ref))
    reps = {}
    for k, fn in ops.items():  # warm-up, then calls per window until a window lasts window_s
        r = 8
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
    # the median once through the generic bisection kernel, and its parity with the fused one:
    # the same volume as a 4-D array with a unit first axis and half size 0 there has the same
    # windows, and only rank 3 takes the fused kernel
    ops["median"]()
    fused_out = y.clone()
    g_in = zt.DeviceArray(x.view(1, n, n, n), (1,) + chunk, dtype)
    g_out = zt.DeviceArray(y.view(1, n, n, n), (1,) + chunk, dtype)
    med4 = zt.RankFilter("median", (0, 1, 1, 1))
    generic_ms = timed(lambda: med4.apply(g_in, g_out, ctx=ctx), stream, 1)
    generic_same = bool(torch.equal(y, fused_out))
    del fused_out

    def line(k):
        v = sorted(ms[k])
        med = v[len(v) // 2]
        gbs = n ** 3 * 2 * esz / (med / 1e3) / 1e9
        return {"ms": round(med, 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                "spread": round((v[-1] - v[0]) / med, 4), "windows_ms": [round(t, 4) for t in ms[k]],
                "calls_per_window": reps[k],
                "gib_per_s": round(n ** 3 * esz / 2 ** 30 / (med / 1e3), 3),
                "roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS,
                             "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
                             "algorithmic_bytes": n ** 3 * 2 * esz}}

    y_ = line("gaussian")
    out = []
    for k in filters:
        r = line(k)
        res = {"op": f"{k} half 1,1,1 (device-resident, fused z-march)",
               "config": {"shape": [n] * 3, "dtype": dtype, "chunk": list(chunk),
                          "rounds": rounds, "window_s": window_s},
               "parity_bit_exact": exact[k], **r,
               "yardstick": {"op": "gaussian sigma 1,1,1 half 1,1,1 (device-resident), same "
                                   "volume, windows alternated with the filter's", **y_},
               "ratio_to_yardstick": round(r["ms"] / y_["ms"], 4)}
        if k == "median":
            res["generic_bisection"] = {"ms": round(generic_ms, 4), "calls": 1,
                                        "equals_fused": generic_same,
                                        "ratio_to_fused": round(generic_ms / r["ms"], 3)}
        out.append(res)
    return out


def bench_sat(n, din, dout, rounds=5, window_s=0.5):
    """zarrs_filter summed-area-table on n^3 din -> dout through SummedAreaTable.apply (ndim
    passes: the x scan reads din and writes dout, the others work on dout in place), alternated
    in one run with zt_reencode_cast of the same type pair on the same volume (one streaming
    pass, the yardstick). Windows as bench_gradient. Bytes per voxel: algorithmic = size(in) +
    size(out); actual = that + 2 * (ndim - 1) * size(out) for the in-place passes. The time per
    pass is the total over ndim; the split by kernel comes from a kernel trace of this run."""
    import math
    import numpy as np
    import torch
    import zarrs_tools_amd as zt
    from zarrs_tools_amd import _abi
    from zarrs_tools_amd.filter import DTYPES, _ptr
    from tests import sat_ref
    from tests.gpu_util import from_dev
    ctx = zt.default_context(0)
    if din == "float32":
        x = zt.synth_step_noise_f32((n, n, n))
    else:
        x = zt.synth_u16((n, n, n))
    y = torch.empty((n, n, n), dtype=zt.torch_dtype(dout), device=x.device)
    chunk = (min(n, 256),) * 3
    a_in, a_out = zt.DeviceArray(x, chunk, din), zt.DeviceArray(y, chunk, dout)
    f = zt.SummedAreaTable()
    stream = torch.cuda.current_stream()

    def cast():
        _abi.check(_abi.lib().zt_reencode_cast(ctx.handle, DTYPES[din], _ptr(x), DTYPES[dout],
                                               _ptr(y), n ** 3))

    ops = {"sat": lambda: f.apply(a_in, a_out, ctx=ctx), "cast": cast}
    # parity (bit-exact): the corner block, whose sums need no element outside it
    m = min(n, 48)
    ops["sat"]()
    torch.cuda.synchronize()
    ref = sat_ref.sat(from_dev(x[:m, :m, :m], din), din, dout)
    got = from_dev(y[:m, :m, :m], dout)
    exact = bool(np.array_equal(got.view(np.uint8), ref.view(np.uint8)))
    reps = {}
    for k, fn in ops.items():  # warm-up, then calls per window until a window lasts window_s
        r = 8
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
    si, so, nd = x.element_size(), y.element_size(), 3
    alg = n ** 3 * (si + so)
    act = alg + n ** 3 * 2 * (nd - 1) * so

    def line(k, nbytes_alg, nbytes_act):
        v = sorted(ms[k])
        med = v[len(v) // 2]
        g_alg, g_act = nbytes_alg / (med / 1e3) / 1e9, nbytes_act / (med / 1e3) / 1e9
        return {"ms": round(med, 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                "spread": round((v[-1] - v[0]) / med, 4), "windows_ms": [round(t, 4) for t in ms[k]],
                "calls_per_window": reps[k],
                "roofline": {"bound": "hbm", "achieved": round(g_alg, 1), "peak": HBM_PEAK_GBS,
                             "unit": "GB/s", "frac": round(g_alg / HBM_PEAK_GBS, 4),
                             "algorithmic_bytes": nbytes_alg},
                "roofline_pass_bytes": {"achieved": round(g_act, 1),
                                        "frac": round(g_act / HBM_PEAK_GBS, 4),
                                        "bytes": nbytes_act}}

    s, y_ = line("sat", alg, act), line("cast", alg, alg)
    return {"op": f"summed_area_table {din} -> {dout} (device-resident)",
            "config": {"shape": [n] * 3, "dtype_in": din, "dtype_out": dout, "chunk": list(chunk),
                       "rounds": rounds, "window_s": window_s, "passes": nd},
            "parity_bit_exact": exact, **s, "ms_per_pass": round(s["ms"] / nd, 4),
            "yardstick": {"op": f"reencode cast {din} -> {dout} (device-resident), same volume, "
                                "windows alternated with the table's", **y_},
            "ratio_to_yardstick": round(s["ms"] / y_["ms"], 4),
            "ratio_to_yardstick_per_pass_byte": round((s["ms"] / act) / (y_["ms"] / alg), 4)}


def bench_pointwise(n, rounds=5, window_s=0.25):
    """The per-element filters on n^3, device-resident, one launch each (pointwise.hip): every
    single op on uint16 -> uint16, float32 -> float32 and uint16 -> uint8 (equal: uint8 -> bool),
    alternated in one run with zt_reencode_cast of the same type pair on the same volume (the
    scalar cast kernel, the yardstick); then the documented chain rescale(0.01275, 0) -> uint8,
    clamp(2, 5), equal(5) -> bool as one fused launch against its three single launches,
    alternated. Windows as bench_gradient. Bytes per element: size(in) + size(out) of the
    launch. One JSON line per group; a sampled block of every result is checked against the
    restatement (tests/pw_ref.py)."""
    import math
    import numpy as np
    import torch
    import zarrs_tools_amd as zt
    from zarrs_tools_amd import _abi
    from zarrs_tools_amd.filter import DTYPES, _ptr
    from tests import pw_ref as R
    from tests.gpu_util import from_dev
    ctx = zt.default_context(0)
    stream = torch.cuda.current_stream()
    u16 = zt.synth_u16((n, n, n))
    f32 = zt.synth_step_noise_f32((n, n, n))
    u8 = zt.PointwiseProgram([zt.Rescale(0.01275, 0.0)], "uint16", ["uint8"],
                             u16.shape).apply_ndarray(u16, ctx)
    src = {"uint16": u16, "float32": f32, "uint8": u8}
    m = 4096  # the sampled check: the first m elements (a crop: its first row's first m)

    def measure(ops):
        reps = {}
        for k, fn in ops.items():  # warm-up, then calls per window until it lasts window_s
            r = 4
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
        return ms, reps

    def line(v, r, nbytes):
        v = sorted(v)
        med = v[len(v) // 2]
        gbs = nbytes / (med / 1e3) / 1e9
        return {"ms": round(med, 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                "spread": round((v[-1] - v[0]) / med, 4), "calls_per_window": r,
                "bytes": nbytes, "GB/s": round(gbs, 1),
                "hbm_frac": round(gbs / HBM_PEAK_GBS, 4)}

    def single(din, dout, name, filt, ref_kw):
        x = src[din]
        prog = zt.PointwiseProgram([filt], din, [dout], x.shape)
        y = torch.empty(tuple(prog.shape), dtype=zt.torch_dtype(dout), device=x.device)
        prog.run(x, y, ctx)
        torch.cuda.synchronize()
        if name == "crop":
            o = prog.offset
            xs = from_dev(x[o[0], o[1], o[2]:o[2] + min(m, prog.shape[2])], din)
            ref = R.reencode(xs, din, dout)
        else:
            ref = R.program(from_dev(x.reshape(-1)[:m], din), din, [(name, dout, ref_kw)])
        got = from_dev(y.reshape(-1)[:ref.size], dout)
        ok = bool(np.array_equal(got.view(np.uint8), ref.view(np.uint8)))
        nbytes = int(y.numel()) * (x.element_size() + y.element_size())
        return (lambda: prog.run(x, y, ctx)), ok, nbytes, y

    out = []
    groups = [("uint16", "uint16", 5), ("float32", "float32", 5.0), ("uint16", "uint8", 5),
              ("uint8", "bool", 5)]
    for din, dout, five in groups:
        x = src[din]
        cases = {"equal": (zt.Equal(five), dict(value=five))} if dout == "bool" else {
            "reencode": (zt.Reencode(), {}),
            "crop": (zt.Crop((8, 8, 8), (n - 16,) * 3), {}),
            "rescale": (zt.Rescale(0.01275, 0.5), dict(multiply=0.01275, add=0.5)),
            "clamp": (zt.Clamp(2, 500), dict(lo=2.0, hi=500.0)),
            "replace_value": (zt.ReplaceValue(five, 0), dict(value=five, replace=0))}
        ops, meta, keep = {}, {}, []
        for name, (filt, kw) in cases.items():
            fn, ok, nbytes, y = single(din, dout, name, filt, kw)
            ops[name], meta[name] = fn, (ok, nbytes)
            keep.append(y)
        yc = torch.empty(tuple(x.shape), dtype=zt.torch_dtype(dout), device=x.device)

        def cast(x=x, yc=yc, din=din, dout=dout):
            _abi.check(_abi.lib().zt_reencode_cast(ctx.handle, DTYPES[din], _ptr(x),
                                                   DTYPES[dout], _ptr(yc), n ** 3))

        ops["cast"] = cast
        ms, reps = measure(ops)
        cast_bytes = n ** 3 * (x.element_size() + yc.element_size())
        yard = line(ms["cast"], reps["cast"], cast_bytes)
        res = {"op": f"pointwise {din} -> {dout} (device-resident), single launches",
               "config": {"shape": [n] * 3, "rounds": rounds, "window_s": window_s},
               "yardstick": {"op": f"reencode cast {din} -> {dout} (zt_reencode_cast), same "
                                   "volume, windows alternated", **yard}, "ops": {}}
        for name in cases:
            ln = line(ms[name], reps[name], meta[name][1])
            ln["parity_bit_exact_sample"] = meta[name][0]
            ln["ratio_to_cast_per_byte"] = round((ln["ms"] / ln["bytes"]) /
                                                 (yard["ms"] / yard["bytes"]), 4)
            res["ops"][name] = ln
        out.append(res)
        del keep, yc
        torch.cuda.empty_cache()
    # the fused chain against its three single launches
    fs = [zt.Rescale(0.01275, 0.0), zt.Clamp(2, 5), zt.Equal(5)]
    ts = ["uint8", "uint8", "bool"]
    a = torch.empty((n, n, n), dtype=torch.uint8, device=u16.device)
    b = torch.empty_like(a)
    c = torch.empty_like(a)
    d = torch.empty_like(a)
    p1 = zt.PointwiseProgram(fs[:1], "uint16", ts[:1], u16.shape)
    p2 = zt.PointwiseProgram(fs[1:2], "uint8", ts[1:2], u16.shape)
    p3 = zt.PointwiseProgram(fs[2:], "uint8", ts[2:], u16.shape)
    pf = zt.PointwiseProgram(fs, "uint16", ts, u16.shape)
    ops = {"fused": lambda: pf.run(u16, d, ctx), "rescale": lambda: p1.run(u16, a, ctx),
           "clamp": lambda: p2.run(a, b, ctx), "equal": lambda: p3.run(b, c, ctx)}
    for fn in ops.values():
        fn()
    torch.cuda.synchronize()
    ref = R.program(from_dev(u16.reshape(-1)[:m], "uint16"), "uint16", [
        ("rescale", "uint8", dict(multiply=0.01275, add=0.0)),
        ("clamp", "uint8", dict(lo=2.0, hi=5.0)), ("equal", "bool", dict(value=5))])
    ok = bool(np.array_equal(from_dev(d.reshape(-1)[:m], "uint8"), ref) and
              torch.equal(c, d))
    ms, reps = measure(ops)
    nb = {"fused": 3, "rescale": 3, "clamp": 2, "equal": 2}
    lines = {k: line(ms[k], reps[k], n ** 3 * nb[k]) for k in ops}
    sum_ms = sum(lines[k]["ms"] for k in ("rescale", "clamp", "equal"))
    out.append({"op": "pointwise chain rescale -> uint8, clamp, equal -> bool on uint16 "
                      "(device-resident): one fused launch against three",
                "config": {"shape": [n] * 3, "rounds": rounds, "window_s": window_s},
                "parity_bit_exact_sample": ok, "fused_equals_unfused": bool(torch.equal(c, d)),
                "launches": lines, "unfused_sum_ms": round(sum_ms, 4),
                "fused_over_unfused": round(lines["fused"]["ms"] / sum_ms, 4),
                "fused_is_faster": bool(lines["fused"]["ms"] < sum_ms)})
    return out


def bench_info(n, rounds=3, window_s=0.25):
    """zarrs_info's reductions on n^3, device-resident (info.hip): per input type the range, the
    histogram at 256 bins (LDS bins, 16 replicas, plain adds), 4096 bins (LDS bins, one replica,
    leader rounds) and 65 536 bins (global bins, leader rounds), each histogram on uniform
    noise and on a copy of it in which 90 % of the elements, scattered, hold one value, alternated
    in one run with the pointwise reencode of the same type on the same volume (one read and one
    write per element: the per-byte yardstick). Windows of at least window_s after a warm-up.
    Bytes: the elements read. One JSON line per type; every result is checked (sum(hist) == n^3;
    a sampled block against tests/info_ref.py)."""
    import math
    import numpy as np
    import torch
    import zarrs_tools_amd as zt
    from tests import info_ref as R
    from tests.gpu_util import from_dev
    ctx = zt.default_context(0)
    stream = torch.cuda.current_stream()
    total = n ** 3
    m = 1 << 16  # the sampled check: the first m elements

    def measure(ops):
        reps = {}
        for k, fn in ops.items():  # warm-up, then calls per window until it lasts window_s
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
        return ms, reps

    def line(v, r, nbytes):
        v = sorted(v)
        med = v[len(v) // 2]
        gbs = nbytes / (med / 1e3) / 1e9
        return {"ms": round(med, 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                "spread": round((v[-1] - v[0]) / med, 4), "calls_per_window": r,
                "bytes_read": nbytes, "GB/s": round(gbs, 1),
                "hbm_frac": round(gbs / HBM_PEAK_GBS, 4)}

    out = []
    for dt in ("uint8", "uint16", "float32"):
        if dt == "float32":
            x, mn, mx, const = zt.synth_step_noise_f32((n, n, n)), 0.0, 600.0, 40.0
        else:
            u16 = zt.synth_u16((n, n, n))
            x, mn, mx, const = u16, 0.0, 65535.0, 40
            if dt == "uint8":
                x = zt.Rescale(255.0 / 65535.0, 0.0).apply_ndarray(u16, dtype_out="uint8")
                mx = 255.0
                del u16
        x90 = x.clone().reshape(-1)
        for i in range(0, total, 1 << 28):  # 90 % of the elements, scattered, hold `const`
            part = x90[i:i + (1 << 28)]
            if dt == "uint16":  # (masked assignment through the signed view of the same bits)
                part = part.view(torch.int16)
            part[torch.rand(part.numel(), device=x.device) < 0.9] = const
        x90 = x90.reshape(x.shape)
        torch.cuda.empty_cache()
        y = torch.empty_like(x)
        prog = zt.PointwiseProgram([zt.Reencode()], dt, [dt], x.shape)
        rng_op = zt.Range()
        rstate = rng_op.new_state(x.device, ctx)
        hists = {nb: zt.Histogram(nb, mn, mx) for nb in (256, 4096, 65536)}
        hstate = {nb: h.new_state(x.device) for nb, h in hists.items()}
        ops = {"reencode": lambda: prog.run(x, y, ctx),
               "range": lambda: rng_op.accumulate(x, rstate, ctx)}
        for nb, h in hists.items():
            for name, src in (("noise", x), ("90pct", x90)):
                ops[f"histogram_{nb}_{name}"] = (
                    lambda h=h, src=src, nb=nb: h.accumulate(src, hstate[nb], ctx))
        # checks: whole-volume counts, and a sampled block against the restatement
        checks = {}
        for nb, h in hists.items():
            for name, src in (("noise", x), ("90pct", x90)):
                _, hist = h.apply_ndarray(src, ctx)
                _, part = h.apply_ndarray(src.reshape(-1)[:m], ctx)
                ref = R.histogram(from_dev(src.reshape(-1)[:m], dt), dt, nb, mn, mx)[1]
                checks[f"histogram_{nb}_{name}"] = bool(int(hist.sum()) == total and
                                                        np.array_equal(part, ref))
        got = rng_op.apply_ndarray(x.reshape(-1)[:m], ctx)
        checks["range"] = bool(got == R.range_(from_dev(x.reshape(-1)[:m], dt), dt))
        ms, reps = measure(ops)
        nbytes = total * x.element_size()
        yard = line(ms["reencode"], reps["reencode"], nbytes)
        yard["bytes_written"] = nbytes
        res = {"op": f"zarrs_info range / histogram on {dt} (device-resident)",
               "config": {"shape": [n] * 3, "rounds": rounds, "window_s": window_s,
                          "histogram_min_max": [mn, mx]},
               "range_whole_volume": list(rng_op.apply_ndarray(x, ctx)),
               "yardstick": {"op": f"pointwise reencode {dt} -> {dt}, same volume, windows "
                                   "alternated (reads and writes every element)", **yard},
               "ops": {}}
        for k in ops:
            if k == "reencode":
                continue
            ln = line(ms[k], reps[k], nbytes)
            ln["exact"] = checks[k]
            ln["ratio_to_reencode_per_byte_read"] = round(ln["ms"] / yard["ms"], 4)
            res["ops"][k] = ln
        for nb in hists:
            a, b = res["ops"][f"histogram_{nb}_noise"], res["ops"][f"histogram_{nb}_90pct"]
            b["ratio_to_noise"] = round(b["ms"] / a["ms"], 4)
        out.append(res)
        del x, x90, y, hstate
        torch.cuda.empty_cache()
    return out


def bench_compare(n, rounds=5, window_s=0.4):
    """zarrs_validate's comparison on two n^3 float32 device arrays (compare.hip): an equal pair
    (the ballot fast path), a pair in which 1 % of the elements, scattered, differ and a pair in
    which every element differs (no fast path), alternated in one run with the range over one
    float32 run of 2 n^3 elements. The equal pair is the two halves of that run, so both read the
    same bytes; `compare_equal_apart` is the first half against a copy allocated on its own (the
    halves lie exactly 4 n^3 bytes apart, a power of two at n = 1024). Windows of at least window_s after a warm-up, `rounds` of each, medians. Bytes:
    the elements read (both arrays). Every result is checked exactly."""
    import math
    import torch
    import zarrs_tools_amd as zt
    ctx = zt.default_context(0)
    stream = torch.cuda.current_stream()
    total = n ** 3
    big = torch.empty(2 * total, dtype=torch.float32, device="cuda")
    big[:total] = zt.synth_step_noise_f32((n, n, n)).reshape(-1)
    big[total:] = big[:total]
    a, b = big[:total], big[total:]
    b_apart, b1, b_all = a.clone(), a.clone(), a.clone()
    n1, first1 = 0, None
    for i in range(0, total, 1 << 28):  # 1 % of the elements, scattered: the lowest bit flipped
        part = b1[i:i + (1 << 28)].view(torch.int32)
        mask = torch.rand(part.numel(), device=part.device) < 0.01
        part[mask] ^= 1
        n1 += int(mask.sum())
        if first1 is None and bool(mask.any()):
            first1 = i + int(torch.nonzero(mask)[0])
        b_all[i:i + (1 << 28)].view(torch.int32).bitwise_xor_(1)
        del mask
    torch.cuda.empty_cache()
    cmp_op, rng_op = zt.Compare(), zt.Range()
    cstate, rstate = cmp_op.new_state(a.device, ctx), rng_op.new_state(a.device, ctx)
    checks = {"compare_equal": cmp_op.apply_ndarray(a, b, ctx) == (0, None),
              "compare_equal_apart": cmp_op.apply_ndarray(a, b_apart, ctx) == (0, None),
              "compare_1pct": cmp_op.apply_ndarray(a, b1, ctx) == (n1, first1),
              "compare_all": cmp_op.apply_ndarray(a, b_all, ctx) == (total, 0)}
    ops = {"range": lambda: rng_op.accumulate(big, rstate, ctx),
           "compare_equal": lambda: cmp_op.accumulate(a, b, cstate, 0, ctx),
           "compare_equal_apart": lambda: cmp_op.accumulate(a, b_apart, cstate, 0, ctx),
           "compare_1pct": lambda: cmp_op.accumulate(a, b1, cstate, 0, ctx),
           "compare_all": lambda: cmp_op.accumulate(a, b_all, cstate, 0, ctx)}
    reps = {}
    for k, fn in ops.items():  # warm-up, then calls per window until it lasts window_s
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
    nbytes = 2 * total * 4
    res = {"op": "zarrs_validate compare on two float32 arrays (device-resident)",
           "config": {"shape": [n] * 3, "rounds": rounds, "window_s": window_s,
                      "differing_1pct": n1,
                      "address_distance": {"compare_equal": b.data_ptr() - a.data_ptr(),
                                           "compare_equal_apart": b_apart.data_ptr() - a.data_ptr(),
                                           "compare_1pct": b1.data_ptr() - a.data_ptr(),
                                           "compare_all": b_all.data_ptr() - a.data_ptr()}},
           "ops": {}}
    for k in ops:
        v = sorted(ms[k])
        med = v[len(v) // 2]
        gbs = nbytes / (med / 1e3) / 1e9
        res["ops"][k] = {"ms": round(med, 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                         "spread": round((v[-1] - v[0]) / med, 4), "calls_per_window": reps[k],
                         "bytes_read": nbytes, "GB/s": round(gbs, 1),
                         "GiB/s": round(nbytes / (med / 1e3) / 2 ** 30, 1),
                         "hbm_frac": round(gbs / HBM_PEAK_GBS, 4)}
        if k != "range":
            res["ops"][k]["exact"] = bool(checks[k])
    for k in ops:
        res["ops"][k]["ratio_to_range"] = round(res["ops"][k]["ms"] / res["ops"]["range"]["ms"], 4)
    return res


def bench_arithmetic(n, rounds=5, window_s=0.5):
    """The two-array arithmetic filter on n^3 device arrays (arithmetic.hip): float32 - float32 ->
    float32 (12 B per voxel), uint16 + uint16 -> uint16 (6 B) and float32 * uint8 -> float32
    (9 B), alternated in one run with Rescale on n^3 float32 -> float32 (8 B per voxel, the
    streaming yardstick). Windows of at least window_s after a warm-up, `rounds` of each, medians.
    Bytes: every element of the three streams once. The f32 result is checked against torch."""
    import math
    import torch
    import zarrs_tools_amd as zt
    ctx = zt.default_context(0)
    stream = torch.cuda.current_stream()
    shape, total = (n, n, n), n ** 3
    a = zt.synth_step_noise_f32(shape)
    b = a.flip(0).contiguous()
    out = torch.empty_like(a)
    ua, ub = zt.synth_u16(shape), zt.synth_u16(shape, seed=7)
    m8 = ub.view(torch.uint8)[..., ::2].contiguous()  # the low byte of every element
    # Arrays allocated one after the other lie a power of two apart at n = 1024 (2^32 bytes for
    # float32), where a lane's accesses to the streams fall on the same place in the address
    # interleave (profiles/compare.txt). The `_apart` ops use operands carved out of one pool at
    # distances that are no power of two: 2 MiB more between each pair.
    pad, at = 2 << 20, 0
    pool = torch.empty(14 * total + 8 * pad, dtype=torch.uint8, device="cuda")

    def carve(dtype, esz):
        nonlocal at
        at += pad
        t = pool[at:at + total * esz].view(dtype).reshape(shape)
        at += total * esz
        return t

    b_ap, out_ap = carve(torch.float32, 4), carve(torch.float32, 4)
    ub_ap, uout_ap, m8_ap = carve(torch.uint16, 2), carve(torch.uint16, 2), carve(torch.uint8, 1)
    b_ap.copy_(b)
    ub_ap.copy_(ub)
    m8_ap.copy_(m8)
    uout = torch.empty_like(ua)
    resc = zt.PointwiseProgram([zt.Rescale(0.5, 1.0)], "float32", ["float32"], shape)
    sub, add, mul = zt.Arithmetic("subtract"), zt.Arithmetic("add"), zt.Arithmetic("multiply")
    exact = True
    for o, bb in ((out, b), (out_ap, b_ap)):
        sub.apply_ndarray(a, bb, out=o, ctx=ctx)
        exact = exact and bool(torch.equal(o, a - b))
    mul.apply_ndarray(a, m8_ap, out=out_ap, ctx=ctx)
    exact = exact and bool(torch.equal(out_ap, a * m8.to(torch.float32)))
    ops = {"rescale_f32": (lambda: resc.run(a, out, ctx), 8, (a, out)),
           "rescale_f32_apart": (lambda: resc.run(a, out_ap, ctx), 8, (a, out_ap)),
           "subtract_f32_f32_f32": (lambda: sub.apply_ndarray(a, b, out=out, ctx=ctx), 12,
                                    (a, b, out)),
           "subtract_f32_f32_f32_apart": (lambda: sub.apply_ndarray(a, b_ap, out=out_ap, ctx=ctx),
                                          12, (a, b_ap, out_ap)),
           "add_u16_u16_u16": (lambda: add.apply_ndarray(ua, ub, out=uout, ctx=ctx), 6,
                               (ua, ub, uout)),
           "add_u16_u16_u16_apart": (lambda: add.apply_ndarray(ua, ub_ap, out=uout_ap, ctx=ctx),
                                     6, (ua, ub_ap, uout_ap)),
           "multiply_f32_u8_f32_apart": (lambda: mul.apply_ndarray(a, m8_ap, out=out_ap, ctx=ctx),
                                         9, (a, m8_ap, out_ap))}
    reps = {}
    for k, (fn, _, _) in ops.items():  # warm-up, then calls per window until it lasts window_s
        r = 1
        while True:
            t = timed(fn, stream, r)
            if t * r >= window_s * 1e3:
                break
            r = math.ceil(window_s * 1e3 / t * 1.05) + 1
        reps[k] = r
    ms = {k: [] for k in ops}
    for _ in range(rounds):
        for k, (fn, _, _) in ops.items():
            ms[k].append(timed(fn, stream, reps[k]))
    res = {"op": "arithmetic on two arrays (device-resident)",
           "config": {"shape": [n] * 3, "rounds": rounds, "window_s": window_s},
           "exact": exact, "ops": {}}
    for k, (_, per, arrays) in ops.items():
        v = sorted(ms[k])
        med = v[len(v) // 2]
        nbytes = total * per
        gbs = nbytes / (med / 1e3) / 1e9
        res["ops"][k] = {"ms": round(med, 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                         "spread": round((v[-1] - v[0]) / med, 4), "calls_per_window": reps[k],
                         "bytes_per_voxel": per, "GB/s": round(gbs, 1),
                         "GiB/s": round(nbytes / (med / 1e3) / 2 ** 30, 1),
                         "hbm_frac": round(gbs / HBM_PEAK_GBS, 4),
                         "ns_per_KiB": round(med * 1e6 / (nbytes / 1024), 5),
                         "address_distance": [t.data_ptr() - arrays[0].data_ptr()
                                              for t in arrays[1:]]}
    for k in ops:  # each against the yardstick placed the same way
        y = res["ops"]["rescale_f32_apart" if k.endswith("_apart") else "rescale_f32"]
        res["ops"][k]["per_byte_ratio_to_rescale"] = round(
            res["ops"][k]["ns_per_KiB"] / y["ns_per_KiB"], 4)
    return res


def bench_connected_components(n, rounds=5, window_s=0.5, scipy_baseline=True, once=False):
    """Connected-component labelling on n^3 uint8 device arrays -> uint32 (connected.hip) at
    connectivity 1 and 3, on sparse noise (density 0.05), dense noise (0.6: one giant component at
    connectivity 1) and a thresholded synth_u16 volume (blobs), through ConnectedComponents.apply,
    alternated in one run with the Reencode uint8 -> uint32 cast of the same volume (one byte read
    and four written per element: the streaming floor, the yardstick). Windows of at least
    window_s after a warm-up, `rounds` of each, medians. Every call synchronises the stream once
    (the host reads K before the labels are written); that wait is inside the windows. With scipy
    installed, scipy.ndimage.label on the host labels the same volumes (the CPU baseline) and its
    labels and K are compared with the device's. once=True: every labelling called once, in the
    order volume by volume, connectivity 1 then 3, and nothing else (for a kernel trace)."""
    import math
    import numpy as np
    import torch
    import zarrs_tools_amd as zt
    ctx = zt.default_context(0)
    stream = torch.cuda.current_stream()
    shape, total = (n, n, n), n ** 3
    gen = torch.Generator(device="cuda").manual_seed(2025)
    noise = torch.rand(shape, device="cuda", generator=gen)
    u16 = zt.synth_u16(shape)
    sample = u16.reshape(-1)[:: max(1, total // (1 << 20))].to(torch.float32)
    level = float(torch.quantile(sample, 0.7))
    volumes = {"sparse_0.05": (noise < 0.05).to(torch.uint8),
               "dense_0.6": (noise < 0.6).to(torch.uint8),
               "blobs": (u16.to(torch.float32) > level).to(torch.uint8)}
    del noise, u16, sample
    out = torch.empty(shape, dtype=torch.uint32, device="cuda")
    cast = zt.PointwiseProgram([zt.Reencode()], "uint8", ["uint32"], shape)
    filters = {1: zt.ConnectedComponents(1), 3: zt.ConnectedComponents(3)}
    chunk = (32, 32, 32)

    def label(v, c):
        return filters[c].apply(zt.DeviceArray(v, chunk, "uint8"),
                                zt.DeviceArray(out, chunk, "uint32"), ctx=ctx)

    if once:
        return {"op": "connected_components, one call each",
                "components": {f"{name}_c{c}": label(v, c)
                               for name, v in volumes.items() for c in (1, 3)}}
    ops, counts = {}, {}
    for name, v in volumes.items():
        ops[f"{name}_cast_u8_u32"] = (lambda v=v: cast.run(v, out, ctx))
        for c in (1, 3):
            counts[f"{name}_c{c}"] = label(v, c)
            ops[f"{name}_c{c}"] = (lambda v=v, c=c: label(v, c))
    reps = {}
    for k, fn in ops.items():  # warm-up, then calls per window until it lasts window_s
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
    res = {"op": "connected_components uint8 -> uint32 (device-resident)",
           "config": {"shape": [n] * 3, "rounds": rounds, "window_s": window_s},
           "foreground": {k: round(float(v.to(torch.float32).mean()), 4)
                          for k, v in volumes.items()},
           "ops": {}}
    for k in ops:
        v = sorted(ms[k])
        med = v[len(v) // 2]
        res["ops"][k] = {"ms": round(med, 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                         "spread": round((v[-1] - v[0]) / med, 4), "calls_per_window": reps[k],
                         "ns_per_voxel": round(med * 1e6 / total, 5)}
        if k in counts:
            res["ops"][k]["components"] = counts[k]
            y = res["ops"][k.rsplit("_c", 1)[0] + "_cast_u8_u32"]
            res["ops"][k]["ratio_to_cast"] = round(med / y["ms"], 3)
        else:
            gbs = total * 5 / (med / 1e3) / 1e9
            res["ops"][k].update({"GB/s": round(gbs, 1), "hbm_frac": round(gbs / HBM_PEAK_GBS, 4)})
    if scipy_baseline:
        try:
            from scipy import ndimage
        except ImportError:
            ndimage = None
        if ndimage is not None:
            for name, v in volumes.items():
                host = v.cpu().numpy()
                for c in (1, 3):
                    t0 = time.perf_counter()
                    want, k_want = ndimage.label(host, ndimage.generate_binary_structure(3, c))
                    dt = time.perf_counter() - t0
                    label(v, c)
                    got = out.cpu().numpy()
                    o = res["ops"][f"{name}_c{c}"]
                    o["scipy_s"] = round(dt, 3)
                    o["scipy_over_gpu"] = round(dt * 1e3 / o["ms"], 1)
                    o["equals_scipy"] = bool(k_want == counts[f"{name}_c{c}"] and
                                             np.array_equal(got, want.astype(np.uint32)))
    return res


def bench_label_statistics(n, rounds=5, window_s=0.5):
    """Per-label statistics and the label size filter (labels.hip) on n^3 uint32 label arrays: the
    three volumes of bench_connected_components labelled at connectivity 1 (K in the tens of
    millions, mostly specks, and a few million blobs) and the dense one at connectivity 3 as well
    (K = 1: every run lands on one label, the contention extreme). Per volume, alternated in one
    run: Range on the label array (the yardstick: it reads the same bytes), the statistics'
    device work (state init + accumulate with n_labels given) without and with a uint16
    intensity array, and LabelSizeFilter (min_size 2) into uint32, which synchronises twice.
    Windows of at least window_s after a warm-up, `rounds` of each, medians. "statistics" is device
    work only; what a caller of LabelStatistics.apply_ndarray waits for (the range reduction for
    n_labels, the kernels, the copy of the state to the host and the numpy columns) is timed once
    per volume on the host clock as `apply_ndarray_s`."""
    import math
    import torch
    import zarrs_tools_amd as zt
    ctx = zt.default_context(0)
    stream = torch.cuda.current_stream()
    shape, total = (n, n, n), n ** 3
    gen = torch.Generator(device="cuda").manual_seed(2025)
    noise = torch.rand(shape, device="cuda", generator=gen)
    u16 = zt.synth_u16(shape)
    sample = u16.reshape(-1)[:: max(1, total // (1 << 20))].to(torch.float32)
    level = float(torch.quantile(sample, 0.7))
    masks = {"sparse_0.05_c1": ((noise < 0.05).to(torch.uint8), 1),
             "dense_0.6_c1": ((noise < 0.6).to(torch.uint8), 1),
             "dense_0.6_c3": ((noise < 0.6).to(torch.uint8), 3),
             "blobs_c1": ((u16.to(torch.float32) > level).to(torch.uint8), 1)}
    del noise, sample
    labels, counts = {}, {}
    for name, (m, c) in masks.items():
        labels[name], counts[name] = zt.ConnectedComponents(c).apply_ndarray(m, "uint32", ctx=ctx)
    ctx.release_scratch()
    del masks
    out = torch.empty(shape, dtype=torch.uint32, device="cuda")
    rng, f = zt.Range(), zt.LabelStatistics()
    rstate = rng.new_state("cuda", ctx)
    size_filter = zt.LabelSizeFilter(min_size=2)
    ops, kept = {}, {}
    for name, lab in labels.items():
        K = counts[name]
        states = {False: f.new_state(3, K, False, "cuda", ctx),
                  True: f.new_state(3, K, True, "cuda", ctx)}

        def stats(lab=lab, K=K, inten=None, st=None):
            zt._abi.check(zt.lib().zt_label_statistics_init(ctx.handle, 3, K, int(inten is not None),
                                                            st.data_ptr()))
            f.accumulate(lab, st, K, inten, None, ctx)

        ops[f"{name}_range"] = (lambda lab=lab: rng.accumulate(lab, rstate, ctx))
        ops[f"{name}_statistics"] = (lambda stats=stats, st=states[False]: stats(st=st))
        ops[f"{name}_statistics_u16"] = (lambda stats=stats, st=states[True]:
                                         stats(inten=u16, st=st))
        kept[name] = size_filter.apply_ndarray(lab, "uint32", ctx, out=out)[1]
        ops[f"{name}_size_filter"] = (lambda lab=lab: size_filter.apply_ndarray(lab, "uint32", ctx,
                                                                               out=out))
    reps = {}
    for k, fn in ops.items():  # warm-up, then calls per window until it lasts window_s
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
    res = {"op": "label_statistics, label_size_filter on uint32 labels (device-resident)",
           "config": {"shape": [n] * 3, "rounds": rounds, "window_s": window_s},
           "n_labels": counts, "kept_min_size_2": kept, "ops": {}}
    res["apply_ndarray_s"] = {}
    for name, lab in labels.items():  # the whole call, host work included, once
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = zt.LabelStatistics().apply_ndarray(lab, ctx=ctx)
        res["apply_ndarray_s"][name] = round(time.perf_counter() - t0, 3)
        assert got["n_labels"] == counts[name]
        del got
    for k in ops:
        v = sorted(ms[k])
        med = v[len(v) // 2]
        res["ops"][k] = {"ms": round(med, 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                         "spread": round((v[-1] - v[0]) / med, 4), "calls_per_window": reps[k],
                         "ns_per_voxel": round(med * 1e6 / total, 5)}
        if k.endswith("_range"):
            gbs = total * 4 / (med / 1e3) / 1e9
            res["ops"][k].update({"GB/s": round(gbs, 1), "hbm_frac": round(gbs / HBM_PEAK_GBS, 4)})
        else:
            base = k[:k.index("_c") + 3] + "_range"
            res["ops"][k]["ratio_to_range"] = round(med / res["ops"][base]["ms"], 3)
    return res


def bench_distance_transform(n, rounds=5, window_s=0.5, scipy_baseline=True, once=False):
    """The exact Euclidean distance transform on n^3 uint8 device arrays -> float32
    (distance.hip) through DistanceTransform.apply, on noise of foreground density 0.5 (shallow
    envelopes) and 0.999 (deep) and on one solid ball of radius 0.39 n (the worst-case stacks), at
    spacing (1, 1, 1) and (3, 1, 1), alternated in one run with the Reencode uint8 -> float32 cast
    of the same volume (one byte read and four written per element: the streaming floor, the
    yardstick). Windows of at least window_s after a warm-up, `rounds` of each, medians. With
    scipy installed and n <= 512, scipy.ndimage.distance_transform_edt on the host transforms
    the same volumes (the CPU baseline; its float64 result as float32 is compared with the
    device's). once=True: every transform called once, volume by volume, spacing ones then
    (3, 1, 1), and nothing else (for a kernel trace)."""
    import math
    import numpy as np
    import torch
    import zarrs_tools_amd as zt
    ctx = zt.default_context(0)
    stream = torch.cuda.current_stream()
    shape, total = (n, n, n), n ** 3
    gen = torch.Generator(device="cuda").manual_seed(2025)
    noise = torch.rand(shape, device="cuda", generator=gen)
    ax = torch.arange(n, device="cuda", dtype=torch.float32) - (n - 1) / 2
    r2 = ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2
    volumes = {"noise_0.5": (noise < 0.5).to(torch.uint8),
               "noise_0.999": (noise < 0.999).to(torch.uint8),
               "ball": (r2 <= (0.39 * n) ** 2).to(torch.uint8)}
    del noise, r2
    out = torch.empty(shape, dtype=torch.float32, device="cuda")
    cast = zt.PointwiseProgram([zt.Reencode()], "uint8", ["float32"], shape)
    spacings = {"s111": (1, 1, 1), "s311": (3, 1, 1)}
    filters = {k: zt.DistanceTransform(sp) for k, sp in spacings.items()}
    chunk = (32, 32, 32)

    def edt(v, k):
        return filters[k].apply(zt.DeviceArray(v, chunk, "uint8"),
                                zt.DeviceArray(out, chunk, "float32"), ctx=ctx)

    if once:
        for name, v in volumes.items():
            for k in spacings:
                edt(v, k)
        torch.cuda.synchronize()
        return {"op": "distance_transform, one call each",
                "calls": [f"{name}_{k}" for name in volumes for k in spacings]}
    ops = {}
    for name, v in volumes.items():
        ops[f"{name}_cast_u8_f32"] = (lambda v=v: cast.run(v, out, ctx))
        for k in spacings:
            ops[f"{name}_{k}"] = (lambda v=v, k=k: edt(v, k))
    reps = {}
    for k, fn in ops.items():  # warm-up, then calls per window until it lasts window_s
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
    res = {"op": "distance_transform uint8 -> float32 (device-resident)",
           "config": {"shape": [n] * 3, "rounds": rounds, "window_s": window_s},
           "foreground": {k: round(float(v.to(torch.float32).mean()), 4)
                          for k, v in volumes.items()},
           "memory_bytes": filters["s111"].memory("uint8", "float32", shape),
           "ops": {}}
    for k in ops:
        v = sorted(ms[k])
        med = v[len(v) // 2]
        res["ops"][k] = {"ms": round(med, 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                         "spread": round((v[-1] - v[0]) / med, 4), "calls_per_window": reps[k],
                         "ns_per_voxel": round(med * 1e6 / total, 5)}
        if k.endswith("_cast_u8_f32"):
            gbs = total * 5 / (med / 1e3) / 1e9
            res["ops"][k].update({"GB/s": round(gbs, 1), "hbm_frac": round(gbs / HBM_PEAK_GBS, 4)})
        else:
            y = res["ops"][k.rsplit("_", 1)[0] + "_cast_u8_f32"]
            res["ops"][k]["ratio_to_cast"] = round(med / y["ms"], 3)
    if scipy_baseline and n <= 512:
        try:
            from scipy import ndimage
        except ImportError:
            ndimage = None
        if ndimage is not None:
            for name, v in volumes.items():
                host = v.cpu().numpy()
                for k, sp in spacings.items():
                    t0 = time.perf_counter()
                    want = ndimage.distance_transform_edt(host, sampling=sp)
                    dt = time.perf_counter() - t0
                    edt(v, k)
                    got = out.cpu().numpy()
                    o = res["ops"][f"{name}_{k}"]
                    o["scipy_s"] = round(dt, 3)
                    o["scipy_over_gpu"] = round(dt * 1e3 / o["ms"], 1)
                    o["equals_scipy"] = bool(np.array_equal(got, want.astype(np.float32)))
    return res


def bench_reconstruction(n, rounds=3, window_s=0.5, scipy_size=256, once=False):
    """Morphological reconstruction (reconstruct.hip) on n^3 device arrays: fill_holes at
    connectivity 1 and 3 on the labelling's three uint8 volumes (noise 0.05, noise 0.6, synth_u16
    above its 0.7 quantile) and h_maxima (h = 1, connectivity 1) on the uint32 squared distance map
    of the blobs volume, alternated in one run with two yardsticks: the connected_components call
    on the same volume and the Reencode uint8 -> uint32 cast. Windows of at least window_s after a
    warm-up, `rounds` of each, medians. Every call synchronises the stream once per batch of
    rounds; those waits are inside the windows. Reported per case: the rounds of the call, ms per
    call, ms per round, and the streaming floor of a round (two reads and one write per element
    at HBM_PEAK_GBS). With scipy installed and scipy_size > 0, the same three masks at
    scipy_size^3 are filled on the host by scipy.ndimage.binary_fill_holes (its time, and equality
    with the device's result on that volume). once=True: every case called once and nothing else
    (for a kernel trace)."""
    import math
    import numpy as np
    import torch
    import zarrs_tools_amd as zt
    ctx = zt.default_context(0)
    stream = torch.cuda.current_stream()
    chunk = (32, 32, 32)

    def masks(m):
        shape, total = (m, m, m), m ** 3
        gen = torch.Generator(device="cuda").manual_seed(2025)
        noise = torch.rand(shape, device="cuda", generator=gen)
        u16 = zt.synth_u16(shape)
        sample = u16.reshape(-1)[:: max(1, total // (1 << 20))].to(torch.float32)
        level = float(torch.quantile(sample, 0.7))
        return {"sparse_0.05": (noise < 0.05).to(torch.uint8),
                "dense_0.6": (noise < 0.6).to(torch.uint8),
                "blobs": (u16.to(torch.float32) > level).to(torch.uint8)}

    shape, total = (n, n, n), n ** 3
    volumes = masks(n)
    out8 = torch.empty(shape, dtype=torch.uint8, device="cuda")
    out32 = torch.empty(shape, dtype=torch.uint32, device="cuda")
    d2 = torch.empty(shape, dtype=torch.uint32, device="cuda")
    zt.DistanceTransform(None, True).apply(zt.DeviceArray(volumes["blobs"], chunk, "uint8"),
                                           zt.DeviceArray(d2, chunk, "uint32"), ctx=ctx)
    ctx.synchronize()
    ctx.release_scratch()
    cast = zt.PointwiseProgram([zt.Reencode()], "uint8", ["uint32"], shape)
    fills = {c: zt.Reconstruction(mode="fill_holes", connectivity=c) for c in (1, 3)}
    hmax = zt.Reconstruction(mode="h_maxima", h=1.0)
    cc = zt.ConnectedComponents(1)

    def fill(v, c, out=None):
        return fills[c].apply(zt.DeviceArray(v, chunk, "uint8"),
                              zt.DeviceArray(out8 if out is None else out, chunk, "uint8"),
                              ctx=ctx)

    def h_maxima():
        return hmax.apply(zt.DeviceArray(d2, chunk, "uint32"),
                          zt.DeviceArray(out32, chunk, "uint32"), ctx=ctx)

    ops, counts, esz = {}, {}, {}
    for name, v in volumes.items():
        ops[f"{name}_cast_u8_u32"] = (lambda v=v: cast.run(v, out32, ctx))
        ops[f"{name}_connected_components_c1"] = (
            lambda v=v: cc.apply(zt.DeviceArray(v, chunk, "uint8"),
                                 zt.DeviceArray(out32, chunk, "uint32"), ctx=ctx))
        for c in (1, 3):
            ops[f"{name}_fill_holes_c{c}"] = (lambda v=v, c=c: fill(v, c))
            esz[f"{name}_fill_holes_c{c}"] = 1
    ops["blobs_d2_u32_h_maxima_1_c1"] = h_maxima
    esz["blobs_d2_u32_h_maxima_1_c1"] = 4
    first_s = {}
    for k in esz:
        t0 = time.perf_counter()
        counts[k] = int(ops[k]())  # the rounds of the call
        ctx.synchronize()
        first_s[k] = round(time.perf_counter() - t0, 4)
    if once:
        return {"op": "reconstruction, one call each", "config": {"shape": [n] * 3},
                "rounds": counts, "first_call_s": first_s}
    reps = {}
    for k, fn in ops.items():  # warm-up, then calls per window until it lasts window_s
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
    res = {"op": "reconstruction (device-resident)",
           "config": {"shape": [n] * 3, "rounds": rounds, "window_s": window_s,
                      "tile_sweeps": os.environ.get("ZT_REC_TILE_SWEEPS", "default")},
           "foreground": {k: round(float(v.to(torch.float32).mean()), 4)
                          for k, v in volumes.items()},
           "ops": {}}
    for k in ops:
        v = sorted(ms[k])
        med = v[len(v) // 2]
        res["ops"][k] = {"ms": round(med, 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                         "spread": round((v[-1] - v[0]) / med, 4), "calls_per_window": reps[k]}
        if k in counts:
            floor = total * 3 * esz[k] / (HBM_PEAK_GBS * 1e9) * 1e3
            name = k.split("_fill_holes")[0].split("_d2_")[0]
            res["ops"][k].update({
                "rounds_of_the_call": counts[k],
                "ms_per_round": round(med / counts[k], 4),
                "round_floor_ms": round(floor, 4),
                "round_over_floor": round(med / counts[k] / floor, 2),
                "ratio_to_cast": round(med / res["ops"][f"{name}_cast_u8_u32"]["ms"], 2),
                "ratio_to_connected_components": round(
                    med / res["ops"][f"{name}_connected_components_c1"]["ms"], 2)})
    if scipy_size > 0:
        try:
            from scipy import ndimage
        except ImportError:
            ndimage = None
        if ndimage is not None:
            small = masks(scipy_size)
            out = torch.empty((scipy_size,) * 3, dtype=torch.uint8, device="cuda")
            res["scipy"] = {"shape": [scipy_size] * 3}
            for name, v in small.items():
                host = v.cpu().numpy()
                for c in (1, 3):
                    t0 = time.perf_counter()
                    want = ndimage.binary_fill_holes(
                        host, structure=ndimage.generate_binary_structure(3, c))
                    dt = time.perf_counter() - t0
                    ms_gpu = timed(lambda v=v, c=c: fill(v, c, out), stream, 3)
                    got = out.cpu().numpy()
                    res["scipy"][f"{name}_fill_holes_c{c}"] = {
                        "scipy_s": round(dt, 3), "gpu_ms": round(ms_gpu, 3),
                        "scipy_over_gpu": round(dt * 1e3 / ms_gpu, 1),
                        "filled": int(want.sum() - host.sum()),
                        "equals_scipy": bool(np.array_equal(got.astype(bool), want))}
                    print(f"scipy {name} c{c}: {dt:.1f} s", file=sys.stderr, flush=True)
    return res


def bench_watershed(n, rounds=3, window_s=0.5):
    """The seeded watershed (watershed.hip) on n^3 device arrays: the relief is the uint32 squared
    distance map of the synth_u16 > q0.7 volume, flooded from its maxima (descending) inside the
    foreground; the seeds are the labelled h-maxima (h = 1) of that map (Reconstruction, then
    ConnectedComponents of the elements the reconstruction lowered). Alternated in one run with
    two yardsticks of unchanged code on the same volume: the Reconstruction h_maxima(1) call and
    the connected_components call (connectivity 1). Windows of at least window_s after a warm-up,
    `rounds` of each, medians. Every call synchronises the stream once per batch of rounds; those
    waits are inside the windows. Reported: the three round counts, ms per call, and the streaming
    floor of the phases the call launches (reads plus writes at HBM_PEAK_GBS)."""
    import math
    import torch
    import zarrs_tools_amd as zt
    ctx = zt.default_context(0)
    stream = torch.cuda.current_stream()
    chunk = (32, 32, 32)
    shape, total = (n, n, n), n ** 3
    u16 = zt.synth_u16(shape)
    sample = u16.reshape(-1)[:: max(1, total // (1 << 20))].to(torch.float32)
    level = float(torch.quantile(sample, 0.7))
    blobs = (u16.to(torch.float32) > level).to(torch.uint8)
    del u16

    def arr(t, dtype):
        return zt.DeviceArray(t, chunk, dtype)

    d2 = torch.empty(shape, dtype=torch.uint32, device="cuda")
    zt.DistanceTransform(None, True).apply(arr(blobs, "uint8"), arr(d2, "uint32"), ctx=ctx)
    out32 = torch.empty(shape, dtype=torch.uint32, device="cuda")
    hmax = zt.Reconstruction(mode="h_maxima", h=1.0)
    cc = zt.ConnectedComponents(1)
    hmax.apply(arr(d2, "uint32"), arr(out32, "uint32"), ctx=ctx)
    ctx.synchronize()
    # the h-maxima: where the reconstruction of d2 - 1 under d2 stays below d2
    maxima = (d2.view(torch.int32) != out32.view(torch.int32)).to(torch.uint8)
    seeds = torch.empty(shape, dtype=torch.uint32, device="cuda")
    n_seeds = int(cc.apply(arr(maxima, "uint8"), arr(seeds, "uint32"), ctx=ctx))
    ctx.synchronize()
    ctx.release_scratch()
    del maxima
    labels = torch.empty(shape, dtype=torch.uint32, device="cuda")
    ws = zt.Watershed(1, descending=True, foreground_only=True)
    ops = {
        "h_maxima_1_c1": lambda: hmax.apply(arr(d2, "uint32"), arr(out32, "uint32"), ctx=ctx),
        "connected_components_c1": lambda: cc.apply(arr(blobs, "uint8"), arr(out32, "uint32"),
                                                    ctx=ctx),
        "watershed_c1": lambda: ws.apply(arr(d2, "uint32"), arr(seeds, "uint32"),
                                         arr(labels, "uint32"), ctx=ctx),
    }
    t0 = time.perf_counter()
    counts = tuple(ops["watershed_c1"]())
    ctx.synchronize()
    first_s = round(time.perf_counter() - t0, 4)
    h_rounds = int(ops["h_maxima_1_c1"]())
    labelled = int((labels.view(torch.int32) != 0).sum())
    foreground = int(blobs.sum())
    reps = {}
    for k, fn in ops.items():  # warm-up, then calls per window until it lasts window_s
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
    res = {"op": "watershed (device-resident)",
           "config": {"shape": [n] * 3, "rounds": rounds, "window_s": window_s,
                      "relief": "uint32 squared distance of synth_u16 > q0.7", "descending": True,
                      "foreground_only": True, "connectivity": 1, "seeds": n_seeds,
                      "tile_sweeps": os.environ.get("ZT_REC_TILE_SWEEPS", "default")},
           "foreground": foreground, "labelled": labelled, "first_call_s": first_s, "ops": {}}
    for k in ops:
        v = sorted(ms[k])
        med = v[len(v) // 2]
        res["ops"][k] = {"ms": round(med, 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                         "spread": round((v[-1] - v[0]) / med, 4), "calls_per_window": reps[k]}
    res["ops"]["h_maxima_1_c1"]["rounds_of_the_call"] = h_rounds
    # bytes per element of the phases launched, 4-byte relief, seeds and indices: init reads the
    # relief and the seeds and writes J0, the relief copy and d (20); a pass round and a distance
    # round read two arrays and write one (12); the parents read c, d and the seeds and write one
    # (16); a jump reads P, gathers P[P] and writes (12); the labels read the roots, gather the
    # seeds and write (12)
    per_elem = 20 + 12 * counts[0] + 12 * counts[1] + 16 + 12 * counts[2] + 12
    floor = total * per_elem / (HBM_PEAK_GBS * 1e9) * 1e3
    w = res["ops"]["watershed_c1"]
    w.update({"pass_rounds": counts[0], "distance_rounds": counts[1], "jumps": counts[2],
              "floor_bytes_per_element": per_elem, "floor_ms": round(floor, 3),
              "over_floor": round(w["ms"] / floor, 2),
              "ratio_to_h_maxima": round(w["ms"] / res["ops"]["h_maxima_1_c1"]["ms"], 2),
              "ratio_to_connected_components": round(
                  w["ms"] / res["ops"]["connected_components_c1"]["ms"], 2)})
    return res


def bench_guided4d(shape, chunk, radius, reps):
    """Config T per GPU: a (T, Z, Y, X) f32 time-series share, chunks
    (4, 256, 256, 256), eps 2500. 4-D arrays take the separable per-axis path."""
    import numpy as np
    import torch
    import zarrs_tools_amd as zt
    from oracle import oracle as O
    ctx = zt.default_context(0)
    x = zt.synth_step_noise_f32(tuple(shape))
    y = torch.empty_like(x)
    g = zt.GuidedFilter(2500.0, radius)
    a_in, a_out = zt.DeviceArray(x, chunk), zt.DeviceArray(y, chunk)
    ms = timed(lambda: g.apply(a_in, a_out, ctx=ctx), torch.cuda.current_stream(), reps)
    n = int(np.prod(shape))
    gbs = n * 8 / (ms / 1e3) / 1e9
    sshape = (4, 64, 64, 64)
    sample = O.synth_step_noise_f32(sshape)
    t0 = time.perf_counter()
    O.guided_filter_apply(sample, (4, 32, 32, 32), 2500.0, radius, nthreads=1)
    cpu_s = time.perf_counter() - t0
    del x, y
    torch.cuda.empty_cache()
    return {"op": f"guided_filter r={radius} 4-D time-series (device-resident)",
            "config": {"shape": list(shape), "dtype": "float32", "chunk": list(chunk),
                       "eps": 2500.0},
            "ms": round(ms, 4), "gib_per_s": round(n * 4 / 2 ** 30 / (ms / 1e3), 3),
            "roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
                         "algorithmic_bytes": n * 8},
            "cpu_baseline": {"gib_per_s": round(int(np.prod(sshape)) * 4 / 2 ** 30 / cpu_s, 5),
                             "cores": 1, "kind": "port",
                             "sample": f"{list(sshape)} f32 block in (4,32,32,32) chunks, oracle "
                             "guided filter (C restatement of guided_filter.rs)"}}


def bench_t_share(reps, radius=2, groups=None, rank=None):
    """Config T's real per-GPU share: rank `rank` of an 8-GPU split of the
    (32, 1024^3) f32 series in (4, 256^3) chunks, timed alone on this GPU. The chunk grid is
    split in (t, z) blocks of whole chunks (shard.block_assignment; `groups` = (t groups, z groups),
    default the input-minimising 2 x 4: 16 output timepoints x 256 planes from a 20 x 264-plane
    input, 1.29x stage-1 work, where rows along t (8 x 1) read 12 timepoints for 4, 3x). The
    rank's halo'd input block is generated from the global synthetic definition and filtered in
    one GuidedFilter::apply_ndarray call on its output box (chunked == whole with the 2r halo,
    SURVEY.md §0.2). Algorithmic bytes: 8 per OUTPUT voxel (halo reads not credited)."""
    import numpy as np
    import torch
    import zarrs_tools_amd as zt
    from zarrs_tools_amd import shard
    from zarrs_tools_amd.filter import ArraySubset
    from oracle import oracle as O
    ctx = zt.default_context(0)
    gshape, chunk, world = (32, 1024, 1024, 1024), (4, 256, 256, 256), 8
    halo = 2 * radius
    groups = tuple(groups) if groups else shard.block_split(world, gshape, chunk, halo)
    if rank is None:  # an interior block (largest input)
        rank = (groups[0] // 2) * groups[1] + groups[1] // 2 if groups[1] > 1 else groups[0] // 2
    a = shard.block_assignment(rank, world, gshape, chunk, halo, groups)
    x = zt.synth_box(a.in_start, a.in_shape, gshape, kind="float32", ctx=ctx)
    rel0 = tuple(o - i for o, i in zip(a.out_start, a.in_start))
    g = zt.GuidedFilter(2500.0, radius)
    sub = ArraySubset(rel0, a.out_shape)
    res = {}

    def run():
        res["y"] = None  # drop the previous output first (the caching allocator reuses it)
        res["y"] = g.apply_ndarray(x, sub, ctx=ctx)

    ms = timed(run, torch.cuda.current_stream(), reps)
    y = res["y"]
    n = int(np.prod(a.out_shape))
    gbs = n * 8 / (ms / 1e3) / 1e9
    # parity: one interior chunk of the share against the oracle's per-chunk result
    cidx = tuple((o + s // 2) // c for o, s, c in zip(a.out_start, a.out_shape, chunk))
    (o0, osh, ref), = O.guided_filter_synth_chunks(gshape, chunk, [cidx], 2500.0, radius,
                                                   nthreads=16)
    sl = tuple(slice(p - q, p - q + s) for p, q, s in zip(o0, a.out_start, osh))
    got = y[sl].cpu().numpy()
    rel = float((np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max())
    del x, y, res
    ctx.release_scratch()
    torch.cuda.empty_cache()
    return {"op": f"guided_filter r={radius} 4-D, config T per-GPU share (device-resident)",
            "config": {"global_shape": list(gshape), "chunk": list(chunk), "world": world,
                       "groups_t_z": list(groups), "rank": rank,
                       "output_box": [list(a.out_start), list(a.out_shape)],
                       "input_box": [list(a.in_start), list(a.in_shape)],
                       "dtype": "float32", "eps": 2500.0,
                       "path": "one apply_ndarray call on the halo'd (t, z) block: 4-D three-kernel form (box3_march_kernel, g4_tab_kernel, box3_final_kernel)"},
            "ms": round(ms, 4), "gib_per_s": round(n * 4 / 2 ** 30 / (ms / 1e3), 3),
            "roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
                         "algorithmic_bytes": n * 8},
            "parity_chunk": list(cidx), "parity_max_rel": rel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pyramid-size", type=int, default=2048)
    ap.add_argument("--gaussian-size", type=int, default=1024)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--t-shape", type=int, nargs=4, default=[4, 1024, 1024, 1024])
    ap.add_argument("--only", default="pyramid,gaussian,tshare")
    ap.add_argument("--t-groups", type=int, nargs=2, default=None,
                    help="config T share: (t groups, z groups) of the 8-GPU split")
    ap.add_argument("--t-rank", type=int, default=None)
    ap.add_argument("--no-scipy", action="store_true",
                    help="connected_components, distance_transform: skip the scipy.ndimage "
                         "baseline on the host")
    ap.add_argument("--cc-once", action="store_true",
                    help="connected_components: call every labelling once, nothing else (for a "
                         "kernel trace)")
    ap.add_argument("--edt-once", action="store_true",
                    help="distance_transform: call every transform once, nothing else (for a "
                         "kernel trace)")
    ap.add_argument("--rec-once", action="store_true",
                    help="reconstruction: call every case once, nothing else (for a kernel trace)")
    ap.add_argument("--rec-scipy-size", type=int, default=256,
                    help="reconstruction: the edge of the volumes that scipy.ndimage."
                         "binary_fill_holes fills on the host (0 or --no-scipy skips it)")
    a = ap.parse_args()
    only = set(a.only.split(","))
    if "tshare" in only:
        print(json.dumps(bench_t_share(a.reps, groups=a.t_groups, rank=a.t_rank)), flush=True)
    if "guided4d" in only:
        print(json.dumps(bench_guided4d(a.t_shape, (4, 256, 256, 256), 2, a.reps)), flush=True)
        if only == {"guided4d"}:
            return
    if "pyramid" in only:
        print(json.dumps(bench_pyramid(a.pyramid_size, a.reps, a.levels)), flush=True)
    if "pyramid_u8" in only:  # the u8 mean pyramid (16-byte rows per lane: 2 level-3 columns)
        print(json.dumps(bench_pyramid(a.pyramid_size, a.reps, a.levels, False, "uint8")),
              flush=True)
    if "pyramid_i8" in only:  # the i8 mean and mode pyramids (the packed-byte kernel)
        for disc in (False, True):
            print(json.dumps(bench_pyramid(a.pyramid_size, a.reps, a.levels, disc, "int8")),
                  flush=True)
    if "pyramid_discrete" in only:
        for dt in ("uint16", "uint8"):
            print(json.dumps(bench_pyramid(a.pyramid_size, a.reps, a.levels, True, dt)),
                  flush=True)
    if "gaussian" in only:
        print(json.dumps(bench_gaussian(a.gaussian_size, a.reps)), flush=True)
    if "gradient" in only:  # with its Gaussian half-size-1 yardstick, alternated
        print(json.dumps(bench_gradient(a.gaussian_size)), flush=True)
    if "rank" in only:  # each with the Gaussian half-size-1 yardstick, alternated
        for dt in ("float32", "uint8"):
            for res in bench_rank(a.gaussian_size, dt):
                print(json.dumps(res), flush=True)
    if "sat" in only:  # each with its reencode-cast yardstick, alternated
        for din, dout in (("float32", "float32"), ("uint16", "uint64")):
            print(json.dumps(bench_sat(a.gaussian_size, din, dout)), flush=True)
    if "pointwise" in only:  # each with its reencode-cast yardstick, alternated
        for res in bench_pointwise(a.gaussian_size):
            print(json.dumps(res), flush=True)
    if "info" in only:  # each with its pointwise-reencode yardstick, alternated
        for res in bench_info(a.gaussian_size):
            print(json.dumps(res), flush=True)
    if "compare" in only:  # with the range over the same bytes, alternated
        print(json.dumps(bench_compare(a.gaussian_size)), flush=True)
    if "arithmetic" in only:  # with the float32 rescale yardstick, alternated
        print(json.dumps(bench_arithmetic(a.gaussian_size)), flush=True)
    if "label_statistics" in only:  # with Range on the same label arrays, alternated
        print(json.dumps(bench_label_statistics(a.gaussian_size)), flush=True)
    if "connected_components" in only:  # with the reencode uint8 -> uint32 yardstick, alternated
        print(json.dumps(bench_connected_components(
            a.gaussian_size, scipy_baseline=not a.no_scipy, once=a.cc_once)), flush=True)
    if "distance_transform" in only:  # with the reencode uint8 -> float32 yardstick, alternated
        print(json.dumps(bench_distance_transform(
            a.gaussian_size, scipy_baseline=not a.no_scipy, once=a.edt_once)), flush=True)
    if "reconstruction" in only:  # with the labelling and the reencode cast, alternated
        print(json.dumps(bench_reconstruction(
            a.gaussian_size, scipy_size=0 if a.no_scipy else a.rec_scipy_size,
            once=a.rec_once)), flush=True)
    if "watershed" in only:  # with h_maxima and the labelling of the same volume, alternated
        print(json.dumps(bench_watershed(a.gaussian_size)), flush=True)


if __name__ == "__main__":
    main()
