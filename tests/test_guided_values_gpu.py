"""GPU parity of the guided filter at the edges of its value range, on each of its arithmetic
paths, against the oracle run on the same input (tests/guided_value_cases.py; the CPU file
tests/test_guided_values.py checks that the inputs are what they claim to be).

Float outputs: scaled_rel_err <= FLOAT_TOL, the suite's 1e-5 taken relative to the data's scale
(tests/gpu_util.py); integer and 16-bit float outputs: assert_cast_bracketed. Every output buffer
is poisoned first, and every case runs on the whole array and chunk by chunk.
"""
import functools
import itertools

import numpy as np
import pytest

from oracle import oracle as O
from tests import guided_value_cases as V
from tests.gpu_util import (FLOAT_TOL, assert_cast_bracketed, from_dev, poisoned, rel_err,
                            scaled_rel_err, to_dev, value_scale)

pytestmark = pytest.mark.gpu

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)


def gpu_whole(v, din, dout, chunk, eps, r):
    import torch
    x, y = to_dev(v, din), poisoned(v.shape, dout)
    zt.GuidedFilter(eps, r).apply(zt.DeviceArray(x, chunk, din), zt.DeviceArray(y, chunk, dout))
    torch.cuda.synchronize()
    return from_dev(y, dout)


def gpu_chunked(v, din, dout, chunk, eps, r):
    """tests/test_guided_filter_gpu.gpu_apply_chunked into a poisoned buffer."""
    import torch
    x, y = to_dev(v, din), poisoned(v.shape, dout)
    a_in, a_out = zt.DeviceArray(x, chunk, din), zt.DeviceArray(y, chunk, dout)
    g = zt.GuidedFilter(eps, r)
    for idx in itertools.product(*[range(n) for n in a_out.chunk_grid_shape()]):
        g.apply_chunk(a_in, a_out, idx)
    torch.cuda.synchronize()
    return from_dev(y, dout)


def both(p: V.Path, v32, eps, stored=None, din=None, dout="float32"):
    """(label, output) of the whole-array and the per-chunk run. `stored` are the values in the
    input type where that is not f32."""
    din = din or p.din
    src = stored if stored is not None else v32.astype(O.NP_STORAGE[din])
    return [("whole", gpu_whole(src, din, dout, p.chunk, float(eps), p.r)),
            ("chunks", gpu_chunked(src, din, dout, p.chunk, float(eps), p.r))]


def check_float(tag, out, ref, S):
    nan = int(np.isnan(out).sum())
    err = scaled_rel_err(np.nan_to_num(out, nan=0.0), ref, S) if nan else scaled_rel_err(out, ref, S)
    print(f"{tag}: scaled rel err {err:.3e} (unscaled max(1, |ref|) form: "
          f"{rel_err(np.nan_to_num(out, nan=0.0), ref):.3e}), NaN {nan}, bit-exact "
          f"{float(np.mean(out == ref)):.4f}")
    assert nan == 0, f"{tag}: {nan} NaN (unwritten or computed) in the output"
    assert err <= FLOAT_TOL, f"{tag}: {err:.3e}"


# ---- A ----

@functools.lru_cache(maxsize=None)
def a_unscaled_gpu(pid, eps0):
    p = V.PATHS[pid]
    v, eps = V.a_input(pid, 0, eps0)
    out = gpu_whole(v.astype(O.NP_STORAGE[p.din]), p.din, "float32", p.chunk, float(eps), p.r)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("k", V.A_KS)
@pytest.mark.parametrize("pid", V.A_PATHS)
def test_a_scale_sweep(pid, k):
    """v0 * 2^k with eps0 * 4^k: the same filter in other units. k = +56 puts s + eps past 2^126
    on 5 % of the elements or more (a subnormal reciprocal), k = -64 makes eps and 1 % of the
    s + eps subnormal; both are finite on the oracle."""
    p = V.PATHS[pid]
    for eps0 in V.A_EPS0:
        v, eps = V.a_input(pid, k, eps0)
        ref = V.oracle(v, p, eps)
        for how, out in both(p, v, eps):
            check_float(f"A {pid} k={k} eps0={eps0} {how}", out, ref, 2.0 ** k)


@pytest.mark.parametrize("pid", V.A_PATHS)
def test_a_scale_equivariance_share(pid):
    """gpu(v0 * 2^k) / 2^k against gpu(v0), bit for bit: printed per k (DESIGN.md §4 records the
    shares); asserted where the arithmetic must be exponent-blind, see A_EXACT_KS."""
    p = V.PATHS[pid]
    for eps0 in V.A_EPS0:
        base = a_unscaled_gpu(pid, eps0)
        for k in V.A_EQUIVARIANT_KS:
            v, eps = V.a_input(pid, k, eps0)
            out = gpu_whole(v.astype(O.NP_STORAGE[p.din]), p.din, "float32", p.chunk, float(eps),
                            p.r)
            want = (base.astype(np.float64) * 2.0 ** k).astype(np.float32)
            share = float(np.mean(out == want))
            print(f"A-equivariance {pid} k={k} eps0={eps0}: bit-equal share {share:.6f}")
            if k in A_EXACT_KS:
                assert share == 1.0, (k, eps0, share)


A_EXACT_KS = (-20, 40)


# ---- B ----

@pytest.mark.parametrize("pid", V.B_PATHS)
def test_b_small_values(pid):
    """A normalised image: the plain max(1, |ref|) metric is an absolute 1e-5 here."""
    p = V.PATHS[pid]
    v = V.b_input(pid)
    S = value_scale(v)
    for eps in V.B_EPS:
        ref = V.oracle(v, p, eps)
        for how, out in both(p, v, eps):
            check_float(f"B {pid} eps={eps:.3g} {how}", out, ref, S)


# ---- C ----

@pytest.mark.parametrize("pid", V.C_PATHS)
def test_c_zero_eps_and_zero_variance(pid):
    p = V.PATHS[pid]
    v = V.c_random(pid)
    ref = V.oracle(v, p, 0.0)
    for how, out in both(p, v, 0.0):
        check_float(f"C {pid} eps=0 {how}", out, ref, 1.0)
        assert rel_err(out, ref) <= FLOAT_TOL
    w = V.c_constant(pid)
    ref = V.oracle(w, p, V.C_CONST_EPS)
    for how, out in both(p, w, V.C_CONST_EPS):
        check_float(f"C {pid} constant rows {how}", out, ref, 1.0)
        assert rel_err(out, ref) <= FLOAT_TOL


# ---- D ----

@pytest.mark.parametrize("din", V.D_TYPES)
@pytest.mark.parametrize("pid", V.D_PATHS)
def test_d_wide_input_types(pid, din):
    """Full-range int32 / uint32 / int64 / uint64 and wide float64 values through the loaders'
    Elem<T>::to_f32 or the f32 staging: one rounding to f32, then s up to 2^126 and beyond."""
    p = V.PATHS[pid]
    v, v32, eps = V.d_input(pid, din)
    S = value_scale(v32)
    ref = V.oracle(v32, p, eps)
    runs = both(p, v32, eps, stored=v, din=din)
    for how, out in runs:
        check_float(f"D {pid} {din} {how}", out, ref, S)
    # The filter sees a value only as its f32 image, rounded once: the same call on the images
    # gives the same bits. One f32 ulp of one input is far below any tolerance (2^-23 relative),
    # so only this comparison notices a conversion that rounds twice (the planted 64-bit integers
    # and the float64 value just above the tie 2^24 + 1).
    same = gpu_whole(v32, "float32", "float32", p.chunk, float(eps), p.r)
    differ = runs[0][1].view(np.uint32) != same.view(np.uint32)
    print(f"D {pid} {din}: {int(differ.sum())} outputs differ from the run on the f32 images")
    assert not differ.any()


# ---- E ----

@pytest.mark.parametrize("dout", list(O.DTYPES))
@pytest.mark.parametrize("k", V.E_SCALES)
def test_e_output_casts_at_range(k, dout):
    """+-300 * 2^40 saturates every integer type (int64 / uint64 in part), overflows float16 and
    sends negative values to 0 in the unsigned types; +-300 truncates toward zero on both sides
    of it."""
    p = V.PATHS[V.E_PATH]
    v, eps = V.e_input(k)
    ref = V.oracle(v, p, eps)
    for how, out in both(p, v, eps, dout=dout):
        if dout in ("float32", "float64"):
            check_float(f"E k={k} {dout} {how}", out, ref, 2.0 ** k)
        else:
            assert_cast_bracketed(out, ref, dout, 2.0 ** k)


# ---- F ----

@pytest.mark.parametrize("kind", list(V.F_VALUES))
@pytest.mark.parametrize("pid", V.F_PATHS)
def test_f_one_non_finite_element(pid, kind):
    """The contract of DESIGN.md §4 for one NaN / +inf / -inf, and no more: the call returns,
    every output within 2r of the element is NaN, every output at least F_BOUND from it along one
    of the last two axes is bitwise the output of the array with 0 in its place (which has no
    NaN, so no poisoned element survives there). No oracle: its NaN pattern is that of its
    summed-area tables."""
    p = V.PATHS[pid]
    bad, clean, pos = V.f_inputs(pid, kind)
    near, far = V.f_masks(pid)
    for run in (gpu_whole, gpu_chunked):
        want = run(clean, "float32", "float32", p.chunk, 50.0, p.r)
        assert not np.isnan(want).any()
        out = run(bad, "float32", "float32", p.chunk, 50.0, p.r)
        print(f"F {pid} {kind} {run.__name__}: NaN share {float(np.isnan(out).mean()):.4f}, "
              f"near {int(near.sum())}, pinned {float(far.mean()):.3f}")
        assert np.isnan(out[near]).all()
        assert np.array_equal(out[far].view(np.uint32), want[far].view(np.uint32))
