"""GPU parity of the fused guided filter where P5's v comes from the leaving stage-1 quad
(gf_fused.hpp, GF_V5LEAVE: r = 4, mode 1). The P12 lanes inside the tile store the quad of the
slice leaving the z-window to the LDS buffer Vs; P5 reads its v from there one barrier later.

tests/test_guided_fused_counts_gpu.py and tests/test_guided_fused_modes_gpu.py cover partial
tiles, short arrays, z-segments, slabs and the integer inputs on array-aligned tiles. This file
adds what the hand-off can newly get wrong: an output box that does not start at the array origin
(tile coordinates differ from array coordinates), two tiles in x and y, the integer stage 1
through Vs, and data on which a v taken from a neighbouring voxel cannot pass.

The criterion is the suite's: |gpu - oracle| <= FLOAT_TOL * max(1, |oracle|), outputs pre-filled
with NaN. The hand-off is enabled for r = 4 in mode 1 only, so every case is quad-aligned r = 4
(asserted: fused_quad_ok's conditions, gf_plan.hpp).
"""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import fused_cases as FC
from tests.gpu_util import FLOAT_TOL, from_dev, to_dev
from tests.test_guided_fused_modes_gpu import apply_array, apply_ndarray_into, report_and_check

pytestmark = pytest.mark.gpu

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)

R = 4
SUB_SHAPE = (20, 80, 136)
SUB_BOX = ((2, 8, 12), (14, 64, 116))  # ox0, oy0 multiples of 4: the launch stays mode 1
WHOLE_SHAPE = (12, 64, 128)            # 2 x 2 tiles of 64 x 32


@functools.lru_cache(maxsize=None)
def ramp_noise(shape, din):
    """A ramp with a different slope per axis (no x/y symmetry, no two voxels of a slice on the
    same ramp value) plus noise of a larger amplitude: neighbouring voxels differ by tens to
    hundreds (f32) or thousands (u16), so a v taken from the wrong lane moves the output by far
    more than the tolerance."""
    rng = np.random.default_rng(4242)
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    if din == "float32":
        v = (0.37 * x + 1.91 * y + 5.3 * z + 300.0 * rng.random(shape)).astype(np.float32)
    else:
        v = (23 * x + 91 * y + 7 * z + rng.integers(0, 40000, size=shape)).astype(np.uint16)
        assert float(v.max()) < 65535
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def oracle_of(shape, din, eps):
    ref = O.guided_filter_apply(O.cast_to_f32(ramp_noise(shape, din), din), shape, eps, R,
                                nthreads=8)
    ref.setflags(write=False)
    return ref


def box_mean(a, r):
    """Mean over the (2r+1)^3 window clamped to the array, in f64 (cumulative sums per axis)."""
    a = a.astype(np.float64)
    for ax, n in enumerate(a.shape):
        c = np.concatenate([np.zeros_like(np.take(a, [0], axis=ax)), np.cumsum(a, axis=ax)], axis=ax)
        i = np.arange(n)
        hi, lo = np.minimum(i + r + 1, n), np.maximum(i - r, 0)
        cnt = (hi - lo).reshape([-1 if k == ax else 1 for k in range(a.ndim)])
        a = (np.take(c, hi, axis=ax) - np.take(c, lo, axis=ax)) / cnt
    return a


def mean_a(v, eps):
    """The coefficient the output multiplies v by: out = mean(a) * v + mean(b)."""
    v = v.astype(np.float64)
    u = box_mean(v, R)
    s = (v - u) ** 2
    return box_mean(s / (s + eps), R)


def fails_criterion(out, ref):
    return np.abs(out.astype(np.float64) - ref) > FLOAT_TOL * np.maximum(1.0, np.abs(ref))


def assert_quad_aligned(L: FC.Launch, in_ptr, out_ptr):
    esz_in, esz_out = FC.ESIZE[L.din], FC.ESIZE[L.dout]
    assert L.r % 2 == 0 and L.ox0 % 4 == 0 and L.nx % 4 == 0 and L.onx % 4 == 0
    assert L.in_sy % 4 == 0 and L.in_sz % 4 == 0 and L.out_sy % 4 == 0 and L.out_sz % 4 == 0
    assert in_ptr % (4 * esz_in) == 0 and out_ptr % (4 * esz_out) == 0


def case(id_, shape, eps, din="float32"):
    return FC.Case(id_, "P", "array", shape, shape, R, eps, FC.M1, 0, din=din, dout="float32")


def sub_launch(din):
    nz, ny, nx = SUB_SHAPE
    (z0, y0, x0), (onz, ony, onx) = SUB_BOX
    return FC.Launch(ny, nx, y0, x0, onz, ony, onx, ny * nx, nx, ony * onx, onx, 0, 0, R, din,
                     "float32", 0)


def run_subset(din, eps):
    import torch
    v = ramp_noise(SUB_SHAPE, din)
    L = sub_launch(din)
    x = to_dev(v, din)
    sub = zt.ArraySubset(*SUB_BOX)
    out = apply_ndarray_into(x, x.data_ptr(), sub, L, eps)
    torch.cuda.synchronize()
    assert_quad_aligned(L, x.data_ptr(), out.data_ptr())
    box = tuple(slice(s, s + n) for s, n in zip(*SUB_BOX))
    return from_dev(out, "float32"), oracle_of(SUB_SHAPE, din, eps)[box], box


@pytest.mark.parametrize("din", ["float32", "uint16"])
@pytest.mark.parametrize("eps", [0.5, 2500.0])
def test_misrouted_v_cannot_pass(din, eps):
    """CPU check of the data (no kernel): the oracle output with v taken one column, or one row,
    away fails the criterion almost everywhere in the output box, so a Vs row / column mix-up
    or a tile-vs-array coordinate slip cannot hide in the tolerance."""
    v = O.cast_to_f32(ramp_noise(SUB_SHAPE, din), din).astype(np.float64)
    ref = oracle_of(SUB_SHAPE, din, eps).astype(np.float64)
    ma = mean_a(v, eps)
    box = tuple(slice(s, s + n) for s, n in zip(*SUB_BOX))
    for axis in (1, 2):
        wrong = ref + ma * (np.roll(v, 1, axis=axis) - v)  # mean(a) * v' + mean(b)
        bad = fails_criterion(wrong[box], ref[box])
        margin = np.abs(wrong[box] - ref[box]) / (FLOAT_TOL * np.maximum(1.0, np.abs(ref[box])))
        print(f"{din} eps {eps:g} axis {axis}: {bad.mean():.4f} of the box fails, median margin "
              f"{np.median(margin):.3g} x the tolerance")
        assert bad.mean() > 0.99
        assert np.median(margin) > 1000.0


@pytest.mark.parametrize("eps", [0.5, 2500.0])
def test_output_box_off_origin(eps):
    """apply_ndarray on (20, 80, 136) with the box (2, 8, 12) + (14, 64, 116): tile origins are
    not array-aligned; 2 x 2 tiles, the second partial in x."""
    out, ref, _ = run_subset("float32", eps)
    report_and_check(case(f"P-sub-f32-eps{eps:g}", SUB_SHAPE, eps), out, ref)


def test_output_box_off_origin_u16():
    """The integer stage 1 through Vs: u16 -> f32, eps 0.5 (a 1-ulp error of v or u shows)."""
    out, ref, _ = run_subset("uint16", 0.5)
    report_and_check(case("P-sub-u16-eps0.5", SUB_SHAPE, 0.5, "uint16"), out, ref)


@pytest.mark.parametrize("eps", [0.5, 2500.0])
def test_two_tiles_each_way(eps):
    """(12, 64, 128) whole array: two full tiles in x and in y, every wave's K5 rows in use."""
    c = case(f"P-whole-f32-eps{eps:g}", WHOLE_SHAPE, eps)
    (L,) = c.launches()
    assert_quad_aligned(L, 0, 0)
    report_and_check(c, apply_array(c, ramp_noise(WHOLE_SHAPE, "float32")),
                     oracle_of(WHOLE_SHAPE, "float32", eps))
