"""GPU parity of the downsample launch forms, loops and values that tests/test_downsample_gpu.py
does not reach, against the oracle, bit for bit (downsample.hip sums in f64 in the reference's
order, or exactly in integers).

How a call is dispatched (downsample.hip launch_ds_types, zt_api.hip zt_pyramid_downsample):
  * Downsample::apply_ndarray_*: rank 3 with window (2, 2, 2) and out_shape[1] <= 65535 takes
    downsample3_kernel / downsample3_mode_kernel (grid z capped at 262144 / (gx * gy), the rest
    looped); everything else the N-d downsample_continuous_kernel / downsample_discrete_kernel
    (at most 16384 workgroups of 256, grid-stride beyond);
  * zt.pyramid: rank 3, factor (2, 2, 2), not f16 / bf16: up to three levels per launch of
    pyramid3_fused_kernel (pyramid3_u8_kernel for 1-byte types), VEC when the rows are whole
    aligned vectors; at most 128 z layers, the level-1 z blocks beyond looped.

NaNs compare by position only, through assert_same_bits_nan and its 2 % cap on the reference.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests.gpu_util import assert_same_bits_nan, from_dev, poisoned, to_dev

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)

pytestmark = pytest.mark.gpu

def gpu_ds(v, din, stride, dout, discrete=False):
    """Downsample::apply_ndarray_continuous / _discrete on the whole block."""
    import torch
    d = zt.Downsample(stride, discrete)
    x = to_dev(v, din)
    y = d.apply_ndarray_discrete(x, dout) if discrete else d.apply_ndarray_continuous(x, dout)
    torch.cuda.synchronize()
    return from_dev(y, dout)


def gpu_ds_array(v, din, stride, dout, discrete=False):
    """Downsample::apply on device arrays, into a poisoned output."""
    import torch
    d = zt.Downsample(stride, discrete)
    oshape = d.output_shape(v.shape)
    y = poisoned(oshape, dout)
    chunk = tuple(max(1, (n + 1) // 2) for n in oshape)
    d.apply(zt.DeviceArray(to_dev(v, din), tuple(v.shape), din), zt.DeviceArray(y, chunk, dout))
    torch.cuda.synchronize()
    return from_dev(y, dout)


def full_range(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype.startswith("float"):
        return (rng.standard_normal(shape) * 1000.0).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, shape, dtype=dtype, endpoint=True)


def few_values(shape, dtype, seed):
    """Five values of the full range: ties and majorities both occur in a window."""
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    pool = rng.integers(info.min, info.max, 5, dtype=dtype, endpoint=True)
    return pool[rng.integers(0, 5, shape)]


def check_pyramid(v, dtype, levels, discrete=False, expect_levels=None):
    """zt.pyramid against the oracle level by level and against one Downsample launch per level;
    returns the oracle's levels. The levels are compared as one concatenated array, so the NaN
    cap of assert_same_bits_nan holds for the pyramid as a whole (its smallest level has a few
    elements only)."""
    import torch
    x = to_dev(v, dtype)
    got = zt.pyramid(x, (2, 2, 2), max_levels=levels, discrete=discrete)
    plain, cur_dev = [], x
    d = zt.Downsample((2, 2, 2), discrete)
    for _ in got:
        cur_dev = (d.apply_ndarray_discrete(cur_dev) if discrete
                   else d.apply_ndarray_continuous(cur_dev))
        plain.append(cur_dev)
    torch.cuda.synchronize()
    assert len(got) == len(zt.pyramid_level_shapes(v.shape, (2, 2, 2), levels))
    if expect_levels is not None:
        assert len(got) == expect_levels
    refs, cur = [], v
    for _ in got:
        cur = O.downsample(cur, dtype, (2, 2, 2), dtype, discrete=discrete)
        refs.append(cur)
    g = [from_dev(t, dtype) for t in got]
    p = [from_dev(t, dtype) for t in plain]
    assert [a.shape for a in g] == [r.shape for r in refs] == [a.shape for a in p]
    flat = lambda levels_: np.concatenate([a.reshape(-1) for a in levels_])  # noqa: E731
    assert_same_bits_nan(flat(g), flat(refs), dtype)
    assert_same_bits_nan(flat(p), flat(refs), dtype)
    return refs


# ---- 1. the N-d kernels ----

ND_CASES = [((11,), (3,)), ((7, 9), (2, 4)), ((3, 4, 5, 6), (2, 1, 2, 3)),
            ((2, 3, 4, 5, 6), (1, 2, 2, 2, 2)),
            ((2, 3, 2, 2, 3, 2, 2, 5), (1, 2, 1, 2, 1, 2, 1, 2)),  # rank 8 = ZT_MAX_DIMS
            ((5, 9), (8, 2)),  # stride 8 > extent 5: the window is min(stride, extent) = 5
            ((9, 10, 13), (2, 2, 3))]  # rank 3, but not the (2, 2, 2) window of the fast path


@pytest.mark.parametrize("shape,stride", ND_CASES)
@pytest.mark.parametrize("din,dout", [("uint16", "float32"), ("int16", "int16"),
                                      ("float32", "uint8")])
def test_nd_mean_ranks(shape, stride, din, dout):
    """downsample_continuous_kernel (launch_ds_types: not rank 3 with a (2, 2, 2) window) at
    ranks 1, 2, 3, 4, 5 and 8: the per-output and per-window index walks over p.ndim axes.
    Through apply_ndarray_continuous and through Downsample::apply into a poisoned output."""
    v = full_range(shape, din, len(shape) * 7 + stride[0])
    ref = O.downsample(v, din, stride, dout)
    assert_same_bits_nan(gpu_ds(v, din, stride, dout), ref, dout)
    assert_same_bits_nan(gpu_ds_array(v, din, stride, dout), ref, dout)


@pytest.mark.parametrize("shape,stride", ND_CASES)
@pytest.mark.parametrize("din,dout", [("uint16", "float32"), ("int16", "int16")])
def test_nd_mode_ranks(shape, stride, din, dout):
    """downsample_discrete_kernel (same dispatch, discrete; integer inputs only) at ranks 1 to
    5 and 8, on five distinct values so that windows have ties (to the smallest value) and
    majorities."""
    v = few_values(shape, din, len(shape) * 5 + stride[0])
    ref = O.downsample(v, din, stride, dout, discrete=True)
    assert_same_bits_nan(gpu_ds(v, din, stride, dout, discrete=True), ref, dout)
    assert_same_bits_nan(gpu_ds_array(v, din, stride, dout, discrete=True), ref, dout)


# ---- 2. the N-d kernels' second grid-stride trip ----

@pytest.mark.parametrize("discrete", [False, True])
def test_nd_second_grid_stride_trip(discrete):
    """launch_ds_types caps the N-d launch at 256 * 64 workgroups of 256 threads = 4 194 304
    outputs per trip; 4 194 604 outputs (1-D uint8, window 2) put 300 of them in the second
    trip of downsample_continuous_kernel / downsample_discrete_kernel."""
    n = 2 * 4194304 + 600
    v = np.random.default_rng(2).integers(0, 255, (n,), dtype=np.uint8, endpoint=True)
    ref = O.downsample(v, "uint8", (2,), "uint8", discrete=discrete)
    assert ref.shape == (4194304 + 300,)
    assert_same_bits_nan(gpu_ds_array(v, "uint8", (2,), "uint8", discrete), ref, "uint8")


# ---- 3. the per-level kernels' z loop ----

@pytest.mark.parametrize("discrete", [False, True])
def test_per_level_z_loop(discrete):
    """downsample3_kernel / downsample3_mode_kernel (rank 3, window (2, 2, 2), out_shape[1] =
    40000 <= 65535): gx * gy = 40000 workgroups per z layer, so launch_ds_types launches
    262144 / 40000 = 6 layers for 16 output slices and `z += gridDim.z` makes three trips, the
    last a partial one."""
    v = np.random.default_rng(3).integers(0, 255, (32, 80000, 4), dtype=np.uint8, endpoint=True)
    ref = O.downsample(v, "uint8", (2, 2, 2), "uint8", discrete=discrete)
    assert ref.shape == (16, 40000, 2)
    assert_same_bits_nan(gpu_ds(v, "uint8", (2, 2, 2), "uint8", discrete), ref, "uint8")


# ---- 4. the fused pyramid's z loop ----

@pytest.mark.parametrize("levels", [3, 2])
@pytest.mark.parametrize("dtype,discrete", [("uint16", False), ("uint8", False), ("uint8", True),
                                            ("int64", False), ("float32", False)])
def test_fused_pyramid_z_loop(dtype, discrete, levels):
    """pyramid3_fused_kernel<T, NL, VEC> (uint16, int64, float32) and pyramid3_u8_kernel<NL, ..>
    (uint8 mean and mode) on (1040, 12, 40): level 1 has 520 slices = 130 z blocks of 4, the
    launch (launch_pyr_fused_t) has min(130, 128) layers, so layers 0 and 1 take a second trip
    of `bz += gridDim.z`; with NL = 3 (max_levels 3) that trip writes lds2 again behind the
    loop's closing barrier, with NL = 2 (max_levels 2) there is no level 3."""
    v = full_range((1040, 12, 40), dtype, 4) if not discrete else few_values((1040, 12, 40),
                                                                             dtype, 4)
    check_pyramid(v, dtype, levels, discrete, expect_levels=levels)


# ---- 5. float values ----

def special_f(dtype="float32"):
    """(18, 20, 41) noise with, each in one aligned 2 x 2 x 2 window: eight -0.0; a NaN; +inf
    and -inf together (their f64 sum is NaN); a lone +inf; eight 3e38 (the f64 sum is finite,
    the mean is 3e38). The NaN and the inf pair share one level-3 window of the pyramid."""
    v = (np.random.default_rng(5).standard_normal((18, 20, 41)) * 1000.0).astype(np.float32)
    v[4:6, 6:8, 10:12] = -0.0
    v[0, 0, 0] = np.nan
    v[0, 0, 2] = np.inf
    v[0, 0, 3] = -np.inf
    v[10, 12, 30] = np.inf
    v[12:14, 2:4, 20:22] = 3e38
    if dtype == "float32":
        return v
    if dtype == "float64":
        return v.astype(np.float64)
    return O.cast_from_f32(v, dtype).reshape(v.shape)  # f16: 3e38 becomes +inf


@pytest.mark.parametrize("dout", list(O.DTYPES))
def test_float_values_per_level_all_outputs(dout):
    """downsample3_kernel<float, TOut, 2, 2, 2> on the special values, to all 13 output types
    (from_f64<TOut>: saturation at the integer bounds, NaN -> 0, f16 overflow to inf, -0.0
    kept by the float types because the f64 sum starts from -0.0)."""
    v = special_f()
    ref = O.downsample(v, "float32", (2, 2, 2), dout)
    if dout == "float32":
        assert (ref.view(np.uint32) == 0x80000000).any()  # the -0.0 window
        assert np.isnan(ref).any() and (ref == np.inf).any() and (ref == np.float32(3e38)).any()
    assert_same_bits_nan(gpu_ds(v, "float32", (2, 2, 2), dout), ref, dout)
    assert_same_bits_nan(gpu_ds_array(v, "float32", (2, 2, 2), dout), ref, dout)


@pytest.mark.parametrize("stride", [(1, 1, 2), (3, 2, 4)])
@pytest.mark.parametrize("dout", ["int8", "uint16", "int64", "float16", "bfloat16", "float32"])
def test_float_values_nd_kernel(stride, dout):
    """downsample_continuous_kernel<float, TOut> (rank 3 but not the (2, 2, 2) window) on the
    special values."""
    v = special_f()
    ref = O.downsample(v, "float32", stride, dout)
    assert_same_bits_nan(gpu_ds_array(v, "float32", stride, dout), ref, dout)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_float_values_fused_pyramid(dtype):
    """pyramid3_fused_kernel<float / double, 3, VEC = false> (launch_pyr_fused_t: the x extent 41
    is no multiple of 8, so rows are read element by element and padded with 0 past the edge):
    pyr_mean8's f64 sum from -0.0. Level 1 holds a -0.0 (a sum from +0.0 gives +0.0)."""
    v = special_f(dtype)
    refs = check_pyramid(v, dtype, 3, expect_levels=3)
    l1 = refs[0]
    assert (l1.view(f"u{l1.itemsize}") == (1 << (8 * l1.itemsize - 1))).any()
    assert np.isnan(l1).any() and np.isinf(l1).any()


@pytest.mark.parametrize("din", ["float16", "bfloat16"])
@pytest.mark.parametrize("dout", ["float32", "uint8"])
def test_half_inputs_special_values(din, dout):
    """downsample3_kernel<f16_t / bf16_t, TOut, 2, 2, 2>: Elem<T>::to_f64 of NaN, +-inf, -0.0
    and (bf16) 3e38."""
    v = special_f(din)
    ref = O.downsample(v, din, (2, 2, 2), dout)
    assert_same_bits_nan(gpu_ds(v, din, (2, 2, 2), dout), ref, dout)


# ---- 6. integer extremes in mean mode ----

def small_sum_windows(v):
    """Aligned 2 x 2 x 2 windows of v that sum to -7 .. -1 and +1 .. +7 (k elements of -1 or +1,
    the rest 0): the mean truncates toward zero to 0, a flooring quotient gives -1 for the
    negative sums. Unsigned types get the positive sums only."""
    signs = (1, -1) if np.iinfo(v.dtype).min < 0 else (1,)
    i = 0
    for sign in signs:
        for k in range(1, 8):
            z, y, x = 2 * (i % 4), 2 * (i // 4), 4
            w = np.zeros(8, dtype=v.dtype)
            w[:k] = sign
            v[z:z + 2, y:y + 2, x:x + 2] = np.roll(w, i).reshape(2, 2, 2)
            i += 1
    return v


def extreme_ints(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == "uint64":
        pool = np.array([2 ** 64 - 1, 2 ** 63, 2 ** 63 + 1, 2 ** 53 + 1, 0], dtype=np.uint64)
        v = pool[rng.integers(0, 5, shape)]
        v[2:6, 4:8, 8:16] = 2 ** 64 - 1  # whole windows of the maximum: the f64 mean is 2^64
        return v
    if dtype == "int64":
        ii = np.iinfo(np.int64)
        pool = np.array([ii.min, ii.max, -1, 2 ** 53 + 1, -(2 ** 53 + 1)], dtype=np.int64)
        v = pool[rng.integers(0, 5, shape)]
        v[2:4, 4:6, 8:12] = ii.max
        v[4:6, 4:6, 8:12] = ii.min
        return v
    return small_sum_windows(full_range(shape, dtype, seed))


@pytest.mark.parametrize("shape", [(18, 20, 40), (16, 16, 64)])
@pytest.mark.parametrize("dtype", ["uint64", "int64", "int32", "int16", "int8"])
def test_integer_extremes_mean(shape, dtype):
    """Mean of extreme integers through downsample3_kernel (f64 sum, from_f64 saturating: eight
    2^64 - 1 average to 2^64 in f64 and must give 2^64 - 1) and through the fused pyramid:
    pyramid3_fused_kernel's pyr_mean8 (the f64 path for the 64-bit types; for int32 / int16
    the integer sum of kPyrIntSum, whose quotient must truncate toward zero like `as`), and
    pyramid3_u8_kernel's v_dot4_i32_i8 path for int8. (18, 20, 40) is the non-VEC form for
    int8 (40 % 16 != 0) and VEC for the others; (16, 16, 64) is VEC for all."""
    v = extreme_ints(shape, dtype, shape[0])
    ref = O.downsample(v, dtype, (2, 2, 2), dtype)
    if dtype == "uint64":
        assert (ref == np.uint64(2 ** 64 - 1)).any()
    if dtype in ("int32", "int16", "int8"):
        s = v[:8, :8, 4:6].astype(np.int64).reshape(4, 2, 4, 2, 2).sum(axis=(1, 3, 4))
        assert set(range(-7, 8)) - {0} <= set(s.ravel().tolist())
        assert all(ref[i % 4, i // 4, 2] == 0 for i in range(14))
    assert_same_bits_nan(gpu_ds(v, dtype, (2, 2, 2), dtype), ref, dtype)
    assert_same_bits_nan(gpu_ds_array(v, dtype, (2, 2, 2), dtype), ref, dtype)
    check_pyramid(v, dtype, 3, expect_levels=3)
    # the same values through downsample_continuous_kernel (another window: the N-d kernel)
    assert_same_bits_nan(gpu_ds_array(v, dtype, (1, 2, 4), dtype),
                         O.downsample(v, dtype, (1, 2, 4), dtype), dtype)
