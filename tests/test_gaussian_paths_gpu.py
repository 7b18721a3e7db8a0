"""GPU parity of the Gaussian launch forms that tests/test_gaussian_gpu.py does not reach, against
the oracle, bit for bit (gaussian.hip follows the reference's f32 operation order).

How run_gaussian (zt_api.hip) dispatches a call, by L = 2 * kernel_half_size + 1 per axis (a
sigma of 0 gives L = 1):
  * ndim >= 3 and the last three axes share one L in 3..13: the z/y/x march (launch_gaussian_zyx),
    earlier axes through launch_gaussian_pass first;
  * else, both of the last two axes with L <= kGaussYXMaxLen (33): launch_gaussian_yx, which
    takes gauss_yx_fast_kernel<L> for f32 input and one L in {3, 5, .., 13} on both axes and
    gauss_yx_kernel<T> otherwise; earlier axes through launch_gaussian_pass;
  * else one launch_gaussian_pass per axis: gauss_row_kernel for the last axis (inner == 1),
    gauss_col_kernel while kGaussSeg + L - 1 <= kGaussColMaxWin (L <= 49), gauss_pass_kernel
    beyond.

Every output is written into a poisoned buffer (tests/gpu_util.poisoned), so an element no
kernel writes fails; NaNs compare by position only, through assert_same_bits_nan and its 2 % cap.
"""
import itertools

import numpy as np
import pytest

from oracle import oracle as O
from tests.gpu_util import assert_same_bits_nan, from_dev, poisoned, to_dev, type_extremes

pytestmark = pytest.mark.gpu

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)

NEG_ZERO_BITS = 0x80000000


def noise(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.random(shape, dtype=np.float32) * 1000 - 200).astype(np.float32)


def typed_noise(shape, din, seed):
    """Values of din (storage) and their f32 images, as test_gaussian_gpu.test_all_input_types."""
    rng = np.random.default_rng(seed)
    v32 = rng.random(shape, dtype=np.float32) * 200 - (50 if din.startswith("int") else 0)
    v = O.cast_from_f32(v32.astype(np.float32), din)
    return v, O.cast_to_f32(v, din).reshape(shape)


def gpu_apply(v, din, dout, chunk, sigma, half):
    """Gaussian::apply on the whole array (zt_gaussian_apply_array), into a poisoned output."""
    import torch
    y = poisoned(v.shape, dout)
    zt.Gaussian(sigma, half).apply(zt.DeviceArray(to_dev(v, din), chunk, din),
                                   zt.DeviceArray(y, chunk, dout))
    torch.cuda.synchronize()
    return from_dev(y, dout)


def gpu_apply_chunks(v, din, chunk, sigma, half):
    """Chunk by chunk (zt_gaussian_apply_ndarray on each chunk's halo'd block: output regions
    that start at the halo, not at 0), f32 output, into a poisoned output."""
    import torch
    y = poisoned(v.shape, "float32")
    a_in, a_out = zt.DeviceArray(to_dev(v, din), chunk, din), zt.DeviceArray(y, chunk)
    g = zt.Gaussian(sigma, half)
    for idx in itertools.product(*[range(n) for n in a_out.chunk_grid_shape()]):
        g.apply_chunk(a_in, a_out, idx)
    torch.cuda.synchronize()
    return from_dev(y, "float32")


def check(v32, v, din, chunk, sigma, half, chunks_too=False):
    ref = O.gaussian_apply(v32, chunk, sigma, half)
    assert_same_bits_nan(gpu_apply(v, din, "float32", chunk, sigma, half), ref, "float32")
    if chunks_too:
        assert_same_bits_nan(gpu_apply_chunks(v, din, chunk, sigma, half), ref, "float32")
    return ref


# ---- 1. gauss_yx_fast_kernel<L> ----

@pytest.mark.parametrize("half", [1, 2, 3, 4, 5, 6])
def test_yx_fast_tiles_and_region_origins(half):
    """gauss_yx_fast_kernel<L>, L = 3..13 (gaussian.hip try_gauss_yx_fast: f32 input and
    py.len == px.len == L; reached from run_gaussian's fuse_yx branch as ndim == 2 < 3).
    (70, 150) over 32 x 64 tiles: 3 x 3 workgroups with partial last tiles on both axes; chunk
    by chunk the output regions start at o0 = (half, half) inside their halo'd blocks."""
    v = noise((70, 150), 100 + half)
    sigma = [0.7 + 0.3 * half, 0.5 + 0.35 * half]
    check(v, v, "float32", (32, 64), sigma, [half, half], chunks_too=True)


@pytest.mark.parametrize("half", [1, 6])
def test_yx_fast_odd_row_length(half):
    """gauss_yx_fast_kernel<3> / <13> (same dispatch) on rows of 149 elements: the 16-byte
    alignment of a row's quads alternates from row to row, so the float4 store and the scalar
    branch both run, and the last quad of every row is partial (c0 + 4 > hx)."""
    v = noise((45, 149), 7 + half)
    check(v, v, "float32", (45, 149), [1.1, 0.9 + 0.2 * half], [half, half])


def test_yx_fast_plane_loop_behind_a_column_pass():
    """sigma 0 on axis 0 gives L = (1, 5, 5): not one L on the last three axes, so no march;
    run_gaussian's fuse_yx branch runs axis 0 through launch_gaussian_pass (gauss_col_kernel,
    L = 1) and the 9 planes through gauss_yx_fast_kernel<5>, whose `o` loop re-uses tile and
    ybuf behind its barrier. The launch has one z layer per plane; the loop's second trip is
    test_grid_cap_yx_fast_outer's."""
    v = noise((9, 40, 70), 21)
    check(v, v, "float32", (9, 40, 70), [0.0, 1.0, 1.0], [0, 2, 2])


# ---- 2. gauss_yx_kernel<T> ----

@pytest.mark.parametrize("din", ["uint8", "int16", "uint16", "float16", "bfloat16", "float64"])
def test_yx_generic_input_types(din):
    """gauss_yx_kernel<T> for T != float (launch_gaussian_yx: try_gauss_yx_fast declines every
    dtype_in != kF32): 2-D, L = 5 on both axes, 3 x 2 tiles with partial last ones, whole array
    and chunk by chunk."""
    v, v32 = typed_noise((33, 70), din, 3)
    check(v32, v, din, (16, 32), [1.0, 1.2], [2, 2], chunks_too=True)


@pytest.mark.parametrize("din", ["int32", "uint32", "int64", "uint64", "float64"])
def test_input_type_extremes(din):
    """Elem<T>::to_f32 at the extremes of the wide types, where the conversion rounds or
    overflows: through gauss_yx_kernel<T> (2-D, L = 5) and through the march's 4- and 8-byte
    buffer loads (gauss_zyx_kernel<3, T, false>: 3-D, L = 3, int32 / uint32 / 64-bit types have
    no quad form in launch_zyx_cfg)."""
    v = type_extremes((33, 70), din, 17)
    v32 = O.cast_to_f32(v, din).reshape(v.shape)
    ref = check(v32, v, din, (16, 32), [1.0, 1.2], [2, 2])
    if din == "float64":
        assert (ref == np.inf).any() and (ref == -np.inf).any() and not np.isnan(ref).any()
    v = type_extremes((6, 11, 40), din, 18)
    v32 = O.cast_to_f32(v, din).reshape(v.shape)
    check(v32, v, din, (6, 11, 40), [0.6, 0.6, 0.6], [1, 1, 1])


def test_yx_generic_largest_beside_smallest_len():
    """gauss_yx_kernel<float> (f32 but py.len 33 != px.len 3, and 33 is no fast L): the largest
    fused L (kGaussYXMaxLen) beside the smallest, 2 x 5 tiles."""
    v = noise((45, 300), 33)
    check(v, v, "float32", (45, 300), [5.0, 0.6], [16, 1], chunks_too=False)
    check(v, v, "float32", (20, 128), [5.0, 0.6], [16, 1], chunks_too=True)


# ---- 3. one pass per axis ----

def test_row_kernel_tiles_and_lines():
    """gauss_row_kernel (launch_gaussian_pass: p.inner == 1), reached because L = 41 on the last
    axis exceeds kGaussYXMaxLen so run_gaussian's fuse_yx is false: three lines (the `o` loop's
    grid has one layer each), tiles of 1024, 1024 and 52 outputs, the last one's window clamped
    at the row's end. Axis 0 (L = 1) goes through gauss_col_kernel."""
    v = noise((3, 2100), 5)
    check(v, v, "float32", (3, 2100), [0.0, 7.0], [0, 20])
    check(v, v, "float32", (2, 1000), [0.0, 7.0], [0, 20], chunks_too=True)


@pytest.mark.parametrize("din", ["float32", "uint16", "int8", "float64"])
def test_separate_passes_long_kernels(din):
    """L = (61, 41, 35): no march (L > 13), no fused y/x pass (L > 33). launch_gaussian_pass
    sends axis 0 to gauss_pass_kernel<T, false> (kGaussSeg + 61 - 1 > kGaussColMaxWin; it reads
    din), axis 1 to gauss_col_kernel (16 + 41 - 1 = 56 window rows, seven batches of 8) and
    axis 2 to gauss_row_kernel."""
    v, v32 = typed_noise((60, 40, 33), din, 9)
    check(v32, v, din, (60, 40, 33), [9.0, 5.0, 6.0], [30, 20, 17])


def test_separate_passes_chunk_regions():
    """The same three kernels chunk by chunk: output regions inside halo'd blocks (o0 != 0, on
    < n on every axis, so each pass keeps the whole block on later axes only)."""
    v = noise((60, 40, 33), 10)
    check(v, v, "float32", (32, 24, 20), [9.0, 5.0, 6.0], [30, 20, 17], chunks_too=True)


def test_largest_half_on_an_axis_shorter_than_the_kernel():
    """kernel_half_size 127 (L = 255 = kGaussMaxTaps, the largest gaussian_args_ok accepts) on
    an axis of 5 elements: gauss_pass_kernel<float, false> with all but a few taps clamped to
    the ends; axis 1 (L = 5) through gauss_row_kernel."""
    v = noise((5, 40), 11)
    check(v, v, "float32", (5, 40), [40.0, 1.0], [127, 2])


# ---- 4. grid caps ----

def test_grid_cap_col_and_row_kernels():
    """More than 65535 rows: rows_grid (gaussian.hip) caps gridDim.y at 65535 and adds z layers.
    (66000, 2, 8) with L = (1, 1, 35) takes one pass per axis (35 > kGaussYXMaxLen): axis 1 is
    gauss_col_kernel over 66000 (outer, segment) rows, axis 2 gauss_row_kernel over 132000
    lines; both use blockIdx.z * gridDim.y + blockIdx.y with gridDim.z = 2 and 3."""
    v = noise((66000, 2, 8), 12)
    check(v, v, "float32", (66000, 2, 8), [0.0, 0.0, 6.0], [0, 0, 17])


def test_grid_cap_pass_kernel():
    """gauss_pass_kernel<float, false> over outer * on = 1100 * 61 = 67100 > 65535 rows
    (rows_grid: two z layers): axis 1 with L = 61; axes 0 and 2 have L = 1."""
    v = noise((1100, 61, 4), 13)
    check(v, v, "float32", (1100, 61, 4), [0.0, 9.0, 0.0], [0, 30, 0])


def test_grid_cap_yx_fast_outer():
    """gauss_yx_fast_kernel<3> with outer = 66000 planes (launch_gaussian_yx: gridDim.z =
    min(outer, 65535)): planes 65535.. are the second trip of the kernel's `o` loop."""
    v = noise((66000, 3, 8), 14)
    check(v, v, "float32", (66000, 3, 8), [0.0, 0.6, 0.6], [0, 1, 1])


def test_grid_cap_yx_generic_outer():
    """gauss_yx_kernel<float> (L = (3, 5): no single L) with outer = 66000 planes: the second
    trip of its `o` loop."""
    v = noise((66000, 3, 8), 15)
    check(v, v, "float32", (66000, 3, 8), [0.0, 0.6, 1.0], [0, 1, 2])


def test_grid_cap_march_outer():
    """The z/y/x march with outer = 66000 volumes (launch_zyx_cfg: gridDim.y = min(outer,
    65535)): 4-D, L = 3 on every axis, so axis 0 runs through gauss_col_kernel first and
    gauss_zyx_kernel<3, float, QUAD> marches 66000 volumes of 3 x 3 x 8, the last 465 in the
    second trip of its `o` loop."""
    v = noise((66000, 3, 3, 8), 16)
    check(v, v, "float32", (66000, 3, 3, 8), [0.6] * 4, [1] * 4)


# ---- 5. / 6. values ----

def special_3d(shape, seed=40):
    """Noise with a NaN, a +inf and a -inf whose windows meet (inf - inf = NaN in the sums), a
    lone -inf, a run of -0.0 and two neighbouring 3e38. Positions as in the (12, 20, 72) input;
    z moves to the last slice where the array is shallower."""
    v = noise(shape, seed)
    nz = shape[0]
    v[3, 6, 12] = np.nan
    v[1, 2, 3] = np.inf
    v[1, 2, 6] = -np.inf
    v[min(9, nz - 1), 15, 60] = -np.inf
    v[6, 10, 30:40] = -0.0
    v[min(10, nz - 1), 3, 50:52] = 3e38
    return v


def special_2d(shape, seed=41):
    v = noise(shape, seed)
    v[30, 60] = np.nan
    v[5, 5] = np.inf
    v[5, 8] = -np.inf
    v[60, 140] = -np.inf
    v[40, 100:102] = 3e38
    return v


def assert_has_specials(ref):
    assert np.isnan(ref).any() and (ref == np.inf).any() and (ref == -np.inf).any()


# the paths: special input, chunk, sigma, half
def path_narrow_march():
    # sigma 0.35 on z: the centre tap is 1.14, so 3e38 * tap overflows to +inf in one product
    return special_3d((12, 20, 72)), (12, 20, 72), [0.35, 1.0, 1.2], [2, 2, 2]


def path_dma_march():
    return special_3d((9, 37, 264)), (9, 37, 264), [1.0, 1.3, 0.9], [3, 3, 3]


def path_yx_fast():
    return special_2d((70, 150)), (32, 64), [1.0, 1.2], [2, 2]


def path_separate():
    # The (70, 150) pattern at the same positions in a (280, 600) array: with L = 41 the NaN's
    # window alone is 41 x 41 elements, 16 % of (70, 150) and past the helper's 2 % cap; in
    # (280, 600) the reference is 1.4 % NaN (1681 from the NaN, 676 where the infinities meet).
    # The -inf's window covers the whole window of the +inf three columns away, so no +inf
    # survives there; a second +inf far from everything keeps one in the reference.
    v = special_2d((280, 600))
    v[200, 400] = np.inf
    return v, (280, 600), [7.0, 7.0], [20, 20]


def path_yx_generic():
    return special_2d((70, 150)), (32, 64), [0.6, 1.0], [1, 2]


def path_long_pass():
    # the same (280, 600) array, L = (61, 5): 305 NaNs from the NaN, 72 where the infinities meet
    return special_2d((280, 600)), (280, 600), [9.0, 1.0], [30, 2]


PATHS = {"narrow_march": path_narrow_march, "dma_march": path_dma_march,
         "yx_fast": path_yx_fast, "separate_passes": path_separate,
         "yx_generic": path_yx_generic, "long_pass": path_long_pass}


@pytest.mark.parametrize("path", list(PATHS))
def test_non_finite_values(path):
    """NaN, +-inf, inf - inf, -0.0 and 3e38 through: gauss_zyx_kernel<5, float, QUAD> (3-D, one
    L = 5, x extent 72 < ZYXWide::TX so launch_zyx_l picks the narrow tiles);
    gauss_zyx_dma_kernel<7> (x extent 264 >= 256, a multiple of 4, f32, L <= 7);
    gauss_yx_fast_kernel<5> (2-D, whole array and chunk by chunk); gauss_col_kernel and
    gauss_row_kernel with L = 41 (2-D, L > kGaussYXMaxLen); gauss_yx_kernel<float> (2-D, L =
    (3, 5): no single L); gauss_pass_kernel<float, false> (L = 61 on axis 0: kGaussSeg + L - 1 >
    kGaussColMaxWin) before a row pass with L = 5. The reference holds all three kinds of
    non-finite value; NaNs by position, everything else by bits."""
    v, chunk, sigma, half = PATHS[path]()
    ref = check(v, v, "float32", chunk, sigma, half,
                chunks_too=path in ("yx_fast", "yx_generic"))
    assert_has_specials(ref)


@pytest.mark.parametrize("path", list(PATHS))
def test_all_negative_zero(path):
    """Every kernel starts its sums from -0.0 (Iterator::sum::<f32>): an array of -0.0 stays
    -0.0 in every element, bit for bit, where a sum started from +0.0 gives +0.0. Same six
    paths and kernels as test_non_finite_values."""
    v, chunk, sigma, half = PATHS[path]()
    z = np.full(v.shape, -0.0, dtype=np.float32)
    ref = O.gaussian_apply(z, chunk, sigma, half)
    assert (ref.view(np.uint32) == NEG_ZERO_BITS).all()
    out = gpu_apply(z, "float32", "float32", chunk, sigma, half)
    assert (out.view(np.uint32) == NEG_ZERO_BITS).all(), \
        f"first +0.0 / other value at {tuple(np.argwhere(out.view(np.uint32) != NEG_ZERO_BITS)[0])}"


# ---- 7. output casts ----

@pytest.fixture(scope="module")
def special_3d_result():
    v, chunk, sigma, half = path_narrow_march()
    ref = O.gaussian_apply(v, chunk, sigma, half)
    assert_has_specials(ref)
    ref.setflags(write=False)
    return v, chunk, sigma, half, ref


@pytest.mark.parametrize("dout", list(O.DTYPES))
def test_output_casts_of_non_finite_values(dout, special_3d_result):
    """launch_cast_from_f32_3d (cast.hip) behind the march (run_gaussian: cast_out = dtype_out !=
    kF32, the march writes scratch and the cast writes the output): NaN -> 0, saturation at the
    integer bounds, +-inf and the f16 overflow, for all 13 output types. Where the f32 result is
    NaN the float outputs (f16, bf16, f32, f64) are NaN too and compare by NaN-ness alone."""
    v, chunk, sigma, half, ref = special_3d_result
    want = O.cast_from_f32(ref, dout).reshape(ref.shape)
    out = gpu_apply(v, "float32", dout, chunk, sigma, half)
    assert_same_bits_nan(out, want, dout)
