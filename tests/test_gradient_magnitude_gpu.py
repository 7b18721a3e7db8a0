"""GPU parity of the gradient magnitude (gradient.hip through the C ABI) against the numpy
restatement of the reference (tests/gm_ref.py): bit-exact, as the kernels perform the reference's
f32 operations in its order (gradient_magnitude.rs:109-147, kernel.rs:75-129)."""
import itertools
import json

import numpy as np
import pytest

from oracle import oracle as O
from tests import gm_ref as R
from tests.gpu_util import from_dev, to_dev
from tests.test_gradient_magnitude import KAT_IN, KAT_OUT

pytestmark = pytest.mark.gpu

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)
from zarrs_tools_amd import store as S  # noqa: E402

OPERATORS = ["sobel", "central_difference"]


def gpu_gm(v, din, dout, chunk, operator="sobel"):
    import torch
    x = to_dev(v, din)
    y = torch.empty(v.shape, dtype=zt.torch_dtype(dout), device="cuda")
    zt.GradientMagnitude(operator).apply(zt.DeviceArray(x, chunk, din),
                                         zt.DeviceArray(y, chunk, dout))
    torch.cuda.synchronize()
    return from_dev(y, dout)


def gpu_gm_block(v, start, shape, operator="sobel"):
    import torch
    out = zt.GradientMagnitude(operator).apply_ndarray(to_dev(v, "float32"),
                                                       zt.ArraySubset(start, shape), "float32")
    torch.cuda.synchronize()
    return from_dev(out, "float32")


def assert_same_bits(out, ref):
    """Equal bytes; for f32 with NaNs: the same NaN positions, equal bytes elsewhere (the sign
    of a generated NaN differs between x86 and the GPU)."""
    assert out.shape == ref.shape and out.dtype == ref.dtype
    if out.dtype == np.float32:
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(out), nan)
        assert np.array_equal(out[~nan].view(np.uint8), ref[~nan].view(np.uint8))
    else:
        assert np.array_equal(np.ascontiguousarray(out).view(np.uint8),
                              np.ascontiguousarray(ref).view(np.uint8))


def noise(shape, seed=0):
    rng = np.random.default_rng(sum(shape) + seed)
    return (rng.random(shape, dtype=np.float32) * 1000 - 200).astype(np.float32)


def test_reference_kat_bit_exact():
    out = gpu_gm(KAT_IN, "float32", "float32", (2, 2))
    assert np.array_equal(out, KAT_OUT)


# The fused 3-D Sobel march (gm_sobel3_kernel, 32 x 64 tiles): unit extents on each axis (a
# triangle pass along a unit axis still rounds), extent 2, x below a tile and no multiple of 4
# (element-wise staging), the aligned quad staging across tile borders in y and x, a ragged last
# tile, and 101 output slices: 4 z segments of 26 (the last one 23), each priming its own ring.
@pytest.mark.parametrize("shape", [
    (1, 5, 9), (5, 1, 9), (5, 9, 1), (1, 1, 1), (2, 2, 2), (7, 33, 67),
    (9, 40, 128), (5, 70, 132), (5, 70, 131), (101, 9, 20),
])
def test_fused_sobel_3d_bit_exact(shape):
    v = noise(shape)
    out = gpu_gm(v, "float32", "float32", shape)
    assert_same_bits(out, R.apply_ndarray(v))


# An interior output region of a block: misaligned (element-wise staging from x = 0) and aligned
# to quads (x origin 8).
@pytest.mark.parametrize("block,start,shape", [
    ((10, 20, 41), (1, 1, 1), (8, 18, 39)),
    ((6, 24, 72), (0, 4, 8), (6, 16, 64)),
])
def test_apply_ndarray_interior_subset(block, start, shape):
    v = noise(block)
    ref = R.apply_ndarray(v)[tuple(slice(s, s + n) for s, n in zip(start, shape))]
    assert_same_bits(gpu_gm_block(v, start, shape), ref)


def test_per_chunk_path_equals_apply():
    import torch
    v = O.synth_step_noise_f32((14, 30, 50))
    chunk = (5, 16, 20)
    x = to_dev(v, "float32")
    y = torch.empty(v.shape, device="cuda")
    a_in, a_out = zt.DeviceArray(x, chunk), zt.DeviceArray(y, chunk)
    g = zt.GradientMagnitude()
    for idx in itertools.product(*[range(n) for n in a_out.chunk_grid_shape()]):
        g.apply_chunk(a_in, a_out, idx)
    torch.cuda.synchronize()
    whole = gpu_gm(v, "float32", "float32", chunk)
    assert_same_bits(from_dev(y, "float32"), whole)
    assert_same_bits(whole, R.apply_chunks(v, chunk))


# The generic pass-by-pass path: every rank but 3, and CentralDifference at any rank.
@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("shape,chunk", [
    ((300,), (64,)),
    ((33, 70), (16, 32)),
    ((6, 7, 8, 9), (3, 4, 4, 5)),
    ((3, 4, 3, 5, 6), (2, 2, 3, 3, 4)),
])
def test_generic_path_bit_exact(shape, chunk, operator):
    v = noise(shape)
    out = gpu_gm(v, "float32", "float32", chunk, operator)
    assert_same_bits(out, R.apply_ndarray(v, operator))


def test_central_difference_3d():
    v = noise((7, 33, 67))
    out = gpu_gm(v, "float32", "float32", (4, 16, 32), "central_difference")
    assert_same_bits(out, R.apply_ndarray(v, "central_difference"))
    # an interior region through the generic finishing kernel
    ref = R.apply_ndarray(v, "central_difference")[1:6, 2:30, 3:60]
    got = gpu_gm_block(v, (1, 2, 3), (5, 28, 57), "central_difference")
    assert_same_bits(got, ref)


@pytest.mark.parametrize("din", list(O.DTYPES))
def test_all_input_types(din):
    rng = np.random.default_rng(3)
    v32 = rng.random((6, 11, 40), dtype=np.float32) * 200 - (50 if din.startswith("int") else 0)
    v = O.cast_from_f32(v32, din)
    if din.startswith("int"):
        assert (O.cast_to_f32(v, din) < 0).any()
    out = gpu_gm(v, din, "float32", (4, 8, 16))
    assert_same_bits(out, R.apply_whole(v, "sobel", din, "float32"))


@pytest.mark.parametrize("dout", list(O.DTYPES))
def test_all_output_types(dout):
    rng = np.random.default_rng(4)
    v = (rng.random((6, 11, 40), dtype=np.float32) * 4000 - 1000).astype(np.float32)
    ref32 = R.apply_ndarray(v)
    assert ref32.max() > 256  # the 8-bit types saturate
    out = gpu_gm(v, "float32", dout, (4, 8, 16))
    assert_same_bits(out, O.cast_from_f32(ref32, dout))


@pytest.mark.parametrize("operator", OPERATORS)
def test_special_values(operator):
    rng = np.random.default_rng(9)
    v = (rng.random((8, 12, 40), dtype=np.float32) * 10).astype(np.float32)
    v[1, 2, 3] = np.inf
    v[5, 9, 6] = -np.inf
    v[3, 6, 12] = np.nan
    v[6, 3, 16] = 3e38   # s * s overflows to inf
    v[2, 8, 17] = -3e38
    tiny = np.finfo(np.float32).tiny
    v[:, :, 20:30] *= np.float32(1e-39)  # subnormal inputs and pass results (preserved)
    v[:, :, 30:] *= np.float32(3e-21)    # normal s, subnormal s * s and g
    assert (np.abs(v[:, :, 20:30]) < tiny).all()
    ref = R.apply_ndarray(v, operator)
    assert np.isnan(ref).any() and np.isinf(ref).any()
    sub = ref[:, :, 32:]
    assert (sub > 0).any() and (sub * sub < tiny).all()
    out = gpu_gm(v, "float32", "float32", v.shape, operator)
    assert_same_bits(out, ref)


def test_store_gradient_magnitude(tmp_path):
    shape, chunk = (20, 33, 70), (8, 16, 32)
    u = O.synth_u16(shape)
    S.create_array(tmp_path / "in.zarr", "uint16", shape, chunk, S.codecs_json("gzip"))
    S.write_array(tmp_path / "in.zarr", u)
    st = S.gradient_magnitude(tmp_path / "in.zarr", tmp_path / "out.zarr", data_type="float32")
    ref = R.apply_whole(u, "sobel", "uint16", "float32")
    whole = S.read_array(tmp_path / "out.zarr")
    assert whole.dtype == np.float32
    assert_same_bits(whole, ref)
    assert st["voxels"] == u.size
    # two "ranks": chunk rows [0, 1) and [1, 3), the second one finishes the metadata
    S.gradient_magnitude(tmp_path / "in.zarr", tmp_path / "rows.zarr", data_type="float32",
                         rows=(0, 1), finish=False)
    assert not (tmp_path / "rows.zarr" / "zarr.json").exists()  # "not finished" marker
    S.gradient_magnitude(tmp_path / "in.zarr", tmp_path / "rows.zarr", data_type="float32",
                         rows=(1, 3), erase=False)
    meta = json.load(open(tmp_path / "rows.zarr" / "zarr.json"))
    assert meta["data_type"] == "float32" and meta["shape"] == list(shape)
    assert_same_bits(S.read_array(tmp_path / "rows.zarr"), ref)
