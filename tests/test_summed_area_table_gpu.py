"""GPU parity of the summed-area table (sat.hip through the C ABI, the store path and the
zarrs_filter command) against the numpy restatement of the reference (tests/sat_ref.py):
bit-exact for every type, as each lane is folded left to right in the output type with one
rounding per add (summed_area_table.rs:47-106).

Borders of the kernels (zt_kernels.hpp, sat.hip): the x scan (inner == 1) gives a workgroup of
T = kSatThreads = 256 threads R = kSatRows = 256 rows and marches along x in tiles of
W = kSatTileW = 32 columns (W = kSatTileW8 = 16 for 8-byte output types); the strided scan
(inner > 1) gives a workgroup T = 256 consecutive lanes and walks the axis 8 elements at a time.
"""
import json

import numpy as np
import pytest

from oracle import oracle as O
from tests import sat_ref as R
from tests.gpu_util import from_dev, to_dev
from tests.test_summed_area_table import KAT_IN, KAT_OUT

pytestmark = pytest.mark.gpu

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)
from zarrs_tools_amd import store as S  # noqa: E402
from zarrs_tools_amd import zarrs_filter as ZF  # noqa: E402

T, ROWS = 256, 256
TILE_W = {"float32": 32, "int64": 16}   # by output type
PAIRS = [("float32", "float32"), ("uint16", "int64")]
FLOATS = ("float16", "bfloat16", "float32", "float64")


def prefill(shape, dout):
    """An output buffer that no result equals by accident: NaN, or the integer type's maximum."""
    import torch
    st = O.NP_STORAGE[dout]
    if dout in ("float16", "bfloat16"):
        fill = np.full(shape, 0x7FFF, dtype=np.uint16)
    elif dout in FLOATS:
        fill = np.full(shape, np.nan, dtype=st)
    else:
        fill = np.full(shape, np.iinfo(st).max, dtype=st)
    return to_dev(fill, dout) if fill.size else torch.empty(shape, dtype=zt.torch_dtype(dout),
                                                            device="cuda")


def gpu_sat(v, din, dout, chunk=None):
    import torch
    x = to_dev(v, din)
    y = prefill(v.shape, dout)
    chunk = chunk or tuple(max(1, n) for n in v.shape)
    zt.SummedAreaTable().apply(zt.DeviceArray(x, chunk, din), zt.DeviceArray(y, chunk, dout))
    torch.cuda.synchronize()
    return from_dev(y, dout)


def _as_float(a, dt):
    if dt == "float16":
        return a.view(np.float16).astype(np.float32)
    if dt == "bfloat16":
        return O.cast_to_f32(a, dt).reshape(a.shape)
    return a


def assert_same_bits(out, ref, dt):
    """Equal bytes; for float types with NaNs: the same NaN positions, equal bytes elsewhere (the
    sign and payload of a generated NaN differ between x86 and the GPU)."""
    assert out.shape == ref.shape and out.dtype == ref.dtype
    if dt in FLOATS:
        nan = np.isnan(_as_float(ref, dt))
        assert np.array_equal(np.isnan(_as_float(out, dt)), nan)
        out, ref = out[~nan], ref[~nan]
    assert np.array_equal(np.ascontiguousarray(out).view(np.uint8),
                          np.ascontiguousarray(ref).view(np.uint8))


def values(shape, din, seed=0):
    """f32 noise in [-200, 800) (f32 sums round from a few elements on), u16 noise for uint16."""
    rng = np.random.default_rng(sum(shape) + seed)
    if din == "uint16":
        return rng.integers(0, 65536, size=shape, dtype=np.uint16)
    return (rng.random(shape, dtype=np.float32) * 1000 - 200).astype(np.float32)


def check(shape, din, dout, chunk=None):
    v = values(shape, din)
    assert_same_bits(gpu_sat(v, din, dout, chunk), R.sat(v, din, dout), dout)


def test_reference_kat():
    out = gpu_sat(KAT_IN, "uint8", "uint16", (2, 2))
    assert np.array_equal(out, KAT_OUT)


# The x scan's tile and band borders on 2-D arrays (rows, nx): nx of 1, one short of a tile, a
# tile, one over, and two tiles and a ragged third; 1 row, one short of a band, and one over
# (a second workgroup with one row). The axis-0 scan of the same arrays is the strided kernel
# with inner = nx and n = rows.
@pytest.mark.parametrize("din,dout", PAIRS)
@pytest.mark.parametrize("k", range(5))
def test_x_scan_tile_and_band_borders(din, dout, k):
    w = TILE_W[dout]
    nx = [1, w - 1, w, w + 1, 2 * w + 3][k]
    for rows in (1, ROWS - 1, ROWS + 1):
        check((rows, nx), din, dout)


# The strided scan: inner of 1 (the x kernel, in place, on a middle axis), 2, one short of a
# workgroup's lanes and one over; n = 19 is two unrolled steps of 8 and a tail of 3.
@pytest.mark.parametrize("din,dout", PAIRS)
@pytest.mark.parametrize("inner", [1, 2, T - 1, T + 1])
def test_strided_scan_borders(din, dout, inner):
    check((3, 19, inner), din, dout)


@pytest.mark.parametrize("din,dout", PAIRS)
@pytest.mark.parametrize("shape", [
    (1, 5, 9), (5, 1, 9), (5, 9, 1), (1, 1, 1), (2, 2, 1000), (1000, 2, 2),
])
def test_unit_extents_and_long_thin(din, dout, shape):
    check(shape, din, dout)


@pytest.mark.parametrize("din,dout", PAIRS)
@pytest.mark.parametrize("shape,chunk", [
    ((300,), (64,)),
    ((33, 70), (16, 32)),
    ((6, 7, 8, 9), (3, 4, 4, 5)),
    ((3, 4, 3, 5, 6), (2, 2, 3, 3, 4)),
])
def test_ranks(din, dout, shape, chunk):
    check(shape, din, dout, chunk)


def test_zero_extent_is_a_no_op():
    import torch
    x = torch.empty((4, 0, 5), dtype=torch.float32, device="cuda")
    out = zt.SummedAreaTable().apply_ndarray(x)
    assert tuple(out.shape) == (4, 0, 5)


def _typed_input(din):
    rng = np.random.default_rng(3)
    v32 = rng.random((5, 6, 70), dtype=np.float32) * 200
    if din == "bool":
        return (v32 > 100).astype(np.uint8)
    if not din.startswith("uint"):
        v32 = v32 - 50  # signed and float inputs: negative values too
    return O.cast_from_f32(v32, din)


# All 13 x 13 type pairs on one block whose sums overflow the narrow outputs: the 8-bit sums
# wrap, f16 reaches inf.
@pytest.mark.parametrize("dout", list(O.DTYPES))
def test_all_type_pairs(dout):
    for din in O.DTYPES:
        v = _typed_input(din)
        ref = R.sat(v, din, dout)
        if din == "uint16" and dout in ("uint8", "int8"):
            assert int(R.sat(v, din, "int64")[-1, -1, -1]) > 1000  # wrapped many times
        if din == "float32" and dout == "float16":
            assert np.isinf(ref.view(np.float16)).any()
        assert_same_bits(gpu_sat(v, din, dout, (4, 4, 32)), ref, dout)


@pytest.mark.parametrize("dout", ["float32", "int32"])
def test_special_values(dout):
    rng = np.random.default_rng(9)
    v = (rng.random((6, 9, 70), dtype=np.float32) * 10 - 3).astype(np.float32)
    v[1, 2, 3] = np.inf
    v[1, 2, 40] = -np.inf     # inf + -inf = NaN further along the row (f32)
    v[4, 7, 6] = -np.inf
    v[3, 5, 12] = np.nan      # as i32: 0
    v[0, 0, 0] = -0.0
    v[0, :, 0] = -0.0         # -0.0 lanes: +0.0 from the zero accumulator
    v[2, 8, 17] = 3e38
    ref = R.sat(v, "float32", dout)
    if dout == "float32":
        assert np.isnan(ref).any() and np.isinf(ref).any()
        assert not np.signbit(ref[0, 0, 0])
    assert_same_bits(gpu_sat(v, "float32", dout), ref, dout)


def test_f32_running_sum_past_2_pow_24_keeps_the_sequential_rounding():
    # past 2^24 every add rounds: the result is that of the left-to-right fold alone
    rng = np.random.default_rng(11)
    v = (rng.random((3, 4, 6000), dtype=np.float32) * 6000).astype(np.float32)
    ref = R.sat(v, "float32", "float32")
    assert ref[0, 0, -1] > 2 ** 24
    assert (ref != R.sat(v, "float32", "float64").astype(np.float32)).any()
    assert_same_bits(gpu_sat(v, "float32", "float32"), ref, "float32")


@pytest.mark.parametrize("din,dout", PAIRS)
@pytest.mark.parametrize("shape", [(9, 7, 40), (9,), (9, 1, 1)])
def test_carry_plane_joins_two_halves(din, dout, shape):
    import torch
    v = values(shape, din, seed=5)
    whole, last = R.sat(v, din, dout, return_carry=True)
    f = zt.SummedAreaTable()
    carry = torch.zeros(shape[1:], dtype=zt.torch_dtype(dout), device="cuda")
    a = f.apply_ndarray(to_dev(v[:4], din), dout, carry=carry)
    b = f.apply_ndarray(to_dev(v[4:], din), dout, carry=carry)
    torch.cuda.synchronize()
    got = np.concatenate([from_dev(a, dout), from_dev(b, dout)])
    assert_same_bits(got, whole, dout)
    assert_same_bits(from_dev(carry, dout), last, dout)
    # no carry equals a zeroed one
    zero = torch.zeros(shape[1:], dtype=zt.torch_dtype(dout), device="cuda")
    c0 = f.apply_ndarray(to_dev(v, din), dout, carry=zero)
    c1 = f.apply_ndarray(to_dev(v, din), dout)
    torch.cuda.synchronize()
    assert_same_bits(from_dev(c0, dout), whole, dout)
    assert_same_bits(from_dev(c1, dout), whole, dout)


# ---- store path: (20, 24, 70) u16 in (8, 8, 32) chunks: ragged on every axis, three chunk
# rows, so the carry plane is handed on twice ----------------------------------------------------
SHAPE, CHUNK = (20, 24, 70), (8, 8, 32)


@pytest.fixture(scope="module")
def store_in(tmp_path_factory):
    d = tmp_path_factory.mktemp("sat")
    u = O.synth_u16(SHAPE)
    S.create_array(d / "in.zarr", "uint16", SHAPE, CHUNK, S.codecs_json("gzip"))
    S.write_array(d / "in.zarr", u)
    return d, u


@pytest.mark.parametrize("dout", ["int64", "float32"])
def test_store_summed_area_table(store_in, tmp_path, dout):
    d, u = store_in
    ref = R.sat(u, "uint16", dout)
    st = S.summed_area_table(d / "in.zarr", tmp_path / "out.zarr", data_type=dout)
    out = S.read_array(tmp_path / "out.zarr")
    assert out.dtype == O.NP_STORAGE[dout]
    assert_same_bits(out, ref, dout)
    assert st["voxels"] == u.size and st["rows"] == 3
    meta = json.load(open(tmp_path / "out.zarr" / "zarr.json"))
    assert meta["data_type"] == dout and meta["shape"] == list(SHAPE)
    # one chunk in flight: no overlap of rows, the same result
    S.summed_area_table(d / "in.zarr", tmp_path / "one.zarr", data_type=dout, chunk_limit=1)
    S.set_chunk_limit(0)
    assert_same_bits(S.read_array(tmp_path / "one.zarr"), ref, dout)


def test_cli_summed_area_table(store_in, tmp_path):
    d, u = store_in
    assert ZF.main(["summed-area-table", str(d / "in.zarr"), str(tmp_path / "out.zarr"),
                    "--data-type", "int64"]) == 0
    out = S.read_array(tmp_path / "out.zarr")
    assert_same_bits(out, R.sat(u, "uint16", "int64"), "int64")


def test_device_chain_after_a_gaussian(store_in, tmp_path):
    d, u = store_in
    sigma, half = [1.0, 1.0, 1.0], [2, 2, 2]
    S.gaussian(d / "in.zarr", tmp_path / "g.zarr", sigma, half)
    g = S.read_array(tmp_path / "g.zarr")
    assert g.dtype == np.uint16
    lines = []
    steps = [{"filter": "gaussian", "input": str(d / "in.zarr"), "output": "$tmp",
              "sigma": sigma, "kernel_half_size": half},
             {"filter": "summed_area_table", "input": "$tmp", "output": str(tmp_path / "o.zarr"),
              "data_type": "int64"}]
    res = ZF.run(steps, tmp=str(tmp_path), log=lines.append)
    assert len(res) == 2 and all(r.get("device_resident") for r in res), lines
    assert_same_bits(S.read_array(tmp_path / "o.zarr"), R.sat(g, "uint16", "int64"), "int64")
