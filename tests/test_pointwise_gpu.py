"""GPU parity of the per-element filters (pointwise.hip through the C ABI, the store path, the
zarrs_filter command and the device-resident chain runner) against the numpy restatement of the
reference (tests/pw_ref.py): bit-exact for every type.

Borders of the kernel (pointwise.hip): a row is cut into vectors of V = 16 / min(input size,
output size) elements; a lane carries 16 elements (16 / V vectors) per step, so a workgroup of
256 lanes reaches REACH = 4096 elements of a row per step, and rows shorter than that share a
workgroup; the first and last vector of a row that its ends cut go element by element, the
others as 16-byte accesses aligned on the side with the smaller element.
"""
import ctypes
import json

import numpy as np
import pytest

from oracle import oracle as O
from tests import pw_ref as R
from tests import sat_ref
from tests.gpu_util import FLOAT_TOL, from_dev, poisoned, rel_err, to_dev

pytestmark = pytest.mark.gpu

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)
from zarrs_tools_amd import _abi  # noqa: E402
from zarrs_tools_amd import store as S  # noqa: E402
from zarrs_tools_amd import zarrs_filter as ZF  # noqa: E402

ALL = list(_abi.DTYPES)
SIZE = {dt: np.dtype(O.NP_STORAGE[dt]).itemsize for dt in ALL}
QUIET = dict(log=lambda *a: None)
REACH = 256 * 16


def V(din, dout):
    return 16 // min(SIZE[din], SIZE[dout])


prefill = poisoned  # an output buffer that no result equals by accident (tests/gpu_util.py)


def gpu(v, din, filters, douts):
    """filters as one program on the storage array v; returns the storage array of douts[-1]."""
    import torch
    prog = zt.PointwiseProgram(filters, din, douts, v.shape)
    y = prefill(prog.shape, douts[-1])
    prog.run(to_dev(v, din), y)
    torch.cuda.synchronize()
    return from_dev(y, douts[-1])


def noise(n, din, seed=0):
    """n elements of din: the type's special values first, then noise."""
    return R.type_values(din, n, seed)[:n]


def read(path):
    """A store array as the restatement holds it (bool as u8)."""
    a = S.read_array(path)
    return a.view(np.uint8) if a.dtype == np.bool_ else a


# ---- flat lengths ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dout", ["uint8", "int64"])
@pytest.mark.parametrize("din", ["uint8", "uint16", "float32", "float64"])
def test_flat_lengths(din, dout):
    v_ = V(din, dout)
    for n in (0, 1, v_ - 1, v_, v_ + 1, 256 * v_ + 3, REACH + 3):
        v = noise(n, din, n)
        out = gpu(v, din, [zt.Reencode()], [dout])
        R.assert_same_bits(out, R.reencode(v, din, dout), dout)


def test_grid_stride_second_trip(monkeypatch):
    # two workgroups: 2 * REACH elements per trip of the grid-stride loop; 2.5 trips
    monkeypatch.setenv("ZT_PW_MAX_BLOCKS", "2")
    n = 5 * REACH + 5
    v = noise(n, "uint16", 1)
    out = gpu(v, "uint16", [zt.Clamp(100.0, 40000.0)], ["uint16"])
    R.assert_same_bits(out, R.clamp(v, "uint16", 100.0, 40000.0), "uint16")
    # rows of a 2-D box with the cap in force: 4 rows per workgroup step, 16 rows, two trips
    v2 = noise(16 * 1024, "float32", 2).reshape(16, 1024)
    out = gpu(v2, "float32", [zt.Crop([0, 1], [16, 1000])], ["uint8"])
    R.assert_same_bits(out, R.crop(v2, "float32", (0, 1), (16, 1000), "uint8"), "uint8")


# ---- misaligned pointers ---------------------------------------------------------------------------

@pytest.mark.parametrize("din,dout", [("uint8", "uint8"), ("uint16", "uint16"),
                                      ("float32", "float32"), ("float64", "float64"),
                                      ("uint8", "float64"), ("float64", "uint8"),
                                      ("uint16", "uint8")])
def test_views_one_element_into_their_buffers(din, dout):
    import torch
    v_ = V(din, dout)
    for n in (1, v_ - 1, 3 * v_ + 2, REACH + v_ // 2):
        v = noise(n + 2, din, n)
        x = to_dev(v, din)
        y = prefill((n + 2,), dout)
        guard = from_dev(y, dout).copy()
        prog = zt.PointwiseProgram([zt.Reencode()], din, [dout], (n,))
        _abi.check(_abi.lib().zt_pointwise_apply_ndarray(
            zt.default_context().handle, _abi.DTYPES[din],
            ctypes.c_void_p(x.data_ptr() + SIZE[din]), _abi.i64_array([n]), 1, None, None,
            prog.ops, 1, ctypes.c_void_p(y.data_ptr() + SIZE[dout])))
        torch.cuda.synchronize()
        out = from_dev(y, dout)
        R.assert_same_bits(out[1:n + 1], R.reencode(v[1:n + 1], din, dout), dout)
        # the element before and the element after the view are untouched
        assert out[:1].tobytes() == guard[:1].tobytes()
        assert out[n + 1:].tobytes() == guard[n + 1:].tobytes()


# ---- sub-boxes ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("din,dout", [("uint16", "uint16"), ("uint8", "float32")])
@pytest.mark.parametrize("rank", [1, 2, 3, 4])
def test_crop_row_lengths_and_offsets(din, dout, rank):
    v_ = V(din, dout)
    outer, ostart = (3, 2, 4)[:rank - 1], (1, 0, 2)[:rank - 1]
    for length in (1, v_ - 1, v_ + 1):
        for x0 in (0, 1, v_ - 1):
            shape = tuple(o + s + 1 for o, s in zip(ostart, outer)) + (x0 + length + 2,)
            v = noise(int(np.prod(shape)), din, length + x0).reshape(shape)
            off, sub = ostart + (x0,), outer + (length,)
            out = gpu(v, din, [zt.Crop(off, sub)], [dout])
            R.assert_same_bits(out, R.crop(v, din, off, sub, dout), dout)


def test_crop_of_the_whole_array_and_of_nothing():
    v = noise(5 * 6 * 7, "int16", 3).reshape(5, 6, 7)
    out = gpu(v, "int16", [zt.Crop((0, 0, 0), (5, 6, 7))], ["float32"])
    R.assert_same_bits(out, R.reencode(v, "int16", "float32"), "float32")
    # full trailing axes merge into the row: planes 1..3 are one contiguous run
    out = gpu(v, "int16", [zt.Crop((1, 0, 0), (3, 6, 7))], ["int16"])
    R.assert_same_bits(out, v[1:4], "int16")
    out = gpu(v, "int16", [zt.Crop((1, 2, 3), (3, 0, 2))], ["int16"])
    assert out.shape == (3, 0, 2)
    with pytest.raises(zt.InvalidParameters, match="outside the array"):
        _abi.check(_abi.lib().zt_pointwise_apply_ndarray(
            zt.default_context().handle, _abi.DTYPES["int16"], ctypes.c_void_p(256),
            _abi.i64_array([5]), 1, _abi.i64_array([3]), _abi.i64_array([3]),
            zt.PointwiseProgram([zt.Reencode()], "int16", ["int16"], (5,)).ops, 1,
            ctypes.c_void_p(256)))


# ---- every op over every input type ------------------------------------------------------------------

def _special(din):
    return {"bool": (True, False)}.get(din, (5, 7))


@pytest.mark.parametrize("din", ALL)
def test_every_op_from_every_type(din):
    v = R.type_values(din, 40, 7)
    value, replace = _special(din)
    for dout in dict.fromkeys([din, "uint8", "float32", "int64"]):
        rep = replace if dout != "bool" else False
        if dout != "bool" and isinstance(rep, bool):
            rep = 7
        cases = [
            ([zt.Reencode()], R.reencode(v, din, dout)),
            ([zt.Crop([3], [v.size - 5])], R.crop(v, din, (3,), (v.size - 5,), dout)),
            ([zt.Rescale(0.5, -3.25)], R.rescale(v, din, 0.5, -3.25, dout=dout)),
            ([zt.Rescale(0.5, -3.25, add_first=True)],
             R.rescale(v, din, 0.5, -3.25, add_first=True, dout=dout)),
            ([zt.Clamp(-5.5, 100.25)], R.clamp(v, din, -5.5, 100.25, dout)),
            ([zt.Clamp(np.nan, 2.0)], R.clamp(v, din, np.nan, 2.0, dout)),
            ([zt.ReplaceValue(value, rep)], R.replace_value(v, din, value, rep, dout)),
        ]
        for filters, ref in cases:
            R.assert_same_bits(gpu(v, din, filters, [dout]), ref, dout)
    values = [value]
    if din in R.FLOATS:
        values += [-0.0, "NaN", "Infinity"]
    for dout in ("bool", "uint8"):
        for val in values:
            out = gpu(v, din, [zt.Equal(val)], [dout])
            R.assert_same_bits(out, R.equal(v, din, val, dout), dout)
    if din in R.FLOATS:  # a NaN `value` replaces nothing
        out = gpu(v, din, [zt.ReplaceValue("NaN", 1.0)], [din])
        R.assert_same_bits(out, v, din)


# ---- rescale: one rounding ------------------------------------------------------------------------------

def test_rescale_is_fused_unless_add_first():
    v = np.arange(4096, dtype=np.uint16)
    fused = R.rescale(v, "uint16", 0.00035, 0.1, dout="float64")
    unfused = R.rescale(v, "uint16", 0.00035, 0.1, dout="float64", fused=False)
    assert np.count_nonzero(fused != unfused) == 1131  # counted on the CPU
    out = gpu(v, "uint16", [zt.Rescale(0.00035, 0.1)], ["float64"])
    R.assert_same_bits(out, fused, "float64")
    out = gpu(v, "uint16", [zt.Rescale(0.00035, 0.1, add_first=True)], ["float64"])
    R.assert_same_bits(out, (v.astype(np.float64) + 0.1) * 0.00035, "float64")


# ---- 64-bit exactness -------------------------------------------------------------------------------------

def test_64_bit_integers_compare_exactly():
    u = np.array([2 ** 53, 2 ** 53 + 1, 2 ** 64 - 1], dtype=np.uint64)
    assert gpu(u, "uint64", [zt.Equal(2 ** 53 + 1)], ["bool"]).tolist() == [0, 1, 0]
    out = gpu(u, "uint64", [zt.ReplaceValue(2 ** 53 + 1, 7)], ["uint64"])
    assert out.tolist() == [2 ** 53, 7, 2 ** 64 - 1]
    i = np.array([-2 ** 63, -2 ** 63 + 1, 2 ** 63 - 1, -2 ** 53 - 1], dtype=np.int64)
    assert gpu(i, "int64", [zt.Equal(-2 ** 63)], ["uint8"]).tolist() == [1, 0, 0, 0]
    out = gpu(i, "int64", [zt.ReplaceValue(-2 ** 63, -1)], ["int64"])
    assert out.tolist() == [-1, -2 ** 63 + 1, 2 ** 63 - 1, -2 ** 53 - 1]
    assert gpu(i, "int64", [zt.Equal(-2 ** 53 - 1)], ["bool"]).tolist() == [0, 0, 0, 1]


# ---- programs ------------------------------------------------------------------------------------------------

CHAIN = [zt.Rescale(0.01275, 0.0), zt.Clamp(2, 5), zt.Equal(5)]
CHAIN_TYPES = ["uint8", "uint8", "bool"]
CHAIN_REF = [("rescale", "uint8", dict(multiply=0.01275, add=0.0)),
             ("clamp", "uint8", dict(lo=2.0, hi=5.0)), ("equal", "bool", dict(value=5))]


def test_the_documented_chain_as_one_program():
    v = noise(3000, "uint16", 5)
    v[:1200] = np.arange(1200)  # the range where the chain's output changes
    fused = gpu(v, "uint16", CHAIN, CHAIN_TYPES)
    step, dt = v, "uint16"
    for f, dout in zip(CHAIN, CHAIN_TYPES):
        step, dt = gpu(step, dt, [f], [dout]), dout
    ref = R.program(v, "uint16", CHAIN_REF)
    assert 0 < int(ref.sum()) < ref.size
    R.assert_same_bits(fused, ref, "bool")
    R.assert_same_bits(step, ref, "bool")


EIGHT = [zt.Reencode(), zt.Rescale(0.37, -11.5), zt.Clamp(-3.0, 200.0), zt.Reencode(),
         zt.ReplaceValue(7, -2), zt.Crop([5], [900]), zt.Rescale(3.0, 1.0, add_first=True),
         zt.ReplaceValue(-3, 65535)]
EIGHT_TYPES = ["float16", "float32", "float32", "int16", "int32", "bfloat16", "int64", "uint16"]
EIGHT_REF = [("reencode", "float16", {}), ("rescale", "float32", dict(multiply=0.37, add=-11.5)),
             ("clamp", "float32", dict(lo=-3.0, hi=200.0)), ("reencode", "int16", {}),
             ("replace_value", "int32", dict(value=7, replace=-2)),
             ("crop", "bfloat16", dict(offset=(5,), shape=(900,))),
             ("rescale", "int64", dict(multiply=3.0, add=1.0, add_first=True)),
             ("replace_value", "uint16", dict(value=-3, replace=65535))]


def test_an_eight_op_program_equals_its_ops_one_by_one():
    v = np.arange(1000, dtype=np.uint16)
    fused = gpu(v, "uint16", EIGHT, EIGHT_TYPES)
    step, dt = v, "uint16"
    for f, dout in zip(EIGHT, EIGHT_TYPES):
        step, dt = gpu(step, dt, [f], [dout]), dout
    ref = R.program(v, "uint16", EIGHT_REF)
    assert len(np.unique(ref)) > 50
    R.assert_same_bits(fused, ref, "uint16")
    R.assert_same_bits(step, ref, "uint16")


def test_nine_ops_are_rejected_by_the_abi():
    ops = (_abi.PointwiseOp * 9)(*[zt.Clamp(0, 5).op("uint8", "uint8")] * 9)
    x = to_dev(np.zeros(4, dtype=np.uint8), "uint8")
    with pytest.raises(zt.InvalidParameters, match="1 to 8"):
        _abi.check(_abi.lib().zt_pointwise_apply_ndarray(
            zt.default_context().handle, _abi.DTYPES["uint8"], ctypes.c_void_p(x.data_ptr()),
            _abi.i64_array([4]), 1, None, None, ops, 9, ctypes.c_void_p(x.data_ptr())))
    bad = (_abi.PointwiseOp * 2)(zt.Reencode().op("uint8", "float32"),
                                 _abi.PointwiseOp(_abi.PW_EQUAL, _abi.DTYPES["int16"], 0, 0, 0, 0))
    with pytest.raises(zt.UnsupportedDataType):  # the type chain is validated
        _abi.check(_abi.lib().zt_pointwise_apply_ndarray(
            zt.default_context().handle, _abi.DTYPES["uint8"], ctypes.c_void_p(x.data_ptr()),
            _abi.i64_array([4]), 1, None, None, bad, 2, ctypes.c_void_p(x.data_ptr())))


# ---- store path ------------------------------------------------------------------------------------------------

SHAPE, CHUNK, FILL = (20, 12, 10), (8, 5, 4), 65535


@pytest.fixture(scope="module")
def stored(tmp_path_factory):
    """A 3-D uint16 array with ragged chunks and the chunks of x >= 8, z >= 8 missing (they read
    as the fill value 65535); returns (path, the array as it reads)."""
    root = tmp_path_factory.mktemp("pw")
    v = (O.synth_u16(SHAPE) // 3).astype(np.uint16)
    v[::7, ::5, ::3] = 5
    S.create_array(root / "in", "uint16", SHAPE, CHUNK, fill_value=FILL)
    S.write_array(root / "in", v[:8])
    S.write_array(root / "in", v[8:, :, :8], start=(8, 0, 0))
    v[8:, :, 8:] = FILL
    assert np.array_equal(S.read_array(root / "in"), v)
    return root, v


STORE_CASES = {
    "reencode": (lambda: zt.Reencode(), dict(), "float32", ["reencode"]),
    "crop": (lambda: zt.Crop((3, 2, 1), (14, 9, 8)), dict(offset=(3, 2, 1), shape=(14, 9, 8)),
             None, ["crop", "3,2,1", "14,9,8"]),
    "rescale": (lambda: zt.Rescale(0.01275, -0.5), dict(multiply=0.01275, add=-0.5), "uint8",
                ["rescale", "0.01275", "-0.5"]),
    "clamp": (lambda: zt.Clamp(-5, 20000.5), dict(lo=-5.0, hi=20000.5), None,
              ["clamp", "-5", "20000.5"]),
    "equal": (lambda: zt.Equal(5), dict(value=5), None, ["equal", "5"]),
    "replace_value": (lambda: zt.ReplaceValue(65535, -1.5), dict(value=65535, replace=-1.5),
                      "float32", ["replace-value", "65535", "-1.5"]),
}


@pytest.mark.parametrize("name", list(STORE_CASES))
def test_store_function_and_subcommand(stored, name, tmp_path):
    root, v = stored
    make, kw, dt, argv = STORE_CASES[name]
    dout = dt or ("bool" if name == "equal" else "uint16")
    ref = R.program(v, "uint16", [(name, dout, kw)])
    f = make()
    args = {"reencode": (), "crop": (f.offset, f.shape) if name == "crop" else (),
            "rescale": (0.01275, -0.5), "clamp": (-5, 20000.5), "equal": (5,),
            "replace_value": (65535, -1.5)}[name]
    st = getattr(S, name)(root / "in", tmp_path / "a", *args, data_type=dt)
    assert st["voxels"] == ref.size and st["kernel_s"] > 0
    a = S.open_array(tmp_path / "a")
    assert a.data_type == dout and a.shape == ref.shape
    R.assert_same_bits(read(tmp_path / "a"), ref, dout)
    # the subcommand, into a sharded output
    argv = [argv[0], str(root / "in"), str(tmp_path / "b")] + argv[1:] + (
        ["--data-type", dt] if dt else []) + ["-s", "16,10,8", "-c", "4,5,4"]
    assert ZF.main(argv) == 0
    b = S.open_array(tmp_path / "b")
    assert b.chunk_shape == (16, 10, 8) and b.inner_chunk_shape == (4, 5, 4)
    R.assert_same_bits(read(tmp_path / "b"), ref, dout)
    if name == "equal":  # Equal::output_data_type: bool, fill value false
        assert a.metadata["fill_value"] is False
    if name == "reencode":  # the fill value follows the data type
        assert a.metadata["fill_value"] == 65535.0


def test_store_rows_split_over_two_processes(stored, tmp_path):
    root, v = stored
    steps = [{"filter": "crop", "input": str(root / "in"), "output": str(tmp_path / "one"),
              "offset": [3, 2, 1], "shape": [14, 9, 8], "data_type": "float32"}]
    ZF.run(steps, **QUIET)
    steps[0]["output"] = str(tmp_path / "two")
    st = ZF.run(steps, gpus=2, gpu_devices=[0, 0], **QUIET)
    assert st[0]["processes"] == 2
    ref = R.crop(v, "uint16", (3, 2, 1), (14, 9, 8), "float32")
    R.assert_same_bits(S.read_array(tmp_path / "one"), ref, "float32")
    R.assert_same_bits(S.read_array(tmp_path / "two"), ref, "float32")


# ---- the reference's example run config, scaled down ----------------------------------------------------------

def test_reference_example_run_config(tmp_path):
    # docs/zarrs_filter.md "Examples (Config)": the same steps, keys and $reencode0 reuse, on a
    # 40 x 24 x 16 input with shards of 16^3 and chunks of 4^3 (the gradient_magnitude step is
    # left out: zarrs_filter rejects it)
    shape = (40, 24, 16)
    v = O.synth_u16(shape)
    v[::3, ::2, ::5] = 65535
    S.create_array(tmp_path / "array.zarr", "uint16", shape, (10, 8, 16), fill_value=0)
    S.write_array(tmp_path / "array.zarr", v)
    p = lambda n: str(tmp_path / n)  # noqa: E731
    cfg = [
        {"_comment": "Rechunk the input", "filter": "reencode", "input": p("array.zarr"),
         "output": "$reencode0", "shard_shape": [16, 16, 16], "chunk_shape": [4, 4, 4]},
        {"filter": "reencode", "output": p("array_float32.zarr"), "data_type": "float32"},
        {"filter": "crop", "input": "$reencode0", "output": p("array_crop.zarr"),
         "offset": [10, 6, 4], "shape": [30, 18, 12]},
        {"filter": "replace_value", "input": "$reencode0", "output": p("array_replace.zarr"),
         "value": 65535, "replace": 0},
        {"filter": "rescale", "input": "$reencode0", "output": p("array_3bit.zarr"),
         "multiply": 0.00035, "add": 0.0, "data_type": "uint8", "fill_value": 0},
        {"filter": "rescale", "input": "$reencode0", "output": p("array_8bit.zarr"),
         "multiply": 0.01275, "add": 0.0, "data_type": "uint8", "fill_value": 0},
        {"filter": "clamp", "output": p("array_3bit_clamp.zarr"), "min": 2, "max": 5,
         "fill_value": 2},
        {"filter": "equal", "input": p("array_3bit_clamp.zarr"),
         "output": p("array_clamp_equal_bool.zarr"), "value": 5},
        {"filter": "equal", "input": p("array_3bit_clamp.zarr"), "output": p("array_3bit_max.zarr"),
         "value": 5, "data_type": "uint8", "fill_value": 0},
        {"filter": "downsample", "input": p("array_3bit_clamp.zarr"),
         "output": p("array_3bit_clamp_by2_continuous.zarr"), "stride": [2, 2, 2],
         "discrete": False, "data_type": "float32", "shard_shape": [8, 8, 8],
         "chunk_shape": [4, 4, 4]},
        {"filter": "downsample", "input": p("array_3bit_clamp.zarr"),
         "output": p("array_3bit_clamp_by2_discrete.zarr"), "stride": [2, 2, 2],
         "discrete": True, "shard_shape": [8, 8, 8], "chunk_shape": [4, 4, 4]},
        {"filter": "gaussian", "input": "$reencode0", "output": p("array_gaussian.zarr"),
         "sigma": [1.0, 1.0, 1.0], "kernel_half_size": [3, 3, 3]},
        {"filter": "summed_area_table", "input": "$reencode0", "output": p("array_sat.zarr"),
         "data_type": "float32"},
        {"filter": "guided_filter", "input": "$reencode0",
         "output": p("array_guided_filter.zarr"), "epsilon": 40000.0, "radius": 3,
         "data_type": "float32"},
    ]
    (tmp_path / "run.json").write_text(json.dumps(cfg))
    (tmp_path / "tmp").mkdir()
    assert ZF.main([p("run.json"), "--tmp", p("tmp")]) == 0

    def rd(n):
        return read(p(n))

    f32 = S.open_array(p("array_float32.zarr"))
    assert f32.chunk_shape == (16, 16, 16) and f32.inner_chunk_shape == (4, 4, 4)
    R.assert_same_bits(rd("array_float32.zarr"), R.reencode(v, "uint16", "float32"), "float32")
    R.assert_same_bits(rd("array_crop.zarr"), v[10:, 6:, 4:], "uint16")
    R.assert_same_bits(rd("array_replace.zarr"), R.replace_value(v, "uint16", 65535, 0),
                       "uint16")
    R.assert_same_bits(rd("array_3bit.zarr"), R.rescale(v, "uint16", 0.00035, 0.0,
                                                          dout="uint8"), "uint8")
    b8 = R.rescale(v, "uint16", 0.01275, 0.0, dout="uint8")
    R.assert_same_bits(rd("array_8bit.zarr"), b8, "uint8")
    cl = R.clamp(b8, "uint8", 2.0, 5.0)  # an omitted input is the previous output: the 8-bit one
    R.assert_same_bits(rd("array_3bit_clamp.zarr"), cl, "uint8")
    assert S.open_array(p("array_3bit_clamp.zarr")).metadata["fill_value"] == 2
    eq = S.open_array(p("array_clamp_equal_bool.zarr"))
    assert eq.data_type == "bool" and eq.metadata["fill_value"] is False
    R.assert_same_bits(rd("array_clamp_equal_bool.zarr"), R.equal(cl, "uint8", 5),
                       "bool")
    assert S.open_array(p("array_3bit_max.zarr")).data_type == "uint8"
    R.assert_same_bits(rd("array_3bit_max.zarr"), R.equal(cl, "uint8", 5, "uint8"), "uint8")
    R.assert_same_bits(rd("array_3bit_clamp_by2_continuous.zarr"),
                       O.downsample(cl, "uint8", (2, 2, 2), "float32"), "float32")
    R.assert_same_bits(rd("array_3bit_clamp_by2_discrete.zarr"),
                       O.downsample(cl, "uint8", (2, 2, 2), "uint8", discrete=True), "uint8")
    g = O.gaussian_apply(v.astype(np.float32), (16, 16, 16), [1.0] * 3, [3] * 3)
    R.assert_same_bits(rd("array_gaussian.zarr"), sat_ref.as_cast(g, "float32", "uint16"),
                       "uint16")
    R.assert_same_bits(rd("array_sat.zarr"), sat_ref.sat(v, "uint16", "float32"), "float32")
    gf = O.guided_filter_apply(v.astype(np.float32), (16, 16, 16), 40000.0, 3, nthreads=8)
    assert rel_err(rd("array_guided_filter.zarr"), gf) <= FLOAT_TOL


# ---- device-resident chains -------------------------------------------------------------------------------------

def _chain_steps(src, dst):
    return [{"filter": "gaussian", "input": src, "output": "$a", "sigma": [1.0, 0.5, 1.0],
             "kernel_half_size": [2, 1, 2]},
            {"filter": "rescale", "input": "$a", "output": "$b", "multiply": 0.0004, "add": 0.0,
             "data_type": "uint8"},
            {"filter": "clamp", "input": "$b", "min": 2, "max": 5},
            {"filter": "equal", "output": dst, "value": 5}]


def test_device_chain_fuses_the_pointwise_steps(stored, tmp_path, capsys):
    root, v = stored
    src = str(root / "in")
    fused = ZF.run(_chain_steps(src, str(tmp_path / "fused")), **QUIET)
    unfused = ZF.run(_chain_steps(src, str(tmp_path / "unfused")), fuse_pointwise=False, **QUIET)
    stores = ZF.run(_chain_steps(src, str(tmp_path / "store")), device_chain=False, **QUIET)
    # the command's flag, on a run config: every step launches on its own
    (tmp_path / "run.json").write_text(json.dumps(_chain_steps(src, str(tmp_path / "cli"))))
    capsys.readouterr()
    assert ZF.main([str(tmp_path / "run.json"), "--no-pointwise-fusion", "--stats",
                    "--tmp", str(tmp_path)]) == 0
    cli = [json.loads(ln) for ln in capsys.readouterr().out.splitlines()
           if ln.startswith('{"step"')]
    assert [st["step"] for st in cli] == [0, 1, 2, 3]
    assert all(st["device_resident"] and st["kernel_s"] > 0 for st in cli)
    assert not any("fused_into" in st or "fused_steps" in st for st in cli)
    (tmp_path / "run.json").write_text(json.dumps(_chain_steps(src, str(tmp_path / "cli2"))))
    assert ZF.main([str(tmp_path / "run.json"), "--stats", "--tmp", str(tmp_path)]) == 0
    cli2 = [json.loads(ln) for ln in capsys.readouterr().out.splitlines()
            if ln.startswith('{"step"')]
    assert [st.get("fused_into") for st in cli2] == [None, 3, 3, None]
    # one launch carries the three per-element steps
    assert all(st.get("device_resident") for st in fused + unfused)
    assert [st.get("fused_into") for st in fused] == [None, 3, 3, None]
    assert fused[3]["fused_steps"] == [1, 2, 3]
    assert fused[1]["kernel_s"] == 0 and fused[2]["kernel_s"] == 0 and fused[3]["kernel_s"] > 0
    assert not any("fused_into" in st or "fused_steps" in st for st in unfused + stores)
    assert all(st["kernel_s"] > 0 for st in unfused)
    g = O.gaussian_apply(v.astype(np.float32), CHUNK, [1.0, 0.5, 1.0], [2, 1, 2])
    ref = R.program(sat_ref.as_cast(g, "float32", "uint16"), "uint16",
                    [("rescale", "uint8", dict(multiply=0.0004, add=0.0))] + CHAIN_REF[1:])
    assert 0 < int(ref.sum()) < ref.size
    for name in ("fused", "unfused", "store", "cli", "cli2"):
        out = S.open_array(tmp_path / name)
        assert out.data_type == "bool" and out.metadata["fill_value"] is False
        R.assert_same_bits(read(tmp_path / name), ref, "bool")


def test_device_chain_splits_nine_pointwise_steps(stored, tmp_path):
    root, v = stored
    steps = [{"filter": "crop", "input": str(root / "in"), "offset": [1, 1, 1],
              "shape": [18, 10, 8]}]
    ref = [("crop", "uint16", dict(offset=(1, 1, 1), shape=(18, 10, 8)))]
    for k in range(8):
        if k == 3:  # a second crop in the middle: the offsets add up
            steps.append({"filter": "crop", "offset": [2, 0, 1], "shape": [16, 10, 6]})
            ref.append(("crop", "uint16", dict(offset=(2, 0, 1), shape=(16, 10, 6))))
        else:
            steps.append({"filter": "rescale", "multiply": 1.0, "add": float(k - 3)})
            ref.append(("rescale", "uint16", dict(multiply=1.0, add=float(k - 3))))
    steps[-1]["output"] = str(tmp_path / "out")
    res = ZF.run(steps, **QUIET)
    assert [st.get("fused_into") for st in res] == [7] * 7 + [None, None]
    assert res[7]["fused_steps"] == list(range(8)) and "fused_steps" not in res[8]
    R.assert_same_bits(S.read_array(tmp_path / "out"), R.program(v, "uint16", ref), "uint16")
