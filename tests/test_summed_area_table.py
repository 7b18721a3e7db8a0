"""Summed-area table (summed_area_table.rs) on the CPU: the numpy restatement (tests/sat_ref.py)
against the reference's known answer and the oracle's f64 table, the zero-accumulator seed, and
the host-only parts of the operator surface and of the zarrs_filter command."""
import numpy as np
import pytest

import zarrs_tools_amd as zt
from oracle import oracle as O
from tests import sat_ref as R
from zarrs_tools_amd import _abi
from zarrs_tools_amd import store as S
from zarrs_tools_amd import zarrs_filter as ZF

# summed_area_table.rs:276-283 (u8 in, chunks 2x2) and :306-313 (u16 out)
KAT_IN = np.array([[31, 2, 4, 33, 5, 36],
                   [12, 26, 9, 10, 29, 25],
                   [13, 17, 21, 22, 20, 18],
                   [24, 23, 15, 16, 14, 19],
                   [30, 8, 28, 27, 11, 7],
                   [1, 35, 34, 3, 32, 6]], dtype=np.uint8)
KAT_OUT = np.array([[31, 33, 37, 70, 75, 111],
                    [43, 71, 84, 127, 161, 222],
                    [56, 101, 135, 200, 254, 333],
                    [80, 148, 197, 278, 346, 444],
                    [110, 186, 263, 371, 450, 555],
                    [111, 222, 333, 444, 555, 666]], dtype=np.uint16)


def test_restatement_reproduces_reference_kat():
    out = R.sat(KAT_IN, "uint8", "uint16")
    assert out.dtype == np.uint16 and np.array_equal(out, KAT_OUT)
    # in u8 the same sums wrap (release builds): 666 mod 256
    assert R.sat(KAT_IN, "uint8", "uint8")[-1, -1] == 666 % 256


def test_restatement_equals_oracle_f32_to_f64():
    rng = np.random.default_rng(1)
    v = (rng.random((5, 7, 9), dtype=np.float32) * 1000 - 200).astype(np.float32)
    ref = O.summed_area_table(v)
    assert ref.dtype == np.float64
    assert np.array_equal(R.sat(v, "float32", "float64"), ref)
    # the accumulator's type is visible at this size: f32 sums are not the rounded f64 sums
    assert (R.sat(v, "float32", "float32") != ref.astype(np.float32)).any()


@pytest.mark.parametrize("dt", ["float32", "float64", "float16", "bfloat16"])
def test_negative_zero_first_elements_become_positive_zero(dt):
    # the fold starts from a zero accumulator and adds it to the first element too
    # (summed_area_table.rs:69, :94-97): 0.0 + -0.0 = +0.0
    v = R.as_cast(np.full((2, 3), -0.0, dtype=np.float32), "float32", dt)
    assert (v.view(np.uint8) != 0).any()  # the sign bits are set
    out = R.sat(v, dt)
    assert not out.view(np.uint8).any()


def test_seed_plane_continues_the_fold():
    rng = np.random.default_rng(2)
    v = (rng.random((6, 5, 7), dtype=np.float32) * 1000).astype(np.float32)
    whole, last = R.sat(v, "float32", return_carry=True)
    assert np.array_equal(last, whole[-1])
    a, ca = R.sat(v[:2], "float32", return_carry=True)
    b = R.sat(v[2:], "float32", carry=ca)
    assert np.array_equal(np.concatenate([a, b]), whole)


def test_is_compatible_all_13_types():
    f = zt.SummedAreaTable()
    assert len(_abi.DTYPES) == 13
    for a in _abi.DTYPES:
        for b in _abi.DTYPES:
            f.is_compatible(a, b)
    with pytest.raises(zt.UnsupportedDataType):
        f.is_compatible("complex64", "float32")
    with pytest.raises(zt.UnsupportedDataType):
        f.is_compatible("float32", "complex64")


def test_memory_per_chunk_is_one_element_of_each_type():
    # summed_area_table.rs:136-142 (sic): 2 + 8, whatever the chunk shape
    f = zt.SummedAreaTable()
    assert f.memory_per_chunk("uint16", "int64", (4, 5, 6)) == 10
    assert f.memory_per_chunk("uint16", "int64", (64, 64, 64)) == 10


def test_name():
    assert zt.SummedAreaTable().name() == "summed area table"


def test_subcommand_parses_to_the_step():
    a = ZF.build_parser().parse_args(["summed-area-table", "in.zarr", "out.zarr",
                                      "--data-type", "int64", "-c", "8,8,32"])
    steps = ZF._steps_from_cli(a)
    assert len(steps) == 1
    st = steps[0]
    assert st["filter"] == "summed_area_table" and st["filter"] in ZF.ON_PATH
    assert (st["input"], st["output"], st["data_type"]) == ("in.zarr", "out.zarr", "int64")
    assert st["chunk_shape"] == [8, 8, 32]
    # no arguments of its own (SummedAreaTableArguments {})
    with pytest.raises(SystemExit):
        ZF.build_parser().parse_args(["summed-area-table", "in.zarr", "out.zarr", "3"])


def test_step_params():
    info = S.ArrayInfo("in.zarr", "uint16", (20, 24, 70), (8, 8, 32), (8, 8, 32))
    f, shape, dt = ZF._step_params({"filter": "summed_area_table"}, info)
    assert isinstance(f, zt.SummedAreaTable) and shape == (20, 24, 70) and dt == "uint16"
    _f, _shape, dt = ZF._step_params({"filter": "summed_area_table", "data_type": "int64"}, info)
    assert dt == "int64"


def test_rows_splittable():
    # each chunk row of a summed-area table needs the previous row's last plane
    assert not ZF.rows_splittable("summed_area_table")
    for name in ("guided_filter", "downsample", "gaussian"):
        assert ZF.rows_splittable(name)


def test_store_rejects_null_paths():
    rc = _abi.lib().zt_store_summed_area_table(None, None, -1, None, 0, 0, 3, None)
    assert rc == _abi.ERR_INVALID_PARAMETERS
