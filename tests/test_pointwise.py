"""CPU: the per-element filters (reencode, crop, rescale, clamp, equal, replace_value) without
device work: the numpy restatement the GPU tests check against (tests/pw_ref.py) pinned by
hand-worked values, the command and run-config grammar, value parsing, crop validation, equal's
output type and the fusion planning of device-resident chains.

The reference has no known-answer test for these filters (src/filter/filters/{reencode,crop,
rescale,clamp,equal,replace_value}.rs carry no #[test]); the values below are worked by hand from
their element expressions.
"""
import numpy as np
import pytest

import zarrs_tools_amd as zt
from tests import pw_ref as R
from zarrs_tools_amd import _abi
from zarrs_tools_amd import filter as F
from zarrs_tools_amd import store as S
from zarrs_tools_amd import zarrs_filter as ZF

NAN = np.nan


# ---- hand-worked values pin the restatement ------------------------------------------------------

def test_clamp_nan_passes_and_casts_to_zero():
    # clamp.rs:59-70: lo = 0.0, hi = 5.0; NaN fails both comparisons and stays NaN; :150 `as u8`:
    # NaN -> 0, 0 -> 0 (from -1 clamped), 0 -> 0, 5 -> 5 (from 7 clamped)
    v = np.array([NAN, -1, 0, 7], dtype=np.float32)
    assert R.clamp(v, "float32", 0.0, 5.0, "uint8").tolist() == [0, 0, 0, 5]
    # in its own type the NaN is still there
    out = R.clamp(v, "float32", 0.0, 5.0)
    assert np.isnan(out[0]) and out[1:].tolist() == [0.0, 0.0, 5.0]


def test_clamp_negative_min_saturates_in_the_input_type():
    # `-5.0 as u8` = 0 (saturating), `200.0 as u8` = 200: nothing below 0 exists, 250 -> 200
    v = np.array([0, 3, 200, 250], dtype=np.uint8)
    assert R.clamp(v, "uint8", -5.0, 200.0).tolist() == [0, 3, 200, 200]
    # a NaN bound becomes 0 for an integer type: max = NaN -> hi = 0, everything above 0 -> 0
    assert R.clamp(v, "uint8", -5.0, NAN).tolist() == [0, 0, 0, 0]
    # for a float type a NaN bound disables its side
    f = np.array([-3.0, 9.0], dtype=np.float32)
    assert R.clamp(f, "float32", NAN, 5.0).tolist() == [-3.0, 5.0]


def test_rescale_saturates_into_uint8():
    # x * 2 + 10 in f64, then `as u8`: 0 -> 10, 100 -> 210, 123 -> 256 -> 255, 65535 -> 255;
    # a negative result saturates at 0
    v = np.array([0, 100, 123, 65535], dtype=np.uint16)
    assert R.rescale(v, "uint16", 2.0, 10.0, dout="uint8").tolist() == [10, 210, 255, 255]
    assert R.rescale(v, "uint16", -1.0, 50.0, dout="uint8").tolist() == [50, 0, 0, 0]
    # add_first: (x + 10) * 2: 0 -> 20, 100 -> 220, 123 -> 266 -> 255
    assert R.rescale(v[:3], "uint16", 2.0, 10.0, add_first=True, dout="uint8").tolist() == [
        20, 220, 255]
    # truncation toward zero: 3 * 0.5 = 1.5 -> 1
    assert R.rescale(np.array([3], dtype=np.uint8), "uint8", 0.5, 0.0).tolist() == [1]


def test_fma_is_one_rounding():
    # 0.1 * 10 - 1 exactly is 2^-54 * 10 = 5.55e-17 (0.1 is 0x1.999999999999ap-4); the product
    # rounded first gives exactly 1.0, so the two-rounding form gives 0
    assert R.fma(0.1, 10.0, -1.0) == 5.551115123125783e-17
    assert 0.1 * 10.0 - 1.0 == 0.0
    assert R.fma(2.0, 3.0, 1.0) == 7.0
    assert np.isnan(R.fma(NAN, 1.0, 1.0)) and R.fma(np.inf, 2.0, 1.0) == np.inf
    assert str(R.fma(-0.0, 1.0, -0.0)) == "-0.0" and str(R.fma(1.0, 1.0, -1.0)) == "0.0"


def test_equal_compares_values_not_bits():
    v = np.array([0.0, -0.0, 1.0, NAN], dtype=np.float32)
    assert R.equal(v, "float32", 0.0).tolist() == [1, 1, 0, 0]
    assert R.equal(v, "float32", -0.0).tolist() == [1, 1, 0, 0]
    assert R.equal(v, "float32", "NaN").tolist() == [0, 0, 0, 0]  # NaN equals nothing
    h = np.array([0x0000, 0x8000, 0x3C00], dtype=np.uint16)  # f16 +0, -0, 1
    assert R.equal(h, "float16", -0.0).tolist() == [1, 1, 0]
    u = np.array([2 ** 53, 2 ** 53 + 1], dtype=np.uint64)  # never compared through f64
    assert R.equal(u, "uint64", 2 ** 53 + 1).tolist() == [0, 1]


def test_replace_value_with_nan_value_replaces_nothing():
    v = np.array([NAN, 1.0, 2.0], dtype=np.float32)
    out = R.replace_value(v, "float32", "NaN", 9.0)
    assert np.isnan(out[0]) and out[1:].tolist() == [1.0, 2.0]
    # `value` in TIn, `replace` in TOut; the others go through `as`
    assert R.replace_value(v, "float32", 1.0, 200, "uint8").tolist() == [0, 200, 2]
    out = R.replace_value(np.array([0, 5], dtype=np.uint8), "uint8", 0, "NaN", "float32")
    assert np.isnan(out[0]) and out[1] == 5.0


def test_crop_and_reencode_restatement():
    v = np.arange(24, dtype=np.int16).reshape(2, 3, 4) - 5
    assert R.crop(v, "int16", (1, 1, 2), (1, 2, 2)).tolist() == [[[13, 14], [17, 18]]]
    assert R.reencode(v[0, 0], "int16", "uint8").tolist() == [251, 252, 253, 254]  # wraps
    chain = R.program(np.array([0, 200, 400], dtype=np.uint16), "uint16", [
        ("rescale", "uint8", dict(multiply=0.0125, add=0.0)),   # 0, 2.5 -> 2, 5
        ("clamp", "uint8", dict(lo=2.0, hi=5.0)),                # 2, 2, 5
        ("equal", "bool", dict(value=5))])
    assert chain.tolist() == [0, 0, 1]


# ---- command and run-config grammar ----------------------------------------------------------------

def _step(argv):
    steps = ZF._steps_from_cli(ZF.build_parser().parse_args(argv))
    assert len(steps) == 1
    return steps[0]


def test_subcommand_grammar_of_the_six():
    st = _step(["reencode", "i", "o", "--data-type", "float32", "-c", "4,4"])
    assert st["filter"] == "reencode" and st["data_type"] == "float32"
    assert st["chunk_shape"] == [4, 4] and (st["input"], st["output"]) == ("i", "o")
    st = _step(["crop", "i", "o", "256,256,256", "768,768,768"])
    assert st["filter"] == "crop" and st["offset"] == [256] * 3 and st["shape"] == [768] * 3
    st = _step(["rescale", "i", "o", "0.5", "-1.5", "--add-first", "-d", "float32"])
    assert (st["filter"], st["multiply"], st["add"], st["add_first"]) == ("rescale", 0.5, -1.5,
                                                                          True)
    st = _step(["rescale", "i", "o", "-2", "-1e-3"])
    assert (st["multiply"], st["add"], st["add_first"]) == (-2.0, -0.001, False)
    st = _step(["clamp", "i", "o", "-5", "7.5"])
    assert (st["filter"], st["min"], st["max"]) == ("clamp", -5.0, 7.5)
    st = _step(["equal", "i", "o", "-3"])
    assert (st["filter"], st["value"]) == ("equal", -3)
    assert _step(["equal", "i", "o", "-Infinity"])["value"] == "-Infinity"
    assert _step(["equal", "i", "o", "NaN"])["value"] == "NaN"
    assert _step(["equal", "i", "o", "true"])["value"] is True
    st = _step(["replace-value", "i", "o", "65535", "-1.5", "--data-type", "float32"])
    assert (st["filter"], st["value"], st["replace"]) == ("replace_value", 65535, -1.5)
    for name in ZF.POINTWISE:
        assert name in ZF.ON_PATH and ZF.rows_splittable(name)
    assert not ZF.rows_splittable("summed_area_table")


def test_run_config_keys_build_the_filters():
    f = ZF.pointwise_filter({"filter": "crop", "offset": [1, 2], "shape": "3,4"})
    assert isinstance(f, zt.Crop) and f.offset == (1, 2) and f.shape == (3, 4)
    f = ZF.pointwise_filter({"filter": "rescale", "multiply": 0.5, "add": -1, "add_first": True})
    assert (f.multiply, f.add, f.add_first) == (0.5, -1.0, True)
    f = ZF.pointwise_filter({"filter": "clamp", "min": -5, "max": 5})
    assert (f.min, f.max) == (-5.0, 5.0)
    assert ZF.pointwise_filter({"filter": "equal", "value": "NaN"}).value == "NaN"
    f = ZF.pointwise_filter({"filter": "replace_value", "value": 0, "replace": 7})
    assert (f.value, f.replace) == (0, 7)
    assert isinstance(ZF.pointwise_filter({"filter": "reencode"}), zt.Reencode)
    for step in ({"filter": "crop", "offset": [1]}, {"filter": "rescale", "multiply": 2},
                 {"filter": "clamp", "min": 0}, {"filter": "equal"},
                 {"filter": "replace_value", "value": 1}):
        with pytest.raises(_abi.InvalidParameters, match="needs"):
            ZF.pointwise_filter(step)
    assert [zt.Reencode().name(), zt.Crop([0], [1]).name(), zt.Rescale(1, 0).name(),
            zt.Clamp(0, 1).name(), zt.Equal(0).name(), zt.ReplaceValue(0, 1).name()] == list(
                ZF.POINTWISE)


def test_a_missing_argument_fails_the_run(tmp_path):
    S.create_array(tmp_path / "in", "uint8", (4,), (4,))
    with pytest.raises(_abi.InvalidParameters, match="needs max"):
        ZF.run([{"filter": "clamp", "input": str(tmp_path / "in"), "output": "$x", "min": 1}],
               log=lambda *a: None)


# ---- value / replace parsing -----------------------------------------------------------------------

def test_value_parsing():
    assert F.element_bits(255, "uint8") == 255
    assert F.element_bits(-1, "int8") == 0xFF and F.element_bits(-1, "int64") == 2 ** 64 - 1
    assert F.element_bits(2 ** 53 + 1, "uint64") == 2 ** 53 + 1
    assert F.element_bits(5.0, "uint16") == 5  # an integral JSON number
    assert F.element_bits(True, "bool") == 1 and F.element_bits(False, "bool") == 0
    assert F.element_bits(1.5, "float32") == 0x3FC00000
    assert F.element_bits(1, "float64") == 0x3FF0000000000000
    assert F.element_bits(-2, "float16") == 0xC000 and F.element_bits(-2, "bfloat16") == 0xC000
    assert F.element_bits("Infinity", "float16") == 0x7C00
    assert F.element_bits("-Infinity", "bfloat16") == 0xFF80
    assert F.element_bits("NaN", "float32") & 0x7FC00000 == 0x7FC00000
    # bf16 rounds to nearest even: 1 + 2^-8 is a tie -> 1.0; 1 + 2^-8 + 2^-20 rounds up
    assert F.element_bits(1.00390625, "bfloat16") == 0x3F80
    assert F.element_bits(1.00390625 + 2.0 ** -20, "bfloat16") == 0x3F81
    # one rounding from the f64 (half's from_f64, which decides on the f64's upper 32 bits: 20
    # mantissa bits): 1 + 2^-8 + 2^-22 is a tie there and goes to even; through f32 (which holds
    # the 2^-22) it would round up
    assert F.element_bits(1.00390625 + 2.0 ** -22, "bfloat16") == 0x3F80
    assert F.element_bits(1.00390625 + 2.0 ** -19, "bfloat16") == 0x3F81
    assert F.element_bits(65520.0, "float16") == 0x7C00 and F.element_bits(6e-8, "float16") == 1
    assert F.element_bits(1e-40, "bfloat16") == 1 and F.element_bits(-1e-60, "float16") == 0x8000
    for dt in ("float16", "bfloat16", "float32", "float64", "uint8", "int32"):
        floats = (1.5, -2.75, 1e-3, 3.3e4, 1.00390625 + 2.0 ** -22, 1e-6, 1e-41, 7e4,
                  1.0 + 2.0 ** -11 + 2.0 ** -21) if dt[0] in "fb" else ()
        for val in (0, 1, 5) + floats:  # the restatement's own reading agrees
            assert F.element_bits(val, dt) == int(R.element(val, dt).view(
                {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[
                    R.element(val, dt).itemsize])[0])


@pytest.mark.parametrize("value,dt", [
    (300, "uint8"), (-1, "uint16"), (128, "int8"), (2 ** 64, "uint64"), (1.5, "int32"),
    ("NaN", "int16"), (1, "bool"), (True, "uint8"), (True, "float32"), ("nan", "float32"),
    ([0, 255], "uint8"), (None, "float64"),
])
def test_incompatible_value_is_invalid_parameters(value, dt):
    with pytest.raises(_abi.InvalidParameters, match="not compatible"):
        F.element_bits(value, dt)
    with pytest.raises(_abi.InvalidParameters):
        zt.Equal(value).op(dt, "bool")
    with pytest.raises(_abi.InvalidParameters):
        zt.ReplaceValue(0 if dt != "bool" else False, value).op(dt, dt)


def test_incompatible_value_fails_the_run(tmp_path):
    S.create_array(tmp_path / "in", "uint8", (4,), (4,))
    with pytest.raises(_abi.InvalidParameters, match="not compatible"):
        ZF.run([{"filter": "equal", "input": str(tmp_path / "in"), "output": "$x",
                 "value": 300}], log=lambda *a: None)


# ---- crop validation, equal's output type ------------------------------------------------------------

def test_crop_rank_and_bounds_errors():
    c = zt.Crop([1, 2], [3, 4])
    assert c.output_shape((4, 6)) == (3, 4)
    with pytest.raises(_abi.InvalidParameters, match="one entry per axis"):
        c.output_shape((4, 6, 8))
    with pytest.raises(_abi.InvalidParameters, match="beyond the input"):
        c.output_shape((4, 5))
    with pytest.raises(_abi.InvalidParameters, match="one entry per axis"):
        zt.Crop([1, 2], [3]).output_shape((4, 6))
    with pytest.raises(_abi.InvalidParameters):
        zt.Crop([-1], [2])
    assert zt.Crop([0, 0], [0, 3]).output_shape((4, 6)) == (0, 3)  # a zero extent is a shape
    assert zt.Reencode().output_shape((4, 6)) == (4, 6)


def test_crop_errors_fail_the_run(tmp_path):
    S.create_array(tmp_path / "in", "uint8", (4, 6), (2, 3))
    for step, msg in (({"offset": [1], "shape": [2]}, "one entry per axis"),
                      ({"offset": [2, 2], "shape": [3, 3]}, "beyond the input")):
        with pytest.raises(_abi.InvalidParameters, match=msg):
            ZF.run([{"filter": "crop", "input": str(tmp_path / "in"), "output": "$x", **step}],
                   log=lambda *a: None)


def test_equal_output_type():
    e = zt.Equal(3)
    assert e.output_data_type("uint16") == ("bool", False)  # equal.rs:121-123
    e.is_compatible("float64", "bool")
    e.is_compatible("int8", "uint8")
    for dt in ("int8", "uint16", "float32", "float64"):
        with pytest.raises(zt.UnsupportedDataType):
            e.is_compatible("uint8", dt)
    with pytest.raises(zt.UnsupportedDataType):
        e.is_compatible("complex64", "bool")
    # output_array_builder (filter_traits.rs:47-82): an explicit type wins and converts the fill
    # value; else the filter's own type and fill value; the other filters keep the input's
    assert S.pointwise_output(e, "uint16") == ("bool", {"fill_value": False,
                                                        "data_type": "bool"})
    assert S.pointwise_output(e, "uint16", "uint8") == ("uint8", {"data_type": "uint8"})
    assert S.pointwise_output(e, "uint16", None, {"data_type": "uint8", "separator": "."}) == (
        "uint8", {"data_type": "uint8", "separator": "."})
    assert S.pointwise_output(zt.Clamp(0, 1), "uint16") == ("uint16", None)
    assert S.pointwise_output(zt.Clamp(0, 1), "uint16", "int8") == ("int8", {"data_type": "int8"})
    for other in (zt.Reencode(), zt.Crop([0], [1]), zt.Rescale(1, 0), zt.Clamp(0, 1),
                  zt.ReplaceValue(0, 1)):
        assert other.output_data_type("uint16") is None
        for a in _abi.DTYPES:
            other.is_compatible(a, "float16")
            other.is_compatible("bfloat16", a)


def test_equal_step_creates_a_bool_array_with_fill_false(tmp_path):
    S.create_array(tmp_path / "in", "uint16", (4, 6), (2, 3), fill_value=7)
    info = S.open_array(tmp_path / "in")
    step = {"filter": "equal", "value": 7}
    f, oshape, dt = ZF._step_params(step, info)
    assert (oshape, dt) == ((4, 6), "bool")
    S.create_output(tmp_path / "in", tmp_path / "out", dt, oshape,
                    ZF.step_encoding(step, info.data_type))
    out = S.open_array(tmp_path / "out")
    assert out.data_type == "bool" and out.metadata["fill_value"] is False
    # a crop's output array has the crop's shape
    f, oshape, dt = ZF._step_params({"filter": "crop", "offset": [1, 2], "shape": [3, 4],
                                     "data_type": "float32"}, info)
    assert (oshape, dt) == ((3, 4), "float32")


def test_memory_per_chunk():
    # chunk elements x (input + output element size); reencode and crop: the output element only
    # (reencode.rs:120-126, crop.rs:152-158)
    n = 4 * 5 * 6
    for f in (zt.Rescale(1, 0), zt.Clamp(0, 1), zt.ReplaceValue(0, 1)):
        assert f.memory_per_chunk("uint16", "float64", (4, 5, 6)) == n * (2 + 8)
    assert zt.Equal(0).memory_per_chunk("float32", "bool", (4, 5, 6)) == n * (4 + 1)
    assert zt.Reencode().memory_per_chunk("uint16", "float64", (4, 5, 6)) == n * 8
    assert zt.Crop([0] * 3, [1] * 3).memory_per_chunk("uint16", "uint8", (4, 5, 6)) == n


# ---- fusion planning -----------------------------------------------------------------------------------

def test_plan_pointwise_fusion():
    names = ["gaussian", "rescale", "clamp", "equal", "guided_filter", "crop", "downsample",
             "reencode", "replace_value"]
    assert ZF.plan_pointwise_fusion(names) == [(0, 0), (1, 3), (4, 4), (5, 5), (6, 6), (7, 8)]
    assert ZF.plan_pointwise_fusion(names, fuse=False) == [(i, i) for i in range(9)]
    # a run longer than 8 ops is split: 9 -> 8 + 1, 17 -> 8 + 8 + 1
    assert ZF.plan_pointwise_fusion(["clamp"] * 9) == [(0, 7), (8, 8)]
    assert ZF.plan_pointwise_fusion(["clamp"] * 17) == [(0, 7), (8, 15), (16, 16)]
    assert ZF.plan_pointwise_fusion(["summed_area_table"] + ["crop"] * 8) == [(0, 0), (1, 8)]
    assert ZF.plan_pointwise_fusion([]) == []


def test_plan_chains_links_pointwise_steps():
    steps = [{"filter": "gaussian", "input": "in", "output": "$a"},
             {"filter": "rescale", "input": "$a", "output": "$b"},
             {"filter": "clamp", "input": "$b"},
             {"filter": "equal", "output": "out"},
             {"filter": "reencode", "input": "in", "output": "out2"}]
    assert ZF.plan_chains(steps) == [(0, 3)]
    # "$reencode0" read by two later steps is a real array: no chain through it
    steps = [{"filter": "reencode", "input": "in", "output": "$reencode0"},
             {"filter": "crop", "input": "$reencode0", "output": "$crop"},
             {"filter": "rescale", "input": "$reencode0", "output": "$r"},
             {"filter": "clamp", "output": "out"}]
    assert ZF.plan_chains(steps) == [(2, 3)]


def test_program_composes_crops_and_types():
    fs = [zt.Crop([1, 2, 3], [6, 6, 6]), zt.Rescale(2, 1), zt.Crop([1, 0, 2], [4, 6, 3]),
          zt.Equal(3)]
    p = zt.PointwiseProgram(fs, "uint16", ["uint16", "float32", "float32", "bool"], (8, 9, 10))
    assert p.offset == (2, 2, 5) and p.shape == (4, 6, 3) and p.n_ops == 4 and p.cropped
    assert [(o.kind, o.dtype_out) for o in p.ops] == [
        (_abi.PW_REENCODE, _abi.DTYPES["uint16"]), (_abi.PW_RESCALE, _abi.DTYPES["float32"]),
        (_abi.PW_REENCODE, _abi.DTYPES["float32"]), (_abi.PW_EQUAL, _abi.DTYPES["bool"])]
    assert p.ops[3].imm0 == 0x40400000  # 3 in the type equal reads: float32
    # the second crop is checked against the first one's shape, not the array's
    with pytest.raises(_abi.InvalidParameters, match="beyond the input"):
        zt.PointwiseProgram([zt.Crop([0, 0], [4, 4]), zt.Crop([1, 1], [4, 4])], "uint8",
                            ["uint8", "uint8"], (8, 8))
    p = zt.PointwiseProgram([zt.Clamp(0, 1)], "uint8", ["uint8"], (8, 8))
    assert not p.cropped and p.box() == (None, None)
    with pytest.raises(_abi.InvalidParameters, match="1 to 8"):
        zt.PointwiseProgram([zt.Clamp(0, 1)] * 9, "uint8", ["uint8"] * 9, (8,))
    with pytest.raises(zt.UnsupportedDataType):  # equal in the middle writes bool / uint8 only
        zt.PointwiseProgram([zt.Equal(1), zt.Reencode()], "uint8", ["int16", "int16"], (8,))
