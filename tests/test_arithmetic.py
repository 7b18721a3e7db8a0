"""CPU: the two-array arithmetic filter without device work: the numpy restatement the GPU tests
check against (tests/arith_ref.py) pinned by hand-written answers, the command and run-config
grammar, the chain planning around a step with a second input, and the operator surface.

The reference has no such filter; the semantics are fixed in DESIGN.md §3.12: both operands `as
f64`, one IEEE f64 operation, the result `as TOut` (float -> integer saturates, NaN -> 0).
"""
import numpy as np
import pytest

import zarrs_tools_amd as zt
from tests import arith_ref as A
from zarrs_tools_amd import _abi
from zarrs_tools_amd import store as S
from zarrs_tools_amd import zarrs_filter as ZF

QUIET = dict(log=lambda *a: None)


def one(a, da, b, db, op, dout=None):
    st = {"uint8": np.uint8, "int8": np.int8, "float32": np.float32, "uint64": np.uint64,
          "int64": np.int64}
    out = A.arithmetic(np.array([a], dtype=st[da]), da, np.array([b], dtype=st[db]), db, op, dout)
    return out[0]


# ---- hand-written answers pin the restatement ------------------------------------------------------

def test_integer_results_saturate_and_truncate():
    assert one(200, "uint8", 100, "uint8", "add") == 255          # 300 as u8
    assert one(3, "uint8", 5, "uint8", "subtract") == 0           # -2 as u8
    assert one(-100, "int8", 100, "int8", "subtract") == -128     # -200 as i8
    assert one(7, "uint8", 2, "uint8", "divide") == 3             # 3.5 truncates toward zero
    assert one(-7, "int8", 2, "int8", "divide") == -3             # -3.5 truncates toward zero
    assert one(3, "uint8", 5, "uint8", "absolute_difference") == 2
    assert one(20, "uint8", 20, "uint8", "multiply") == 255       # 400 as u8


def test_division_by_zero_and_nan():
    assert one(1, "float32", 0, "float32", "divide") == np.inf
    assert np.isnan(one(0, "float32", 0, "float32", "divide"))
    assert one(0, "float32", 0, "float32", "divide", "uint8") == 0   # NaN as u8
    assert one(1, "float32", 0, "float32", "divide", "uint8") == 255  # +inf as u8


def test_minimum_and_maximum_are_a_compare_and_a_select():
    nan = np.float32(np.nan)
    assert np.isnan(one(nan, "float32", 1, "float32", "minimum"))    # 1 < NaN is false: x
    assert one(1, "float32", nan, "float32", "minimum") == 1.0       # NaN < 1 is false: x
    assert np.isnan(one(nan, "float32", 1, "float32", "maximum"))
    assert one(1, "float32", nan, "float32", "maximum") == 1.0
    r = one(-0.0, "float32", 0.0, "float32", "maximum")              # +0 > -0 is false: x
    assert r == 0.0 and np.signbit(r)
    r = one(0.0, "float32", -0.0, "float32", "minimum")              # -0 < +0 is false: x
    assert r == 0.0 and not np.signbit(r)
    assert one(3, "uint8", 5, "uint8", "minimum") == 3 and one(3, "uint8", 5, "uint8",
                                                                "maximum") == 5


def test_64_bit_integers_round_through_f64():
    # 2^64 - 1 rounds up to 2^64 as f64, then saturates back to 2^64 - 1
    assert int(one(2 ** 64 - 1, "uint64", 0, "uint64", "add")) == 2 ** 64 - 1
    # 2^53 + 1 is a tie between 2^53 and 2^53 + 2: to even
    assert int(one(2 ** 53 + 1, "int64", 0, "int64", "add")) == 2 ** 53
    assert int(one(2 ** 53 + 3, "int64", 0, "int64", "add")) == 2 ** 53 + 4


def test_default_output_type_is_the_firsts_and_f32_equals_the_f32_operation():
    a = np.array([1.1, 2.5, -3.75, 1e-30], dtype=np.float32)
    b = np.array([0.3, 7.0, 1e10, 3e-20], dtype=np.float32)
    for op, f in (("add", np.add), ("subtract", np.subtract), ("multiply", np.multiply),
                  ("divide", np.divide)):
        out = A.arithmetic(a, "float32", b, "float32", op)
        assert out.dtype == np.float32
        # f64 carries more than 2 * 24 + 2 bits: the double rounding is the f32 operation
        assert out.tobytes() == f(a, b).tobytes()
    u = np.array([0, 1, 2, 255], dtype=np.uint8)
    assert A.arithmetic(a, "float32", u, "uint8", "add", "int16").tolist() == [1, 3, -1, 255]
    assert A.OPERATORS == zt.ARITHMETIC_OPERATORS


# ---- command and run-config grammar ----------------------------------------------------------------

def _step(argv):
    steps = ZF._steps_from_cli(ZF.build_parser().parse_args(argv))
    assert len(steps) == 1
    return steps[0]


def test_subcommand_grammar():
    st = _step(["arithmetic", "a", "o", "subtract", "b"])
    assert (st["filter"], st["input"], st["output"], st["operator"], st["other"]) == (
        "arithmetic", "a", "o", "subtract", "b")
    assert st["data_type"] is None
    st = _step(["arithmetic", "a", "o", "absolute-difference", "b", "--data-type", "float32",
                "-s", "16,16", "-c", "4,4", "-f", "-1.5"])
    assert st["operator"] == "absolute_difference" and st["data_type"] == "float32"
    assert st["shard_shape"] == [16, 16] and st["chunk_shape"] == [4, 4]
    assert st["fill_value"] == -1.5
    for name in zt.ARITHMETIC_OPERATORS:
        assert _step(["arithmetic", "a", "o", name.replace("_", "-"), "b"])["operator"] == name
    with pytest.raises(SystemExit):
        ZF.build_parser().parse_args(["arithmetic", "a", "o", "power", "b"])
    with pytest.raises(SystemExit):  # OTHER is required
        ZF.build_parser().parse_args(["arithmetic", "a", "o", "add"])


def test_run_config_keys():
    assert ZF.arithmetic_args({"filter": "arithmetic", "operator": "absolute_difference",
                               "other": "$b"}) == ("absolute_difference", "$b")
    assert ZF.arithmetic_args({"operator": "absolute-difference", "other": "p"})[0] == (
        "absolute_difference")
    with pytest.raises(_abi.InvalidParameters, match="arithmetic needs other"):
        ZF.arithmetic_args({"filter": "arithmetic", "operator": "add"})
    with pytest.raises(_abi.InvalidParameters, match="arithmetic needs operator"):
        ZF.arithmetic_args({"filter": "arithmetic", "other": "x"})
    with pytest.raises(_abi.InvalidParameters, match="arithmetic needs operator, other"):
        ZF.arithmetic_args({"filter": "arithmetic"})
    with pytest.raises(_abi.InvalidParameters, match="unknown operator"):
        ZF.arithmetic_args({"filter": "arithmetic", "operator": "power", "other": "x"})


def test_the_filter_is_on_the_path_and_not_per_element():
    assert "arithmetic" in ZF.ON_PATH and ZF.BINARY == ("arithmetic",)
    assert ZF.rows_splittable("arithmetic")
    assert "arithmetic" not in ZF.POINTWISE


def test_a_missing_other_or_an_unwritten_temporary_fails_the_run(tmp_path):
    S.create_array(tmp_path / "in", "uint8", (4,), (4,))
    src = str(tmp_path / "in")
    with pytest.raises(_abi.InvalidParameters, match="arithmetic needs other"):
        ZF.run([{"filter": "arithmetic", "input": src, "output": "$x", "operator": "add"}],
               **QUIET)
    with pytest.raises(_abi.InvalidParameters, match=r"other \$b is not the output"):
        ZF.run([{"filter": "arithmetic", "input": src, "output": "$x", "operator": "add",
                 "other": "$b"}], **QUIET)
    # written, but by a later step
    with pytest.raises(_abi.InvalidParameters, match=r"other \$b is not the output"):
        ZF.run([{"filter": "arithmetic", "input": src, "output": "$x", "operator": "add",
                 "other": "$b"},
                {"filter": "reencode", "input": src, "output": "$b"}], **QUIET)
    assert not (tmp_path / "x").exists()


# ---- chain planning ------------------------------------------------------------------------------------

def test_a_temporary_read_as_other_is_not_swallowed_by_a_chain():
    steps = [{"filter": "gaussian", "input": "in", "output": "$a"},
             {"filter": "rescale", "output": "$b"},
             {"filter": "arithmetic", "input": "$b", "other": "$a", "operator": "subtract",
              "output": "out"}]
    assert ZF.plan_chains(steps) == []
    # the same config without the arithmetic step plans as before: one chain over both steps
    assert ZF.plan_chains(steps[:2]) == [(0, 1)]
    # an arithmetic step ends the chain before it and starts none
    steps = [{"filter": "gaussian", "input": "in", "output": "$a"},
             {"filter": "rescale", "input": "$a", "output": "$b"},
             {"filter": "arithmetic", "input": "$b", "other": "in", "operator": "add"},
             {"filter": "clamp"},
             {"filter": "equal", "output": "out"}]
    assert ZF.plan_chains(steps) == [(0, 1), (3, 4)]
    # configs without the new key plan exactly as before
    steps = [{"filter": "gaussian", "input": "in", "output": "$a"},
             {"filter": "rescale", "input": "$a", "output": "$b"},
             {"filter": "clamp", "input": "$b"},
             {"filter": "equal", "output": "out"},
             {"filter": "reencode", "input": "in", "output": "out2"}]
    assert ZF.plan_chains(steps) == [(0, 3)]


# ---- the operator surface -------------------------------------------------------------------------------

def test_is_compatible_memory_per_chunk_and_names():
    f = zt.Arithmetic("subtract")
    assert f.name() == "arithmetic" and f.operator == "subtract"
    assert zt.Arithmetic("absolute-difference").operator == "absolute_difference"
    for a in _abi.DTYPES:
        f.is_compatible(a, "float32", a)
        f.is_compatible("uint8", a, "bfloat16")
        f.is_compatible("bool", "int64", a)
    with pytest.raises(zt.UnsupportedDataType):
        f.is_compatible("uint8", "complex64", "uint8")
    with pytest.raises(zt.UnsupportedDataType):
        _abi.check(_abi.lib().zt_arithmetic_is_compatible(0, 5, 5, 99))
    with pytest.raises(zt.InvalidParameters, match="unknown operator"):
        zt.Arithmetic("power")
    for code in (-1, 7):
        with pytest.raises(zt.InvalidParameters, match="unknown arithmetic operator"):
            _abi.check(_abi.lib().zt_arithmetic_is_compatible(code, 5, 5, 5))
    # chunk elements x the sum of the three element sizes
    assert f.memory_per_chunk("uint16", "float32", "float64", (4, 5, 6)) == 120 * (2 + 4 + 8)
    assert f.memory_per_chunk("bool", "uint8", "int8", (7,)) == 21
    assert zt.ARITHMETIC_OPERATORS == ("add", "subtract", "multiply", "divide", "minimum",
                                       "maximum", "absolute_difference")
    assert [_abi.AR_OPERATORS[n] for n in zt.ARITHMETIC_OPERATORS] == list(range(7))


def test_step_params_of_an_arithmetic_step(tmp_path):
    S.create_array(tmp_path / "in", "uint16", (4, 6), (2, 3))
    info = S.open_array(tmp_path / "in")
    f, oshape, dt = ZF._step_params({"filter": "arithmetic", "operator": "add", "other": "x"},
                                    info)
    assert isinstance(f, zt.Arithmetic) and (oshape, dt) == ((4, 6), "uint16")
    _f, _s, dt = ZF._step_params({"filter": "arithmetic", "operator": "divide", "other": "x",
                                  "data_type": "float32"}, info)
    assert dt == "float32"
