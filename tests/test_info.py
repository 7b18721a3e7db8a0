"""CPU: zarrs_info (src/bin/zarrs_info.rs, src/info/range.rs, src/info/histogram.rs).

The numpy restatement of the two reductions (tests/info_ref.py) is pinned by hand-worked values;
the host functions around the kernels (bin edges, combining partial results, element decoding)
and the zarrs_info command's metadata subcommands and argument validation run without a GPU."""
import json
import math

import numpy as np
import pytest

import zarrs_tools_amd as zt
from tests import info_ref as R
from zarrs_tools_amd import _abi
from zarrs_tools_amd import filter as F
from zarrs_tools_amd import store as S
from zarrs_tools_amd import zarrs_info as ZI

# u8 0..49 once each, 49 bins on [0, 49]: x / 49 * 49 < x in f64 for x in LOW, which fall one
# bin low
HIST_0_49 = [2, 1, 0, 2, 0, 1, 1, 2, 0, 1, 1, 1, 1, 1, 1, 2, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 0, 1,
             1, 1, 2, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2]
LOW = [1, 2, 4, 8, 16, 27, 32]


# ---- the restatement, pinned ----------------------------------------------------------------------

def test_histogram_f32_hand_worked():
    v = np.array([-1, 0, 0.5, 1, 2, np.nan, np.inf], dtype=np.float32)
    edges, hist = R.histogram(v, "float32", 4, 0.0, 1.0)
    assert hist.tolist() == [3, 0, 1, 3] and hist.dtype == np.uint64
    assert edges.tolist() == [0.0, 0.25, 0.5, 0.75, 1.0]
    assert R.bins(v, "float32", 4, 0.0, 1.0).tolist() == [0, 0, 2, 3, 3, 0, 3]


def test_histogram_u8_division_rounds_seven_values_low():
    v = np.arange(50, dtype=np.uint8)
    _, hist = R.histogram(v, "uint8", 49, 0.0, 49.0)
    assert hist.tolist() == HIST_0_49 and len(HIST_0_49) == 49 and sum(HIST_0_49) == 50
    b = R.bins(v, "uint8", 49, 0.0, 49.0)
    exact = np.minimum(v.astype(np.int64), 48)
    assert np.flatnonzero(b != exact).tolist() == LOW and (b[LOW] == np.array(LOW) - 1).all()
    # a variant that multiplies by n_bins / (max - min) puts exactly those 7 elsewhere
    f = v.astype(np.float64)
    scaled = np.minimum(np.floor((f - 0.0) * (49.0 / 49.0)), 48).astype(np.int64)
    assert np.flatnonzero(scaled != b).tolist() == LOW


def test_histogram_u8_reciprocal_variant_differs_in_24_values():
    v = np.arange(256, dtype=np.uint8)
    b = R.bins(v, "uint8", 255, 0.0, 255.0)
    f = v.astype(np.float64)
    recip = np.minimum(np.floor(np.maximum((f - 0.0) * (1.0 / 255.0) * 255.0, 0.0)), 254)
    assert int(np.count_nonzero(recip.astype(np.int64) != b)) == 24


def test_histogram_max_equals_min():
    v = np.array([1.0, 2.0, 3.0, 2.0, np.nan], dtype=np.float64)
    # (x - 2) / 0: -inf -> bin 0, 0 / 0 = NaN -> bin 0, +inf -> the last bin
    assert R.bins(v, "float64", 5, 2.0, 2.0).tolist() == [0, 0, 4, 0, 0]
    _, hist = R.histogram(v, "float64", 5, 2.0, 2.0)
    assert hist.tolist() == [4, 0, 0, 0, 1]


def test_histogram_u64_goes_through_f64():
    v = np.array([2**53 + 1, 2**64 - 1, 2**63, 0], dtype=np.uint64)
    assert R.bins(v, "uint64", 4, 0.0, 2.0**64).tolist() == [0, 3, 2, 0]


def test_histogram_half_types_widen_exactly():
    f16 = np.array([0.5, -2.0, np.inf, np.nan], dtype=np.float16).view(np.uint16)
    assert R.bins(f16, "float16", 4, 0.0, 1.0).tolist() == [2, 0, 3, 0]
    bf16 = (np.array([0.5, -2.0, np.inf, np.nan], dtype=np.float32).view(np.uint32) >> 16).astype(
        np.uint16)
    assert R.bins(bf16, "bfloat16", 4, 0.0, 1.0).tolist() == [2, 0, 3, 0]


def test_range_floats():
    z = np.array([0.0, -0.0, np.nan], dtype=np.float32)
    lo, hi = R.range_(z, "float32")
    assert R.same_value(lo, -0.0) and R.same_value(hi, 0.0) and not R.same_value(lo, 0.0)
    assert R.range_(np.array([-0.0, -0.0]), "float64")[1].hex() == (-0.0).hex()
    v = np.array([np.nan, 3.5, -np.inf, np.inf, np.nan, -7.0], dtype=np.float64)
    assert R.range_(v, "float64") == (-math.inf, math.inf)
    assert R.range_(np.array([np.nan, 2.0, np.nan, -1.0], np.float32), "float32") == (-1.0, 2.0)
    assert R.range_(np.full(5, np.nan, np.float32), "float32") == (None, None)
    assert R.range_(np.zeros(0, np.float32), "float32") == (None, None)
    f16 = np.array([1.5, np.nan, -65504.0], dtype=np.float16).view(np.uint16)
    assert R.range_(f16, "float16") == (-65504.0, 1.5)


def test_range_64_bit_integers_exact():
    u = np.array([2**64 - 1, 2**64 - 2, 2**53 + 1, 1], dtype=np.uint64)
    assert R.range_(u, "uint64") == (1, 2**64 - 1)
    i = np.array([-2**63, 2**63 - 1, -2**53 - 1, 2**53 + 1], dtype=np.int64)
    assert R.range_(i, "int64") == (-2**63, 2**63 - 1)
    assert R.range_(np.array([-2**53 - 1, -2**53], np.int64), "int64") == (-2**53 - 1, -2**53)


# ---- host functions of the package ----------------------------------------------------------------

def test_bin_edges_match_the_restatement():
    for n, mn, mx in ((4, 0.0, 1.0), (49, 0.0, 49.0), (7, -3.25, 1e9), (3, 2.0, 2.0)):
        e = zt.Histogram(n, mn, mx).bin_edges()
        assert e.dtype == np.float64 and e.tobytes() == R.bin_edges(n, mn, mx).tobytes()


@pytest.mark.parametrize("args", [(0, 0.0, 1.0), (-1, 0.0, 1.0), (4, math.nan, 1.0),
                                  (4, 0.0, math.inf), (4, -math.inf, 0.0)])
def test_histogram_invalid_parameters(args):
    with pytest.raises(_abi.InvalidParameters):
        zt.Histogram(*args)


def test_is_compatible():
    for dt in R.NUMERIC:
        zt.Range().is_compatible(dt)
        zt.Histogram(4, 0.0, 1.0).is_compatible(dt)
    with pytest.raises(_abi.UnsupportedDataType):
        zt.Range().is_compatible("bool")
    with pytest.raises(_abi.UnsupportedDataType):
        zt.Histogram(4, 0.0, 1.0).is_compatible("bool")


def test_combine_ranges():
    assert zt.combine_ranges([(None, None), (3, 9), (-4, 2)]) == (-4, 9)
    assert zt.combine_ranges([(None, None), (None, None)]) == (None, None)
    assert zt.combine_ranges([]) == (None, None)
    lo, hi = zt.combine_ranges([(0.0, 0.0), (-0.0, -0.0)])
    assert R.same_value(lo, -0.0) and R.same_value(hi, 0.0)
    assert zt.combine_ranges([(1.0, math.inf), (-math.inf, 2.0)]) == (-math.inf, math.inf)
    assert zt.combine_ranges([(2**64 - 1, 2**64 - 1), (2**64 - 2, 2**64 - 2)]) == (
        2**64 - 2, 2**64 - 1)


def test_combine_histograms():
    e = zt.Histogram(3, 0.0, 3.0).bin_edges()
    a = np.array([1, 0, 2**63], dtype=np.uint64)
    b = np.array([4, 5, 2**63 - 1], dtype=np.uint64)
    edges, hist = zt.combine_histograms([(e, a), (e, b)])
    assert hist.dtype == np.uint64 and hist.tolist() == [5, 5, 2**64 - 1]
    assert edges.tolist() == e.tolist()
    with pytest.raises(_abi.InvalidParameters):
        zt.combine_histograms([(e, a), (zt.Histogram(3, 0.0, 4.0).bin_edges(), b)])


def test_element_value_inverts_element_bits():
    for dt, x in (("int8", -128), ("int16", -2), ("int64", -2**63), ("uint64", 2**64 - 1),
                  ("uint8", 255), ("float32", -0.0), ("float64", 1e300), ("float16", 65504.0),
                  ("bfloat16", -1.5), ("float32", math.inf)):
        got = F.element_value(F.element_bits(x, dt) if not (isinstance(x, float) and
                                                             math.isinf(x))
                              else F.element_bits("Infinity", dt), dt)
        assert R.same_value(got, x), (dt, x, got)


# ---- the zarrs_info command -----------------------------------------------------------------------

def run_info(capsys, *argv):
    rc = ZI.main([str(a) for a in argv])
    return rc, capsys.readouterr().out


@pytest.fixture
def arrays(tmp_path):
    plain = tmp_path / "plain.zarr"
    S.create_array(plain, "uint16", (5, 6, 7), (2, 3, 4), fill_value=7)
    named = tmp_path / "named.zarr"
    S.create_output(plain, named, encoding={
        "dimension_names": ["z", "y", "x"],
        "attributes": {"note": "hello", "_zarrs": {"version": "x"}}})
    group = tmp_path / "group.zarr"
    group.mkdir()
    (group / "zarr.json").write_text(json.dumps(
        {"zarr_format": 3, "node_type": "group", "attributes": {"a": 1, "_zarrs": {"v": 0}}}))
    return plain, named, group


def test_cli_metadata_commands(capsys, arrays):
    plain, named, _ = arrays
    for p in (plain, named):
        meta = json.load(open(p / "zarr.json"))
        rc, out = run_info(capsys, p, "metadata")
        assert rc == 0 and json.loads(out) == meta
        assert out == json.dumps(meta, indent=2) + "\n"  # pretty-printed
        rc, out = run_info(capsys, p, "metadata-v3")
        v3 = json.loads(out)
        assert rc == 0 and "_zarrs" not in v3.get("attributes", {})
        v3_expected = json.loads(json.dumps(meta))
        v3_expected.get("attributes", {}).pop("_zarrs", None)
        assert v3 == v3_expected
        rc, out = run_info(capsys, p, "attributes")
        assert rc == 0 and json.loads(out) == meta.get("attributes", {})
        rc, out = run_info(capsys, p, "shape")
        assert rc == 0 and json.loads(out) == {"shape": [5, 6, 7]}
        rc, out = run_info(capsys, p, "data-type")
        assert rc == 0 and json.loads(out) == {"data_type": "uint16"}
        rc, out = run_info(capsys, p, "fill-value")
        assert rc == 0 and json.loads(out) == {"fill_value": 7}
    assert json.load(open(named / "zarr.json"))["attributes"]["note"] == "hello"
    rc, out = run_info(capsys, plain, "dimension-names")
    assert rc == 0 and json.loads(out) == {"dimension_names": None}
    rc, out = run_info(capsys, named, "dimension-names")
    assert rc == 0 and json.loads(out) == {"dimension_names": ["z", "y", "x"]}


def test_cli_group(capsys, arrays):
    group = arrays[2]
    rc, out = run_info(capsys, group, "metadata")
    assert rc == 0 and json.loads(out)["node_type"] == "group"
    rc, out = run_info(capsys, group, "metadata-v3")
    assert rc == 0 and json.loads(out) == {"zarr_format": 3, "node_type": "group",
                                           "attributes": {"a": 1}}
    rc, out = run_info(capsys, group, "attributes")
    assert rc == 0 and json.loads(out) == {"a": 1, "_zarrs": {"v": 0}}
    for cmd, name in (("shape", "Shape"), ("data-type", "DataType"), ("fill-value", "FillValue"),
                      ("dimension-names", "DimensionNames"), ("range", "Range")):
        rc, out = run_info(capsys, group, cmd)
        assert rc == 0 and out.strip() == f"The {name} command is not supported for a group"
    rc, out = run_info(capsys, group, "histogram", "4", "0", "1")
    assert rc == 0 and out.startswith("The Histogram(HistogramParams { n_bins: 4,")
    assert out.strip().endswith("command is not supported for a group")


def test_cli_bad_path(capsys, tmp_path):
    rc, out = run_info(capsys, tmp_path / "nothing.zarr", "shape")
    assert rc != 0 and "nothing.zarr" in out
    (tmp_path / "broken.zarr").mkdir()
    (tmp_path / "broken.zarr" / "zarr.json").write_text("{not json")
    rc, out = run_info(capsys, tmp_path / "broken.zarr", "metadata")
    assert rc != 0 and out.strip()


def test_cli_histogram_zero_bins_is_an_error(capsys, arrays):
    rc, out = run_info(capsys, arrays[0], "histogram", "0", "0", "1")
    assert rc != 0 and "n_bins" in out
    rc, out = run_info(capsys, arrays[0], "histogram", "4", "0", "inf")
    assert rc != 0 and "finite" in out


def test_cli_bool_array_is_unsupported(capsys, tmp_path):
    p = tmp_path / "b.zarr"
    S.create_array(p, "bool", (4, 4), (2, 2))
    rc, out = run_info(capsys, p, "range")
    assert rc != 0 and "bool" in out
    rc, out = run_info(capsys, p, "histogram", "2", "0", "1")
    assert rc != 0 and "bool" in out
    with pytest.raises(_abi.UnsupportedDataType):
        S.range(p)


def test_json_number():
    assert ZI.json_number(math.inf) == "Infinity" and ZI.json_number(-math.inf) == "-Infinity"
    assert ZI.json_number(None) is None and ZI.json_number(2**64 - 1) == 2**64 - 1
    assert json.dumps(ZI.json_number(0.1)) == "0.1"
