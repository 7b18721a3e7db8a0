"""CPU half of the connected-component labelling: the numpy restatement
tests/ccl_ref.py against hand-written answers and, where scipy is installed, against
scipy.ndimage.label; and everything of the feature that needs no GPU: the command and run-config
grammar, the chain planner, the type rules, the connectivity limits, the memory formula and the
exported symbols."""
import numpy as np
import pytest

from tests import ccl_ref as C

import zarrs_tools_amd as zt
from zarrs_tools_amd import _abi
from zarrs_tools_amd import zarrs_filter as ZF

ALL = list(_abi.DTYPES)
SIZE = {"bool": 1, "int8": 1, "uint8": 1, "int16": 2, "uint16": 2, "bfloat16": 2, "float16": 2,
        "int32": 4, "uint32": 4, "float32": 4, "int64": 8, "uint64": 8, "float64": 8}


# ---- the checker itself ------------------------------------------------------------------------

def test_faces_give_three_components_and_the_full_neighbourhood_one():
    fig = np.array([[1, 1, 0, 0, 0],
                    [0, 0, 1, 0, 0],
                    [0, 0, 1, 1, 0],
                    [0, 0, 0, 0, 1]], dtype=bool)
    lab, k = C.label(fig, 1)
    assert k == 3
    assert lab.tolist() == [[1, 1, 0, 0, 0],
                            [0, 0, 2, 0, 0],
                            [0, 0, 2, 2, 0],
                            [0, 0, 0, 0, 3]]
    lab, k = C.label(fig, 2)
    assert k == 1 and np.array_equal(lab, fig.astype(np.uint64))


def test_components_are_numbered_by_their_first_element():
    # the U reaches (0, 4) before the dot at (0, 6) starts, though most of it lies further on;
    # the bar of the last row is found last
    fig = np.array([[0, 0, 0, 0, 1, 0, 1],
                    [1, 0, 0, 0, 1, 0, 0],
                    [1, 1, 1, 1, 1, 0, 0],
                    [0, 0, 0, 0, 0, 0, 0],
                    [1, 1, 0, 0, 0, 0, 0]], dtype=bool)
    lab, k = C.label(fig, 1)
    assert k == 3
    assert lab.tolist() == [[0, 0, 0, 0, 1, 0, 2],
                            [1, 0, 0, 0, 1, 0, 0],
                            [1, 1, 1, 1, 1, 0, 0],
                            [0, 0, 0, 0, 0, 0, 0],
                            [3, 3, 0, 0, 0, 0, 0]]
    # nothing wraps: the last element of a row and the first of the next are no neighbours
    lab, k = C.label(np.array([[0, 0, 1], [1, 0, 0]], dtype=bool), 1)
    assert k == 2 and lab.tolist() == [[0, 0, 1], [2, 0, 0]]
    # 1-D, and connectivity limits
    lab, k = C.label(np.array([1, 1, 0, 1, 0, 0, 1, 1, 1], dtype=bool), 1)
    assert k == 3 and lab.tolist() == [1, 1, 0, 2, 0, 0, 3, 3, 3]
    for c in (0, 3):
        with pytest.raises(ValueError):
            C.label(np.ones((2, 2), dtype=bool), c)
    lab, k = C.label(np.zeros((3, 0, 4), dtype=bool), 2)
    assert k == 0 and lab.shape == (3, 0, 4)


def test_foreground_rules_per_type():
    def fg(values, np_type, dtype):
        return C.foreground(np.array(values, dtype=np_type), dtype).tolist()

    # floats: value != 0, so both zeros are background and NaN, subnormals, infinities are not
    tiny32, tiny64 = np.float32(1e-45), 5e-324
    assert fg([0.0, -0.0, np.nan, -np.nan, tiny32, np.inf, -np.inf, 1.0], np.float32,
              "float32") == [False, False, True, True, True, True, True, True]
    assert fg([0.0, -0.0, np.nan, tiny64, -np.inf], np.float64,
              "float64") == [False, False, True, True, True]
    # the 16-bit floats as storage bits: 0x8000 is -0.0
    assert fg([0x0000, 0x8000, 0x0001, 0x8001, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x3C00], np.uint16,
              "float16") == [False, False, True, True, True, True, True, True, True]
    assert fg([0x0000, 0x8000, 0x0001, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x3F80], np.uint16,
              "bfloat16") == [False, False, True, True, True, True, True, True]
    # integers: any bit, also the high ones of the 8-byte types; 0x8000 is a value here
    assert fg([0, 1 << 32, 1 << 63, 1], np.uint64, "uint64") == [False, True, True, True]
    assert fg([0, 1 << 32, -(1 << 63), -1], np.int64, "int64") == [False, True, True, True]
    assert fg([0, 0x8000, 1], np.uint16, "uint16") == [False, True, True]
    assert fg([0, -128, 127], np.int8, "int8") == [False, True, True]
    assert fg([0, 1], np.uint8, "bool") == [False, True]


def test_labels_never_wrap_in_the_restatement():
    dots = np.zeros((2, 600), dtype=np.uint8)
    dots[0, ::2] = 1  # 300 isolated elements
    lab, k = C.connected_components(dots, "uint8", 1, "uint16")
    assert k == 300 and lab.dtype == np.uint16 and lab.max() == 300
    with pytest.raises(OverflowError, match="300 components do not fit uint8"):
        C.connected_components(dots, "uint8", 1, "uint8")
    with pytest.raises(TypeError):
        C.connected_components(dots, "uint8", 1, "float32")


SCIPY_SHAPES = [(37,), (9, 70), (5, 33, 67), (3, 4, 9, 17)]


@pytest.mark.parametrize("shape", SCIPY_SHAPES)
def test_restatement_agrees_with_scipy(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(len(shape))
    figures = [rng.random(shape) < d for d in (0.3, 0.6, 0.9)] + [C.serpentine(shape)]
    for c in range(1, len(shape) + 1):
        structure = ndi.generate_binary_structure(len(shape), c)
        for fig in figures:
            want, k_want = ndi.label(fig, structure)
            got, k = C.label(fig, c)
            assert k == k_want
            assert np.array_equal(got, want.astype(np.uint64))
    assert C.label(C.serpentine(shape), 1)[1] == 1


# ---- the feature ---------------------------------------------------------------------------------

def test_subcommand_grammar():
    p = ZF.build_parser()
    a = p.parse_args(["connected-components", "in", "out"])
    assert ZF._steps_from_cli(a) == [{"filter": "connected_components", "input": "in",
                                      "output": "out", "connectivity": 1, "data_type": None,
                                      "chunk_limit": None}]
    a = p.parse_args(["connected-components", "in", "out", "--connectivity", "3", "--data-type",
                      "uint16", "-c", "16,16,16", "--skip-empty-chunks"])
    step = ZF._steps_from_cli(a)[0]
    assert step["connectivity"] == 3 and step["data_type"] == "uint16"
    assert step["chunk_shape"] == [16, 16, 16] and a.filter_skip_empty_chunks
    with pytest.raises(SystemExit):
        p.parse_args(["connected-components", "in"])
    with pytest.raises(SystemExit):
        p.parse_args(["connected-components", "in", "out", "--connectivity", "faces"])


def test_on_path_and_rows():
    assert "connected_components" in ZF.ON_PATH
    assert ZF.rows_splittable("connected_components") is False
    assert ZF.rows_splittable("summed_area_table") is False
    assert ZF.rows_splittable("gaussian") is True


def test_run_config_step_and_chain_planning():
    steps = [{"filter": "equal", "input": "in", "value": 3},
             {"filter": "connected_components", "connectivity": 2},
             {"filter": "downsample", "stride": [2, 2, 2], "discrete": True, "output": "out"}]
    assert ZF.plan_chains(steps) == [(0, 2)]
    steps = [{"filter": "equal", "input": "in", "value": 3, "output": "$mask"},
             {"filter": "connected_components", "input": "$mask", "output": "out"}]
    assert ZF.plan_chains(steps) == [(0, 1)]
    assert ZF.connectivity_of({"filter": "connected_components"}) == 1
    assert ZF.connectivity_of({"filter": "connected_components", "connectivity": "2"}) == 2
    with pytest.raises(zt.InvalidParameters, match="not an integer"):
        ZF.connectivity_of({"filter": "connected_components", "connectivity": "faces"})


def test_step_params_and_output_encoding():
    from zarrs_tools_amd import store as S
    info = S.ArrayInfo("in", "bool", (20, 30, 40), (8, 8, 8), (8, 8, 8))
    f, shape, dt = ZF._step_params({"filter": "connected_components", "connectivity": 3}, info)
    assert isinstance(f, zt.ConnectedComponents) and f.connectivity == 3
    assert shape == (20, 30, 40) and dt == "uint32"  # whatever the input type
    f, shape, dt = ZF._step_params({"filter": "connected_components", "data_type": "int16"}, info)
    assert f.connectivity == 1 and dt == "int16"
    for c in (0, 4, -1):
        with pytest.raises(zt.InvalidParameters, match="connectivity"):
            ZF._step_params({"filter": "connected_components", "connectivity": c}, info)
    with pytest.raises(zt.UnsupportedDataType):
        ZF._step_params({"filter": "connected_components", "data_type": "float32"}, info)
    # the output array: uint32 with fill value 0 unless given
    assert ZF.step_encoding({"filter": "connected_components"}, "float32") == {
        "data_type": "uint32", "fill_value": 0}
    enc = ZF.step_encoding({"filter": "connected_components", "data_type": "uint8",
                            "fill_value": 9, "chunk_shape": "4,4,4"}, "float32")
    assert enc == {"data_type": "uint8", "fill_value": 9, "chunk_shape": [4, 4, 4]}


def test_is_compatible_thirteen_in_eight_out():
    f = zt.ConnectedComponents()
    assert f.name() == "connected components" and f.connectivity == 1
    for din in ALL:
        for dout in C.INT_OUT:
            f.is_compatible(din, dout)
        for dout in ("bool", "bfloat16", "float16", "float32", "float64"):
            with pytest.raises(zt.UnsupportedDataType, match="integer output type"):
                f.is_compatible(din, dout)
    with pytest.raises(zt.UnsupportedDataType):
        f.is_compatible("complex64", "uint32")
    with pytest.raises(zt.UnsupportedDataType):
        f.is_compatible("uint8", "uint128")


def test_connectivity_limits():
    with pytest.raises(zt.InvalidParameters, match=r"connectivity 0 not in \[1, rank\]"):
        zt.ConnectedComponents(0)
    for rank in (1, 2, 3, 5):
        shape = (3,) * rank
        zt.ConnectedComponents(rank).memory("uint8", "uint32", shape)
        with pytest.raises(zt.InvalidParameters,
                           match=rf"connectivity {rank + 1} not in \[1, {rank}\]"):
            zt.ConnectedComponents(rank + 1).memory("uint8", "uint32", shape)
        with pytest.raises(zt.InvalidParameters):
            zt.ConnectedComponents(rank + 1).check_connectivity(rank)


def test_memory_formula_for_both_index_widths(monkeypatch):
    """input + scratch + output; scratch = two index arrays and the fixed tail (K and the offset
    table of the rank's full neighbourhood). The index is 32 bits below 2^32 - 1 elements."""
    assert _abi.cc_tail_bytes(1) == 64 + 16 * 1 and _abi.cc_tail_bytes(3) == 64 + 16 * 13
    assert _abi.cc_tail_bytes(8) == 64 + 16 * 3280
    f = zt.ConnectedComponents()
    monkeypatch.delenv("ZT_CC_INDEX64", raising=False)
    cases = [("uint8", "uint32", (70, 45, 67), 4), ("float64", "uint8", (9, 70), 4),
             ("bool", "int64", (1000,), 4), ("uint16", "uint16", (3, 4, 9, 17), 4),
             ("uint8", "uint32", (1024, 1024, 1024), 4),
             ("uint8", "uint32", (1, 2, 2147483647), 4),  # 2^32 - 2 elements: still 32 bits
             ("uint8", "uint32", (3, 1431655765), 8),     # 2^32 - 1
             ("uint16", "uint32", (2048, 2048, 2048), 8)]
    for din, dout, shape, width in cases:
        n = int(np.prod([int(s) for s in shape], dtype=object))
        want = n * (SIZE[din] + SIZE[dout] + 2 * width) + _abi.cc_tail_bytes(len(shape))
        assert f.memory(din, dout, shape) == want, (din, dout, shape)
    assert f.memory("uint8", "uint32", (5, 0, 7)) == 0
    # the knob forces the 64-bit index at any size
    monkeypatch.setenv("ZT_CC_INDEX64", "1")
    assert f.memory("uint8", "uint32", (70, 45, 67)) == 70 * 45 * 67 * (1 + 4 + 16) + \
        _abi.cc_tail_bytes(3)
    monkeypatch.setenv("ZT_CC_INDEX64", "0")
    assert f.memory("uint8", "uint32", (70, 45, 67)) == 70 * 45 * 67 * (1 + 4 + 8) + \
        _abi.cc_tail_bytes(3)


def test_symbols_tile_and_export():
    syms = _abi.header_symbols()
    for name in ("zt_connected_components_is_compatible", "zt_connected_components_memory",
                 "zt_connected_components_apply_array"):
        assert name in syms
        assert hasattr(_abi.lib(), name)
    text = open(_abi.HEADER_PATH).read()
    for axis, extent in zip("ZYX", _abi.CC_TILE):
        assert f"#define ZT_CC_TILE_{axis} {extent}\n" in text
    assert "ConnectedComponents" in zt.__all__
    # the read and write helpers moved; their old home still offers them
    from zarrs_tools_amd import device_io
    assert ZF.read_to_device is device_io.read_to_device
    assert ZF.write_from_device is device_io.write_from_device
