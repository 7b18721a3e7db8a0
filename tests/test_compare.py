"""CPU: zarrs_validate (src/bin/zarrs_validate.rs).

The numpy restatement of the comparison (tests/cmp_ref.py) is pinned by hand-worked cases; the
host functions around the kernel (combining partial results, the command's grammar and region
arithmetic, the shape and data type checks that precede any device work) run without a GPU."""
import numpy as np
import pytest

import zarrs_tools_amd as zt
from tests import cmp_ref as C
from zarrs_tools_amd import _abi
from zarrs_tools_amd import store as S
from zarrs_tools_amd import zarrs_validate as ZV


# ---- the restatement, pinned ----------------------------------------------------------------------

def test_zero_signs_differ():
    a = np.array([1.0, 0.0, 2.0], dtype=np.float32)
    b = np.array([1.0, -0.0, 2.0], dtype=np.float32)
    assert (a == b).all()  # numerically equal
    assert C.compare(a, b) == (1, 1)


def test_nan_with_equal_bits_is_equal():
    a = np.array([0x7FC00000, 0x7FC00001, 0xFFC00000], dtype=np.uint32).view(np.float32)
    assert np.isnan(a).all()
    assert C.compare(a, a.copy()) == (0, None)


def test_nan_payloads_differ():
    a = np.array([5, 0x7FC00000, 0x7FC00000], dtype=np.uint32).view(np.float32)
    b = np.array([5, 0x7FC00001, 0xFFC00000], dtype=np.uint32).view(np.float32)
    assert C.compare(a, b) == (2, 1)
    d = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)
    e = np.array([0x7FF8000000000001], dtype=np.uint64).view(np.float64)
    assert C.compare(d, e) == (1, 0)


def test_u64_differing_in_both_words_counts_once():
    a = np.array([7, 0x0000000100000001, 9], dtype=np.uint64)
    b = np.array([7, 0x0000000200000002, 9], dtype=np.uint64)
    assert C.compare(a, b) == (1, 1)


def test_two_u16_in_one_word_count_twice():
    a = np.array([1, 2, 3, 4], dtype=np.uint16)
    b = np.array([1, 2, 30, 40], dtype=np.uint16)  # elements 2 and 3 share a 32-bit word
    assert C.compare(a, b) == (2, 2)


def test_bool_is_a_byte_and_shapes_flatten_in_c_order():
    a = np.zeros((2, 3), dtype=np.bool_)
    b = a.copy()
    b[1, 0] = True
    assert C.compare(a, b) == (1, 3)
    assert C.compare(np.zeros(0, np.uint8), np.zeros(0, np.uint8)) == (0, None)


# ---- host functions of the package ----------------------------------------------------------------

def test_combine_compares():
    assert zt.combine_compares([(0, None), (3, 40), (2, 17)]) == (5, 17)
    assert zt.combine_compares([(0, None), (0, None)]) == (0, None)
    assert zt.combine_compares([]) == (0, None)
    assert zt.combine_compares([(2**63, 2**40), (2**63, 0)]) == (2**64, 0)


def test_is_compatible():
    c = zt.Compare()
    assert c.name() == "compare"
    for dt in C.ALL_TYPES:
        c.is_compatible(dt, dt)
    with pytest.raises(_abi.InvalidParameters, match="Array data types do not match: uint16 vs "
                       "int16"):
        c.is_compatible("uint16", "int16")
    with pytest.raises(_abi.UnsupportedDataType):
        c.is_compatible("complex64", "complex64")


def test_new_header_symbols_are_exported():
    names = _abi.header_symbols()
    lib = _abi.lib()
    for n in ("zt_compare_init", "zt_compare_accumulate", "zt_compare_finish",
              "zt_store_compare"):
        assert n in names and hasattr(lib, n), n
    assert lib.zt_abi_version() == 4


# ---- the zarrs_validate command -------------------------------------------------------------------

def test_cli_grammar():
    a = ZV.build_parser().parse_args(["a.zarr", "b.zarr"])
    assert (a.first, a.second, a.concurrent_chunks, a.device) == ("a.zarr", "b.zarr", 0, 0)
    a = ZV.build_parser().parse_args(["--concurrent-chunks", "3", "--device", "1", "x", "y"])
    assert (a.first, a.second, a.concurrent_chunks, a.device) == ("x", "y", 3, 1)
    for argv in (["only_one"], ["a", "b", "c"], ["--concurrent-chunks", "many", "a", "b"]):
        with pytest.raises(SystemExit):
            ZV.build_parser().parse_args(argv)


def test_chunk_region_is_clipped_to_the_shape():
    shape, chunk = (5, 9, 11), (2, 4, 8)
    assert ZV.chunk_region(0, shape, chunk) == zt.ArraySubset((0, 0, 0), (2, 4, 8))
    last = 5 * 9 * 11 - 1  # element (4, 8, 10): the corner chunk, one element
    assert ZV.chunk_region(last, shape, chunk) == zt.ArraySubset((4, 8, 8), (1, 1, 3))
    idx = (3 * 9 + 5) * 11 + 9  # element (3, 5, 9)
    assert ZV.chunk_region(idx, shape, chunk) == zt.ArraySubset((2, 4, 8), (2, 4, 3))
    assert ZV.chunk_region(99, (100,), (7,)) == zt.ArraySubset((98,), (2,))
    assert "start=(98,)" in str(ZV.chunk_region(99, (100,), (7,)))


@pytest.fixture
def arrays(tmp_path):
    a = tmp_path / "a.zarr"
    S.create_array(a, "uint16", (5, 9, 11), (2, 4, 8))
    b = tmp_path / "b.zarr"
    S.create_array(b, "uint16", (5, 9, 12), (3, 9, 4))
    c = tmp_path / "c.zarr"
    S.create_array(c, "int16", (5, 9, 11), (3, 9, 4))
    return a, b, c


def test_store_compare_shape_mismatch(arrays):
    a, b, _ = arrays
    with pytest.raises(_abi.InvalidParameters,
                       match=r"Array shapes do not match: \[5, 9, 11\] vs \[5, 9, 12\]"):
        S.compare(a, b)


def test_store_compare_data_type_mismatch(arrays):
    a, _, c = arrays
    with pytest.raises(_abi.InvalidParameters,
                       match="Array data types do not match: uint16 vs int16"):
        S.compare(a, c)
    with pytest.raises(_abi.FilterError):
        S.compare(a, a.parent / "nothing.zarr")


def test_cli_mismatches_go_to_stderr(arrays, capsys):
    a, b, c = arrays
    assert ZV.main([str(a), str(b)]) == 1
    cap = capsys.readouterr()
    assert cap.out == "" and "Array shapes do not match: [5, 9, 11] vs [5, 9, 12]" in cap.err
    assert ZV.main([str(a), str(c)]) == 1
    cap = capsys.readouterr()
    assert cap.out == "" and "Array data types do not match: uint16 vs int16" in cap.err
