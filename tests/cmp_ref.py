"""numpy restatement of zarrs_validate's comparison (src/bin/zarrs_validate.rs:145-147,
`bytes_first == bytes_second`) on storage arrays (float16 / bfloat16 as raw uint16, bool as a
byte): the elements are compared by their storage bits, as unsigned integers of their size."""
import numpy as np

ALL_TYPES = ("bool", "int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64",
             "bfloat16", "float16", "float32", "float64")
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def bits(v: np.ndarray) -> np.ndarray:
    """The elements of v, flattened in C order, as unsigned integers of the element size."""
    v = np.ascontiguousarray(v)
    return v.reshape(-1).view(UINT[v.dtype.itemsize])


def compare(a: np.ndarray, b: np.ndarray):
    """(the number of elements whose bits differ, the C-order index of the first or None)."""
    assert a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize
    bad = np.flatnonzero(bits(a) != bits(b))
    return int(bad.size), (int(bad[0]) if bad.size else None)
