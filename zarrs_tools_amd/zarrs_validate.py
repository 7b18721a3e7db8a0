"""zarrs_validate — compare the data in two Zarr V3 arrays (src/bin/zarrs_validate.rs).

    zarrs_validate [--concurrent-chunks N] [--device D] FIRST SECOND

Equality is determined by the shape, the data type and the data; encoding (codecs, chunk grid,
chunk key encoding) and attributes are ignored (:18-22). The data are compared by their storage
bits on the GPU (store.compare; compare.hip). On success `Success: FIRST and SECOND match` goes
to stdout with status 0; otherwise the message goes to stderr with status 1 (:80-88).

Where this differs from the reference, deliberately: the reference stops at
whichever differing chunk a thread meets first; here everything is scanned and the region named
is the first array's chunk that holds the first differing element in C order, followed by the
number of differing elements and that element's index. Only the elements inside the shape are
compared (the reference also compares the stored padding of the first array's edge chunks).
"""
from __future__ import annotations

import argparse
import sys

from . import _abi
from .filter import ArraySubset


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(
        prog="zarrs_validate", description="Compare the data in two Zarr arrays. Equality of "
        "the arrays is determined by comparing the shape, data type, and data. Differences in "
        "encoding (e.g codecs, chunk key encoding) and attributes are ignored.")
    ap.add_argument("first", help="The path to the first zarr array.")
    ap.add_argument("second", help="The path to the second zarr array.")
    ap.add_argument("--concurrent-chunks", type=int, default=0,
                    help="Number of concurrent chunks to compare (0: bounded by memory only).")
    ap.add_argument("--device", type=int, default=0, help="The GPU the comparison runs on.")
    return ap


def chunk_region(index: int, shape, chunk_shape) -> ArraySubset:
    """The chunk of a regular grid that holds the element with C-order index `index`, clipped to
    the array's shape (Array::chunk_subset_bounded)."""
    coords = []
    for n in reversed(shape):
        coords.append(index % n)
        index //= n
    coords.reverse()
    start = tuple(c // k * k for c, k in zip(coords, chunk_shape))
    end = tuple(min(s + k, n) for s, k, n in zip(start, chunk_shape, shape))
    return ArraySubset(start, tuple(e - s for s, e in zip(start, end)))


def run(a):
    """(True, the success message) or (False, the mismatch message)."""
    from . import store
    n_diff, first = store.compare(a.first, a.second, device=a.device,
                                  chunk_limit=a.concurrent_chunks)
    if first is None:
        return True, f"Success: {a.first} and {a.second} match"
    info = store.open_array(a.first)
    region = chunk_region(first, info.shape, info.chunk_shape)
    return False, (f"Data differs in region: {region} ({n_diff} differing elements, the first "
                   f"at index {first})")


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    try:
        ok, message = run(a)
    except _abi.FilterError as e:
        ok, message = False, str(e)
    if ok:
        print(message)
        return 0
    print(message, file=sys.stderr)  # zarrs_validate.rs:84-87
    return 1


if __name__ == "__main__":
    sys.exit(main())
