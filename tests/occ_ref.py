"""numpy restatement of which chunks a store holds when empty chunks are elided (zarrs'
`store_empty_chunks = false`, the reference's default), and of the device pass that finds them.

A cell (a chunk, or an inner chunk of a shard) is empty when the storage bits of every element of
it inside the array's shape equal the fill value's bits (zarrs' FillValue::equals_all compares
bytes): a NaN fill matches only NaNs with the same payload, +0.0 does not match -0.0, bool is a
byte. Elements of an edge cell outside the array are padding and do not count.

* Unsharded array: an empty chunk has no file.
* Sharded array: an empty inner chunk adds no bytes to its shard and both words of its index
  entry are 2^64 - 1 (Zarr V3 sharding specification); the other inner chunks follow each other
  without gaps in C order of the shard's inner grid; a shard of empty inner chunks has no file.
"""
import os
import struct

import numpy as np

NONE = (1 << 64) - 1

_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def bits_of(a: np.ndarray) -> np.ndarray:
    """The storage bits of every element, as an unsigned integer array of the same shape."""
    a = np.ascontiguousarray(a)
    return a.view(_UINT[a.dtype.itemsize]).reshape(a.shape)


def occupancy(a: np.ndarray, cell_shape, fill_bits: int) -> np.ndarray:
    """uint8 map over ceil(shape / cell_shape): 1 where some element of the cell differs bitwise
    from the fill value (given as its zero-extended storage bits). The cells start at the origin;
    the last cell of an axis may be partial."""
    b = bits_of(a)
    grid = tuple(-(-n // c) for n, c in zip(a.shape, cell_shape))
    out = np.zeros(grid, dtype=np.uint8)
    if a.size == 0:
        return out
    diff = b != b.dtype.type(fill_bits & ((1 << (8 * b.dtype.itemsize)) - 1))
    # pad every axis to whole cells with "equal", then fold each cell's elements
    cell = [min(int(c), int(n)) for c, n in zip(cell_shape, a.shape)]
    padded = np.zeros([g * c for g, c in zip(grid, cell)], dtype=bool)
    padded[tuple(slice(0, n) for n in a.shape)] = diff
    split = padded.reshape([v for g, c in zip(grid, cell) for v in (g, c)])
    return split.any(axis=tuple(range(1, 2 * a.ndim, 2))).astype(np.uint8)


def chunk_files(root) -> set:
    """The chunk files under root/c as keys relative to root ("c/0/1/2")."""
    found = set()
    base = os.path.join(root, "c")
    for d, _dirs, files in os.walk(base):
        for f in files:
            found.add(os.path.relpath(os.path.join(d, f), root).replace(os.sep, "/"))
    return found


def expected_files(a: np.ndarray, chunk_shape, fill_bits: int, inner_shape=None) -> set:
    """The chunk (shard) files an elided store of `a` holds: chunks with an occupied cell."""
    occ = occupancy(a, inner_shape or chunk_shape, fill_bits)
    per = [c // i for c, i in zip(chunk_shape, inner_shape or chunk_shape)]
    grid = tuple(-(-n // c) for n, c in zip(a.shape, chunk_shape))
    keep = set()
    for idx in np.ndindex(*grid):
        sl = tuple(slice(i * p, (i + 1) * p) for i, p in zip(idx, per))
        if occ[sl].any():
            keep.add("c/" + "/".join(str(i) for i in idx))
    return keep


def all_files(shape, chunk_shape) -> set:
    grid = tuple(-(-n // c) for n, c in zip(shape, chunk_shape))
    return {"c/" + "/".join(str(i) for i in idx) for idx in np.ndindex(*grid)}


def elided_counts(a: np.ndarray, chunk_shape, fill_bits: int, inner_shape=None) -> tuple:
    """(chunk files not written, empty inner chunks inside the array's inner-chunk grid)."""
    occ = occupancy(a, inner_shape or chunk_shape, fill_bits)
    n_files = len(all_files(a.shape, chunk_shape)) - len(
        expected_files(a, chunk_shape, fill_bits, inner_shape))
    return n_files, int(occ.size - occ.sum())


def shard_index(path, n_inner: int) -> np.ndarray:
    """The (offset, nbytes) pairs of a shard file whose index lies at its end: the last
    16 * n_inner + 4 bytes (little-endian u64 pairs, then the crc32c of the index)."""
    with open(path, "rb") as f:
        data = f.read()
    tail = data[len(data) - (16 * n_inner + 4):]
    words = struct.unpack("<%dQ" % (2 * n_inner), tail[:16 * n_inner])
    return np.array(words, dtype=np.uint64).reshape(n_inner, 2), len(data)


def check_shard(path, occ_of_shard: np.ndarray) -> None:
    """The shard at `path` against the flags of its inner chunks (C order of the shard's inner
    grid, 0 for inner chunks outside the array): (2^64-1, 2^64-1) exactly at the empty ones, the
    others contiguous from offset 0 in C order, the index right after them."""
    flags = occ_of_shard.reshape(-1)
    idx, size = shard_index(path, flags.size)
    at = 0
    for c, f in enumerate(flags):
        o, n = int(idx[c, 0]), int(idx[c, 1])
        if not f:
            assert (o, n) == (NONE, NONE), (path, c, o, n)
        else:
            assert o == at and 0 < n < NONE, (path, c, o, n, at)
            at += n
    assert at + 16 * flags.size + 4 == size, (path, at, size)


def check_shards(root, a: np.ndarray, shard_shape, inner_shape, fill_bits: int) -> None:
    """Every shard of an elided store of `a`: present exactly when it has an occupied inner chunk,
    and then with the index check_shard expects."""
    occ = occupancy(a, inner_shape, fill_bits)
    per = [s // i for s, i in zip(shard_shape, inner_shape)]
    grid = tuple(-(-n // s) for n, s in zip(a.shape, shard_shape))
    assert chunk_files(root) == expected_files(a, shard_shape, fill_bits, inner_shape)
    for sidx in np.ndindex(*grid):
        full = np.zeros(per, dtype=np.uint8)  # inner chunks beyond the array stay 0
        sl = tuple(slice(i * p, (i + 1) * p) for i, p in zip(sidx, per))
        part = occ[sl]
        full[tuple(slice(0, n) for n in part.shape)] = part
        path = os.path.join(root, "c", *[str(i) for i in sidx])
        if full.any():
            check_shard(path, full)
        else:
            assert not os.path.exists(path), path
