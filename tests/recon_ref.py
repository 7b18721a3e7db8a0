"""numpy restatement of morphological reconstruction, the semantics the GPU path
is held to bit for bit. No scipy here: tests/test_reconstruction.py compares this file with
scipy.ndimage.binary_propagation and binary_fill_holes where scipy is installed.

Elements are only ever selected, under the rank filters' total order (tests/rank_ref.py: to_key /
from_key): every output element carries the storage bits of some marker or mask element. Two
elements are neighbours when their coordinates differ by at most 1 on every axis and on at most
`connectivity` axes; nothing wraps or replicates at the array edges.

  by dilation   J0 = min(marker, mask); out = the least J >= J0 with
                J[p] = min(max(J[q] : q = p or a neighbour of p), mask[p]) for every p
  by erosion    the same with the order reversed = the dilation on complemented keys

A marker above the mask (below it, by erosion) is clipped by J0, not an error. The generated markers:
  fill_holes    by erosion; the mask where any coordinate is 0 or extent - 1, the type's greatest
                key elsewhere
  h_maxima(h)   by dilation; (mask as f64 - h) as T, the arithmetic filter's subtract
  h_minima(h)   by erosion; (mask as f64 + h) as T

Arrays are storage arrays as the oracle holds them: bool as uint8, bfloat16 and float16 as uint16.
"""
import itertools

import numpy as np

from tests import arith_ref
from tests.rank_ref import from_key, to_key

METHODS = ("dilation", "erosion")
MODES = ("marker", "fill_holes", "h_maxima", "h_minima")


def neighbour_offsets(ndim: int, connectivity: int) -> list:
    """Every offset in {-1, 0, 1}^ndim with 1 .. connectivity non-zero entries."""
    return [d for d in itertools.product((-1, 0, 1), repeat=ndim)
            if 0 < sum(1 for v in d if v) <= connectivity]


def _shifted(shape, d):
    """(destination slices, source slices): dst[p] pairs with src[p + d] wherever both exist."""
    dst, src = [], []
    for n, v in zip(shape, d):
        dst.append(slice(max(0, -v), n - max(0, v)))
        src.append(slice(max(0, v), n - max(0, -v)))
    return tuple(dst), tuple(src)


def sweep(j: np.ndarray, mask: np.ndarray, offsets) -> np.ndarray:
    """One Jacobi sweep on keys: min(max(J over p and its neighbours), mask)."""
    new = j.copy()
    for d in offsets:
        dst, src = _shifted(j.shape, d)
        np.maximum(new[dst], j[src], out=new[dst])
    return np.minimum(new, mask)


def reconstruct_keys(j0: np.ndarray, mask: np.ndarray, connectivity: int):
    """(fixed point, sweeps) of the dilation on unsigned keys, from J0 <= mask."""
    nd = mask.ndim
    if nd < 1 or not 1 <= int(connectivity) <= nd:
        raise ValueError(f"connectivity {connectivity} not in [1, {nd}]")
    offsets = neighbour_offsets(nd, int(connectivity))
    j, sweeps = j0, 0
    while j.size:
        sweeps += 1
        new = sweep(j, mask, offsets)
        if np.array_equal(new, j):
            break
        j = new
    return j, sweeps


def reconstruct(mask, marker, dt: str, method: str = "dilation", connectivity: int = 1,
                with_sweeps: bool = False):
    """The reconstruction of `marker` under `mask` (storage arrays of data type `dt`)."""
    assert method in METHODS, method
    assert np.shape(mask) == np.shape(marker), (np.shape(mask), np.shape(marker))
    km, kj = to_key(mask, dt), to_key(marker, dt)
    if method == "erosion":  # the dilation on complemented keys
        km, kj = ~km, ~kj
    out, sweeps = reconstruct_keys(np.minimum(kj, km), km, connectivity)
    if method == "erosion":
        out = ~out
    out = from_key(out, dt).reshape(np.shape(mask))
    return (out, sweeps) if with_sweeps else out


def border(shape) -> np.ndarray:
    """True where any coordinate is 0 or extent - 1."""
    b = np.zeros(shape, dtype=bool)
    for a in range(len(shape)):
        idx = [slice(None)] * len(shape)
        for at in (0, -1):
            idx[a] = at
            b[tuple(idx)] = True
    return b


def fill_holes_marker(mask, dt: str) -> np.ndarray:
    """The mask on the array's border, the type's greatest key elsewhere."""
    k = to_key(mask, dt)
    greatest = np.full_like(k, np.iinfo(k.dtype).max)
    return from_key(np.where(border(np.shape(mask)), k, greatest), dt).reshape(np.shape(mask))


def h_marker(mask, dt: str, h: float, sign: int) -> np.ndarray:
    """(mask as f64 + sign * h) as T: the arithmetic filter with a constant second operand."""
    if dt == "bool" or not (np.isfinite(h) and h > 0):
        raise ValueError("h modes need a numeric type and a finite h > 0")
    other = np.full(np.shape(mask), float(h), dtype=np.float64)
    return arith_ref.arithmetic(mask, dt, other, "float64", "subtract" if sign < 0 else "add", dt)


def apply(mask, dt: str, mode: str = "marker", marker=None, method: str = "dilation",
          connectivity: int = 1, h=None) -> np.ndarray:
    """Reconstruction as the filter offers it: `mode` one of MODES."""
    assert mode in MODES, mode
    if mode == "marker":
        return reconstruct(mask, marker, dt, method, connectivity)
    if mode == "fill_holes":
        return reconstruct(mask, fill_holes_marker(mask, dt), dt, "erosion", connectivity)
    if mode == "h_maxima":
        return reconstruct(mask, h_marker(mask, dt, h, -1), dt, "dilation", connectivity)
    return reconstruct(mask, h_marker(mask, dt, h, +1), dt, "erosion", connectivity)
