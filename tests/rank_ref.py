"""numpy restatement of the rank filters (minimum, median, maximum), the checker
of the rank filter tests. The reference has no such filter: the semantics are this file's.

For output index k the window is the multiset in[clamp(k_a + i_a, 0, n_a - 1)], i_a in
[-h_a, h_a] on every axis (N = prod(2 h_a + 1) entries, edges replicate). The result is the
entry of rank 0, (N - 1) // 2 or N - 1 of the sorted window under a total order on keys:
  unsigned integers, bool   the storage bits
  signed integers           bits ^ sign bit
  floats                    bits ^ (sign ? all ones : sign bit)
compared unsigned, so -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN. The selected element
keeps its storage bits.

Arrays hold an element type in the oracle's storage type (O.NP_STORAGE: bool as u8, f16 and bf16
as raw u16 bits) next to the type's name.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from oracle import oracle as O
from tests import pw_ref

KINDS = ("minimum", "median", "maximum")
FLOATS = ("float16", "bfloat16", "float32", "float64")
SIGNED = ("int8", "int16", "int32", "int64")


def _unsigned(dt):
    return {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[
        np.dtype(O.NP_STORAGE[dt]).itemsize]


def to_key(v, dt):
    """Storage array -> unsigned order keys of the same width."""
    u = _unsigned(dt)
    bits = np.ascontiguousarray(v, dtype=O.NP_STORAGE[dt]).view(u)
    nbits = 8 * np.dtype(u).itemsize
    sign = u(1 << (nbits - 1))
    ones = u((1 << nbits) - 1)
    if dt in FLOATS:
        return bits ^ np.where(bits & sign != 0, ones, sign).astype(u)
    if dt in SIGNED:
        return bits ^ sign
    return bits.copy()


def from_key(k, dt):
    """Order keys -> storage array (the inverse of to_key)."""
    u = _unsigned(dt)
    k = np.ascontiguousarray(k, dtype=u)
    nbits = 8 * np.dtype(u).itemsize
    sign = u(1 << (nbits - 1))
    ones = u((1 << nbits) - 1)
    if dt in FLOATS:
        bits = k ^ np.where(k & sign != 0, sign, ones).astype(u)
    elif dt in SIGNED:
        bits = k ^ sign
    else:
        bits = k
    return np.ascontiguousarray(bits).view(O.NP_STORAGE[dt])


def _pick(kind, n):
    return {"minimum": 0, "median": (n - 1) // 2, "maximum": n - 1}[kind]


def apply_ndarray(v, kind, half, dt, out_subset=None):
    """The filter of a block in its own type, clamped at the block's bounds; `out_subset` =
    (start, shape) of the part to return (default: all)."""
    v = np.ascontiguousarray(v, dtype=O.NP_STORAGE[dt])
    half = tuple(int(h) for h in half)
    assert len(half) == v.ndim and all(h >= 0 for h in half) and kind in KINDS
    k = np.pad(to_key(v, dt), [(h, h) for h in half], mode="edge")
    win = sliding_window_view(k, tuple(2 * h + 1 for h in half))
    win = win.reshape(v.shape + (-1,))
    n = win.shape[-1]
    if out_subset is not None:
        start, shape = out_subset
        win = win[tuple(slice(s, s + m) for s, m in zip(start, shape))]
    sel = np.sort(win, axis=-1)[..., _pick(kind, n)]
    return from_key(sel, dt).reshape(win.shape[:-1])


def apply_chunks(v, chunk, kind, half, dt):
    """Chunk by chunk: every output chunk from its input chunk plus a halo of `half` clamped to
    the array (ArraySubsetOverlap), the block clamping at its own bounds."""
    v = np.ascontiguousarray(v, dtype=O.NP_STORAGE[dt])
    out = np.empty_like(v)
    grid = [range(0, n, c) for n, c in zip(v.shape, chunk)]
    for start in np.stack(np.meshgrid(*grid, indexing="ij"), -1).reshape(-1, v.ndim):
        stop = [min(s + c, n) for s, c, n in zip(start, chunk, v.shape)]
        lo = [max(0, s - h) for s, h in zip(start, half)]
        hi = [min(n, e + h) for e, h, n in zip(stop, half, v.shape)]
        block = v[tuple(slice(a, b) for a, b in zip(lo, hi))]
        sub = ([s - a for s, a in zip(start, lo)], [e - s for s, e in zip(start, stop)])
        out[tuple(slice(s, e) for s, e in zip(start, stop))] = apply_ndarray(
            block, kind, half, dt, sub)
    return out


def apply_separable(v, kind, half, dt):
    """Minimum / maximum as one pass per axis (they separate under a total order)."""
    assert kind in ("minimum", "maximum")
    for a, h in enumerate(half):
        one = [0] * len(half)
        one[a] = h
        v = apply_ndarray(v, kind, one, dt)
    return v


def apply_whole(v, kind, half, din, dout=None):
    """One pass over the whole array, then the `as` cast to dout (default: din)."""
    r = apply_ndarray(v, kind, half, din)
    return r if dout in (None, din) else pw_ref.reencode(r, din, dout)
