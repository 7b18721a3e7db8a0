"""numpy f32 restatement of the reference's gradient magnitude, the checker of the
gradient-magnitude tests (every intermediate is np.float32, one rounding per operation).

  triangle / difference passes     src/filter/kernel.rs:75-129
  GradientMagnitude::apply_ndarray src/filter/filters/gradient_magnitude.rs:109-147
  apply_chunk (halo 1, casts)      src/filter/filters/gradient_magnitude.rs:68-107
"""
import itertools

import numpy as np

from oracle import oracle as O

Q, H = np.float32(0.25), np.float32(0.5)


def _neighbours(v, axis):
    n = v.shape[axis]
    k = np.arange(n)
    prev = np.take(v, np.maximum(k - 1, 0), axis=axis)       # k.saturating_sub(1)
    nxt = np.take(v, np.minimum(k + 1, n - 1), axis=axis)    # min(k + 1, axis_len - 1)
    return prev, nxt


def triangle(v, axis):
    """apply_1d_triangle_filter (kernel.rs:76-102): prev * 0.25 + element * 0.5 + next * 0.25."""
    prev, nxt = _neighbours(v, axis)
    return (prev * Q + v * H) + nxt * Q


def difference(v, axis):
    """apply_1d_difference_operator (kernel.rs:105-129): 0.5 * (next - prev)."""
    prev, nxt = _neighbours(v, axis)
    return H * (nxt - prev)


def apply_ndarray(v, operator="sobel"):
    """GradientMagnitude::apply_ndarray (gradient_magnitude.rs:109-147) on an f32 block."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    g = np.zeros(v.shape, dtype=np.float32)
    with np.errstate(all="ignore"):
        for axis in range(v.ndim):
            if operator == "sobel":
                s = v
                for i in range(v.ndim):
                    s = difference(s, i) if i == axis else triangle(s, i)
            else:
                s = difference(v, axis)
            g = g + s * s
        out = np.sqrt(g)
    assert out.dtype == np.float32
    return out


def apply_chunks(v, chunk, operator="sobel", dtype_in="float32", dtype_out="float32"):
    """GradientMagnitude::apply: every output chunk from its halo-1 block (clamped to the array,
    ArraySubsetOverlap), input `as` f32, result `as` the output type. `v` holds dtype_in in the
    oracle's storage type."""
    out = np.empty(v.shape, dtype=O.NP_STORAGE[dtype_out])
    grid = [range(-(-n // c)) for n, c in zip(v.shape, chunk)]
    for idx in itertools.product(*grid):
        o0 = [i * c for i, c in zip(idx, chunk)]
        o1 = [min(s + c, n) for s, c, n in zip(o0, chunk, v.shape)]
        i0 = [max(s - 1, 0) for s in o0]
        i1 = [min(e + 1, n) for e, n in zip(o1, v.shape)]
        block = O.cast_to_f32(v[tuple(slice(a, b) for a, b in zip(i0, i1))], dtype_in)
        res = apply_ndarray(block, operator)
        res = res[tuple(slice(s - a, e - a) for s, e, a in zip(o0, o1, i0))]
        out[tuple(slice(s, e) for s, e in zip(o0, o1))] = O.cast_from_f32(res, dtype_out)
    return out


def apply_whole(v, operator="sobel", dtype_in="float32", dtype_out="float32"):
    """One pass over the whole array (what the chunk loop equals, as the halo is the reach)."""
    return O.cast_from_f32(apply_ndarray(O.cast_to_f32(v, dtype_in), operator), dtype_out)
