"""numpy restatement of the exact Euclidean distance transform, the semantics
the GPU path is held to bit for bit. No scipy here: tests/test_distance_transform.py compares this
file with scipy.ndimage.distance_transform_edt where scipy is installed.

An element is foreground when its value is not zero (tests/ccl_ref.py: any bit set for bool and
the integers, value != 0 for the float types). With one integer spacing >= 1 per axis,

    d2(p) = min over background q of sum_a spacing_a^2 * (p_a - q_a)^2,

an integer: 0 on the background, +inf everywhere when the array has no background element; nothing
wraps or replicates at the array edges. The stored element is sqrt(d2 as f64) as TOut (the
oracle's Rust-`as` cast from f64), or with `squared` d2 itself: saturated at the maximum of an
integer TOut, (d2 as f64) as TOut for a float TOut.

`squared_distance` is the restatement: one broadcast minimum per axis, no envelope logic.
`brute_force` is the definition itself over an explicit list of background coordinates in Python
integers; it pins the restatement on small arrays.

Arrays are storage arrays as the oracle holds them: bool as uint8, bfloat16 and float16 as uint16.
"""
import numpy as np

from oracle import oracle as O
from tests.ccl_ref import foreground

INF = 1 << 62  # no squared distance reaches it: B >= 2^62 is an error
OUT_TYPES = ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "bfloat16",
             "float16", "float32", "float64")
INT_OUT = OUT_TYPES[:8]


def check_spacing(spacing, ndim):
    """The spacing as a tuple of Python integers (None: all ones); ValueError as the filter's
    InvalidParameters: not an integer, below 1, or not one entry per axis."""
    if spacing is None:
        return (1,) * ndim
    sp = tuple(spacing)
    if len(sp) != ndim:
        raise ValueError(f"spacing {list(sp)} has {len(sp)} entries for rank {ndim}")
    for s in sp:
        if isinstance(s, bool) or int(s) != s or int(s) < 1:
            raise ValueError(f"spacing {s!r} is not an integer >= 1")
    return tuple(int(s) for s in sp)


def bound(shape, spacing=None) -> int:
    """B = sum_a spacing_a^2 * (n_a - 1)^2 over the axes of extent > 1, a Python integer."""
    sp = check_spacing(spacing, len(shape))
    return sum(s * s * (int(n) - 1) ** 2 for s, n in zip(sp, shape) if int(n) > 1)


def work_bytes(shape, spacing=None, force64: bool = False) -> int:
    """The width of the device's work elements: 4 when B < 2^32 - 1, else 8; ValueError from 2^62."""
    b = bound(shape, spacing)
    if b >= 1 << 62:
        raise ValueError(f"B = {b} is not below 2^62")
    return 8 if force64 or b >= (1 << 32) - 1 else 4


def memory(dtype_in, dtype_out, shape, spacing=None, force64: bool = False) -> int:
    """input + scratch + output of one call: n * (size_in + size_out) + n * (2 * W + 8), the two
    work arrays and the apex and breakpoint stacks; 0 for a zero extent."""
    n = 1
    for s in shape:
        n *= int(s)
    if n == 0:
        return 0
    size = {k: np.dtype(v).itemsize for k, v in O.NP_STORAGE.items()}
    return n * (size[dtype_in] + size[dtype_out]) + \
        n * (2 * work_bytes(shape, spacing, force64) + 8)


def squared_distance(fg: np.ndarray, spacing=None) -> np.ndarray:
    """d2 as int64, INF where there is no background at all."""
    fg = np.asarray(fg, dtype=bool)
    sp = check_spacing(spacing, fg.ndim)
    if bound(fg.shape, sp) >= 1 << 62:
        raise ValueError("B is not below 2^62")
    g = np.where(fg, np.int64(INF), np.int64(0))
    if fg.size == 0:
        return g
    for axis, s in enumerate(sp):
        n = fg.shape[axis]
        if n == 1:
            continue
        v = np.moveaxis(g, axis, -1)  # [..., j]
        i = np.arange(n, dtype=np.int64)
        # a Python-integer weight; the products stay below 2^62 by the bound, and a sentinel is
        # never added to: where(v == INF) keeps it
        cost = (np.int64(s * s) * (i[:, None] - i[None, :]) ** 2)  # [i, j]
        out = np.empty_like(v)
        for k in range(n):  # one output position at a time: memory stays n times the array / n
            cand = np.where(v == INF, np.int64(INF), v + cost[k])
            out[..., k] = np.minimum(cand.min(axis=-1), np.int64(INF))
        g = np.ascontiguousarray(np.moveaxis(out, -1, axis))
    return g


def brute_force(fg: np.ndarray, spacing=None) -> np.ndarray:
    """The definition: for every element the minimum, over an explicit list of the background
    coordinates, of the weighted squared coordinate differences in uint64 integers (B < 2^62, so
    nothing wraps). int64, INF everywhere when there is no background at all."""
    fg = np.asarray(fg, dtype=bool)
    sp = check_spacing(spacing, fg.ndim)
    if bound(fg.shape, sp) >= 1 << 62:
        raise ValueError("B is not below 2^62")
    background = np.argwhere(~fg).astype(np.int64)  # [Q, ndim]
    if len(background) == 0:
        return np.full(fg.shape, INF, dtype=np.int64)
    points = np.argwhere(np.ones(fg.shape, bool)).astype(np.int64)  # every p, in C order
    weight = np.array([s * s if n > 1 else 0 for s, n in zip(sp, fg.shape)], dtype=np.uint64)
    out = np.empty(len(points), dtype=np.uint64)
    step = max(1, (1 << 22) // len(background))
    for a in range(0, len(points), step):
        diff = np.abs(points[a:a + step, None, :] - background[None, :, :]).astype(np.uint64)
        out[a:a + step] = (diff * diff * weight).sum(axis=-1).min(axis=-1)
    return out.astype(np.int64).reshape(fg.shape)


def store(d2: np.ndarray, dtype_out: str = "float32", squared: bool = False) -> np.ndarray:
    """The output rule on an int64 d2 (INF = +inf), into dtype_out's storage type."""
    if dtype_out not in OUT_TYPES:
        raise TypeError(f"distances need a numeric type, not {dtype_out}")
    d2 = np.asarray(d2, dtype=np.int64)
    inf = d2 >= INF
    if squared and dtype_out in INT_OUT:
        most = int(np.iinfo(O.NP_STORAGE[dtype_out]).max)
        sat = np.where(inf | (d2 > min(most, INF)), most, d2.astype(np.uint64))
        return sat.astype(O.NP_STORAGE[dtype_out]).reshape(d2.shape)
    v = d2.astype(np.float64)  # round to nearest even, as the device's u64 -> f64
    if not squared:
        v = np.sqrt(v)  # IEEE: correctly rounded
    v = np.where(inf, np.inf, v)
    if dtype_out == "float64":
        return np.ascontiguousarray(v)
    if dtype_out == "float32":
        with np.errstate(over="ignore"):
            return v.astype(np.float32)
    return O.cast_from_f64(np.ascontiguousarray(v), dtype_out).reshape(d2.shape)


def distance_transform(a: np.ndarray, dtype: str, spacing=None, squared: bool = False,
                       dtype_out=None) -> np.ndarray:
    """Storage array of data type `dtype` in, storage array of dtype_out (default float32, uint32
    with `squared`) out."""
    dtype_out = dtype_out or ("uint32" if squared else "float32")
    if dtype_out not in OUT_TYPES:
        raise TypeError(f"distances need a numeric type, not {dtype_out}")
    return store(squared_distance(foreground(a, dtype), spacing), dtype_out, squared)
