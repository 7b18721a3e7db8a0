"""numpy restatement of the connected-component labelling, the semantics the
GPU path is held to bit for bit. No scipy here: tests/test_connected_components.py compares this
file with scipy.ndimage.label where scipy is installed.

An element is foreground when its value is not zero: any bit set for bool and the integers, value
!= 0 for the float types (+-0.0 background; NaNs, subnormals and infinities foreground). Two
foreground elements are neighbours when their coordinates differ by at most 1 on every axis and on
at most `connectivity` axes; nothing wraps at the array edges. Components are numbered 1 .. K in
the C order of their first elements, background is 0.

Arrays are storage arrays as the oracle holds them: bool as uint8, bfloat16 and float16 as uint16.
"""
import itertools

import numpy as np

INT_OUT = ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64")
_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def foreground(a: np.ndarray, dtype: str) -> np.ndarray:
    """The foreground mask of a storage array of data type `dtype`."""
    a = np.ascontiguousarray(a)
    bits = a.view(_UINT[a.dtype.itemsize]).reshape(a.shape)
    if dtype in ("bfloat16", "float16"):
        return (bits & np.uint16(0x7FFF)) != 0  # every encoding but +0.0 and -0.0
    if dtype == "float32":
        return a.view(np.float32).reshape(a.shape) != 0  # NaN != 0 holds
    if dtype == "float64":
        return a.view(np.float64).reshape(a.shape) != 0
    return bits != 0


def neighbour_offsets(ndim: int, connectivity: int) -> list:
    """Every offset in {-1, 0, 1}^ndim with 1 .. connectivity non-zero entries."""
    return [d for d in itertools.product((-1, 0, 1), repeat=ndim)
            if 0 < sum(1 for v in d if v) <= connectivity]


def label(fg: np.ndarray, connectivity: int = 1):
    """(labels as uint64, K) of a boolean mask, by flood fill: the mask is scanned in C order,
    every foreground element not yet labelled starts component K + 1 and the fill labels
    everything it reaches, so a component's number is the rank of its first element."""
    fg = np.asarray(fg, dtype=bool)
    nd = fg.ndim
    if nd < 1 or not 1 <= int(connectivity) <= nd:
        raise ValueError(f"connectivity {connectivity} not in [1, {nd}]")
    if fg.size == 0:
        return np.zeros(fg.shape, dtype=np.uint64), 0
    # a border of background: no bounds test, and a flat offset can never wrap into another row
    pad = np.zeros([s + 2 for s in fg.shape], dtype=bool)
    inner = tuple(slice(1, -1) for _ in range(nd))
    pad[inner] = fg
    strides = [int(np.prod(pad.shape[k + 1:])) for k in range(nd)]
    deltas = [sum(v * s for v, s in zip(d, strides))
              for d in neighbour_offsets(nd, int(connectivity))]
    flat = pad.ravel().tolist()
    lab = [0] * len(flat)
    k = 0
    for i in np.flatnonzero(pad.ravel()).tolist():
        if lab[i]:
            continue
        k += 1
        lab[i] = k
        stack = [i]
        while stack:
            j = stack.pop()
            for d in deltas:
                m = j + d
                if flat[m] and not lab[m]:
                    lab[m] = k
                    stack.append(m)
    out = np.array(lab, dtype=np.uint64).reshape(pad.shape)[inner]
    return np.ascontiguousarray(out), k


def connected_components(a: np.ndarray, dtype: str, connectivity: int = 1,
                         dtype_out: str = "uint32"):
    """(labels in dtype_out's storage, K). OverflowError when K exceeds dtype_out's maximum:
    labels never wrap."""
    if dtype_out not in INT_OUT:
        raise TypeError(f"labels need an integer type, not {dtype_out}")
    lab, k = label(foreground(a, dtype), connectivity)
    if k > np.iinfo(dtype_out).max:
        raise OverflowError(f"connected_components: {k} components do not fit {dtype_out}")
    return lab.astype(dtype_out), k


# ---- figures that both test files use -------------------------------------------------------------

def serpentine(shape):
    """One component at connectivity 1: the even rows of the last two axes in full, joined at
    alternating ends; further axes in front repeat it at even indices, joined at the origin."""
    a = np.zeros(shape, dtype=bool)
    if a.ndim == 1:
        a[:] = True
        return a
    plane = np.zeros(shape[-2:], dtype=bool)
    plane[::2] = True
    for y in range(1, shape[-2], 2):
        plane[y, -1 if (y // 2) % 2 == 0 else 0] = True
    a[...] = plane
    for ax in range(a.ndim - 2):
        odd = [slice(None)] * a.ndim
        odd[ax] = slice(1, None, 2)
        keep = a[tuple(odd)].copy()
        keep[...] = False
        keep[(Ellipsis, 0, 0)] = True
        a[tuple(odd)] = keep
    return a


def spiral(shape):
    """One component at every connectivity: a rectangular spiral path in the last two axes, one
    element wide with one element of background between its turns; further axes in front repeat
    it at even indices, joined at the origin."""
    h, w = shape[-2:]
    plane = np.zeros((h, w), dtype=bool)
    y = x = 0
    dy, dx = 0, 1
    plane[0, 0] = True
    while True:
        moved = False
        while True:
            ny, nx, ny2, nx2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if not (0 <= ny < h and 0 <= nx < w) or plane[ny, nx]:
                break
            if 0 <= ny2 < h and 0 <= nx2 < w and plane[ny2, nx2]:
                break
            y, x = ny, nx
            plane[y, x] = True
            moved = True
        if not moved:
            break
        dy, dx = dx, -dy
    a = np.zeros(shape, dtype=bool)
    a[...] = plane
    for ax in range(a.ndim - 2):
        odd = [slice(None)] * a.ndim
        odd[ax] = slice(1, None, 2)
        keep = np.zeros_like(a[tuple(odd)])
        keep[(Ellipsis, 0, 0)] = True
        a[tuple(odd)] = keep
    return a
