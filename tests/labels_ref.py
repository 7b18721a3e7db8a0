"""numpy restatement of the per-label statistics and the label size filter, the
semantics the GPU path is held to exactly. No scipy here: tests/test_label_statistics.py compares
this file with scipy.ndimage where scipy is installed.

A label array holds 0 for background and 1 .. K for objects. For every label the statistics are
the element count, the bounding box (inclusive; -1 for an absent label), the coordinate sums and
the centroid coord_sum / count as Python's int / int (the correctly rounded quotient; NaN for an
absent label); with an intensity array also the smallest and largest non-NaN intensity (-0.0
orders below +0.0, the infinities are values) and, for the integer types of up to 32 bits, the
exact integer sum and the mean sum / count. Arrays are indexed by label - 1.

Arrays are storage arrays as the oracle holds them: bfloat16 and float16 as uint16.
"""
import numpy as np

INT_TYPES = ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64")
SUM_TYPES = ("int8", "int16", "int32", "uint8", "uint16", "uint32")
FLOAT_TYPES = ("bfloat16", "float16", "float32", "float64")


class InvalidLabels(ValueError):
    pass


def intensity_values(a: np.ndarray, dtype: str) -> np.ndarray:
    """Storage of an intensity array -> values (bfloat16 widened exactly to float32)."""
    a = np.ascontiguousarray(a)
    if dtype == "float16":
        return a.view(np.float16)
    if dtype == "bfloat16":
        return (a.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return a


def _below(a, b) -> bool:
    """a orders below b with -0.0 below +0.0."""
    return bool(a < b or (a == b and np.signbit(a) and not np.signbit(b)))


def label_statistics(labels: np.ndarray, n_labels=None, intensity=None, dtype_intensity=None,
                     origin=None) -> dict:
    """The statistics of `labels` (an integer array of rank >= 1), a plain loop over the
    foreground elements with Python-int sums."""
    labels = np.asarray(labels)
    nd = labels.ndim
    K = int(n_labels) if n_labels is not None else (max(0, int(labels.max())) if labels.size else 0)
    bad = int(((labels < 0) | (labels > K)).sum()) if labels.size else 0
    if bad:
        raise InvalidLabels(f"label_statistics: {bad} elements outside [0, {K}]")
    origin = [0] * nd if origin is None else [int(o) for o in origin]
    count = [0] * K
    cmin = [[-1] * nd for _ in range(K)]
    cmax = [[-1] * nd for _ in range(K)]
    csum = [[0] * nd for _ in range(K)]
    with_i = intensity is not None
    sums_kept = with_i and dtype_intensity in SUM_TYPES
    vals = intensity_values(intensity, dtype_intensity) if with_i else None
    valid = [False] * K
    imin, imax, isum = [0] * K, [0] * K, [0] * K
    for idx in np.argwhere(labels != 0):
        idx = tuple(int(i) for i in idx)
        j = int(labels[idx]) - 1
        count[j] += 1
        for a in range(nd):
            c = origin[a] + idx[a]
            cmin[j][a] = c if count[j] == 1 else min(cmin[j][a], c)
            cmax[j][a] = max(cmax[j][a], c)
            csum[j][a] += c
        if with_i:
            v = vals[idx]
            if sums_kept:
                isum[j] += int(v)
            if v == v:  # NaN is skipped
                if not valid[j]:
                    valid[j], imin[j], imax[j] = True, v, v
                else:
                    if _below(v, imin[j]):
                        imin[j] = v
                    if _below(imax[j], v):
                        imax[j] = v
    res = {
        "n_labels": K,
        "background": int(labels.size) - sum(count),
        "count": np.array(count, dtype=np.uint64).reshape(K),
        "bbox_min": np.array(cmin, dtype=np.int64).reshape(K, nd),
        "bbox_max": np.array(cmax, dtype=np.int64).reshape(K, nd),
        "coord_sum": np.array(csum, dtype=np.uint64).reshape(K, nd),
        "centroid": np.array([[csum[j][a] / count[j] if count[j] else float("nan")
                               for a in range(nd)] for j in range(K)],
                             dtype=np.float64).reshape(K, nd),
    }
    if with_i:
        vt = vals.dtype
        none = np.nan if vt.kind == "f" else 0
        res["intensity_dtype"] = dtype_intensity
        res["intensity_valid"] = np.array(valid, dtype=bool).reshape(K)
        res["intensity_min"] = np.array([imin[j] if valid[j] else none for j in range(K)],
                                        dtype=vt).reshape(K)
        res["intensity_max"] = np.array([imax[j] if valid[j] else none for j in range(K)],
                                        dtype=vt).reshape(K)
        if sums_kept:
            s = np.empty(K, dtype=object)
            for j in range(K):
                s[j] = isum[j]
            res["intensity_sum"] = s
            res["intensity_mean"] = np.array(
                [isum[j] / count[j] if count[j] else float("nan") for j in range(K)],
                dtype=np.float64).reshape(K)
        else:
            res["intensity_sum"] = None
            res["intensity_mean"] = None
    return res


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """Equal dtype, shape and bytes, except that any NaN equals any NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        nan = np.isnan(a)
        if not np.array_equal(nan, np.isnan(b)):
            return False
        u = f"u{a.dtype.itemsize}"
        return bool(np.array_equal(a.view(u)[~nan], b.view(u)[~nan]))
    if a.dtype == object:
        return all(type(x) is int and type(y) is int and x == y
                   for x, y in zip(a.tolist(), b.tolist()))
    return a.tobytes() == b.tobytes()


def assert_same(got: dict, want: dict) -> None:
    """Every entry of two results equal: ints as ints, arrays by their bytes."""
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k, w in want.items():
        g = got[k]
        if w is None or isinstance(w, (int, str)):
            assert g == w and type(g) is type(w), (k, g, w)
        else:
            assert isinstance(g, np.ndarray) and same_bits(g, w), (k, g, w)


def label_size_filter(labels: np.ndarray, min_size=1, max_size=None, relabel=True, dtype_out=None):
    """(out, K'): labels whose count lies in [min_size, max_size] are kept, renumbered 1 .. K' in
    increasing order of their old value with `relabel`; every other label becomes 0."""
    labels = np.asarray(labels)
    if min_size < 1 or (max_size is not None and max_size < min_size):
        raise ValueError("min_size >= 1 and max_size >= min_size")
    if labels.size and int(labels.min()) < 0:
        raise InvalidLabels("label_size_filter: the labels have a negative element")
    out_t = np.dtype(dtype_out) if dtype_out is not None else labels.dtype
    K = int(labels.max()) if labels.size else 0
    count = np.bincount(labels.reshape(-1).astype(np.int64), minlength=K + 1)
    keep = (count >= min_size) & (count <= (max_size if max_size is not None else labels.size))
    keep[0] = False
    remap = np.where(keep, np.cumsum(keep) if relabel else np.arange(K + 1), 0)
    kept = int(keep.sum())
    largest = int(remap.max()) if remap.size else 0
    if largest > np.iinfo(out_t).max:
        raise InvalidLabels(f"label_size_filter: the largest label {largest} does not fit")
    return remap[labels.astype(np.int64)].astype(out_t), kept
