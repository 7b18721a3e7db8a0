"""numpy restatement of zarrs_info's reductions (src/info/histogram.rs:51-68 as written;
src/info/range.rs with the documented meaning) on storage arrays (float16 /
bfloat16 as raw uint16, oracle.NP_STORAGE). Everything is f64 arithmetic, one rounding per
operation."""
import math

import numpy as np

FLOATS = ("bfloat16", "float16", "float32", "float64")
NUMERIC = ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64") + FLOATS


def to_f64(v: np.ndarray, dtype: str) -> np.ndarray:
    """`x as f64`: exact for every type but the 64-bit integers (round to nearest even)."""
    v = np.asarray(v)
    if dtype == "bfloat16":
        return (v.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    if dtype == "float16":
        return v.view(np.float16).astype(np.float64)
    return v.astype(np.float64)


def bins(v: np.ndarray, dtype: str, n_bins: int, mn: float, mx: float) -> np.ndarray:
    """The bin of every element: min(floor(max((x - min) / (max - min) * n_bins, 0)) as usize,
    n_bins - 1); NaN -> bin 0; the clip is done in f64 before the integer cast."""
    mn, mx, nb = np.float64(mn), np.float64(mx), np.float64(n_bins)
    with np.errstate(all="ignore"):
        norm = (to_f64(v, dtype) - mn) / (mx - mn)
        s = norm * nb
        s = np.where(s > 0.0, s, 0.0)  # f64::max(s, 0.0): NaN and negatives -> 0
        s = np.minimum(np.floor(s), np.float64(n_bins - 1))
    return s.astype(np.int64)


def bin_edges(n_bins: int, mn: float, mx: float) -> np.ndarray:
    mn, mx = np.float64(mn), np.float64(mx)
    with np.errstate(all="ignore"):
        return (np.arange(n_bins + 1, dtype=np.float64) / np.float64(n_bins)) * (mx - mn) + mn


def histogram(v: np.ndarray, dtype: str, n_bins: int, mn: float, mx: float):
    """(bin_edges f64[n_bins + 1], hist u64[n_bins])."""
    b = bins(np.asarray(v).reshape(-1), dtype, n_bins, mn, mx)
    return bin_edges(n_bins, mn, mx), np.bincount(b, minlength=n_bins).astype(np.uint64)


def range_(v: np.ndarray, dtype: str):
    """(min, max) as Python values (integers exact, floats widened to f64), NaN ignored, -0.0
    below +0.0; (None, None) without a non-NaN element."""
    v = np.asarray(v).reshape(-1)
    if dtype not in FLOATS:
        return (int(v.min()), int(v.max())) if v.size else (None, None)
    x = to_f64(v, dtype)
    x = x[~np.isnan(x)]
    if x.size == 0:
        return None, None
    lo, hi = float(x.min()), float(x.max())
    zeros = x[x == 0.0]
    if lo == 0.0:
        lo = -0.0 if np.signbit(zeros).any() else 0.0
    if hi == 0.0:
        hi = 0.0 if (~np.signbit(zeros)).any() else -0.0
    return lo, hi


def same_value(a, b) -> bool:
    """Equal as range results: None with None, integers exactly, floats by value and sign."""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, float) or isinstance(b, float):
        a, b = float(a), float(b)
        return a == b and math.copysign(1.0, a) == math.copysign(1.0, b)
    return a == b
