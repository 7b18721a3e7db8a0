"""Helpers shared by the -m gpu tests: host<->device transfer of any Zarr element type."""
import numpy as np

from oracle import oracle as O


def to_dev(a: np.ndarray, dtype: str):
    import torch
    from zarrs_tools_amd import torch_dtype
    a = np.ascontiguousarray(a, dtype=O.NP_STORAGE[dtype])
    if a.size == 0:
        return torch.empty(a.shape, dtype=torch_dtype(dtype), device="cuda")
    flat = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).cuda()
    return flat.view(torch_dtype(dtype)).reshape(a.shape)


def from_dev(t, dtype: str) -> np.ndarray:
    import torch
    shape = tuple(t.shape)
    if t.numel() == 0:
        return np.zeros(shape, dtype=O.NP_STORAGE[dtype])
    b = t.contiguous().reshape(-1).view(torch.uint8).cpu().numpy()
    return b.view(O.NP_STORAGE[dtype]).reshape(shape)


FLOATS = ("float16", "bfloat16", "float32", "float64")


def poisoned(shape, dtype: str):
    """A device output buffer that no result equals by accident: NaN for f32 / f64, the NaN
    0x7FFF for the 16-bit floats, the type's maximum for integers. torch.empty often hands back
    the previous (correct) result of the same size, so an element that a kernel never writes
    passes in such a buffer and fails in this one."""
    st = O.NP_STORAGE[dtype]
    if dtype in ("float16", "bfloat16"):
        fill = np.full(shape, 0x7FFF, dtype=np.uint16)
    elif dtype in FLOATS:
        fill = np.full(shape, np.nan, dtype=st)
    else:
        fill = np.full(shape, np.iinfo(st).max, dtype=st)
    return to_dev(fill, dtype)


def float_values(a: np.ndarray, dtype: str) -> np.ndarray:
    """Storage of a float type -> values whose NaN-ness is the element's (f16 / bf16 as f32)."""
    a = np.ascontiguousarray(a, dtype=O.NP_STORAGE[dtype])
    if dtype == "float16":
        return a.view(np.float16).astype(np.float32)
    if dtype == "bfloat16":
        return (a.astype(np.uint32) << 16).view(np.float32)
    return a


def assert_same_bits_nan(out: np.ndarray, ref: np.ndarray, dtype: str,
                         max_nan_share: float = 0.02) -> None:
    """Bit-exact comparison of storage arrays with the one exemption the project allows: where
    the reference of a float type is NaN the output must be NaN too, of any sign and payload
    (those of a generated NaN differ between x86 and the GPU); every other element, and every
    element of an integer type (NaN casts to 0 on both sides), has equal bytes. The share of
    exempt elements is bounded on the reference first, so the exemption cannot hide a kernel."""
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert out.dtype == ref.dtype == np.dtype(O.NP_STORAGE[dtype]), (out.dtype, ref.dtype, dtype)
    out, ref = np.ascontiguousarray(out), np.ascontiguousarray(ref)
    if ref.size == 0:
        return
    bits = f"u{ref.dtype.itemsize}"
    differ = out.view(bits) != ref.view(bits)
    if dtype in FLOATS:
        nan = np.isnan(float_values(ref, dtype))
        share = float(nan.mean())
        assert share <= max_nan_share, f"the reference is {share:.2%} NaN: too many exempt"
        differ = np.where(nan, ~np.isnan(float_values(out, dtype)), differ)
    if differ.any():
        i = tuple(int(k) for k in np.argwhere(differ)[0])
        raise AssertionError(f"{int(differ.sum())} of {ref.size} elements differ, first at {i}: "
                             f"got {out[i]!r}, want {ref[i]!r} ({dtype} storage)")


def rel_err(out: np.ndarray, ref: np.ndarray) -> float:
    out = out.astype(np.float64)
    ref = ref.astype(np.float64)
    if out.size == 0:
        return 0.0
    return float(np.max(np.abs(out - ref) / np.maximum(1.0, np.abs(ref))))


# Float tolerance (stated in DESIGN.md §4, "Tolerance"): |gpu - ref| <= 1e-5 * max(1, |ref|). The
# GPU sums box windows in f32 (fixed tree order); the reference in f64 through summed-area tables.
# The figure was stated and measured on data in [0, 300): there max(1, |ref|) is relative for all
# but the smallest values. For data outside [1, ~500) the same bound is taken relative to the
# data's scale (scaled_rel_err): on values in [0, 1) the plain form is an absolute 1e-5, which a
# result wrong by a percent passes, and at 1e14 its floor of 1 is far below one f32 ulp.
FLOAT_TOL = 1e-5


def value_scale(v: np.ndarray) -> float:
    """The power of two S that puts max |v| into [256, 512): the value range of the [0, 300)
    data at which FLOAT_TOL was stated and measured. Non-finite elements are left out."""
    a = np.abs(np.asarray(v, dtype=np.float64))
    top = float(a[np.isfinite(a)].max())
    assert top > 0
    return 2.0 ** (int(np.floor(np.log2(top))) - 8)


def scaled_rel_err(out: np.ndarray, ref: np.ndarray, S: float) -> float:
    """rel_err of the values in units of S (value_scale of the input): a power of two, so the
    division is exact in f64 for every f32 value, subnormal ones included."""
    return rel_err(out.astype(np.float64) / S, ref.astype(np.float64) / S)


def assert_cast_bracketed(out: np.ndarray, ref_f32: np.ndarray, dout: str, S: float) -> None:
    """An integer or 16-bit float output against the f32 reference, at any magnitude. The casts
    are monotone, so an f32 result within t = FLOAT_TOL * S * max(1, |ref| / S) of the reference
    lands in cast(ref - t) <= out <= cast(ref + t), elementwise (the ends are cast from f64, where
    ref +- t is formed; an f32 value casts alike from either). 16-bit floats compare as values
    (-0.0 == 0.0; +-inf are ordered); a NaN must meet a NaN."""
    assert out.shape == ref_f32.shape and out.dtype == np.dtype(O.NP_STORAGE[dout]), (out.dtype,
                                                                                      dout)
    ref = ref_f32.astype(np.float64)
    t = FLOAT_TOL * S * np.maximum(1.0, np.abs(ref) / S)
    lo, hi = O.cast_from_f64(ref - t, dout), O.cast_from_f64(ref + t, dout)
    if dout in ("float16", "bfloat16"):
        out, lo, hi = (float_values(a, dout) for a in (out, lo, hi))
        nan = np.isnan(ref)
        bad = np.where(nan, ~np.isnan(out), ~((lo <= out) & (out <= hi)))
    else:
        bad = ~((lo <= out) & (out <= hi))
    if bad.any():
        i = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError(f"{int(bad.sum())} of {out.size} elements outside the bracket, first "
                             f"at {i}: got {out[i]!r}, want [{lo[i]!r}, {hi[i]!r}] for the f32 "
                             f"reference {ref_f32[i]!r} ({dout})")


def type_extremes(shape, din, seed):
    """The full range of an integer type (32- and 64-bit values round once to f32, to nearest
    even); for float64, magnitudes up to 1e30 with values that `as f32` turns into +inf, -inf
    (far apart, so no NaN arises), zero (1e-50) and a subnormal (1e-40)."""
    rng = np.random.default_rng(seed)
    if din == "float64":
        v = rng.standard_normal(shape) * 10.0 ** rng.integers(-30, 31, shape)
        flat = v.reshape(-1)
        flat[flat.size // 5] = 1e300
        flat[3 * flat.size // 5] = -3.5e38
        flat[7] = 1e-50
        flat[11] = -1e-40
        flat[13] = -0.0
        return v
    info = np.iinfo(din)
    v = rng.integers(info.min, info.max, shape, dtype=din, endpoint=True)
    v.reshape(-1)[:4] = [info.max, info.min, info.max - 1, info.max // 2 + 1]
    return v
