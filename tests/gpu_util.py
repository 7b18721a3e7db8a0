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


# Float tolerance (stated in DESIGN.md §5): |gpu - ref| <= 1e-5 * max(1, |ref|). The GPU sums
# box windows in f32 (fixed tree order); the reference in f64 through summed-area tables.
FLOAT_TOL = 1e-5
