"""numpy restatement of the reference's summed-area table, the checker of the summed-area-table
tests: an explicit loop along the scanned axis (vectorised across the lanes), the accumulator in
the output type, seeded with zeros, `element += acc` on every element, the first included.

  SummedAreaTable::apply_dim   src/filter/filters/summed_area_table.rs:47-106
  SummedAreaTable::apply       src/filter/filters/summed_area_table.rs:144-253 (axes last to first)
  input cast `v.as_()`         :81 (num-traits AsPrimitive, half 2.6.0)

Arrays hold an element type in the oracle's storage type (O.NP_STORAGE: bool as u8, f16 and bf16
as raw u16 bits). numpy's cumsum is not used: it keeps the sign of a leading -0.0, where the
reference's `0.0 + -0.0` gives +0.0.
"""
import numpy as np

from oracle import oracle as O

HALF = ("float16", "bfloat16")
FLOAT = ("float32", "float64")


def _canon(dt):
    return "uint8" if dt == "bool" else dt  # the reference's (Bool, u8) arms


def as_cast(v, din, dout):
    """Rust `as` / half's AsPrimitive from din to dout: a half type converts through f32 (to f64
    directly and exactly); to a half type through f32 and from_f32 (from f64: from_f64); float ->
    int saturates, NaN -> 0 (the oracle's cast_from_*); int -> int wraps and int -> float rounds
    to nearest (numpy astype does both)."""
    din, dout = _canon(din), _canon(dout)
    v = np.ascontiguousarray(v, dtype=O.NP_STORAGE[din])
    if din == dout:
        return v.copy()
    if din in HALF:
        f = O.cast_to_f32(v, din)
        return f.astype(np.float64) if dout == "float64" else as_cast(f, "float32", dout)
    if dout in HALF:
        if din == "float64":
            return O.cast_from_f64(v, dout)
        return O.cast_from_f32(as_cast(v, din, "float32"), dout)
    if din in FLOAT and dout not in FLOAT:
        return O.cast_from_f32(v, dout) if din == "float32" else O.cast_from_f64(v, dout)
    with np.errstate(all="ignore"):
        return v.astype(O.NP_STORAGE[dout])


def _to_work(a, dt):
    """Storage -> the array the adds run on: f16 as np.float16, bf16 as its exact f32 values."""
    shape = np.shape(a)
    if dt == "float16":
        return np.array(a).view(np.float16)
    if dt == "bfloat16":
        return O.cast_to_f32(a, dt).reshape(shape)
    return np.array(a)


def _from_work(a, dt):
    shape = np.shape(a)
    if dt == "float16":
        return np.ascontiguousarray(a).view(np.uint16).reshape(shape)
    if dt == "bfloat16":
        return O.cast_from_f32(a, dt).reshape(shape)
    return np.ascontiguousarray(a).reshape(shape)


def _add(e, acc, dt):
    """`*element += acc` in the output type: one rounding to it per add."""
    with np.errstate(all="ignore"):
        if dt == "float16":  # half: f32 add, then from_f32
            return (e.astype(np.float32) + acc.astype(np.float32)).astype(np.float16)
        if dt == "bfloat16":
            s = np.ascontiguousarray(e + acc, dtype=np.float32)
            return O.cast_to_f32(O.cast_from_f32(s, dt), dt).reshape(s.shape)
        return np.add(e, acc, dtype=e.dtype)  # integers wrap (release builds)


def scan(a, axis, dt, seed=None):
    """Inclusive running sum of the work array `a` along `axis`, in place; returns the last
    accumulator (shape of `a` without `axis`). `seed`: the accumulator's start, zeros if None."""
    view = np.moveaxis(a, axis, 0)
    acc = np.zeros(view.shape[1:], dtype=a.dtype) if seed is None else seed.copy()
    for k in range(view.shape[0]):
        acc = _add(view[k], acc, dt)
        view[k] = acc
    return acc


def sat(v, din, dout=None, carry=None, return_carry=False):
    """The summed-area table of `v` (din, storage type) as dout (storage type). `carry`: the
    seed plane of the axis-0 sum (dout storage, shape v.shape[1:]), zeros if None; with
    return_carry also the last output plane."""
    dout = _canon(dout or din)
    a = _to_work(as_cast(v, din, dout), dout)
    last = None
    for axis in range(a.ndim - 1, -1, -1):
        seed = None
        if axis == 0 and carry is not None:
            seed = _to_work(np.asarray(carry, dtype=O.NP_STORAGE[dout]), dout)
        last = scan(a, axis, dout, seed)
    out = _from_work(a, dout)
    assert out.dtype == O.NP_STORAGE[dout] and out.shape == tuple(np.shape(v))
    if return_carry:
        return out, _from_work(last, dout)
    return out
