"""numpy restatement of the reference's per-element filters, the checker of the pointwise tests.

  Reencode::apply_chunk_convert     src/filter/filters/reencode.rs:58-88        v as TOut
  Crop::apply_chunk_convert         src/filter/filters/crop.rs:62-122, :160-162 in[offset + i] as TOut
  Rescale::apply_chunk / _elements  src/filter/filters/rescale.rs:86-122        mul_add | (x + a) * m
  Clamp::apply_elements_inplace     src/filter/filters/clamp.rs:59-70, :150     num_traits::clamp
  Equal::apply_elements             src/filter/filters/equal.rs:62-77           (v == value) as TOut
  ReplaceValue::apply_elements      src/filter/filters/replace_value.rs:82-97   v == value ? replace

Arrays hold an element type in the oracle's storage type (O.NP_STORAGE: bool as u8, f16 and bf16
as raw u16 bits); `as` is sat_ref.as_cast over the oracle's cast helpers. `value` / `replace`
follow the fill_value grammar: a number, True / False, "NaN", "Infinity", "-Infinity".
"""
from fractions import Fraction

import numpy as np

from oracle import oracle as O
from tests.sat_ref import as_cast

FLOATS = ("float16", "bfloat16", "float32", "float64")


def work(a, dt):
    """Storage -> values that compare like the type's: f16 / bf16 as their exact f32 values."""
    a = np.ascontiguousarray(a, dtype=O.NP_STORAGE[dt])
    if dt == "float16":
        return a.view(np.float16).astype(np.float32)
    if dt == "bfloat16":
        return O.cast_to_f32(a, dt).reshape(a.shape)
    return a


def element(value, dt):
    """`value` as one element of dt (storage type), as fill_value_from_metadata reads it."""
    st = O.NP_STORAGE[dt]
    if dt == "bool":
        assert isinstance(value, bool)
        return np.array([1 if value else 0], dtype=st)
    if dt not in FLOATS:
        assert isinstance(value, int) and not isinstance(value, bool)
        assert np.iinfo(st).min <= value <= np.iinfo(st).max
        return np.array([value], dtype=st)
    x = {"NaN": np.nan, "Infinity": np.inf, "-Infinity": -np.inf}.get(value, value)
    x64 = np.array([x], dtype=np.float64)
    if dt == "float64":
        return x64
    if dt == "float32":
        with np.errstate(all="ignore"):
            return x64.astype(np.float32)
    return O.cast_from_f64(x64, dt)  # half's from_f64: one rounding, never through f32


def reencode(v, din, dout):
    return as_cast(v, din, dout)


def crop(v, din, offset, shape, dout=None):
    sl = tuple(slice(o, o + n) for o, n in zip(offset, shape))
    return as_cast(np.ascontiguousarray(np.asarray(v)[sl]), din, dout or din)


def fma(x: float, m: float, a: float) -> float:
    """x.mul_add(m, a): the exact product and sum, rounded once (Python 3.10 has no math.fma;
    Fraction arithmetic is exact and float() of a Fraction rounds to nearest even)."""
    if not (np.isfinite(x) and np.isfinite(m) and np.isfinite(a)):
        with np.errstate(all="ignore"):
            return float(np.float64(x) * np.float64(m) + np.float64(a))
    p = Fraction(x) * Fraction(m)
    s = p + Fraction(a)
    if s == 0:  # the sign of an exact zero: that of the zero operands' sum, else +0.0
        return float(np.float64(x) * np.float64(m) + np.float64(a)) if p == 0 else 0.0
    try:
        return float(s)
    except OverflowError:
        return float("inf") if s > 0 else float("-inf")


def rescale(v, din, multiply, add, add_first=False, dout=None, fused=True):
    """fused=False with add_first=False restates the defect of rounding the product and the sum
    separately (the tests assert that it differs from the fused form somewhere)."""
    x = as_cast(v, din, "float64")
    with np.errstate(all="ignore"):
        if add_first:
            r = (x + np.float64(add)) * np.float64(multiply)
        elif fused:
            r = np.array([fma(float(e), float(multiply), float(add)) for e in x.reshape(-1)],
                         dtype=np.float64).reshape(x.shape)
        else:
            r = x * np.float64(multiply) + np.float64(add)
    return as_cast(r, "float64", dout or din)


def clamp(v, din, lo, hi, dout=None):
    v = np.ascontiguousarray(v, dtype=O.NP_STORAGE[din])
    lo_s = as_cast(np.array([lo], dtype=np.float64), "float64", din)  # min as TIn
    hi_s = as_cast(np.array([hi], dtype=np.float64), "float64", din)
    w, lo_w, hi_w = work(v, din), work(lo_s, din), work(hi_s, din)
    with np.errstate(all="ignore"):  # a NaN fails both comparisons
        c = np.where(w < lo_w, lo_s, np.where(w > hi_w, hi_s, v)).astype(v.dtype)
    return as_cast(c, din, dout or din)


def equal(v, din, value, dout="bool"):
    assert dout in ("bool", "uint8")
    with np.errstate(all="ignore"):
        return (work(v, din) == work(element(value, din), din)).astype(np.uint8)


def replace_value(v, din, value, replace, dout=None):
    dout = dout or din
    with np.errstate(all="ignore"):
        mask = work(v, din) == work(element(value, din), din)
    out = as_cast(v, din, dout)
    out[mask] = element(replace, dout)[0]
    return out


def program(v, din, ops):
    """ops: [(name, dout, kwargs)] applied in order, every intermediate materialised."""
    fn = {"reencode": reencode, "crop": crop, "rescale": rescale, "clamp": clamp, "equal": equal,
          "replace_value": replace_value}
    for name, dout, kw in ops:
        v = fn[name](v, din, dout=dout, **kw)
        din = dout
    return v


def assert_same_bits(out, ref, dt):
    """Equal bytes; for float types with NaNs: the same NaN positions, equal bytes elsewhere (the
    sign and payload of a generated NaN differ between x86 and the GPU)."""
    assert out.shape == ref.shape and out.dtype == ref.dtype, (out.shape, ref.shape, out.dtype)
    if dt in FLOATS:
        nan = np.isnan(work(ref, dt))
        assert np.array_equal(np.isnan(work(out, dt)), nan)
        out, ref = out[~nan], ref[~nan]
    assert np.array_equal(np.ascontiguousarray(out).view(np.uint8),
                          np.ascontiguousarray(ref).view(np.uint8))


def type_values(dt, n=0, seed=0):
    """Values of dt (storage) that include its extremes, +-0, +-inf, NaN and subnormals where
    they exist, followed by n random ones."""
    st = O.NP_STORAGE[dt]
    rng = np.random.default_rng(seed + len(dt))
    if dt == "bool":
        return np.concatenate([np.array([0, 1, 1, 0], dtype=st),
                               rng.integers(0, 2, n).astype(st)])
    if dt not in FLOATS:
        ii = np.iinfo(st)
        base = [ii.min, ii.max, 0, 1, 2, 5, 7, 100, ii.max - 1, ii.min + 1, ii.max // 2]
        if ii.min < 0:
            base += [-1, -2, -5, -100]
        if ii.bits == 64:
            base += [2 ** 53, 2 ** 53 + 1, (-2 ** 53 - 1) if ii.min < 0 else 2 ** 63 + 1025]
        rnd = rng.integers(ii.min, ii.max, n, dtype=st, endpoint=True)
        return np.concatenate([np.array(base, dtype=st), rnd])
    fi = {"float16": np.finfo(np.float16), "bfloat16": np.finfo(np.float32),
          "float32": np.finfo(np.float32), "float64": np.finfo(np.float64)}[dt]
    tiny = {"float16": 6e-8, "bfloat16": 1e-40, "float32": 1e-45, "float64": 5e-324}[dt]
    base = [0.0, -0.0, np.inf, -np.inf, np.nan, float(fi.max), -float(fi.max), float(fi.tiny),
            tiny, -tiny, 1.0, -1.0, 0.5, 2.5, 3.5, -2.5, 5.0, 7.0, 254.5, 255.5, 256.0, 65535.7,
            -129.0, 3e9, -3e9, 1e19, -1e19, 1e-3]
    rnd = (rng.random(n) - 0.3) * 1000
    x = np.concatenate([np.array(base, dtype=np.float64), rnd])
    with np.errstate(all="ignore"):
        if dt == "float64":
            return x
        if dt == "float32":
            return x.astype(np.float32)
        if dt == "float16":
            return x.astype(np.float16).view(np.uint16)
        return O.cast_from_f64(x, "bfloat16")
