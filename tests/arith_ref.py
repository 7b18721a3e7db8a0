"""numpy restatement of the two-array arithmetic filter (an extension: the reference has no such
filter), the checker of the arithmetic tests.

    x = first[i] as f64, y = second[i] as f64      (sat_ref.as_cast: Rust `as`)
    r = one IEEE f64 operation                     (numpy float64, no contraction)
    out[i] = r as TOut                             (the final cast of pw_ref.rescale)

minimum is `y < x ? y : x` and maximum `y > x ? y : x`, written as np.where: a NaN on either side,
or +-0 against -+0, returns x. np.minimum / np.fmin are not used: their NaN and signed-zero rules
differ. Arrays hold an element type in the oracle's storage type (O.NP_STORAGE: bool as u8, f16 and
bf16 as raw u16 bits).
"""
import numpy as np

from tests.sat_ref import as_cast

OPERATORS = ("add", "subtract", "multiply", "divide", "minimum", "maximum", "absolute_difference")


def arithmetic(a, da, b, db, operator, dout=None):
    """first `operator` second as dout (default: the first's type), storage arrays in and out."""
    assert np.shape(a) == np.shape(b), (np.shape(a), np.shape(b))
    x = as_cast(a, da, "float64").reshape(np.shape(a))
    y = as_cast(b, db, "float64").reshape(np.shape(a))
    with np.errstate(all="ignore"):
        if operator == "add":
            r = x + y
        elif operator == "subtract":
            r = x - y
        elif operator == "multiply":
            r = x * y
        elif operator == "divide":
            r = x / y
        elif operator == "minimum":
            r = np.where(y < x, y, x)
        elif operator == "maximum":
            r = np.where(y > x, y, x)
        elif operator == "absolute_difference":
            r = np.fabs(x - y)
        else:
            raise ValueError(operator)
    out = as_cast(np.ascontiguousarray(r, dtype=np.float64), "float64", dout or da)
    return out.reshape(np.shape(a))
