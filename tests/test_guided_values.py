"""The inputs of tests/test_guided_values_gpu.py keep, on the CPU oracle, the conditions that make
them worth running (tests/guided_value_cases.py): an input that drifts fails here and cannot
silently hollow out a GPU test.

  A-E  the oracle's result has no NaN (A, B, C: no inf either);
  A    for -56 <= k <= +56 the oracle's result is bitwise 2^k times the unscaled one; at k = -60
       s = (v - u)^2 is subnormal where |v0 - u0| < 1/8 and rounds differently, so up to 0.03 %
       of the elements differ there (at least 99.9 % are bitwise equal, all within 1e-6 in units
       of the data's scale); at k = +56 at least 5 % of the elements have s + eps >= 2^126,
       where the reciprocal of the denominator is subnormal; at k = -64 with eps0 = 0.5 eps and
       some s + eps are subnormal and the result stays within 1e-6 of the unscaled one;
  C    at eps = 0 the oracle returns its input bitwise;
  D    64-bit integers reach s >= 2^126 too; the planted float64 values round as described;
  E    the 2^40 input saturates every integer type and overflows float16.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import guided_value_cases as V
from tests.gpu_util import (FLOAT_TOL, assert_cast_bracketed, rel_err, scaled_rel_err,
                            value_scale)

TWO126 = np.float32(2.0 ** 126)
TINY = np.finfo(np.float32).tiny  # 2^-126


@pytest.mark.parametrize("eps0", V.A_EPS0)
@pytest.mark.parametrize("pid", V.A_PATHS)
def test_a_scale_sweep_inputs(pid, eps0):
    p = V.PATHS[pid]
    v0 = V.a_base(pid)
    assert 256 <= float(v0.max()) < 512 and value_scale(v0) == 1.0
    base = V.oracle(v0, p, eps0)
    assert np.isfinite(base).all()
    for k in V.A_KS:
        v, eps = V.a_input(pid, k, eps0)
        assert value_scale(v) == 2.0 ** k
        ref = V.oracle(v, p, eps)
        assert np.isfinite(ref).all(), (k, eps0)
        want = base.astype(np.float64) * 2.0 ** k
        if k >= -56:
            assert np.array_equal(ref, want.astype(np.float32)), (k, eps0)
        else:
            assert scaled_rel_err(ref, want, 2.0 ** k) <= 1e-6, (k, eps0)
        if k == -60:
            assert float(np.mean(ref == want.astype(np.float32))) >= 0.999, eps0
        with np.errstate(over="ignore"):
            den = V.variance_term(v, p.r) + eps
        if k == 56:
            assert float(np.mean(den >= TWO126)) >= 0.05, (eps0, float(np.mean(den >= TWO126)))
            assert np.isfinite(den).all()
        if k == -64 and eps0 == 0.5:
            assert 0 < eps < TINY
            assert float(np.mean(den < TINY)) > 0.001


@pytest.mark.parametrize("pid", V.B_PATHS)
def test_b_small_values_inputs(pid):
    p = V.PATHS[pid]
    v = V.b_input(pid)
    assert float(v.max()) < 2.0 ** -10 and value_scale(v) == 2.0 ** -19
    for eps in V.B_EPS:
        assert np.isfinite(V.oracle(v, p, eps)).all()


@pytest.mark.parametrize("pid", V.C_PATHS)
def test_c_zero_eps_inputs(pid):
    p = V.PATHS[pid]
    v = V.c_random(pid)
    assert np.all(V.variance_term(v, p.r) > 0)
    ref = V.oracle(v, p, 0.0)
    assert np.array_equal(ref.view(np.uint32), v.view(np.uint32))
    w = V.c_constant(pid)
    assert np.all(w[:, :V.C_CONST_ROWS] == 7) and p.shape[1] > V.C_CONST_ROWS
    s = V.variance_term(w, p.r)
    assert float(np.mean(s == 0)) > 0.2
    assert np.isfinite(V.oracle(w, p, V.C_CONST_EPS)).all()


@pytest.mark.parametrize("din", V.D_TYPES)
@pytest.mark.parametrize("pid", V.D_PATHS)
def test_d_wide_type_inputs(pid, din):
    p = V.PATHS[pid]
    v, v32, eps = V.d_input(pid, din)
    assert np.isfinite(v32).all() and 256 <= float(np.abs(v32).max()) / value_scale(v32) < 512
    ref = V.oracle(v32, p, eps)
    assert float(np.isnan(ref).mean()) == 0.0
    if din != "float64":
        info = np.iinfo(din)
        assert list(v.reshape(-1)[:4]) == [info.max, info.min, info.max - 1, info.max // 2 + 1]
        assert np.isfinite(ref).all()
        # the conversions round: the values are not all f32 images
        assert np.any(v32.astype(np.float64) != v.astype(np.float64))
    else:
        flat, flat32 = v.reshape(-1), v32.reshape(-1)
        assert flat32[5] == np.float32(2.0 ** 24 + 2) and flat32[7] == 0 and flat[7] > 0
    if din in ("int64", "uint64"):
        for i, w in enumerate(V.D_DOUBLE_ROUNDING[din]):
            once, twice = v32.reshape(-1)[4 + i], np.float32(np.float64(w))
            assert int(v.reshape(-1)[4 + i]) == w and float(np.float64(w)) != w
            assert once != twice and abs(float(once)) > abs(float(twice))
        with np.errstate(over="ignore"):
            s = V.variance_term(v32, p.r)
        assert float(np.mean(s >= TWO126)) > 0.002


def test_e_output_cast_inputs():
    p = V.PATHS[V.E_PATH]
    for k in V.E_SCALES:
        v, eps = V.e_input(k)
        assert value_scale(v) == 2.0 ** k
        ref = V.oracle(v, p, eps)
        assert np.isfinite(ref).all()
        assert (ref < 0).mean() > 0.2 and (ref > 0).mean() > 0.2
    v, eps = V.e_input(40)  # the saturation claims
    ref = V.oracle(v, p, eps)
    for dout in ("int8", "int16", "int32", "uint8", "uint16", "uint32"):
        st = np.iinfo(O.NP_STORAGE[dout])
        c = O.cast_from_f32(ref, dout)
        assert float(np.mean((c == st.max) | (c == st.min))) > 0.99, dout
    assert float(np.mean(O.cast_from_f32(ref, "uint64") == 0)) > 0.2
    i64 = O.cast_from_f32(ref, "int64")
    assert np.any(i64 == np.iinfo(np.int64).max) or float(np.abs(ref).max()) < 2.0 ** 63
    h = O.cast_from_f32(ref, "float16").view(np.float16)
    assert np.isinf(h).mean() > 0.9


@pytest.mark.parametrize("pid", V.F_PATHS)
def test_f_non_finite_geometry(pid):
    """The element sits in the first quarter of every axis, its 2r neighbourhood is inside the
    array's first half, and the part the contract pins bitwise is at least half of the array."""
    p = V.PATHS[pid]
    shape = V.F_SHAPE[pid]
    assert shape[:-1] == p.shape[:-1] and shape[-1] >= p.shape[-1]
    bad, clean, pos = V.f_inputs(pid, "nan")
    assert all(q < n / 4 for q, n in zip(pos, shape))
    assert np.isnan(bad[pos]) and clean[pos] == 0 and np.isfinite(clean).all()
    assert int(np.sum(bad.view(np.uint32) != clean.view(np.uint32))) == 1
    near, far = V.f_masks(pid)
    assert near[pos] and not (near & far).any()
    assert float(far.mean()) >= 0.5, float(far.mean())


def test_f_bounds_follow_the_kernels_constants():
    """F_BOUND is derived from tile and segment sizes; a change of those must revisit it."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "zarrs_tools_amd", "csrc")
    sep = open(os.path.join(csrc, "guided_filter.hip")).read()
    g4 = open(os.path.join(csrc, "guided4d.hip")).read()
    assert re.search(r"constexpr int kSepSeg = (\d+);", sep).group(1) == str(V.F_SEP_SEG)
    assert re.search(r"constexpr int kTX = (\d+),", g4).group(1) == str(V.F_TILE_X)
    m = re.search(r"constexpr int kMX = (\d+), kMY = (\d+),", g4)
    assert m.group(1) == m.group(2) == str(V.F_TM_TILE)
    from tests import fused_cases as FC
    assert FC.TX == V.F_TILE_X and all(FC.tile_y(r) <= V.F_TILE_X for r in range(1, 9))


def test_scaled_rel_err_is_relative_to_the_data():
    """The metric the GPU file asserts: on [0, 1)-sized data an error of 2^-10 relative fails
    (the plain rel_err passes it); on the [0, 300) data both agree; an exact power-of-two rescale
    of data and error leaves it unchanged."""
    rng = np.random.default_rng(1)
    ref = (rng.random(1000) * 2.0 ** -10).astype(np.float32)
    out = (ref * np.float32(1 + 2.0 ** -10)).astype(np.float32)
    assert rel_err(out, ref) <= FLOAT_TOL
    assert scaled_rel_err(out, ref, value_scale(ref)) > FLOAT_TOL
    big = (rng.random(1000) * 300).astype(np.float32)
    near = np.nextafter(big, np.float32(1000))
    assert value_scale(big) == 1.0
    assert scaled_rel_err(near, big, 1.0) == rel_err(near, big)
    f = np.float32(2.0 ** 56)
    assert scaled_rel_err(near * f, big * f, 2.0 ** 56) == rel_err(near, big)


def test_cast_bracket_accepts_the_cast_and_rejects_a_wrapped_or_shifted_one():
    ref = np.array([-3e14, -1.5, 0.25, 2.75, 70000.0, 3e9, 1e19, 3e38], dtype=np.float32)
    S = 2.0 ** 40
    for dout in O.DTYPES:
        if dout in ("float32", "float64"):
            continue
        good = O.cast_from_f32(ref, dout)
        assert_cast_bracketed(good, ref, dout, 1.0)
        assert_cast_bracketed(good, ref, dout, S)
    wrapped = np.clip(ref.astype(np.float64), -2.0 ** 62, 2.0 ** 62).astype(np.int64) \
        .astype(np.int32)  # 3e9 wraps to a negative value
    with pytest.raises(AssertionError):
        assert_cast_bracketed(wrapped, ref, "int32", 1.0)
    off = O.cast_from_f32(ref, "int64")
    off[0] += 2 ** 33  # 8.6e9 at -3e14: past the bracket's 1e-5 * 3e14 = 3e9
    with pytest.raises(AssertionError):
        assert_cast_bracketed(off, ref, "int64", S)
    nan_ref = np.array([np.nan, 1.0], dtype=np.float32)
    assert_cast_bracketed(O.cast_from_f32(nan_ref, "float16"), nan_ref, "float16", 1.0)
    with pytest.raises(AssertionError):
        assert_cast_bracketed(O.cast_from_f32(np.array([1.0, 1.0], np.float32), "float16"),
                              nan_ref, "float16", 1.0)
