"""Gradient magnitude (gradient_magnitude.rs, kernel.rs:75-129) on the CPU: the numpy restatement
against the reference's known-answer test, the halo property that lets the GPU run one pass over
a whole array instead of a loop over chunks, and the host-only parts of the operator surface."""
import numpy as np
import pytest

import zarrs_tools_amd as zt
from zarrs_tools_amd import _abi
from zarrs_tools_amd import store as S
from tests import gm_ref as R

# gradient_magnitude.rs:286-325: 4x4 f32 (i + j), chunks 2x2, Sobel
KAT_IN = np.array([[i + j for j in range(4)] for i in range(4)], dtype=np.float32)
KAT_OUT = np.array([[0.70710677, 1.118034, 1.118034, 0.70710677],
                    [1.118034, 1.4142135, 1.4142135, 1.118034],
                    [1.118034, 1.4142135, 1.4142135, 1.118034],
                    [0.70710677, 1.118034, 1.118034, 0.70710677]], dtype=np.float32)


def test_restatement_reproduces_reference_kat_bit_exactly():
    assert np.array_equal(R.apply_chunks(KAT_IN, (2, 2)), KAT_OUT)
    assert np.array_equal(R.apply_ndarray(KAT_IN), KAT_OUT)


def test_extent_one_axis_is_not_the_identity():
    # (0.25 v + 0.5 v) + 0.25 v along a unit axis: its roundings return v for normal values, but
    # the products of the smallest subnormals round away, so the pass may not be skipped
    v = np.random.default_rng(1).random((1, 1, 1000), dtype=np.float32)
    v[0, 0, :8] = np.arange(1, 9, dtype=np.uint32).view(np.float32)  # 1..8 ulp subnormals
    with np.errstate(under="ignore"):
        t = R.triangle(v, 0)
        want = (v * np.float32(0.25) + v * np.float32(0.5)) + v * np.float32(0.25)
    assert np.array_equal(t, want)
    assert np.array_equal(t[0, 0, 8:], v[0, 0, 8:])
    assert (t[0, 0, :8] != v[0, 0, :8]).any()


@pytest.mark.parametrize("operator", ["sobel", "central_difference"])
@pytest.mark.parametrize("shape,chunk", [
    ((9, 17), (4, 5)),
    ((7, 9, 11), (3, 4, 5)),
    ((4, 5, 6, 7), (2, 3, 4, 3)),
])
def test_chunked_equals_whole_block(shape, chunk, operator):
    # every pass reaches 1 and each axis gets one pass, so a halo of 1 clamped to the array makes
    # every chunk's indices clamp exactly where the whole array's do
    rng = np.random.default_rng(len(shape))
    v = (rng.random(shape, dtype=np.float32) * 100 - 30).astype(np.float32)
    assert np.array_equal(R.apply_chunks(v, chunk, operator), R.apply_ndarray(v, operator))


def test_memory_per_chunk_matches_reference_formula():
    # gradient_magnitude.rs:177-195: 6*7*8 * (2 + 16) + 4*5*6 * (4 + 4)
    g = zt.GradientMagnitude()
    assert g.memory_per_chunk("uint16", "float32", (4, 5, 6)) == 7008


def test_is_compatible_all_13_types():
    g = zt.GradientMagnitude("central_difference")
    for a in _abi.DTYPES:
        for b in _abi.DTYPES:
            g.is_compatible(a, b)
    with pytest.raises(zt.UnsupportedDataType):
        g.is_compatible("complex64", "float32")
    with pytest.raises(zt.UnsupportedDataType):
        g.is_compatible("float32", "complex64")


def test_operator_names():
    assert zt.GradientMagnitude().name() == "gradient_magnitude"
    assert zt.GradientMagnitude().operator == "sobel"
    assert zt.GradientMagnitude("central_difference").operator == "central_difference"
    with pytest.raises(zt.InvalidParameters):
        zt.GradientMagnitude("prewitt")
    with pytest.raises(zt.InvalidParameters):
        S.gradient_magnitude("in", "out", operator="prewitt")


def test_unknown_operator_code_is_rejected_by_the_abi(tmp_path):
    S.create_array(tmp_path / "in", "float32", (8, 8), (4, 4))
    rc = _abi.lib().zt_store_gradient_magnitude(str(tmp_path / "in").encode(),
                                                str(tmp_path / "out").encode(), -1, None, 7, 0,
                                                0, -1, 0, 3, None)
    assert rc == _abi.ERR_INVALID_PARAMETERS


def test_not_enough_memory_is_the_reference_error(tmp_path, monkeypatch):
    S.create_array(tmp_path / "in", "float32", (64, 64, 64), (32, 64, 64))
    monkeypatch.setenv("ZT_STORE_HOST_MEMORY", "100000")  # < one 512 KiB chunk row
    with pytest.raises(_abi.FilterError, match="not enough available memory") as e:
        S.gradient_magnitude(tmp_path / "in", tmp_path / "out")
    assert e.value.status == _abi.ERR_OUT_OF_MEMORY
