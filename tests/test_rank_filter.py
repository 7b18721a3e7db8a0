"""The rank filters (minimum, median, maximum) on the CPU: the numpy restatement
against hand-written answers, the halo property that lets the GPU run one pass over a whole array
instead of a loop over chunks, the per-axis separation of minimum / maximum, and the host-only
parts of the operator surface."""
import numpy as np
import pytest

import zarrs_tools_amd as zt
from zarrs_tools_amd import _abi
from zarrs_tools_amd import store as S
from zarrs_tools_amd import zarrs_filter as ZF
from tests import rank_ref as R


def test_row_with_ties():
    v = np.array([3, 1, 1, 2, 3, 3, 0], dtype=np.uint8)
    # windows (edges replicate): 331 311 112 123 233 330 300
    assert R.apply_ndarray(v, "minimum", (1,), "uint8").tolist() == [1, 1, 1, 1, 2, 0, 0]
    assert R.apply_ndarray(v, "median", (1,), "uint8").tolist() == [3, 1, 1, 2, 3, 3, 0]
    assert R.apply_ndarray(v, "maximum", (1,), "uint8").tolist() == [3, 3, 2, 3, 3, 3, 3]
    # h = 2: windows 33311 33112 31123 11233 12330 23300 33000
    assert R.apply_ndarray(v, "median", (2,), "uint8").tolist() == [3, 2, 2, 2, 2, 2, 0]


def test_3x3_block():
    v = np.array([[5, -7, 2], [0, 9, -1], [4, 4, -128]], dtype=np.int8)
    # the centre's window is the whole block: -128 -7 -1 0 2 4 4 5 9
    assert R.apply_ndarray(v, "minimum", (1, 1), "int8")[1, 1] == -128
    assert R.apply_ndarray(v, "median", (1, 1), "int8")[1, 1] == 2
    assert R.apply_ndarray(v, "maximum", (1, 1), "int8")[1, 1] == 9
    # the corner (0, 0): rows 0, 0, 1 x columns 0, 0, 1 = 5 5 -7 5 5 -7 0 0 9
    assert R.apply_ndarray(v, "median", (1, 1), "int8")[0, 0] == 5
    assert R.apply_ndarray(v, "minimum", (1, 1), "int8")[0, 0] == -7
    # h = (0, 1): rows alone
    assert R.apply_ndarray(v, "median", (0, 1), "int8").tolist() == [[5, 2, 2], [0, 0, -1],
                                                                     [4, 4, -128]]


def test_float_order_of_nans_and_zeros():
    # the order: -NaN < -1 < -0.0 < +0.0 < 1 < +NaN; each of the four specials at every rank
    pnan, nnan, pz, nz = 0x7FC00001, 0xFFC00002, 0x00000000, 0x80000000
    one, mone = 0x3F800000, 0xBF800000
    order = [nnan, mone, nz, pz, one, pnan]
    keys = R.to_key(np.array(order, dtype=np.uint32).view(np.float32), "float32")
    assert (np.diff(keys.astype(np.int64)) > 0).all()
    rank = {"minimum": 0, "median": 1, "maximum": 2}
    for a in range(len(order)):
        for b in range(a + 1, len(order)):
            for c in range(b + 1, len(order)):
                trip = [order[a], order[b], order[c]]
                for perm in ([0, 1, 2], [2, 0, 1], [1, 2, 0], [2, 1, 0]):
                    v = np.array([trip[i] for i in perm], dtype=np.uint32).view(np.float32)
                    for kind, r in rank.items():
                        got = R.apply_ndarray(v, kind, (1,), "float32")[1:2].view(np.uint32)[0]
                        assert got == trip[r], (trip, perm, kind)
    # an isolated NaN disappears under the median, a +NaN dilates under the maximum; bits pass
    row = np.array([one, one, pnan, one, one], dtype=np.uint32).view(np.float32)
    assert R.apply_ndarray(row, "median", (1,), "float32").view(np.uint32).tolist() == [one] * 5
    assert R.apply_ndarray(row, "maximum", (1,), "float32").view(np.uint32).tolist() == [
        one, pnan, pnan, pnan, one]
    # float16 works from its u16 bits
    h = np.array([0x8000, 0x0000, 0xFE01], dtype=np.uint16)  # -0.0, +0.0, -NaN
    assert R.apply_ndarray(h, "median", (1,), "float16").tolist() == [0x8000, 0x8000, 0xFE01]
    assert R.apply_ndarray(h, "minimum", (1,), "float16").tolist() == [0x8000, 0xFE01, 0xFE01]


@pytest.mark.parametrize("kind", R.KINDS)
def test_chunked_equals_whole_block(kind):
    rng = np.random.default_rng(5)
    v = rng.integers(0, 6, (7, 33, 67)).astype(np.uint8)  # ties everywhere
    whole = R.apply_ndarray(v, kind, (1, 1, 1), "uint8")
    assert np.array_equal(R.apply_chunks(v, (4, 16, 32), kind, (1, 1, 1), "uint8"), whole)
    f = (rng.random((7, 33, 67), dtype=np.float32) - 0.5).astype(np.float32)
    assert np.array_equal(
        R.apply_chunks(f, (4, 16, 32), kind, (2, 0, 1), "float32").view(np.uint32),
        R.apply_ndarray(f, kind, (2, 0, 1), "float32").view(np.uint32))


@pytest.mark.parametrize("kind", ["minimum", "maximum"])
def test_per_axis_passes_equal_the_window(kind):
    rng = np.random.default_rng(6)
    v = rng.integers(-100, 100, (6, 9, 11)).astype(np.int16)
    for half in ((1, 1, 1), (2, 0, 3), (0, 4, 1)):
        assert np.array_equal(R.apply_separable(v, kind, half, "int16"),
                              R.apply_ndarray(v, kind, half, "int16"))
    f = (rng.random((5, 12), dtype=np.float32) - 0.5).astype(np.float32)
    f.view(np.uint32)[2, 3] = 0xFFC00000  # -NaN is the smallest
    f.view(np.uint32)[3, 8] = 0x7FC00000  # +NaN the largest
    assert np.array_equal(R.apply_separable(f, kind, (1, 2), "float32").view(np.uint32),
                          R.apply_ndarray(f, kind, (1, 2), "float32").view(np.uint32))


def test_is_compatible_all_13_types():
    f = zt.Median((1, 1, 1))
    for a in _abi.DTYPES:
        for b in _abi.DTYPES:
            f.is_compatible(a, b)
    with pytest.raises(zt.UnsupportedDataType):
        f.is_compatible("complex64", "float32")
    with pytest.raises(zt.UnsupportedDataType):
        f.is_compatible("float32", "complex64")


def test_names_and_classes():
    assert zt.Median((1, 2)).name() == "median" and zt.Median((1, 2)).kernel_half_size() == (1, 2)
    assert zt.Minimum((0,)).name() == "minimum" and zt.Maximum((3,)).name() == "maximum"
    assert zt.RankFilter("maximum", (1, 1)).kind == "maximum"
    assert isinstance(zt.Median((1,)), zt.RankFilter)
    with pytest.raises(zt.InvalidParameters):
        zt.RankFilter("mode", (1, 1))


def test_memory_per_chunk_is_the_formula():
    # nin * 3 * size_in + nout * (size_in + size_out), nin = prod(chunk + 2 h)
    f = zt.Minimum((1, 2, 3))
    assert f.memory_per_chunk("uint16", "float32", (4, 5, 6)) == (
        6 * 9 * 12 * 3 * 2 + 4 * 5 * 6 * (2 + 4))
    assert zt.Median((0, 0)).memory_per_chunk("float64", "uint8", (7, 9)) == 63 * 24 + 63 * 9


def test_subcommand_grammar():
    p = ZF.build_parser()
    for name in R.KINDS:
        a = p.parse_args([name, "in", "out", "1,2,3", "--data-type", "float32",
                          "--skip-empty-chunks"])
        (step,) = ZF._steps_from_cli(a)
        assert step == {"filter": name, "input": "in", "output": "out",
                        "kernel_half_size": [1, 2, 3], "data_type": "float32",
                        "chunk_limit": None}
        assert a.filter_skip_empty_chunks and name in ZF.ON_PATH and ZF.rows_splittable(name)
    a = p.parse_args(["median", "in", "out", "-1,1"])  # a value, not an option
    assert ZF._steps_from_cli(a)[0]["kernel_half_size"] == [-1, 1]
    a = p.parse_args(["minimum", "in", "out", "-2"])
    assert ZF._steps_from_cli(a)[0]["kernel_half_size"] == [-2]
    assert "gradient_magnitude" not in ZF.ON_PATH


def test_negative_half_size_on_the_command_line_is_invalid_parameters(tmp_path, capsys):
    S.create_array(tmp_path / "in", "uint8", (8, 8), (4, 4))
    assert ZF.main(["median", str(tmp_path / "in"), str(tmp_path / "out"), "-1,1"]) == 1
    assert "negative kernel_half_size" in capsys.readouterr().err


def test_run_validates_the_half_sizes(tmp_path):
    S.create_array(tmp_path / "in", "uint8", (40, 40, 40), (20, 20, 20))
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    info = S.open_array(src)

    def step(name, half):
        return {"filter": name, "input": src, "output": dst, "kernel_half_size": half}

    for bad in (step("median", [1, 1]), step("minimum", [1, 1, 1, 1]),
                step("maximum", [1, -1, 1]), step("median", [8, 8, 8]),  # N = 4913 > 4096
                step("median", None)):
        with pytest.raises(zt.InvalidParameters):
            ZF.run([bad], log=lambda *_: None)
        assert not (tmp_path / "out").exists()
    # 15 * 15 * 17 = 3825 <= 4096 is a median; minimum has no cap
    f, shape, dt = ZF._step_params(step("median", [7, 7, 8]), info)
    assert f.name() == "median" and shape == (40, 40, 40) and dt == "uint8"
    f, _, _ = ZF._step_params(step("minimum", "8,8,8"), info)
    assert f.kernel_half_size() == (8, 8, 8)
    with pytest.raises(zt.InvalidParameters):
        zt.Median((8, 8, 8))
    with pytest.raises(zt.InvalidParameters):
        zt.Maximum((1, -1))
    with pytest.raises(zt.InvalidParameters):
        zt.Minimum((1, 1)).memory_per_chunk("uint8", "uint8", (4, 4, 4))  # rank 3


def test_unknown_kind_is_rejected_by_the_abi(tmp_path):
    S.create_array(tmp_path / "in", "float32", (8, 8), (4, 4))
    half = _abi.i64_array([1, 1])
    rc = _abi.lib().zt_store_rank_filter(str(tmp_path / "in").encode(),
                                         str(tmp_path / "out").encode(), -1, None, 7, half, 0,
                                         0, -1, 0, 3, None)
    assert rc == _abi.ERR_INVALID_PARAMETERS
    with pytest.raises(zt.InvalidParameters):
        S.rank_filter("in", "out", "mode", (1, 1))
    # the store step has the median's cap and the sign check too
    for kind, h in ((1, [40, 40]), (0, [-1, 0])):
        rc = _abi.lib().zt_store_rank_filter(str(tmp_path / "in").encode(),
                                             str(tmp_path / "out").encode(), -1, None, kind,
                                             _abi.i64_array(h), 0, 0, -1, 0, 3, None)
        assert rc == _abi.ERR_INVALID_PARAMETERS


@pytest.mark.parametrize("kind", R.KINDS)
def test_not_enough_memory_is_the_reference_error(tmp_path, monkeypatch, kind):
    S.create_array(tmp_path / "in", "float32", (64, 64, 64), (32, 64, 64))
    monkeypatch.setenv("ZT_STORE_HOST_MEMORY", "100000")  # < one 512 KiB chunk row
    with pytest.raises(_abi.FilterError, match="not enough available memory") as e:
        S.rank_filter(tmp_path / "in", tmp_path / "out", kind, (1, 1, 1))
    assert e.value.status == _abi.ERR_OUT_OF_MEMORY
