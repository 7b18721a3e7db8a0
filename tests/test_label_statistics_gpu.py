"""GPU parity of the per-label statistics (labels.hip through the C ABI and LabelStatistics) against
their numpy restatement (tests/labels_ref.py): every count, bound and sum equal as integers, every
centroid and mean equal as the bytes of the correctly rounded quotient. The state is made of
integer sums, minima and maxima, so the result is unique and no run is repeated to look for races.

Borders of the kernel (labels.hip): a workgroup owns tiles of T = _abi.LABELS_TILE_ROWS rows x 64 x
(rows = every axis but the last, flattened) and loads full 64-element rows 16 bytes per lane when
the rows are 16-byte aligned, element by element otherwise; runs of equal labels along x are one
contribution; a workgroup's LDS table has 256 slots (ZT_LABELS_LDS_SLOTS lowers it) addressed by
label % slots with 8 probes, beyond which a run goes to the global atomics directly; the grid is
capped at ZT_LABELS_MAX_BLOCKS and loops.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import labels_ref as R
from tests.gpu_util import from_dev, to_dev

pytestmark = pytest.mark.gpu

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)
from zarrs_tools_amd import _abi  # noqa: E402

T = _abi.LABELS_TILE_ROWS
SLOTS = 256
NUMERIC = [d for d in _abi.DTYPES if d != "bool"]


def gpu(labels, dtype_l="uint32", n_labels=None, intensity=None, dtype_i=None):
    x = to_dev(labels, dtype_l)
    y = None if intensity is None else to_dev(intensity, dtype_i)
    return zt.LabelStatistics(n_labels).apply_ndarray(x, y)


def check(labels, dtype_l="uint32", n_labels=None, intensity=None, dtype_i=None):
    labels = np.ascontiguousarray(labels, dtype=O.NP_STORAGE[dtype_l])
    if intensity is not None:
        intensity = np.ascontiguousarray(intensity, dtype=O.NP_STORAGE[dtype_i])
    want = R.label_statistics(labels, n_labels, intensity, dtype_i)
    got = gpu(labels, dtype_l, n_labels, intensity, dtype_i)
    R.assert_same(got, want)
    return got


def layouts(shape, seed=0):
    """The label layouts of the issue on one shape: (name, labels as int64, n_labels)."""
    n = int(np.prod(shape))
    x = np.indices(shape)[-1]
    rng = np.random.default_rng(seed)
    return [
        ("background", np.zeros(shape, np.int64), None),
        ("background, K = 5", np.zeros(shape, np.int64), 5),
        ("one label", np.ones(shape, np.int64), None),
        ("every element alone", np.arange(1, n + 1, dtype=np.int64).reshape(shape), None),
        ("alternating along x", 1 + (x % 2), None),
        ("colliding slots", np.where(rng.random(shape) < 0.7,
                                     1 + SLOTS * rng.integers(0, 12, shape), 0), None),
        ("absent rows", np.where(rng.random(shape) < 0.5, 3 * rng.integers(1, 5, shape), 0), 20),
        ("runs", np.repeat(rng.integers(0, 4, (n + 4) // 5), 5)[:n].reshape(shape), None),
    ]


SHAPES = ([(3, 5, e) for e in (1, 2, 63, 64, 65, 129, 80)]
          + [(e, 70) for e in (1, T, T + 1)] + [(T + 1, 2, 64)]
          + [(37,), (200,), (9, 70), (3, 4, 9, 17), (2, 2, 3, 5, 9)])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_and_layouts(shape):
    rng = np.random.default_rng(len(shape))
    inten = rng.integers(0, 65536, shape).astype(np.uint16)
    for k, (name, lab, K) in enumerate(layouts(shape, seed=k_seed(shape))):
        check(lab, "uint32", K)
        check(lab, "uint32", K, inten, "uint16")


def k_seed(shape):
    return sum(shape) + len(shape)


def test_zero_extents_and_rank():
    for shape in ((0,), (3, 0, 5), (0, 4)):
        got = check(np.zeros(shape, np.int64), "uint8", 3)
        assert got["background"] == 0 and got["count"].tolist() == [0, 0, 0]
        assert got["bbox_min"].tolist() == [[-1] * len(shape)] * 3
        assert np.isnan(got["centroid"]).all()
    got = check(np.zeros((0,), np.int64), "uint8")
    assert got["n_labels"] == 0 and got["count"].shape == (0,)
    got = check(np.ones((1, 1, 2, 1, 3, 1, 2, 5), np.int64), "int16")  # ZT_MAX_DIMS axes
    assert got["count"].tolist() == [60] and got["bbox_max"].tolist() == [[0, 0, 1, 0, 2, 0, 1, 4]]


@pytest.mark.parametrize("shape", [(9, 9, 129), (17, 33, 70)], ids=["9x9x129", "17x33x70"])
def test_connected_components_of_noise(shape):
    import torch
    rng = np.random.default_rng(5)
    inten = rng.integers(-2 ** 31, 2 ** 31, shape).astype(np.int32)
    for density in (0.05, 0.3, 0.6, 0.95):
        mask = (rng.random(shape) < density).astype(np.uint8)
        lab, k = zt.ConnectedComponents(1).apply_ndarray(to_dev(mask, "uint8"))
        torch.cuda.synchronize()
        got = check(from_dev(lab, "uint32"), "uint32", None, inten, "int32")
        assert got["n_labels"] == k and (got["count"] > 0).all()
        assert got["background"] == int((mask == 0).sum())


@pytest.mark.parametrize("blocks,slots", [(2, 4), (1, 1), (3, 256), (65535, 2)])
def test_grid_cap_and_slot_count_knobs(monkeypatch, blocks, slots):
    """A few thousand elements reach the grid loop's second trip, probe collisions, the flush of
    a half-full table and the direct path; the result does not depend on either knob."""
    shape = (40, 150)
    rng = np.random.default_rng(11)
    inten = rng.integers(-128, 128, shape).astype(np.int8)
    monkeypatch.setenv("ZT_LABELS_MAX_BLOCKS", str(blocks))
    monkeypatch.setenv("ZT_LABELS_LDS_SLOTS", str(slots))
    for name, lab, K in layouts(shape, seed=3):
        check(lab, "int32", K, inten, "int8")
        check(lab, "int32", K)


LABEL_MAX = {"int8": 127, "uint8": 255, "int16": 32767, "uint16": 65535, "int32": 70001,
             "uint32": 70001, "int64": 70001, "uint64": 70001}


@pytest.mark.parametrize("dtype", list(LABEL_MAX))
def test_label_types_largest_values_and_invalid_elements(dtype):
    K = LABEL_MAX[dtype]  # the type's largest value where the state of that many labels is small
    shape = (5, 70)
    rng = np.random.default_rng(K)
    lab = np.where(rng.random(shape) < 0.5, rng.integers(K - 3, K + 1, shape), 0)
    lab[0, 0], lab[4, 69] = K, 1
    got = check(lab, dtype)
    assert got["n_labels"] == K and got["count"][K - 1] >= 1
    st = O.NP_STORAGE[dtype]
    # an element above K, and (signed types) a negative one: counted, reported, never written
    bad = lab.astype(st)
    bad[2, 3] = K  # still valid
    bad[3, 7] = min(K + 1, np.iinfo(st).max)
    if bad[3, 7] > K:
        with pytest.raises(zt.InvalidParameters, match=rf"label_statistics: 1 elements outside "
                                                       rf"\[0, {K}\]"):
            gpu(bad, dtype, K)
    with pytest.raises(zt.InvalidParameters, match=r"label_statistics: 3 elements outside \[0, 2\]"):
        gpu(np.array([0, 1, 2, 3, 3, 2, 7], dtype=st), dtype, 2)
    if dtype.startswith("int"):
        neg = lab.astype(st)
        neg[1, 1] = -1
        neg[4, 0] = np.iinfo(st).min
        with pytest.raises(zt.InvalidParameters, match=r"label_statistics: 2 elements outside"):
            gpu(neg, dtype, K)
    if st().itemsize == 8:  # a value whose low 32 bits are a valid label
        big = lab.astype(st)
        big[2, 2] = (1 << 32) + 1
        with pytest.raises(zt.InvalidParameters, match=r"label_statistics: 1 elements outside"):
            gpu(big, dtype, K)


def special_values(dtype):
    """Storage values of `dtype` that order non-trivially, and a NaN (floats)."""
    st = O.NP_STORAGE[dtype]
    if dtype in R.INT_TYPES:
        ii = np.iinfo(st)
        return np.array([ii.min, ii.max, 0, 1, ii.max - 1, ii.min + 1], dtype=st), None
    if dtype == "float64":
        f = np.array([-0.0, 0.0, np.inf, -np.inf, 5e-324, -5e-324, 1.5, -1.5,
                      np.finfo(np.float64).max], dtype=np.float64)
        return f, np.float64(np.nan)
    if dtype == "float32":
        f = np.array([-0.0, 0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.5, -1.5,
                      np.finfo(np.float32).max], dtype=np.float32)
        return f, np.float32(np.nan)
    if dtype == "float16":
        bits = [0x8000, 0x0000, 0x7C00, 0xFC00, 0x0001, 0x8001, 0x3E00, 0xBE00, 0x7BFF]
        return np.array(bits, dtype=np.uint16), np.uint16(0x7E01)
    bits = [0x8000, 0x0000, 0x7F80, 0xFF80, 0x0001, 0x8001, 0x3FC0, 0xBFC0, 0x7F7F]
    return np.array(bits, dtype=np.uint16), np.uint16(0xFFC1)  # bfloat16; a negative NaN


@pytest.mark.parametrize("dtype", NUMERIC)
def test_intensity_types_on_special_values(dtype):
    vals, nan = special_values(dtype)
    shape = (6, 130)
    rng = np.random.default_rng(len(dtype))
    inten = vals[rng.integers(0, len(vals), shape)]
    lab = rng.integers(0, 9, shape)
    lab[lab == 8] = 0
    if nan is not None:
        inten[rng.random(shape) < 0.2] = nan
    # label 9: the two zeros only (floats: -0.0 is the minimum, +0.0 the maximum)
    lab[5, 100:120] = 9
    inten[5, 100:120] = vals[:2][np.arange(20) % 2] if nan is not None else vals[2]
    if nan is not None:
        lab[0, 3:40] = 10  # label 10: NaN only -> none
        inten[0, 3:40] = nan
        lab[2, 63:65] = 11  # label 11: one NaN beside one value, across a 64-lane border
        inten[2, 63], inten[2, 64] = vals[6], nan
    got = check(lab, "uint16", 12, inten, dtype)
    if dtype in R.SUM_TYPES:
        assert all(type(s) is int for s in got["intensity_sum"])
    else:
        assert got["intensity_sum"] is None and got["intensity_mean"] is None
    if nan is not None:
        assert not got["intensity_valid"][9] and got["intensity_valid"][10]
        assert np.signbit(got["intensity_min"][8]) and not np.signbit(got["intensity_max"][8])
    assert not got["intensity_valid"][11]  # absent


def test_intensity_sum_carries_and_borrows():
    """One label over two tiles: -1 everywhere in the first, +1 in the second; the 128-bit sum goes
    below zero and back (in either order)."""
    lab = np.ones((2 * T, 64), np.int32)
    inten = np.concatenate([np.full((T, 64), -1), np.full((T, 64), 1)]).astype(np.int32)
    got = check(lab, "int32", None, inten, "int32")
    assert got["intensity_sum"][0] == 0
    got = check(lab, "int32", None, -np.abs(inten).astype(np.int64) * 2 ** 31, "int32")
    assert got["intensity_sum"][0] == -(2 ** 31) * 2 * T * 64
    # every element 2^32 - 1
    u = np.full((3, 200), 2 ** 32 - 1, dtype=np.uint32)
    got = check(np.where(np.indices(u.shape)[1] % 7 < 5, 2, 1), "uint8", None, u, "uint32")
    assert int(got["intensity_sum"].sum()) == (2 ** 32 - 1) * 600


def test_element_aligned_pointers_and_strided_input():
    """Labels and intensities one element past a 16-byte boundary: rows that may not be loaded by
    vectors; a non-contiguous tensor is copied."""
    import torch
    shape = (5, 128)
    rng = np.random.default_rng(2)
    lab = rng.integers(0, 6, shape).astype(np.uint16)
    inten = rng.integers(0, 255, shape).astype(np.uint8)
    want = R.label_statistics(lab, None, inten, "uint8")
    fl = to_dev(np.concatenate([[9], lab.reshape(-1)]).astype(np.uint16), "uint16")
    fi = to_dev(np.concatenate([[9], inten.reshape(-1)]).astype(np.uint8), "uint8")
    x, y = fl[1:].view(shape), fi[1:].view(shape)
    assert x.data_ptr() % 16 == 2 and y.data_ptr() % 16 == 1 and x.is_contiguous()
    f = zt.LabelStatistics()
    R.assert_same(f.apply_ndarray(x, y), want)
    R.assert_same(f.apply_ndarray(x, to_dev(inten, "uint8")), want)  # one of the two aligned
    R.assert_same(f.apply_ndarray(to_dev(lab, "uint16"), y), want)
    xt = to_dev(np.ascontiguousarray(lab.T), "uint16").t()
    assert not xt.is_contiguous()
    R.assert_same(f.apply_ndarray(xt, to_dev(inten, "uint8")), want)
    with pytest.raises(zt.InvalidParameters, match="Array shapes do not match"):
        f.apply_ndarray(x, to_dev(inten[:4], "uint8"))
    with pytest.raises(zt.UnsupportedDataType):
        f.apply_ndarray(to_dev(lab.astype(np.float32), "float32"))
    with pytest.raises(zt.UnsupportedDataType):
        f.apply_ndarray(x, zt.DeviceArray(to_dev(inten, "uint8").view(shape), shape, "bool"))
    torch.cuda.synchronize()


def test_two_halves_with_origin_equal_the_whole():
    import torch
    shape = (7, 6, 90)
    rng = np.random.default_rng(8)
    lab = rng.integers(0, 40, shape).astype(np.int64)
    inten = rng.standard_normal(shape).astype(np.float32)
    K = 41
    want = R.label_statistics(lab, K, inten, "float32")
    f = zt.LabelStatistics(K)
    state = f.new_state(3, K, True)
    f.accumulate(to_dev(lab[:3], "int64"), state, K, to_dev(inten[:3], "float32"), (0, 0, 0))
    f.accumulate(to_dev(lab[3:], "int64"), state, K, to_dev(inten[3:], "float32"), (3, 0, 0))
    R.assert_same(f.finish(state, 3, K, lab.size, "float32"), want)
    # the same through two results and combine_label_statistics; a split along x
    parts = []
    for x0, x1 in ((0, 33), (33, 90)):
        st = f.new_state(3, K, True)
        f.accumulate(to_dev(lab[..., x0:x1], "int64"), st, K,
                     to_dev(inten[..., x0:x1], "float32"), (0, 0, x0))
        parts.append(f.finish(st, 3, K, lab[..., x0:x1].size, "float32"))
    R.assert_same(zt.combine_label_statistics(parts), want)
    # an origin that is not zero moves the box
    moved = R.label_statistics(lab, K, origin=(10, 20, 1 << 33))
    st = f.new_state(3, K, False)
    f.accumulate(to_dev(lab, "int64"), st, K, None, (10, 20, 1 << 33))
    R.assert_same(f.finish(st, 3, K, lab.size), moved)
    torch.cuda.synchronize()


def test_c_abi_errors():
    lib, ctx = _abi.lib(), zt.default_context(0)
    f = zt.LabelStatistics(3)
    state = f.new_state(2, 3, False)
    x = to_dev(np.zeros((4, 4), np.uint8), "uint8")
    U8 = _abi.DTYPES["uint8"]

    def acc(shape, origin, K, dtype_i=_abi.NO_DTYPE, inten=None):
        return lib.zt_label_statistics_accumulate(
            ctx.handle, U8, x.data_ptr(), dtype_i, inten, _abi.i64_array(shape),
            None if origin is None else _abi.i64_array(origin), len(shape), K, state.data_ptr())

    with pytest.raises(zt.InvalidParameters, match="n_labels -1 not in"):
        _abi.check(acc((4, 4), None, -1))
    with pytest.raises(zt.InvalidParameters, match=r"n_labels 2147483647 not in \[0, 2147483646\]"):
        _abi.check(acc((4, 4), None, 2 ** 31 - 1))
    with pytest.raises(zt.InvalidParameters, match="origin must be >= 0"):
        _abi.check(acc((4, 4), (0, -1), 3))
    with pytest.raises(zt.InvalidParameters, match="more than 274877906944 elements"):
        _abi.check(acc((1 << 20, (1 << 18) + 1), None, 3))
    with pytest.raises(zt.InvalidParameters, match="no coordinate sum wraps"):
        _abi.check(acc((4, 4), (0, (1 << 62) - 4), 3))
    with pytest.raises(zt.InvalidParameters, match="go together"):
        _abi.check(acc((4, 4), None, 3, U8, None))
    with pytest.raises(zt.InvalidParameters, match="8-byte aligned"):
        _abi.check(lib.zt_label_statistics_init(ctx.handle, 2, 3, 0, state.data_ptr() + 4))
    with pytest.raises(zt.InvalidParameters, match=r"ndim 9 not in \[1, 8\]"):
        _abi.check(lib.zt_label_statistics_init(ctx.handle, 9, 3, 0, state.data_ptr()))
    _abi.check(acc((4, 4), None, 3))
    assert f.finish(state, 2, 3, 16)["background"] == 16


# ---- store path and zarrs_info ------------------------------------------------------------------------

SHAPE, CHUNK = (70, 45, 67), (32, 32, 32)


@pytest.fixture(scope="module")
def stored(tmp_path_factory):
    """uint16 labels with ragged chunks, the chunks of z >= 32, x >= 32 missing (they read as the
    fill value 0), and float32 intensities of the same shape in another chunk grid, sharded and
    gzip compressed, with missing shards (they read as the fill value -1.5)."""
    import json
    from zarrs_tools_amd import store as S
    root = tmp_path_factory.mktemp("labels")
    rng = np.random.default_rng(7)
    lab = np.where(rng.random(SHAPE) < 0.4, rng.integers(1, 30, SHAPE), 0).astype(np.uint16)
    lab[lab == 17] = 0  # an absent label
    S.create_array(root / "lab", "uint16", SHAPE, CHUNK, fill_value=0)
    S.write_array(root / "lab", lab[:32])
    S.write_array(root / "lab", lab[32:, :, :32], start=(32, 0, 0))
    lab[32:, :, 32:] = 0
    assert np.array_equal(S.read_array(root / "lab"), lab)
    inten = rng.standard_normal(SHAPE).astype(np.float32)
    inten[rng.random(SHAPE) < 0.1] = np.nan
    assert S.codec_available("gzip")
    enc = {"shard_shape": [40, 48, 64], "chunk_shape": [20, 16, 32], "fill_value": -1.5,
           "bytes_to_bytes_codecs": [{"name": "gzip", "configuration": {"level": 1}}]}
    S.create_output(root / "lab", root / "int", "float32", None, json.dumps(enc))
    S.write_array(root / "int", inten[:40])
    inten[40:] = -1.5
    got = S.read_array(root / "int")
    assert np.array_equal(np.isnan(got), np.isnan(inten))
    assert np.array_equal(got[~np.isnan(got)], inten[~np.isnan(inten)])
    assert S.open_array(root / "int").chunk_shape != CHUNK
    return str(root / "lab"), str(root / "int"), lab, inten


def test_store_function_and_info_command(stored, capsys):
    import json
    from zarrs_tools_amd import store as S
    from zarrs_tools_amd import zarrs_info as ZI
    lab_path, int_path, lab, inten = stored
    want = R.label_statistics(lab, None, inten, "float32")
    R.assert_same(S.label_statistics(lab_path, int_path), want)
    R.assert_same(S.label_statistics(lab_path), R.label_statistics(lab))
    R.assert_same(S.label_statistics(lab_path, n_labels=40), R.label_statistics(lab, 40))
    with pytest.raises(zt.InvalidParameters, match=r"label_statistics: \d+ elements outside \[0, 5\]"):
        S.label_statistics(lab_path, n_labels=5)
    # the command prints the same columns as JSON
    assert ZI.main([lab_path, "label-statistics", "--intensity", int_path]) == 0
    doc = json.loads(capsys.readouterr().out)
    K = want["n_labels"]
    assert doc["n_labels"] == K == 29 and doc["background"] == want["background"]
    assert doc["count"] == want["count"].tolist() and doc["count"][16] == 0
    assert doc["bbox_min"][16] is None and doc["bbox_max"][16] is None and doc["centroid"][16] is None
    assert doc["bbox_min"][0] == want["bbox_min"][0].tolist()
    assert doc["bbox_max"][28] == want["bbox_max"][28].tolist()
    assert doc["coord_sum"] == want["coord_sum"].tolist()
    assert doc["centroid"][3] == want["centroid"][3].tolist()
    assert doc["intensity_min"][16] is None and doc["intensity_sum"] is None
    assert doc["intensity_min"][2] == float(want["intensity_min"][2])
    assert doc["intensity_max"][2] == float(want["intensity_max"][2])
    assert ZI.main([lab_path, "label-statistics", "--n-labels", "31"]) == 0
    doc = json.loads(capsys.readouterr().out)
    assert doc["n_labels"] == 31 and "intensity_min" not in doc and doc["count"][30] == 0
    # --max-labels
    assert ZI.main([lab_path, "label-statistics", "--max-labels", "28"]) == 1
    out = capsys.readouterr().out
    assert "29 labels are more than --max-labels 28" in out and "store.label_statistics" in out
    assert ZI.main([lab_path, "label-statistics", "--max-labels", "29"]) == 0
    capsys.readouterr()
    # a float array has no labels; shapes must agree
    assert ZI.main([int_path, "label-statistics"]) == 1
    assert "integer type, not float32" in capsys.readouterr().out


def test_store_refusals_before_anything_is_read(stored, tmp_path, monkeypatch):
    from zarrs_tools_amd import device_io
    from zarrs_tools_amd import store as S
    lab_path, int_path, lab, inten = stored

    def no_read(*a, **k):
        raise AssertionError("an input was read")

    monkeypatch.setattr(device_io, "read_to_device", no_read)
    S.create_array(tmp_path / "other", "float32", (70, 45, 66), CHUNK, fill_value=0)
    with pytest.raises(zt.InvalidParameters, match="Array shapes do not match"):
        S.label_statistics(lab_path, tmp_path / "other")
    with pytest.raises(zt.UnsupportedDataType):
        S.label_statistics(int_path)
    need = lab.size * (2 + 4) + zt.LabelStatistics().state_bytes(3, 10, True)
    monkeypatch.setenv("ZT_STORE_DEVICE_MEMORY", str(need))  # 80 % of it is too little
    with pytest.raises(zt.FilterError, match="not enough available memory") as e:
        S.label_statistics(lab_path, int_path, n_labels=10)
    assert e.value.status == _abi.ERR_OUT_OF_MEMORY and f"needs {need} bytes" in str(e.value)
