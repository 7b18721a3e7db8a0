"""The per-label statistics and the label size filter without a GPU: the numpy restatement
(tests/labels_ref.py) against hand-written answers and scipy.ndimage, the type tables, the errors
raised before any device work, the state and memory formulas, combine_label_statistics over split
boxes and the exported symbols."""
import numpy as np
import pytest

from tests import labels_ref as R

import zarrs_tools_amd as zt
from zarrs_tools_amd import _abi
from zarrs_tools_amd import filter as F


# ---- the restatement ---------------------------------------------------------------------------

def test_restatement_hand_written():
    lab = np.array([[0, 1, 1, 0, 3],
                    [2, 1, 0, 0, 3],
                    [2, 0, 0, 0, 3]], dtype=np.int16)
    s = R.label_statistics(lab, 4)
    assert s["n_labels"] == 4 and s["background"] == 7
    assert s["count"].tolist() == [3, 2, 3, 0]
    assert s["bbox_min"].tolist() == [[0, 1], [1, 0], [0, 4], [-1, -1]]
    assert s["bbox_max"].tolist() == [[1, 2], [2, 0], [2, 4], [-1, -1]]
    assert s["coord_sum"].tolist() == [[1, 4], [3, 0], [3, 12], [0, 0]]
    assert s["centroid"][:3].tolist() == [[1 / 3, 4 / 3], [1.5, 0.0], [1.0, 4.0]]
    assert np.isnan(s["centroid"][3]).all()
    assert s["count"].dtype == np.uint64 and s["bbox_min"].dtype == np.int64
    # an origin moves the coordinates; n_labels=None is the largest label present
    s = R.label_statistics(lab, None, origin=(10, 100))
    assert s["n_labels"] == 3 and s["bbox_min"].tolist() == [[10, 101], [11, 100], [10, 104]]
    assert s["coord_sum"].tolist() == [[31, 304], [23, 200], [33, 312]]
    with pytest.raises(R.InvalidLabels, match=r"3 elements outside \[0, 2\]"):
        R.label_statistics(lab, 2)
    with pytest.raises(R.InvalidLabels, match=r"1 elements outside \[0, 3\]"):
        R.label_statistics(np.array([1, -1, 3]), 3)


def test_restatement_intensities_hand_written():
    lab = np.array([1, 1, 1, 2, 2, 3, 3, 0, 4], dtype=np.uint8)
    f = np.array([-0.0, 0.0, np.nan, np.inf, -np.inf, np.nan, np.nan, 7.0, 1e-45],
                 dtype=np.float32)
    s = R.label_statistics(lab, 5, f, "float32")
    assert s["intensity_valid"].tolist() == [True, True, False, True, False]
    assert np.signbit(s["intensity_min"][0]) and not np.signbit(s["intensity_max"][0])
    assert s["intensity_min"][1] == -np.inf and s["intensity_max"][1] == np.inf
    assert np.isnan(s["intensity_min"][2]) and s["intensity_min"][3] == np.float32(1e-45)
    assert s["intensity_sum"] is None and s["intensity_mean"] is None
    i = np.array([-128, 127, -128, 5, 6, 0, -1, 99, 127], dtype=np.int8)
    s = R.label_statistics(lab, 5, i, "int8")
    assert s["intensity_min"].tolist() == [-128, 5, -1, 127, 0]
    assert s["intensity_max"].tolist() == [127, 6, 0, 127, 0]
    assert s["intensity_sum"].tolist() == [-129, 11, -1, 127, 0]
    assert all(type(v) is int for v in s["intensity_sum"])
    assert s["intensity_mean"][:4].tolist() == [-43.0, 5.5, -0.5, 127.0]
    assert np.isnan(s["intensity_mean"][4]) and s["intensity_min"].dtype == np.int8
    # 16-bit floats are storage bits; bfloat16 widens to float32
    h = np.array([0x8000, 0x0000, 0x7E00, 0x7C00, 0xFC00, 0, 0, 0, 0x0001], dtype=np.uint16)
    s = R.label_statistics(lab, 4, h, "float16")
    assert s["intensity_min"].dtype == np.float16 and np.signbit(s["intensity_min"][0])
    s = R.label_statistics(lab, 4, h, "bfloat16")
    assert s["intensity_min"].dtype == np.float32 and s["intensity_max"][3] == np.float32(2 ** -133)
    # sums beyond 64 bits stay exact
    u = np.full(9, 2 ** 32 - 1, dtype=np.uint32)
    assert R.label_statistics(np.ones(9, np.uint8), 1, u, "uint32")["intensity_sum"][0] == \
        9 * (2 ** 32 - 1)


def test_restatement_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    for shape in ((40,), (9, 31), (5, 6, 17)):
        lab = np.where(rng.random(shape) < 0.6, rng.integers(1, 12, shape), 0).astype(np.int32)
        inten = rng.integers(-1000, 1000, shape).astype(np.int32)
        K = 13  # labels 12 and 13 are absent
        s = R.label_statistics(lab, K, inten, "int32")
        idx = np.arange(1, K + 1)
        assert s["count"].tolist() == ndi.sum_labels(np.ones(shape), lab, idx).astype(int).tolist()
        assert s["intensity_sum"].tolist() == \
            ndi.sum_labels(inten.astype(np.int64), lab, idx).astype(int).tolist()
        boxes = ndi.find_objects(lab, max_label=K)
        for j, box in enumerate(boxes):
            if box is None:
                assert s["count"][j] == 0 and (s["bbox_min"][j] == -1).all()
            else:
                assert s["bbox_min"][j].tolist() == [b.start for b in box]
                assert s["bbox_max"][j].tolist() == [b.stop - 1 for b in box]
        present = s["count"] > 0
        com = np.array(ndi.center_of_mass(np.ones(shape), lab, idx[present])).reshape(-1, len(shape))
        np.testing.assert_allclose(s["centroid"][present], com, rtol=1e-9)  # scipy sums in floats
        lo = ndi.minimum(inten, lab, idx[present])
        hi = ndi.maximum(inten, lab, idx[present])
        assert s["intensity_min"][present].tolist() == lo.tolist()
        assert s["intensity_max"][present].tolist() == hi.tolist()


def test_restatement_of_the_size_filter():
    lab = np.array([[5, 5, 5, 0, 2],
                    [9, 0, 2, 2, 2],
                    [9, 7, 0, 0, 0]], dtype=np.uint16)  # counts: 2 -> 4, 5 -> 3, 7 -> 1, 9 -> 2
    out, k = R.label_size_filter(lab, 2)
    assert k == 3 and out.dtype == np.uint16
    assert out.tolist() == [[2, 2, 2, 0, 1], [3, 0, 1, 1, 1], [3, 0, 0, 0, 0]]
    out, k = R.label_size_filter(lab, 2, 3, relabel=False)
    assert k == 2 and out.tolist() == [[5, 5, 5, 0, 0], [9, 0, 0, 0, 0], [9, 0, 0, 0, 0]]
    out, k = R.label_size_filter(lab, 1, 1, dtype_out=np.int8)
    assert k == 1 and out.dtype == np.int8 and out.sum() == 1 and out[2, 1] == 1
    assert R.label_size_filter(lab, 5)[1] == 0
    with pytest.raises(R.InvalidLabels, match="does not fit"):
        R.label_size_filter(np.array([300, 300], np.uint16), relabel=False, dtype_out=np.uint8)
    assert R.label_size_filter(np.array([300, 300], np.uint16), dtype_out=np.uint8)[1] == 1
    with pytest.raises(R.InvalidLabels, match="negative"):
        R.label_size_filter(np.array([1, -1]))


# ---- the host side of the package -----------------------------------------------------------------

def test_type_tables():
    for d in _abi.DTYPES:
        if d in R.INT_TYPES:
            zt.LabelStatistics().is_compatible(d)
            for i in _abi.DTYPES:
                if i == "bool":
                    with pytest.raises(zt.UnsupportedDataType, match="numeric type, not bool"):
                        zt.LabelStatistics().is_compatible(d, i)
                else:
                    zt.LabelStatistics().is_compatible(d, i)
            for o in _abi.DTYPES:
                if o in R.INT_TYPES:
                    zt.LabelSizeFilter().is_compatible(d, o)
                else:
                    with pytest.raises(zt.UnsupportedDataType, match=f"integer type, not {o}"):
                        zt.LabelSizeFilter().is_compatible(d, o)
        else:
            with pytest.raises(zt.UnsupportedDataType, match=f"integer type, not {d}"):
                zt.LabelStatistics().is_compatible(d)
            with pytest.raises(zt.UnsupportedDataType, match=f"integer type, not {d}"):
                zt.LabelSizeFilter().is_compatible(d, "uint32")
    with pytest.raises(zt.UnsupportedDataType):
        zt.LabelStatistics().is_compatible("uint8", "complex64")
    assert F.LABEL_SUM_TYPES == R.SUM_TYPES
    assert zt.LabelStatistics().name() == "label statistics"
    assert zt.LabelSizeFilter().name() == "label size filter"


def test_state_and_memory_formulas():
    f = zt.LabelStatistics()
    for nd in range(1, 9):
        for K in (0, 1, 7, 70000):
            assert f.state_bytes(nd, K) == 8 * ((1 + 3 * nd) * (K + 1) + 1)
            assert f.state_bytes(nd, K, True) == 8 * ((5 + 3 * nd) * (K + 1) + 1)
    assert zt.LabelStatistics(9).state_bytes(3) == 8 * (10 * 10 + 1)
    assert f.state_bytes(8, 2 ** 31 - 2, True) == 8 * (29 * (2 ** 31 - 1) + 1)
    g = zt.LabelSizeFilter()
    for K in (0, 1, 2, 255, 70001):
        scratch = 8 * (K + 2) + (4 * (K + 1) + 7) // 8 * 8 + 16
        assert g.memory("uint16", "int64", (3, 5, 7), K) == 105 * (2 + 8) + scratch
    assert g.memory("uint8", "uint8", (3, 0, 7), 9) == 0
    assert _abi.LABELS_TILE_ROWS == 16 and _abi.NO_DTYPE == -1


def test_errors_before_any_device_work():
    for K in (-1, 2 ** 31 - 1):
        with pytest.raises(zt.InvalidParameters, match=rf"n_labels {K} not in \[0, 2147483646\]"):
            zt.LabelStatistics(K)
        with pytest.raises(zt.InvalidParameters, match=rf"n_labels {K} not in \[0, 2147483646\]"):
            zt.LabelStatistics().state_bytes(3, K)
        with pytest.raises(zt.InvalidParameters, match=rf"n_labels {K} not in"):
            zt.LabelSizeFilter().memory("uint8", "uint8", (4, 4), K)
    for nd in (0, 9):
        with pytest.raises(zt.InvalidParameters, match=rf"ndim {nd} not in \[1, 8\]"):
            zt.LabelStatistics().state_bytes(nd, 3)
    with pytest.raises(zt.InvalidParameters, match="state_bytes needs n_labels"):
        zt.LabelStatistics().state_bytes(3)
    with pytest.raises(zt.InvalidParameters, match="min_size 0 is below 1"):
        zt.LabelSizeFilter(0)
    with pytest.raises(zt.InvalidParameters, match="max_size 4 is below min_size 5"):
        zt.LabelSizeFilter(5, 4)
    with pytest.raises(zt.InvalidParameters, match="more than 274877906944 elements"):
        zt.LabelSizeFilter().memory("uint8", "uint8", (1 << 20, (1 << 18) + 1), 3)
    with pytest.raises(zt.InvalidParameters, match="negative extent"):
        zt.LabelSizeFilter().memory("uint8", "uint8", (4, -1), 3)
    lib = _abi.lib()
    with pytest.raises(zt.InvalidParameters, match="null context"):
        _abi.check(lib.zt_label_statistics_init(None, 3, 3, 0, None))
    with pytest.raises(zt.InvalidParameters, match="null context"):
        _abi.check(lib.zt_label_size_filter_apply_array(None, 5, None, 5, None, None, 1, 1, -1, 1,
                                                        None))


def test_keys_decode_to_values():
    k = np.array([0, 0x7F, 0x80, 0xFF], dtype=np.uint64)
    assert F._keys_to_values(k, "uint8").tolist() == [0, 127, 128, 255]
    assert F._keys_to_values(k, "int8").tolist() == [-128, -1, 0, 127]
    k = np.array([0x007FFFFF, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFF800000], dtype=np.uint64)
    v = F._keys_to_values(k, "float32")
    assert v.dtype == np.float32 and v[0] == -np.inf and v[4] == np.inf
    assert v[1] == 0 and np.signbit(v[1]) and v[2] == 0 and not np.signbit(v[2])
    assert v[3] == np.float32(1e-45)
    assert F._keys_to_values(np.array([0xBC00], np.uint64), "float16").tolist() == [1.0]
    assert F._keys_to_values(np.array([0xBF80], np.uint64), "bfloat16").tolist() == [1.0]
    assert F._keys_to_values(np.array([1 << 63], np.uint64), "int64").tolist() == [0]
    assert F._keys_to_values(np.array([0x3FF0 << 48 | 1 << 63], np.uint64),
                             "float64").tolist() == [1.0]


def test_exact_quotients():
    num = np.array([[1, 4], [2 ** 53 + 1, 10], [7, 0]], dtype=np.uint64)
    den = np.array([3, 3, 0], dtype=np.uint64)
    q = F._quotient(num, den)
    assert q[0].tolist() == [1 / 3, 4 / 3] and q[1].tolist() == [(2 ** 53 + 1) / 3, 10 / 3]
    assert np.isnan(q[2]).all()
    big = np.empty(2, dtype=object)
    big[0], big[1] = -(2 ** 100) - 1, 2 ** 64 + 3
    q = F._exact_quotient(big, np.array([7, 3], dtype=np.uint64))
    assert q.tolist() == [(-(2 ** 100) - 1) / 7, (2 ** 64 + 3) / 3]


@pytest.mark.parametrize("dtype", ["int16", "float32", "uint64"])
def test_combine_over_split_boxes(dtype):
    rng = np.random.default_rng(3)
    shape = (6, 7, 20)
    lab = np.where(rng.random(shape) < 0.7, rng.integers(1, 9, shape), 0).astype(np.uint8)
    if dtype == "float32":
        inten = rng.standard_normal(shape).astype(np.float32)
        inten[rng.random(shape) < 0.3] = np.nan
        inten[lab == 2] = np.nan                                # label 2: none in every part
        inten[lab == 3] = np.where(rng.random(shape) < 0.5, 0.0, -0.0)[lab == 3]
    else:
        inten = rng.integers(0, 30000, shape).astype(dtype)
    K = 10
    whole = R.label_statistics(lab, K, inten, dtype)
    cuts = [(slice(0, 2),), (slice(2, 3),), (slice(3, 6), slice(0, 4)), (slice(3, 6), slice(4, 7))]
    parts = []
    for cut in cuts:
        origin = [c.start for c in cut] + [0] * (3 - len(cut))
        parts.append(R.label_statistics(lab[cut], K, inten[cut], dtype, origin=origin))
    R.assert_same(zt.combine_label_statistics(parts), whole)
    R.assert_same(zt.combine_label_statistics(reversed(parts)), whole)
    R.assert_same(zt.combine_label_statistics([whole]), whole)
    plain = [R.label_statistics(lab[c], K, origin=[s.start for s in c] + [0] * (3 - len(c)))
             for c in cuts]
    R.assert_same(zt.combine_label_statistics(plain), R.label_statistics(lab, K))
    with pytest.raises(zt.InvalidParameters, match="no parts"):
        zt.combine_label_statistics([])
    with pytest.raises(zt.InvalidParameters, match="the parts differ"):
        zt.combine_label_statistics([whole, R.label_statistics(lab, K + 1, inten, dtype)])
    with pytest.raises(zt.InvalidParameters, match="the parts differ"):
        zt.combine_label_statistics([whole, plain[0]])


def test_symbols_and_abi_version():
    syms = _abi.header_symbols()
    for name in ("zt_label_statistics_is_compatible", "zt_label_statistics_state_bytes",
                 "zt_label_statistics_init", "zt_label_statistics_accumulate",
                 "zt_label_statistics_finish", "zt_label_size_filter_is_compatible",
                 "zt_label_size_filter_memory", "zt_label_size_filter_apply_array"):
        assert name in syms
        assert hasattr(_abi.lib(), name)
    assert _abi.lib().zt_abi_version() == 4
    for name in ("LabelStatistics", "LabelSizeFilter", "combine_label_statistics",
                 "label_statistics", "label_size_filter"):
        assert name in zt.__all__ and hasattr(zt, name)


# ---- grammar: the zarrs_filter step and the zarrs_info command ------------------------------------

def test_size_filter_grammar_and_planning():
    from zarrs_tools_amd import zarrs_filter as ZF
    a = ZF.build_parser().parse_args(["label-size-filter", "in", "out"])
    assert (a.min_size, a.max_size, a.no_relabel) == (1, None, False)
    st = ZF._steps_from_cli(a)
    assert len(st) == 1 and st[0]["filter"] == "label_size_filter" and st[0]["relabel"] is True
    assert (st[0]["input"], st[0]["output"], st[0]["min_size"], st[0]["max_size"]) == \
        ("in", "out", 1, None)
    a = ZF.build_parser().parse_args(["label-size-filter", "in", "out", "--min-size", "3",
                                      "--max-size", "90", "--no-relabel", "-d", "int64",
                                      "-c", "4,4,4"])
    st = ZF._steps_from_cli(a)[0]
    assert (st["min_size"], st["max_size"], st["relabel"], st["data_type"]) == (3, 90, False, "int64")
    assert st["chunk_shape"] == [4, 4, 4] or st["chunk_shape"] == "4,4,4"
    assert "label_size_filter" in ZF.WHOLE_ARRAY and "label_size_filter" in ZF.ON_PATH
    assert not ZF.rows_splittable("label_size_filter")
    assert ZF.BINARY == ("arithmetic",)  # the statistics are no step: a table is not an array
    assert "label_statistics" not in ZF.ON_PATH
    steps = [{"filter": "equal", "input": "/x", "value": 2, "output": "$mask"},
             {"filter": "connected_components", "input": "$mask", "output": "$labels"},
             {"filter": "label_size_filter", "input": "$labels", "min_size": 5, "output": "$kept"},
             {"filter": "distance_transform", "input": "$kept", "output": "/out"}]
    assert ZF.plan_chains(steps) == [(0, 3)]
    # the step's own defaults: the input's type, fill value 0; explicit values win
    assert ZF.step_encoding({"filter": "label_size_filter"}, "uint16") == \
        {"data_type": "uint16", "fill_value": 0}
    assert ZF.step_encoding({"filter": "label_size_filter", "data_type": "int8", "fill_value": 7},
                            "uint16") == {"data_type": "int8", "fill_value": 7}
    f = ZF.label_size_filter_of({"filter": "label_size_filter", "min_size": "4", "max_size": 9,
                                 "relabel": False})
    assert (f.min_size, f.max_size, f.relabel) == (4, 9, False)
    f = ZF.label_size_filter_of({"filter": "label_size_filter"})
    assert (f.min_size, f.max_size, f.relabel) == (1, None, True)
    # the budget of the step: the most labels the type and the element count allow
    assert f.memory("uint8", "uint8", (10, 100)) == zt.LabelSizeFilter().memory(
        "uint8", "uint8", (10, 100), 255)
    assert f.memory("uint32", "uint16", (10, 100)) == zt.LabelSizeFilter().memory(
        "uint32", "uint16", (10, 100), 1000)
    with pytest.raises(zt.InvalidParameters, match="min_size and max_size are integers"):
        ZF.label_size_filter_of({"min_size": "many"})
    with pytest.raises(zt.InvalidParameters, match="min_size 0 is below 1"):
        ZF.label_size_filter_of({"min_size": 0})
    with pytest.raises(zt.InvalidParameters, match="max_size 1 is below min_size 2"):
        ZF.label_size_filter_of({"min_size": 2, "max_size": 1})


def test_info_command_grammar_and_json():
    from zarrs_tools_amd import zarrs_info as ZI
    a = ZI.build_parser().parse_args(["p", "label-statistics"])
    assert (a.intensity, a.n_labels, a.max_labels) == (None, None, 1_000_000)
    a = ZI.build_parser().parse_args(["p", "label-statistics", "--intensity", "q", "--n-labels",
                                      "7", "--max-labels", "3"])
    assert (a.path, a.intensity, a.n_labels, a.max_labels) == ("p", "q", 7, 3)
    assert ZI._DEBUG_NAMES["label-statistics"] == "LabelStatistics" and ZI._debug_command(a) == \
        "LabelStatistics"
    lab = np.array([[1, 1, 0], [3, 0, 3]], dtype=np.uint8)
    f = np.array([[np.inf, -0.0, 1], [np.nan, 2, np.nan]], dtype=np.float32)
    doc = ZI.label_statistics_json(R.label_statistics(lab, 4, f, "float32"))
    assert doc == {
        "n_labels": 4, "background": 2, "count": [2, 0, 2, 0],
        "bbox_min": [[0, 0], None, [1, 0], None], "bbox_max": [[0, 1], None, [1, 2], None],
        "coord_sum": [[0, 1], [0, 0], [2, 2], [0, 0]],
        "centroid": [[0.0, 0.5], None, [1.0, 1.0], None],
        "intensity_min": [-0.0, None, None, None], "intensity_max": ["Infinity", None, None, None],
        "intensity_sum": None, "intensity_mean": None}
    assert str(doc["intensity_min"][0]) == "-0.0"
    doc = ZI.label_statistics_json(R.label_statistics(lab, 3, lab.astype(np.int16) * -7, "int16"))
    assert doc["intensity_sum"] == [-14, 0, -42] and doc["intensity_mean"] == [-7.0, None, -21.0]
    assert doc["intensity_min"] == [-7, None, -21] and "intensity_valid" not in doc
    ZI._pretty(doc)  # serialisable: no NaN, no numpy scalars
