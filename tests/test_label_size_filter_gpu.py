"""GPU parity of the label size filter (labels.hip through the C ABI and LabelSizeFilter) against
its numpy restatement (tests/labels_ref.py): equal storage bytes and equal K' everywhere. The
counts are integer sums and the remap table a prefix sum over them, so the result is unique and no
run is repeated to look for races.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import ccl_ref as C
from tests import labels_ref as R
from tests.gpu_util import from_dev, poisoned, to_dev

pytestmark = pytest.mark.gpu

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)
from zarrs_tools_amd import _abi  # noqa: E402

T = _abi.LABELS_TILE_ROWS


def gpu(lab, dtype="uint32", dtype_out=None, **kw):
    import torch
    dtype_out = dtype_out or dtype
    y = poisoned(lab.shape, dtype_out)
    out, k = zt.LabelSizeFilter(**kw).apply_ndarray(to_dev(lab, dtype), dtype_out, out=y)
    torch.cuda.synchronize()
    assert out is y
    return from_dev(y, dtype_out), k


def check(lab, dtype="uint32", dtype_out=None, **kw):
    lab = np.ascontiguousarray(lab, dtype=O.NP_STORAGE[dtype])
    ref, k_ref = R.label_size_filter(lab, dtype_out=O.NP_STORAGE[dtype_out or dtype], **kw)
    out, k = gpu(lab, dtype, dtype_out, **kw)
    assert k == k_ref, (lab.shape, kw, k, k_ref)
    assert out.dtype == ref.dtype and out.tobytes() == ref.tobytes(), (lab.shape, kw)
    return k


def blobs(shape, seed, labels=9):
    """Labels of very different sizes, some absent, some of one element."""
    rng = np.random.default_rng(seed)
    lab = rng.choice(np.arange(labels + 1), size=shape,
                     p=np.array([30] + [2 ** (j % 6) for j in range(labels)]) /
                     (30 + sum(2 ** (j % 6) for j in range(labels))))
    return np.where(lab == 4, 0, lab)  # label 4 is absent


SHAPES = ([(3, 5, e) for e in (1, 2, 63, 64, 65, 129, 80)] + [(e, 70) for e in (1, T, T + 1)]
          + [(37,), (9, 70), (3, 4, 9, 17), (2, 2, 3, 5, 9), (40, 4100)])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_bounds_and_relabel(shape):
    lab = blobs(shape, len(shape) + shape[-1])
    n = lab.size
    for relabel in (True, False):
        for kw in (dict(min_size=1), dict(min_size=2), dict(min_size=n + 1),
                   dict(max_size=max(1, n // 40)), dict(min_size=3, max_size=max(3, n // 10))):
            check(lab, relabel=relabel, **kw)
    assert check(np.zeros(shape, np.int64)) == 0
    assert check(np.ones(shape, np.int64), min_size=n) == 1
    assert check(np.ones(shape, np.int64), max_size=n - 1 or 1) == (1 if n == 1 else 0)


def test_zero_extent_is_a_no_op():
    for shape in ((0,), (3, 0, 5)):
        out, k = gpu(np.zeros(shape, np.uint8), "uint8")
        assert k == 0 and out.shape == shape


def test_connected_components_stay_in_first_element_order():
    """On the labelling's output, relabel=True equals the labelling of the kept mask."""
    import torch
    shape = (9, 17, 70)
    mask = (np.random.default_rng(4).random(shape) < 0.35).astype(np.uint8)
    lab, k = zt.ConnectedComponents(1).apply_ndarray(to_dev(mask, "uint8"))
    torch.cuda.synchronize()
    lab = from_dev(lab, "uint32")
    out, kept = gpu(lab, "uint32", min_size=3)
    ref, k_ref = C.connected_components((out != 0).astype(np.uint8), "uint8", 1, "uint32")
    assert 0 < kept < k and kept == k_ref and out.tobytes() == ref.tobytes()
    check(lab, min_size=3)
    check(lab, min_size=2, max_size=5, relabel=False)


@pytest.mark.parametrize("dtype_in", R.INT_TYPES)
def test_type_table(dtype_in):
    lab = blobs((5, 70), 6)
    for dtype_out in R.INT_TYPES:
        check(lab, dtype_in, dtype_out, min_size=2)
        check(lab, dtype_in, dtype_out, min_size=2, relabel=False)
    for bad in ("bool", "float32", "bfloat16"):
        with pytest.raises(zt.UnsupportedDataType):
            zt.LabelSizeFilter().apply_ndarray(to_dev(lab, dtype_in), bad)
    with pytest.raises(zt.UnsupportedDataType):
        zt.LabelSizeFilter().apply_ndarray(to_dev(lab.astype(np.float32), "float32"))


def test_labels_that_do_not_fit_leave_the_output_untouched():
    import torch
    lab = np.repeat(np.arange(1, 301), 2).reshape(6, 100)  # 300 labels of 2 elements
    lab[0, :2] = 0                                          # label 1 is absent
    lab[1, 0] = 0                                           # label 51 has one element
    for keep, fits in ((255, True), (256, False)):
        a = np.repeat(np.arange(1, keep + 1), 2).reshape(2, keep)
        a = np.concatenate([a, np.full((1, keep), 0)])
        a[2, 0] = 1000  # one element: dropped at min_size 2, and above uint8 before the renumbering
        if fits:
            assert check(a, "uint16", "uint8", min_size=2) == 255
        else:
            y = poisoned(a.shape, "uint8")
            with pytest.raises(zt.InvalidParameters, match="the largest label 256 does not fit uint8"):
                zt.LabelSizeFilter(min_size=2).apply_ndarray(to_dev(a, "uint16"), "uint8", out=y)
            torch.cuda.synchronize()
            assert (from_dev(y, "uint8") == 255).all()
    # without relabel the largest kept value decides
    y = poisoned(lab.shape, "uint8")
    with pytest.raises(zt.InvalidParameters, match="the largest label 300 does not fit uint8"):
        zt.LabelSizeFilter(relabel=False).apply_ndarray(to_dev(lab, "uint16"), "uint8", out=y)
    torch.cuda.synchronize()
    assert (from_dev(y, "uint8") == 255).all()
    assert check(np.where(lab > 255, 0, lab), "uint16", "uint8", relabel=False) == 254
    assert check(lab, "uint16", "int16", min_size=2, relabel=False) == 298


def test_errors():
    lab = blobs((5, 70), 6)
    for kw, msg in ((dict(min_size=0), "min_size 0 is below 1"),
                    (dict(min_size=3, max_size=2), "max_size 2 is below min_size 3")):
        with pytest.raises(zt.InvalidParameters, match=msg):
            zt.LabelSizeFilter(**kw)
    neg = lab.astype(np.int16)
    neg[3, 3] = -2
    y = poisoned(lab.shape, "int16")
    with pytest.raises(zt.InvalidParameters, match="negative element"):
        zt.LabelSizeFilter().apply_ndarray(to_dev(neg, "int16"), out=y)
    assert (from_dev(y, "int16") == 32767).all()
    big = lab.astype(np.uint32)
    big[0, 0] = 2 ** 31 - 1
    with pytest.raises(zt.InvalidParameters, match="the largest label 2147483647 is above"):
        zt.LabelSizeFilter().apply_ndarray(to_dev(big, "uint32"))
    with pytest.raises(zt.InvalidParameters, match="Array shapes do not match"):
        zt.LabelSizeFilter().apply_ndarray(to_dev(lab, "uint8"), out=poisoned((5, 69), "uint8"))
    x = to_dev(lab, "uint8")
    lib, ctx = _abi.lib(), zt.default_context(0)
    U8 = _abi.DTYPES["uint8"]
    args = (ctx.handle, U8, x.data_ptr(), U8, x.data_ptr(), _abi.i64_array(lab.shape), 2)
    with pytest.raises(zt.InvalidParameters, match="must not overlap"):
        _abi.check(lib.zt_label_size_filter_apply_array(*args, 1, -1, 1, None))
    with pytest.raises(zt.InvalidParameters, match="min_size 0 is below 1"):
        _abi.check(lib.zt_label_size_filter_apply_array(*args, 0, -1, 1, None))


def test_knobs_and_element_aligned_pointer(monkeypatch):
    lab = blobs((40, 150), 9, labels=40).astype(np.uint16)
    flat = to_dev(np.concatenate([[7], lab.reshape(-1)]).astype(np.uint16), "uint16")
    x = flat[1:].view(lab.shape)
    assert x.data_ptr() % 16 == 2
    ref, k_ref = R.label_size_filter(lab, 4, 200)
    for blocks, slots in ((None, None), (2, 4), (1, 1)):
        if blocks:
            monkeypatch.setenv("ZT_LABELS_MAX_BLOCKS", str(blocks))
            monkeypatch.setenv("ZT_LABELS_LDS_SLOTS", str(slots))
        out, k = zt.LabelSizeFilter(4, 200).apply_ndarray(x)
        assert k == k_ref and from_dev(out, "uint16").tobytes() == ref.tobytes()
        check(lab, "uint16", min_size=4, max_size=200)


# ---- store path ---------------------------------------------------------------------------------------

SHAPE, CHUNK = (70, 45, 67), (32, 32, 32)


@pytest.fixture(scope="module")
def stored(tmp_path_factory):
    """uint16 labels with ragged chunks; the chunks of z >= 32, x >= 32 are missing (fill 0)."""
    from zarrs_tools_amd import store as S
    root = tmp_path_factory.mktemp("lsf")
    lab = blobs(SHAPE, 12, labels=300).astype(np.uint16)
    S.create_array(root / "in", "uint16", SHAPE, CHUNK, fill_value=0)
    S.write_array(root / "in", lab[:32])
    S.write_array(root / "in", lab[32:, :, :32], start=(32, 0, 0))
    lab[32:, :, 32:] = 0
    return str(root / "in"), lab


def test_store_function(stored, tmp_path):
    import json
    from zarrs_tools_amd import store as S
    src, lab = stored
    ref, k_ref = R.label_size_filter(lab, 300, 4000)
    st = S.label_size_filter(src, tmp_path / "a", 300, 4000)
    assert 0 < k_ref < 299 and st["components"] == k_ref and st["voxels"] == lab.size
    a = S.open_array(tmp_path / "a")
    assert a.data_type == "uint16" and a.shape == SHAPE and a.chunk_shape == CHUNK
    assert a.metadata["fill_value"] == 0
    assert S.read_array(tmp_path / "a").tobytes() == ref.tobytes()
    # sharded and gzip compressed, another type, the values kept
    ref, k_ref = R.label_size_filter(lab, 300, relabel=False, dtype_out=np.int32)
    enc = {"shard_shape": [32, 32, 64], "chunk_shape": [16, 16, 32],
           "bytes_to_bytes_codecs": [{"name": "gzip", "configuration": {"level": 1}}]}
    st = S.label_size_filter(src, tmp_path / "b", 300, relabel=False, data_type="int32",
                             encoding=json.dumps(enc))
    b = S.open_array(tmp_path / "b")
    assert st["components"] == k_ref and b.data_type == "int32"
    assert b.chunk_shape == (32, 32, 64) and b.inner_chunk_shape == (16, 16, 32)
    assert S.read_array(tmp_path / "b").tobytes() == ref.tobytes()


def test_store_overflow_and_memory_refusals_write_nothing(stored, tmp_path, monkeypatch):
    from tests import occ_ref
    from zarrs_tools_amd import device_io
    from zarrs_tools_amd import store as S
    src, lab = stored
    _, kept = R.label_size_filter(lab, 1)
    assert kept > 255
    with pytest.raises(zt.InvalidParameters, match=f"the largest label {kept} does not fit uint8"):
        S.label_size_filter(src, tmp_path / "u8", data_type="uint8")
    assert not (tmp_path / "u8" / "zarr.json").exists()
    assert occ_ref.chunk_files(tmp_path / "u8") == set()
    need = zt.LabelSizeFilter().memory("uint16", "uint16", SHAPE, 65535)

    def no_read(*a, **k):
        raise AssertionError("the input was read")

    monkeypatch.setattr(device_io, "read_to_device", no_read)
    monkeypatch.setenv("ZT_STORE_DEVICE_MEMORY", str(need))  # 80 % of it is too little
    with pytest.raises(zt.FilterError, match="not enough available memory") as e:
        S.label_size_filter(src, tmp_path / "out")
    assert e.value.status == _abi.ERR_OUT_OF_MEMORY and f"needs {need} bytes" in str(e.value)
    assert not (tmp_path / "out" / "zarr.json").exists()


# ---- the zarrs_filter step ----------------------------------------------------------------------------

QUIET = dict(log=lambda *a: None)


def test_subcommand_and_run_config(stored, tmp_path):
    import json
    from zarrs_tools_amd import store as S
    from zarrs_tools_amd import zarrs_filter as ZF
    src, lab = stored
    ref, k_ref = R.label_size_filter(lab, 300, 4000)
    assert ZF.main(["label-size-filter", src, str(tmp_path / "a"), "--min-size", "300",
                    "--max-size", "4000"]) == 0
    a = S.open_array(tmp_path / "a")
    assert a.data_type == "uint16" and a.chunk_shape == CHUNK and a.metadata["fill_value"] == 0
    assert S.read_array(tmp_path / "a").tobytes() == ref.tobytes()
    # sharded and gzip compressed, another type, values kept
    ref2, k2 = R.label_size_filter(lab, 300, relabel=False, dtype_out=np.uint32)
    argv = ["label-size-filter", src, str(tmp_path / "b"), "--min-size", "300", "--no-relabel",
            "--data-type", "uint32", "-s", "32,32,64", "-c", "16,16,32",
            "--bytes-to-bytes-codecs", json.dumps([{"name": "gzip", "configuration": {"level": 1}}])]
    assert ZF.main(argv) == 0
    b = S.open_array(tmp_path / "b")
    assert b.data_type == "uint32" and b.chunk_shape == (32, 32, 64)
    assert b.inner_chunk_shape == (16, 16, 32)
    assert S.read_array(tmp_path / "b").tobytes() == ref2.tobytes()
    # a run config; the step logs K'
    lines = []
    cfg = [{"filter": "label_size_filter", "input": src, "output": str(tmp_path / "c"),
            "min_size": 300, "max_size": 4000, "data_type": "int32"}]
    (tmp_path / "run.json").write_text(json.dumps(cfg))
    assert ZF.main([str(tmp_path / "run.json"), "--tmp", str(tmp_path)]) == 0
    assert S.read_array(tmp_path / "c").tobytes() == ref.astype(np.int32).tobytes()
    res = ZF.run(cfg, log=lines.append)
    assert res[0]["components"] == k_ref and f"   {k_ref} components" in lines
    # an overflow leaves no chunk and no zarr.json
    from tests import occ_ref
    assert ZF.main(["label-size-filter", src, str(tmp_path / "u8"), "-d", "uint8"]) == 1
    assert not (tmp_path / "u8" / "zarr.json").exists()
    assert occ_ref.chunk_files(tmp_path / "u8") == set()


def test_skip_empty_chunks(stored, tmp_path):
    from tests import occ_ref
    from zarrs_tools_amd import store as S
    from zarrs_tools_amd import zarrs_filter as ZF
    src, lab = stored
    ref, _ = R.label_size_filter(lab, 300, 4000)
    argv = ["label-size-filter", src, str(tmp_path / "e"), "--min-size", "300", "--max-size", "4000"]
    assert ZF.main(argv + ["--skip-empty-chunks"]) == 0
    want = occ_ref.expected_files(ref, CHUNK, 0)
    assert want < occ_ref.all_files(SHAPE, CHUNK)  # the missing chunks are background only
    assert occ_ref.chunk_files(tmp_path / "e") == want
    assert S.read_array(tmp_path / "e").tobytes() == ref.tobytes()
    argv[2] = str(tmp_path / "f")
    assert ZF.main(argv) == 0
    assert occ_ref.chunk_files(tmp_path / "f") == occ_ref.all_files(SHAPE, CHUNK)


def test_four_step_chain_against_the_store_steps(stored, tmp_path):
    from tests import edt_ref  # noqa: F401  (the chain's last step has its own tests)
    from zarrs_tools_amd import store as S
    from zarrs_tools_amd import zarrs_filter as ZF
    src, lab = stored
    value = int(np.bincount(lab.reshape(-1))[1:].argmax()) + 1  # the most frequent label
    steps = [{"filter": "equal", "input": src, "value": value, "output": "$mask"},
             {"filter": "connected_components", "input": "$mask", "output": "$labels"},
             {"filter": "label_size_filter", "input": "$labels", "min_size": 2, "output": "$kept"},
             {"filter": "distance_transform", "input": "$kept", "output": str(tmp_path / "chain")}]
    assert ZF.plan_chains(steps) == [(0, 3)]
    lines = []
    res = ZF.run(steps, tmp=str(tmp_path), log=lines.append)
    assert all(st.get("device_resident") for st in res)
    steps[3]["output"] = str(tmp_path / "store")
    res2 = ZF.run(steps, tmp=str(tmp_path), device_chain=False, **QUIET)
    assert not res2[0].get("device_resident")
    labels, k = C.connected_components((lab == value).astype(np.uint8), "bool", 1)
    kept, k_kept = R.label_size_filter(labels, 2)
    assert 0 < k_kept < k
    assert res[1]["components"] == res2[1]["components"] == k
    assert res[2]["components"] == res2[2]["components"] == k_kept
    assert f"   {k} components" in lines and f"   {k_kept} components" in lines
    chain, store = S.read_array(tmp_path / "chain"), S.read_array(tmp_path / "store")
    assert chain.dtype == np.float32 and chain.tobytes() == store.tobytes()
    assert np.array_equal(chain == 0, kept == 0)  # distances vanish exactly on what was dropped


def test_two_gpus_run_the_step_in_one_process(stored, tmp_path):
    from zarrs_tools_amd import store as S
    from zarrs_tools_amd import zarrs_filter as ZF
    src, lab = stored
    ref, k_ref = R.label_size_filter(lab, 300)
    lines = []
    steps = [{"filter": "label_size_filter", "input": src, "min_size": 300,
              "output": str(tmp_path / "two")}]
    res = ZF.run(steps, gpus=2, gpu_devices=[0, 0], log=lines.append)
    assert "processes" not in res[0] and res[0]["components"] == k_ref
    assert any("label_size_filter" in line and "one process on device 0, not 2" in line
               for line in lines)
    assert S.read_array(tmp_path / "two").tobytes() == ref.tobytes()
