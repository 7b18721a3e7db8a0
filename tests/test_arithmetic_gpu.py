"""GPU parity of the two-array arithmetic filter (arithmetic.hip through the C ABI, the store
path, the zarrs_filter command and run configs) against its numpy restatement
(tests/arith_ref.py): bit-exact for every type in every position.

Borders of the kernel (arithmetic.hip): the run is cut into vectors of V = 16 / (the smallest of
the three element sizes) elements, aligned on the stream with the smallest element (the output on
a tie, then the first input); a lane carries 16 elements (16 / V vectors) per step, so a
workgroup of 256 lanes covers STEP = 4096 elements per step; the elements before the first
aligned vector and after the last whole one go element by element.
"""
import ctypes
import json

import numpy as np
import pytest

from oracle import oracle as O
from tests import arith_ref as A
from tests import occ_ref
from tests import pw_ref as R
from tests.gpu_util import from_dev, poisoned, to_dev

pytestmark = pytest.mark.gpu

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)
from zarrs_tools_amd import _abi  # noqa: E402
from zarrs_tools_amd import store as S  # noqa: E402
from zarrs_tools_amd import zarrs_filter as ZF  # noqa: E402

ALL = list(_abi.DTYPES)
SIZE = {dt: np.dtype(O.NP_STORAGE[dt]).itemsize for dt in ALL}
OPS = zt.ARITHMETIC_OPERATORS
QUIET = dict(log=lambda *a: None)
STEP = 256 * 16
# a type triple (first, second, out) for each triple of element sizes
TYPES = {(1, 1, 1): ("uint8", "int8", "uint8"), (2, 2, 2): ("uint16", "float16", "int16"),
         (4, 4, 4): ("float32", "int32", "float32"), (8, 8, 8): ("float64", "int64", "float64"),
         (4, 1, 4): ("float32", "uint8", "float32"), (1, 8, 2): ("uint8", "float64", "bfloat16"),
         (8, 2, 1): ("int64", "uint16", "uint8"), (1, 8, 4): ("int8", "uint64", "int32")}


def V(*dts):
    return 16 // min(SIZE[d] for d in dts)


def values(dt, n, seed=0):
    """n elements of dt: the type's special values first, then noise."""
    return R.type_values(dt, n, seed)[:n]


def gpu(a, da, b, db, op, dout):
    import torch
    y = poisoned(a.shape, dout)
    out = zt.Arithmetic(op).apply_ndarray(to_dev(a, da), to_dev(b, db), dout, out=y)
    torch.cuda.synchronize()
    assert out is y
    return from_dev(y, dout)


def read(path):
    """A store array as the restatement holds it (bool as u8)."""
    a = S.read_array(path)
    return a.view(np.uint8) if a.dtype == np.bool_ else a


# ---- flat lengths ----------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes", [(1, 1, 1), (2, 2, 2), (4, 4, 4), (8, 8, 8), (4, 1, 4),
                                   (1, 8, 2), (8, 2, 1)])
def test_flat_lengths(sizes):
    da, db, dout = TYPES[sizes]
    assert (SIZE[da], SIZE[db], SIZE[dout]) == sizes
    v_ = V(da, db, dout)
    for k, n in enumerate((0, 1, v_ - 1, v_, v_ + 1, 256 * v_ + 3, STEP + 3)):
        a, b = values(da, n, n), values(db, n, n + 1)[::-1].copy()
        op = OPS[k % len(OPS)]
        R.assert_same_bits(gpu(a, da, b, db, op, dout), A.arithmetic(a, da, b, db, op, dout), dout)


# ---- every type in every position ----------------------------------------------------------------------

N = 4100


@pytest.mark.parametrize("position", ["first", "second", "out"])
@pytest.mark.parametrize("dt", ALL)
def test_every_type_in_every_position(dt, position):
    da, db, dout = {"first": (dt, "float32", dt), "second": ("float32", dt, "float32"),
                    "out": ("float32", "int16", dt)}[position]
    # the second array reversed: special values meet noise, and each other in the middle
    a, b = values(da, N, 3), values(db, N, 4)[::-1].copy()
    b[:40] = values(db, 40, 5)  # ... and the special values of both types meet, shifted by one
    a[1:41] = values(da, 40, 6)
    for op in OPS:
        R.assert_same_bits(gpu(a, da, b, db, op, dout), A.arithmetic(a, da, b, db, op, dout), dout)


def test_device_arrays_and_default_type():
    import torch
    a, b = values("uint16", 600, 1).reshape(10, 6, 10), values("int8", 600, 2).reshape(10, 6, 10)
    f = zt.Arithmetic("absolute-difference")
    out = f.apply_ndarray(to_dev(a, "uint16"), to_dev(b, "int8"))
    torch.cuda.synchronize()
    assert zt.dtype_of(out) == "uint16"  # the first array's type
    ref = A.arithmetic(a, "uint16", b, "int8", "absolute_difference")
    R.assert_same_bits(from_dev(out, "uint16"), ref, "uint16")
    y = poisoned(a.shape, "float32")
    f.apply(zt.DeviceArray(to_dev(a, "uint16"), (4, 4, 4)), zt.DeviceArray(to_dev(b, "int8"),
            (4, 4, 4)), zt.DeviceArray(y, (4, 4, 4)))
    torch.cuda.synchronize()
    R.assert_same_bits(from_dev(y, "float32"),
                       A.arithmetic(a, "uint16", b, "int8", "absolute_difference", "float32"),
                       "float32")
    with pytest.raises(zt.InvalidParameters, match=r"Array shapes do not match: \[10, 6, 10\]"):
        f.apply_ndarray(to_dev(a, "uint16"), to_dev(b[:9], "int8"))


# ---- misaligned pointers ---------------------------------------------------------------------------

@pytest.mark.parametrize("sizes", [(1, 1, 1), (4, 4, 4), (1, 8, 4)])
def test_views_one_element_into_their_buffers(sizes):
    import torch
    da, db, dout = TYPES[sizes]
    assert (SIZE[da], SIZE[db], SIZE[dout]) == sizes
    v_ = V(da, db, dout)
    for n in (1, v_ - 1, 3 * v_ + 2):
        a, b = values(da, n + 2, n), values(db, n + 2, n + 7)[::-1].copy()
        x, w = to_dev(a, da), to_dev(b, db)
        for oa in (0, 1):
            for ob in (0, 1):
                for oo in (0, 1):
                    y = poisoned((n + 2,), dout)
                    guard = from_dev(y, dout).copy()
                    _abi.check(_abi.lib().zt_arithmetic_apply(
                        zt.default_context().handle, _abi.AR_OPERATORS["subtract"],
                        _abi.DTYPES[da], ctypes.c_void_p(x.data_ptr() + oa * SIZE[da]),
                        _abi.DTYPES[db], ctypes.c_void_p(w.data_ptr() + ob * SIZE[db]), n,
                        _abi.DTYPES[dout], ctypes.c_void_p(y.data_ptr() + oo * SIZE[dout])))
                    torch.cuda.synchronize()
                    out = from_dev(y, dout)
                    ref = A.arithmetic(a[oa:oa + n], da, b[ob:ob + n], db, "subtract", dout)
                    R.assert_same_bits(out[oo:oo + n], ref, dout)
                    # the elements before and after the view are untouched
                    assert out[:oo].tobytes() == guard[:oo].tobytes()
                    assert out[oo + n:].tobytes() == guard[oo + n:].tobytes()


def test_grid_stride_second_trip(monkeypatch):
    # two workgroups: 2 * STEP elements per trip of the grid-stride loop; 2.5 trips
    monkeypatch.setenv("ZT_AR_MAX_BLOCKS", "2")
    n = 5 * STEP + 5
    a, b = values("uint16", n, 1), values("float32", n, 2)[::-1].copy()
    R.assert_same_bits(gpu(a, "uint16", b, "float32", "multiply", "float32"),
                       A.arithmetic(a, "uint16", b, "float32", "multiply", "float32"), "float32")


def test_abi_argument_checks():
    x = to_dev(np.zeros(8, dtype=np.uint16), "uint16")
    h, p = zt.default_context().handle, ctypes.c_void_p(x.data_ptr())
    u16 = _abi.DTYPES["uint16"]
    L = _abi.lib()
    _abi.check(L.zt_arithmetic_apply(h, 0, u16, None, u16, None, 0, u16, None))  # n == 0
    with pytest.raises(zt.InvalidParameters, match="unknown arithmetic operator"):
        _abi.check(L.zt_arithmetic_apply(h, 7, u16, p, u16, p, 4, u16, p))
    with pytest.raises(zt.InvalidParameters, match="element aligned"):
        _abi.check(L.zt_arithmetic_apply(h, 0, u16, ctypes.c_void_p(x.data_ptr() + 1), u16, p, 4,
                                         u16, p))
    with pytest.raises(zt.UnsupportedDataType):
        _abi.check(L.zt_arithmetic_apply(h, 0, u16, p, 99, p, 4, u16, p))


# ---- store path ------------------------------------------------------------------------------------------------

SHAPE, CHUNK, FILL = (37, 50, 70), (16, 32, 32), 7
CHUNK2, FILL2 = (24, 50, 35), -2.5


@pytest.fixture(scope="module")
def stored(tmp_path_factory):
    """first: uint16 with ragged chunks and the chunks of z >= 16, x >= 32 missing (they read as
    the fill value 7). second: float32 on another chunk grid, taller than the first's rows and not
    dividing them, with the chunks of its last row missing; once plain and once sharded and gzip
    compressed. Returns (root, first as it reads, second as it reads)."""
    root = tmp_path_factory.mktemp("ar")
    v = (O.synth_u16(SHAPE) // 5).astype(np.uint16)
    v[::7, ::5, ::3] = 0
    S.create_array(root / "first", "uint16", SHAPE, CHUNK, fill_value=FILL)
    S.write_array(root / "first", v[:16])
    S.write_array(root / "first", v[16:, :, :32], start=(16, 0, 0))
    v[16:, :, 32:] = FILL
    assert np.array_equal(S.read_array(root / "first"), v)
    w = (O.synth_step_noise_f32(SHAPE) / 3).astype(np.float32)
    w[::5, ::3, ::2] = 0.0
    w[24:] = FILL2
    S.create_array(root / "second", "float32", SHAPE, CHUNK2, fill_value=FILL2)
    S.write_array(root / "second", w[:24])
    assert S.codec_available("gzip")
    S.create_array(root / "second_sharded", "float32", SHAPE, CHUNK2,
                   S.codecs_json("gzip", 1, shard_inner=(12, 25, 35)), fill_value=FILL2)
    S.write_array(root / "second_sharded", w[:24])
    for name in ("second", "second_sharded"):
        assert np.array_equal(S.read_array(root / name), w)
    return root, v, w


@pytest.mark.parametrize("second", ["second", "second_sharded"])
@pytest.mark.parametrize("dt", [None, "float32"])
def test_store_function_subcommand_and_run_config(stored, tmp_path, second, dt):
    root, v, w = stored
    dout = dt or "uint16"
    first, other = str(root / "first"), str(root / second)
    for op in ("divide", "subtract"):
        ref = A.arithmetic(v, "uint16", w, "float32", op, dout)
        st = S.arithmetic(first, other, tmp_path / "a", op, data_type=dt)
        assert st["voxels"] == v.size and st["kernel_s"] > 0 and st["rows"] == 3
        a = S.open_array(tmp_path / "a")
        assert a.data_type == dout and a.shape == SHAPE and a.chunk_shape == CHUNK
        R.assert_same_bits(read(tmp_path / "a"), ref, dout)
    # the subcommand, into a sharded output whose rows are twice the first array's
    argv = ["arithmetic", first, str(tmp_path / "b"), "absolute-difference", other] + (
        ["--data-type", dt] if dt else []) + ["-s", "32,32,64", "-c", "16,16,32"]
    assert ZF.main(argv) == 0
    b = S.open_array(tmp_path / "b")
    assert b.chunk_shape == (32, 32, 64) and b.inner_chunk_shape == (16, 16, 32)
    ref = A.arithmetic(v, "uint16", w, "float32", "absolute_difference", dout)
    R.assert_same_bits(read(tmp_path / "b"), ref, dout)
    # a run config; the operands the other way round: the output follows the float32 array
    cfg = [{"filter": "arithmetic", "input": other, "other": first, "operator": "maximum",
            "output": str(tmp_path / "c"), **({"data_type": dt} if dt else {})}]
    (tmp_path / "run.json").write_text(json.dumps(cfg))
    assert ZF.main([str(tmp_path / "run.json"), "--tmp", str(tmp_path)]) == 0
    c = S.open_array(tmp_path / "c")
    assert c.data_type == "float32" and c.chunk_shape == CHUNK2
    R.assert_same_bits(read(tmp_path / "c"),
                       A.arithmetic(w, "float32", v, "uint16", "maximum", "float32"), "float32")


def test_chunk_limit_and_row_ranges(stored, tmp_path):
    root, v, w = stored
    first, other = str(root / "first"), str(root / "second")
    ref = A.arithmetic(v, "uint16", w, "float32", "add", "float32")
    st = S.arithmetic(first, other, tmp_path / "lim", "add", data_type="float32", chunk_limit=1)
    assert st["rows_in_flight"] == 1 and not st["double_buffered"] and st["threads"] == 1
    R.assert_same_bits(read(tmp_path / "lim"), ref, "float32")
    S.arithmetic(first, other, tmp_path / "rows", "add", data_type="float32", rows=(0, 2),
                 finish=False)
    S.arithmetic(first, other, tmp_path / "rows", "add", data_type="float32", rows=(2, 3),
                 erase=False)
    R.assert_same_bits(read(tmp_path / "rows"), ref, "float32")


def test_subtracting_an_array_from_itself_elides_every_chunk(tmp_path):
    shape, chunk = (20, 12, 10), (8, 5, 4)
    src = str(tmp_path / "in")
    S.create_array(src, "uint16", shape, chunk, fill_value=0)
    S.write_array(src, O.synth_u16(shape))
    n_chunks = len(occ_ref.all_files(shape, chunk))
    assert ZF.main(["arithmetic", src, str(tmp_path / "cli"), "subtract", src,
                    "--skip-empty-chunks"]) == 0
    assert occ_ref.chunk_files(tmp_path / "cli") == set()
    assert not read(tmp_path / "cli").any()
    S.set_store_empty_chunks(False)
    try:
        st = S.arithmetic(src, src, tmp_path / "out", "subtract")
        assert st["chunks_elided"] == n_chunks and S.last_elided() == (n_chunks, n_chunks)
    finally:
        S.set_store_empty_chunks(True)
    assert occ_ref.chunk_files(tmp_path / "out") == set()
    # stored in full otherwise
    st = S.arithmetic(src, src, tmp_path / "full", "subtract")
    assert st["chunks_elided"] == 0
    assert occ_ref.chunk_files(tmp_path / "full") == occ_ref.all_files(shape, chunk)


def test_rows_split_over_two_processes(stored, tmp_path):
    root, v, w = stored
    steps = [{"filter": "arithmetic", "input": str(root / "first"),
              "other": str(root / "second_sharded"), "operator": "multiply",
              "output": str(tmp_path / "one"), "data_type": "float32"}]
    ZF.run(steps, **QUIET)
    steps[0]["output"] = str(tmp_path / "two")
    st = ZF.run(steps, gpus=2, gpu_devices=[0, 0], **QUIET)
    assert st[0]["processes"] == 2 and st[0]["voxels"] == v.size
    ref = A.arithmetic(v, "uint16", w, "float32", "multiply", "float32")
    R.assert_same_bits(read(tmp_path / "one"), ref, "float32")
    R.assert_same_bits(read(tmp_path / "two"), ref, "float32")


def test_difference_of_gaussians_as_one_run_config(stored, tmp_path):
    root, v, w = stored
    src = str(root / "first")
    g1 = {"filter": "gaussian", "input": src, "sigma": [1.0] * 3, "kernel_half_size": [3] * 3,
          "data_type": "float32"}
    g2 = {"filter": "gaussian", "input": src, "sigma": [2.0] * 3, "kernel_half_size": [6] * 3,
          "data_type": "float32"}
    cfg = [{**g1, "output": "$a"}, {**g2, "output": "$b"},
           {"filter": "arithmetic", "input": "$a", "other": "$b", "operator": "subtract",
            "output": str(tmp_path / "dog")}]
    assert ZF.plan_chains(cfg) == []
    res = ZF.run(cfg, tmp=str(tmp_path), **QUIET)
    assert len(res) == 3 and not any(st.get("device_resident") for st in res)
    # the two Gaussian steps on their own, to real paths
    ZF.run([{**g1, "output": str(tmp_path / "ga")}], **QUIET)
    ZF.run([{**g2, "output": str(tmp_path / "gb")}], **QUIET)
    ga, gb = read(tmp_path / "ga"), read(tmp_path / "gb")
    assert ga.dtype == np.float32 and not np.array_equal(ga, gb)
    ref = A.arithmetic(ga, "float32", gb, "float32", "subtract")
    assert np.count_nonzero(ref) > ref.size // 2
    R.assert_same_bits(read(tmp_path / "dog"), ref, "float32")
    # the same with a per-element step in between: `$a` would live only in HBM if the planner
    # did not count its use as `other`
    cfg = [{**g1, "output": "$a"},
           {"filter": "rescale", "multiply": 2.0, "add": 0.0, "add_first": True, "output": "$c"},
           {"filter": "arithmetic", "input": "$c", "other": "$a", "operator": "subtract",
            "output": str(tmp_path / "twice")}]
    ZF.run(cfg, tmp=str(tmp_path), **QUIET)
    twice = R.rescale(ga, "float32", 2.0, 0.0, add_first=True)
    R.assert_same_bits(read(tmp_path / "twice"),
                       A.arithmetic(twice, "float32", ga, "float32", "subtract"), "float32")


def test_errors(stored, tmp_path):
    root, v, w = stored
    S.create_array(tmp_path / "small", "uint16", (37, 50, 69), CHUNK)
    with pytest.raises(zt.InvalidParameters,
                       match=r"Array shapes do not match: \[37, 50, 70\] vs \[37, 50, 69\]"):
        S.arithmetic(root / "first", tmp_path / "small", tmp_path / "out", "add")
    assert not (tmp_path / "out").exists()
    with pytest.raises(zt.InvalidParameters, match="unknown operator"):
        S.arithmetic(root / "first", root / "second", tmp_path / "out", "power")
    with pytest.raises(zt.InvalidParameters, match=r"other \$nothing is not the output"):
        ZF.run([{"filter": "arithmetic", "input": str(root / "first"), "other": "$nothing",
                 "operator": "add", "output": str(tmp_path / "out")}], **QUIET)
