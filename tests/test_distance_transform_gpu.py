"""GPU parity of the exact Euclidean distance transform (distance.hip through the C ABI, the store
step, the zarrs_filter command, run configs and device-resident chains) against its numpy
restatement (tests/edt_ref.py): equal storage bytes everywhere. The result is unique and the
kernels have no communication between workgroups, so no run is repeated to look for races.

Borders of the kernels (distance.hip): the innermost-axis pass gives a wave a row, which it walks
in segments of 64 elements; where the rows are 16-byte aligned it loads groups of 16 / size
segments (1024 bytes) by 16-byte vectors and the rest element by element; a row of one segment
needs no backward sweep. Every further axis of extent > 1 is one launch with a lane per line, 256
lanes per workgroup. The write stores 16 bytes per lane where the output is 16-byte aligned. Every
grid is capped at 2^14 workgroups and the kernels loop over the rest.
"""
import json

import numpy as np
import pytest

from oracle import oracle as O
from tests import edt_ref as E
from tests import occ_ref
from tests.ccl_ref import foreground
from tests.gpu_util import from_dev, poisoned, to_dev
from tests.test_connected_components_gpu import typed_figure

pytestmark = pytest.mark.gpu

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)
from zarrs_tools_amd import _abi  # noqa: E402
from zarrs_tools_amd import store as S  # noqa: E402
from zarrs_tools_amd import zarrs_filter as ZF  # noqa: E402

ALL = list(_abi.DTYPES)
QUIET = dict(log=lambda *a: None)


def gpu(a, dtype="uint8", spacing=None, squared=False, dtype_out=None):
    import torch
    dtype_out = dtype_out or ("uint32" if squared else "float32")
    y = poisoned(a.shape, dtype_out)
    out = zt.DistanceTransform(spacing, squared).apply_ndarray(to_dev(a, dtype), dtype_out, out=y)
    torch.cuda.synchronize()
    assert out is y
    return from_dev(y, dtype_out)


def same(out, ref, what):
    assert out.dtype == ref.dtype and out.shape == ref.shape, what
    if out.tobytes() != ref.tobytes():
        bits = f"u{ref.dtype.itemsize}"
        bad = out.view(bits) != ref.view(bits)
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{int(bad.sum())} of {ref.size} elements differ ({what}), first at "
                             f"{i}: got {out[i]!r}, want {ref[i]!r}")


def check(a, dtype="uint8", spacings=(None,), outs=((False, None), (True, None))):
    """Equal bytes for every spacing and every (squared, output type) asked for; the squared
    distance of the restatement is computed once per spacing."""
    a = np.ascontiguousarray(a, dtype=O.NP_STORAGE[dtype])
    for sp in spacings:
        d2 = E.squared_distance(foreground(a, dtype), sp)
        for squared, dtype_out in outs:
            dtype_out = dtype_out or ("uint32" if squared else "float32")
            same(gpu(a, dtype, sp, squared, dtype_out), E.store(d2, dtype_out, squared),
                 (a.shape, dtype, sp, squared, dtype_out))


def noise(shape, density, seed=0):
    """Foreground of about `density`; one element forced to background when it came out all
    foreground: the no-background case is only ever tested on purpose."""
    a = (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)
    if a.all():
        a.reshape(-1)[a.size // 3] = 0
    return a


def aniso(ndim):
    return tuple((3, 1, 2, 5)[k % 4] for k in range(ndim))


# ---- shapes ----------------------------------------------------------------------------------------

SHAPES = ([(3, 5, e) for e in (1, 2, 63, 64, 65, 128, 129, 64 + 16)]
          + [(e, 5, 7) for e in (1, 2, 3, 64, 65)] + [(3, e, 7) for e in (1, 2, 3, 64, 65)]
          + [(9, 9, 129), (37,), (9, 70), (3, 4, 9, 17), (2, 2, 3, 5, 9), (1, 1, 9, 9, 70),
             (3, 300),          # more lines than a workgroup has lanes
             (5, 9),            # fewer lines than a wave has lanes
             (3, 1024 + 80)])   # a group loaded by vectors, a full segment and a tail that are not


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_spacings_and_densities(shape):
    for k, density in enumerate((0.5, 0.9, 0.99, 0.999)):
        check(noise(shape, density, seed=len(shape) * 10 + k), spacings=(None, aniso(len(shape))),
              outs=((False, None),) if k % 2 else ((True, None),))


def test_element_aligned_input_pointer():
    """One element past a 16-byte boundary: rows that may not be loaded by vectors."""
    import torch
    a = noise((3, 1024 + 128), 0.9, 7)
    flat = to_dev(np.concatenate([[1], a.reshape(-1)]).astype(np.uint8), "uint8")
    x = flat[1:].view(a.shape)
    assert x.data_ptr() % 16 == 1 and x.is_contiguous()
    y = poisoned(a.shape, "uint32")
    zt.DistanceTransform(squared=True).apply_ndarray(x, "uint32", out=y)
    torch.cuda.synchronize()
    same(from_dev(y, "uint32"), E.distance_transform(a, "uint8", squared=True), "offset input")
    # ... and an output one element past: the write goes element by element
    flat = poisoned((a.size + 1,), "float32")
    y = flat[1:].view(a.shape)
    assert y.data_ptr() % 16 == 4
    zt.DistanceTransform().apply_ndarray(to_dev(a, "uint8"), "float32", out=y)
    torch.cuda.synchronize()
    same(from_dev(y, "float32"), E.distance_transform(a, "uint8"), "offset output")


def test_the_grid_loops():
    """More rows, more lines and more output groups than the capped grids hold at once, against
    the closed form for a single background element."""
    for shape, at in (((70000, 3), (35000, 1)), ((2, 4200000), (1, 1234567))):
        a = np.ones(shape, np.uint8)
        a[at] = 0
        idx = np.indices(shape).astype(np.int64)
        d2 = (3 * (idx[0] - at[0])) ** 2 + (idx[1] - at[1]) ** 2
        same(gpu(a, "uint8", (3, 1), True, "float64"), E.store(d2, "float64", True), shape)
        same(gpu(a, "uint8", (3, 1), False, "float32"), E.store(d2, "float32"), shape)


# ---- patterns ------------------------------------------------------------------------------------------

BOX, FLAT = (9, 20, 70), (17, 130)


@pytest.mark.parametrize("shape", [BOX, FLAT], ids=["3d", "2d"])
def test_single_background_element(shape):
    """The deepest envelopes: every other site stays a sentinel until the last axis."""
    import itertools
    spots = list(itertools.product(*((0, n - 1) for n in shape))) + [tuple(n // 2 for n in shape)]
    for at in spots:
        a = np.ones(shape, np.uint8)
        a[at] = 0
        check(a, spacings=(None, aniso(len(shape))))


@pytest.mark.parametrize("shape", [BOX, FLAT, (200,)], ids=["3d", "2d", "1d"])
def test_uniform_single_foreground_and_checkerboard(shape):
    check(np.zeros(shape, np.uint8))
    ones = np.ones(shape, np.uint8)
    check(ones, outs=[(sq, dt) for sq in (False, True) for dt in ("float32", "uint32", "int8",
                                                                  "float16", "float64")])
    assert np.isposinf(gpu(ones)).all() and (gpu(ones, squared=True) == 0xFFFFFFFF).all()
    a = np.zeros(shape, np.uint8)
    a[tuple(n // 2 for n in shape)] = 1
    check(a)
    assert gpu(a).sum() == 1.0
    board = (np.indices(shape).sum(axis=0) % 2 == 0).astype(np.uint8)
    check(board, spacings=(None, aniso(len(shape))))


@pytest.mark.parametrize("shape", [BOX, FLAT], ids=["3d", "2d"])
def test_background_planes_ball_and_sentinel_rows(shape):
    sp = (None, aniso(len(shape)))
    for axis in range(len(shape)):
        a = np.ones(shape, np.uint8)
        at = [slice(None)] * len(shape)
        at[axis] = shape[axis] // 3
        a[tuple(at)] = 0
        check(a, spacings=sp)
    # a solid ball: the worst-case stacks
    idx = np.indices(shape)
    r2 = sum((idx[k] - shape[k] // 2) ** 2 for k in range(len(shape)))
    check((r2 <= (min(shape) // 2 - 1) ** 2).astype(np.uint8), spacings=sp)
    check((r2 > (min(shape) // 2 - 1) ** 2).astype(np.uint8), spacings=sp)
    # rows that are entirely foreground next to rows that are not: sentinels enter the axis passes
    a = noise(shape, 0.9, 3)
    a[..., ::2, :] = 1
    check(a, spacings=sp)
    a = np.ones(shape, np.uint8)
    a[0, ..., 5] = 0  # every row but those of the first index is all foreground
    check(a, spacings=sp)


# ---- element types ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ALL)
def test_every_input_type_with_its_special_values(dtype):
    per = 16 // np.dtype(O.NP_STORAGE[dtype]).itemsize
    x = 64 * per + 64 + per  # one group by vectors, a full segment and a tail element by element
    a = typed_figure(dtype, (2, 3, x))
    check(a, dtype, outs=((True, None),))
    check(a[..., :x - 1], dtype, outs=((False, None),))  # rows not 16-byte aligned
    # sparse background: long distances over the same special values
    a = a.copy()
    a[foreground(a, dtype) == 0] = a[foreground(a, dtype)][0]
    a[1, 1, 64 * per + 3] = 0
    a[0, 2, 5] = 0
    check(a, dtype, spacings=((2, 3, 1),))


OUT_SHAPE = (2, 6, 23, 257)  # as tests/test_distance_transform.py: k^2, k^2 +- 1, the type borders
_out_refs = {}


def out_ref(sp):
    if sp not in _out_refs:
        a = np.ones(OUT_SHAPE, np.uint8)
        a[0, 0, 0, 0] = 0
        d2 = E.squared_distance(a != 0, sp)
        for v in ((0, 1, 2, 3, 8, 24, 255, 256, 257, 65535, 65536, 65537) if sp is None else ()):
            assert (d2 == v).any(), v
        _out_refs[sp] = (a, d2)
    return _out_refs[sp]


@pytest.mark.parametrize("dtype_out", E.OUT_TYPES)
def test_every_output_type(dtype_out):
    for sp in (None, (1, 1, 1, 17)):  # the second takes d2 past 2^24
        a, d2 = out_ref(sp)
        for squared in (False, True):
            same(gpu(a, "uint8", sp, squared, dtype_out), E.store(d2, dtype_out, squared),
                 (sp, squared, dtype_out))


@pytest.mark.parametrize("dtype_out", ["float64", "uint64", "float32", "int64"])
def test_squared_distances_past_2_53(dtype_out):
    s = (1 << 27) + 1
    a = np.array([0, 1, 1, 1, 1], np.uint8)
    check(a, spacings=((s,),), outs=((True, dtype_out), (False, dtype_out)))
    check(noise((3, 70), 0.95, 5), spacings=((s, 3),), outs=((True, dtype_out), (False, dtype_out)))
    # along the rows: (2^27 + 1)^2 * 8^2 is about 2^60, below the bound of 2^62
    check(noise((3, 9), 0.8, 6), spacings=((3, s),), outs=((True, dtype_out), (False, dtype_out)))


def test_bool_output_is_refused():
    with pytest.raises(zt.UnsupportedDataType, match="numeric output type, not bool"):
        zt.DistanceTransform().apply_ndarray(to_dev(noise((5, 9), 0.5), "uint8"), "bool")


# ---- work width ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(9, 9, 129), (9, 70), (3, 4, 9, 17)], ids=["3d", "2d", "4d"])
def test_the_64_bit_work_type_gives_the_same_bytes(shape, monkeypatch):
    monkeypatch.setenv("ZT_EDT_WORK64", "1")  # read at every call
    n = int(np.prod(shape))
    assert zt.DistanceTransform().memory("uint8", "float32", shape) == n * (1 + 4 + 24)
    check(noise(shape, 0.9, 5), spacings=(None, aniso(len(shape))))
    check(noise(shape, 0.999, 6))
    check(np.ones(shape, np.uint8))


def test_a_spacing_that_needs_64_bits():
    shape, sp = (3, 5, 7), (70000, 1, 1)
    assert E.work_bytes(shape, sp) == 8
    assert zt.DistanceTransform(sp).memory("uint8", "float32", shape) == 105 * (1 + 4 + 24)
    for k, density in enumerate((0.5, 0.9, 0.99)):
        check(noise(shape, density, k), spacings=(sp,),
              outs=((False, None), (True, None), (True, "uint64"), (True, "float64")))
    a = np.ones(shape, np.uint8)
    a[2, 4, 6] = 0
    out = gpu(a, "uint8", sp, True, "uint64")
    assert int(out[0, 0, 0]) == 4 * 70000 ** 2 + 16 + 36
    assert (gpu(a, "uint8", sp, True)[0] == 0xFFFFFFFF).all()  # saturated, never wrapped


# ---- errors --------------------------------------------------------------------------------------------------

def test_zero_extents_shapes_and_layout():
    import torch
    for shape in ((0,), (3, 0, 5), (0, 4)):
        assert gpu(np.zeros(shape, np.uint8)).shape == shape
    a = noise((5, 9, 70), 0.9, 3)
    f = zt.DistanceTransform()
    out = f.apply_ndarray(to_dev(a, "uint8"))
    torch.cuda.synchronize()
    assert zt.dtype_of(out) == "float32"  # whatever the input type
    same(from_dev(out, "float32"), E.distance_transform(a, "uint8"), "default type")
    out = zt.DistanceTransform(squared=True).apply_ndarray(to_dev(a, "uint8"))
    torch.cuda.synchronize()
    assert zt.dtype_of(out) == "uint32"
    y = poisoned(a.shape, "float64")
    assert f.apply(zt.DeviceArray(to_dev(a, "uint8"), (4, 4, 4)),
                   zt.DeviceArray(y, (4, 4, 4))) is None
    torch.cuda.synchronize()
    same(from_dev(y, "float64"), E.distance_transform(a, "uint8", dtype_out="float64"), "apply")
    with pytest.raises(zt.InvalidParameters, match="Array shapes do not match"):
        f.apply_ndarray(to_dev(a, "uint8"), out=poisoned((5, 9, 69), "float32"))
    with pytest.raises(zt.InvalidParameters, match="must be contiguous"):
        f.apply_ndarray(to_dev(a, "uint8"), out=poisoned((5, 9, 140), "float32")[..., ::2])
    with pytest.raises(zt.InvalidParameters, match="3 entries for an array of rank 2"):
        zt.DistanceTransform((1, 2, 3)).apply_ndarray(to_dev(a[0], "uint8"))
    # the C ABI's own checks: overlapping arrays, a spacing below 1; and a NULL spacing
    x, y = to_dev(a, "uint8"), poisoned(a.shape, "uint8")
    ctx = zt.default_context(0)
    u8 = _abi.DTYPES["uint8"]
    call = _abi.lib().zt_distance_transform_apply_array
    shape = _abi.i64_array(a.shape)
    with pytest.raises(zt.InvalidParameters, match="must not overlap"):
        _abi.check(call(ctx.handle, u8, x.data_ptr(), u8, x.data_ptr() + 16, shape, None, 3, 0))
    with pytest.raises(zt.InvalidParameters, match="integer >= 1"):
        _abi.check(call(ctx.handle, u8, x.data_ptr(), u8, y.data_ptr(), shape,
                        _abi.i64_array((1, 0, 1)), 3, 0))
    _abi.check(call(ctx.handle, u8, x.data_ptr(), u8, y.data_ptr(), shape, None, 3, 1))
    torch.cuda.synchronize()
    same(from_dev(y, "uint8"), E.distance_transform(a, "uint8", None, True, "uint8"), "C ABI")


# ---- store path ---------------------------------------------------------------------------------------------

SHAPE, CHUNK = (70, 45, 67), (32, 32, 32)


@pytest.fixture(scope="module")
def stored(tmp_path_factory):
    """uint8 with ragged chunks: values 0, 1 and 2, mostly foreground; the chunks of z >= 32,
    x >= 32 missing (they read as the fill value 0: background). Returns (path, the array as it
    reads, its squared distances at spacing ones and (3, 1, 2))."""
    root = tmp_path_factory.mktemp("edt")
    rng = np.random.default_rng(42)
    v = rng.integers(1, 3, SHAPE).astype(np.uint8)
    v[rng.random(SHAPE) < 0.002] = 0
    v[:20, :20, :20] = 0  # a block of background inside the first chunk
    S.create_array(root / "in", "uint8", SHAPE, CHUNK, fill_value=0)
    S.write_array(root / "in", v[:32])
    S.write_array(root / "in", v[32:, :, :32], start=(32, 0, 0))
    v[32:, :, 32:] = 0
    assert np.array_equal(S.read_array(root / "in"), v)
    d2 = {sp: E.squared_distance(v != 0, sp) for sp in (None, (3, 1, 2))}
    return str(root / "in"), v, d2


def test_store_function_subcommand_and_run_config(stored, tmp_path):
    src, v, d2 = stored
    st = S.distance_transform(src, tmp_path / "a")
    assert st["voxels"] == v.size and st["kernel_s"] > 0 and "components" not in st
    a = S.open_array(tmp_path / "a")
    assert a.data_type == "float32" and a.shape == SHAPE and a.chunk_shape == CHUNK
    assert a.metadata["fill_value"] == 0
    assert S.read_array(tmp_path / "a").tobytes() == E.store(d2[None], "float32").tobytes()
    # the subcommand, into a sharded and gzip compressed uint16 output, anisotropic and squared
    assert S.codec_available("gzip")
    argv = ["distance-transform", src, str(tmp_path / "b"), "--spacing", "3,1,2", "--squared",
            "--data-type", "uint16", "-s", "32,32,64", "-c", "16,16,32",
            "--bytes-to-bytes-codecs", json.dumps([{"name": "gzip", "configuration": {"level": 1}}])]
    assert ZF.main(argv) == 0
    b = S.open_array(tmp_path / "b")
    assert b.data_type == "uint16" and b.chunk_shape == (32, 32, 64)
    assert b.inner_chunk_shape == (16, 16, 32)
    assert S.read_array(tmp_path / "b").tobytes() == E.store(d2[(3, 1, 2)], "uint16", True).tobytes()
    # the default type of the squared form
    assert ZF.main(["distance-transform", src, str(tmp_path / "sq"), "--squared"]) == 0
    assert S.open_array(tmp_path / "sq").data_type == "uint32"
    assert S.read_array(tmp_path / "sq").tobytes() == E.store(d2[None], "uint32", True).tobytes()
    # a run config
    lines = []
    cfg = [{"filter": "distance_transform", "input": src, "output": str(tmp_path / "c"),
            "spacing": [3, 1, 2], "data_type": "float64"}]
    (tmp_path / "run.json").write_text(json.dumps(cfg))
    assert ZF.main([str(tmp_path / "run.json"), "--tmp", str(tmp_path)]) == 0
    assert S.read_array(tmp_path / "c").tobytes() == E.store(d2[(3, 1, 2)], "float64").tobytes()
    res = ZF.run(cfg, log=lines.append)
    assert "components" not in res[0] and not any("components" in line for line in lines)
    assert any("distance_transform spacing=[3, 1, 2]" in line for line in lines)


def test_skip_empty_chunks(stored, tmp_path):
    src, v, d2 = stored
    ref = E.store(d2[None], "float32")
    assert ZF.main(["distance-transform", src, str(tmp_path / "e"), "--skip-empty-chunks"]) == 0
    want = occ_ref.expected_files(ref, CHUNK, 0)
    assert want < occ_ref.all_files(SHAPE, CHUNK)  # a chunk of background is never stored
    assert occ_ref.chunk_files(tmp_path / "e") == want
    assert S.read_array(tmp_path / "e").tobytes() == ref.tobytes()
    assert ZF.main(["distance-transform", src, str(tmp_path / "f")]) == 0
    assert occ_ref.chunk_files(tmp_path / "f") == occ_ref.all_files(SHAPE, CHUNK)


def test_equal_distance_clamp_as_a_device_chain(stored, tmp_path):
    """Erosion by a ball: the mask of the elements equal to 2, its distance transform, clamped."""
    src, v, d2 = stored
    steps = [{"filter": "equal", "input": src, "value": 2, "output": "$mask"},
             {"filter": "distance_transform", "input": "$mask", "spacing": [3, 1, 2]},
             {"filter": "clamp", "min": 0, "max": 2.5, "output": str(tmp_path / "chain")}]
    assert ZF.plan_chains(steps) == [(0, 2)]
    lines = []
    res = ZF.run(steps, tmp=str(tmp_path), log=lines.append)
    assert all(st.get("device_resident") for st in res)
    assert not any("components" in st for st in res)
    assert not any("components" in line for line in lines)
    steps[2]["output"] = str(tmp_path / "store")
    res2 = ZF.run(steps, tmp=str(tmp_path), device_chain=False, **QUIET)
    assert not res2[0].get("device_resident")
    from tests import pw_ref
    dist = E.distance_transform((v == 2).astype(np.uint8), "bool", (3, 1, 2))
    ref = pw_ref.clamp(dist, "float32", 0, 2.5)
    assert ref.max() == 2.5 and ref.tobytes() == np.minimum(dist, np.float32(2.5)).tobytes()
    chain = S.read_array(tmp_path / "chain")
    assert chain.dtype == np.float32 and chain.tobytes() == ref.tobytes()
    assert S.read_array(tmp_path / "store").tobytes() == ref.tobytes()


def test_two_gpus_run_the_step_in_one_process(stored, tmp_path):
    src, v, d2 = stored
    lines = []
    steps = [{"filter": "distance_transform", "input": src, "output": str(tmp_path / "two")}]
    res = ZF.run(steps, gpus=2, gpu_devices=[0, 0], log=lines.append)
    assert "processes" not in res[0]
    assert any("distance_transform" in line and "one process on device 0, not 2" in line
               for line in lines)
    assert S.read_array(tmp_path / "two").tobytes() == E.store(d2[None], "float32").tobytes()


def test_an_array_that_does_not_fit_fails_before_anything_is_read(stored, tmp_path, monkeypatch):
    from zarrs_tools_amd import device_io
    src, v, d2 = stored
    need = zt.DistanceTransform().memory("uint8", "float32", SHAPE)
    assert need == v.size * (1 + 4 + 16)

    def no_read(*a, **k):
        raise AssertionError("the input was read")

    monkeypatch.setattr(device_io, "read_to_device", no_read)
    monkeypatch.setenv("ZT_STORE_DEVICE_MEMORY", str(need))  # 80 % of it is too little
    with pytest.raises(zt.FilterError, match="not enough available memory") as e:
        S.distance_transform(src, tmp_path / "out")
    assert e.value.status == _abi.ERR_OUT_OF_MEMORY and "no store -> store path" in str(e.value)
    assert not (tmp_path / "out" / "zarr.json").exists()
    assert occ_ref.chunk_files(tmp_path / "out") == set()
    assert ZF.main(["distance-transform", src, str(tmp_path / "out")]) == 1
    assert not (tmp_path / "out" / "zarr.json").exists()
    # the pinned host buffers are budgeted too
    monkeypatch.delenv("ZT_STORE_DEVICE_MEMORY")
    monkeypatch.setenv("ZT_STORE_HOST_MEMORY", "100000")
    with pytest.raises(zt.FilterError, match="pinned host buffers") as e:
        S.distance_transform(src, tmp_path / "out")
    assert e.value.status == _abi.ERR_OUT_OF_MEMORY
    assert not (tmp_path / "out" / "zarr.json").exists()
    assert occ_ref.chunk_files(tmp_path / "out") == set()
