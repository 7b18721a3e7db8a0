"""GPU parity of the connected-component labelling (connected.hip through the C ABI, the store
step, the zarrs_filter command, run configs and device-resident chains) against its numpy
restatement (tests/ccl_ref.py): equal storage bytes and equal K everywhere. The result is unique
(components numbered by their first elements), so no run is repeated to look for races.

Borders of the kernels (connected.hip): a workgroup of the local phase owns a tile of
T = _abi.CC_TILE = (8, 8, 64) elements of the three innermost axes and loads full 64-element rows
16 bytes per lane when the rows are 16-byte aligned, element by element otherwise; the merge phase
visits tile faces for rank <= 3 and every element when an axis in front of the innermost three has
an extent above 1; the numbering works on blocks of 4096 elements.
"""
import json

import numpy as np
import pytest

from oracle import oracle as O
from tests import ccl_ref as C
from tests import occ_ref
from tests.gpu_util import from_dev, poisoned, to_dev

pytestmark = pytest.mark.gpu

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)
from zarrs_tools_amd import _abi  # noqa: E402
from zarrs_tools_amd import store as S  # noqa: E402
from zarrs_tools_amd import zarrs_filter as ZF  # noqa: E402

ALL = list(_abi.DTYPES)
TZ, TY, TX = _abi.CC_TILE
BIG = (TZ + 1, TY + 1, 2 * TX + 1)  # more than one tile on every axis, a one-element last tile
FLAT = (2 * TY + 1, 2 * TX + 1)
QUIET = dict(log=lambda *a: None)


def gpu(a, dtype="uint8", connectivity=1, dtype_out="uint32"):
    import torch
    y = poisoned(a.shape, dtype_out)
    out, k = zt.ConnectedComponents(connectivity).apply_ndarray(to_dev(a, dtype), dtype_out, out=y)
    torch.cuda.synchronize()
    assert out is y
    return from_dev(y, dtype_out), k


def check(a, dtype="uint8", connectivities=None, dtype_out="uint32"):
    """Equal bytes and equal K at every connectivity of the rank (or the ones given)."""
    a = np.ascontiguousarray(a, dtype=O.NP_STORAGE[dtype])
    counts = []
    for c in connectivities or range(1, a.ndim + 1):
        ref, k_ref = C.connected_components(a, dtype, c, dtype_out)
        out, k = gpu(a, dtype, c, dtype_out)
        assert k == k_ref, (a.shape, dtype, c, k, k_ref)
        assert out.dtype == ref.dtype and out.shape == ref.shape
        if out.tobytes() != ref.tobytes():
            i = tuple(int(v) for v in np.argwhere(out != ref)[0])
            raise AssertionError(f"{int((out != ref).sum())} of {ref.size} labels differ at "
                                 f"connectivity {c}, first at {i}: got {out[i]}, want {ref[i]}")
        counts.append(k)
    return counts


def noise(shape, density, seed=0):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


# ---- shapes ----------------------------------------------------------------------------------------

SHAPES = ([(e, 5, 7) for e in (1, TZ, TZ + 1, 2 * TZ + 1)]
          + [(3, e, 7) for e in (1, TY, TY + 1, 2 * TY + 1)]
          + [(3, 5, e) for e in (1, TX, TX + 1, 2 * TX + 1)]
          + [BIG, (3, 5, TX + 16),  # 16-byte rows: a full tile loads by vectors, the last does not
             (37,), (9, 70), FLAT, (3, 4, 9, 17), (2, 2, 3, 5, 9), (1, 1, 9, 9, 70)])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_connectivities_and_densities(shape):
    for k, density in enumerate((0.05, 0.3, 0.6, 0.95)):
        check(noise(shape, density, seed=len(shape) * 10 + k))


def test_zero_extent_is_a_no_op():
    for shape in ((0,), (3, 0, 5), (0, 4)):
        out, k = gpu(np.zeros(shape, np.uint8), "uint8", 1)
        assert k == 0 and out.shape == shape


def test_device_arrays_default_type_and_errors():
    import torch
    a = noise((5, 9, 70), 0.4, 3)
    f = zt.ConnectedComponents(2)
    out, k = f.apply_ndarray(to_dev(a, "uint8"))
    torch.cuda.synchronize()
    assert zt.dtype_of(out) == "uint32"  # whatever the input type
    ref, k_ref = C.connected_components(a, "uint8", 2)
    assert k == k_ref and from_dev(out, "uint32").tobytes() == ref.tobytes()
    y = poisoned(a.shape, "int64")
    k = f.apply(zt.DeviceArray(to_dev(a, "uint8"), (4, 4, 4)), zt.DeviceArray(y, (4, 4, 4)))
    torch.cuda.synchronize()
    assert k == k_ref
    assert from_dev(y, "int64").tobytes() == ref.astype(np.int64).tobytes()
    with pytest.raises(zt.InvalidParameters, match=r"connectivity 4 not in \[1, 3\]"):
        zt.ConnectedComponents(4).apply_ndarray(to_dev(a, "uint8"))
    with pytest.raises(zt.UnsupportedDataType, match="integer output type"):
        f.apply_ndarray(to_dev(a, "uint8"), "float32")
    with pytest.raises(zt.InvalidParameters, match="Array shapes do not match"):
        f.apply_ndarray(to_dev(a, "uint8"), out=poisoned((5, 9, 69), "uint32"))
    # the C ABI's own check of the connectivity, and a NULL count
    x, y = to_dev(a, "uint8"), poisoned(a.shape, "uint32")
    ctx = zt.default_context(0)
    args = (ctx.handle, _abi.DTYPES["uint8"], x.data_ptr(), _abi.DTYPES["uint32"], y.data_ptr(),
            _abi.i64_array(a.shape), 3)
    for c in (0, 4):
        with pytest.raises(zt.InvalidParameters, match=rf"connectivity {c} not in \[1, 3\]"):
            _abi.check(_abi.lib().zt_connected_components_apply_array(*args, c, None))
    _abi.check(_abi.lib().zt_connected_components_apply_array(*args, 2, None))
    torch.cuda.synchronize()
    assert from_dev(y, "uint32").tobytes() == ref.tobytes()


def test_element_aligned_input_pointer():
    """One element past a 16-byte boundary: 64-element rows that may not be loaded by vectors."""
    import torch
    a = noise((3, 9, 2 * TX), 0.5, 7)
    flat = to_dev(np.concatenate([[1], a.reshape(-1)]).astype(np.uint8), "uint8")
    x = flat[1:].view(a.shape)
    assert x.data_ptr() % 16 == 1 and x.is_contiguous()
    y = poisoned(a.shape, "uint32")
    _, k = zt.ConnectedComponents(3).apply_ndarray(x, "uint32", out=y)
    torch.cuda.synchronize()
    ref, k_ref = C.connected_components(a, "uint8", 3)
    assert k == k_ref and from_dev(y, "uint32").tobytes() == ref.tobytes()


# ---- adversarial figures -----------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [BIG, FLAT], ids=["3d", "2d"])
def test_uniform_and_checkerboard(shape):
    rank, n = len(shape), int(np.prod(shape))
    assert check(np.zeros(shape, np.uint8)) == [0] * rank
    assert check(np.ones(shape, np.uint8)) == [1] * rank
    board = (np.indices(shape).sum(axis=0) % 2 == 0).astype(np.uint8)
    counts = check(board)
    assert counts[0] == (n + 1) // 2 and counts[-1] == 1  # every element alone; all joined


@pytest.mark.parametrize("shape", [BIG, FLAT], ids=["3d", "2d"])
def test_serpentine_and_spiral(shape):
    """One component that crosses tile borders many times: the longest union chains."""
    for figure in (C.serpentine(shape), C.spiral(shape)):
        assert check(figure.astype(np.uint8)) == [1] * len(shape)
    # mirrored: the chains run against the direction the indices grow in
    assert check(C.spiral(shape)[..., ::-1, ::-1].astype(np.uint8)) == [1] * len(shape)


@pytest.mark.parametrize("shape", [BIG, FLAT], ids=["3d", "2d"])
def test_single_lines_along_each_axis(shape):
    for axis in range(len(shape)):
        a = np.zeros(shape, np.uint8)
        at = [s // 2 for s in shape]
        at[axis] = slice(None)
        a[tuple(at)] = 1
        assert check(a) == [1] * len(shape)
    # one line per axis in one array, apart from each other
    a = np.zeros(shape, np.uint8)
    for axis in range(len(shape)):
        at = [2 * axis] * len(shape)
        at[axis] = slice(4, None)
        a[tuple(at)] = 1
    check(a)


def test_blobs_that_meet_across_a_tile_corner():
    # 3-D: the corner of tiles (0,0,0) and (1,1,1) at (TZ, TY, TX); the elements (TZ-1, TY-1,
    # TX-1) and (TZ, TY, TX) differ on three axes: one component at connectivity 3 only
    a = np.zeros(BIG, np.uint8)
    a[TZ - 3:TZ, TY - 3:TY, TX - 3:TX] = 1
    a[TZ:, TY:, TX:TX + 3] = 1
    assert check(a) == [2, 2, 1]
    # the other diagonals: +1 on some axes behind a -1 (the high faces of the merge phase)
    a = np.zeros(BIG, np.uint8)
    a[TZ - 3:TZ, TY:, TX - 3:TX] = 1
    a[TZ:, TY - 3:TY, TX:TX + 3] = 1
    assert check(a) == [2, 2, 1]
    a = np.zeros(BIG, np.uint8)
    a[TZ - 3:TZ, TY - 3:TY, TX:TX + 3] = 1
    a[TZ:, TY:, TX - 3:TX] = 1
    assert check(a) == [2, 2, 1]
    # across an edge only: two axes differ
    a = np.zeros(BIG, np.uint8)
    a[2, TY - 3:TY, TX:TX + 3] = 1
    a[2, TY:, TX - 3:TX] = 1
    assert check(a) == [2, 1, 1]
    # 2-D
    a = np.zeros(FLAT, np.uint8)
    a[TY - 3:TY, TX - 3:TX] = 1
    a[TY:TY + 3, TX:TX + 3] = 1
    a[2 * TY:, 2 * TX - 3:2 * TX] = 1  # ... and the anti-diagonal at the next corner
    a[2 * TY - 3:2 * TY, 2 * TX:] = 1
    assert check(a) == [4, 2]


def test_first_element_in_the_last_tile():
    """The last tile of BIG is the single element at its far corner: a component that starts
    there is numbered last, whatever order the tiles ran in."""
    a = np.zeros(BIG, np.uint8)
    a[0:3, 0:3, 0:3] = 1
    a[-1, -1, -1] = 1
    for c in (1, 2, 3):
        out, k = gpu(a, "uint8", c)
        assert k == 2 and out[-1, -1, -1] == 2 and out[0, 0, 0] == 1
    check(a)
    # a component whose first element lies in the last full tile and that leaves it for a tile
    # of higher indices but lower number
    a = np.zeros((2 * TZ, 2 * TY, 2 * TX), np.uint8)
    a[1, 1, 1] = 1
    a[TZ + 2, TY + 3, TX + 5:] = 1
    a[TZ + 2:, TY + 3, TX + 5] = 1
    a[-1, :TY + 3, TX + 5] = 1
    assert check(a) == [2, 2, 2]


# ---- element types ---------------------------------------------------------------------------------------

SPECIAL = {  # storage bits of (foreground values, background values)
    "bool": ([1], [0]),
    "int8": ([0x01, 0xFF, 0x80, 0x7F], [0]), "uint8": ([0x01, 0xFF, 0x80], [0]),
    "int16": ([1, 0xFFFF, 0x8000, 0x0100], [0]), "uint16": ([1, 0xFFFF, 0x8000, 0x0100], [0]),
    "int32": ([1, 0xFFFFFFFF, 0x80000000, 0x00010000], [0]),
    "uint32": ([1, 0xFFFFFFFF, 0x80000000, 0x00010000], [0]),
    "int64": ([1, 1 << 32, 1 << 63, (1 << 64) - 1, 1 << 62], [0]),
    "uint64": ([1, 1 << 32, 1 << 63, (1 << 64) - 1, 1 << 31], [0]),
    # subnormals, infinities, NaNs of both signs, 1.0; +0.0 and -0.0 (0x8000 for the 16-bit ones)
    "float16": ([0x0001, 0x8001, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x3C00], [0x0000, 0x8000]),
    "bfloat16": ([0x0001, 0x8001, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x3F80], [0x0000, 0x8000]),
    "float32": ([0x00000001, 0x80000001, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000,
                 0x3F800000], [0x00000000, 0x80000000]),
    "float64": ([1, (1 << 63) | 1, 0x7FF0 << 48, 0xFFF0 << 48, 0x7FF8 << 48, 0xFFF8 << 48,
                 0x3FF0 << 48, 1 << 32], [0, 1 << 63]),
}


def typed_figure(dtype, shape, seed=11):
    """A noise mask whose foreground cycles through the type's special non-zero values and whose
    background cycles through its zeros."""
    st = np.dtype(O.NP_STORAGE[dtype])
    mask = np.random.default_rng(seed).random(shape) < 0.45
    fg_bits, bg_bits = (np.array(v, dtype=np.uint64) for v in SPECIAL[dtype])
    idx = np.arange(mask.size).reshape(shape)
    bits = np.where(mask, fg_bits[idx % len(fg_bits)], bg_bits[idx % len(bg_bits)])
    a = bits.astype(f"u{st.itemsize}").view(st).reshape(shape)
    assert np.array_equal(C.foreground(a, dtype), mask)
    return a


@pytest.mark.parametrize("dtype", ALL)
def test_every_input_type_with_its_special_values(dtype):
    a = typed_figure(dtype, (5, 9, 2 * TX))  # 16-byte rows of full tiles: loaded by vectors
    check(a, dtype, (1, 3))
    check(a[..., :2 * TX - 1], dtype, (2,))  # ... and element by element


@pytest.mark.parametrize("dtype_out", C.INT_OUT)
def test_every_output_type(dtype_out):
    a = np.zeros(BIG, np.uint8)
    a[::4, ::4, ::16] = 1  # 81 isolated elements in every tile
    a[1, :, 3] = 1
    assert check(a, "uint8", (1, 3), dtype_out)[0] == 3 * 3 * 9 + 1


@pytest.mark.parametrize("dtype_out,most", [("uint8", 255), ("int8", 127)])
def test_labels_never_wrap(dtype_out, most):
    import torch
    dots = np.zeros(2 * most + 2, np.uint8)
    dots[:2 * most:2] = 1
    out, k = gpu(dots, "uint8", 1, dtype_out)
    assert k == most and int(out.astype(np.int64).max()) == most
    assert out.tobytes() == C.connected_components(dots, "uint8", 1, dtype_out)[0].tobytes()
    dots[2 * most] = 1  # one more
    y = poisoned(dots.shape, dtype_out)
    before = from_dev(y, dtype_out).tobytes()
    with pytest.raises(zt.InvalidParameters,
                       match=f"connected_components: {most + 1} components do not fit {dtype_out}"):
        zt.ConnectedComponents().apply_ndarray(to_dev(dots, "uint8"), dtype_out, out=y)
    torch.cuda.synchronize()
    assert from_dev(y, dtype_out).tobytes() == before  # nothing was written


# ---- index width --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [BIG, (9, 70), (3, 4, 9, 17)], ids=["3d", "2d", "4d"])
def test_the_64_bit_index_gives_the_same_bytes(shape, monkeypatch):
    monkeypatch.setenv("ZT_CC_INDEX64", "1")  # read at every call
    f = zt.ConnectedComponents()
    assert f.memory("uint8", "uint32", shape) == int(np.prod(shape)) * (1 + 4 + 16) + \
        _abi.cc_tail_bytes(len(shape))
    check(noise(shape, 0.45, 5))
    check(C.spiral(shape).astype(np.uint8))


# ---- store path ---------------------------------------------------------------------------------------------

SHAPE, CHUNK = (70, 45, 67), (32, 32, 32)


@pytest.fixture(scope="module")
def stored(tmp_path_factory):
    """uint8 with ragged chunks: values 0, 1 and 2 in blobs, the chunks of z >= 32, x >= 32
    missing (they read as the fill value 0). Returns (path, the array as it reads, labels and K of
    its non-zero elements at connectivity 1 and 3)."""
    root = tmp_path_factory.mktemp("cc")
    rng = np.random.default_rng(42)
    v = np.zeros(SHAPE, np.uint8)
    for _ in range(60):  # boxes of ones and twos, some overlapping, some alone
        z, y, x = (int(rng.integers(0, s - 2)) for s in SHAPE)
        dz, dy, dx = (int(rng.integers(1, 9)) for _ in range(3))
        v[z:z + dz, y:y + dy, x:x + dx] = rng.integers(1, 3)
    v[::9, ::7, ::5] |= 1  # and isolated elements: more than 255 components
    S.create_array(root / "in", "uint8", SHAPE, CHUNK, fill_value=0)
    S.write_array(root / "in", v[:32])
    S.write_array(root / "in", v[32:, :, :32], start=(32, 0, 0))
    v[32:, :, 32:] = 0
    assert np.array_equal(S.read_array(root / "in"), v)
    refs = {c: C.connected_components(v, "uint8", c) for c in (1, 3)}
    assert 255 < refs[1][1] < 65535
    return str(root / "in"), v, refs


def test_store_function_subcommand_and_run_config(stored, tmp_path):
    src, v, refs = stored
    ref, k_ref = refs[1]
    st = S.connected_components(src, tmp_path / "a")
    assert st["components"] == k_ref and st["voxels"] == v.size and st["kernel_s"] > 0
    a = S.open_array(tmp_path / "a")
    assert a.data_type == "uint32" and a.shape == SHAPE and a.chunk_shape == CHUNK
    assert a.metadata["fill_value"] == 0
    assert S.read_array(tmp_path / "a").tobytes() == ref.tobytes()
    # the subcommand, into a sharded and gzip compressed uint16 output, the full neighbourhood
    ref3, k3 = refs[3]
    assert S.codec_available("gzip")
    argv = ["connected-components", src, str(tmp_path / "b"), "--connectivity", "3",
            "--data-type", "uint16", "-s", "32,32,64", "-c", "16,16,32",
            "--bytes-to-bytes-codecs", json.dumps([{"name": "gzip", "configuration": {"level": 1}}])]
    assert ZF.main(argv) == 0
    b = S.open_array(tmp_path / "b")
    assert b.data_type == "uint16" and b.chunk_shape == (32, 32, 64)
    assert b.inner_chunk_shape == (16, 16, 32)
    assert S.read_array(tmp_path / "b").tobytes() == ref3.astype(np.uint16).tobytes()
    # a run config; the step logs K
    lines = []
    cfg = [{"filter": "connected_components", "input": src, "output": str(tmp_path / "c"),
            "connectivity": 3, "data_type": "int32"}]
    (tmp_path / "run.json").write_text(json.dumps(cfg))
    assert ZF.main([str(tmp_path / "run.json"), "--tmp", str(tmp_path)]) == 0
    assert S.read_array(tmp_path / "c").tobytes() == ref3.astype(np.int32).tobytes()
    res = ZF.run(cfg, log=lines.append)
    assert res[0]["components"] == k3 and f"   {k3} components" in lines


def test_skip_empty_chunks(stored, tmp_path):
    src, v, refs = stored
    ref, _ = refs[1]
    assert ZF.main(["connected-components", src, str(tmp_path / "e"), "--skip-empty-chunks"]) == 0
    want = occ_ref.expected_files(ref, CHUNK, 0)
    assert want < occ_ref.all_files(SHAPE, CHUNK)  # the missing chunks are background only
    assert occ_ref.chunk_files(tmp_path / "e") == want
    assert S.read_array(tmp_path / "e").tobytes() == ref.tobytes()
    assert ZF.main(["connected-components", src, str(tmp_path / "f")]) == 0
    assert occ_ref.chunk_files(tmp_path / "f") == occ_ref.all_files(SHAPE, CHUNK)


def test_equal_then_labelling_as_a_device_chain(stored, tmp_path):
    src, v, refs = stored
    steps = [{"filter": "equal", "input": src, "value": 2, "output": "$mask"},
             {"filter": "connected_components", "input": "$mask", "connectivity": 2,
              "output": str(tmp_path / "chain")}]
    assert ZF.plan_chains(steps) == [(0, 1)]
    lines = []
    res = ZF.run(steps, tmp=str(tmp_path), log=lines.append)
    assert all(st.get("device_resident") for st in res)
    steps[1]["output"] = str(tmp_path / "store")
    res2 = ZF.run(steps, tmp=str(tmp_path), device_chain=False, **QUIET)
    assert not res2[0].get("device_resident")
    ref, k_ref = C.connected_components((v == 2).astype(np.uint8), "bool", 2)
    assert res[1]["components"] == res2[1]["components"] == k_ref
    assert f"   {k_ref} components" in lines
    chain = S.read_array(tmp_path / "chain")
    assert chain.dtype == np.uint32 and chain.tobytes() == ref.tobytes()
    assert S.read_array(tmp_path / "store").tobytes() == ref.tobytes()


def test_two_gpus_run_the_step_in_one_process(stored, tmp_path):
    src, v, refs = stored
    lines = []
    steps = [{"filter": "connected_components", "input": src, "output": str(tmp_path / "two")}]
    res = ZF.run(steps, gpus=2, gpu_devices=[0, 0], log=lines.append)
    assert "processes" not in res[0] and res[0]["components"] == refs[1][1]
    assert any("connected_components" in line and "one process on device 0, not 2" in line
               for line in lines)
    assert S.read_array(tmp_path / "two").tobytes() == refs[1][0].tobytes()


def test_an_array_that_does_not_fit_fails_before_anything_is_read(stored, tmp_path, monkeypatch):
    from zarrs_tools_amd import device_io
    src, v, refs = stored
    need = zt.ConnectedComponents().memory("uint8", "uint32", SHAPE)

    def no_read(*a, **k):
        raise AssertionError("the input was read")

    monkeypatch.setattr(device_io, "read_to_device", no_read)
    monkeypatch.setenv("ZT_STORE_DEVICE_MEMORY", str(need))  # 80 % of it is too little
    with pytest.raises(zt.FilterError, match="not enough available memory") as e:
        S.connected_components(src, tmp_path / "out")
    assert e.value.status == _abi.ERR_OUT_OF_MEMORY and "no store -> store path" in str(e.value)
    assert not (tmp_path / "out" / "zarr.json").exists()
    assert ZF.main(["connected-components", src, str(tmp_path / "out")]) == 1
    assert not (tmp_path / "out" / "zarr.json").exists()
    # the pinned host buffers are budgeted too
    monkeypatch.delenv("ZT_STORE_DEVICE_MEMORY")
    monkeypatch.setenv("ZT_STORE_HOST_MEMORY", "100000")
    with pytest.raises(zt.FilterError, match="pinned host buffers") as e:
        S.connected_components(src, tmp_path / "out")
    assert e.value.status == _abi.ERR_OUT_OF_MEMORY
    assert not (tmp_path / "out" / "zarr.json").exists()


def test_too_many_components_for_the_output_type_write_nothing(stored, tmp_path):
    src, v, refs = stored
    k = refs[1][1]
    with pytest.raises(zt.InvalidParameters,
                       match=f"connected_components: {k} components do not fit uint8"):
        S.connected_components(src, tmp_path / "u8", data_type="uint8")
    assert not (tmp_path / "u8" / "zarr.json").exists()
    assert occ_ref.chunk_files(tmp_path / "u8") == set()
    assert ZF.main(["connected-components", src, str(tmp_path / "u8"), "-d", "uint8"]) == 1
    assert not (tmp_path / "u8" / "zarr.json").exists()
    assert occ_ref.chunk_files(tmp_path / "u8") == set()
