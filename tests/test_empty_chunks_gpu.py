"""GPU: the chunk-occupancy kernel (occupancy.hip through the C ABI) and the store filters that
elide fill-value chunks with it, against the numpy restatement (tests/occ_ref.py). Everything is
exact: flags, files, shard indices and element bits.

Borders of the kernel: the box is one contiguous run split into the elements before the first
16-byte boundary (head), aligned 16-byte vectors of PER = 16 / element size elements and a tail
of fewer than PER elements; a wave owns consecutive chunks of 64 lanes x 4 vectors (4 KiB);
ZT_INFO_MAX_BLOCKS caps the grid, so a small cap gives every wave several chunks (its row position
then advances from chunk to chunk, and after a chunk with data the wave looks at the flags before
it loads the next). A vector may straddle rows of the box and cells."""
import json
import os

import numpy as np
import pytest

from tests import occ_ref as R
from tests.gpu_util import to_dev

pytestmark = pytest.mark.gpu

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)
from zarrs_tools_amd import store as S  # noqa: E402
from zarrs_tools_amd import zarrs_filter as ZF  # noqa: E402
from zarrs_tools_amd import zarrs_ome as ZO  # noqa: E402

BOX, CELLS = (3, 5, 23), (2, 2, 5)
from oracle import oracle as O  # noqa: E402

STORAGE = O.NP_STORAGE  # the numpy type that holds a data type's storage bits
FILL_BITS = {1: 0x5A, 2: 0x7E01, 4: 0x7FC00001, 8: 0x7FF8000000000001}


def occupancy(a, dtype, cells, fill_bits):
    """The kernel's map of a host array, as numpy."""
    occ = zt.chunk_occupancy(to_dev(a, dtype), cells, hex(fill_bits))
    return occ.cpu().numpy()


def filled(shape, dtype, fill_bits):
    """An array of the fill value, as its storage type."""
    st = np.dtype(STORAGE[dtype])
    u = np.full(shape, fill_bits, dtype=R._UINT[st.itemsize])
    return u.view(st)


def sparse(shape, dtype, fill_bits, seed, density):
    a = filled(shape, dtype, fill_bits)
    rng = np.random.default_rng(seed)
    hit = rng.random(shape) < density
    R.bits_of(a)[hit] ^= rng.integers(1, 1 << 8, size=shape, dtype=np.uint64).astype(
        R._UINT[a.dtype.itemsize])[hit]
    return a


def test_every_position_of_a_uint8_box_marks_exactly_its_cell():
    import torch
    n = int(np.prod(BOX))
    assert n == 345
    # variant i (345 bytes from byte offset 345 * i: every alignment mod 16) has element i non-fill
    host = np.full((n, n), 0x5A, dtype=np.uint8)
    host[np.arange(n), np.arange(n)] = 0x5B
    dev = torch.from_numpy(host).cuda()
    got = torch.stack([zt.chunk_occupancy(dev[i].view(BOX), CELLS, 0x5A) for i in range(n)])
    got = got.cpu().numpy()
    want = np.zeros((n,) + (2, 3, 5), dtype=np.uint8)
    for i, idx in enumerate(np.ndindex(*BOX)):
        want[(i,) + tuple(v // c for v, c in zip(idx, CELLS))] = 1
    assert want.reshape(n, -1).sum(axis=1).tolist() == [1] * n
    assert np.array_equal(got, want)


@pytest.mark.parametrize("dtype", ["int16", "bfloat16", "float16", "uint32", "float32", "int64",
                                   "float64", "bool"])
def test_wider_types_sparse_fill_and_dense(dtype):
    fb = FILL_BITS[np.dtype(STORAGE[dtype]).itemsize]
    for seed, density in ((1, 0.01), (2, 0.05), (3, 0.3)):
        a = sparse(BOX, dtype, fb, seed, density)
        assert np.array_equal(occupancy(a, dtype, CELLS, fb), R.occupancy(a, CELLS, fb))
    a = filled(BOX, dtype, fb)
    assert not occupancy(a, dtype, CELLS, fb).any()
    assert occupancy(a, dtype, CELLS, fb ^ 1).all()  # dense: no element has this fill value


def test_float_fill_values_are_compared_by_their_bits():
    a = np.array([0x7FC00001, 0x7FC00000, 0x7FC00001, 0x7FC00001], np.uint32).view(np.float32)
    assert occupancy(a, "float32", (1,), 0x7FC00001).tolist() == [0, 1, 0, 0]
    z = np.array([0.0, -0.0, 0.0], np.float64)
    assert occupancy(z, "float64", (1,), 0).tolist() == [0, 1, 0]
    assert occupancy(z, "float64", (1,), 1 << 63).tolist() == [1, 0, 1]
    # the value forms of a fill value: a number, "NaN" (the canonical one), true / false
    x = to_dev(np.array([0.0, np.nan, 1.0], np.float32), "float32")
    assert zt.chunk_occupancy(x, (1,), 0.0).cpu().tolist() == [0, 1, 1]
    assert zt.chunk_occupancy(x, (1,), "NaN").cpu().tolist() == [1, 0, 1]
    dev_arr = zt.DeviceArray(x, (2,))
    assert dev_arr.chunk_occupancy(1.0).cpu().tolist() == [1, 0]
    assert zt.default_context().chunk_occupancy(x, (3,), 0).cpu().tolist() == [1]


@pytest.mark.parametrize("shape, cells", [
    ((1000,), (7,)),
    ((37, 53), (5, 16)),
    ((3, 4, 9, 11), (2, 3, 4, 5)),
    ((2, 3, 5, 7, 23), (1, 1, 2, 2, 5)),          # tczyx with unit cells on t and c
    ((2, 1, 3, 2, 2, 3, 2, 5), (1, 1, 2, 1, 2, 2, 1, 3)),
])
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_ranks(shape, cells, dtype):
    fb = FILL_BITS[np.dtype(STORAGE[dtype]).itemsize]
    for seed, density in ((4, 0.003), (5, 0.05)):
        a = sparse(shape, dtype, fb, seed, density)
        assert np.array_equal(occupancy(a, dtype, cells, fb), R.occupancy(a, cells, fb))


@pytest.mark.parametrize("cells", [(1, 1, 1), (1, 5, 1), (3, 5, 23), (4, 9, 100), (2, 9, 23),
                                   (1, 2, 40)])
def test_unit_cells_and_cells_larger_than_the_box(cells):
    for dtype in ("uint8", "int16", "float64"):
        fb = FILL_BITS[np.dtype(STORAGE[dtype]).itemsize]
        a = sparse(BOX, dtype, fb, 6, 0.02)
        got = occupancy(a, dtype, cells, fb)
        assert got.shape == tuple(-(-n // c) for n, c in zip(BOX, cells))
        assert np.array_equal(got, R.occupancy(a, cells, fb))


@pytest.mark.parametrize("dtype", ["uint8", "int16", "float32", "float64"])
def test_data_pointer_at_an_odd_element_offset(dtype):
    fb = FILL_BITS[np.dtype(STORAGE[dtype]).itemsize]
    n = int(np.prod(BOX))
    big = sparse((n + 9,), dtype, fb, 7, 0.02)
    dev = to_dev(big, dtype)
    for off in (1, 3, 7):
        got = zt.chunk_occupancy(dev[off:off + n].view(BOX), CELLS, hex(fb)).cpu().numpy()
        assert np.array_equal(got, R.occupancy(big[off:off + n].reshape(BOX), CELLS, fb))


def test_zero_extent_box():
    import torch
    x = torch.empty((4, 0, 6), dtype=torch.float32, device="cuda")
    assert tuple(zt.chunk_occupancy(x, (2, 2, 2), 0.0).shape) == (2, 0, 3)
    with pytest.raises(zt.InvalidParameters):
        zt.chunk_occupancy(x, (2, 0, 2), 0.0)
    with pytest.raises(zt.InvalidParameters):
        zt.chunk_occupancy(x, (2, 2), 0.0)


@pytest.mark.parametrize("blocks", ["1", "3"])
def test_waves_with_several_chunks(monkeypatch, blocks):
    """A capped grid: every wave walks many 4 KiB chunks, through rows that are no multiple of a
    vector, with fill, sparse and dense stretches (the dense ones take the look-before-load path)."""
    monkeypatch.setenv("ZT_INFO_MAX_BLOCKS", blocks)
    shape, cells = (9, 61, 1003), (4, 16, 100)
    for dtype in ("uint8", "float32"):
        fb = FILL_BITS[np.dtype(STORAGE[dtype]).itemsize]
        a = sparse(shape, dtype, fb, 8, 0.0002)
        R.bits_of(a)[2:5, 10:40, 300:900] ^= 1  # a dense block
        R.bits_of(a)[7] = fb                      # planes of fill
        assert np.array_equal(occupancy(a, dtype, cells, fb), R.occupancy(a, cells, fb))


def test_indices_beyond_2_to_the_31():
    import torch
    n = (1 << 31) + 48
    x = torch.full((n,), 3, dtype=torch.uint8, device="cuda")
    assert zt.chunk_occupancy(x, (1 << 30,), 3).cpu().tolist() == [0, 0, 0]
    x[n - 1] = 4
    assert zt.chunk_occupancy(x, (1 << 30,), 3).cpu().tolist() == [0, 0, 1]
    del x
    torch.cuda.empty_cache()


# ---- the store filters -----------------------------------------------------------------------------

SHAPE, CHUNK = (20, 12, 40), (8, 8, 16)
SHARD, INNER = (16, 16, 32), (8, 8, 16)
VOXELS = [(9, 5, 17), (9, 5, 18), (19, 11, 39)]


@pytest.fixture(autouse=True)
def default_setting_afterwards():
    yield
    S.set_store_empty_chunks(True)


def make_input(path, sharded, value=7):
    a = np.zeros(SHAPE, dtype=np.uint16)
    for v in VOXELS:
        a[v] = value
    codecs = S.codecs_json(None, shard_inner=INNER) if sharded else None
    S.create_array(path, "uint16", SHAPE, SHARD if sharded else CHUNK, codecs)
    S.write_array(path, a)
    return a


def check_store(path, want, sharded, fill_bits=0):
    if sharded:
        R.check_shards(path, want, SHARD, INNER, fill_bits)
    else:
        assert R.chunk_files(path) == R.expected_files(want, CHUNK, fill_bits)


@pytest.mark.parametrize("sharded", [False, True])
@pytest.mark.parametrize("op", ["equal", "reencode"])
def test_store_filters_elide(tmp_path, op, sharded):
    src = str(tmp_path / "in")
    a = make_input(src, sharded)
    run = (lambda dst, **kw: S.equal(src, dst, 7, **kw)) if op == "equal" else (
        lambda dst, **kw: S.reencode(src, dst, **kw))
    want = (a == 7) if op == "equal" else a
    full, el = str(tmp_path / "full"), str(tmp_path / "elided")
    st_full = run(full)
    assert st_full["chunks_elided"] == 0
    grid = SHARD if sharded else CHUNK
    assert R.chunk_files(full) == R.all_files(SHAPE, grid)
    S.set_store_empty_chunks(False)
    steps = []
    S.set_progress_callback(lambda p: steps.append((p["step"], p["num_steps"])))
    try:
        st = run(el)
    finally:
        S.set_progress_callback(None)
    S.set_store_empty_chunks(True)
    check_store(el, want, sharded)
    counts = R.elided_counts(want, grid, 0, INNER if sharded else None)
    assert st["chunks_elided"] == counts[0] and S.last_elided() == counts
    assert st["bytes_written"] < st_full["bytes_written"]
    # an elided chunk still is a progress step
    n_chunks = len(R.all_files(SHAPE, grid))
    assert sorted(steps) == [(i + 1, n_chunks) for i in range(n_chunks)]
    assert S.compare(el, full) == (0, None)
    assert json.load(open(os.path.join(el, "zarr.json"))) == json.load(
        open(os.path.join(full, "zarr.json")))
    # two halves of the chunk rows give the same store as one call
    halves = str(tmp_path / "halves")
    S.set_store_empty_chunks(False)
    n_rows = -(-SHAPE[0] // grid[0])
    run(halves, rows=(0, 1), finish=False)
    run(halves, rows=(1, n_rows), erase=False)
    assert R.chunk_files(halves) == R.chunk_files(el)
    for key in R.chunk_files(el):
        assert open(os.path.join(halves, key), "rb").read() == open(
            os.path.join(el, key), "rb").read()


def test_overwriting_removes_chunks_that_became_empty(tmp_path):
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    a = make_input(src, False)
    S.reencode(src, dst)
    assert R.chunk_files(dst) == R.all_files(SHAPE, CHUNK)
    S.set_store_empty_chunks(False)
    S.reencode(src, dst)
    assert R.chunk_files(dst) == R.expected_files(a, CHUNK, 0)
    assert np.array_equal(S.read_array(dst), a)


def test_other_store_filters_elide_too(tmp_path):
    """downsample (--discrete), Gaussian and the guided filter with a column window go through
    the same rows: their elided outputs equal their default outputs, with fewer files."""
    src = str(tmp_path / "in")
    a = np.zeros((32, 24, 48), dtype=np.uint16)
    a[20:24, 10:14, 30:40] = 5
    S.create_array(src, "uint16", a.shape, (8, 8, 16))
    S.write_array(src, a)
    runs = {
        "ds": lambda d: S.downsample(src, d, (2, 2, 2), discrete=True),
        "gauss": lambda d: S.gaussian(src, d, (1.0, 1.0, 1.0), (2, 2, 2)),
        "guided_cols": lambda d: S.guided_filter(src, d, 1.0, 1, cols=(1, 3)),
    }
    for name, run in runs.items():
        full, el = str(tmp_path / (name + "_full")), str(tmp_path / (name + "_el"))
        S.set_store_empty_chunks(True)
        run(full)
        S.set_store_empty_chunks(False)
        st = run(el)
        S.set_store_empty_chunks(True)
        assert st["chunks_elided"] > 0 and S.compare(el, full) == (0, None), name
        info = S.open_array(el)
        if name == "guided_cols":  # the window's chunks only
            want = S.read_array(full)
            keep = {k for k in R.expected_files(want, info.chunk_shape, 0)
                    if k.split("/")[2] in ("1", "2")}
            assert R.chunk_files(el) == keep
        else:
            want = S.read_array(el)
            assert R.chunk_files(el) == R.expected_files(want, info.chunk_shape, 0), name


def test_device_resident_chain_equals_the_store_path(tmp_path):
    src = str(tmp_path / "in")
    a = make_input(src, True)

    def steps(out):
        return [{"filter": "equal", "input": src, "output": "$m", "value": 7},
                {"filter": "reencode", "input": "$m", "output": out, "data_type": "uint8"}]
    dev_out, store_out = str(tmp_path / "dev"), str(tmp_path / "store")
    res = ZF.run(steps(dev_out), tmp=str(tmp_path), log=lambda *x: None, skip_empty_chunks=True)
    assert any(r.get("device_resident") for r in res)
    res2 = ZF.run(steps(store_out), tmp=str(tmp_path), log=lambda *x: None, device_chain=False,
                  skip_empty_chunks=True)
    assert S.store_empty_chunks() is True  # put back after the run
    want = (a == 7).astype(np.uint8)
    for out in (dev_out, store_out):
        R.check_shards(out, want, SHARD, INNER, 0)
        assert np.array_equal(S.read_array(out), want)
    counts = R.elided_counts(want, SHARD, 0, INNER)
    assert res[-1]["chunks_elided"] == res2[-1]["chunks_elided"] == counts[0]
    for key in R.chunk_files(dev_out):
        assert open(os.path.join(dev_out, key), "rb").read() == open(
            os.path.join(store_out, key), "rb").read()


@pytest.mark.parametrize("device_resident", [True, False])
def test_zarrs_ome_skips_the_empty_chunks_of_a_label_pyramid(tmp_path, device_resident):
    src, out = str(tmp_path / "in"), str(tmp_path / "ome")
    a = np.zeros((64, 64, 64), dtype=np.uint16)
    a[40:56, 8:24, 32:48] = 3  # one label; the rest is background (the fill value)
    S.create_array(src, "uint16", a.shape, (8, 8, 8))
    S.write_array(src, a)
    assert ZO.main([src, out, "--discrete", "--skip-empty-chunks", "--max-levels", "2"]
                   + ([] if device_resident else ["--no-device-resident"])) == 0
    assert S.store_empty_chunks() is True
    # level 0 is a copy of the input's files
    assert R.chunk_files(os.path.join(out, "0")) == R.all_files(a.shape, (8, 8, 8))
    lvl = a
    for i in (1, 2):
        lvl = lvl[::2, ::2, ::2]  # the mode of 2x2x2 blocks of a block-aligned label
        path = os.path.join(out, str(i))
        info = S.open_array(path)
        assert np.array_equal(S.read_array(path), lvl)
        want = R.expected_files(lvl, info.chunk_shape, 0)
        assert R.chunk_files(path) == want
        assert len(want) < len(R.all_files(lvl.shape, info.chunk_shape))
