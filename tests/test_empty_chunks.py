"""CPU: eliding fill-value chunks on write (zarrs' `store_empty_chunks = false`), host-scan path.

store.set_store_empty_chunks(False) makes the writes of this thread leave out the chunks, and
the inner chunks of shards, that hold nothing but the fill value; tests/occ_ref.py restates which
ones those are and what a shard's index then looks like. Writes from host data decide with a host
scan (memcmp against the fill pattern), so everything here runs without a GPU. The default
setting stores every chunk, as before."""
import json
import os

import numpy as np
import pytest

from tests import occ_ref as R
from zarrs_tools_amd import _abi
from zarrs_tools_amd import store as S

SHAPE, CHUNK = (20, 12, 40), (8, 8, 16)
SHARD, INNER = (16, 16, 32), (8, 8, 16)


@pytest.fixture(autouse=True)
def default_setting_afterwards():
    yield
    S.set_store_empty_chunks(True)


def sparse_u16(positions, shape=SHAPE, fill=0):
    a = np.full(shape, fill, dtype=np.uint16)
    for p in positions:
        a[p] = 7
    return a


def write(path, a, data_type, chunk, codecs=None, fill_value=None, elide=True):
    S.create_array(path, data_type, a.shape, chunk, codecs, fill_value)
    S.set_store_empty_chunks(not elide)
    S.write_array(path, a)
    elided = S.last_elided()
    S.set_store_empty_chunks(True)
    return elided


CASES = {
    "one_voxel": [(0, 0, 0)],
    "corners": [(0, 0, 0), (19, 11, 39)],
    "edge_chunks": [(17, 9, 33), (3, 9, 20)],
    "interior": [(9, 5, 17), (9, 5, 18), (15, 7, 31)],
    "nothing": [],
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_unsharded_files_data_and_counts(tmp_path, case):
    a = sparse_u16(CASES[case])
    p = str(tmp_path / "a")
    elided = write(p, a, "uint16", CHUNK)
    assert R.chunk_files(p) == R.expected_files(a, CHUNK, 0)
    assert np.array_equal(S.read_array(p), a)
    assert elided == R.elided_counts(a, CHUNK, 0)
    meta = json.load(open(os.path.join(p, "zarr.json")))
    # the default setting: every chunk file, the same metadata
    q = str(tmp_path / "b")
    assert write(q, a, "uint16", CHUNK, elide=False) == (0, 0)
    assert R.chunk_files(q) == R.all_files(SHAPE, CHUNK)
    assert np.array_equal(S.read_array(q), a)
    assert json.load(open(os.path.join(q, "zarr.json"))) == meta


def test_default_setting_is_store_every_chunk(tmp_path):
    assert S.store_empty_chunks() is True
    p = str(tmp_path / "a")
    S.create_array(p, "uint16", SHAPE, CHUNK)
    S.write_array(p, np.zeros(SHAPE, np.uint16))
    assert R.chunk_files(p) == R.all_files(SHAPE, CHUNK)
    assert S.last_elided() == (0, 0)


@pytest.mark.parametrize("compression", [None, "gzip"])
@pytest.mark.parametrize("case", ["one_voxel", "corners", "interior"])
def test_sharded_index_and_files(tmp_path, compression, case):
    a = sparse_u16(CASES[case])
    p = str(tmp_path / "a")
    codecs = S.codecs_json(compression, 1, shard_inner=INNER)
    elided = write(p, a, "uint16", SHARD, codecs)
    R.check_shards(p, a, SHARD, INNER, 0)
    assert np.array_equal(S.read_array(p), a)
    assert elided == R.elided_counts(a, SHARD, 0, INNER)
    # an all-fill shard has no file, and some shard of each case is all fill
    assert len(R.chunk_files(p)) < len(R.all_files(SHAPE, SHARD))
    # the default setting: every shard, no (2^64-1, 2^64-1) entry
    q = str(tmp_path / "b")
    write(q, a, "uint16", SHARD, codecs, elide=False)
    assert R.chunk_files(q) == R.all_files(SHAPE, SHARD)
    for key in R.chunk_files(q):
        idx, _ = R.shard_index(os.path.join(q, key), 8)
        assert (idx != np.uint64(R.NONE)).all()


def test_a_fully_empty_sharded_array_has_no_files(tmp_path):
    p = str(tmp_path / "a")
    a = sparse_u16([])
    elided = write(p, a, "uint16", SHARD, S.codecs_json(None, shard_inner=INNER))
    assert R.chunk_files(p) == set()
    assert elided == R.elided_counts(a, SHARD, 0, INNER)
    assert np.array_equal(S.read_array(p), a)


def test_stale_chunk_file_is_removed(tmp_path):
    p = str(tmp_path / "a")
    a = sparse_u16([(0, 0, 0), (9, 5, 17)])
    write(p, a, "uint16", CHUNK, elide=False)
    assert os.path.exists(os.path.join(p, "c/1/0/1"))
    b = sparse_u16([(0, 0, 0)])  # chunk (1, 0, 1) becomes empty
    S.set_store_empty_chunks(False)
    S.write_array(p, b)
    assert not os.path.exists(os.path.join(p, "c/1/0/1"))
    assert R.chunk_files(p) == R.expected_files(b, CHUNK, 0)
    assert np.array_equal(S.read_array(p), b)


def test_stale_shard_file_is_removed(tmp_path):
    p = str(tmp_path / "a")
    codecs = S.codecs_json(None, shard_inner=INNER)
    a = sparse_u16([(0, 0, 0), (17, 9, 33)])
    write(p, a, "uint16", SHARD, codecs, elide=False)
    assert os.path.exists(os.path.join(p, "c/1/0/1"))
    b = sparse_u16([(0, 0, 0)])  # shard (1, 0, 1) becomes empty
    S.set_store_empty_chunks(False)
    S.write_array(p, b)
    assert not os.path.exists(os.path.join(p, "c/1/0/1"))
    R.check_shards(p, b, SHARD, INNER, 0)
    assert np.array_equal(S.read_array(p), b)


def test_nan_fill_matches_only_its_payload(tmp_path):
    fill = 0x7FC00001
    bits = np.full(SHAPE, fill, dtype=np.uint32)
    bits[9, 5, 17] = 0x7FC00000  # another NaN: occupied
    a = bits.view(np.float32)
    p = str(tmp_path / "a")
    elided = write(p, a, "float32", CHUNK, fill_value="0x7fc00001")
    assert R.chunk_files(p) == R.expected_files(a, CHUNK, fill) == {"c/1/0/1"}
    assert elided == R.elided_counts(a, CHUNK, fill)
    assert np.array_equal(R.bits_of(S.read_array(p)), bits)


def test_negative_zero_is_not_the_fill_of_positive_zero(tmp_path):
    a = np.zeros(SHAPE, dtype=np.float32)
    a[17, 9, 33] = -0.0
    p = str(tmp_path / "a")
    write(p, a, "float32", CHUNK, fill_value=0.0)
    assert R.chunk_files(p) == R.expected_files(a, CHUNK, 0) == {"c/2/1/2"}
    assert np.array_equal(R.bits_of(S.read_array(p)), R.bits_of(a))


def test_bool_is_a_byte(tmp_path):
    a = np.zeros(SHAPE, dtype=np.bool_)
    a[3, 9, 20] = True
    p = str(tmp_path / "a")
    write(p, a, "bool", CHUNK, fill_value=False)
    assert R.chunk_files(p) == R.expected_files(a, CHUNK, 0) == {"c/0/1/1"}
    assert np.array_equal(S.read_array(p), a)
    # fill value true: the chunks of false are the occupied ones
    q = str(tmp_path / "b")
    b = ~a
    write(q, b, "bool", CHUNK, fill_value=True)
    assert R.chunk_files(q) == R.expected_files(b, CHUNK, 1) == {"c/0/1/1"}
    assert np.array_equal(S.read_array(q), b)


def test_int64_minus_one_fill(tmp_path):
    a = np.full(SHAPE, -1, dtype=np.int64)
    a[0, 0, 0] = 0
    a[19, 11, 39] = 0xFFFFFFFF  # equal to the fill value in its low word only
    p = str(tmp_path / "a")
    elided = write(p, a, "int64", CHUNK, fill_value=-1)
    fill = (1 << 64) - 1
    assert R.chunk_files(p) == R.expected_files(a, CHUNK, fill) == {"c/0/0/0", "c/2/1/2"}
    assert elided == R.elided_counts(a, CHUNK, fill)
    assert np.array_equal(S.read_array(p), a)


def test_partial_edge_chunk_of_fill_is_elided(tmp_path):
    # the edge chunks (2, *, *), (*, 1, *) and (*, *, 2) hold 4 of 8 planes, 4 of 8 rows and 8 of
    # 16 columns of the array: with a nonzero fill value their padding is not "data" either
    a = sparse_u16([(0, 0, 0)], fill=9)
    p = str(tmp_path / "a")
    elided = write(p, a, "uint16", CHUNK, fill_value=9)
    assert R.chunk_files(p) == {"c/0/0/0"}
    assert elided == (17, 17)
    assert np.array_equal(S.read_array(p), a)
    # and in a shard: the inner chunks of the edge shards beyond the array are not counted
    q = str(tmp_path / "b")
    elided = write(q, a, "uint16", SHARD, S.codecs_json(None, shard_inner=INNER), fill_value=9)
    R.check_shards(q, a, SHARD, INNER, 9)
    assert elided == (3, 17)
    assert np.array_equal(S.read_array(q), a)


def test_write_synth_scans_on_the_host(tmp_path):
    # noise: nothing is empty, nothing is elided, the files are those of the default setting
    p, q = str(tmp_path / "a"), str(tmp_path / "b")
    for path, store_all in ((p, True), (q, False)):
        S.create_array(path, "uint16", SHAPE, CHUNK)
        S.set_store_empty_chunks(store_all)
        S.write_synth(path, S.SYNTH_U16)
        assert S.last_elided() == (0, 0)
    assert R.chunk_files(p) == R.chunk_files(q) == R.all_files(SHAPE, CHUNK)
    assert np.array_equal(S.read_array(p), S.read_array(q))


def test_caller_supplied_map(tmp_path):
    a = sparse_u16(CASES["interior"])
    occ = R.occupancy(a, CHUNK, 0)
    p = str(tmp_path / "a")
    S.create_array(p, "uint16", SHAPE, CHUNK)
    S.set_store_empty_chunks(False)
    S.write_array(p, a, occupied=occ)
    assert R.chunk_files(p) == R.expected_files(a, CHUNK, 0)
    assert S.last_elided() == R.elided_counts(a, CHUNK, 0)
    assert np.array_equal(S.read_array(p), a)
    with pytest.raises(_abi.InvalidParameters):
        S.write_array(p, a, occupied=occ[:2])
    # a subset at an offset: the map is over the subset's inner chunks
    q = str(tmp_path / "b")
    S.create_array(q, "uint16", SHAPE, SHARD, S.codecs_json(None, shard_inner=INNER))
    S.write_array(q, a[16:], start=(16, 0, 0), occupied=R.occupancy(a[16:], INNER, 0))
    S.write_array(q, a[:16], start=(0, 0, 0), occupied=R.occupancy(a[:16], INNER, 0))
    R.check_shards(q, a, SHARD, INNER, 0)
    assert np.array_equal(S.read_array(q), a)
    # with the default setting the map is not consulted
    r = str(tmp_path / "c")
    S.create_array(r, "uint16", SHAPE, CHUNK)
    S.set_store_empty_chunks(True)
    S.write_array(r, a, occupied=np.zeros_like(occ))
    assert R.chunk_files(r) == R.all_files(SHAPE, CHUNK)


def test_write_empty_removes_files_without_data(tmp_path):
    p = str(tmp_path / "a")
    a = sparse_u16(CASES["corners"])
    write(p, a, "uint16", CHUNK, elide=False)
    S.set_store_empty_chunks(False)
    S.write_empty(p, (8, 0, 0), (12, 12, 40))
    assert R.chunk_files(p) == {k for k in R.all_files(SHAPE, CHUNK) if k.startswith("c/0/")}
    assert S.last_elided() == (12, 12)
    S.set_store_empty_chunks(True)
    with pytest.raises(_abi.InvalidParameters):  # no data needs elision on
        S.write_empty(p, (8, 0, 0), (12, 12, 40))


def test_new_symbols_and_the_pinned_abi():
    lib = _abi.lib()
    for name in ("zt_chunk_occupancy_is_compatible", "zt_chunk_occupancy",
                 "zt_store_set_store_empty_chunks", "zt_store_write_subset_occupancy",
                 "zt_store_last_elided"):
        assert name in _abi.header_symbols() and hasattr(lib, name)
    assert lib.zt_abi_version() == 4
    for dt in _abi.DTYPES.values():
        assert lib.zt_chunk_occupancy_is_compatible(dt) == 0
    assert lib.zt_chunk_occupancy_is_compatible(99) == _abi.ERR_UNSUPPORTED_DATA_TYPE


def test_restatement_pinned_by_hand():
    a = np.zeros((3, 5), dtype=np.uint8)
    a[2, 4] = 1
    assert R.occupancy(a, (2, 2), 0).tolist() == [[0, 0, 0], [0, 0, 1]]
    assert R.occupancy(a, (2, 2), 1).tolist() == [[1, 1, 1], [1, 1, 0]]
    assert R.occupancy(a, (4, 9), 0).tolist() == [[1]]
    f = np.array([0.0, -0.0], dtype=np.float32)
    assert R.occupancy(f, (1,), 0).tolist() == [0, 1]
    assert R.expected_files(a, (2, 2), 0) == {"c/1/2"}
    assert R.elided_counts(a, (2, 2), 0) == (5, 5)


def test_cli_flag_is_on_every_command():
    from zarrs_tools_amd import zarrs_filter as ZF
    from zarrs_tools_amd import zarrs_ome as ZO
    ap = ZF.build_parser()
    assert ap.parse_args(["--skip-empty-chunks", "reencode", "a", "b"]).skip_empty_chunks
    for argv in (["guided-filter", "a", "b", "1", "1"], ["downsample", "a", "b", "2,2,2"],
                 ["gaussian", "a", "b", "1,1,1", "3,3,3"], ["summed-area-table", "a", "b"],
                 ["reencode", "a", "b"], ["crop", "a", "b", "0,0,0", "1,1,1"],
                 ["rescale", "a", "b", "1", "0"], ["clamp", "a", "b", "0", "1"],
                 ["equal", "a", "b", "1"], ["replace-value", "a", "b", "1", "2"]):
        assert ap.parse_args(argv + ["--skip-empty-chunks"]).filter_skip_empty_chunks
        assert not ap.parse_args(argv).filter_skip_empty_chunks
    assert ZO.build_parser().parse_args(["a", "b", "--skip-empty-chunks"]).filter_skip_empty_chunks
