"""CPU half of the seeded watershed: the numpy restatement
tests/watershed_ref.py against hand-written answers and against an independent heap-based minimax
search written here; and everything of the feature that needs no GPU: the type table, the limits on
connectivity and rank, the shape refusals, the memory formula, the exported symbols and the
driver's grammar."""
import heapq
import itertools

import numpy as np
import pytest

from tests import ccl_ref
from tests import watershed_ref as W

import zarrs_tools_amd as zt
from zarrs_tools_amd import _abi
from zarrs_tools_amd import zarrs_watershed as ZW

ALL = list(_abi.DTYPES)
INTS = ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64")
SIZE = {"bool": 1, "int8": 1, "uint8": 1, "int16": 2, "uint16": 2, "bfloat16": 2, "float16": 2,
        "int32": 4, "uint32": 4, "float32": 4, "int64": 8, "uint64": 8, "float64": 8}
INF = 1 << 70


# ---- hand answers ---------------------------------------------------------------------------------

def test_plateau_tie_goes_to_the_lower_index():
    relief = np.ones(7, dtype=np.uint8)
    seeds = np.array([2, 0, 0, 0, 0, 0, 1], dtype=np.uint8)
    labels, st = W.watershed(relief, "uint8", seeds, with_steps=True)
    assert labels.tolist() == [2, 2, 2, 2, 1, 1, 1]
    assert st["d"].tolist() == [0, 1, 2, 3, 2, 1, 0]
    assert labels.dtype == seeds.dtype


def test_pass_element_drains_to_the_lower_side():
    relief = np.array([0, 3, 1, 5, 2, 4, 0], dtype=np.uint8)
    seeds = np.array([1, 0, 0, 0, 0, 0, 2], dtype=np.int16)
    labels, st = W.watershed(relief, "uint8", seeds, with_steps=True)
    assert labels.tolist() == [1, 1, 1, 1, 2, 2, 2]
    assert st["c"].tolist() == [0, 3, 3, 5, 4, 4, 0]


def test_foreground_only_stops_at_the_background():
    relief = np.array([2, 2, 0, 2, 2, 0, 2], dtype=np.uint8)
    seeds = np.array([0, 7, 0, 0, 0, 0, 0], dtype=np.uint8)
    assert W.watershed(relief, "uint8", seeds, foreground_only=True).tolist() == \
        [7, 7, 0, 0, 0, 0, 0]
    # without it the background is the lowest ground and everything is reached
    assert W.watershed(relief, "uint8", seeds).tolist() == [7] * 7
    # a seed outside the domain is ignored
    seeds2 = np.array([0, 0, 5, 0, 0, 0, 0], dtype=np.uint8)
    assert not W.watershed(relief, "uint8", seeds2, foreground_only=True).any()


def test_wall_at_both_connectivities():
    relief = np.array([[1, 1, 1, 1, 1], [1, 9, 9, 9, 1], [1, 1, 1, 1, 1]], dtype=np.uint8)
    seeds = np.zeros((3, 5), dtype=np.uint8)
    seeds[0, 0], seeds[2, 4] = 1, 2
    assert W.watershed(relief, "uint8", seeds, 1).tolist() == \
        [[1, 1, 1, 1, 2], [1, 1, 1, 1, 2], [1, 1, 2, 2, 2]]
    assert W.watershed(relief, "uint8", seeds, 2).tolist() == \
        [[1, 1, 1, 2, 2], [1, 1, 1, 1, 2], [1, 1, 2, 2, 2]]
    for c in (0, 3):
        with pytest.raises(ValueError):
            W.watershed(relief, "uint8", seeds, c)
    empty = np.zeros((3, 0, 4), dtype=np.uint8)
    assert W.watershed(empty, "uint8", empty, 2).shape == (3, 0, 4)


def test_long_chain_jumps():
    """A ramp of 4097 elements seeded at its foot: parents form one chain of 4096 links, which
    twelve jumps shorten to nothing; the thirteenth changes nothing."""
    relief = np.arange(4097, dtype=np.uint16)
    seeds = np.zeros(4097, dtype=np.uint8)
    seeds[0] = 3
    labels, st = W.watershed(relief, "uint16", seeds, with_steps=True)
    assert (labels == 3).all() and st["rounds"][2] == 13
    assert st["parent"].tolist() == [0] + list(range(4096))


# ---- an independent search ------------------------------------------------------------------------

def minimax(key, sources, allowed, connectivity):
    """Dijkstra with max in place of +: the least over paths inside `allowed` from a source of the
    greatest key on the path. Python ints; INF where no path exists."""
    shape = key.shape
    offsets = ccl_ref.neighbour_offsets(key.ndim, connectivity)
    cost = np.full(shape, INF, dtype=object)
    heap = []
    for p in zip(*np.nonzero(sources & allowed)):
        cost[p] = int(key[p])
        heapq.heappush(heap, (cost[p], p))
    while heap:
        c, p = heapq.heappop(heap)
        if c > cost[p]:
            continue
        for d in offsets:
            q = tuple(a + b for a, b in zip(p, d))
            if any(v < 0 or v >= n for v, n in zip(q, shape)) or not allowed[q]:
                continue
            cq = max(c, int(key[q]))
            if cq < cost[q]:
                cost[q] = cq
                heapq.heappush(heap, (cq, q))
    return cost


def random_case(rng, shape):
    relief = rng.integers(0, 4, size=shape).astype(np.uint8)  # few levels: ties abound; 0 = ground
    seeds = np.zeros(shape, dtype=np.int8)
    k = max(2, relief.size // 12)
    at = rng.choice(relief.size, size=k, replace=False)
    seeds.ravel()[at] = rng.choice(np.array([-3, 1, 2, 127], dtype=np.int8), size=k)
    return relief, seeds


@pytest.mark.parametrize("shape", [(37,), (9, 23), (4, 6, 9)])
def test_restatement_against_the_search(shape):
    rng = np.random.default_rng(len(shape) * 7919)
    for conn, fg, desc in itertools.product(range(1, len(shape) + 1), (False, True),
                                            (False, True)):
        relief, seeds = random_case(rng, shape)
        labels, st = W.watershed(relief, "uint8", seeds, conn, desc, fg, with_steps=True)
        dom = relief != 0 if fg else np.ones(shape, dtype=bool)
        seeded = dom & (seeds != 0)
        key = W.flood_key(relief, "uint8", desc)
        best = minimax(key, seeded, dom, conn)
        reached = best != INF
        what = (shape, conn, fg, desc)
        # seeds keep their labels; exactly the elements a seed reaches inside D are labelled
        assert np.array_equal(labels[seeded], seeds[seeded]), what
        assert np.array_equal(labels != 0, reached), what
        assert not reached[~dom].any()
        # c is the minimax cost
        assert np.array_equal(st["c"][reached].astype(object), best[reached]), what
        assert (st["d"][dom & ~reached] == W.NONE).all() and (st["d"][reached] >= 0).all(), what
        # the forest is optimal: inside every basin, from that basin's seeds alone, the cost is
        # the global one
        for lab in np.unique(seeds[seeded]):
            basin = labels == lab
            own = minimax(key, seeded & (seeds == lab), basin, conn)
            assert np.array_equal(own[basin], best[basin]), what + (int(lab),)
        # (c, d) falls strictly along parents
        flat_c, flat_d, par = st["c"].ravel(), st["d"].ravel(), st["parent"].ravel()
        for p in np.flatnonzero(reached.ravel() & ~seeded.ravel()):
            q = par[p]
            assert (flat_c[q], flat_d[q]) < (flat_c[p], flat_d[p]), what


def test_descending_is_ascending_on_negated_integers():
    rng = np.random.default_rng(5)
    for shape, conn in (((41,), 1), ((7, 19), 2), ((3, 5, 8), 3)):
        relief = rng.integers(-3, 4, size=shape).astype(np.int8)
        seeds = np.zeros(shape, dtype=np.uint16)
        at = rng.choice(relief.size, size=4, replace=False)
        seeds.ravel()[at] = [1, 2, 65535, 4]
        for fg in (False, True):
            a = W.watershed(relief, "int8", seeds, conn, True, fg)
            b = W.watershed((-relief).astype(np.int8), "int8", seeds, conn, False, fg)
            assert np.array_equal(a, b), (shape, fg)


def test_float_order_on_zeros_infinities_and_nans():
    """-NaN < -inf < -1 < -0.0 < +0.0 < 1 < +inf < +NaN, strictly: a rising ramp seeded at its foot
    has d = 0 everywhere (equal neighbours would give a plateau) and c = its own keys."""
    bits = np.array([0xFFC00001, 0xFF800000, 0xBF800000, 0x80000000, 0x00000000, 0x3F800000,
                     0x7F800000, 0x7FC00001], dtype=np.uint32)
    relief = bits.view(np.float32)
    seeds = np.array([1, 0, 0, 0, 0, 0, 0, 2], dtype=np.uint8)
    labels, st = W.watershed(relief, "float32", seeds, with_steps=True)
    assert labels.tolist() == [1] * 7 + [2]
    assert (st["d"] == 0).all() and (np.diff(st["c"].astype(np.int64)) > 0).all()
    labels, st = W.watershed(relief, "float32", seeds, descending=True, with_steps=True)
    assert labels.tolist() == [1] + [2] * 7
    assert (st["d"] == 0).all()
    # +-0.0 are background with foreground_only; the NaNs and infinities are not
    labels = W.watershed(relief, "float32", seeds, foreground_only=True)
    assert labels.tolist() == [1, 1, 1, 0, 0, 2, 2, 2]
    # the 16-bit floats travel as their bits
    half = np.array([0xFE01, 0xFC00, 0x8000, 0x0000, 0x7C00, 0x7E01], dtype=np.uint16)
    s16 = np.array([0, 0, 0, 9, 0, 0], dtype=np.int64)
    for dt in ("float16", "bfloat16"):
        h = half if dt == "float16" else np.array([0xFFC1, 0xFF80, 0x8000, 0x0000, 0x7F80, 0x7FC1],
                                                  dtype=np.uint16)
        _, st = W.watershed(h, dt, s16, with_steps=True)
        assert st["c"].tolist() == [int(W.flood_key(h, dt)[3])] * 4 + \
            W.flood_key(h, dt)[4:].tolist()


# ---- the surfaces that need no GPU ----------------------------------------------------------------

def test_type_table():
    f = zt.Watershed()
    assert f.name() == "watershed"
    assert (f.connectivity, f.descending, f.foreground_only) == (1, False, False)
    for relief in ALL:
        for seeds in ALL:
            if seeds in INTS:
                f.is_compatible(relief, seeds)
            else:
                with pytest.raises(zt.UnsupportedDataType, match="integer type"):
                    f.is_compatible(relief, seeds)
    with pytest.raises(zt.UnsupportedDataType):
        f.is_compatible("complex64", "uint8")
    assert _abi.lib().zt_watershed_is_compatible(_abi.DTYPES["float32"], 99) == \
        _abi.ERR_UNSUPPORTED_DATA_TYPE


def test_shape_refusals():
    import torch
    f = zt.Watershed()
    relief = torch.zeros((4, 5), dtype=torch.float32)
    with pytest.raises(zt.InvalidParameters, match="Array shapes do not match"):
        f.apply_ndarray(relief, torch.zeros((5, 4), dtype=torch.int32))
    with pytest.raises(zt.InvalidParameters, match="Array shapes do not match"):
        f.apply_ndarray(relief, torch.zeros((4, 5), dtype=torch.int32),
                        out=torch.zeros((4, 6), dtype=torch.int32))
    with pytest.raises(zt.UnsupportedDataType, match="integer type"):
        f.apply_ndarray(relief, torch.zeros((4, 5), dtype=torch.float32))
    with pytest.raises(zt.UnsupportedDataType, match="the seeds' data type int32, not int16"):
        f.apply_ndarray(relief, torch.zeros((4, 5), dtype=torch.int32),
                        out=torch.zeros((4, 5), dtype=torch.int16))


def test_connectivity_and_rank_limits():
    with pytest.raises(zt.InvalidParameters, match=r"connectivity 0 not in \[1, rank\]"):
        zt.Watershed(connectivity=0)
    lib = _abi.lib()
    out = _abi.ctypes.c_uint64()
    for shape in ((3,), (3, 3), (3, 3, 3), (1, 1, 3, 3, 3)):
        rank = len(shape)
        zt.Watershed(connectivity=rank).memory("uint8", "uint8", shape)
        with pytest.raises(zt.InvalidParameters,
                           match=rf"watershed: connectivity {rank + 1} not in \[1, {rank}\]"):
            zt.Watershed(connectivity=rank + 1).memory("uint8", "uint8", shape)
        # the library says the same, whoever calls it
        assert lib.zt_watershed_memory(5, 5, _abi.i64_array(shape), rank, rank + 1, 0,
                                       _abi.ctypes.byref(out)) == _abi.ERR_INVALID_PARAMETERS
        assert f"connectivity {rank + 1} not in [1, {rank}]" in lib.zt_last_error().decode()
    f = zt.Watershed()
    for shape in ((2, 3, 3, 3), (1, 2, 3, 3, 3), (2, 1, 3, 3, 3)):
        with pytest.raises(zt.InvalidParameters,
                           match=r"watershed: rank \d is supported only when every axis in front "
                                 "of the innermost three has extent 1"):
            f.memory("uint8", "uint8", shape)
    f.memory("uint8", "uint8", (1, 1, 1, 1, 1, 3, 3, 3))
    assert f.memory("uint8", "uint8", (2, 0, 3, 3, 3)) == 0  # a zero extent is a no-op
    # n < 2^32 - 1: indices are 32 bits wide and two values are marks
    f.memory("uint8", "uint8", (2 ** 32 - 2,))
    with pytest.raises(zt.InvalidParameters, match="elements are more than 4294967294"):
        f.memory("uint8", "uint8", (2 ** 32 - 1,))
    with pytest.raises(zt.InvalidParameters, match="elements are more than"):
        f.memory("uint8", "uint8", (2048, 2048, 1024))


def test_memory_formula():
    """inputs + output + scratch. The scratch, every part rounded up to 16 bytes: two working
    arrays of the relief's type for the pass values, a third with foreground_only (the relief with
    the greatest key outside the domain), two arrays of 4-byte indices (the distances, then the
    parents and roots), and 64 bytes of flag words."""
    def pad(b):
        return (b + 15) // 16 * 16
    cases = [("uint8", "uint8", (70, 45, 67)), ("float64", "int16", (9, 70)),
             ("bool", "uint64", (1001,)), ("uint16", "int8", (1, 4, 9, 17)),
             ("uint32", "uint32", (1024, 1024, 1024)), ("bfloat16", "int32", (3, 5, 7))]
    for relief, seeds, shape in cases:
        n = int(np.prod([int(s) for s in shape], dtype=object))
        for fg in (False, True):
            scratch = (3 if fg else 2) * pad(n * SIZE[relief]) + 2 * pad(4 * n) + 64
            got = zt.Watershed(foreground_only=fg).memory(relief, seeds, shape)
            assert got == n * SIZE[relief] + 2 * n * SIZE[seeds] + scratch, (relief, seeds, shape)
    assert zt.Watershed().memory("uint8", "uint8", (5, 0, 7)) == 0
    with pytest.raises(zt.UnsupportedDataType):
        zt.Watershed().memory("uint8", "float32", (5, 7))


def test_symbols_and_export():
    syms = _abi.header_symbols()
    for name in ("zt_watershed_is_compatible", "zt_watershed_memory", "zt_watershed_apply_array"):
        assert name in syms
        assert hasattr(_abi.lib(), name)
    assert "Watershed" in zt.__all__ and zt.Watershed is zt.filter.Watershed
    assert _abi.lib().zt_abi_version() == 4


def test_driver_grammar():
    ap = ZW.build_parser()
    a = ap.parse_args(["relief.zarr", "seeds.zarr", "out.zarr"])
    assert ZW.step_of(a) == {
        "input_path": "relief.zarr", "seeds_path": "seeds.zarr", "output_path": "out.zarr",
        "connectivity": 1, "descending": False, "foreground_only": False, "data_type": None,
        "device": 0, "nthreads": 0, "encoding": None}
    assert a.filter_skip_empty_chunks is False
    a = ap.parse_args(["--device", "1", "r", "s", "o", "--connectivity", "3", "--descending",
                       "--foreground-only", "--skip-empty-chunks", "-c", "16,16,32", "-s",
                       "32,32,64", "--bytes-to-bytes-codecs",
                       '[{"name": "gzip", "configuration": {"level": 1}}]', "-d", "uint32"])
    kw = ZW.step_of(a)
    assert (kw["connectivity"], kw["descending"], kw["foreground_only"], kw["device"]) == \
        (3, True, True, 1)
    assert kw["data_type"] == "uint32" and a.filter_skip_empty_chunks is True
    assert kw["encoding"] == {
        "data_type": "uint32", "chunk_shape": [16, 16, 32], "shard_shape": [32, 32, 64],
        "bytes_to_bytes_codecs": [{"name": "gzip", "configuration": {"level": 1}}]}
    for bad in (["r", "s"], ["r", "s", "o", "--connectivity", "x"], ["r", "s", "o", "extra"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    # the step kinds of zarrs_filter are untouched: the watershed is a tool of its own
    from zarrs_tools_amd import zarrs_filter as ZF
    assert "watershed" not in ZF.STEP_KINDS and "watershed" not in ZF.ON_PATH


def test_store_refusals_before_anything_is_read(tmp_path):
    from zarrs_tools_amd import store as S
    relief, seeds, bad_type, bad_shape, out = (str(tmp_path / n) for n in (
        "relief", "seeds", "bad_type", "bad_shape", "out"))
    S.create_array(relief, "float32", (6, 8), (4, 4))
    S.create_array(seeds, "uint16", (6, 8), (3, 8))
    S.create_array(bad_type, "float32", (6, 8), (4, 4))
    S.create_array(bad_shape, "uint16", (8, 6), (4, 4))
    with pytest.raises(zt.UnsupportedDataType, match="integer type"):
        S.watershed(relief, bad_type, out)
    with pytest.raises(zt.InvalidParameters, match="Array shapes do not match"):
        S.watershed(relief, bad_shape, out)
    with pytest.raises(zt.UnsupportedDataType, match="the seeds' data type uint16, not uint32"):
        S.watershed(relief, seeds, out, data_type="uint32")
    with pytest.raises(zt.InvalidParameters, match=r"connectivity 3 not in \[1, 2\]"):
        S.watershed(relief, seeds, out, connectivity=3)
    import os
    assert not os.path.exists(out)
    assert S.watershed_output("int8", None, {"chunk_shape": [2, 2]}) == (
        "int8", {"chunk_shape": [2, 2], "data_type": "int8", "fill_value": 0})
