"""GPU: zarrs_validate's comparison (compare.hip through the C ABI, the store path and the
zarrs_validate command) against the numpy restatement (tests/cmp_ref.py). Counts and indices are
exact: there is no tolerance anywhere.

Borders of the kernel (compare.hip, zt_info.hpp): the first run decides the split into the
elements before the first 16-byte boundary (head), aligned 16-byte vectors of PER = 16 / element
size elements, and a tail of fewer than PER elements; a workgroup step is 256 lanes x 4 vectors =
STEP_VECS vectors, steps are grid-strided, ZT_INFO_MAX_BLOCKS caps the grid. The second run is
read as aligned vectors when it is congruent to the first mod 16, else at element alignment."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import cmp_ref as C
from tests.gpu_util import to_dev
from tests.test_info_gpu import dev
from tests.test_info_gpu import noise as numeric_noise

pytestmark = pytest.mark.gpu

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)
from zarrs_tools_amd import store as S  # noqa: E402
from zarrs_tools_amd import zarrs_validate as ZV  # noqa: E402

STEP_VECS = 256 * 4
SIZE = {dt: np.dtype(O.NP_STORAGE[dt]).itemsize for dt in C.ALL_TYPES}
FLOATS = ("bfloat16", "float16", "float32", "float64")
NAN = {2: (0x7E01, 0x7E02), 4: (0x7FC00001, 0x7FC00002), 8: (0x7FF8000000000001,
                                                            0x7FF8000000000002)}


def per(dt):
    return 16 // SIZE[dt]


def noise(dt, n, seed=0):
    """n storage elements of noise (test_info_gpu.noise; bool: bytes 0 and 1)."""
    if dt == "bool":
        return np.random.default_rng(seed).integers(0, 2, size=n, dtype=np.uint8)
    return numeric_noise(dt, n, seed)


def plant(v, positions):
    """A copy of v whose elements at `positions` (flat) have their lowest bit flipped."""
    w = v.copy()
    C.bits(w)[np.asarray(positions, dtype=np.int64)] ^= 1
    return w


def check(ta, tb, a, b):
    got, want = zt.Compare().apply_ndarray(ta, tb), C.compare(a, b)
    assert got == want, (got, want)
    return got


# ---- every type -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", C.ALL_TYPES)
def test_all_types(dt):
    shape = (7, 33, 70)
    n = int(np.prod(shape))
    a = noise(dt, n, 1)
    rng = np.random.default_rng(2)
    pos = np.unique(np.concatenate([[0, n - 1], rng.choice(n, size=10, replace=False)]))
    b = plant(a, pos)
    planted = len(pos)
    if dt in FLOATS:
        ua, ub = C.bits(a), C.bits(b)
        free = np.setdiff1d(np.arange(100, 200), pos)[:3]
        sign = 1 << (8 * SIZE[dt] - 1)
        ua[free[0]], ub[free[0]] = 0, sign  # +0.0 against -0.0: differs
        ua[free[1]], ub[free[1]] = NAN[SIZE[dt]]  # two NaN payloads: differ
        ua[free[2]] = ub[free[2]] = NAN[SIZE[dt]][0]  # one NaN, the same bits: equal
        planted += 2
    a, b = a.reshape(shape), b.reshape(shape)
    ta, tb = dev(a, dt), dev(b, dt)
    assert check(ta, tb, a, b) == (planted, 0)
    assert check(ta, ta.clone(), a, a) == (0, None)
    assert check(zt.DeviceArray(ta, (4, 16, 32)), zt.DeviceArray(tb, (2, 33, 8)), a, b)[0] == planted
    # without the planted first element: the first difference is somewhere inside
    C.bits(b)[0] = C.bits(a)[0]
    assert check(ta, dev(b, dt), a, b)[0] == planted - 1


def test_mismatches_are_invalid_parameters():
    import torch
    a = torch.zeros((4, 6), dtype=torch.float32, device="cuda")
    with pytest.raises(zt.InvalidParameters, match="Array shapes do not match"):
        zt.Compare().apply_ndarray(a, a.reshape(6, 4))
    with pytest.raises(zt.InvalidParameters, match="Array data types do not match"):
        zt.Compare().apply_ndarray(a, a.to(torch.int32))


# ---- lengths around the kernel's borders ----------------------------------------------------------

@pytest.mark.parametrize("blocks", ["1", "2"])
@pytest.mark.parametrize("dt", ["uint8", "float64"])
def test_lengths(monkeypatch, dt, blocks):
    # one workgroup: every step is a trip of the grid-stride loop; two: the last length takes two
    monkeypatch.setenv("ZT_INFO_MAX_BLOCKS", blocks)
    p, step = per(dt), STEP_VECS * per(dt)
    for n in (0, 1, p - 1, p, p + 1, step - 1, step, step + 1, 2 * step + p + 1):
        a = noise(dt, n, 10 + n % 7)
        ta = dev(a, dt)
        assert check(ta, ta.clone(), a, a) == (0, None)
        if n == 0:
            continue
        places = {0: [0], n - 1: [n - 1]}
        if n >= p:  # the last whole vector's last element
            places[n // p * p - 1] = [n // p * p - 1]
        places["all"] = sorted(k for k in places if k != "all")
        for where, pos in places.items():
            b = plant(a, pos)
            assert check(ta, dev(b, dt), a, b) == (len(pos), pos[0]), (n, where)


# ---- alignment ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["uint8", "float32"])
def test_alignment(dt):
    p = per(dt)
    n = STEP_VECS * p + 3 * p + 2  # two steps, a tail
    a = noise(dt, n, 20)
    rng = np.random.default_rng(21)
    pos = np.unique(np.concatenate([[0, n - 1], rng.choice(n, size=8, replace=False)]))
    b = plant(a, pos)
    inner = plant(a, pos[1:-1])
    for oa in (0, 1, 3):
        for ob in (0, 1, 3):  # oa == ob: congruent mod 16, both aligned vector paths
            ta, tb = dev(a, dt, oa), dev(b, dt, ob)
            assert (ta.data_ptr() - tb.data_ptr()) % 16 == ((oa - ob) * SIZE[dt]) % 16
            assert check(ta, tb, a, b) == (len(pos), 0), (oa, ob)
            assert check(ta, dev(a, dt, ob), a, a) == (0, None), (oa, ob)
            assert check(ta, dev(inner, dt, ob), a, inner) == (len(pos) - 2, int(pos[1])), (oa, ob)


# ---- elements are counted, not words or bytes -----------------------------------------------------

def test_element_counting():
    a = np.full(64, 7, dtype=np.uint64)
    b = a.copy()
    a[33], b[33] = 0x0000000100000001, 0x0000000200000002  # both words differ: one element
    assert check(dev(a, "uint64"), dev(b, "uint64"), a, b) == (1, 33)
    a = np.arange(1, 65, dtype=np.uint16)
    b = a.copy()
    b[34], b[35] = 3000, 4000  # the two halves of one 32-bit word: two elements
    assert check(dev(a, "uint16"), dev(b, "uint16"), a, b) == (2, 34)
    a = np.arange(64, dtype=np.int64)
    b = a.copy()
    b[5] ^= np.int64(1) << np.int64(56)  # only the high byte differs
    b[63] ^= np.int64(-2**63)
    assert check(dev(a, "int64"), dev(b, "int64"), a, b) == (2, 5)
    a = np.zeros(64, dtype=np.uint8)
    b = a.copy()
    b[16:32] = 0x80  # every byte of one vector
    b[40] = 1
    assert check(dev(a, "uint8"), dev(b, "uint8"), a, b) == (17, 16)


# ---- accumulation ---------------------------------------------------------------------------------

def test_accumulation_across_calls_with_base():
    dt = "float32"
    n = 30001
    a = noise(dt, n, 30)
    pos = [12345 + 777, 20000, n - 1]
    b = plant(a, pos)
    cuts = [0, 12345, 20003, n]  # the first run is equal, the first difference is in the second
    c = zt.Compare()
    state = c.new_state()
    assert c.finish(state) == (0, None)
    for i in range(3):
        lo, hi = cuts[i], cuts[i + 1]
        c.accumulate(dev(a[lo:hi], dt), dev(b[lo:hi], dt, i), state, base=lo)
    c.accumulate(dev(a[:0], dt), dev(b[:0], dt), state, base=5)  # n == 0: a no-op
    assert c.finish(state) == C.compare(a, b) == (3, pos[0])
    # the order of the runs does not matter
    state = c.new_state()
    for i in (2, 0, 1):
        lo, hi = cuts[i], cuts[i + 1]
        c.accumulate(dev(a[lo:hi], dt), dev(b[lo:hi], dt), state, base=lo)
    assert c.finish(state) == (3, pos[0])
    # an index past 2^32 survives
    state = c.new_state()
    c.accumulate(dev(a[:100], dt), dev(plant(a[:100], [7]), dt), state, base=2**40)
    assert c.finish(state) == (1, 2**40 + 7)


# ---- the store path -------------------------------------------------------------------------------

SHAPE, CHUNK_A, CHUNK_B = (5, 9, 11), (2, 4, 8), (3, 9, 4)  # partial edge chunks in both grids
CODECS_B = {"gzip": dict(compression="gzip", level=1), "sharded": dict(shard_inner=(3, 3, 2))}


@pytest.fixture(scope="module")
def u16_data():
    return noise("uint16", int(np.prod(SHAPE)), 40).reshape(SHAPE)


def make_store(path, data, chunk, dt="uint16", codecs=None, **kw):
    S.create_array(path, dt, data.shape, chunk, S.codecs_json(**(codecs or {})), **kw)
    S.write_array(path, data)
    return path


@pytest.mark.parametrize("codec", ["gzip", "sharded"])
def test_store_two_chunk_grids(tmp_path, u16_data, codec):
    a = make_store(tmp_path / "a.zarr", u16_data, CHUNK_A)
    b = make_store(tmp_path / "b.zarr", u16_data, CHUNK_B, codecs=CODECS_B[codec])
    stats = {}
    assert S.compare(a, b, stats=stats) == (0, None)
    assert stats["voxels"] == u16_data.size and stats["rows"] == 3
    assert S.compare(b, a) == (0, None)
    rng = np.random.default_rng(41)
    pos = np.sort(rng.choice(u16_data.size, size=9, replace=False))
    other = plant(u16_data, pos)
    want = C.compare(u16_data, other)
    assert want == (9, int(pos[0]))
    d = make_store(tmp_path / "d.zarr", other, CHUNK_B, codecs=CODECS_B[codec])
    assert S.compare(a, d) == want
    assert S.compare(d, a) == want
    assert S.compare(a, d, chunk_limit=2, nthreads=2) == want
    # rows of the first array combine to the whole
    parts = [S.compare(a, d, rows=(r, r + 1)) for r in range(3)]
    for r, part in enumerate(parts):
        lo, hi = 2 * r * 99, min(2 * (r + 1), 5) * 99
        inside = pos[(pos >= lo) & (pos < hi)]
        assert part == (len(inside), int(inside[0]) if len(inside) else None)
    assert zt.combine_compares(parts) == want
    assert S.compare(a, d, rows=(3, 5)) == (0, None)  # no such rows


def test_store_progress_counts_the_chunks_of_both(tmp_path, u16_data):
    a = make_store(tmp_path / "a.zarr", u16_data, CHUNK_A)
    b = make_store(tmp_path / "b.zarr", u16_data, CHUNK_B)
    steps = []
    S.set_progress_callback(lambda s: steps.append((s["step"], s["num_steps"])))
    try:
        assert S.compare(a, b) == (0, None)
    finally:
        S.set_progress_callback(None)
    # rows of 2 planes: 3 x 2 chunks of a each; planes 0-1, 2-3 and 4 meet 1, 2 and 1 chunk rows
    # of b, 1 x 3 chunks each
    total = 3 * 6 + (1 + 2 + 1) * 3
    assert sorted(s for s, _ in steps) == list(range(1, total + 1))
    assert {t for _, t in steps} == {total}


def test_store_absent_chunk_equals_stored_fill_values(tmp_path, u16_data):
    data = u16_data.copy()
    data[2:4, 4:8, 8:11] = 1234  # chunk (1, 1, 1) of the first grid, clipped to the shape
    a = make_store(tmp_path / "a.zarr", data, CHUNK_A, fill_value=1234)
    os.remove(a / "c" / "1" / "1" / "1")
    b = make_store(tmp_path / "b.zarr", data, CHUNK_B, codecs=CODECS_B["gzip"])
    assert S.compare(a, b) == (0, None)
    assert S.compare(b, a) == (0, None)
    # against the original noise the absent chunk differs wherever the noise is not the fill
    o = make_store(tmp_path / "o.zarr", u16_data, CHUNK_B)
    assert S.compare(a, o) == C.compare(data, u16_data)
    assert C.compare(data, u16_data)[0] >= 20


def test_store_rank_1(tmp_path):
    data = noise("float32", 100, 42)
    a = make_store(tmp_path / "a.zarr", data, (7,), dt="float32")
    b = make_store(tmp_path / "b.zarr", data, (13,), dt="float32")
    assert S.compare(a, b) == (0, None)
    other = plant(data, [50, 98, 99])
    d = make_store(tmp_path / "d.zarr", other, (13,), dt="float32")
    assert S.compare(a, d) == C.compare(data, other) == (3, 50)
    parts = [S.compare(d, a, rows=(r, r + 1)) for r in range(8)]
    assert zt.combine_compares(parts) == (3, 50)
    assert parts[3] == (1, 50) and parts[7] == (2, 98)


# ---- the command ----------------------------------------------------------------------------------

def test_cli(tmp_path, u16_data, capsys):
    a = make_store(tmp_path / "a.zarr", u16_data, CHUNK_A)
    b = make_store(tmp_path / "b.zarr", u16_data, CHUNK_B, codecs=CODECS_B["gzip"])
    assert ZV.main([str(a), str(b)]) == 0
    cap = capsys.readouterr()
    assert cap.out == f"Success: {a} and {b} match\n" and cap.err == ""
    idx = (3 * 9 + 5) * 11 + 9  # element (3, 5, 9): chunk (1, 1, 1) of the first grid
    other = plant(u16_data, [idx, idx + 1, u16_data.size - 1])
    d = make_store(tmp_path / "d.zarr", other, CHUNK_B)
    assert ZV.main(["--concurrent-chunks", "2", str(a), str(d)]) == 1
    cap = capsys.readouterr()
    region = zt.ArraySubset((2, 4, 8), (2, 4, 3))
    assert cap.out == "" and cap.err.startswith(f"Data differs in region: {region}")
    assert "3 differing elements" in cap.err and f"index {idx}" in cap.err
    # the second array's grid names its own chunk
    assert ZV.main([str(d), str(a)]) == 1
    cap = capsys.readouterr()
    assert cap.err.startswith(f"Data differs in region: {zt.ArraySubset((3, 0, 8), (2, 9, 3))}")
    e = tmp_path / "e.zarr"
    S.create_array(e, "uint16", (5, 9, 12), CHUNK_B)
    assert ZV.main([str(a), str(e)]) == 1
    cap = capsys.readouterr()
    assert cap.out == "" and "Array shapes do not match: [5, 9, 11] vs [5, 9, 12]" in cap.err
