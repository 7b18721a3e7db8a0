"""GPU parity of morphological reconstruction (reconstruct.hip through the C ABI, the store step,
the zarrs_filter command, run configs and device-resident chains) against its numpy restatement
(tests/recon_ref.py): equal storage bytes everywhere, into a poisoned output. The result is the
unique least fixed point, so no run is repeated to look for races.

Borders of the kernels (reconstruct.hip): a workgroup of a round owns a tile of T = _abi.REC_TILE
= (8, 8, 32) elements of the three innermost axes with a one-element apron; the init kernel works
16 bytes per lane when every pointer is 16-byte aligned and element by element otherwise; the host
launches _abi.REC_BATCH rounds between two reads of their flag words.
"""
import json

import numpy as np
import pytest

from oracle import oracle as O
from tests import ccl_ref as C
from tests import occ_ref
from tests import recon_ref as R
from tests.gpu_util import from_dev, poisoned, to_dev

pytestmark = pytest.mark.gpu

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)
from zarrs_tools_amd import _abi  # noqa: E402
from zarrs_tools_amd import store as S  # noqa: E402
from zarrs_tools_amd import zarrs_filter as ZF  # noqa: E402

ALL = list(_abi.DTYPES)
TZ, TY, TX = _abi.REC_TILE
BIG = (TZ + 1, TY + 1, 2 * TX + 1)  # more than one tile on every axis, a one-element last tile
FLAT = (2 * TY + 1, 2 * TX + 1)
QUIET = dict(log=lambda *a: None)


def gpu(mask, dtype="uint8", mode="marker", marker=None, method="dilation", connectivity=1,
        h=None):
    import torch
    y = poisoned(mask.shape, dtype)
    f = zt.Reconstruction(method, connectivity, mode, h)

    def named(a):  # the data type by name: a bool array travels as a uint8 tensor
        return zt.DeviceArray(to_dev(a, dtype), (4,) * a.ndim, dtype)

    out, rounds = f.apply_ndarray(named(mask), None if marker is None else named(marker), out=y)
    torch.cuda.synchronize()
    assert out is y
    return from_dev(y, dtype), rounds


def same(out, ref, what):
    assert out.dtype == ref.dtype and out.shape == ref.shape, what
    if out.tobytes() != ref.tobytes():
        bits = f"u{ref.dtype.itemsize}"
        differ = out.view(bits) != ref.view(bits)
        i = tuple(int(v) for v in np.argwhere(differ)[0])
        raise AssertionError(f"{int(differ.sum())} of {ref.size} elements differ ({what}), first "
                             f"at {i}: got {out[i]!r}, want {ref[i]!r}")


def check(mask, dtype="uint8", mode="marker", marker=None, methods=("dilation",),
          connectivities=None, h=None):
    """Equal bytes at every connectivity of the rank (or the ones given); returns the rounds and
    the last result."""
    mask = np.ascontiguousarray(mask, dtype=O.NP_STORAGE[dtype])
    if marker is not None:
        marker = np.ascontiguousarray(marker, dtype=O.NP_STORAGE[dtype])
    rounds, out = [], None
    for c in connectivities or range(1, mask.ndim + 1):
        for method in methods:
            ref = R.apply(mask, dtype, mode, marker, method, c, h)
            out, r = gpu(mask, dtype, mode, marker, method, c, h)
            same(out, ref, (mask.shape, dtype, mode, method, c))
            assert 1 <= r <= mask.size + 1
            rounds.append(r)
    return rounds, out


def grey(shape, seed=0):
    """(mask, marker): uint8 values 0 to 5, 3 % of the marker set to the mask."""
    rng = np.random.default_rng(seed)
    mask = rng.integers(0, 6, shape).astype(np.uint8)
    return mask, np.where(rng.random(shape) < 0.03, mask, 0).astype(np.uint8)


def noise(shape, density, seed=0):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


# ---- shapes ----------------------------------------------------------------------------------------

SHAPES = ([(e, 5, 7) for e in (1, TZ, TZ + 1, 2 * TZ + 1)]
          + [(3, e, 7) for e in (1, TY, TY + 1, 2 * TY + 1)]
          + [(3, 5, e) for e in (1, TX, TX + 1, 2 * TX + 1)]
          + [BIG, (37,), (9, 70), FLAT, (1, 1, 9, 9, 70)])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_connectivities_methods_and_modes(shape):
    seed = len(shape) * 100 + sum(shape)
    mask, marker = grey(shape, seed)
    check(mask, "uint8", "marker", marker, R.METHODS)
    check(noise(shape, 0.6, seed), "uint8", "fill_holes")
    check(mask, "uint8", "h_maxima", h=2.0)
    check(mask, "uint8", "h_minima", h=2.0)


def test_zero_extent_is_a_no_op():
    for shape in ((0,), (3, 0, 5), (0, 4)):
        z = np.zeros(shape, np.uint8)
        out, rounds = gpu(z, "uint8", "marker", z)
        assert rounds == 0 and out.shape == shape
        assert gpu(z, "uint8", "fill_holes")[1] == 0


def test_device_arrays_and_the_c_abi():
    import torch
    mask, marker = grey((5, 9, 70), 3)
    ref = R.reconstruct(mask, marker, "uint8", "dilation", 2)
    f = zt.Reconstruction(connectivity=2)
    out, rounds = f.apply_ndarray(to_dev(mask, "uint8"), to_dev(marker, "uint8"))
    torch.cuda.synchronize()
    assert zt.dtype_of(out) == "uint8" and rounds >= 1
    assert from_dev(out, "uint8").tobytes() == ref.tobytes()
    y = poisoned(mask.shape, "uint8")
    r2 = f.apply(zt.DeviceArray(to_dev(mask, "uint8"), (4, 4, 4)),
                 zt.DeviceArray(to_dev(marker, "uint8"), (4, 4, 4)), zt.DeviceArray(y, (4, 4, 4)))
    torch.cuda.synchronize()
    assert r2 == rounds and from_dev(y, "uint8").tobytes() == ref.tobytes()
    # a generated marker: apply(mask, output)
    y = poisoned(mask.shape, "uint8")
    zt.Reconstruction(mode="fill_holes", connectivity=3).apply(
        zt.DeviceArray(to_dev(mask, "uint8"), (4, 4, 4)), zt.DeviceArray(y, (4, 4, 4)))
    torch.cuda.synchronize()
    assert from_dev(y, "uint8").tobytes() == R.apply(mask, "uint8", "fill_holes",
                                                     connectivity=3).tobytes()
    # the C ABI with a NULL rounds pointer and a NULL marker
    x, y = to_dev(mask, "uint8"), poisoned(mask.shape, "uint8")
    ctx = zt.default_context(0)
    _abi.check(_abi.lib().zt_reconstruction_apply_array(
        ctx.handle, _abi.DTYPES["uint8"], x.data_ptr(), None, _abi.REC_MODES["h_maxima"], 1.0,
        y.data_ptr(), _abi.i64_array(mask.shape), 3, 1, 0, None))
    torch.cuda.synchronize()
    assert from_dev(y, "uint8").tobytes() == R.apply(mask, "uint8", "h_maxima", h=1.0).tobytes()


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "float64"])
def test_element_aligned_pointers(dtype):
    """A base pointer one element past a 16-byte boundary: the init kernel goes element by
    element, and the rounds load at element alignment."""
    import torch
    rng = np.random.default_rng(7)
    st = O.NP_STORAGE[dtype]
    shape = (3, 9, 2 * TX)
    mask = rng.integers(0, 6, shape).astype(st)
    marker = np.where(rng.random(shape) < 0.05, mask, 0).astype(st)
    esz = np.dtype(st).itemsize
    flat = to_dev(np.concatenate([[1], mask.reshape(-1)]).astype(st), dtype)
    x = flat[1:].view(shape)
    assert x.data_ptr() % 16 == esz % 16 and x.is_contiguous()
    for mode, m in (("marker", marker), ("fill_holes", None)):
        y = poisoned(shape, dtype)
        zt.Reconstruction(connectivity=3, mode=mode).apply_ndarray(
            x, None if m is None else to_dev(m, dtype), out=y)
        torch.cuda.synchronize()
        same(from_dev(y, dtype), R.apply(mask, dtype, mode, m, connectivity=3), (dtype, mode))
    # ... and the marker and the output off the boundary, the mask on it
    mflat = to_dev(np.concatenate([[1], marker.reshape(-1)]).astype(st), dtype)
    yflat = poisoned((mask.size + 1,), dtype)
    zt.Reconstruction().apply_ndarray(to_dev(mask, dtype), mflat[1:].view(shape),
                                      out=yflat[1:].view(shape))
    torch.cuda.synchronize()
    same(from_dev(yflat, dtype)[1:].reshape(shape), R.reconstruct(mask, marker, dtype), dtype)


# ---- structures ------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [BIG, FLAT], ids=["3d", "2d"])
def test_least_marker_and_marker_equal_to_the_mask_take_one_round(shape):
    mask, _ = grey(shape, 1)
    rounds, out = check(mask, "uint8", "marker", np.zeros(shape, np.uint8))
    assert rounds == [1] * len(shape) and not out.any()  # least AND mask
    rounds, out = check(mask, "uint8", "marker", np.full(shape, 255, np.uint8),
                        methods=("erosion",))
    assert rounds == [1] * len(shape) and (out == 255).all()
    for method in R.METHODS:
        rounds, out = check(mask, "uint8", "marker", mask, methods=(method,))
        assert rounds == [1] * len(shape) and np.array_equal(out, mask)
    # a marker above the mask is clipped, not an error
    rounds, out = check(mask, "uint8", "marker", np.full(shape, 255, np.uint8))
    assert np.array_equal(out, mask)


@pytest.mark.parametrize("shape", [BIG, FLAT, (2 * TX + 1,)], ids=["3d", "2d", "1d"])
def test_a_single_seed_in_the_last_tile_floods_against_the_c_order(shape):
    mask = np.full(shape, 7, np.uint8)
    marker = np.zeros(shape, np.uint8)
    marker[(-1,) * len(shape)] = 9
    rounds, out = check(mask, "uint8", "marker", marker)
    assert (out == 7).all() and min(rounds) >= 2
    # by erosion: one low element pulls a plateau down to the mask
    low = np.full(shape, 200, np.uint8)
    low[(-1,) * len(shape)] = 3
    rounds, out = check(np.full(shape, 3, np.uint8), "uint8", "marker", low, methods=("erosion",))
    assert (out == 3).all()


@pytest.mark.parametrize("shape", [BIG, FLAT], ids=["3d", "2d"])
def test_serpentine_and_spiral_corridors(shape):
    """Corridors one element wide that cross tile faces many times, a seed at one end."""
    for figure in (C.serpentine(shape), C.spiral(shape), C.spiral(shape)[..., ::-1, ::-1]):
        mask = figure.astype(np.uint8) * 5
        for at in ((0,) * len(shape), tuple(int(v) for v in np.argwhere(figure)[-1])):
            marker = np.zeros(shape, np.uint8)
            marker[at] = 9
            rounds, out = check(mask, "uint8", "marker", marker)
            assert np.array_equal(out, mask)  # the whole corridor is reached


def test_one_sweep_per_round_spans_several_flag_batches(monkeypatch):
    """ZT_REC_TILE_SWEEPS=1: a round is one Jacobi sweep of the whole array (in a 2-D array a
    tile's column along z is one element, so nothing moves faster), the seed's value advances one
    element per round along the corridor, and the call takes as many rounds as the restatement
    takes sweeps: the corridor's length, many batches of flag words."""
    figure = C.serpentine(FLAT)
    length = int(figure.sum())
    assert length > 4 * _abi.REC_BATCH  # from T alone: (TY + 1) rows of 2 TX + 1, and the joints
    mask = figure.astype(np.uint8) * 5
    marker = np.zeros(FLAT, np.uint8)
    marker[0, 0] = 5
    ref, sweeps = R.reconstruct(mask, marker, "uint8", with_sweeps=True)
    assert sweeps == length and np.array_equal(ref, mask)
    _, few = gpu(mask, "uint8", "marker", marker)
    monkeypatch.setenv("ZT_REC_TILE_SWEEPS", "1")  # read at every call
    out, rounds = gpu(mask, "uint8", "marker", marker)
    same(out, ref, "one sweep per round")
    assert rounds > _abi.REC_BATCH and rounds == sweeps and few < rounds
    # 3-D, where a column along z moves in one sweep: no fewer rounds than the longest corridor
    # in a plane needs, and the same bytes
    figure = C.serpentine(BIG)
    mask = figure.astype(np.uint8) * 5
    marker = np.zeros(BIG, np.uint8)
    marker[0, 0, 0] = 5
    out, rounds = gpu(mask, "uint8", "marker", marker, connectivity=3)
    same(out, R.reconstruct(mask, marker, "uint8", "dilation", 3), "3-D, one sweep per round")
    assert rounds > _abi.REC_BATCH


def reached(a, b, shape, connectivity):
    """Whether a seed in blob `a` reaches blob `b` (index tuples of slices) under a + b."""
    mask = np.zeros(shape, np.uint8)
    mask[a] = 4
    mask[b] = 4
    marker = np.zeros(shape, np.uint8)
    marker[a] = 4
    _, out = check(mask, "uint8", "marker", marker, connectivities=(connectivity,))
    got = out[b]
    assert (got == 4).all() or not got.any()
    return bool(got.all())


def test_blobs_that_meet_across_a_tile_corner_or_edge():
    s = slice
    # 3-D corners of the tiles at (TZ, TY, TX): the blobs differ on three axes, on every diagonal
    corners = [((s(TZ - 3, TZ), s(TY - 3, TY), s(TX - 3, TX)), (s(TZ, None), s(TY, None), s(TX, TX + 3))),
               ((s(TZ - 3, TZ), s(TY, None), s(TX - 3, TX)), (s(TZ, None), s(TY - 3, TY), s(TX, TX + 3))),
               ((s(TZ - 3, TZ), s(TY - 3, TY), s(TX, TX + 3)), (s(TZ, None), s(TY, None), s(TX - 3, TX))),
               ((s(TZ - 3, TZ), s(TY, None), s(TX, TX + 3)), (s(TZ, None), s(TY - 3, TY), s(TX - 3, TX)))]
    for a, b in corners:
        for first, second in ((a, b), (b, a)):
            assert [reached(first, second, BIG, c) for c in (1, 2, 3)] == [False, False, True]
    # across an edge only: two axes differ
    edges = [((s(2, 3), s(TY - 3, TY), s(TX, TX + 3)), (s(2, 3), s(TY, None), s(TX - 3, TX))),
             ((s(TZ - 3, TZ), s(4, 5), s(TX - 3, TX)), (s(TZ, None), s(4, 5), s(TX, TX + 3))),
             ((s(TZ - 3, TZ), s(TY, None), s(5, 6)), (s(TZ, None), s(TY - 3, TY), s(5, 6)))]
    for a, b in edges:
        for first, second in ((a, b), (b, a)):
            assert [reached(first, second, BIG, c) for c in (1, 2, 3)] == [False, True, True]
    # 2-D: both diagonals of a tile corner
    for a, b in [((s(TY - 3, TY), s(TX - 3, TX)), (s(TY, TY + 3), s(TX, TX + 3))),
                 ((s(TY, TY + 3), s(TX - 3, TX)), (s(TY - 3, TY), s(TX, TX + 3)))]:
        for first, second in ((a, b), (b, a)):
            assert [reached(first, second, FLAT, c) for c in (1, 2)] == [False, True]


def test_holes_across_tiles_and_a_diagonal_gap_on_a_tile_corner():
    # 2-D: a ring around the corner of four tiles; its hole spans all four
    ring = np.zeros(FLAT, np.uint8)
    ring[TY - 4:TY + 4, TX - 5:TX + 5] = 1
    ring[TY - 3:TY + 3, TX - 4:TX + 4] = 0
    filled = ring.copy()
    filled[TY - 3:TY + 3, TX - 4:TX + 4] = 1
    for c in (1, 2):
        _, out = check(ring, "uint8", "fill_holes", connectivities=(c,))
        assert np.array_equal(out, filled)
    _, out = check(ring, "bool", "fill_holes")
    assert np.array_equal(out, filled)
    # 3-D: a hollow box around the corner of eight tiles
    box = np.zeros(BIG, np.uint8)
    box[TZ - 3:TZ + 1, TY - 3:TY + 1, TX - 4:TX + 4] = 1
    box[TZ - 2:TZ, TY - 2:TY, TX - 3:TX + 3] = 0
    solid = box.copy()
    solid[TZ - 2:TZ, TY - 2:TY, TX - 3:TX + 3] = 1
    for c in (1, 2, 3):
        _, out = check(box, "uint8", "fill_holes", connectivities=(c,))
        assert np.array_equal(out, solid)
    # the ring's corner element is the first element of tile (1, 1) and is missing: the hole's
    # last element (TY - 1, TX - 1), in tile (0, 0), touches the outside by that diagonal only
    ring = np.zeros(FLAT, np.uint8)
    ring[2:TY + 1, TX - 6:TX + 1] = 1
    ring[3:TY, TX - 5:TX] = 0
    ring[TY, TX] = 0
    filled = ring.copy()
    filled[3:TY, TX - 5:TX] = 1
    _, out = check(ring, "uint8", "fill_holes", connectivities=(1,))
    assert np.array_equal(out, filled)
    _, out = check(ring, "uint8", "fill_holes", connectivities=(2,))
    assert np.array_equal(out, ring)  # it leaks
    # the same gap in 3-D, on the corner (TZ, TY, TX): it leaks at connectivity 3 only
    box = np.zeros(BIG, np.uint8)
    box[TZ - 3:TZ + 1, TY - 3:TY + 1, TX - 4:TX + 1] = 1
    box[TZ - 2:TZ, TY - 2:TY, TX - 3:TX] = 0
    box[TZ, TY, TX] = 0
    solid = box.copy()
    solid[TZ - 2:TZ, TY - 2:TY, TX - 3:TX] = 1
    for c, want in ((1, solid), (2, solid), (3, box)):
        _, out = check(box, "uint8", "fill_holes", connectivities=(c,))
        assert np.array_equal(out, want), c


# ---- element types ---------------------------------------------------------------------------------------

SPECIAL = {  # storage bits
    "bool": [0, 1],
    "int8": [0x00, 0x01, 0xFF, 0x80, 0x7F], "uint8": [0x00, 0x01, 0xFF, 0x80, 0x7F],
    "int16": [0, 1, 0xFFFF, 0x8000, 0x7FFF, 0x0100], "uint16": [0, 1, 0xFFFF, 0x8000, 0x0100],
    "int32": [0, 1, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 0x00010000],
    "uint32": [0, 1, 0xFFFFFFFF, 0x80000000, 0x00010000],
    # values that differ only in bit 32 and above (low words 5 and 0), and 1 << 63 against 1
    "int64": [0, 1, 5, (1 << 32) | 5, (2 << 32) | 5, 1 << 63, (1 << 64) - 1, (1 << 63) | 5,
              3 << 32],
    "uint64": [0, 1, 5, (1 << 32) | 5, (2 << 32) | 5, 1 << 63, (1 << 64) - 1, (1 << 63) | 5,
               3 << 32],
    # +-0.0, subnormals, 1.0, infinities and NaNs of both signs (with payloads)
    "float16": [0x0000, 0x8000, 0x0001, 0x8001, 0x3C00, 0xBC00, 0x7C00, 0xFC00, 0x7E01, 0xFE01],
    "bfloat16": [0x0000, 0x8000, 0x0001, 0x8001, 0x3F80, 0xBF80, 0x7F80, 0xFF80, 0x7FC1, 0xFFC1],
    "float32": [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x3F800000, 0xBF800000,
                0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC00001],
    "float64": [0, 1 << 63, 1, (1 << 63) | 1, 0x3FF0 << 48, 0xBFF0 << 48, 0x7FF0 << 48,
                0xFFF0 << 48, (0x7FF8 << 48) | 1, (0xFFF8 << 48) | 1, 1 << 32, (1 << 63) | (1 << 32)],
}


def typed(dtype, shape, seed):
    st = np.dtype(O.NP_STORAGE[dtype])
    bits = np.array(SPECIAL[dtype], dtype=np.uint64)
    pick = np.random.default_rng(seed).integers(0, len(bits), shape)
    return bits[pick].astype(f"u{st.itemsize}").view(st).reshape(shape)


@pytest.mark.parametrize("dtype", ALL)
def test_every_type_on_its_special_values(dtype):
    shape = (5, 9, TX + 3)
    mask = typed(dtype, shape, 11)
    check(mask, dtype, "marker", typed(dtype, shape, 13), R.METHODS, (1, 3))
    check(mask, dtype, "fill_holes", connectivities=(2,))


@pytest.mark.parametrize("dtype", ["int64", "uint64"])
def test_64_bit_keys_are_compared_whole(dtype):
    """A comparison of the low words alone fails here. A = 2 << 32 | 1 is above B = 1 << 32 | 7
    and their low words order the other way: a seed of A floods the B elements as B, where a
    truncated minimum keeps A. For uint64, 1 << 63 is above 1 and its low word, 0, is below."""
    st = O.NP_STORAGE[dtype]
    a, b, p = (2 << 32) | 1, (1 << 32) | 7, 1 << 63

    def run(mask, marker, method="dilation"):
        mask, marker = (np.array(v, dtype=np.uint64).view(st) for v in (mask, marker))
        out, _ = gpu(mask, dtype, "marker", marker, method, 1)
        same(out, R.reconstruct(mask, marker, dtype, method, 1), (dtype, method))
        return out.view(np.uint64).tolist()

    assert run([a, b, a, b, a], [a, 0, 0, 0, 0]) == [a, b, b, b, b]
    assert run([b, a, b, a, b], [b, a, a, a, a], "erosion") == [b, a, a, a, a]
    if dtype == "uint64":
        assert run([p, 1, p], [p, 0, 0]) == [p, 1, 1]
    else:  # 1 << 63 is the least int64
        assert run([1, p, 1], [1, p, p]) == [1, p, p]
        assert run([p, 1, p], [p, 1, 1], "erosion") == [p, 1, 1]
    # and a plateau of values that differ in bit 32 and above only
    u = np.array([(3 << 32) | 5, (1 << 32) | 5, (2 << 32) | 5, 5, p, 1], dtype=np.uint64)
    mask = np.tile(u.view(st), 12).reshape(4, 18)
    marker = np.roll(mask, 1, axis=1)
    for method in R.METHODS:
        out, _ = gpu(mask, dtype, "marker", marker, method, 1)
        same(out, R.reconstruct(mask, marker, dtype, method, 1), (dtype, method))


@pytest.mark.parametrize("dtype", [d for d in ALL if d != "bool"])
def test_h_modes_per_type_and_saturation(dtype):
    st = np.dtype(O.NP_STORAGE[dtype])
    rng = np.random.default_rng(21)
    shape = (3, 9, TX + 1)
    if dtype in ("float16", "bfloat16", "float32", "float64"):
        values = rng.integers(-6, 7, shape).astype(np.float64) * 0.5
        values[rng.random(shape) < 0.03] = np.inf
        values[rng.random(shape) < 0.03] = -np.inf
        from tests.sat_ref import as_cast
        mask = as_cast(values, "float64", dtype).reshape(shape)
        h = 1.5
    else:
        info = np.iinfo(st)
        near = np.array([info.min, info.min + 1, info.min + 3, info.max - 3, info.max - 1,
                         info.max], dtype=st)
        mask = near[rng.integers(0, len(near), shape)]
        h = 2.0
    for mode in ("h_maxima", "h_minima"):
        check(mask, dtype, mode, h=h, connectivities=(1, 3))
    if dtype in ("int8", "uint8"):  # h beyond the whole range: the marker is the type's limit
        info = np.iinfo(st)
        _, out = check(mask, dtype, "h_maxima", h=300.0, connectivities=(1,))
        assert (out == mask.min()).all()  # flat at the lowest value: info.min is present
        assert mask.min() == info.min and mask.max() == info.max
        _, out = check(mask, dtype, "h_minima", h=300.0, connectivities=(1,))
        assert (out == info.max).all()


# ---- refusals --------------------------------------------------------------------------------------------

def test_refusals_leave_the_output_untouched():
    import torch
    mask, marker = grey((5, 9, 20), 2)
    x, m = to_dev(mask, "uint8"), to_dev(marker, "uint8")

    def refused(exc, match, f, *args, shape=mask.shape, dtype="uint8"):
        y = poisoned(shape, dtype)
        before = from_dev(y, dtype).tobytes()
        with pytest.raises(exc, match=match):
            f.apply_ndarray(*args, out=y)
        torch.cuda.synchronize()
        assert from_dev(y, dtype).tobytes() == before

    f = zt.Reconstruction()
    refused(zt.UnsupportedDataType, "one data type", f, x, to_dev(marker.astype(np.uint16),
                                                                  "uint16"))
    refused(zt.UnsupportedDataType, "one data type", f, x, m, dtype="int8")
    refused(zt.InvalidParameters, "Array shapes do not match", f, x,
            to_dev(marker[:, :, :19], "uint8"))
    refused(zt.InvalidParameters, "Array shapes do not match", f, x, m, shape=(5, 9, 19))
    refused(zt.InvalidParameters, "needs a marker array", f, x)
    refused(zt.InvalidParameters, "no marker array is given", zt.Reconstruction(mode="fill_holes"),
            x, m)
    b = zt.DeviceArray(to_dev((mask > 2).astype(np.uint8), "bool"), (4, 4, 4), "bool")
    for mode in ("h_maxima", "h_minima"):
        refused(zt.UnsupportedDataType, "not bool", zt.Reconstruction(mode=mode, h=1.0), b,
                dtype="bool")
    # a bool mask and a uint8 marker are two types, though both travel as uint8 tensors
    refused(zt.UnsupportedDataType, "one data type", f, b, m, dtype="bool")
    refused(zt.InvalidParameters, r"connectivity 4 not in \[1, 3\]",
            zt.Reconstruction(connectivity=4), x, m)
    x4 = to_dev(np.zeros((2, 3, 4, 5), np.uint8), "uint8")
    refused(zt.InvalidParameters, "rank 4 is supported only when every axis in front of the "
            "innermost three has extent 1", zt.Reconstruction(mode="fill_holes"), x4,
            shape=(2, 3, 4, 5))
    # the C ABI's own checks: connectivity, h, the method, the marker mode
    y = poisoned(mask.shape, "uint8")
    before = from_dev(y, "uint8").tobytes()
    ctx = zt.default_context(0)

    def call(mode, h, connectivity, method, marker_ptr=m.data_ptr()):
        return _abi.lib().zt_reconstruction_apply_array(
            ctx.handle, _abi.DTYPES["uint8"], x.data_ptr(), marker_ptr, mode, h, y.data_ptr(),
            _abi.i64_array(mask.shape), 3, connectivity, method, None)

    for c in (0, 4):
        with pytest.raises(zt.InvalidParameters, match=rf"connectivity {c} not in \[1, 3\]"):
            _abi.check(call(0, 0.0, c, 0))
    for h in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(zt.InvalidParameters, match="h must be finite and > 0"):
            _abi.check(call(2, h, 1, 0))
    with pytest.raises(zt.InvalidParameters, match="unknown method 2"):
        _abi.check(call(0, 0.0, 1, 2))
    with pytest.raises(zt.InvalidParameters, match="unknown marker mode 4"):
        _abi.check(call(4, 0.0, 1, 0))
    with pytest.raises(zt.InvalidParameters, match="null data pointer"):
        _abi.check(call(0, 0.0, 1, 0, None))
    torch.cuda.synchronize()
    assert from_dev(y, "uint8").tobytes() == before


# ---- store path ---------------------------------------------------------------------------------------------

SHAPE, CHUNK = (40, 33, 45), (16, 16, 32)


@pytest.fixture(scope="module")
def stored(tmp_path_factory):
    """uint8 with ragged chunks: boxes of 1 and 2 with hollow ones among them, the chunks of
    z >= 32, x >= 32 missing (they read as the fill value 0); and a marker of another chunk grid.
    Returns the paths, the arrays as they read, and the references that several tests share."""
    root = tmp_path_factory.mktemp("rec")
    rng = np.random.default_rng(42)
    v = np.zeros(SHAPE, np.uint8)
    for _ in range(40):
        z, y, x = (int(rng.integers(0, s - 2)) for s in SHAPE)
        dz, dy, dx = (int(rng.integers(3, 12)) for _ in range(3))
        v[z:z + dz, y:y + dy, x:x + dx] = rng.integers(1, 3)
        if rng.random() < 0.6:  # hollow
            v[z + 1:z + dz - 1, y + 1:y + dy - 1, x + 1:x + dx - 1] = 0
    S.create_array(root / "in", "uint8", SHAPE, CHUNK, fill_value=0)
    S.write_array(root / "in", v[:32])
    S.write_array(root / "in", v[32:, :, :32], start=(32, 0, 0))
    v[32:, :, 32:] = 0
    assert np.array_equal(S.read_array(root / "in"), v)
    m = np.where(rng.random(SHAPE) < 0.01, v, 0).astype(np.uint8)
    S.create_array(root / "marker", "uint8", SHAPE, (8, 33, 16), fill_value=0)
    S.write_array(root / "marker", m)
    refs = {"fill1": R.apply(v, "uint8", "fill_holes", connectivity=1),
            "fill3": R.apply(v, "uint8", "fill_holes", connectivity=3),
            "rec2": R.reconstruct(v, m, "uint8", "dilation", 2)}
    assert not np.array_equal(refs["fill1"], v) and refs["rec2"].any()
    return str(root / "in"), str(root / "marker"), v, m, refs


def test_store_function_subcommand_and_run_config(stored, tmp_path):
    src, marker, v, m, refs = stored
    st = S.reconstruction(src, tmp_path / "a", mode="fill_holes")
    assert st["rounds"] >= 2 and st["voxels"] == v.size and st["kernel_s"] > 0
    a = S.open_array(tmp_path / "a")
    assert a.data_type == "uint8" and a.shape == SHAPE and a.chunk_shape == CHUNK
    assert a.metadata["fill_value"] == 0
    assert S.read_array(tmp_path / "a").tobytes() == refs["fill1"].tobytes()
    # a marker with another chunk grid, through the store function
    st = S.reconstruction(src, tmp_path / "m", marker, connectivity=2)
    assert st["rounds"] >= 2
    assert S.read_array(tmp_path / "m").tobytes() == refs["rec2"].tobytes()
    # the subcommand, into a sharded and gzip compressed output
    assert S.codec_available("gzip")
    argv = ["reconstruction", src, str(tmp_path / "b"), "--marker", marker, "--connectivity", "2",
            "-s", "32,32,64", "-c", "16,16,32",
            "--bytes-to-bytes-codecs", json.dumps([{"name": "gzip", "configuration": {"level": 1}}])]
    assert ZF.main(argv) == 0
    b = S.open_array(tmp_path / "b")
    assert b.data_type == "uint8" and b.chunk_shape == (32, 32, 64)
    assert b.inner_chunk_shape == (16, 16, 32)
    assert S.read_array(tmp_path / "b").tobytes() == refs["rec2"].tobytes()
    assert ZF.main(["reconstruction", src, str(tmp_path / "b3"), "--fill-holes",
                    "--connectivity", "3"]) == 0
    assert S.read_array(tmp_path / "b3").tobytes() == refs["fill3"].tobytes()
    # by erosion, and the h modes, through the subcommand
    assert ZF.main(["reconstruction", src, str(tmp_path / "e"), "--marker", marker, "--method",
                    "erosion"]) == 0
    assert S.read_array(tmp_path / "e").tobytes() == R.reconstruct(v, m, "uint8",
                                                                   "erosion").tobytes()
    assert ZF.main(["reconstruction", src, str(tmp_path / "h"), "--h-maxima", "1"]) == 0
    assert S.read_array(tmp_path / "h").tobytes() == R.apply(v, "uint8", "h_maxima",
                                                             h=1.0).tobytes()
    # a run config; the step logs its rounds
    lines = []
    cfg = [{"filter": "reconstruction", "input": src, "output": str(tmp_path / "c"),
            "mode": "h_minima", "h": 1, "connectivity": 3}]
    (tmp_path / "run.json").write_text(json.dumps(cfg))
    assert ZF.main([str(tmp_path / "run.json"), "--tmp", str(tmp_path)]) == 0
    assert S.read_array(tmp_path / "c").tobytes() == R.apply(v, "uint8", "h_minima", h=1.0,
                                                             connectivity=3).tobytes()
    res = ZF.run(cfg, log=lines.append)
    assert res[0]["rounds"] >= 1 and f"   {res[0]['rounds']} rounds" in lines
    # refusals of the store step: a marker of another shape or type, another output type
    S.create_array(tmp_path / "short", "uint8", (40, 33, 44), CHUNK, fill_value=0)
    with pytest.raises(zt.InvalidParameters, match="Array shapes do not match"):
        S.reconstruction(src, tmp_path / "x", tmp_path / "short")
    S.create_array(tmp_path / "wide", "uint16", SHAPE, CHUNK, fill_value=0)
    with pytest.raises(zt.UnsupportedDataType, match="one data type"):
        S.reconstruction(src, tmp_path / "x", tmp_path / "wide")
    with pytest.raises(zt.UnsupportedDataType, match="the input's data type uint8"):
        S.reconstruction(src, tmp_path / "x", mode="fill_holes", data_type="uint16")
    assert not (tmp_path / "x" / "zarr.json").exists()


def test_skip_empty_chunks(stored, tmp_path):
    src, marker, v, m, refs = stored
    ref = refs["rec2"]
    assert ZF.main(["reconstruction", src, str(tmp_path / "e"), "--marker", marker,
                    "--connectivity", "2", "--skip-empty-chunks"]) == 0
    want = occ_ref.expected_files(ref, CHUNK, 0)
    assert want < occ_ref.all_files(SHAPE, CHUNK)  # the missing chunks stay empty
    assert occ_ref.chunk_files(tmp_path / "e") == want
    assert S.read_array(tmp_path / "e").tobytes() == ref.tobytes()
    assert ZF.main(["reconstruction", src, str(tmp_path / "f"), "--marker", marker,
                    "--connectivity", "2"]) == 0
    assert occ_ref.chunk_files(tmp_path / "f") == occ_ref.all_files(SHAPE, CHUNK)


def test_fill_holes_in_a_device_chain_and_a_named_marker(stored, tmp_path):
    src, marker, v, m, refs = stored
    steps = [{"filter": "equal", "input": src, "value": 1, "output": "$mask"},
             {"filter": "reconstruction", "input": "$mask", "mode": "fill_holes",
              "output": "$filled"},
             {"filter": "connected_components", "input": "$filled", "connectivity": 1,
              "output": str(tmp_path / "chain")}]
    assert ZF.plan_chains(steps) == [(0, 2)]
    lines = []
    res = ZF.run(steps, tmp=str(tmp_path), log=lines.append)
    assert all(st.get("device_resident") for st in res)
    steps[2]["output"] = str(tmp_path / "store")
    res2 = ZF.run(steps, tmp=str(tmp_path), device_chain=False, **QUIET)
    assert not res2[0].get("device_resident")
    filled = R.apply((v == 1).astype(np.uint8), "bool", "fill_holes", connectivity=1)
    assert filled.sum() > (v == 1).sum()  # something was filled
    ref, k_ref = C.connected_components(filled, "bool", 1)
    assert res[2]["components"] == res2[2]["components"] == k_ref
    assert res[1]["rounds"] == res2[1]["rounds"] and f"   {res[1]['rounds']} rounds" in lines
    assert S.read_array(tmp_path / "chain").tobytes() == ref.tobytes()
    assert S.read_array(tmp_path / "store").tobytes() == ref.tobytes()
    # a $name marker produced by an earlier step: it is written to the store, the step that
    # reads it runs store -> store; opening by reconstruction: erode, then rebuild under the input
    steps = [{"filter": "minimum", "input": src, "kernel_half_size": [1, 1, 1],
              "output": "$seeds"},
             {"filter": "reconstruction", "input": src, "marker": "$seeds", "connectivity": 3,
              "output": str(tmp_path / "opened")}]
    assert ZF.plan_chains(steps) == []
    res = ZF.run(steps, tmp=str(tmp_path), **QUIET)
    from tests import rank_ref
    seeds = rank_ref.apply_ndarray(v, "minimum", (1, 1, 1), "uint8")
    ref = R.reconstruct(v, seeds, "uint8", "dilation", 3)
    assert res[1]["rounds"] >= 1
    assert S.read_array(tmp_path / "opened").tobytes() == ref.tobytes()


def test_two_gpus_run_the_step_in_one_process(stored, tmp_path):
    src, marker, v, m, refs = stored
    lines = []
    steps = [{"filter": "reconstruction", "input": src, "mode": "fill_holes",
              "output": str(tmp_path / "two")}]
    res = ZF.run(steps, gpus=2, gpu_devices=[0, 0], log=lines.append)
    assert "processes" not in res[0] and res[0]["rounds"] >= 2
    assert any("reconstruction" in line and "one process on device 0, not 2" in line
               for line in lines)
    assert S.read_array(tmp_path / "two").tobytes() == refs["fill1"].tobytes()


def test_arrays_that_do_not_fit_fail_before_anything_is_read(stored, tmp_path, monkeypatch):
    from zarrs_tools_amd import device_io
    src, marker, v, m, refs = stored
    n = int(np.prod(SHAPE))
    need = zt.Reconstruction().memory("uint8", "uint8", SHAPE)
    assert need == 3 * n + (n + 15) // 16 * 16 + 64

    def no_read(*a, **k):
        raise AssertionError("an array was read")

    monkeypatch.setattr(device_io, "read_to_device", no_read)
    monkeypatch.setenv("ZT_STORE_DEVICE_MEMORY", str(need))  # 80 % of it is too little
    with pytest.raises(zt.FilterError, match="not enough available memory") as e:
        S.reconstruction(src, tmp_path / "out", marker)
    assert e.value.status == _abi.ERR_OUT_OF_MEMORY and "no store -> store path" in str(e.value)
    assert "mask, marker, output and one working array" in str(e.value)
    assert not (tmp_path / "out" / "zarr.json").exists()
    # a generated marker needs one array less
    less = zt.Reconstruction(mode="fill_holes").memory("uint8", "uint8", SHAPE)
    assert less == need - n
    monkeypatch.setenv("ZT_STORE_DEVICE_MEMORY", str(less))
    with pytest.raises(zt.FilterError, match="mask, output and one working array"):
        S.reconstruction(src, tmp_path / "out", mode="fill_holes")
    assert ZF.main(["reconstruction", src, str(tmp_path / "out"), "--fill-holes"]) == 1
    assert not (tmp_path / "out" / "zarr.json").exists()
    # the pinned host buffers are budgeted too: the mask's and the marker's
    monkeypatch.delenv("ZT_STORE_DEVICE_MEMORY")
    monkeypatch.setenv("ZT_STORE_HOST_MEMORY", "10000")
    for args in ((marker,), ()):
        with pytest.raises(zt.FilterError, match="pinned host buffers") as e:
            S.reconstruction(src, tmp_path / "out", *args, mode=None if args else "fill_holes")
        assert e.value.status == _abi.ERR_OUT_OF_MEMORY
    assert not (tmp_path / "out" / "zarr.json").exists()
