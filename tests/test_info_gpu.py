"""GPU: zarrs_info's range and histogram (info.hip through the C ABI, the store path and the
zarrs_info command) against the numpy restatement (tests/info_ref.py). Counts and ranges are
exact: there is no tolerance anywhere.

Borders of the kernels (info.hip): a run is read as the elements before the first 16-byte
boundary (head), aligned 16-byte vectors of PER = 16 / element size elements, and a tail of
fewer than PER elements; a workgroup step is 256 lanes x 4 vectors = STEP_VECS vectors, steps are
grid-strided, ZT_INFO_MAX_BLOCKS caps the grid. Up to K = 4096 bins are privatised in LDS (with
replicas below K / 2; up to 512 bins have 8 or more and take plain adds, above that lanes that
share a bin add once), more go to the global histogram directly."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import info_ref as R
from tests.gpu_util import to_dev
from tests.test_info import HIST_0_49

pytestmark = pytest.mark.gpu

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)
from zarrs_tools_amd import store as S  # noqa: E402
from zarrs_tools_amd import zarrs_info as ZI  # noqa: E402

K = 4096
STEP_VECS = 256 * 4
SIZE = {dt: np.dtype(O.NP_STORAGE[dt]).itemsize for dt in R.NUMERIC}


def per(dt):
    return 16 // SIZE[dt]


def noise(dt, n, seed=0):
    """n storage elements: noise over the type's span with its extremes and, for floats, NaN,
    the infinities and both zeros in it."""
    rng = np.random.default_rng(seed)
    st = O.NP_STORAGE[dt]
    if dt not in R.FLOATS:
        v = rng.integers(0, 256, size=n * SIZE[dt], dtype=np.uint8).view(st).copy()
        special = np.array([np.iinfo(st).min, np.iinfo(st).max, 0], dtype=st)
    else:
        f = (rng.standard_normal(n) * 700.0).astype(np.float32)
        sp = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 3.0e38, -3.0e38], dtype=np.float32)
        if dt == "float16":
            with np.errstate(all="ignore"):
                v = f.astype(np.float16).view(np.uint16)
                special = sp.astype(np.float16).view(np.uint16)
        elif dt == "bfloat16":
            v = (f.view(np.uint32) >> 16).astype(np.uint16)
            special = (sp.view(np.uint32) >> 16).astype(np.uint16)
        else:
            with np.errstate(all="ignore"):
                v, special = f.astype(st), sp.astype(st)
        v = v.copy()
    if n >= 4 * len(special):
        pos = rng.choice(n, size=len(special), replace=False)
        v[pos] = special
    return v


def hist_args(dt):
    """(min, max) of a histogram that leaves part of the noise outside on both sides."""
    if dt in R.FLOATS:
        return -1000.0, 1500.0
    info = np.iinfo(O.NP_STORAGE[dt])
    return float(info.min) / 2 + 3.0, float(info.max) / 2


def dev(v, dt, offset=0):
    """v on the device; offset > 0: a view that starts `offset` elements past an aligned base."""
    if offset == 0:
        return to_dev(v, dt)
    pad = np.zeros(offset, dtype=v.dtype)
    return to_dev(np.concatenate([pad, v]), dt)[offset:]


def check_range(t, v, dt):
    got, want = zt.Range().apply_ndarray(t), R.range_(v, dt)
    assert R.same_value(got[0], want[0]) and R.same_value(got[1], want[1]), (dt, got, want)


def check_hist(t, v, dt, n_bins, mn, mx):
    edges, hist = zt.Histogram(n_bins, mn, mx).apply_ndarray(t)
    redges, rhist = R.histogram(v, dt, n_bins, mn, mx)
    assert hist.dtype == np.uint64 and hist.shape == (n_bins,)
    assert int(hist.sum()) == v.size
    bad = np.flatnonzero(hist != rhist)
    assert bad.size == 0, (dt, n_bins, bad[:8], hist[bad[:8]], rhist[bad[:8]])
    assert edges.tobytes() == redges.tobytes()


# ---- every type -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", R.NUMERIC)
def test_all_types(dt):
    v = noise(dt, 7 * 33 * 70, 1).reshape(7, 33, 70)
    t = dev(v, dt)
    check_range(t, v, dt)
    mn, mx = hist_args(dt)
    for n_bins in (256, K + 1):  # LDS bins, global bins
        check_hist(t, v, dt, n_bins, mn, mx)
    check_range(zt.DeviceArray(t, (4, 16, 32)), v, dt)
    check_hist(zt.DeviceArray(t, (4, 16, 32)), v, dt, 7, mn, mx)


def test_bool_is_unsupported():
    import torch
    t = torch.zeros(64, dtype=torch.bool, device="cuda")
    with pytest.raises(zt.UnsupportedDataType):
        zt.Range().apply_ndarray(t)
    with pytest.raises(zt.UnsupportedDataType):
        zt.Histogram(2, 0.0, 1.0).apply_ndarray(t)


# ---- lengths around the kernel's borders ------------------------------------------------------------

@pytest.mark.parametrize("dt", ["uint8", "int16", "float32", "float64"])
def test_lengths_and_misaligned_base(dt):
    p, step = per(dt), STEP_VECS * per(dt)
    mn, mx = hist_args(dt)
    for n in (0, 1, p - 1, p, p + 1, 2 * p + 1, step - 1, step, step + 1):
        v = noise(dt, n, 10 + n % 7)
        for offset in (0, 1):  # offset 1: the base one element past a 16-byte boundary
            t = dev(v, dt, offset)
            assert offset == 0 or n == 0 or t.data_ptr() % 16 == SIZE[dt] % 16
            check_range(t, v, dt)
            check_hist(t, v, dt, 64, mn, mx)
    # every head length
    v = noise(dt, 3 * p + 5, 3)
    for offset in range(2, p):
        t = dev(v, dt, offset)
        check_range(t, v, dt)
        check_hist(t, v, dt, K + 7, mn, mx)


@pytest.mark.parametrize("dt", ["uint8", "uint16", "float32", "int64"])
def test_grid_stride_second_trip(monkeypatch, dt):
    # two workgroups: two steps per trip of the grid-stride loop; 2.5 trips and a tail
    monkeypatch.setenv("ZT_INFO_MAX_BLOCKS", "2")
    n = 5 * STEP_VECS * per(dt) + 5
    v = noise(dt, n, 4)
    t = dev(v, dt, 1)
    mn, mx = hist_args(dt)
    check_range(t, v, dt)
    check_hist(t, v, dt, 100, mn, mx)
    check_hist(t, v, dt, K + 1, mn, mx)


# ---- bin counts ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_bins", [1, 2, 3, 255, 256, K, K + 1, 5000])
def test_bin_counts(n_bins):
    for dt in ("uint16", "float32"):
        v = noise(dt, 20011, 5)
        mn, mx = hist_args(dt)
        check_hist(dev(v, dt), v, dt, n_bins, mn, mx)


def test_max_equals_min_and_reversed():
    v = np.array([1.0, 2.0, 3.0, 2.0, np.nan] * 13, dtype=np.float64)
    check_hist(dev(v, "float64"), v, "float64", 5, 2.0, 2.0)
    check_hist(dev(v, "float64"), v, "float64", 5, 3.0, 1.0)
    u = np.array([2**53 + 1, 2**64 - 1, 2**63, 0] * 5, dtype=np.uint64)
    check_hist(dev(u, "uint64"), u, "uint64", 4, 0.0, 2.0**64)
    check_range(dev(u, "uint64"), u, "uint64")
    i = np.array([-2**63, 2**63 - 1, -2**53 - 1, 2**53 + 1] * 5, dtype=np.int64)
    check_hist(dev(i, "int64"), i, "int64", 6, -2.0**63, 2.0**63)
    check_range(dev(i, "int64"), i, "int64")


# ---- one bin takes (nearly) everything ------------------------------------------------------------------

@pytest.mark.parametrize("dt,value", [("uint8", 17), ("uint16", 40000), ("float32", 12.5)])
def test_constant_array(dt, value):
    n = 1 << 20  # every wave uniform: one lane adds the count; one bin far past 2^16
    v = np.full(n, value, dtype=O.NP_STORAGE[dt])
    t = dev(v, dt)
    for n_bins in (1, 16, K + 1):
        check_hist(t, v, dt, n_bins, 0.0, 65535.0)
    check_range(t, v, dt)


@pytest.mark.parametrize("dt", ["uint8", "uint16", "float32"])
def test_ninety_percent_constant(dt):
    n = 1 << 19
    rng = np.random.default_rng(6)
    # scattered: 90 % of the elements one value, no wave uniform
    v = noise(dt, n, 7)
    const = np.full(1, 40, dtype=O.NP_STORAGE[dt]) if dt != "float32" else np.float32([40.0])
    v[rng.random(n) < 0.9] = const[0]
    mn, mx = (0.0, 255.0) if dt == "uint8" else (0.0, 65535.0) if dt == "uint16" else (
        -1000.0, 1500.0)
    check_hist(dev(v, dt), v, dt, 256, mn, mx)
    # a constant background with noise behind it: uniform waves, mixed waves and noise waves
    w = noise(dt, n, 8)
    w[: n * 9 // 10 + 3] = const[0]
    check_hist(dev(w, dt, 1), w, dt, 256, mn, mx)
    for n_bins in (512, 513, K, K + 1):  # 8 replicas: plain adds; fewer, and global: leader rounds
        check_hist(dev(w, dt), w, dt, n_bins, mn, mx)
        check_hist(dev(v, dt), v, dt, n_bins, mn, mx)


# ---- the division is the IEEE one -------------------------------------------------------------------

def test_division_anchors():
    v = np.tile(np.arange(50, dtype=np.uint8), 100)
    _, hist = zt.Histogram(49, 0.0, 49.0).apply_ndarray(dev(v, "uint8"))
    assert hist.tolist() == [100 * h for h in HIST_0_49]
    for dt in ("uint8", "int16", "uint32", "float32", "float64", "int64"):
        w = np.tile(np.arange(50), 100).astype(O.NP_STORAGE[dt])
        _, hist = zt.Histogram(49, 0.0, 49.0).apply_ndarray(dev(w, dt, 1))
        assert hist.tolist() == [100 * h for h in HIST_0_49], dt
    v = np.tile(np.arange(256, dtype=np.uint8), 20)
    check_hist(dev(v, "uint8"), v, "uint8", 255, 0.0, 255.0)
    w = np.tile(np.arange(256, dtype=np.uint16), 20)
    check_hist(dev(w, "uint16"), w, "uint16", 255, 0.0, 255.0)


# ---- accumulation -----------------------------------------------------------------------------------

def test_accumulation_across_calls():
    dt = "float32"
    v = noise(dt, 30001, 9)
    a, b = v[:12345], v[12345:]
    mn, mx = hist_args(dt)
    h = zt.Histogram(300, mn, mx)
    state = h.new_state()
    h.accumulate(dev(a, dt), state)
    h.accumulate(dev(b, dt, 1), state)
    h.accumulate(dev(v[:0], dt), state)  # n == 0: a no-op
    _, hist = h.finish(state)
    assert np.array_equal(hist, R.histogram(v, dt, 300, mn, mx)[1])
    r = zt.Range()
    rs = r.new_state()
    assert r.finish(rs, dt) == (None, None)
    r.accumulate(dev(np.full(777, np.nan, np.float32), dt), rs)
    assert r.finish(rs, dt) == (None, None)  # NaN only: still none
    r.accumulate(dev(a, dt), rs)
    r.accumulate(dev(b, dt, 1), rs)
    got, want = r.finish(rs, dt), R.range_(v, dt)
    assert R.same_value(got[0], want[0]) and R.same_value(got[1], want[1])
    # the zeros' order does not depend on which call saw which
    for first, second in ((0.0, -0.0), (-0.0, 0.0)):
        rs = r.new_state()
        r.accumulate(dev(np.float32([first]), dt), rs)
        r.accumulate(dev(np.float32([second]), dt), rs)
        lo, hi = r.finish(rs, dt)
        assert R.same_value(lo, -0.0) and R.same_value(hi, 0.0)
    assert zt.Range().apply_ndarray(dev(np.full(100, np.nan, np.float64), "float64")) == (
        None, None)


def test_device_resident_chain():
    v = noise("uint16", 9 * 31 * 65, 11).reshape(9, 31, 65)
    y = zt.Rescale(0.01275, 0.0).apply_ndarray(dev(v, "uint16"), dtype_out="uint8")
    assert y.is_cuda
    edges, hist = zt.Histogram(32, 0.0, 255.0).apply_ndarray(y)
    y_host = y.cpu().numpy()
    assert np.array_equal(hist, R.histogram(y_host, "uint8", 32, 0.0, 255.0)[1])
    assert zt.Range().apply_ndarray(y) == R.range_(y_host, "uint8")


# ---- the store path ---------------------------------------------------------------------------------

SHAPE, CHUNK = (40, 33, 70), (16, 16, 32)  # every axis overhangs its last chunk


@pytest.fixture(scope="module")
def u16_data():
    return noise("uint16", int(np.prod(SHAPE)), 12).reshape(SHAPE)


def make_store(path, data, dt="uint16", **kw):
    S.create_array(path, dt, data.shape, CHUNK[-data.ndim:], S.codecs_json(**kw.pop("codecs", {})),
                   **kw)
    S.write_array(path, data)
    return path


def check_store(path, data, dt="uint16", n_bins=300, mn=100.0, mx=60000.0):
    stats = {}
    assert S.range(path, stats=stats) == R.range_(data, dt)
    assert stats["voxels"] == data.size and stats["rows"] == -(-data.shape[0] // CHUNK[0])
    edges, hist = S.histogram(path, n_bins, mn, mx, stats=stats)
    redges, rhist = R.histogram(data, dt, n_bins, mn, mx)
    assert int(hist.sum()) == data.size and stats["voxels"] == data.size
    assert np.array_equal(hist, rhist) and edges.tobytes() == redges.tobytes()


def test_store_overhanging_chunks(tmp_path, u16_data):
    p = make_store(tmp_path / "a.zarr", u16_data)
    check_store(p, u16_data)
    check_store(p, u16_data, n_bins=K + 5)
    steps = []
    S.set_progress_callback(lambda s: steps.append((s["step"], s["num_steps"])))
    try:
        S.range(p, chunk_limit=2)
    finally:
        S.set_progress_callback(None)
    assert sorted(s for s, _ in steps) == list(range(1, 28)) and {t for _, t in steps} == {27}


def test_store_missing_chunk_counts_as_fill(tmp_path, u16_data):
    p = make_store(tmp_path / "m.zarr", u16_data, fill_value=1234)
    os.remove(p / "c" / "1" / "1" / "1")
    want = u16_data.copy()
    want[16:32, 16:32, 32:64] = 1234
    check_store(p, want)
    edges, hist = S.histogram(p, 65536, 0.0, 65536.0)
    assert hist[1234] == np.count_nonzero(want == 1234) >= 16 * 16 * 32


@pytest.mark.parametrize("codecs", [dict(compression="gzip", level=1),
                                    dict(shard_inner=(8, 8, 16))], ids=["gzip", "sharded"])
def test_store_codecs(tmp_path, u16_data, codecs):
    check_store(make_store(tmp_path / "c.zarr", u16_data, codecs=codecs), u16_data)


def test_store_rows_combine(tmp_path, u16_data):
    p = make_store(tmp_path / "r.zarr", u16_data)
    parts_r, parts_h = [], []
    for r in range(3):
        parts_r.append(S.range(p, rows=(r, r + 1)))
        parts_h.append(S.histogram(p, 77, 0.0, 65535.0, rows=(r, r + 1)))
        rows = u16_data[16 * r: 16 * (r + 1)]
        assert parts_r[-1] == R.range_(rows, "uint16")
        assert int(parts_h[-1][1].sum()) == rows.size
    assert zt.combine_ranges(parts_r) == S.range(p) == R.range_(u16_data, "uint16")
    edges, hist = zt.combine_histograms(parts_h)
    whole = S.histogram(p, 77, 0.0, 65535.0)
    assert np.array_equal(hist, whole[1]) and np.array_equal(edges, whole[0])
    assert np.array_equal(hist, R.histogram(u16_data, "uint16", 77, 0.0, 65535.0)[1])
    assert S.range(p, rows=(3, 5)) == (None, None)  # no such rows


def test_store_cli(tmp_path, u16_data, capsys):
    p = make_store(tmp_path / "cli.zarr", u16_data)
    assert ZI.main([str(p), "range"]) == 0
    out = json.loads(capsys.readouterr().out)
    lo, hi = R.range_(u16_data, "uint16")
    assert out == {"min": lo, "max": hi}
    assert ZI.main(["--chunk-limit", "3", str(p), "histogram", "16", "0", "65535"]) == 0
    out = json.loads(capsys.readouterr().out)
    redges, rhist = R.histogram(u16_data, "uint16", 16, 0.0, 65535.0)
    assert out == {"bin_edges": redges.tolist(), "hist": rhist.tolist()}
    assert sum(out["hist"]) == 40 * 33 * 70


def test_store_cli_float_values(tmp_path, capsys):
    data = noise("float32", 20 * 19, 13).reshape(20, 19)
    finite = np.where(np.isfinite(data), data, np.float32(1.5)).astype(np.float32)
    finite[3, 4], finite[5, 6] = np.nan, -0.0
    p = tmp_path / "f.zarr"
    S.create_array(p, "float32", finite.shape, (16, 16))
    S.write_array(p, finite)
    assert ZI.main([str(p), "range"]) == 0
    lo, hi = R.range_(finite, "float32")
    assert json.loads(capsys.readouterr().out) == {"min": lo, "max": hi}
    q = tmp_path / "g.zarr"
    S.create_array(q, "float32", data.shape, (16, 16))
    S.write_array(q, data)
    assert ZI.main([str(q), "range"]) == 0
    assert json.loads(capsys.readouterr().out) == {"min": "-Infinity", "max": "Infinity"}
    n = tmp_path / "n.zarr"
    S.create_array(n, "float32", (4, 4), (2, 2), fill_value="NaN")
    assert ZI.main([str(n), "range"]) == 0
    assert json.loads(capsys.readouterr().out) == {"min": None, "max": None}
