"""GPU parity of the rank filters (rank.hip through the C ABI) against the numpy restatement
(tests/rank_ref.py): equality of storage bytes everywhere. The filters select an element and
never compute one, so no NaN is generated and no position is exempt."""
import itertools
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import pw_ref
from tests import rank_ref as R
from tests.gpu_util import from_dev, to_dev

pytestmark = pytest.mark.gpu

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)
from zarrs_tools_amd import store as S  # noqa: E402
from zarrs_tools_amd import zarrs_filter as ZF  # noqa: E402

KINDS = R.KINDS
QUIET = {"log": lambda *_: None}


def gpu_rank(v, kind, half, din, dout=None, chunk=None):
    import torch
    dout = dout or din
    x = to_dev(v, din)
    y = torch.empty(v.shape, dtype=zt.torch_dtype(dout), device="cuda")
    chunk = chunk or v.shape
    zt.RankFilter(kind, half).apply(zt.DeviceArray(x, chunk, din), zt.DeviceArray(y, chunk, dout))
    torch.cuda.synchronize()
    return from_dev(y, dout)


def gpu_rank_block(v, kind, half, din, start, shape):
    import torch
    out = zt.RankFilter(kind, half).apply_ndarray(to_dev(v, din), zt.ArraySubset(start, shape))
    torch.cuda.synchronize()
    return from_dev(out, din)


def assert_same_bytes(out, ref):
    assert out.shape == ref.shape and out.dtype == ref.dtype, (out.shape, ref.shape, out.dtype)
    assert np.array_equal(np.ascontiguousarray(out).view(np.uint8),
                          np.ascontiguousarray(ref).view(np.uint8))


def noise(shape, seed=0):
    rng = np.random.default_rng(sum(shape) + seed)
    return (rng.random(shape, dtype=np.float32) * 1000 - 200).astype(np.float32)


# The fused 3-D march (rank3_kernel, 32 x 64 tiles), the shapes of test_fused_sobel_3d_bit_exact
# for its reasons: unit extents on each axis, extent 2, x below a tile and no multiple of 4, tile
# borders in y and x, a ragged last tile, and 101 output slices: 4 z segments, each priming its
# own ring.
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [
    (1, 5, 9), (5, 1, 9), (5, 9, 1), (1, 1, 1), (2, 2, 2), (7, 33, 67),
    (9, 40, 128), (5, 70, 132), (5, 70, 131), (101, 9, 20),
])
def test_fused_3d_bit_exact(shape, kind):
    v = noise(shape)
    assert_same_bytes(gpu_rank(v, kind, (1, 1, 1), "float32"),
                      R.apply_ndarray(v, kind, (1, 1, 1), "float32"))


@pytest.mark.parametrize("shape", [(5, 9, 20), (9, 40, 128)])
def test_ties(shape):
    rng = np.random.default_rng(11)
    v = rng.integers(0, 4, shape).astype(np.uint8)
    k = np.pad(v, 1, mode="edge")
    win = np.lib.stride_tricks.sliding_window_view(k, (3, 3, 3)).reshape(shape + (27,))
    for kind in KINDS:
        out = gpu_rank(v, kind, (1, 1, 1), "uint8")
        assert_same_bytes(out, R.apply_ndarray(v, kind, (1, 1, 1), "uint8"))
        assert (win == out[..., None]).any(axis=-1).all()  # every output occurs in its window
        if kind == "median":
            assert (out != v).mean() > 0.3  # the filter does something on such data


def _typed_values(din, shape, rng):
    """Values of din (storage) for the all-types test: negatives for the signed types, and for
    the 64-bit types neighbours that differ only below bit 32 or only above it."""
    st = O.NP_STORAGE[din]
    n = int(np.prod(shape))
    if din == "bool":
        return rng.integers(0, 2, shape).astype(st)
    if np.dtype(st).itemsize == 8:
        hi = rng.integers(0, 3, n).astype(np.uint64)
        lo = rng.integers(0, 3, n).astype(np.uint64) * np.uint64(0x01000001)
        if din == "float64":  # exponents around 1.0, both signs
            sign = rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63)
            bits = sign | ((np.uint64(0x3FF00000) + hi) << np.uint64(32)) | lo
        elif din == "int64":  # around zero: ... -2^32, -1, 0, 2^32 ...
            bits = ((hi - np.uint64(1)) << np.uint64(32)) + lo - np.uint64(0x01000001)
        else:
            bits = ((hi + np.uint64(0x7FFFFFFF)) << np.uint64(32)) | lo  # across bit 63
        return bits.view(st).reshape(shape)
    if din in R.FLOATS:
        return O.cast_from_f32((rng.random(shape, dtype=np.float32) * 200 - 100), din)
    ii = np.iinfo(st)
    return rng.integers(ii.min, ii.max, shape, dtype=st, endpoint=True)


@pytest.mark.parametrize("din", list(O.DTYPES))
def test_all_input_types(din):
    shape, chunk = (6, 11, 40), (4, 8, 16)
    v = _typed_values(din, shape, np.random.default_rng(3))
    if din in R.SIGNED:
        assert (v < 0).any() and (v > 0).any()
    if din in R.FLOATS:
        assert (O.cast_to_f32(v, din) < 0).any() if din != "float64" else (v < 0).any()
    if np.dtype(O.NP_STORAGE[din]).itemsize == 8:
        b = v.view(np.uint64).reshape(-1)
        d = b[1:] ^ b[:-1]
        assert ((d != 0) & (d >> np.uint64(32) == 0)).any()         # only below bit 32
        assert ((d != 0) & (d & np.uint64(0xFFFFFFFF) == 0)).any()  # only above
    for kind in KINDS:
        assert_same_bytes(gpu_rank(v, kind, (1, 1, 1), din, chunk=chunk),
                          R.apply_ndarray(v, kind, (1, 1, 1), din))
    # and through the generic kernels
    for kind in KINDS:
        assert_same_bytes(gpu_rank(v, kind, (1, 0, 2), din, chunk=chunk),
                          R.apply_ndarray(v, kind, (1, 0, 2), din))


@pytest.mark.parametrize("dout", list(O.DTYPES))
def test_all_output_types(dout):
    rng = np.random.default_rng(4)
    # a ramp along x from -200000 to 200000 under noise, so that the selected elements keep the
    # range; the first columns scaled to values around the 8-bit ranges
    v = (np.linspace(-200000, 200000, 40, dtype=np.float32)
         + rng.random((6, 11, 40), dtype=np.float32) * 300).astype(np.float32)
    v[:, :, :10] /= np.float32(1000)
    for kind in KINDS:
        ref = R.apply_whole(v, kind, (1, 1, 1), "float32", dout)
        sel = R.apply_ndarray(v, kind, (1, 1, 1), "float32")
        assert sel.max() > 65536 and sel.min() < -65536 and (np.abs(sel) < 256).any()
        assert_same_bytes(gpu_rank(v, kind, (1, 1, 1), "float32", dout, chunk=(4, 8, 16)), ref)


@pytest.mark.parametrize("din", ["float32", "float16"])
def test_special_values(din):
    rng = np.random.default_rng(9)
    shape = (8, 12, 40)
    v = O.cast_from_f32((rng.random(shape, dtype=np.float32) * 10 - 5).astype(np.float32), din)
    u = v.view(np.uint32 if din == "float32" else np.uint16)
    if din == "float32":
        pnan, nnan, pinf, ninf, nz = 0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x80000000
        sub = [0x00000001, 0x80000007, 0x007FFFFF]
    else:
        pnan, nnan, pinf, ninf, nz = 0x7E00, 0xFE00, 0x7C00, 0xFC00, 0x8000
        sub = [0x0001, 0x8007, 0x03FF]
    u[1, 2, 3] = pnan | 0x11          # NaNs with distinct payloads, some of them neighbours
    u[1, 2, 4] = pnan | 0x12
    u[1, 3, 3] = nnan | 0x13
    u[5, 9, 6] = nnan | 0x21
    u[5, 9, 30] = pnan | 0x22         # an isolated +NaN
    u[0, 0, 0] = pnan | 0x23          # in a corner: replicated by the clamp
    u[3, 6, 12] = pinf
    u[3, 6, 13] = ninf
    u[6, 3, 16:22] = [0, nz, nz, 0, 0, nz]  # +-0.0 next to each other
    u[6, 4, 16:22] = [nz, 0, 0, nz, nz, 0]
    u[7, 4, 16:22] = 0
    u[2, 8, 30:33] = sub              # subnormals
    u[2, 7, 30:33] = sub[::-1]
    for kind in KINDS:
        ref = R.apply_ndarray(v, kind, (1, 1, 1), din)
        assert_same_bytes(gpu_rank(v, kind, (1, 1, 1), din), ref)
        assert_same_bytes(gpu_rank(v, kind, (1, 2, 0), din), R.apply_ndarray(v, kind, (1, 2, 0), din))
    mx = R.apply_ndarray(v, "maximum", (1, 1, 1), din).view(u.dtype)
    assert (mx[4:7, 8:11, 29:32] == (pnan | 0x22)).all()  # a +NaN dilates
    md = R.apply_ndarray(v, "median", (1, 1, 1), din).view(u.dtype)
    assert md[5, 9, 30] != (pnan | 0x22)                  # and disappears under the median


# The generic kernels: per-axis minimum / maximum passes and the bisecting median, every rank.
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,half", [
    ((300,), (7,)),
    ((33, 70), (2, 1)),
    ((33, 70), (0, 3)),
    ((7, 33, 67), (2, 1, 1)),
    ((7, 33, 67), (0, 0, 0)),
    ((6, 7, 8, 9), (1, 0, 1, 2)),
    ((3, 4, 3, 5, 6), (1, 1, 0, 1, 1)),
])
def test_generic_paths_bit_exact(shape, half, kind):
    v = noise(shape)
    assert_same_bytes(gpu_rank(v, kind, half, "float32"), R.apply_ndarray(v, kind, half, "float32"))
    w = np.random.default_rng(len(shape)).integers(-3, 4, shape).astype(np.int16)  # ties
    assert_same_bytes(gpu_rank(w, kind, half, "int16"), R.apply_ndarray(w, kind, half, "int16"))


def test_median_window_wider_than_the_extent_1d():
    v = noise((200,))
    assert_same_bytes(gpu_rank(v, "median", (40,), "float32"),
                      R.apply_ndarray(v, "median", (40,), "float32"))
    s = noise((30,), 1)  # the window (81) holds more replicated edges than elements
    for kind in KINDS:
        assert_same_bytes(gpu_rank(s, kind, (40,), "float32"),
                          R.apply_ndarray(s, kind, (40,), "float32"))


# An interior output region of a block: misaligned, and aligned to quads (x origin 8); through
# the fused march and through the generic kernels.
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("half", [(1, 1, 1), (2, 1, 0)])
@pytest.mark.parametrize("block,start,shape", [
    ((10, 20, 41), (1, 1, 1), (8, 18, 39)),
    ((6, 24, 72), (0, 4, 8), (6, 16, 64)),
])
def test_apply_ndarray_interior_subset(block, start, shape, half, kind):
    v = noise(block)
    ref = R.apply_ndarray(v, kind, half, "float32", (start, shape))
    assert_same_bytes(gpu_rank_block(v, kind, half, "float32", start, shape), ref)


@pytest.mark.parametrize("kind", KINDS)
def test_per_chunk_path_equals_apply(kind):
    import torch
    v = O.synth_step_noise_f32((14, 30, 50))
    chunk = (5, 16, 20)
    x = to_dev(v, "float32")
    y = torch.empty(v.shape, device="cuda")
    a_in, a_out = zt.DeviceArray(x, chunk), zt.DeviceArray(y, chunk)
    f = zt.RankFilter(kind, (1, 1, 1))
    for idx in itertools.product(*[range(n) for n in a_out.chunk_grid_shape()]):
        f.apply_chunk(a_in, a_out, idx)
    torch.cuda.synchronize()
    whole = gpu_rank(v, kind, (1, 1, 1), "float32", chunk=chunk)
    assert_same_bytes(from_dev(y, "float32"), whole)
    assert_same_bytes(whole, R.apply_chunks(v, chunk, kind, (1, 1, 1), "float32"))


@pytest.mark.parametrize("kind", KINDS)
def test_store_rank_filter(tmp_path, kind):
    shape, chunk = (20, 33, 70), (8, 16, 32)
    u = O.synth_u16(shape)
    S.create_array(tmp_path / "in.zarr", "uint16", shape, chunk, S.codecs_json("gzip"))
    S.write_array(tmp_path / "in.zarr", u)
    st = S.rank_filter(tmp_path / "in.zarr", tmp_path / "out.zarr", kind, (1, 1, 1))
    ref = R.apply_whole(u, kind, (1, 1, 1), "uint16")
    whole = S.read_array(tmp_path / "out.zarr")
    assert_same_bytes(whole, ref)
    assert st["voxels"] == u.size
    # another output type, and a halo of 2 on axis 0 through the generic kernels
    S.rank_filter(tmp_path / "in.zarr", tmp_path / "f32.zarr", kind, (2, 0, 1),
                  data_type="float32")
    assert_same_bytes(S.read_array(tmp_path / "f32.zarr"),
                      R.apply_whole(u, kind, (2, 0, 1), "uint16", "float32"))
    # two "ranks": chunk rows [0, 1) and [1, 3), the second one finishes the metadata
    S.rank_filter(tmp_path / "in.zarr", tmp_path / "rows.zarr", kind, (1, 1, 1), rows=(0, 1),
                  finish=False)
    assert not (tmp_path / "rows.zarr" / "zarr.json").exists()  # "not finished" marker
    S.rank_filter(tmp_path / "in.zarr", tmp_path / "rows.zarr", kind, (1, 1, 1), rows=(1, 3),
                  erase=False)
    meta = json.load(open(tmp_path / "rows.zarr" / "zarr.json"))
    assert meta["data_type"] == "uint16" and meta["shape"] == list(shape)
    assert_same_bytes(S.read_array(tmp_path / "rows.zarr"), ref)


def test_store_skip_empty_chunks(tmp_path):
    shape, chunk = (20, 33, 70), (8, 16, 32)
    u = O.synth_u16(shape)
    u[:8] = 0  # the first chunk row is the fill value
    src, full, el = (str(tmp_path / n) for n in ("in.zarr", "full.zarr", "el.zarr"))
    S.create_array(src, "uint16", shape, chunk, S.codecs_json("gzip"))
    S.write_array(src, u)
    ref = R.apply_whole(u, "median", (1, 1, 1), "uint16")
    assert not ref[:8].any() and ref[8:].any()  # 18 of plane 7's 27 window entries are zero
    assert ZF.main(["median", src, full, "1,1,1"]) == 0
    assert ZF.main(["median", src, el, "1,1,1", "--skip-empty-chunks"]) == 0
    assert S.store_empty_chunks() is True
    assert_same_bytes(S.read_array(full), ref)
    assert_same_bytes(S.read_array(el), ref)
    assert os.path.isdir(os.path.join(full, "c", "0")) and not os.path.exists(
        os.path.join(el, "c", "0"))
    assert os.path.isdir(os.path.join(el, "c", "1"))


def test_store_step_split_over_processes(tmp_path):
    """zarrs_filter --gpus 2 (rehearsed with both processes on device 0): the chunk rows of a
    rank step split over two processes, each reading its rows plus the halo, give the whole
    array's result, and zarr.json is written once at the end."""
    shape, chunk = (20, 33, 70), (8, 16, 32)
    u = O.synth_u16(shape)
    S.create_array(tmp_path / "in.zarr", "uint16", shape, chunk)
    S.write_array(tmp_path / "in.zarr", u)
    res = ZF.run([{"filter": "median", "input": str(tmp_path / "in.zarr"),
                   "output": str(tmp_path / "out.zarr"), "kernel_half_size": [2, 1, 1]}],
                 gpus=2, gpu_devices=[0, 0], **QUIET)
    assert res[0].get("processes") == 2
    assert_same_bytes(S.read_array(tmp_path / "out.zarr"),
                      R.apply_whole(u, "median", (2, 1, 1), "uint16"))


def test_cli_median_subcommand(tmp_path):
    shape, chunk = (12, 20, 33), (8, 16, 16)
    v = O.synth_step_noise_f32(shape)
    S.create_array(tmp_path / "in.zarr", "float32", shape, chunk)
    S.write_array(tmp_path / "in.zarr", v)
    rc = ZF.main(["median", str(tmp_path / "in.zarr"), str(tmp_path / "out.zarr"), "1,2,0",
                  "--data-type", "int16"])
    assert rc == 0
    assert_same_bytes(S.read_array(tmp_path / "out.zarr"),
                      R.apply_whole(v, "median", (1, 2, 0), "float32", "int16"))


def test_run_config_chain_device_resident_equals_store_path(tmp_path):
    shape, chunk = (24, 30, 40), (8, 16, 16)
    v = O.synth_step_noise_f32(shape)
    src = str(tmp_path / "in.zarr")
    S.create_array(src, "float32", shape, chunk)
    S.write_array(src, v)

    def steps(out):
        return [{"filter": "gaussian", "input": src, "output": "$g", "sigma": [1.0, 1.0, 1.0],
                 "kernel_half_size": [2, 2, 2]},
                {"filter": "median", "input": "$g", "output": "$m", "kernel_half_size": [1, 1, 1]},
                {"filter": "clamp", "input": "$m", "output": out, "min": 50.0, "max": 550.0}]
    dev_out, store_out = str(tmp_path / "dev.zarr"), str(tmp_path / "store.zarr")
    res = ZF.run(steps(dev_out), tmp=str(tmp_path), **QUIET)
    assert len(res) == 3 and all(r.get("device_resident") for r in res)
    res = ZF.run(steps(store_out), tmp=str(tmp_path), device_chain=False, **QUIET)
    assert not any(r.get("device_resident") for r in res)
    a, b = S.read_array(dev_out), S.read_array(store_out)
    assert_same_bytes(a, b)
    assert S.compare(dev_out, store_out) == (0, None)
    assert S.open_array(dev_out).metadata == S.open_array(store_out).metadata
    g = O.gaussian_apply(v, chunk, [1.0] * 3, [2] * 3)
    want = pw_ref.clamp(R.apply_ndarray(g, "median", (1, 1, 1), "float32"), "float32", 50.0, 550.0)
    assert (want == 50.0).any() and (want == 550.0).any()
    assert_same_bytes(a, want)
    assert sorted(os.listdir(tmp_path)) == ["dev.zarr", "in.zarr", "store.zarr"]
