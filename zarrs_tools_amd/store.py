"""Zarr V3 filesystem arrays and the store -> store filters (host side of the C ABI).

Mirrors what the reference does through zarrs (0.20.0-beta.2): ``load_array`` / ``create_array``
in src/bin/zarrs_filter.rs:63-87, the filters' ``apply`` over Array<FilesystemStore>
(guided_filter.rs:240-319, downsample.rs:170-286) and zarrs_ome's level loop
(zarrs_ome.rs:515-738). All I/O and compute run in libzarrs_tools_amd.so; this module only
marshals arguments (numpy is used for host buffers in tests and tools).
"""
from __future__ import annotations

import ctypes
import json
import os
import threading
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _abi
from ._abi import DTYPES, DTYPE_NAMES, check, i64_array, lib

NUMPY = {
    "bool": np.bool_, "int8": np.int8, "int16": np.int16, "int32": np.int32, "int64": np.int64,
    "uint8": np.uint8, "uint16": np.uint16, "uint32": np.uint32, "uint64": np.uint64,
    "bfloat16": np.uint16, "float16": np.float16, "float32": np.float32, "float64": np.float64,
}

SYNTH_STEP_NOISE_F32 = 0
SYNTH_U16 = 1
SEED = 0x5EED2025


def _b(path) -> bytes:
    return os.fspath(path).encode()


def _dt(dtype) -> int:
    if dtype is None:
        return -1
    if isinstance(dtype, int):
        return dtype
    if dtype not in DTYPES:
        raise _abi.UnsupportedDataType(_abi.ERR_UNSUPPORTED_DATA_TYPE,
                                       f"unsupported data type {dtype}")
    return DTYPES[dtype]


@dataclass
class ArrayInfo:
    path: str
    data_type: str
    shape: tuple
    chunk_shape: tuple
    inner_chunk_shape: tuple

    @property
    def ndim(self) -> int:
        return len(self.shape)

    @property
    def metadata(self) -> dict:
        with open(os.path.join(self.path, "zarr.json")) as f:
            return json.load(f)


def open_array(path) -> ArrayInfo:
    """Array::open on a filesystem store (zarr.json V3)."""
    dt, nd = ctypes.c_int(), ctypes.c_int()
    shp, ch, inner = (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 8)()
    check(lib().zt_store_array_info(_b(path), ctypes.byref(dt), ctypes.byref(nd), shp, ch, inner))
    n = nd.value
    return ArrayInfo(os.fspath(path), DTYPE_NAMES[dt.value], tuple(shp[:n]), tuple(ch[:n]),
                     tuple(inner[:n]))


def codecs_json(compression: Optional[str] = None, level: int = 1,
                shard_inner: Optional[Sequence[int]] = None) -> Optional[str]:
    """A Zarr V3 codec list: bytes (+ gzip/zstd), optionally inside sharding_indexed."""
    chain = [{"name": "bytes", "configuration": {"endian": "little"}}]
    if compression == "gzip":
        chain.append({"name": "gzip", "configuration": {"level": int(level)}})
    elif compression == "zstd":
        chain.append({"name": "zstd", "configuration": {"level": int(level), "checksum": False}})
    elif compression not in (None, "none"):
        raise ValueError(f"unknown compression {compression}")
    if shard_inner is not None:
        chain = [{"name": "sharding_indexed", "configuration": {
            "chunk_shape": [int(c) for c in shard_inner], "codecs": chain,
            "index_codecs": [{"name": "bytes", "configuration": {"endian": "little"}},
                             {"name": "crc32c"}],
            "index_location": "end"}}]
    return json.dumps(chain)


def create_array(path, data_type: str, shape, chunk_shape, codecs: Optional[str] = None,
                 fill_value=None) -> ArrayInfo:
    """ArrayBuilder::build + store_metadata for a filesystem store."""
    shape = [int(s) for s in shape]
    fv = None if fill_value is None else json.dumps(fill_value).encode()
    check(lib().zt_store_create_array(_b(path), _dt(data_type), len(shape), i64_array(shape),
                                      i64_array(chunk_shape),
                                      None if codecs is None else codecs.encode(), fv))
    return open_array(path)


def read_array(path, start=None, shape=None, nthreads: int = 0,
               out: Optional[np.ndarray] = None) -> np.ndarray:
    """Array::retrieve_array_subset_ndarray into a numpy array (bfloat16 as raw uint16); `out`:
    an existing C-contiguous array of that shape and type to fill (e.g. a view of pinned host
    memory)."""
    info = open_array(path)
    start = [0] * info.ndim if start is None else [int(s) for s in start]
    shape = list(info.shape) if shape is None else [int(s) for s in shape]
    if out is None:
        out = np.empty(shape, dtype=NUMPY[info.data_type])
    elif (list(out.shape) != shape or out.dtype != np.dtype(NUMPY[info.data_type])
          or not out.flags["C_CONTIGUOUS"]):
        raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS, "read_array: bad out array")
    check(lib().zt_store_read_subset(_b(path), i64_array(start), i64_array(shape),
                                     out.ctypes.data_as(ctypes.c_void_p), int(nthreads)))
    return out


def write_array(path, data: np.ndarray, start=None, nthreads: int = 0, occupied=None) -> None:
    """Array::store_array_subset_ndarray for a chunk-aligned subset. `occupied` (used when this
    thread elides empty chunks, set_store_empty_chunks(False)): what the caller already knows
    about the data, one byte per inner chunk of the subset in C order of ceil(shape / inner chunk
    shape), 0 = nothing but the fill value (filter.chunk_occupancy of the same data); None = the
    data is scanned on the host."""
    info = open_array(path)
    data = np.ascontiguousarray(data)
    start = [0] * info.ndim if start is None else [int(s) for s in start]
    occ = None
    if occupied is not None:
        grid = tuple(-(-int(n) // int(c)) for n, c in zip(data.shape, info.inner_chunk_shape))
        occ = np.ascontiguousarray(occupied, dtype=np.uint8)
        if occ.shape != grid:
            raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                         f"write_array: occupied has shape {occ.shape}, the "
                                         f"subset has {grid} inner chunks")
    check(lib().zt_store_write_subset_occupancy(
        _b(path), i64_array(start), i64_array(data.shape), data.ctypes.data_as(ctypes.c_void_p),
        None if occ is None else occ.ctypes.data_as(ctypes.c_void_p), int(nthreads)))


def write_empty(path, start, shape, nthreads: int = 0) -> None:
    """write_array of a chunk-aligned subset that the caller knows to hold nothing but the fill
    value, for a thread that elides empty chunks: nothing is written and the subset's chunk files
    are removed. No data is passed."""
    info = open_array(path)
    grid = [-(-int(n) // int(c)) for n, c in zip(shape, info.inner_chunk_shape)]
    occ = np.zeros(grid, dtype=np.uint8)
    check(lib().zt_store_write_subset_occupancy(
        _b(path), i64_array(start), i64_array(shape), None,
        occ.ctypes.data_as(ctypes.c_void_p), int(nthreads)))


def fill_value_of(path):
    """The fill_value of an array's metadata (also of an array whose metadata is held)."""
    for name in ("zarr.json", PENDING_METADATA):
        try:
            with open(os.path.join(path, name)) as f:
                return json.load(f)["fill_value"]
        except FileNotFoundError:
            continue
    raise _abi.FilterError(_abi.ERR_STORAGE, f"no Zarr V3 array at {path}")


def write_synth(path, kind: int = SYNTH_STEP_NOISE_F32, seed: int = SEED,
                nthreads: int = 0) -> None:
    """Fill an array with the SURVEY.md §8(d) synthetic volume (same values as the device
    generator and oracle.synth_step_noise_f32 / synth_u16)."""
    check(lib().zt_store_write_synth(_b(path), int(kind), int(seed), int(nthreads)))


def codec_available(name: str) -> bool:
    return bool(lib().zt_store_codec_available(name.encode()))


def _enc(encoding) -> Optional[bytes]:
    """Reencoding arguments (ZarrReencodingArgs keys, lib.rs:274-377) as the ABI's JSON."""
    if encoding is None:
        return None
    if isinstance(encoding, (bytes, str)):
        return encoding.encode() if isinstance(encoding, str) else encoding
    return json.dumps({k: v for k, v in encoding.items() if v is not None}).encode()


_progress_keep = None


def set_progress_callback(fn) -> None:
    """Per-chunk progress of the store filters (Progress, progress.rs:15-119): `fn(stats)` with
    stats = {step, num_steps, read_s, process_s, write_s} after every output chunk is written.
    Process-wide; None disables."""
    global _progress_keep
    if fn is None:
        lib().zt_store_set_progress_callback(_abi.PROGRESS_FN(), None)
        _progress_keep = None
        return

    def _cb(p, _user):
        s = p.contents
        fn({"step": s.step, "num_steps": s.num_steps, "read_s": s.read_s,
            "process_s": s.process_s, "write_s": s.write_s})

    _progress_keep = _abi.PROGRESS_FN(_cb)
    lib().zt_store_set_progress_callback(_progress_keep, None)


def create_output_like(input_path, output_path, data_type: Optional[str] = None,
                       encoding=None) -> None:
    """The output array a filter creates (output_array_builder, filter_traits.rs:47-82), with
    its zarr.json written."""
    check(lib().zt_store_create_output_like(_b(input_path), _b(output_path), _dt(data_type),
                                            _enc(encoding)))


def create_output(input_path, output_path, data_type: Optional[str] = None, shape=None,
                  encoding=None) -> None:
    """The output array of a filter step with an explicit shape (None = the input's), as the
    store filters create it (reencoding included), zarr.json written, no chunk data."""
    nd = 0 if shape is None else len(shape)
    check(lib().zt_store_create_output(_b(input_path), _b(output_path), _dt(data_type),
                                       None if shape is None else i64_array(shape), nd,
                                       _enc(encoding)))


def host_available_bytes() -> int:
    """Host memory the store pipeline may budget (as host_available_bytes in host/zt_store.cpp):
    ZT_STORE_HOST_MEMORY if set, else MemAvailable capped at the cgroup's limit minus its usage,
    the usage without the cgroup's inactive file pages (reclaimable page cache, which MemAvailable
    counts as available). ZT_MEMINFO / ZT_CGROUP_ROOT relocate the files read (tests)."""
    env = os.environ.get("ZT_STORE_HOST_MEMORY")
    if env:
        return int(env)
    avail = 16 << 30
    try:
        with open(os.environ.get("ZT_MEMINFO", "/proc/meminfo")) as f:
            for line in f:
                if line.startswith("MemAvailable:"):
                    avail = int(line.split()[1]) * 1024
                    break
    except OSError:
        pass

    def _u64(path):
        try:
            with open(path) as f:
                t = f.read().strip()
            return int(t) if t.isdigit() else None
        except OSError:
            return None

    def _stat(path, key):
        try:
            with open(path) as f:
                for line in f:
                    k, _, v = line.partition(" ")
                    if k == key:
                        return int(v)
        except (OSError, ValueError):
            pass
        return 0

    root = os.environ.get("ZT_CGROUP_ROOT", "/sys/fs/cgroup")
    for lim_p, use_p, stat_p, key in (
            ("memory.max", "memory.current", "memory.stat", "inactive_file"),
            ("memory/memory.limit_in_bytes", "memory/memory.usage_in_bytes",
             "memory/memory.stat", "total_inactive_file")):
        lim, use = _u64(os.path.join(root, lim_p)), _u64(os.path.join(root, use_p))
        if lim is not None and use is not None:
            if lim < (1 << 60):
                used = max(0, use - _stat(os.path.join(root, stat_p), key))
                avail = min(avail, max(0, lim - used))
            break
    return avail


PENDING_METADATA = ".zt_pending.json"  # kPendingMetadata, host/zt_zarr.hpp


def hold_metadata(path) -> None:
    """Hide a new array's zarr.json until its chunks are written ("not finished",
    zarrs_filter.rs:297-313; the reference stores metadata after the chunks): Zarr readers do not
    see the array, the store functions of this package still open it."""
    os.replace(os.path.join(path, "zarr.json"), os.path.join(path, PENDING_METADATA))


def publish_metadata(path) -> None:
    """The array is finished: its held metadata becomes zarr.json (an atomic rename)."""
    os.replace(os.path.join(path, PENDING_METADATA), os.path.join(path, "zarr.json"))


def set_chunk_limit(chunk_limit) -> None:
    """--chunk-limit for the store filters this thread calls next: at most that many chunks in
    flight (zt_store_set_chunk_limit; 0 / None = bounded by memory only)."""
    check(lib().zt_store_set_chunk_limit(int(chunk_limit or 0)))


STORE_EMPTY_CHUNKS_ENV = "ZT_STORE_EMPTY_CHUNKS"  # "0": the default of new threads is to elide
_store_empty = threading.local()


def store_empty_chunks() -> bool:
    """This thread's setting (set_store_empty_chunks)."""
    if not hasattr(_store_empty, "v"):
        _store_empty.v = os.environ.get(STORE_EMPTY_CHUNKS_ENV) != "0"
    return _store_empty.v


def set_store_empty_chunks(store_empty_chunks: bool) -> None:
    """zarrs' `store_empty_chunks` for the store filters and writes this thread makes next
    (zt_store_set_store_empty_chunks). True (the default) stores every chunk; False leaves out
    the chunks, and the inner chunks of shards, that hold nothing but the fill value, and removes
    the files of chunks that became empty, as the reference's stores do."""
    check(lib().zt_store_set_store_empty_chunks(int(bool(store_empty_chunks))))
    _store_empty.v = bool(store_empty_chunks)


def last_elided() -> tuple:
    """(chunks, inner_chunks) that the last store filter or write of this thread elided: chunk
    files not written, and empty inner chunks inside the array's inner-chunk grid (the chunks
    themselves for an unsharded array)."""
    c, i = ctypes.c_int64(), ctypes.c_int64()
    check(lib().zt_store_last_elided(ctypes.byref(c), ctypes.byref(i)))
    return c.value, i.value


def _stats(st) -> dict:
    """The stats of a store filter that just ran on this thread."""
    return {**st.as_dict(), "chunks_elided": last_elided()[0]}


def _flags(erase: bool, finish: bool) -> int:
    return (_abi.STORE_ERASE_OUTPUT_METADATA if erase else 0) | (
        _abi.STORE_FINISH_OUTPUT if finish else 0)


def guided_filter(input_path, output_path, epsilon: float, radius: int,
                  data_type: Optional[str] = None, device: int = 0, rows=None,
                  nthreads: int = 0, erase: bool = True, finish: bool = True,
                  encoding=None, chunk_limit: int = 0, cols=None) -> dict:
    """zarrs_filter guided-filter INPUT OUTPUT EPSILON RADIUS [--data-type T] on GPU `device`.
    `rows` = (begin, end) output chunk rows along axis 0 (None = all); `cols` = (begin, end)
    output chunk columns along axis 1 (None = all; a (t, z) block of a multi-GPU split);
    `chunk_limit` = at most that many chunks in flight (--chunk-limit, 0 = memory-bounded).
    Returns the run stats."""
    set_chunk_limit(chunk_limit)
    st = _abi.StoreStats()
    r0, r1 = (0, -1) if rows is None else (int(rows[0]), int(rows[1]))
    c0, c1 = (0, -1) if cols is None else (int(cols[0]), int(cols[1]))
    check(lib().zt_store_guided_filter_box(_b(input_path), _b(output_path), _dt(data_type),
                                           _enc(encoding), float(epsilon), int(radius),
                                           int(device), r0, r1, c0, c1, int(nthreads),
                                           _flags(erase, finish), ctypes.byref(st)))
    return _stats(st)


def downsample(input_path, output_path, stride, discrete: bool = False,
               data_type: Optional[str] = None, device: int = 0, rows=None, nthreads: int = 0,
               erase: bool = True, finish: bool = True, encoding=None,
               chunk_limit: int = 0) -> dict:
    """zarrs_filter downsample INPUT OUTPUT STRIDE [--discrete] / one zarrs_ome level."""
    set_chunk_limit(chunk_limit)
    st = _abi.StoreStats()
    r0, r1 = (0, -1) if rows is None else (int(rows[0]), int(rows[1]))
    check(lib().zt_store_downsample(_b(input_path), _b(output_path), i64_array(stride),
                                    int(bool(discrete)), _dt(data_type), _enc(encoding),
                                    int(device), r0, r1,
                                    int(nthreads), _flags(erase, finish), ctypes.byref(st)))
    return _stats(st)


def _sigma_half(sigma, kernel_half_size):
    sigma = [float(x) for x in sigma]
    half = [int(x) for x in kernel_half_size]
    return (ctypes.c_float * len(sigma))(*sigma), i64_array(half)


def gaussian(input_path, output_path, sigma, kernel_half_size, data_type: Optional[str] = None,
             device: int = 0, rows=None, nthreads: int = 0, erase: bool = True,
             finish: bool = True, encoding=None, chunk_limit: int = 0) -> dict:
    """zarrs_filter gaussian INPUT OUTPUT SIGMA KERNEL_HALF_SIZE [--data-type T]."""
    set_chunk_limit(chunk_limit)
    st = _abi.StoreStats()
    r0, r1 = (0, -1) if rows is None else (int(rows[0]), int(rows[1]))
    sg, hs = _sigma_half(sigma, kernel_half_size)
    check(lib().zt_store_gaussian(_b(input_path), _b(output_path), _dt(data_type),
                                  _enc(encoding), sg, hs,
                                  int(device), r0, r1, int(nthreads), _flags(erase, finish),
                                  ctypes.byref(st)))
    return _stats(st)


def gradient_magnitude(input_path, output_path, operator: str = "sobel",
                       data_type: Optional[str] = None, device: int = 0, rows=None,
                       nthreads: int = 0, erase: bool = True, finish: bool = True, encoding=None,
                       chunk_limit: int = 0) -> dict:
    """zarrs_filter gradient-magnitude INPUT OUTPUT [--operator OP] [--data-type T]
    (gradient_magnitude.rs:197-274); `operator`: "sobel" or "central_difference"."""
    from .filter import gm_operator
    op = gm_operator(operator)
    set_chunk_limit(chunk_limit)
    st = _abi.StoreStats()
    r0, r1 = (0, -1) if rows is None else (int(rows[0]), int(rows[1]))
    check(lib().zt_store_gradient_magnitude(_b(input_path), _b(output_path), _dt(data_type),
                                            _enc(encoding), op, int(device), r0, r1,
                                            int(nthreads), _flags(erase, finish),
                                            ctypes.byref(st)))
    return _stats(st)


def rank_filter(input_path, output_path, kind: str, kernel_half_size,
                data_type: Optional[str] = None, device: int = 0, rows=None, nthreads: int = 0,
                erase: bool = True, finish: bool = True, encoding=None,
                chunk_limit: int = 0) -> dict:
    """zarrs_filter median | minimum | maximum INPUT OUTPUT KERNEL_HALF_SIZE [--data-type T];
    `kind`: "minimum", "median" or "maximum"."""
    from .filter import rank_kind
    code = rank_kind(kind)
    set_chunk_limit(chunk_limit)
    st = _abi.StoreStats()
    r0, r1 = (0, -1) if rows is None else (int(rows[0]), int(rows[1]))
    check(lib().zt_store_rank_filter(_b(input_path), _b(output_path), _dt(data_type),
                                     _enc(encoding), code,
                                     i64_array([int(x) for x in kernel_half_size]), int(device),
                                     r0, r1, int(nthreads), _flags(erase, finish),
                                     ctypes.byref(st)))
    return _stats(st)


def arithmetic(first, second, output, operator: str, data_type: Optional[str] = None,
               device: int = 0, rows=None, nthreads: int = 0, erase: bool = True,
               finish: bool = True, encoding=None, chunk_limit: int = 0) -> dict:
    """zarrs_filter arithmetic FIRST OUTPUT OPERATOR SECOND [--data-type T]: output = first
    `operator` second, element by element (filter.Arithmetic); the output array is built from the
    first array. `operator`: one of filter.ARITHMETIC_OPERATORS."""
    from .filter import arithmetic_operator
    op = arithmetic_operator(operator)
    set_chunk_limit(chunk_limit)
    st = _abi.StoreStats()
    r0, r1 = (0, -1) if rows is None else (int(rows[0]), int(rows[1]))
    check(lib().zt_store_arithmetic(_b(first), _b(second), _b(output), _dt(data_type),
                                    _enc(encoding), op, int(device), r0, r1, int(nthreads),
                                    _flags(erase, finish), ctypes.byref(st)))
    return _stats(st)


def summed_area_table(input_path, output_path, data_type: Optional[str] = None, device: int = 0,
                      nthreads: int = 0, erase: bool = True, finish: bool = True, encoding=None,
                      chunk_limit: int = 0) -> dict:
    """zarrs_filter summed-area-table INPUT OUTPUT [--data-type T] (summed_area_table.rs:144-253)
    in one read and one write of the store. The chunk rows depend on each other in order, so
    there is no `rows` range."""
    set_chunk_limit(chunk_limit)
    st = _abi.StoreStats()
    check(lib().zt_store_summed_area_table(_b(input_path), _b(output_path), _dt(data_type),
                                           _enc(encoding), int(device), int(nthreads),
                                           _flags(erase, finish), ctypes.byref(st)))
    return _stats(st)


def device_available_bytes(device: int = 0) -> int:
    """Device memory a store step may budget (as device_available_bytes in host/zt_store.cpp):
    ZT_STORE_DEVICE_MEMORY if set, else the free memory of `device`."""
    env = os.environ.get("ZT_STORE_DEVICE_MEMORY")
    if env:
        return int(env)
    import torch
    return int(torch.cuda.mem_get_info(device)[0])


def _encoding_dict(encoding) -> dict:
    """Reencoding arguments (a dict, its JSON, or None) as a dict of the caller's own."""
    return dict(encoding) if isinstance(encoding, dict) else (
        json.loads(encoding) if encoding else {})


def _typed_output(default: str, data_type: Optional[str], encoding):
    """(output data type, encoding) of an output array whose filter sets its type: an explicit
    data type (`data_type` or the encoding's) wins, else `default`; the fill value is 0 unless
    given."""
    enc = _encoding_dict(encoding)
    dt = enc.get("data_type") or data_type or default
    enc["data_type"] = dt
    if enc.get("fill_value") is None:
        enc["fill_value"] = 0
    return dt, enc


def _pinned_read_bytes(shape, chunk_shape, esz: int) -> int:
    """The pinned host bytes of reading an array of `shape` (no axis empty) into device memory:
    device_io.read_to_device holds up to three buffers of the largest of its pieces."""
    from .device_io import _read_pieces
    pieces = _read_pieces([0] * len(shape), shape, chunk_shape, esz)
    plane2 = int(np.prod(shape[2:])) if len(shape) > 2 else 1
    return min(3, len(pieces)) * esz * max(
        (b - a) * (yb - ya) * plane2 for a, b, ya, yb in pieces)


PINNED_BUFFERS_NEED = "its pinned host buffers need {} bytes"


def _not_enough_memory(need: int, budget: int, needs: str, why: str):
    """The error of an array that does not fit 80 % of the available memory: `needs` says what
    needs the `need` bytes (its {} is their place), `why` what the step cannot do instead."""
    raise _abi.FilterError(
        _abi.ERR_OUT_OF_MEMORY,
        f"There is not enough available memory to process the array: {needs.format(need)} and "
        f"80 % of the available memory is {budget}; {why}")


def connected_components_output(data_type: Optional[str] = None, encoding=None):
    """(output data type, encoding) of a labelling's output array: uint32 unless given
    (_typed_output)."""
    return _typed_output("uint32", data_type, encoding)


def connected_components(input_path, output_path, connectivity: int = 1,
                         data_type: Optional[str] = None, device: int = 0, nthreads: int = 0,
                         encoding=None) -> dict:
    """zarrs_filter connected-components INPUT OUTPUT [--connectivity C] [--data-type T]: labels
    the connected sets of non-zero elements (filter.ConnectedComponents; uint32 labels and fill
    value 0 unless given). A component may span every chunk, so the whole array is read into
    device memory, labelled there and written once; there is no store -> store path, and an
    array that does not fit 80 % of the free device memory fails with ZT_ERR_OUT_OF_MEMORY before
    anything is read. When K does not fit the output type the step fails with InvalidParameters,
    writes no chunk and publishes no zarr.json. Returns the run stats and "components": K."""
    import time
    from . import filter as F
    t0 = time.perf_counter()
    info = open_array(input_path)
    filt = F.ConnectedComponents(connectivity)
    dt, enc = connected_components_output(data_type, encoding)
    filt.is_compatible(info.data_type, dt)
    filt.check_connectivity(info.ndim)
    st, k = _whole_array_step(
        input_path, output_path, info, filt, dt, enc, device, nthreads, t0,
        "input, labels and two index arrays",
        "connected_components labels the whole array in device memory (a component "
        "may span every chunk): there is no store -> store path to fall back to")
    st["components"] = int(k)
    return st


def _whole_array_step(input_path, output_path, info, filt, dt, enc, device, nthreads, t0,
                      terms: str, no_fallback: str):
    """A filter whose unit of work is the whole array (connected_components, distance_transform):
    budgets checked before anything is read, the metadata held back, the array read into device
    memory, `filt.apply` on it, the result written once, the metadata published. Returns (run
    stats, what `filt.apply` returned)."""
    import time
    from . import filter as F
    from .device_io import _row_spans, read_to_device, write_from_device
    for name in ("zarr.json", PENDING_METADATA):  # the output is not finished until the end
        try:
            os.remove(os.path.join(output_path, name))
        except FileNotFoundError:
            pass
    # budgets, before anything is read: the array, its result and the scratch on the device; the
    # pinned pieces of the read and the pinned rows of the write on the host
    shape = [int(s) for s in info.shape]
    in_esz, out_esz = NUMPY[info.data_type]().itemsize, NUMPY[dt]().itemsize
    need = filt.memory(info.data_type, dt, shape)
    budget = device_available_bytes(device) // 10 * 8
    if need > budget:
        _not_enough_memory(need, budget, f"it needs {{}} bytes of device memory ({terms})",
                           no_fallback)
    host_need = 0
    if all(s > 0 for s in shape):
        out_chunk0 = int((enc.get("shard_shape") or enc.get("chunk_shape") or info.chunk_shape)[0])
        rows = max(b - a for a, b in _row_spans(0, shape[0], out_chunk0))
        row_b = rows * int(np.prod(shape[1:])) * out_esz
        host_need = max(_pinned_read_bytes(shape, info.chunk_shape, in_esz),
                        min(2, -(-shape[0] // out_chunk0)) * row_b)
    host_budget = host_available_bytes() // 10 * 8
    if host_need > host_budget:
        _not_enough_memory(host_need, host_budget, PINNED_BUFFERS_NEED, no_fallback)
    create_output(input_path, output_path, dt, None, enc)
    hold_metadata(output_path)  # "not finished" until the chunks are written
    out_info = open_array(output_path)
    import torch
    t1 = time.perf_counter()
    x = read_to_device(input_path, device, nthreads)
    t_read = time.perf_counter() - t1
    y = torch.empty(tuple(shape), dtype=F.torch_dtype(dt), device=x.device)
    ctx = F.default_context(device)
    t1 = time.perf_counter()
    try:
        ret = filt.apply(F.DeviceArray(x, info.chunk_shape, info.data_type),
                         F.DeviceArray(y, out_info.chunk_shape, dt), ctx=ctx)
        ctx.synchronize()
    finally:
        ctx.release_scratch()
    t_kernel = time.perf_counter() - t1
    del x
    t1 = time.perf_counter()
    elided = write_from_device(output_path, y, nthreads) or 0
    publish_metadata(output_path)
    t_write = time.perf_counter() - t1
    n = int(np.prod(shape)) if shape else 0
    return {"wall_s": time.perf_counter() - t0, "decode_s": t_read, "encode_s": t_write,
            "h2d_s": 0.0, "kernel_s": t_kernel, "d2h_s": 0.0, "bytes_read": n * in_esz,
            "bytes_written": n * out_esz, "voxels": n, "rows": 0, "threads": int(nthreads),
            "rows_in_flight": 0, "double_buffered": 0, "chunks_elided": int(elided),
            "device_resident": True}, ret


def distance_transform_output(squared: bool = False, data_type: Optional[str] = None,
                              encoding=None):
    """(output data type, encoding) of a distance transform's output array: float32, or uint32
    for squared distances, unless given (_typed_output)."""
    from .filter import distance_transform_default_type
    return _typed_output(distance_transform_default_type(squared), data_type, encoding)


def distance_transform(input_path, output_path, spacing=None, squared: bool = False,
                       data_type: Optional[str] = None, device: int = 0, nthreads: int = 0,
                       encoding=None) -> dict:
    """zarrs_filter distance-transform INPUT OUTPUT [--spacing S[,S...]] [--squared]
    [--data-type T]: the exact Euclidean distance of every element to the nearest zero element
    (filter.DistanceTransform; float32, or uint32 with `squared`, and fill value 0 unless given).
    The nearest background element may lie in any chunk, so the whole array is read into device
    memory, transformed there and written once; there is no store -> store path, and an array that
    does not fit 80 % of the free device memory fails with ZT_ERR_OUT_OF_MEMORY before anything is
    read. Returns the run stats."""
    import time
    from . import filter as F
    t0 = time.perf_counter()
    info = open_array(input_path)
    filt = F.DistanceTransform(spacing, squared)
    dt, enc = distance_transform_output(squared, data_type, encoding)
    filt.is_compatible(info.data_type, dt)
    filt.check_spacing(info.ndim)
    st, _ = _whole_array_step(
        input_path, output_path, info, filt, dt, enc, device, nthreads, t0,
        "input, distances, two work arrays and two stacks",
        "distance_transform works on the whole array in device memory (the nearest background "
        "element may lie in any chunk): there is no store -> store path to fall back to")
    return st


def label_size_filter_output(input_data_type: str, data_type: Optional[str] = None,
                             encoding=None):
    """(output data type, encoding) of a size filter's output array: the input's type unless
    given (_typed_output)."""
    return _typed_output(input_data_type, data_type, encoding)


class SizeFilterStep:
    """LabelSizeFilter as a whole-array step drives it. The scratch depends on the largest label,
    which is known only once the array is on the device; the budget takes the largest it can be:
    the input type's maximum, the limit on labels, and (a label array made by
    connected_components never exceeds it) the element count."""

    def __init__(self, filt):
        self.filt = filt
        self.min_size, self.max_size, self.relabel = filt.min_size, filt.max_size, filt.relabel

    def is_compatible(self, dtype_in, dtype_out) -> None:
        self.filt.is_compatible(dtype_in, dtype_out)

    def memory(self, dtype_in, dtype_out, shape) -> int:
        n = int(np.prod(shape)) if len(shape) else 0
        k = min(int(np.iinfo(NUMPY[dtype_in]).max), _abi.LABELS_MAX, max(n, 1))
        return self.filt.memory(dtype_in, dtype_out, shape, k)

    def apply(self, input, output, ctx=None):
        return self.filt.apply(input, output, ctx=ctx)


def label_size_filter(input_path, output_path, min_size: int = 1, max_size: Optional[int] = None,
                      relabel: bool = True, data_type: Optional[str] = None, device: int = 0,
                      nthreads: int = 0, encoding=None) -> dict:
    """zarrs_filter label-size-filter INPUT OUTPUT [--min-size N] [--max-size N] [--no-relabel]
    [--data-type T]: keeps the labels of an integer label array whose element count lies in [min_size,
    max_size] and sets every other label to 0 (filter.LabelSizeFilter; the input's data type and
    fill value 0 unless given); with `relabel` the kept labels are renumbered 1 .. K'. A label may
    span every chunk, so the whole array is read into device memory, filtered there and written
    once; an array that does not fit 80 % of the free device memory fails with
    ZT_ERR_OUT_OF_MEMORY before anything is read. When the largest output label does not fit the
    output type, or an element is negative, the step fails with InvalidParameters, writes no chunk
    and publishes no zarr.json. Returns the run stats and "components": K'."""
    import time
    from . import filter as F
    t0 = time.perf_counter()
    info = open_array(input_path)
    filt = F.LabelSizeFilter(min_size, max_size, relabel)
    dt, enc = label_size_filter_output(info.data_type, data_type, encoding)
    filt.is_compatible(info.data_type, dt)
    st, k = _whole_array_step(
        input_path, output_path, info, SizeFilterStep(filt), dt, enc, device, nthreads, t0,
        "input, output, the counts and the remap table of the most labels the input can hold",
        "label_size_filter counts every label over the whole array in device memory (a label "
        "may span every chunk): there is no store -> store path to fall back to")
    st["components"] = int(k)
    return st


def reconstruction_output(input_path, data_type: Optional[str] = None, encoding=None):
    """(output data type, encoding) of a reconstruction's output array: the input's type (an
    explicit other type is UnsupportedDataType) and, unless given, the input's fill value."""
    enc = _encoding_dict(encoding)
    info = open_array(input_path)
    dt = enc.get("data_type") or data_type or info.data_type
    if dt != info.data_type:
        raise _abi.UnsupportedDataType(
            _abi.ERR_UNSUPPORTED_DATA_TYPE,
            f"reconstruction: the output has the input's data type {info.data_type}, not {dt}")
    enc["data_type"] = dt
    return dt, enc


class MarkerStep:
    """Reconstruction with a marker array as a whole-array step drives it: the marker is read into
    device memory after the mask (its bytes are in `memory`) and released with the step."""

    def __init__(self, filt, marker_path, device: int, nthreads: int):
        self.filt, self.marker_path = filt, marker_path
        self.device, self.nthreads = device, nthreads

    def memory(self, dtype_in, dtype_out, shape) -> int:
        return self.filt.memory(dtype_in, dtype_out, shape)

    def apply(self, input, output, ctx=None):
        from . import filter as F
        from .device_io import read_to_device
        info = open_array(self.marker_path)
        marker = read_to_device(self.marker_path, self.device, self.nthreads)
        return self.filt.apply(input, F.DeviceArray(marker, info.chunk_shape, info.data_type),
                               output, ctx=ctx)


def reconstruction(input_path, output_path, marker_path=None, method: str = "dilation",
                   connectivity: int = 1, mode: Optional[str] = None, h=None,
                   data_type: Optional[str] = None, device: int = 0, nthreads: int = 0,
                   encoding=None) -> dict:
    """zarrs_filter reconstruction INPUT OUTPUT (--marker PATH | --fill-holes | --h-maxima H |
    --h-minima H) [--method dilation|erosion] [--connectivity C]: morphological reconstruction
    under the mask INPUT (filter.Reconstruction) of the marker array at `marker_path` (same shape
    and data type; any chunk grid and codecs), or of a marker made from the mask (`mode`
    "fill_holes", "h_maxima", "h_minima"). The output has the input's data type and fill value. The
    result at an element may depend on every chunk, so the arrays are read into device memory,
    reconstructed there and the result written once; there is no store -> store path, and arrays
    that do not fit 80 % of the free device memory fail with ZT_ERR_OUT_OF_MEMORY before anything
    is read. Returns the run stats and "rounds"."""
    import time
    from . import filter as F
    t0 = time.perf_counter()
    info = open_array(input_path)
    mode = mode or "marker"
    filt = F.Reconstruction(method, connectivity, mode, h)
    if (filt.mode == "marker") != (marker_path is not None):
        raise _abi.InvalidParameters(
            _abi.ERR_INVALID_PARAMETERS,
            "reconstruction: mode marker needs a marker array" if marker_path is None else
            f"reconstruction: {filt.mode} makes its marker from the mask; no marker array is given")
    dt, enc = reconstruction_output(input_path, data_type, encoding)
    step = filt
    if marker_path is not None:
        minfo = open_array(marker_path)
        filt.is_compatible(info.data_type, minfo.data_type)
        if tuple(minfo.shape) != tuple(info.shape):
            raise _abi.InvalidParameters(
                _abi.ERR_INVALID_PARAMETERS,
                f"Array shapes do not match: {list(info.shape)} vs {list(minfo.shape)}")
        step = MarkerStep(filt, marker_path, device, nthreads)
    else:
        filt.is_compatible(info.data_type)
    filt.check_connectivity(info.ndim)
    no_fallback = ("reconstruction works on the whole array in device memory (the result at an "
                   "element may depend on every chunk): there is no store -> store path to fall "
                   "back to")
    shape = [int(s) for s in info.shape]
    if marker_path is not None and all(s > 0 for s in shape):
        # the pinned pieces of the marker's read, before anything is read (the mask's pieces and
        # the output's rows are _whole_array_step's)
        host_need = _pinned_read_bytes(shape, minfo.chunk_shape,
                                       NUMPY[minfo.data_type]().itemsize)
        host_budget = host_available_bytes() // 10 * 8
        if host_need > host_budget:
            _not_enough_memory(host_need, host_budget, PINNED_BUFFERS_NEED, no_fallback)
    st, rounds = _whole_array_step(
        input_path, output_path, info, step, dt, enc, device, nthreads, t0,
        "mask, marker, output and one working array" if marker_path is not None else
        "mask, output and one working array", no_fallback)
    st["rounds"] = int(rounds)
    return st


def watershed_output(seeds_data_type: str, data_type: Optional[str] = None, encoding=None):
    """(output data type, encoding) of a watershed's output array: the seeds' type (an explicit
    other type is UnsupportedDataType) and fill value 0 unless given."""
    dt, enc = _typed_output(seeds_data_type, data_type, encoding)
    if dt != seeds_data_type:
        raise _abi.UnsupportedDataType(
            _abi.ERR_UNSUPPORTED_DATA_TYPE,
            f"watershed: the output has the seeds' data type {seeds_data_type}, not {dt}")
    return dt, enc


class SeedsStep:
    """Watershed as a whole-array step drives it: the seeds are read into device memory after the
    relief (their bytes are in `memory`) and released with the step."""

    def __init__(self, filt, seeds_path, device: int, nthreads: int):
        self.filt, self.seeds_path = filt, seeds_path
        self.device, self.nthreads = device, nthreads

    def memory(self, dtype_in, dtype_out, shape) -> int:
        return self.filt.memory(dtype_in, dtype_out, shape)

    def apply(self, input, output, ctx=None):
        from . import filter as F
        from .device_io import read_to_device
        info = open_array(self.seeds_path)
        seeds = read_to_device(self.seeds_path, self.device, self.nthreads)
        return self.filt.apply(input, F.DeviceArray(seeds, info.chunk_shape, info.data_type),
                               output, ctx=ctx)


def watershed(input_path, seeds_path, output_path, connectivity: int = 1,
              descending: bool = False, foreground_only: bool = False,
              data_type: Optional[str] = None, device: int = 0, nthreads: int = 0,
              encoding=None) -> dict:
    """zarrs_watershed RELIEF SEEDS OUT [--connectivity C] [--descending] [--foreground-only]:
    the marker-controlled watershed (filter.Watershed) of the relief at `input_path` from the
    non-zero elements of the integer array at `seeds_path` (same shape; any chunk grid and
    codecs). The output has the seeds' data type and fill value 0. A basin may span every chunk,
    so the arrays are read into device memory, flooded there and the labels written once; there is
    no store -> store path, and arrays that do not fit 80 % of the free device memory fail with
    ZT_ERR_OUT_OF_MEMORY before anything is read. Returns the run stats and "rounds": (pass
    rounds, distance rounds, jumps)."""
    import time
    from . import filter as F
    t0 = time.perf_counter()
    info = open_array(input_path)
    sinfo = open_array(seeds_path)
    filt = F.Watershed(connectivity, descending, foreground_only)
    filt.is_compatible(info.data_type, sinfo.data_type)
    dt, enc = watershed_output(sinfo.data_type, data_type, encoding)
    if tuple(sinfo.shape) != tuple(info.shape):
        raise _abi.InvalidParameters(
            _abi.ERR_INVALID_PARAMETERS,
            f"Array shapes do not match: {list(info.shape)} vs {list(sinfo.shape)}")
    filt.check_connectivity(info.ndim)
    no_fallback = ("watershed works on the whole array in device memory (a basin may span every "
                   "chunk): there is no store -> store path to fall back to")
    shape = [int(s) for s in info.shape]
    if all(s > 0 for s in shape):
        # the pinned pieces of the seeds' read, before anything is read (the relief's pieces and
        # the output's rows are _whole_array_step's)
        host_need = _pinned_read_bytes(shape, sinfo.chunk_shape,
                                       NUMPY[sinfo.data_type]().itemsize)
        host_budget = host_available_bytes() // 10 * 8
        if host_need > host_budget:
            _not_enough_memory(host_need, host_budget, PINNED_BUFFERS_NEED, no_fallback)
    st, rounds = _whole_array_step(
        input_path, output_path, info, SeedsStep(filt, seeds_path, device, nthreads), dt, enc,
        device, nthreads, t0,
        "relief, seeds, labels, the working arrays of the pass values and two index arrays",
        no_fallback)
    st["rounds"] = tuple(int(r) for r in rounds)
    return st


def label_statistics(labels_path, intensity_path=None, n_labels: Optional[int] = None,
                     device: int = 0, nthreads: int = 0) -> dict:
    """zarrs_info PATH label-statistics [--intensity PATH] [--n-labels K]: the per-label count,
    bounding box, coordinate sums and centroid of an integer label array, and with an intensity
    array of the same shape (any chunk grid and codecs) the smallest, largest, summed and mean
    intensity (filter.LabelStatistics, whose result dict this returns). Only elements inside the
    shape count and a missing chunk is its fill value. Both arrays are read into device memory;
    arrays (and, with n_labels given, the state) that do not fit 80 % of the free device memory
    fail with ZT_ERR_OUT_OF_MEMORY before anything is read; with n_labels=None the state is
    budgeted once the range reduction has given the largest label."""
    from . import filter as F
    from .device_io import read_to_device
    info = open_array(labels_path)
    iinfo = open_array(intensity_path) if intensity_path is not None else None
    filt = F.LabelStatistics(n_labels)
    filt.is_compatible(info.data_type, iinfo.data_type if iinfo else None)
    shape = [int(s) for s in info.shape]
    if iinfo is not None and [int(s) for s in iinfo.shape] != shape:
        raise _abi.InvalidParameters(
            _abi.ERR_INVALID_PARAMETERS,
            f"Array shapes do not match: {shape} vs {[int(s) for s in iinfo.shape]}")
    n = int(np.prod(shape)) if shape else 0
    arrays = n * NUMPY[info.data_type]().itemsize + \
        (n * NUMPY[iinfo.data_type]().itemsize if iinfo else 0)
    budget = device_available_bytes(device) // 10 * 8

    def refuse(need, k, hint):
        _not_enough_memory(need, budget, "it needs {} bytes of device memory (labels, "
                           f"intensities and the state of {k} labels)",
                           f"label_statistics reduces the whole array in device memory{hint}")

    # budget, before anything is read: the arrays, and the state when n_labels says how large it
    # is; with n_labels=None the state is budgeted once the range reduction has given K
    state = filt.state_bytes(info.ndim, n_labels, iinfo is not None) if n_labels is not None else 0
    if arrays + state > budget:
        refuse(arrays + state, n_labels if n_labels is not None else "the", "")
    x = read_to_device(labels_path, device, nthreads)
    y = read_to_device(intensity_path, device, nthreads) if iinfo else None
    ctx = F.default_context(device)
    lab = F.DeviceArray(x, info.chunk_shape, info.data_type)
    if n_labels is None:
        k = filt.largest_label(lab, ctx)
        if k > _abi.LABELS_MAX:
            raise _abi.InvalidParameters(
                _abi.ERR_INVALID_PARAMETERS,
                f"label_statistics: n_labels {k} not in [0, {_abi.LABELS_MAX}]")
        state = filt.state_bytes(info.ndim, k, iinfo is not None)
        if arrays + state > budget:
            refuse(arrays + state, k, ": pass a smaller n_labels only if the labels allow it")
        filt = F.LabelStatistics(k)
    return filt.apply_ndarray(lab, None if y is None else
                              F.DeviceArray(y, iinfo.chunk_shape, iinfo.data_type), ctx)


def pointwise_output(filt, input_data_type: str, data_type: Optional[str] = None, encoding=None):
    """(output data type, encoding) of a per-element filter's output array, as
    output_array_builder decides it (filter_traits.rs:47-82): an explicit data type (`data_type`
    or the encoding's) wins; else the filter's own (Equal::output_data_type: bool with fill value
    false, equal.rs:121-123), which also sets the fill value; else the input's."""
    enc = _encoding_dict(encoding)
    dt = enc.get("data_type") or data_type
    if dt is None:
        auto = filt.output_data_type(input_data_type)
        if auto is not None:
            dt, enc["fill_value"] = auto
    if dt is not None:
        enc["data_type"] = dt
    return dt or input_data_type, (enc or None)


def pointwise(input_path, output_path, filters, dtypes_out, device: int = 0, rows=None,
              nthreads: int = 0, erase: bool = True, finish: bool = True, encoding=None,
              chunk_limit: int = 0) -> dict:
    """Consecutive per-element filters (filter.Reencode ... ReplaceValue) over a store in one
    pass (zt_store_pointwise): filter k writes dtypes_out[k]; the last one is the output array's
    data type and must agree with `encoding`."""
    from .filter import PointwiseProgram
    info = open_array(input_path)
    prog = PointwiseProgram(filters, info.data_type, dtypes_out, info.shape)
    off, shp = prog.box()
    set_chunk_limit(chunk_limit)
    st = _abi.StoreStats()
    r0, r1 = (0, -1) if rows is None else (int(rows[0]), int(rows[1]))
    check(lib().zt_store_pointwise(_b(input_path), _b(output_path), _dt(dtypes_out[-1]),
                                   _enc(encoding), prog.ops, prog.n_ops, off, shp, int(device),
                                   r0, r1, int(nthreads), _flags(erase, finish),
                                   ctypes.byref(st)))
    return _stats(st)


def _pointwise_one(filt, input_path, output_path, data_type, encoding, **kw) -> dict:
    dt, enc = pointwise_output(filt, open_array(input_path).data_type, data_type, encoding)
    return pointwise(input_path, output_path, [filt], [dt], encoding=enc, **kw)


def reencode(input_path, output_path, data_type: Optional[str] = None, device: int = 0,
             rows=None, nthreads: int = 0, erase: bool = True, finish: bool = True,
             encoding=None, chunk_limit: int = 0) -> dict:
    """zarrs_filter reencode INPUT OUTPUT [--data-type T ...] (reencode.rs:128-218)."""
    from .filter import Reencode
    return _pointwise_one(Reencode(), input_path, output_path, data_type, encoding,
                          device=device, rows=rows, nthreads=nthreads, erase=erase,
                          finish=finish, chunk_limit=chunk_limit)


def crop(input_path, output_path, offset, shape, data_type: Optional[str] = None,
         device: int = 0, rows=None, nthreads: int = 0, erase: bool = True, finish: bool = True,
         encoding=None, chunk_limit: int = 0) -> dict:
    """zarrs_filter crop INPUT OUTPUT OFFSET SHAPE [--data-type T] (crop.rs:164-247)."""
    from .filter import Crop
    return _pointwise_one(Crop(offset, shape), input_path, output_path, data_type, encoding,
                          device=device, rows=rows, nthreads=nthreads, erase=erase,
                          finish=finish, chunk_limit=chunk_limit)


def rescale(input_path, output_path, multiply: float, add: float, add_first: bool = False,
            data_type: Optional[str] = None, device: int = 0, rows=None, nthreads: int = 0,
            erase: bool = True, finish: bool = True, encoding=None,
            chunk_limit: int = 0) -> dict:
    """zarrs_filter rescale INPUT OUTPUT MULTIPLY ADD [--add-first] [--data-type T]
    (rescale.rs:160-239)."""
    from .filter import Rescale
    return _pointwise_one(Rescale(multiply, add, add_first), input_path, output_path, data_type,
                          encoding, device=device, rows=rows, nthreads=nthreads, erase=erase,
                          finish=finish, chunk_limit=chunk_limit)


def clamp(input_path, output_path, min: float, max: float, data_type: Optional[str] = None,
          device: int = 0, rows=None, nthreads: int = 0, erase: bool = True, finish: bool = True,
          encoding=None, chunk_limit: int = 0) -> dict:
    """zarrs_filter clamp INPUT OUTPUT MIN MAX [--data-type T] (clamp.rs:108-211)."""
    from .filter import Clamp
    return _pointwise_one(Clamp(min, max), input_path, output_path, data_type, encoding,
                          device=device, rows=rows, nthreads=nthreads, erase=erase,
                          finish=finish, chunk_limit=chunk_limit)


def equal(input_path, output_path, value, data_type: Optional[str] = None, device: int = 0,
          rows=None, nthreads: int = 0, erase: bool = True, finish: bool = True, encoding=None,
          chunk_limit: int = 0) -> dict:
    """zarrs_filter equal INPUT OUTPUT VALUE [--data-type bool|uint8] (equal.rs:125-214); the
    output is bool with fill value false unless a data type is given."""
    from .filter import Equal
    return _pointwise_one(Equal(value), input_path, output_path, data_type, encoding,
                          device=device, rows=rows, nthreads=nthreads, erase=erase,
                          finish=finish, chunk_limit=chunk_limit)


def replace_value(input_path, output_path, value, replace, data_type: Optional[str] = None,
                  device: int = 0, rows=None, nthreads: int = 0, erase: bool = True,
                  finish: bool = True, encoding=None, chunk_limit: int = 0) -> dict:
    """zarrs_filter replace-value INPUT OUTPUT VALUE REPLACE [--data-type T]
    (replace_value.rs:135-240)."""
    from .filter import ReplaceValue
    return _pointwise_one(ReplaceValue(value, replace), input_path, output_path, data_type,
                          encoding, device=device, rows=rows, nthreads=nthreads, erase=erase,
                          finish=finish, chunk_limit=chunk_limit)


def range(path, device: int = 0, rows=None, nthreads: int = 0, chunk_limit: int = 0,
          stats: Optional[dict] = None):
    """zarrs_info PATH range over a store (zt_store_range): (min, max) of the elements inside the
    array's shape as Python values (int, or float widened to f64), (None, None) when there is no
    non-NaN element. `rows` = (begin, end) input chunk rows along axis 0 (None = all): partial
    results combine with filter.combine_ranges. `stats`: a dict that receives the run stats."""
    from .filter import element_value
    set_chunk_limit(chunk_limit)
    st = _abi.StoreStats()
    r0, r1 = (0, -1) if rows is None else (int(rows[0]), int(rows[1]))
    dt, none = ctypes.c_int(-1), ctypes.c_int()
    lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
    check(lib().zt_store_range(_b(path), int(device), r0, r1, int(nthreads), ctypes.byref(dt),
                               ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(none),
                               ctypes.byref(st)))
    if stats is not None:
        stats.update(st.as_dict())
    if none.value:
        return None, None
    name = DTYPE_NAMES[dt.value]
    return element_value(lo.value, name), element_value(hi.value, name)


def histogram(path, n_bins: int, min: float, max: float, device: int = 0, rows=None,
              nthreads: int = 0, chunk_limit: int = 0, stats: Optional[dict] = None):
    """zarrs_info PATH histogram N_BINS MIN MAX over a store (zt_store_histogram): (bin_edges:
    np.float64[n_bins + 1], hist: np.uint64[n_bins]). `rows` as `range`: partial results combine
    with filter.combine_histograms."""
    from .filter import Histogram
    edges = Histogram(n_bins, min, max).bin_edges()  # validates n_bins, min, max
    set_chunk_limit(chunk_limit)
    st = _abi.StoreStats()
    r0, r1 = (0, -1) if rows is None else (int(rows[0]), int(rows[1]))
    hist = np.zeros(int(n_bins), dtype=np.uint64)
    check(lib().zt_store_histogram(_b(path), int(n_bins), float(min), float(max), int(device),
                                   r0, r1, int(nthreads),
                                   hist.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                   ctypes.byref(st)))
    if stats is not None:
        stats.update(st.as_dict())
    return edges, hist


def compare(first, second, device: int = 0, rows=None, nthreads: int = 0, chunk_limit: int = 0,
            stats: Optional[dict] = None):
    """zarrs_validate FIRST SECOND over two stores (zt_store_compare): (n_diff, first_index) of
    the elements inside the shape compared by their storage bits, first_index the C-order index
    in the whole array or None when the arrays are equal. InvalidParameters with the reference's
    message when the shapes or the data types differ (checked before any device work). `rows` =
    (begin, end) chunk rows of the first array along axis 0 (None = all): partial results combine
    with filter.combine_compares. `stats`: a dict that receives the run stats."""
    set_chunk_limit(chunk_limit)
    st = _abi.StoreStats()
    r0, r1 = (0, -1) if rows is None else (int(rows[0]), int(rows[1]))
    n_diff, idx = ctypes.c_uint64(), ctypes.c_int64()
    check(lib().zt_store_compare(_b(first), _b(second), int(device), r0, r1, int(nthreads),
                                 ctypes.byref(n_diff), ctypes.byref(idx), ctypes.byref(st)))
    if stats is not None:
        stats.update(st.as_dict())
    return n_diff.value, (None if idx.value < 0 else idx.value)


def downsample_gaussian(input_path, output_path, stride, sigma, kernel_half_size,
                        data_type: Optional[str] = None, device: int = 0, rows=None,
                        nthreads: int = 0, erase: bool = True, finish: bool = True,
                        encoding=None, chunk_limit: int = 0) -> dict:
    """One zarrs_ome level with --gaussian-sigma (zarrs_ome.rs:236-271)."""
    set_chunk_limit(chunk_limit)
    st = _abi.StoreStats()
    r0, r1 = (0, -1) if rows is None else (int(rows[0]), int(rows[1]))
    sg, hs = _sigma_half(sigma, kernel_half_size)
    check(lib().zt_store_downsample_gaussian(_b(input_path), _b(output_path), i64_array(stride),
                                             sg, hs, _dt(data_type), _enc(encoding),
                                             int(device), r0, r1,
                                             int(nthreads), _flags(erase, finish),
                                             ctypes.byref(st)))
    return _stats(st)
