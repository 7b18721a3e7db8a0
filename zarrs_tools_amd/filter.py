"""Host-side mirror of the reference's filter-operator surface for the hot path.

Names, argument meaning and error behaviour follow LDeakin/zarrs_tools 0.7.2:
  - ``GuidedFilter`` <- src/filter/filters/guided_filter.rs (GuidedFilter::new(epsilon, radius,
    chunk_limit), apply_ndarray :117, apply_chunk :75, apply :240, is_compatible :203,
    memory_per_chunk :229)
  - ``Downsample`` <- src/filter/filters/downsample.rs (Downsample::new(stride, discrete,
    chunk_limit), input_subset :64, apply_ndarray_continuous :72, apply_ndarray_discrete :99,
    output_shape :162, apply :170)
  - ``GradientMagnitude`` <- src/filter/filters/gradient_magnitude.rs (GradientMagnitude::new(
    operator, chunk_limit), apply_chunk :68, apply_ndarray :109, is_compatible :151,
    memory_per_chunk :177, apply :197)
  - ``RankFilter`` (``Median``, ``Minimum``, ``Maximum``): an extension with no counterpart in
    the reference; its semantics are DESIGN.md §3.11
  - ``SummedAreaTable`` <- src/filter/filters/summed_area_table.rs (SummedAreaTable::new(
    chunk_limit), apply_dim :47, is_compatible :110, memory_per_chunk :136, apply :144)
  - ``Reencode``, ``Crop``, ``Rescale``, ``Clamp``, ``Equal``, ``ReplaceValue`` <-
    src/filter/filters/{reencode,crop,rescale,clamp,equal,replace_value}.rs (the per-element
    filters; ``PointwiseProgram`` runs consecutive ones as one launch)
  - ``Range``, ``Histogram`` <- src/info/range.rs, src/info/histogram.rs (zarrs_info's
    reductions; ``combine_ranges`` / ``combine_histograms`` join partial results)
  - ``Compare`` <- src/bin/zarrs_validate.rs:145-147 (the bitwise comparison of two arrays;
    ``combine_compares`` joins partial results)
  - ``Arithmetic``: an extension with no counterpart in the reference (two arrays in, one out);
    its semantics are DESIGN.md §3.12
  - ``ConnectedComponents``: an extension with no counterpart in the reference (labels of the
    connected sets of non-zero elements); its semantics are DESIGN.md §3.13
  - ``Reconstruction``: an extension with no counterpart in the reference (morphological
    reconstruction of a marker under a mask: fill holes, h-maxima, h-minima); DESIGN.md §3.16
  - ``DistanceTransform``: an extension with no counterpart in the reference (the exact Euclidean
    distance to the nearest zero element); its semantics are DESIGN.md §3.14
  - ``LabelStatistics``, ``LabelSizeFilter``: extensions with no counterpart in the reference
    (per-label count, bounding box, centroid and intensity statistics of a label array, and the
    removal of labels by size; ``combine_label_statistics`` joins partial results); their
    semantics are DESIGN.md §3.15
  - ``chunk_occupancy`` <- zarrs' ``store_empty_chunks = false`` (which chunks of a device
    array hold anything but the fill value)
  - ``ArraySubsetOverlap`` <- src/filter/array_subset_overlap.rs:4-52
Arrays are device-resident torch tensors (torch is used only for device memory and streams);
every computation runs in libzarrs_tools_amd.so through the C ABI.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Optional, Sequence

from . import _abi
from ._abi import DTYPES, check, i64_array, lib


def _torch():
    import torch
    return torch


def torch_dtype(name: str):
    torch = _torch()
    return {
        "bool": torch.uint8, "int8": torch.int8, "int16": torch.int16, "int32": torch.int32,
        "int64": torch.int64, "uint8": torch.uint8, "uint16": torch.uint16,
        "uint32": torch.uint32, "uint64": torch.uint64, "bfloat16": torch.bfloat16,
        "float16": torch.float16, "float32": torch.float32, "float64": torch.float64,
    }[name]


def dtype_of(t) -> str:
    torch = _torch()
    m = {torch.int8: "int8", torch.int16: "int16", torch.int32: "int32", torch.int64: "int64",
         torch.uint8: "uint8", torch.uint16: "uint16", torch.uint32: "uint32",
         torch.uint64: "uint64", torch.bfloat16: "bfloat16", torch.float16: "float16",
         torch.float32: "float32", torch.float64: "float64", torch.bool: "bool"}
    return m[t.dtype]


class Context:
    """One HIP stream + scratch per (host thread, device) (zt_ctx)."""

    def __init__(self, device: int = 0, stream=None):
        h = ctypes.c_void_p()
        check(lib().zt_ctx_create(int(device), ctypes.byref(h)))
        self._h = h
        self.device = device
        if stream is not None:
            self.set_stream(stream)

    @property
    def handle(self):
        return self._h

    def set_stream(self, stream) -> None:
        """Run subsequent work on `stream` (a torch stream or a raw HIP stream handle). After a
        switch to a different stream, everything the context issues is ordered after everything it
        issued before the switch. A call that sets the stream it already has does nothing."""
        ptr = getattr(stream, "cuda_stream", stream)
        check(lib().zt_ctx_set_stream(self._h, ctypes.c_void_p(ptr)))

    def synchronize(self) -> None:
        check(lib().zt_ctx_synchronize(self._h))

    def scratch_bytes(self) -> int:
        n = ctypes.c_uint64()
        check(lib().zt_ctx_scratch_bytes(self._h, ctypes.byref(n)))
        return int(n.value)

    def release_scratch(self) -> None:
        """Free the device scratch the context keeps between calls."""
        check(lib().zt_ctx_release_scratch(self._h))

    def last_kernel_ms(self) -> float:
        ms = ctypes.c_float()
        check(lib().zt_ctx_last_kernel_ms(self._h, ctypes.byref(ms)))
        return float(ms.value)

    def chunk_occupancy(self, x, cell_shape=None, fill_value=0):
        """chunk_occupancy(x, cell_shape, fill_value) on this context."""
        return chunk_occupancy(x, cell_shape, fill_value, ctx=self)

    def close(self) -> None:
        if self._h:
            lib().zt_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx: dict[int, Context] = {}


def default_context(device: Optional[int] = None) -> Context:
    torch = _torch()
    if device is None:
        device = torch.cuda.current_device()
    ctx = _default_ctx.get(device)
    if ctx is None:
        ctx = Context(device)
        _default_ctx[device] = ctx
    ctx.set_stream(torch.cuda.current_stream(device))
    return ctx


def _ptr(t) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr())


@dataclass
class ArraySubset:
    start: tuple
    shape: tuple

    @property
    def end_exc(self):
        return tuple(s + n for s, n in zip(self.start, self.shape))


class ArraySubsetOverlap:
    """array_subset_overlap.rs:4-52 (computed by zt_subset_overlap)."""

    def __init__(self, shape_src: Sequence[int], subset_src: ArraySubset,
                 overlap: Sequence[int]):
        nd = len(shape_src)
        istart, ishape, dst = i64_array([0] * nd), i64_array([0] * nd), i64_array([0] * nd)
        check(lib().zt_subset_overlap(i64_array(shape_src), nd, i64_array(subset_src.start),
                                      i64_array(subset_src.shape), i64_array(overlap), istart,
                                      ishape, dst))
        self._input = ArraySubset(tuple(istart[:nd]), tuple(ishape[:nd]))
        self._dst = ArraySubset(tuple(dst[:nd]), tuple(subset_src.shape))

    def subset_input(self) -> ArraySubset:
        return self._input

    def subset_dst_in_src(self) -> ArraySubset:
        return self._dst

    def extract_subset(self, array):
        sl = tuple(slice(s, e) for s, e in zip(self._dst.start, self._dst.end_exc))
        return array[sl].clone()


class DeviceArray:
    """A device-resident chunked array: the in-HBM analogue of zarrs::Array for this path."""

    def __init__(self, data, chunk_shape: Sequence[int], dtype: Optional[str] = None):
        self.data = data
        self.chunk_shape = tuple(int(c) for c in chunk_shape)
        self.dtype = dtype or dtype_of(data)

    @property
    def shape(self):
        return tuple(self.data.shape)

    def chunk_grid_shape(self):
        return tuple(-(-s // c) for s, c in zip(self.shape, self.chunk_shape))

    def chunk_occupancy(self, fill_value=0, cell_shape=None, ctx=None):
        """Which chunks (or cells of `cell_shape`) hold anything but `fill_value`
        (chunk_occupancy)."""
        return chunk_occupancy(self, cell_shape, fill_value, ctx=ctx)

    def chunk_subset_bounded(self, chunk_indices) -> ArraySubset:
        start = tuple(i * c for i, c in zip(chunk_indices, self.chunk_shape))
        shape = tuple(min(s + c, n) - s for s, c, n in zip(start, self.chunk_shape, self.shape))
        return ArraySubset(start, shape)


def _check_radius(radius: int) -> int:
    r = int(radius)
    if not 0 <= r <= 255:
        raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS, "radius is a u8")
    return r


class GuidedFilter:
    """guided_filter.rs:52-320 — `GuidedFilter::new(epsilon, radius, chunk_limit)`."""

    def __init__(self, epsilon: float, radius: int, chunk_limit: Optional[int] = None):
        self._epsilon = float(epsilon)
        self._radius = _check_radius(radius)
        self.chunk_limit = chunk_limit

    def epsilon(self) -> float:
        return self._epsilon

    def radius(self) -> int:
        return self._radius

    def name(self) -> str:
        return "guided_filter"

    def is_compatible(self, dtype_in: str, dtype_out: str) -> None:
        for d in (dtype_in, dtype_out):
            if d not in DTYPES:
                raise _abi.UnsupportedDataType(_abi.ERR_UNSUPPORTED_DATA_TYPE,
                                               f"Unsupported data type {d}")
        check(lib().zt_guided_filter_is_compatible(DTYPES[dtype_in], DTYPES[dtype_out]))

    def memory_per_chunk(self, dtype_in: str, dtype_out: str, chunk_shape) -> int:
        out = ctypes.c_uint64()
        check(lib().zt_guided_filter_memory_per_chunk(DTYPES[dtype_in], DTYPES[dtype_out],
                                                      i64_array(chunk_shape), len(chunk_shape),
                                                      ctypes.byref(out)))
        return int(out.value)

    def apply_ndarray(self, v, out_subset: Optional[ArraySubset] = None,
                      dtype_out: Optional[str] = None, ctx: Optional[Context] = None):
        """guided_filter.rs:117-164 (+ extract_subset and the `as` casts of apply_chunk).

        `v` is the (halo'd) device block. Returns the filtered `out_subset` of the block
        (the whole block by default) as `dtype_out` (default: the input's dtype)."""
        torch = _torch()
        ctx = ctx or default_context(v.device.index)
        dtype_in = dtype_of(v)
        dtype_out = dtype_out or dtype_in
        nd = v.dim()
        if out_subset is None:
            out_subset = ArraySubset((0,) * nd, tuple(v.shape))
        out = torch.empty(out_subset.shape, dtype=torch_dtype(dtype_out), device=v.device)
        in_strides = i64_array(v.stride())
        check(lib().zt_guided_filter_apply_ndarray(
            ctx.handle, DTYPES[dtype_in], _ptr(v), i64_array(v.shape), in_strides, nd,
            i64_array(out_subset.start), i64_array(out_subset.shape), DTYPES[dtype_out], _ptr(out),
            i64_array(out.stride()), self._epsilon, self._radius))
        return out

    def apply_chunk(self, input: DeviceArray, output: DeviceArray, chunk_indices,
                    ctx: Optional[Context] = None) -> None:
        """guided_filter.rs:75-114 on device-resident arrays: halo'd read, filter, interior
        write."""
        subset_output = output.chunk_subset_bounded(chunk_indices)
        overlap = ArraySubsetOverlap(input.shape, subset_output,
                                     [(self._radius * 2) & 0xFF] * len(input.shape))
        si = overlap.subset_input()
        block = input.data[tuple(slice(s, s + n) for s, n in zip(si.start, si.shape))]
        res = self.apply_ndarray(block, overlap.subset_dst_in_src(), output.dtype, ctx)
        output.data[tuple(slice(s, s + n) for s, n in
                          zip(subset_output.start, subset_output.shape))] = res

    def apply(self, input: DeviceArray, output: DeviceArray, ctx: Optional[Context] = None,
              chunk_grid_start=None, chunk_grid_count=None) -> None:
        """guided_filter.rs:240-319 over every output chunk (batched into one launch)."""
        if tuple(output.shape) != tuple(input.shape):
            raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                         "input and output shapes differ")
        ctx = ctx or default_context(input.data.device.index)
        nd = len(input.shape)
        check(lib().zt_guided_filter_apply_array(
            ctx.handle, DTYPES[input.dtype], _ptr(input.data), DTYPES[output.dtype],
            _ptr(output.data), i64_array(input.shape), nd, i64_array(output.chunk_shape),
            self._epsilon, self._radius,
            None if chunk_grid_start is None else i64_array(chunk_grid_start),
            None if chunk_grid_count is None else i64_array(chunk_grid_count)))


class Gaussian:
    """gaussian.rs:49-250 — `Gaussian::new(sigma, kernel_half_size, chunk_limit)`: the separable
    sampled Gaussian, per axis in order, replicate edges (kernel.rs:17-73)."""

    def __init__(self, sigma: Sequence[float], kernel_half_size: Sequence[int],
                 chunk_limit: Optional[int] = None):
        self.sigma = tuple(float(s) for s in sigma)
        self._half = tuple(int(h) for h in kernel_half_size)
        if len(self.sigma) != len(self._half):
            raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                         "sigma and kernel_half_size lengths differ")
        self.chunk_limit = chunk_limit

    def name(self) -> str:
        return "gaussian"

    def kernel_half_size(self) -> tuple:
        return self._half

    def kernel(self, axis: int) -> list:
        """create_sampled_gaussian_kernel (gaussian.rs:252-267) for one axis."""
        n = ctypes.c_int64()
        check(lib().zt_gaussian_kernel(self.sigma[axis], self._half[axis], None, ctypes.byref(n)))
        taps = (ctypes.c_float * n.value)()
        check(lib().zt_gaussian_kernel(self.sigma[axis], self._half[axis], taps, ctypes.byref(n)))
        return list(taps)

    def _args(self, nd: int):
        if len(self.sigma) != nd:
            raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                         "sigma / kernel_half_size must have one entry per axis")
        return (ctypes.c_float * nd)(*self.sigma), i64_array(self._half)

    def is_compatible(self, dtype_in: str, dtype_out: str) -> None:
        for d in (dtype_in, dtype_out):
            if d not in DTYPES:
                raise _abi.UnsupportedDataType(_abi.ERR_UNSUPPORTED_DATA_TYPE,
                                               f"Unsupported data type {d}")
        check(lib().zt_gaussian_is_compatible(DTYPES[dtype_in], DTYPES[dtype_out]))

    def memory_per_chunk(self, dtype_in: str, dtype_out: str, chunk_shape) -> int:
        out = ctypes.c_uint64()
        check(lib().zt_gaussian_memory_per_chunk(DTYPES[dtype_in], DTYPES[dtype_out],
                                                 i64_array(chunk_shape), len(chunk_shape),
                                                 i64_array(self._half), ctypes.byref(out)))
        return int(out.value)

    def apply_ndarray(self, v, out_subset: Optional[ArraySubset] = None,
                      dtype_out: Optional[str] = None, ctx: Optional[Context] = None):
        """gaussian.rs:110-119 (+ extract_subset and the `as` casts of apply_chunk) on a
        device block; returns `out_subset` of the result (whole block by default)."""
        torch = _torch()
        v = v.contiguous()
        ctx = ctx or default_context(v.device.index)
        dtype_in = dtype_of(v)
        dtype_out = dtype_out or dtype_in
        nd = v.dim()
        if out_subset is None:
            out_subset = ArraySubset((0,) * nd, tuple(v.shape))
        sig, half = self._args(nd)
        out = torch.empty(out_subset.shape, dtype=torch_dtype(dtype_out), device=v.device)
        check(lib().zt_gaussian_apply_ndarray(
            ctx.handle, DTYPES[dtype_in], _ptr(v), i64_array(v.shape), nd,
            i64_array(out_subset.start), i64_array(out_subset.shape), DTYPES[dtype_out],
            _ptr(out), sig, half))
        return out

    def apply_chunk(self, input: DeviceArray, output: DeviceArray, chunk_indices,
                    ctx: Optional[Context] = None) -> None:
        """gaussian.rs:73-108 on device-resident arrays."""
        subset_output = output.chunk_subset_bounded(chunk_indices)
        overlap = ArraySubsetOverlap(input.shape, subset_output, self._half)
        si = overlap.subset_input()
        block = input.data[tuple(slice(s, s + n) for s, n in zip(si.start, si.shape))]
        res = self.apply_ndarray(block, overlap.subset_dst_in_src(), output.dtype, ctx)
        output.data[tuple(slice(s, s + n) for s, n in
                          zip(subset_output.start, subset_output.shape))] = res

    def apply(self, input: DeviceArray, output: DeviceArray,
              ctx: Optional[Context] = None) -> None:
        """gaussian.rs:170-249 over every output chunk (one pass over the array)."""
        if tuple(output.shape) != tuple(input.shape):
            raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                         "input and output shapes differ")
        ctx = ctx or default_context(input.data.device.index)
        nd = len(input.shape)
        sig, half = self._args(nd)
        check(lib().zt_gaussian_apply_array(
            ctx.handle, DTYPES[input.dtype], _ptr(input.data.contiguous()), DTYPES[output.dtype],
            _ptr(output.data), i64_array(input.shape), nd, i64_array(output.chunk_shape), sig,
            half))


def gm_operator(operator: str) -> int:
    """GradientMagnitudeOperator (gradient_magnitude.rs:24-29) as the ABI's ZT_GM_* code."""
    op = _abi.GM_OPERATORS.get(str(operator).replace("-", "_").lower())
    if op is None:
        raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                     f"unknown gradient magnitude operator {operator!r} "
                                     "(sobel or central_difference)")
    return op


class GradientMagnitude:
    """gradient_magnitude.rs:55-275 — `GradientMagnitude::new(operator, chunk_limit)`: per axis
    the triangle / difference passes (kernel.rs:75-129), sqrt of the summed squares."""

    def __init__(self, operator: str = "sobel", chunk_limit: Optional[int] = None):
        self._op = gm_operator(operator)
        self.operator = {v: k for k, v in _abi.GM_OPERATORS.items()}[self._op]
        self.chunk_limit = chunk_limit

    def name(self) -> str:
        return "gradient_magnitude"

    def is_compatible(self, dtype_in: str, dtype_out: str) -> None:
        for d in (dtype_in, dtype_out):
            if d not in DTYPES:
                raise _abi.UnsupportedDataType(_abi.ERR_UNSUPPORTED_DATA_TYPE,
                                               f"Unsupported data type {d}")
        check(lib().zt_gradient_magnitude_is_compatible(DTYPES[dtype_in], DTYPES[dtype_out]))

    def memory_per_chunk(self, dtype_in: str, dtype_out: str, chunk_shape) -> int:
        out = ctypes.c_uint64()
        check(lib().zt_gradient_magnitude_memory_per_chunk(
            DTYPES[dtype_in], DTYPES[dtype_out], i64_array(chunk_shape), len(chunk_shape),
            ctypes.byref(out)))
        return int(out.value)

    def apply_ndarray(self, v, out_subset: Optional[ArraySubset] = None,
                      dtype_out: Optional[str] = None, ctx: Optional[Context] = None):
        """gradient_magnitude.rs:109-147 (+ extract_subset and the `as` casts of apply_chunk) on
        a device block; returns `out_subset` of the result (whole block by default)."""
        torch = _torch()
        v = v.contiguous()
        ctx = ctx or default_context(v.device.index)
        dtype_in = dtype_of(v)
        dtype_out = dtype_out or dtype_in
        nd = v.dim()
        if out_subset is None:
            out_subset = ArraySubset((0,) * nd, tuple(v.shape))
        out = torch.empty(out_subset.shape, dtype=torch_dtype(dtype_out), device=v.device)
        check(lib().zt_gradient_magnitude_apply_ndarray(
            ctx.handle, DTYPES[dtype_in], _ptr(v), i64_array(v.shape), nd,
            i64_array(out_subset.start), i64_array(out_subset.shape), DTYPES[dtype_out],
            _ptr(out), self._op))
        return out

    def apply_chunk(self, input: DeviceArray, output: DeviceArray, chunk_indices,
                    ctx: Optional[Context] = None) -> None:
        """gradient_magnitude.rs:68-107 on device-resident arrays."""
        subset_output = output.chunk_subset_bounded(chunk_indices)
        overlap = ArraySubsetOverlap(input.shape, subset_output, [1] * len(input.shape))
        si = overlap.subset_input()
        block = input.data[tuple(slice(s, s + n) for s, n in zip(si.start, si.shape))]
        res = self.apply_ndarray(block, overlap.subset_dst_in_src(), output.dtype, ctx)
        output.data[tuple(slice(s, s + n) for s, n in
                          zip(subset_output.start, subset_output.shape))] = res

    def apply(self, input: DeviceArray, output: DeviceArray,
              ctx: Optional[Context] = None) -> None:
        """gradient_magnitude.rs:197-274 over every output chunk (one pass over the array)."""
        if tuple(output.shape) != tuple(input.shape):
            raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                         "input and output shapes differ")
        ctx = ctx or default_context(input.data.device.index)
        nd = len(input.shape)
        check(lib().zt_gradient_magnitude_apply_array(
            ctx.handle, DTYPES[input.dtype], _ptr(input.data.contiguous()), DTYPES[output.dtype],
            _ptr(output.data), i64_array(input.shape), nd, i64_array(output.chunk_shape),
            self._op))


def rank_kind(kind) -> int:
    """A rank filter's kind ("minimum", "median", "maximum") as the ABI's ZT_RANK_* code."""
    code = _abi.RANK_KINDS.get(str(kind).lower())
    if code is None:
        raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                     f"unknown rank filter {kind!r} (minimum, median or maximum)")
    return code


def check_rank_half(kind: str, half, ndim: Optional[int] = None) -> None:
    """The limits of a rank filter's kernel_half_size: one non-negative entry per axis, and a
    median window of at most 4096 entries."""
    if ndim is not None and len(half) != ndim:
        raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                     f"{kind} kernel_half_size needs one entry per axis")
    if any(h < 0 for h in half):
        raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                     f"{kind}: negative kernel_half_size")
    if kind == "median" and math.prod(2 * h + 1 for h in half) > _abi.RANK_MEDIAN_MAX_WINDOW:
        raise _abi.InvalidParameters(
            _abi.ERR_INVALID_PARAMETERS,
            f"median window of more than {_abi.RANK_MEDIAN_MAX_WINDOW} elements")


class RankFilter:
    """`RankFilter(kind, kernel_half_size, chunk_limit)`: the minimum, median or maximum of the
    window of half sizes kernel_half_size around every element, replicate edges (an extension:
    the reference has no such filter). The result is one of the window's
    elements, bit for bit, under a total order (floats: -NaN < -inf < ... < -0.0 < +0.0 < ... <
    +inf < +NaN); another output type is its `as` cast."""

    def __init__(self, kind: str, kernel_half_size: Sequence[int],
                 chunk_limit: Optional[int] = None):
        self._kind = rank_kind(kind)
        self.kind = str(kind).lower()
        self._half = tuple(int(h) for h in kernel_half_size)
        check_rank_half(self.kind, self._half)
        self.chunk_limit = chunk_limit

    def name(self) -> str:
        return self.kind

    def kernel_half_size(self) -> tuple:
        return self._half

    def _args(self, nd: int):
        check_rank_half(self.kind, self._half, nd)
        return i64_array(self._half)

    def is_compatible(self, dtype_in: str, dtype_out: str) -> None:
        for d in (dtype_in, dtype_out):
            if d not in DTYPES:
                raise _abi.UnsupportedDataType(_abi.ERR_UNSUPPORTED_DATA_TYPE,
                                               f"Unsupported data type {d}")
        check(lib().zt_rank_filter_is_compatible(DTYPES[dtype_in], DTYPES[dtype_out]))

    def memory_per_chunk(self, dtype_in: str, dtype_out: str, chunk_shape) -> int:
        out = ctypes.c_uint64()
        half = self._args(len(chunk_shape))
        check(lib().zt_rank_filter_memory_per_chunk(DTYPES[dtype_in], DTYPES[dtype_out],
                                                    i64_array(chunk_shape), len(chunk_shape),
                                                    half, ctypes.byref(out)))
        return int(out.value)

    def apply_ndarray(self, v, out_subset: Optional[ArraySubset] = None,
                      dtype_out: Optional[str] = None, ctx: Optional[Context] = None):
        """The filter of a device block, edges clamped at the block's bounds; returns
        `out_subset` of the result (whole block by default) as dtype_out (default: the
        input's)."""
        torch = _torch()
        v = v.contiguous()
        ctx = ctx or default_context(v.device.index)
        dtype_in = dtype_of(v)
        dtype_out = dtype_out or dtype_in
        nd = v.dim()
        if out_subset is None:
            out_subset = ArraySubset((0,) * nd, tuple(v.shape))
        half = self._args(nd)
        out = torch.empty(out_subset.shape, dtype=torch_dtype(dtype_out), device=v.device)
        check(lib().zt_rank_filter_apply_ndarray(
            ctx.handle, DTYPES[dtype_in], _ptr(v), i64_array(v.shape), nd,
            i64_array(out_subset.start), i64_array(out_subset.shape), DTYPES[dtype_out],
            _ptr(out), self._kind, half))
        return out

    def apply_chunk(self, input: DeviceArray, output: DeviceArray, chunk_indices,
                    ctx: Optional[Context] = None) -> None:
        """One output chunk from the input chunk plus a halo of kernel_half_size clamped to the
        array (ArraySubsetOverlap), on device-resident arrays."""
        subset_output = output.chunk_subset_bounded(chunk_indices)
        overlap = ArraySubsetOverlap(input.shape, subset_output, self._half)
        si = overlap.subset_input()
        block = input.data[tuple(slice(s, s + n) for s, n in zip(si.start, si.shape))]
        res = self.apply_ndarray(block, overlap.subset_dst_in_src(), output.dtype, ctx)
        output.data[tuple(slice(s, s + n) for s, n in
                          zip(subset_output.start, subset_output.shape))] = res

    def apply(self, input: DeviceArray, output: DeviceArray,
              ctx: Optional[Context] = None) -> None:
        """Every output chunk (one pass over the array)."""
        if tuple(output.shape) != tuple(input.shape):
            raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                         "input and output shapes differ")
        ctx = ctx or default_context(input.data.device.index)
        nd = len(input.shape)
        half = self._args(nd)
        check(lib().zt_rank_filter_apply_array(
            ctx.handle, DTYPES[input.dtype], _ptr(input.data.contiguous()), DTYPES[output.dtype],
            _ptr(output.data), i64_array(input.shape), nd, i64_array(output.chunk_shape),
            self._kind, half))


class Median(RankFilter):
    """`Median(kernel_half_size)`: the entry of rank (N - 1) / 2 of the sorted window."""

    def __init__(self, kernel_half_size: Sequence[int], chunk_limit: Optional[int] = None):
        super().__init__("median", kernel_half_size, chunk_limit)


class Minimum(RankFilter):
    """`Minimum(kernel_half_size)`: grey-scale erosion by the box of half sizes h."""

    def __init__(self, kernel_half_size: Sequence[int], chunk_limit: Optional[int] = None):
        super().__init__("minimum", kernel_half_size, chunk_limit)


class Maximum(RankFilter):
    """`Maximum(kernel_half_size)`: grey-scale dilation by the box of half sizes h."""

    def __init__(self, kernel_half_size: Sequence[int], chunk_limit: Optional[int] = None):
        super().__init__("maximum", kernel_half_size, chunk_limit)


class SummedAreaTable:
    """summed_area_table.rs:38-254 — `SummedAreaTable::new(chunk_limit)`: an inclusive running
    sum along every axis, last axis first, in the output type (integers wrap; floats keep the
    reference's left-to-right order, one rounding per add)."""

    def __init__(self, chunk_limit: Optional[int] = None):
        self.chunk_limit = chunk_limit

    def name(self) -> str:
        return "summed area table"

    def is_compatible(self, dtype_in: str, dtype_out: str) -> None:
        for d in (dtype_in, dtype_out):
            if d not in DTYPES:
                raise _abi.UnsupportedDataType(_abi.ERR_UNSUPPORTED_DATA_TYPE,
                                               f"Unsupported data type {d}")
        check(lib().zt_summed_area_table_is_compatible(DTYPES[dtype_in], DTYPES[dtype_out]))

    def memory_per_chunk(self, dtype_in: str, dtype_out: str, chunk_shape) -> int:
        out = ctypes.c_uint64()
        check(lib().zt_summed_area_table_memory_per_chunk(
            DTYPES[dtype_in], DTYPES[dtype_out], i64_array(chunk_shape), len(chunk_shape),
            ctypes.byref(out)))
        return int(out.value)

    def apply_ndarray(self, v, dtype_out: Optional[str] = None, ctx: Optional[Context] = None,
                      carry=None):
        """summed_area_table.rs:47-106 for every axis on a device block; returns the table as
        `dtype_out` (the input's type by default). `carry`: None, or a contiguous device tensor
        of v.shape[1:] in the output type: the seed plane of the axis-0 sum on entry (the
        reference's sum_last between chunks), the last output plane on return."""
        torch = _torch()
        v = v.contiguous()
        ctx = ctx or default_context(v.device.index)
        dtype_in = dtype_of(v)
        dtype_out = dtype_out or dtype_in
        out = torch.empty(tuple(v.shape), dtype=torch_dtype(dtype_out), device=v.device)
        if carry is not None:
            if (tuple(carry.shape) != tuple(v.shape[1:]) or carry.dtype != out.dtype
                    or carry.device != v.device or not carry.is_contiguous()):
                raise _abi.InvalidParameters(
                    _abi.ERR_INVALID_PARAMETERS,
                    "carry must be a contiguous device tensor of the block's shape[1:] in the "
                    "output type")
        check(lib().zt_summed_area_table_apply_ndarray(
            ctx.handle, DTYPES[dtype_in], _ptr(v), i64_array(v.shape), v.dim(),
            DTYPES[dtype_out], _ptr(out), None if carry is None else _ptr(carry)))
        return out

    def apply(self, input: DeviceArray, output: DeviceArray,
              ctx: Optional[Context] = None) -> None:
        """summed_area_table.rs:144-253 over a device-resident array (one pass per axis; the
        chunk grid does not enter the result)."""
        if tuple(output.shape) != tuple(input.shape):
            raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                         "input and output shapes differ")
        ctx = ctx or default_context(input.data.device.index)
        check(lib().zt_summed_area_table_apply_array(
            ctx.handle, DTYPES[input.dtype], _ptr(input.data.contiguous()),
            DTYPES[output.dtype], _ptr(output.data), i64_array(input.shape), len(input.shape),
            i64_array(output.chunk_shape)))


def _invalid(msg: str):
    return _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS, msg)


_INT_BITS = {"int8": 8, "int16": 16, "int32": 32, "int64": 64,
             "uint8": 8, "uint16": 16, "uint32": 32, "uint64": 64}


def element_bits(value, dtype: str) -> int:
    """A `value` / `replace` argument (the fill_value grammar of parse_fill_value: a JSON number,
    true / false, "NaN", "Infinity", "-Infinity") as an element of `dtype`, the way
    fill_value_from_metadata reads it: its storage bits, zero-extended (zt_pointwise_op's element
    immediates). A value the type cannot hold (300 for uint8, 1.5 or "NaN" for an integer type,
    a number for bool) raises InvalidParameters; the reference panics there. A float16 / bfloat16
    value is rounded once from the f64, as half's from_f64 does (`f64 as f16` of the kernels)."""
    import numpy as np
    if dtype not in DTYPES:
        raise _abi.UnsupportedDataType(_abi.ERR_UNSUPPORTED_DATA_TYPE,
                                       f"Unsupported data type {dtype}")
    bad = _invalid(f"value {value!r} is not compatible with data type {dtype}")
    if dtype == "bool":
        if not isinstance(value, bool):
            raise bad
        return int(value)
    if isinstance(value, bool):
        raise bad
    if dtype in _INT_BITS:
        if isinstance(value, float) and value.is_integer():
            value = int(value)
        if not isinstance(value, int):
            raise bad
        bits = _INT_BITS[dtype]
        lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if dtype[0] == "i" else (
            0, (1 << bits) - 1)
        if not lo <= value <= hi:
            raise bad
        return value & ((1 << bits) - 1)
    if isinstance(value, str):
        if value not in ("NaN", "Infinity", "-Infinity"):
            raise bad
        x = {"NaN": math.nan, "Infinity": math.inf, "-Infinity": -math.inf}[value]
    elif isinstance(value, (int, float)):
        x = float(value)
    else:
        raise bad
    if dtype == "float64":
        return _f64_bits(x)
    if dtype == "float32":
        with np.errstate(all="ignore"):
            return int(np.float32(x).view(np.uint32))
    return _half_from_f64(x, dtype == "bfloat16")


def _half_from_f64(x: float, bf16: bool) -> int:
    """half 2.6.0's f16::from_f64 / bf16::from_f64 (f64_to_f16_bits / f64_to_bf16_bits of
    csrc/zt_device.hpp, the kernel's `f64 as f16`): one rounding to nearest even, decided on the
    upper 32 bits of the f64, never through f32."""
    val = _f64_bits(x)
    hi, lo = val >> 32, val & 0xFFFFFFFF
    sign, exp, man = hi & 0x80000000, hi & 0x7FF00000, hi & 0x000FFFFF
    ebits, mbits, bias = (8, 7, 127) if bf16 else (5, 10, 15)
    shift = 20 - mbits  # mantissa bits of the upper word that are dropped
    inf = ((1 << ebits) - 1) << mbits
    if exp == 0x7FF00000:
        nan_bit = 0 if (man == 0 and lo == 0) else 1 << (mbits - 1)
        return (sign >> 16) | inf | nan_bit | (man >> shift)
    half_sign = sign >> 16
    half_exp = (exp >> 20) - 1023 + bias
    if half_exp >= (1 << ebits) - 1:
        return half_sign | inf
    if half_exp <= 0:
        if shift - half_exp > 21:
            return half_sign
        m = man | 0x00100000
        half_man = m >> (shift + 1 - half_exp)
        round_bit = 1 << (shift - half_exp)
        if (m & round_bit) and (m & (3 * round_bit - 1)):
            half_man += 1
        return half_sign | half_man
    r = half_sign | (half_exp << mbits) | (man >> shift)
    round_bit = 1 << (shift - 1)
    if (man & round_bit) and (man & (3 * round_bit - 1)):
        r += 1
    return r & 0xFFFF


def _f64_bits(x: float) -> int:
    import struct
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


class _Pointwise:
    """The operator surface the per-element filters share (FilterTraits, filter_traits.rs): `name`,
    `is_compatible`, `memory_per_chunk`, `output_shape`, `output_data_type`, `apply_ndarray`,
    `apply`; `op` is the filter as one zt_pointwise_op between two element types."""

    kind = _abi.PW_REENCODE
    _name = ""

    def name(self) -> str:
        return self._name

    def is_compatible(self, dtype_in: str, dtype_out: str) -> None:
        for d in (dtype_in, dtype_out):
            if d not in DTYPES:
                raise _abi.UnsupportedDataType(_abi.ERR_UNSUPPORTED_DATA_TYPE,
                                               f"Unsupported data type {d}")
        check(lib().zt_pointwise_is_compatible(self.kind, DTYPES[dtype_in], DTYPES[dtype_out]))

    def memory_per_chunk(self, dtype_in: str, dtype_out: str, chunk_shape) -> int:
        out = ctypes.c_uint64()
        check(lib().zt_pointwise_memory_per_chunk(self.kind, DTYPES[dtype_in], DTYPES[dtype_out],
                                                  i64_array(chunk_shape), len(chunk_shape),
                                                  ctypes.byref(out)))
        return int(out.value)

    def output_shape(self, input_shape) -> tuple:
        return tuple(int(s) for s in input_shape)

    def output_data_type(self, dtype_in: str):
        """(data type, fill value) when the filter sets the output type itself, else None."""
        return None

    def crop_box(self, input_shape):
        """(offset, shape) of the input box the output reads, None for the whole array."""
        return None

    def _imm(self, dtype_in: str, dtype_out: str):
        return 0, 0, 0

    def op(self, dtype_in: str, dtype_out: str) -> "_abi.PointwiseOp":
        self.is_compatible(dtype_in, dtype_out)
        imm0, imm1, flags = self._imm(dtype_in, dtype_out)
        return _abi.PointwiseOp(self.kind, DTYPES[dtype_out], imm0, imm1, flags, 0)

    def apply_ndarray(self, v, dtype_out: Optional[str] = None, ctx: Optional[Context] = None):
        """The filter's element work on a device block (the box of `crop_box` for a crop);
        returns a new tensor of `dtype_out` (default: the filter's own output type, else the
        input's)."""
        dtype_in = dtype_of(v)
        auto = self.output_data_type(dtype_in)
        dtype_out = dtype_out or (auto[0] if auto else dtype_in)
        return PointwiseProgram([self], dtype_in, [dtype_out], v.shape).apply_ndarray(v, ctx)

    def apply(self, input: DeviceArray, output: DeviceArray,
              ctx: Optional[Context] = None) -> None:
        """The filter's `apply` over a device-resident array: one launch."""
        PointwiseProgram([self], input.dtype, [output.dtype], input.shape).run(
            input.data, output.data, ctx)


class Reencode(_Pointwise):
    """reencode.rs:35-219 — `Reencode::new(chunk_limit)`: every element `as` the output type."""
    _name = "reencode"

    def __init__(self, chunk_limit: Optional[int] = None):
        self.chunk_limit = chunk_limit


class Crop(_Pointwise):
    """crop.rs:46-248 — `Crop::new(offset, shape, chunk_limit)`: output element i is input
    element offset + i, `as` the output type; the output has `shape`."""
    _name = "crop"

    def __init__(self, offset: Sequence[int], shape: Sequence[int],
                 chunk_limit: Optional[int] = None):
        self.offset = tuple(int(o) for o in offset)
        self.shape = tuple(int(s) for s in shape)
        if any(o < 0 for o in self.offset) or any(s < 0 for s in self.shape):
            raise _invalid("crop offset and shape are unsigned")
        self.chunk_limit = chunk_limit

    def crop_box(self, input_shape):
        nd = len(input_shape)
        if len(self.offset) != nd or len(self.shape) != nd:
            raise _invalid(f"crop offset and shape need one entry per axis ({nd})")
        for o, s, n in zip(self.offset, self.shape, input_shape):
            if o + s > n:
                raise _invalid(f"crop offset {list(self.offset)} + shape {list(self.shape)} "
                               f"is beyond the input {list(input_shape)}")
        return self.offset, self.shape

    def output_shape(self, input_shape) -> tuple:
        """Crop::output_shape (crop.rs:160-162)."""
        return self.crop_box(input_shape)[1]


class Rescale(_Pointwise):
    """rescale.rs:51-240 — `Rescale::new(multiply, add, add_first, chunk_limit)`: in f64,
    fma(v, multiply, add) (one rounding), or (v + add) * multiply with add_first."""
    kind = _abi.PW_RESCALE
    _name = "rescale"

    def __init__(self, multiply: float, add: float, add_first: bool = False,
                 chunk_limit: Optional[int] = None):
        self.multiply, self.add, self.add_first = float(multiply), float(add), bool(add_first)
        self.chunk_limit = chunk_limit

    def _imm(self, dtype_in, dtype_out):
        return (_f64_bits(self.multiply), _f64_bits(self.add),
                _abi.PW_ADD_FIRST if self.add_first else 0)


class Clamp(_Pointwise):
    """clamp.rs:44-212 — `Clamp::new(min, max, chunk_limit)`: num_traits::clamp between
    `min as TIn` and `max as TIn`, then `as` the output type."""
    kind = _abi.PW_CLAMP
    _name = "clamp"

    def __init__(self, min: float, max: float, chunk_limit: Optional[int] = None):
        self.min, self.max = float(min), float(max)
        self.chunk_limit = chunk_limit

    def _imm(self, dtype_in, dtype_out):
        return _f64_bits(self.min), _f64_bits(self.max), 0


class Equal(_Pointwise):
    """equal.rs:52-215 — `Equal::new(value, chunk_limit)`: (v == value) as bool or uint8; a NaN
    `value` equals nothing."""
    kind = _abi.PW_EQUAL
    _name = "equal"

    def __init__(self, value, chunk_limit: Optional[int] = None):
        self.value = value
        self.chunk_limit = chunk_limit

    def output_data_type(self, dtype_in: str):
        """Equal::output_data_type (equal.rs:121-123): bool with fill value false."""
        return "bool", False

    def _imm(self, dtype_in, dtype_out):
        return element_bits(self.value, dtype_in), 0, 0


class ReplaceValue(_Pointwise):
    """replace_value.rs:63-241 — `ReplaceValue::new(value, replace, chunk_limit)`:
    v == value ? replace : v as the output type (`value` in the input type, `replace` in the
    output type); a NaN `value` replaces nothing."""
    kind = _abi.PW_REPLACE_VALUE
    _name = "replace_value"

    def __init__(self, value, replace, chunk_limit: Optional[int] = None):
        self.value, self.replace = value, replace
        self.chunk_limit = chunk_limit

    def _imm(self, dtype_in, dtype_out):
        return element_bits(self.value, dtype_in), element_bits(self.replace, dtype_out), 0


POINTWISE = {"reencode": Reencode, "crop": Crop, "rescale": Rescale, "clamp": Clamp,
             "equal": Equal, "replace_value": ReplaceValue}


class PointwiseProgram:
    """Consecutive per-element filters as one launch (zt_pointwise_apply_ndarray): filter k reads
    the type filter k-1 wrote (`dtype_in` for the first) and writes dtypes_out[k]; crops compose
    by adding their offsets, since per-element ops commute with the selection. At most
    PW_MAX_OPS (8) filters."""

    def __init__(self, filters: Sequence[_Pointwise], dtype_in: str, dtypes_out: Sequence[str],
                 input_shape: Sequence[int]):
        if not 1 <= len(filters) <= _abi.PW_MAX_OPS or len(filters) != len(dtypes_out):
            raise _invalid(f"a pointwise program has 1 to {_abi.PW_MAX_OPS} filters, each with "
                           "its output type")
        self.dtype_in = dtype_in
        self.dtype_out = dtypes_out[-1]
        self.input_shape = tuple(int(s) for s in input_shape)
        nd = len(self.input_shape)
        self.offset, self.shape = (0,) * nd, self.input_shape
        self.cropped = False
        ops, dt = [], dtype_in
        for f, dout in zip(filters, dtypes_out):
            box = f.crop_box(self.shape)
            if box is not None:
                self.offset = tuple(a + b for a, b in zip(self.offset, box[0]))
                self.shape = tuple(box[1])
                self.cropped = True
            ops.append(f.op(dt, dout))
            dt = dout
        self.ops = (_abi.PointwiseOp * len(ops))(*ops)
        self.n_ops = len(ops)

    def box(self):
        """(offset, shape) i64 arrays of the composed crop, or (None, None)."""
        if not self.cropped:
            return None, None
        return i64_array(self.offset), i64_array(self.shape)

    def run(self, x, y, ctx: Optional[Context] = None) -> None:
        """x (device tensor, input_shape, dtype_in) -> y (contiguous, the box's shape,
        dtype_out)."""
        if tuple(x.shape) != self.input_shape or tuple(y.shape) != tuple(self.shape):
            raise _invalid("pointwise program: array shapes differ from the program's")
        if not y.is_contiguous():
            raise _invalid("pointwise program: the output must be contiguous")
        x = x.contiguous()
        ctx = ctx or default_context(x.device.index)
        off, shp = self.box()
        check(lib().zt_pointwise_apply_ndarray(
            ctx.handle, DTYPES[self.dtype_in], _ptr(x), i64_array(self.input_shape),
            len(self.input_shape), off, shp, self.ops, self.n_ops, _ptr(y)))

    def apply_ndarray(self, v, ctx: Optional[Context] = None):
        torch = _torch()
        out = torch.empty(tuple(self.shape), dtype=torch_dtype(self.dtype_out), device=v.device)
        self.run(v, out, ctx)
        return out


def element_value(bits: int, dtype: str):
    """An element given as its storage bits (zero-extended; the inverse of element_bits) as a
    Python value: integers as int, the float types widened exactly to f64 as float."""
    import struct
    if dtype in _INT_BITS:
        n = _INT_BITS[dtype]
        bits &= (1 << n) - 1
        return bits - (1 << n) if dtype[0] == "i" and bits >> (n - 1) else bits
    if dtype == "float64":
        return struct.unpack("<d", struct.pack("<Q", bits))[0]
    if dtype == "float32":
        return struct.unpack("<f", struct.pack("<I", bits & 0xFFFFFFFF))[0]
    if dtype == "float16":
        return struct.unpack("<e", struct.pack("<H", bits & 0xFFFF))[0]
    if dtype == "bfloat16":
        return struct.unpack("<f", struct.pack("<I", (bits & 0xFFFF) << 16))[0]
    raise _abi.UnsupportedDataType(_abi.ERR_UNSUPPORTED_DATA_TYPE,
                                   f"Unsupported data type {dtype}")


def _info_dtype(dtype: str) -> int:
    if dtype not in DTYPES:
        raise _abi.UnsupportedDataType(_abi.ERR_UNSUPPORTED_DATA_TYPE,
                                       f"Unsupported data type {dtype}")
    return DTYPES[dtype]


def _info_run(v):
    """(contiguous device tensor, data type name) of a tensor or DeviceArray."""
    if isinstance(v, DeviceArray):
        return v.data.contiguous(), v.dtype
    return v.contiguous(), dtype_of(v)


def _order_key(x):
    """Orders -0.0 below +0.0 (the kernels' key order); integers as they are."""
    return (x, math.copysign(1.0, x)) if isinstance(x, float) else (x, 0)


def combine_ranges(parts):
    """The range of the union of parts that each gave (min, max), (None, None) for a part with
    no non-NaN element: ranges fold."""
    los = [p[0] for p in parts if p[0] is not None]
    his = [p[1] for p in parts if p[1] is not None]
    if not los:
        return None, None
    return min(los, key=_order_key), max(his, key=_order_key)


def combine_histograms(parts):
    """The histogram of the union of parts that each gave (bin_edges, hist) for the same n_bins,
    min and max: histograms add."""
    import numpy as np
    parts = list(parts)
    if not parts:
        raise _invalid("combine_histograms: no parts")
    edges = np.asarray(parts[0][0], dtype=np.float64)
    hist = np.zeros(len(edges) - 1, dtype=np.uint64)
    for e, h in parts:
        if len(e) != len(edges) or not np.array_equal(np.asarray(e), edges):
            raise _invalid("combine_histograms: the parts' bin edges differ")
        hist += np.asarray(h, dtype=np.uint64)
    return edges, hist


class Range:
    """src/info/range.rs — calculate_range with the meaning its documentation gives it (the
    smallest and largest element; NaN ignored, -0.0 below +0.0, integers exact). The 12 numeric
    types; bool is UnsupportedDataType (`unimplemented!`, range.rs:92-95)."""

    def name(self) -> str:
        return "range"

    def is_compatible(self, dtype: str) -> None:
        check(lib().zt_range_is_compatible(_info_dtype(dtype)))

    def new_state(self, device=None, ctx: Optional[Context] = None):
        """An empty device state (16 bytes) that `accumulate` folds arrays into."""
        torch = _torch()
        state = torch.empty(2, dtype=torch.int64, device="cuda" if device is None else device)
        ctx = ctx or default_context(state.device.index)
        check(lib().zt_range_init(ctx.handle, _ptr(state)))
        return state

    def accumulate(self, v, state, ctx: Optional[Context] = None) -> None:
        x, dtype = _info_run(v)
        ctx = ctx or default_context(x.device.index)
        check(lib().zt_range_accumulate(ctx.handle, _info_dtype(dtype), _ptr(x), x.numel(),
                                        _ptr(state)))

    def finish(self, state, dtype: str, ctx: Optional[Context] = None):
        """(min, max) of everything folded into `state` as elements of `dtype`, or (None, None)."""
        ctx = ctx or default_context(state.device.index)
        lo, hi, none = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
        check(lib().zt_range_finish(ctx.handle, _info_dtype(dtype), _ptr(state), ctypes.byref(lo),
                                    ctypes.byref(hi), ctypes.byref(none)))
        if none.value:
            return None, None
        return element_value(lo.value, dtype), element_value(hi.value, dtype)

    def apply_ndarray(self, v, ctx: Optional[Context] = None):
        """(min, max) of a device tensor or DeviceArray; (None, None) when it has no non-NaN
        element."""
        x, dtype = _info_run(v)
        self.is_compatible(dtype)
        ctx = ctx or default_context(x.device.index)
        state = self.new_state(x.device, ctx)
        self.accumulate(v, state, ctx)
        return self.finish(state, dtype, ctx)


class Histogram:
    """src/info/histogram.rs — calculate_histogram(n_bins, min, max): per element, in f64,
    bin = min(floor(max((x - min) / (max - min) * n_bins, 0)), n_bins - 1) (:51-68). n_bins == 0
    and a non-finite min or max raise InvalidParameters."""

    def __init__(self, n_bins: int, min: float, max: float):
        self.n_bins, self.min, self.max = int(n_bins), float(min), float(max)
        self._edges = self._bin_edges()

    def name(self) -> str:
        return "histogram"

    def is_compatible(self, dtype: str) -> None:
        check(lib().zt_histogram_is_compatible(_info_dtype(dtype)))

    def _bin_edges(self):
        import numpy as np
        n = self.n_bins if 0 < self.n_bins <= (1 << 30) else 0
        edges = np.empty(n + 1, dtype=np.float64)
        check(lib().zt_histogram_bin_edges(
            self.n_bins, self.min, self.max,
            edges.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return edges

    def bin_edges(self):
        """histogram.rs:62-68: n_bins + 1 f64 edges."""
        return self._edges.copy()

    def new_state(self, device=None):
        """A zeroed device histogram (n_bins u64 counts, held as int64) for `accumulate`."""
        torch = _torch()
        return torch.zeros(self.n_bins, dtype=torch.int64,
                           device="cuda" if device is None else device)

    def accumulate(self, v, hist, ctx: Optional[Context] = None) -> None:
        x, dtype = _info_run(v)
        ctx = ctx or default_context(x.device.index)
        if hist.numel() != self.n_bins or not hist.is_contiguous() or hist.element_size() != 8:
            raise _invalid("histogram state: n_bins contiguous 8-byte counts")
        check(lib().zt_histogram_accumulate(ctx.handle, _info_dtype(dtype), _ptr(x), x.numel(),
                                            self.n_bins, self.min, self.max, _ptr(hist)))

    def finish(self, hist):
        """(bin_edges, hist as np.uint64) of a device state."""
        import numpy as np
        return self.bin_edges(), hist.cpu().numpy().view(np.uint64).copy()

    def apply_ndarray(self, v, ctx: Optional[Context] = None):
        """(bin_edges: np.float64[n_bins + 1], hist: np.uint64[n_bins]) of a device tensor or
        DeviceArray."""
        x, dtype = _info_run(v)
        self.is_compatible(dtype)
        hist = self.new_state(x.device)
        self.accumulate(v, hist, ctx)
        return self.finish(hist)


def fill_value_bits(fill_value, dtype: str) -> int:
    """The storage bits (zero-extended) of a fill value of `dtype`: a Zarr V3 fill_value (a JSON
    number, true / false, "NaN", "Infinity", "-Infinity", or the raw bits as "0x..." for a float
    type), read as element_bits reads a value."""
    if isinstance(fill_value, str) and fill_value[:2] in ("0x", "0X"):
        if dtype not in DTYPES:
            raise _abi.UnsupportedDataType(_abi.ERR_UNSUPPORTED_DATA_TYPE,
                                           f"Unsupported data type {dtype}")
        size = lib().zt_dtype_size(DTYPES[dtype])
        return int(fill_value, 16) & ((1 << (8 * size)) - 1)
    return element_bits(fill_value, dtype)


def chunk_occupancy(x, cell_shape: Optional[Sequence[int]] = None, fill_value=0,
                    ctx: Optional[Context] = None):
    """Which cells of a device tensor (or DeviceArray, whose chunk shape is the default cell
    shape) hold anything but the fill value: a uint8 device tensor of shape ceil(shape /
    cell_shape), 1 = some element's storage bits differ from the fill value's
    (zt_chunk_occupancy; what zarrs' store_empty_chunks = false tests per chunk). The cells tile
    the tensor from its origin. `fill_value` as fill_value_bits takes it."""
    torch = _torch()
    if isinstance(x, DeviceArray) and cell_shape is None:
        cell_shape = x.chunk_shape
    v, dtype = _info_run(x)
    if cell_shape is None or len(cell_shape) != v.dim():
        raise _invalid("chunk_occupancy: one cell extent per axis")
    cell = [int(c) for c in cell_shape]
    if any(c < 1 for c in cell):
        raise _invalid("chunk_occupancy: cell extents must be >= 1")
    bits = fill_value_bits(fill_value, dtype)
    grid = [-(-int(n) // c) for n, c in zip(v.shape, cell)]
    occ = torch.empty(grid, dtype=torch.uint8, device=v.device)
    ctx = ctx or default_context(v.device.index)
    check(lib().zt_chunk_occupancy(ctx.handle, _info_dtype(dtype), _ptr(v), i64_array(v.shape),
                                   v.dim(), i64_array(cell), bits, _ptr(occ)))
    return occ


def combine_compares(parts):
    """The comparison of the union of parts that each gave (n_diff, first_index | None) with
    indices in the whole array: counts add, the first index is the minimum."""
    parts = list(parts)
    firsts = [p[1] for p in parts if p[1] is not None]
    return sum(int(p[0]) for p in parts), (min(firsts) if firsts else None)


class Compare:
    """src/bin/zarrs_validate.rs:145-147 — `bytes_first == bytes_second`: two arrays of one shape
    and data type compared by their storage bits (a NaN equals a NaN with the same bits only,
    +0.0 differs from -0.0, bool is a byte). All 13 types. The result is (the number of differing
    elements, the C-order index of the first or None)."""

    def name(self) -> str:
        return "compare"

    def is_compatible(self, dtype_a: str, dtype_b: str) -> None:
        _info_dtype(dtype_a), _info_dtype(dtype_b)
        if dtype_a != dtype_b:  # zarrs_validate.rs:107-112
            raise _invalid(f"Array data types do not match: {dtype_a} vs {dtype_b}")

    def new_state(self, device=None, ctx: Optional[Context] = None):
        """An empty device state (16 bytes) that `accumulate` folds pairs of arrays into."""
        torch = _torch()
        state = torch.empty(2, dtype=torch.int64, device="cuda" if device is None else device)
        ctx = ctx or default_context(state.device.index)
        check(lib().zt_compare_init(ctx.handle, _ptr(state)))
        return state

    def _pair(self, a, b):
        """(contiguous a, contiguous b, data type) of two tensors or DeviceArrays of one shape,
        data type and device."""
        x, dtype = _info_run(a)
        y, dtype_b = _info_run(b)
        if tuple(x.shape) != tuple(y.shape):  # zarrs_validate.rs:101-106
            raise _invalid(f"Array shapes do not match: {list(x.shape)} vs {list(y.shape)}")
        self.is_compatible(dtype, dtype_b)
        if x.device != y.device:
            raise _invalid("compare: the two arrays are on different devices")
        return x, y, dtype

    def accumulate(self, a, b, state, base: int = 0, ctx: Optional[Context] = None) -> None:
        """Folds the pair into `state`; an element's index is `base` plus its C-order index in
        the pair."""
        x, y, dtype = self._pair(a, b)
        ctx = ctx or default_context(x.device.index)
        check(lib().zt_compare_accumulate(ctx.handle, _info_dtype(dtype), _ptr(x), _ptr(y),
                                          x.numel(), int(base), _ptr(state)))

    def finish(self, state, ctx: Optional[Context] = None):
        """(n_diff, first_index | None) of everything folded into `state`."""
        ctx = ctx or default_context(state.device.index)
        n_diff, first = ctypes.c_uint64(), ctypes.c_int64()
        check(lib().zt_compare_finish(ctx.handle, _ptr(state), ctypes.byref(n_diff),
                                      ctypes.byref(first)))
        return n_diff.value, (None if first.value < 0 else first.value)

    def apply_ndarray(self, a, b, ctx: Optional[Context] = None):
        """(n_diff, first_index | None) of two device tensors or DeviceArrays; InvalidParameters
        when their shapes or data types differ."""
        x, y, dtype = self._pair(a, b)
        ctx = ctx or default_context(x.device.index)
        state = self.new_state(x.device, ctx)
        check(lib().zt_compare_accumulate(ctx.handle, _info_dtype(dtype), _ptr(x), _ptr(y),
                                          x.numel(), 0, _ptr(state)))
        return self.finish(state, ctx)


ARITHMETIC_OPERATORS = tuple(_abi.AR_OPERATORS)


def arithmetic_operator(operator) -> int:
    """The ZT_AR_* code of an operator name (hyphens or underscores)."""
    key = str(operator).replace("-", "_")
    if key not in _abi.AR_OPERATORS:
        raise _invalid(f"arithmetic: unknown operator {operator!r} "
                       f"(one of {', '.join(ARITHMETIC_OPERATORS)})")
    return _abi.AR_OPERATORS[key]


class Arithmetic:
    """An extension with no counterpart in the reference: out = (first as f64
    `operator` second as f64) as TOut, element by element, for two arrays of one shape. All 13
    types for each of the three arrays; the default output type is the first array's."""

    def __init__(self, operator: str, chunk_limit: Optional[int] = None):
        self.op = arithmetic_operator(operator)
        self.operator = str(operator).replace("-", "_")
        self.chunk_limit = chunk_limit

    def name(self) -> str:
        return "arithmetic"

    def is_compatible(self, dtype_a: str, dtype_b: str, dtype_out: str) -> None:
        codes = [_info_dtype(d) for d in (dtype_a, dtype_b, dtype_out)]
        check(lib().zt_arithmetic_is_compatible(self.op, *codes))

    def memory_per_chunk(self, dtype_a: str, dtype_b: str, dtype_out: str, chunk_shape) -> int:
        out = ctypes.c_uint64()
        check(lib().zt_arithmetic_memory_per_chunk(
            self.op, DTYPES[dtype_a], DTYPES[dtype_b], DTYPES[dtype_out], i64_array(chunk_shape),
            len(chunk_shape), ctypes.byref(out)))
        return int(out.value)

    def _run(self, x, dtype_a, y, dtype_b, out, dtype_out, ctx) -> None:
        if tuple(x.shape) != tuple(y.shape):
            raise _invalid(f"Array shapes do not match: {list(x.shape)} vs {list(y.shape)}")
        if tuple(out.shape) != tuple(x.shape):
            raise _invalid(f"Array shapes do not match: {list(x.shape)} vs {list(out.shape)}")
        if x.device != y.device or x.device != out.device:
            raise _invalid("arithmetic: the arrays are on different devices")
        if not out.is_contiguous():
            raise _invalid("arithmetic: the output must be contiguous")
        self.is_compatible(dtype_a, dtype_b, dtype_out)
        ctx = ctx or default_context(x.device.index)
        check(lib().zt_arithmetic_apply(ctx.handle, self.op, DTYPES[dtype_a], _ptr(x),
                                        DTYPES[dtype_b], _ptr(y), x.numel(), DTYPES[dtype_out],
                                        _ptr(out)))

    def apply_ndarray(self, a, b, dtype_out: Optional[str] = None, ctx: Optional[Context] = None,
                      out=None):
        """first `operator` second on two device tensors of one shape; returns a new tensor of
        `dtype_out` (default: the first's type), or fills and returns `out` (contiguous, of
        `dtype_out`, not overlapping an input)."""
        x, dtype_a = _info_run(a)
        y, dtype_b = _info_run(b)
        dtype_out = dtype_out or (dtype_of(out) if out is not None else dtype_a)
        if out is None:
            out = _torch().empty(tuple(x.shape), dtype=torch_dtype(dtype_out), device=x.device)
        self._run(x, dtype_a, y, dtype_b, out, dtype_out, ctx)
        return out

    def apply(self, first: DeviceArray, second: DeviceArray, output: DeviceArray,
              ctx: Optional[Context] = None) -> None:
        """The filter's `apply` over device-resident arrays: one launch."""
        x, dtype_a = _info_run(first)
        y, dtype_b = _info_run(second)
        self._run(x, dtype_a, y, dtype_b, output.data, output.dtype, ctx)


CC_DEFAULT_DATA_TYPE = "uint32"


class ConnectedComponents:
    """An extension with no counterpart in the reference: every connected set of
    non-zero elements gets its own integer 1 .. K, background 0, components numbered in the C
    order of their first elements (scipy.ndimage.label's numbering). Two foreground elements are
    neighbours when their coordinates differ by at most 1 on every axis and on at most
    `connectivity` axes: 1 = faces (the default), the array's rank = the full neighbourhood. All
    13 types in; the eight integer types out, uint32 by default. Labelling is a whole-array
    operation (a component may span every chunk), so there is no per-chunk form."""

    def __init__(self, connectivity: int = 1):
        self.connectivity = int(connectivity)
        if self.connectivity < 1:
            raise _invalid(f"connected_components: connectivity {self.connectivity} not in "
                           "[1, rank]")

    def name(self) -> str:
        return "connected components"

    def check_connectivity(self, ndim: int) -> None:
        """InvalidParameters unless 1 <= connectivity <= ndim."""
        if not 1 <= self.connectivity <= int(ndim):
            raise _invalid(f"connected_components: connectivity {self.connectivity} not in "
                           f"[1, {int(ndim)}]")

    def is_compatible(self, dtype_in: str, dtype_out: str) -> None:
        check(lib().zt_connected_components_is_compatible(_info_dtype(dtype_in),
                                                          _info_dtype(dtype_out)))

    def memory(self, dtype_in: str, dtype_out: str, shape) -> int:
        """Device bytes of one call on an array of `shape`: input + scratch + output."""
        self.check_connectivity(len(shape))
        out = ctypes.c_uint64()
        check(lib().zt_connected_components_memory(
            _info_dtype(dtype_in), _info_dtype(dtype_out), i64_array(shape), len(shape),
            ctypes.byref(out)))
        return int(out.value)

    def _run(self, x, dtype_in, out, dtype_out, ctx) -> int:
        if tuple(out.shape) != tuple(x.shape):
            raise _invalid(f"Array shapes do not match: {list(x.shape)} vs {list(out.shape)}")
        if x.device != out.device:
            raise _invalid("connected_components: the arrays are on different devices")
        if not out.is_contiguous():
            raise _invalid("connected_components: the output must be contiguous")
        self.is_compatible(dtype_in, dtype_out)
        self.check_connectivity(x.dim())
        ctx = ctx or default_context(x.device.index)
        count = ctypes.c_uint64()
        check(lib().zt_connected_components_apply_array(
            ctx.handle, DTYPES[dtype_in], _ptr(x), DTYPES[dtype_out], _ptr(out),
            i64_array(x.shape), x.dim(), self.connectivity, ctypes.byref(count)))
        return int(count.value)

    def apply_ndarray(self, v, dtype_out: Optional[str] = None, ctx: Optional[Context] = None,
                      out=None):
        """Labels a device tensor; returns (labels, K). labels is a new tensor of `dtype_out`
        (default uint32), or `out` (contiguous, of `dtype_out`, not overlapping the input). When
        K does not fit `dtype_out` the call raises InvalidParameters and writes nothing."""
        x, dtype_in = _info_run(v)
        dtype_out = dtype_out or (dtype_of(out) if out is not None else CC_DEFAULT_DATA_TYPE)
        if out is None:
            self.is_compatible(dtype_in, dtype_out)
            out = _torch().empty(tuple(x.shape), dtype=torch_dtype(dtype_out), device=x.device)
        return out, self._run(x, dtype_in, out, dtype_out, ctx)

    def apply(self, input: DeviceArray, output: DeviceArray,
              ctx: Optional[Context] = None) -> int:
        """The filter's `apply` over device-resident arrays; returns K."""
        x, dtype_in = _info_run(input)
        return self._run(x, dtype_in, output.data, output.dtype, ctx)


def distance_transform_default_type(squared: bool) -> str:
    """float32 distances, uint32 squared distances (exact integers)."""
    return "uint32" if squared else "float32"


class DistanceTransform:
    """An extension with no counterpart in the reference: the exact Euclidean
    distance of every element to the nearest background element, background being what the
    labelling calls background (zero bits for bool and the integers, value == 0 for the floats).
    `spacing` is one integer >= 1 per axis, the length of a step along it (default all 1), and
    d2(p) = min over background q of sum_a spacing_a^2 (p_a - q_a)^2 is an integer: +inf everywhere
    when the array has no background. The output is sqrt(d2 as f64) as TOut (default float32),
    or with `squared` d2 itself (default uint32; saturated at an integer type's maximum, (d2 as
    f64) as TOut for a float type). All 13 types in, the 12 numeric types out. The transform is a
    whole-array operation (the nearest background may lie in any chunk): no per-chunk form."""

    def __init__(self, spacing=None, squared: bool = False):
        self.squared = bool(squared)
        self.spacing = None
        if spacing is not None:
            vals = []
            for s in spacing:
                try:
                    ok = not isinstance(s, bool) and int(s) == s and int(s) >= 1
                except (TypeError, ValueError):
                    ok = False
                if not ok:
                    raise _invalid(f"distance_transform: spacing {s!r} is not an integer >= 1")
                vals.append(int(s))
            self.spacing = tuple(vals)

    def name(self) -> str:
        return "distance transform"

    def check_spacing(self, ndim: int) -> None:
        """InvalidParameters unless the spacing has one entry per axis (or is the default)."""
        if self.spacing is not None and len(self.spacing) != int(ndim):
            raise _invalid(f"distance_transform: spacing {list(self.spacing)} has "
                           f"{len(self.spacing)} entries for an array of rank {int(ndim)}")

    def _spacing_arg(self):
        return i64_array(self.spacing) if self.spacing is not None else None

    def is_compatible(self, dtype_in: str, dtype_out: str) -> None:
        check(lib().zt_distance_transform_is_compatible(_info_dtype(dtype_in),
                                                        _info_dtype(dtype_out)))

    def memory(self, dtype_in: str, dtype_out: str, shape) -> int:
        """Device bytes of one call on an array of `shape`: input + scratch + output."""
        self.check_spacing(len(shape))
        out = ctypes.c_uint64()
        check(lib().zt_distance_transform_memory(
            _info_dtype(dtype_in), _info_dtype(dtype_out), i64_array(shape), self._spacing_arg(),
            len(shape), ctypes.byref(out)))
        return int(out.value)

    def _run(self, x, dtype_in, out, dtype_out, ctx) -> None:
        if tuple(out.shape) != tuple(x.shape):
            raise _invalid(f"Array shapes do not match: {list(x.shape)} vs {list(out.shape)}")
        if x.device != out.device:
            raise _invalid("distance_transform: the arrays are on different devices")
        if not out.is_contiguous():
            raise _invalid("distance_transform: the output must be contiguous")
        self.is_compatible(dtype_in, dtype_out)
        self.check_spacing(x.dim())
        ctx = ctx or default_context(x.device.index)
        check(lib().zt_distance_transform_apply_array(
            ctx.handle, DTYPES[dtype_in], _ptr(x), DTYPES[dtype_out], _ptr(out),
            i64_array(x.shape), self._spacing_arg(), x.dim(), int(self.squared)))

    def apply_ndarray(self, v, dtype_out: Optional[str] = None, ctx: Optional[Context] = None,
                      out=None):
        """Transforms a device tensor; returns a new tensor of `dtype_out` (default float32, or
        uint32 with `squared`), or `out` (contiguous, of `dtype_out`, not overlapping the input)."""
        x, dtype_in = _info_run(v)
        dtype_out = dtype_out or (dtype_of(out) if out is not None
                                  else distance_transform_default_type(self.squared))
        if out is None:
            self.is_compatible(dtype_in, dtype_out)
            out = _torch().empty(tuple(x.shape), dtype=torch_dtype(dtype_out), device=x.device)
        self._run(x, dtype_in, out, dtype_out, ctx)
        return out

    def apply(self, input: DeviceArray, output: DeviceArray,
              ctx: Optional[Context] = None) -> None:
        """The filter's `apply` over device-resident arrays."""
        x, dtype_in = _info_run(input)
        self._run(x, dtype_in, output.data, output.dtype, ctx)


_LABEL_TYPES = ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64")
# intensity types whose sums are kept (exact integers); the 64-bit and float types give None
LABEL_SUM_TYPES = ("int8", "int16", "int32", "uint8", "uint16", "uint32")


def _exact_quotient(num, den):
    """num / den per element as the correctly rounded f64 quotient of the two integers (Python's
    int / int); NaN where den == 0. num: an object array of Python ints, den: uint64."""
    import numpy as np
    out = np.full(num.shape, np.nan, dtype=np.float64)
    d = np.broadcast_to(den.reshape(den.shape + (1,) * (num.ndim - den.ndim)), num.shape)
    for i in np.ndindex(num.shape):
        if d[i]:
            out[i] = int(num[i]) / int(d[i])
    return out


def _quotient(num, den):
    """_exact_quotient, vectorised where both integers are below 2^53 in magnitude (f64 holds
    them, and IEEE division rounds correctly); the Python loop only for the entries beyond."""
    import numpy as np
    d = np.broadcast_to(den.reshape(den.shape + (1,) * (num.ndim - den.ndim)), num.shape)
    if num.size == 0:
        return np.full(num.shape, np.nan, dtype=np.float64)
    f = num.astype(np.float64)  # exact below 2^53; the entries beyond are redone as integers
    small = (np.abs(f) < 2.0 ** 53) & (d < np.uint64(2 ** 53))
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(d != 0, f / d.astype(np.float64), np.nan)
    rest = ~small & (d != 0)
    if rest.any():
        obj = num.astype(object)
        for i in zip(*np.nonzero(rest)):
            out[i] = int(obj[i]) / int(d[i])
    return out


def _sums_128(lo, hi):
    """The 128-bit two's complement sums (lo, hi: uint64 columns) as an object array of Python
    ints: one vectorised step where the sum fits an int64 (hi is the sign extension of lo), a loop
    over the others."""
    import numpy as np
    neg = lo >= np.uint64(1 << 63)
    fits = np.where(neg, hi == np.uint64(2 ** 64 - 1), hi == np.uint64(0))
    sums = lo.view(np.int64).astype(object)
    for i in np.flatnonzero(~fits):
        v = (int(hi[i]) << 64) | int(lo[i])
        sums[i] = v - (1 << 128) if v >> 127 else v
    return sums


def _keys_to_values(keys, dtype: str):
    """The elements whose orderable keys (include/zarrs_tools_amd.h) are `keys` (uint64), as a
    numpy array of `dtype` (bfloat16 widened exactly to float32)."""
    import numpy as np
    nbits = 8 * {"bfloat16": 2, "float16": 2, "float32": 4, "float64": 8}.get(
        dtype, _INT_BITS.get(dtype, 0) // 8)
    u = np.dtype(f"uint{nbits}")
    sign = np.uint64(1 << (nbits - 1))
    mask = np.uint64((1 << nbits) - 1)
    if dtype.startswith("uint"):
        return keys.astype(u)
    if dtype.startswith("int"):
        return (keys ^ sign).astype(u).view(np.dtype(f"int{nbits}"))
    bits = np.where((keys & sign) != 0, keys & ~sign, ~keys & mask).astype(u)
    if dtype == "bfloat16":
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return bits.view(np.dtype(f"float{nbits}"))


def _label_result(K, ndim, count, cmin, cmax, csum, total, intensity=None):
    """The result dict from the columns of labels 1 .. K. intensity: (dtype, valid, min, max,
    sums or None)."""
    import numpy as np
    present = count != 0
    res = {
        "n_labels": int(K),
        "background": int(total) - int(count.sum(dtype=np.uint64)),
        "count": count,
        "bbox_min": np.where(present[:, None], cmin.astype(np.int64), -1),
        "bbox_max": np.where(present[:, None], cmax.astype(np.int64), -1),
        "coord_sum": csum,
        "centroid": _quotient(csum, count),
    }
    if intensity is not None:
        dtype, valid, imin, imax, sums = intensity
        res["intensity_dtype"] = dtype
        res["intensity_valid"] = valid
        res["intensity_min"] = imin
        res["intensity_max"] = imax
        res["intensity_sum"] = sums
        res["intensity_mean"] = None if sums is None else _quotient(sums, count)
    return res


def combine_label_statistics(parts):
    """The statistics of the union of disjoint boxes that each gave a LabelStatistics result for
    the same n_labels (and intensity type): counts and sums add, minima and maxima fold."""
    import numpy as np
    parts = list(parts)
    if not parts:
        raise _invalid("combine_label_statistics: no parts")
    K, nd = parts[0]["n_labels"], parts[0]["bbox_min"].shape[1]
    with_i = "intensity_min" in parts[0]
    for p in parts:
        if p["n_labels"] != K or p["bbox_min"].shape[1] != nd or ("intensity_min" in p) != with_i \
                or (with_i and p["intensity_dtype"] != parts[0]["intensity_dtype"]):
            raise _invalid("combine_label_statistics: the parts differ in n_labels, rank or "
                           "intensity type")
    count = np.zeros(K, dtype=np.uint64)
    csum = np.zeros((K, nd), dtype=np.uint64)
    cmin = np.full((K, nd), np.iinfo(np.int64).max, dtype=np.int64)
    cmax = np.full((K, nd), -1, dtype=np.int64)
    total = 0
    for p in parts:
        here = (p["count"] != 0)[:, None]
        count += p["count"]
        csum += p["coord_sum"]
        cmin = np.where(here, np.minimum(cmin, p["bbox_min"]), cmin)
        cmax = np.where(here, np.maximum(cmax, p["bbox_max"]), cmax)
        total += p["background"] + int(p["count"].sum(dtype=np.uint64))
    intensity = None
    if with_i:
        first = parts[0]
        valid = first["intensity_valid"].copy()
        imin, imax = first["intensity_min"].copy(), first["intensity_max"].copy()
        sums = None if first["intensity_sum"] is None else first["intensity_sum"].copy()
        for p in parts[1:]:
            v, a, b = p["intensity_valid"], p["intensity_min"], p["intensity_max"]
            # -0.0 orders below +0.0, as the kernels' keys do
            lower = (a < imin) | ((a == imin) & np.signbit(a) & ~np.signbit(imin))
            upper = (b > imax) | ((b == imax) & ~np.signbit(b) & np.signbit(imax))
            imin = np.where(v & (~valid | lower), a, imin)
            imax = np.where(v & (~valid | upper), b, imax)
            valid = valid | v
            if sums is not None:
                sums = sums + p["intensity_sum"]
        intensity = (first["intensity_dtype"], valid, imin, imax, sums)
    return _label_result(K, nd, count, cmin, cmax, csum, total, intensity)


class LabelStatistics:
    """An extension with no counterpart in the reference: per label 1 .. K of an
    integer label array (0 = background) the element count, the bounding box (inclusive), the
    coordinate sums and the centroid, and with an intensity array of the same shape the smallest,
    largest, summed and mean intensity. Every result is exact: counts, sums, minima and maxima are
    integers reduced on the device, the centroid and the mean are the correctly rounded f64
    quotients of two integers. n_labels=None takes the largest label present. A label element
    below 0 or above n_labels raises InvalidParameters."""

    def __init__(self, n_labels: Optional[int] = None):
        self.n_labels = None if n_labels is None else int(n_labels)
        if self.n_labels is not None and not 0 <= self.n_labels <= _abi.LABELS_MAX:
            raise _invalid(f"label_statistics: n_labels {self.n_labels} not in "
                           f"[0, {_abi.LABELS_MAX}]")

    def name(self) -> str:
        return "label statistics"

    def is_compatible(self, dtype_labels: str, dtype_intensity: Optional[str] = None) -> None:
        check(lib().zt_label_statistics_is_compatible(
            _info_dtype(dtype_labels),
            _abi.NO_DTYPE if dtype_intensity is None else _info_dtype(dtype_intensity)))

    def state_bytes(self, ndim: int, n_labels: Optional[int] = None,
                    with_intensity: bool = False) -> int:
        """Bytes of the device state of `n_labels` labels (default: the filter's) over ndim axes."""
        K = self.n_labels if n_labels is None else int(n_labels)
        if K is None:
            raise _invalid("label_statistics: state_bytes needs n_labels")
        out = ctypes.c_uint64()
        check(lib().zt_label_statistics_state_bytes(int(ndim), K, int(bool(with_intensity)),
                                                    ctypes.byref(out)))
        return int(out.value)

    def largest_label(self, labels, ctx: Optional[Context] = None) -> int:
        """The n_labels that n_labels=None stands for: the largest element, at least 0."""
        lo, hi = Range().apply_ndarray(labels, ctx)
        return max(0, int(hi)) if hi is not None else 0

    def new_state(self, ndim: int, n_labels: int, with_intensity: bool, device=None,
                  ctx: Optional[Context] = None):
        """An empty device state that `accumulate` folds boxes into."""
        torch = _torch()
        words = self.state_bytes(ndim, n_labels, with_intensity) // 8
        state = torch.empty(words, dtype=torch.int64, device="cuda" if device is None else device)
        ctx = ctx or default_context(state.device.index)
        check(lib().zt_label_statistics_init(ctx.handle, int(ndim), int(n_labels),
                                             int(bool(with_intensity)), _ptr(state)))
        return state

    def accumulate(self, labels, state, n_labels: int, intensity=None, origin=None,
                   ctx: Optional[Context] = None) -> None:
        """Folds the box `labels` (with `intensity`) that lies at `origin` of the whole array."""
        x, dtype_l = _info_run(labels)
        y, dtype_i = _info_run(intensity) if intensity is not None else (None, None)
        self.is_compatible(dtype_l, dtype_i)
        if y is not None and tuple(y.shape) != tuple(x.shape):
            raise _invalid(f"Array shapes do not match: {list(x.shape)} vs {list(y.shape)}")
        if y is not None and y.device != x.device:
            raise _invalid("label_statistics: the arrays are on different devices")
        if origin is not None and len(origin) != x.dim():
            raise _invalid("label_statistics: origin must have one entry per axis")
        ctx = ctx or default_context(x.device.index)
        check(lib().zt_label_statistics_accumulate(
            ctx.handle, DTYPES[dtype_l], _ptr(x),
            _abi.NO_DTYPE if y is None else DTYPES[dtype_i], None if y is None else _ptr(y),
            i64_array(x.shape), None if origin is None else i64_array(origin), x.dim(),
            int(n_labels), _ptr(state)))

    def finish(self, state, ndim: int, n_labels: int, total: int,
               dtype_intensity: Optional[str] = None, ctx: Optional[Context] = None) -> dict:
        """The result dict of everything folded into `state`; `total` is the number of elements
        folded (background = total - the sum of the counts). Arrays are indexed by label - 1."""
        import numpy as np
        K, nd, with_i = int(n_labels), int(ndim), dtype_intensity is not None
        ctx = ctx or default_context(state.device.index)
        host = np.empty(self.state_bytes(nd, K, with_i) // 8, dtype=np.uint64)
        bad = ctypes.c_uint64()
        check(lib().zt_label_statistics_finish(
            ctx.handle, _ptr(state), nd, K, int(with_i), ctypes.c_void_p(host.ctypes.data),
            ctypes.byref(bad)))
        cols = host[:-1].reshape(-1, K + 1)[:, 1:]
        count = cols[0].copy()
        cmin = np.stack([cols[1 + 3 * a] for a in range(nd)], axis=1)
        cmax = np.stack([cols[2 + 3 * a] for a in range(nd)], axis=1)
        csum = np.stack([cols[3 + 3 * a] for a in range(nd)], axis=1)
        intensity = None
        if with_i:
            klo, khi = cols[1 + 3 * nd], cols[2 + 3 * nd]
            valid = klo <= khi
            imin = _keys_to_values(np.where(valid, klo, khi), dtype_intensity)
            imax = _keys_to_values(khi, dtype_intensity)
            if imin.dtype.kind == "f":
                imin = np.where(valid, imin, np.nan).astype(imin.dtype)
                imax = np.where(valid, imax, np.nan).astype(imax.dtype)
            else:
                imin = np.where(valid, imin, 0).astype(imin.dtype)
                imax = np.where(valid, imax, 0).astype(imax.dtype)
            sums = None
            if dtype_intensity in LABEL_SUM_TYPES:
                sums = _sums_128(cols[3 + 3 * nd], cols[4 + 3 * nd])
            intensity = (dtype_intensity, valid, imin, imax, sums)
        return _label_result(K, nd, count, cmin, cmax, csum, total, intensity)

    def apply_ndarray(self, labels, intensity=None, ctx: Optional[Context] = None) -> dict:
        """The statistics of a device tensor of labels (and one of intensities) as a dict of numpy
        arrays indexed by label - 1: count (uint64), bbox_min / bbox_max (int64, K x ndim, -1 for
        an absent label), coord_sum (uint64), centroid (float64, NaN for an absent label), and
        n_labels, background as ints; with intensity also intensity_valid, intensity_min,
        intensity_max (the intensity type; bfloat16 as float32), intensity_sum (Python ints) and
        intensity_mean (float64), the last two None for the 64-bit and float types."""
        x, dtype_l = _info_run(labels)
        y, dtype_i = _info_run(intensity) if intensity is not None else (None, None)
        self.is_compatible(dtype_l, dtype_i)
        if y is not None and tuple(y.shape) != tuple(x.shape):
            raise _invalid(f"Array shapes do not match: {list(x.shape)} vs {list(y.shape)}")
        ctx = ctx or default_context(x.device.index)
        K = self.n_labels if self.n_labels is not None else self.largest_label(x, ctx)
        if K > _abi.LABELS_MAX:
            raise _invalid(f"label_statistics: n_labels {K} not in [0, {_abi.LABELS_MAX}]")
        nd = max(x.dim(), 1)
        if x.dim() == 0:
            raise _invalid("label_statistics: ndim 0 not in [1, 8]")
        state = self.new_state(nd, K, y is not None, x.device, ctx)
        self.accumulate(x, state, K, y, None, ctx)
        return self.finish(state, nd, K, x.numel(), dtype_i, ctx)


def label_statistics(labels, n_labels: Optional[int] = None, intensity=None,
                     ctx: Optional[Context] = None) -> dict:
    """LabelStatistics(n_labels).apply_ndarray(labels, intensity)."""
    return LabelStatistics(n_labels).apply_ndarray(labels, intensity, ctx)


class LabelSizeFilter:
    """An extension with no counterpart in the reference: a label whose element
    count lies in [min_size, max_size] is kept, every other label becomes 0. With `relabel` the
    kept labels are renumbered 1 .. K' in increasing order of their old value; otherwise they keep
    their values. The eight integer types in and out (the input type by default). A whole-array
    operation: a label may span every chunk."""

    def __init__(self, min_size: int = 1, max_size: Optional[int] = None, relabel: bool = True):
        self.min_size = int(min_size)
        self.max_size = None if max_size is None else int(max_size)
        self.relabel = bool(relabel)
        if self.min_size < 1:
            raise _invalid(f"label_size_filter: min_size {self.min_size} is below 1")
        if self.max_size is not None and self.max_size < self.min_size:
            raise _invalid(f"label_size_filter: max_size {self.max_size} is below min_size "
                           f"{self.min_size}")

    def name(self) -> str:
        return "label size filter"

    def is_compatible(self, dtype_in: str, dtype_out: str) -> None:
        check(lib().zt_label_size_filter_is_compatible(_info_dtype(dtype_in),
                                                       _info_dtype(dtype_out)))

    def memory(self, dtype_in: str, dtype_out: str, shape, n_labels: int) -> int:
        """Device bytes of one call on an array of `shape` whose largest label is n_labels:
        input + scratch + output."""
        out = ctypes.c_uint64()
        check(lib().zt_label_size_filter_memory(
            _info_dtype(dtype_in), _info_dtype(dtype_out), i64_array(shape), len(shape),
            int(n_labels), ctypes.byref(out)))
        return int(out.value)

    def _run(self, x, dtype_in, out, dtype_out, ctx) -> int:
        if tuple(out.shape) != tuple(x.shape):
            raise _invalid(f"Array shapes do not match: {list(x.shape)} vs {list(out.shape)}")
        if x.device != out.device:
            raise _invalid("label_size_filter: the arrays are on different devices")
        if not out.is_contiguous():
            raise _invalid("label_size_filter: the output must be contiguous")
        self.is_compatible(dtype_in, dtype_out)
        ctx = ctx or default_context(x.device.index)
        kept = ctypes.c_uint64()
        check(lib().zt_label_size_filter_apply_array(
            ctx.handle, DTYPES[dtype_in], _ptr(x), DTYPES[dtype_out], _ptr(out),
            i64_array(x.shape), x.dim(), self.min_size,
            -1 if self.max_size is None else self.max_size, int(self.relabel),
            ctypes.byref(kept)))
        return int(kept.value)

    def apply_ndarray(self, v, dtype_out: Optional[str] = None, ctx: Optional[Context] = None,
                      out=None):
        """Filters a device tensor of labels; returns (out, K'). out is a new tensor of
        `dtype_out` (default: the input type), or `out` (contiguous, not overlapping the input).
        When the largest output label does not fit `dtype_out` the call raises InvalidParameters
        and writes nothing."""
        x, dtype_in = _info_run(v)
        dtype_out = dtype_out or (dtype_of(out) if out is not None else dtype_in)
        if out is None:
            self.is_compatible(dtype_in, dtype_out)
            out = _torch().empty(tuple(x.shape), dtype=torch_dtype(dtype_out), device=x.device)
        return out, self._run(x, dtype_in, out, dtype_out, ctx)

    def apply(self, input: DeviceArray, output: DeviceArray,
              ctx: Optional[Context] = None) -> int:
        """The filter's `apply` over device-resident arrays; returns K'."""
        x, dtype_in = _info_run(input)
        return self._run(x, dtype_in, output.data, output.dtype, ctx)


def label_size_filter(labels, min_size: int = 1, max_size: Optional[int] = None,
                      relabel: bool = True, dtype_out: Optional[str] = None,
                      ctx: Optional[Context] = None):
    """LabelSizeFilter(min_size, max_size, relabel).apply_ndarray(labels): (out, K')."""
    return LabelSizeFilter(min_size, max_size, relabel).apply_ndarray(labels, dtype_out, ctx)


class Reconstruction:
    """An extension with no counterpart in the reference: morphological
    reconstruction of a marker under a mask of the same shape and element type, any of the 13.
    Elements are only selected, under the rank filters' total order; neighbours are the
    labelling's (coordinates differ by at most 1 on every axis and on at most `connectivity`
    axes). By dilation the result is the least J >= min(marker, mask) with J[p] = min(max(J over p
    and its neighbours), mask[p]); a marker above the mask is clipped, not an error. By erosion the
    order is reversed. `mode` "marker" takes a marker array; the other modes make the marker from
    the mask on the device: "fill_holes" (by erosion; the mask on the array's border, the type's
    greatest key elsewhere), "h_maxima" (by dilation; (mask as f64 - h) as T) and "h_minima" (by
    erosion; (mask as f64 + h) as T), `h` a finite number > 0. `method` counts with "marker"
    only. A whole-array operation: there is no per-chunk form."""

    def __init__(self, method: str = "dilation", connectivity: int = 1, mode: str = "marker",
                 h: Optional[float] = None):
        self.method = str(method)
        self.mode = str(mode).replace("-", "_")
        self.connectivity = int(connectivity)
        if self.mode not in _abi.REC_MODES:
            raise _invalid(f"reconstruction: unknown mode {mode!r} (one of "
                           f"{', '.join(_abi.REC_MODES)})")
        if self.method not in _abi.REC_METHODS:
            raise _invalid(f"reconstruction: unknown method {method!r} (dilation or erosion)")
        implied = {"fill_holes": "erosion", "h_maxima": "dilation", "h_minima": "erosion"}
        if self.mode != "marker":
            if self.method not in ("dilation", implied[self.mode]):
                raise _invalid(f"reconstruction: {self.mode} is by {implied[self.mode]}; a method "
                               "is only given with a marker array")
            self.method = implied[self.mode]
        if self.connectivity < 1:
            raise _invalid(f"reconstruction: connectivity {self.connectivity} not in [1, rank]")
        if self.mode in ("h_maxima", "h_minima"):
            try:
                self.h = float(h)
            except (TypeError, ValueError):
                raise _invalid(f"reconstruction: {self.mode} needs a number h, not {h!r}") from None
            if not (math.isfinite(self.h) and self.h > 0):
                raise _invalid(f"reconstruction: h {self.h} is not a finite number > 0")
        elif h is not None:
            raise _invalid(f"reconstruction: h is only given with h_maxima or h_minima, not "
                           f"{self.mode}")
        else:
            self.h = 0.0

    def name(self) -> str:
        return "reconstruction"

    def check_connectivity(self, ndim: int) -> None:
        """InvalidParameters unless 1 <= connectivity <= ndim."""
        if not 1 <= self.connectivity <= int(ndim):
            raise _invalid(f"reconstruction: connectivity {self.connectivity} not in "
                           f"[1, {int(ndim)}]")

    def is_compatible(self, dtype_mask: str, dtype_marker: Optional[str] = None) -> None:
        """UnsupportedDataType when the marker's type is not the mask's, or for bool with h."""
        check(lib().zt_reconstruction_is_compatible(
            _info_dtype(dtype_mask), _info_dtype(dtype_marker or dtype_mask),
            _abi.REC_MODES[self.mode]))

    def memory(self, dtype_in: str, dtype_out: Optional[str], shape) -> int:
        """Device bytes of one call on an array of `shape`: input(s) + scratch + output."""
        self.is_compatible(dtype_in, dtype_out)
        self.check_connectivity(len(shape))
        out = ctypes.c_uint64()
        check(lib().zt_reconstruction_memory(
            _info_dtype(dtype_in), _abi.REC_MODES[self.mode], i64_array(shape), len(shape),
            ctypes.byref(out)))
        return int(out.value)

    def _run(self, x, dtype, marker, out, dtype_out, ctx) -> int:
        if self.mode == "marker":
            if marker is None:
                raise _invalid("reconstruction: mode marker needs a marker array")
            m, dtype_marker = _info_run(marker)
            if tuple(m.shape) != tuple(x.shape):
                raise _invalid(f"Array shapes do not match: {list(x.shape)} vs {list(m.shape)}")
            if m.device != x.device:
                raise _invalid("reconstruction: the arrays are on different devices")
        elif marker is not None:
            raise _invalid(f"reconstruction: {self.mode} makes its marker from the mask; no "
                           "marker array is given")
        else:
            m, dtype_marker = None, dtype
        if tuple(out.shape) != tuple(x.shape):
            raise _invalid(f"Array shapes do not match: {list(x.shape)} vs {list(out.shape)}")
        if x.device != out.device:
            raise _invalid("reconstruction: the arrays are on different devices")
        if not out.is_contiguous():
            raise _invalid("reconstruction: the output must be contiguous")
        self.is_compatible(dtype, dtype_marker)
        self.is_compatible(dtype, dtype_out)
        self.check_connectivity(x.dim())
        ctx = ctx or default_context(x.device.index)
        rounds = ctypes.c_uint64()
        check(lib().zt_reconstruction_apply_array(
            ctx.handle, DTYPES[dtype], _ptr(x), _ptr(m) if m is not None else None,
            _abi.REC_MODES[self.mode], self.h, _ptr(out), i64_array(x.shape), x.dim(),
            self.connectivity, _abi.REC_METHODS[self.method], ctypes.byref(rounds)))
        return int(rounds.value)

    def apply_ndarray(self, mask, marker=None, ctx: Optional[Context] = None, out=None):
        """Reconstructs on device tensors; returns (out, rounds). out is a new tensor of the mask's
        type, or `out` (contiguous, of that type, not overlapping the inputs); rounds counts the
        rounds up to and including the first that changed nothing. A bool array travels as a
        uint8 tensor: it is named by a DeviceArray of data type bool, and then a tensor `out` of
        the mask's torch type is taken to be bool too."""
        x, dtype = _info_run(mask)
        if out is None:
            out = _torch().empty(tuple(x.shape), dtype=x.dtype, device=x.device)
            dtype_out = dtype
        elif isinstance(out, DeviceArray):
            out, dtype_out = out.data, out.dtype
        else:
            dtype_out = dtype if out.dtype == x.dtype else dtype_of(out)
        return out, self._run(x, dtype, marker, out, dtype_out, ctx)

    def apply(self, mask: DeviceArray, marker: Optional[DeviceArray] = None,
              output: Optional[DeviceArray] = None, ctx: Optional[Context] = None) -> int:
        """The filter's `apply` over device-resident arrays; returns the rounds. The generated
        marker modes may be called as apply(mask, output)."""
        if output is None and self.mode != "marker":
            marker, output = None, marker
        if output is None:
            raise _invalid("reconstruction: apply needs an output array")
        x, dtype = _info_run(mask)
        return self._run(x, dtype, marker, output.data, output.dtype, ctx)


class Watershed:
    """An extension with no counterpart in the reference: the marker-controlled
    watershed. Every non-zero element of `seeds` (one of the 8 integer types, the relief's shape)
    is a label, carried as storage bits; the result has the seeds' type. The relief, any of the 13
    types, is compared only under the rank filters' total order, complemented with `descending` (a
    distance map flooded from its maxima). The domain is every element, or with `foreground_only`
    the non-zero elements of the relief (the labelling's rule); elements outside it get 0, are
    never crossed, and a seed there is ignored. An element takes the label of the seed that
    reaches it over the lowest pass; ties are decided by the distance on the plateau and then by
    the least linear index, so the result is unique. Elements of the domain that no seed reaches
    get 0. Neighbours are the labelling's. A whole-array operation: there is no per-chunk form."""

    def __init__(self, connectivity: int = 1, descending: bool = False,
                 foreground_only: bool = False):
        self.connectivity = int(connectivity)
        self.descending = bool(descending)
        self.foreground_only = bool(foreground_only)
        if self.connectivity < 1:
            raise _invalid(f"watershed: connectivity {self.connectivity} not in [1, rank]")

    def name(self) -> str:
        return "watershed"

    def check_connectivity(self, ndim: int) -> None:
        """InvalidParameters unless 1 <= connectivity <= ndim."""
        if not 1 <= self.connectivity <= int(ndim):
            raise _invalid(f"watershed: connectivity {self.connectivity} not in "
                           f"[1, {int(ndim)}]")

    def is_compatible(self, dtype_relief: str, dtype_seeds: str) -> None:
        """UnsupportedDataType unless the seeds (and so the labels) have an integer type."""
        check(lib().zt_watershed_is_compatible(_info_dtype(dtype_relief),
                                               _info_dtype(dtype_seeds)))

    def memory(self, dtype_relief: str, dtype_seeds: str, shape) -> int:
        """Device bytes of one call on arrays of `shape`: inputs + output + scratch."""
        self.is_compatible(dtype_relief, dtype_seeds)
        self.check_connectivity(len(shape))
        out = ctypes.c_uint64()
        check(lib().zt_watershed_memory(
            _info_dtype(dtype_relief), _info_dtype(dtype_seeds), i64_array(shape), len(shape),
            self.connectivity, int(self.foreground_only), ctypes.byref(out)))
        return int(out.value)

    def _run(self, x, dtype, seeds, out, dtype_out, ctx) -> tuple:
        s, dtype_seeds = _info_run(seeds)
        if tuple(s.shape) != tuple(x.shape):
            raise _invalid(f"Array shapes do not match: {list(x.shape)} vs {list(s.shape)}")
        if tuple(out.shape) != tuple(x.shape):
            raise _invalid(f"Array shapes do not match: {list(x.shape)} vs {list(out.shape)}")
        if s.device != x.device or x.device != out.device:
            raise _invalid("watershed: the arrays are on different devices")
        if not out.is_contiguous():
            raise _invalid("watershed: the output must be contiguous")
        self.is_compatible(dtype, dtype_seeds)
        if dtype_out != dtype_seeds:
            raise _abi.UnsupportedDataType(
                _abi.ERR_UNSUPPORTED_DATA_TYPE,
                f"watershed: the labels have the seeds' data type {dtype_seeds}, not {dtype_out}")
        self.check_connectivity(x.dim())
        ctx = ctx or default_context(x.device.index)
        rounds = (ctypes.c_int64 * 3)()
        check(lib().zt_watershed_apply_array(
            ctx.handle, DTYPES[dtype], _ptr(x), DTYPES[dtype_seeds], _ptr(s), _ptr(out),
            i64_array(x.shape), x.dim(), self.connectivity, int(self.descending),
            int(self.foreground_only), rounds))
        return tuple(int(r) for r in rounds)

    def apply_ndarray(self, relief, seeds, ctx: Optional[Context] = None, out=None):
        """The watershed on device tensors; returns (labels, rounds). labels is a new tensor of
        the seeds' type, or `out` (contiguous, of that type, not overlapping the inputs); rounds is
        (pass rounds, distance rounds, jumps), each counting the first round that changed
        nothing. A bool or 16-bit float relief is named by a DeviceArray."""
        x, dtype = _info_run(relief)
        s, dtype_seeds = _info_run(seeds)
        if out is None:
            if tuple(s.shape) != tuple(x.shape):
                raise _invalid(f"Array shapes do not match: {list(x.shape)} vs {list(s.shape)}")
            out = _torch().empty(tuple(x.shape), dtype=s.dtype, device=x.device)
            dtype_out = dtype_seeds
        elif isinstance(out, DeviceArray):
            out, dtype_out = out.data, out.dtype
        else:
            dtype_out = dtype_seeds if out.dtype == s.dtype else dtype_of(out)
        return out, self._run(x, dtype, seeds, out, dtype_out, ctx)

    def apply(self, relief: DeviceArray, seeds: DeviceArray, output: DeviceArray,
              ctx: Optional[Context] = None) -> tuple:
        """The filter's `apply` over device-resident arrays; returns the rounds."""
        x, dtype = _info_run(relief)
        return self._run(x, dtype, seeds, output.data, output.dtype, ctx)


class Downsample:
    """downsample.rs:49-287 — `Downsample::new(stride, discrete, chunk_limit)`."""

    def __init__(self, stride: Sequence[int], discrete: bool = False,
                 chunk_limit: Optional[int] = None):
        self.stride = tuple(int(s) for s in stride)
        self.discrete = bool(discrete)
        self.chunk_limit = chunk_limit

    def name(self) -> str:
        return "downsample"

    def is_compatible(self, dtype_in: str, dtype_out: str) -> None:
        check(lib().zt_downsample_is_compatible(DTYPES[dtype_in], DTYPES[dtype_out],
                                                int(self.discrete)))

    def output_shape(self, input_shape) -> tuple:
        nd = len(input_shape)
        out = i64_array([0] * nd)
        check(lib().zt_downsample_output_shape(i64_array(input_shape), nd,
                                               i64_array(self.stride), out))
        return tuple(out[:nd])

    def input_subset(self, input_shape, output_subset: ArraySubset) -> ArraySubset:
        nd = len(input_shape)
        s, n = i64_array([0] * nd), i64_array([0] * nd)
        check(lib().zt_downsample_input_subset(i64_array(input_shape), nd, i64_array(self.stride),
                                               i64_array(output_subset.start),
                                               i64_array(output_subset.shape), s, n))
        return ArraySubset(tuple(s[:nd]), tuple(n[:nd]))

    def _apply(self, v, dtype_out, discrete, ctx):
        torch = _torch()
        v = v.contiguous()
        ctx = ctx or default_context(v.device.index)
        dtype_in = dtype_of(v)
        dtype_out = dtype_out or dtype_in
        nd = v.dim()
        win = [min(s, n) for s, n in zip(self.stride, v.shape)]
        oshape = [n // w if w > 0 else 0 for n, w in zip(v.shape, win)]
        out = torch.empty(oshape, dtype=torch_dtype(dtype_out), device=v.device)
        check(lib().zt_downsample_apply_ndarray(ctx.handle, DTYPES[dtype_in], _ptr(v),
                                                i64_array(v.shape), nd, i64_array(self.stride),
                                                int(discrete), DTYPES[dtype_out], _ptr(out)))
        return out

    def apply_ndarray_continuous(self, v, dtype_out: Optional[str] = None,
                                 ctx: Optional[Context] = None):
        """downsample.rs:72-97"""
        return self._apply(v, dtype_out, False, ctx)

    def apply_ndarray_discrete(self, v, dtype_out: Optional[str] = None,
                               ctx: Optional[Context] = None):
        """downsample.rs:99-120 (ties -> smallest value)"""
        return self._apply(v, dtype_out, True, ctx)

    def apply(self, input: DeviceArray, output: DeviceArray, ctx: Optional[Context] = None):
        """downsample.rs:170-286: the whole output array (chunk-independent, one launch)."""
        if tuple(output.shape) != self.output_shape(input.shape):
            raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS, "output shape mismatch")
        # Per chunk the reference reads input_subset(output chunk) and keeps complete windows;
        # with out = max(shape/stride, 1) those are exactly the whole-array windows.
        res = self._apply(input.data, output.dtype, self.discrete, ctx)
        output.data.copy_(res.reshape(output.data.shape))


def reencode_cast(v, dtype_out: str, ctx: Optional[Context] = None):
    """Reencode::apply_chunk_convert's element conversion (reencode.rs:58-77) on a device tensor:
    every element `as` dtype_out (zt_reencode_cast). Returns a new contiguous tensor; bfloat16 is
    torch.bfloat16."""
    torch = _torch()
    v = v.contiguous()
    ctx = ctx or default_context(v.device.index)
    dtype_in = dtype_of(v)
    out = torch.empty(tuple(v.shape), dtype=torch_dtype(dtype_out), device=v.device)
    check(lib().zt_reencode_cast(ctx.handle, DTYPES[dtype_in], _ptr(v), DTYPES[dtype_out],
                                 _ptr(out), int(v.numel())))
    return out


def pyramid_level_shapes(shape, factor, max_levels: int) -> list:
    """zarrs_ome.rs:515-560/:731-737 level shapes + stop rule."""
    nd = len(shape)
    buf = i64_array([0] * (nd * max(max_levels, 1)))
    n = ctypes.c_int()
    check(lib().zt_pyramid_level_shapes(i64_array(shape), nd, i64_array(factor), int(max_levels),
                                        buf, ctypes.byref(n)))
    return [tuple(buf[i * nd:(i + 1) * nd]) for i in range(n.value)]


def pyramid(level0, factor=None, max_levels: int = 10, discrete: bool = False,
            ctx: Optional[Context] = None) -> list:
    """Device-resident zarrs_ome mean (or mode) pyramid: returns [level1, level2, ...]."""
    torch = _torch()
    level0 = level0.contiguous()
    ctx = ctx or default_context(level0.device.index)
    nd = level0.dim()
    factor = tuple(factor or (2,) * nd)
    shapes = pyramid_level_shapes(level0.shape, factor, max_levels)
    outs = [torch.empty(s, dtype=level0.dtype, device=level0.device) for s in shapes]
    ptrs = (ctypes.c_void_p * max(len(outs), 1))(*[o.data_ptr() for o in outs])
    written = ctypes.c_int()
    check(lib().zt_pyramid_downsample(ctx.handle, DTYPES[dtype_of(level0)], _ptr(level0),
                                      i64_array(level0.shape), nd, i64_array(factor),
                                      int(max_levels), int(discrete), ptrs, ctypes.byref(written)))
    return outs[:written.value]


def synth_step_noise_f32(shape, seed: int = 0x5EED2025, global_shape=None, z0: int = 0,
                         device=None, ctx: Optional[Context] = None):
    """SURVEY.md §8(d) synthetic volume generated on the device."""
    torch = _torch()
    out = torch.empty(tuple(shape), dtype=torch.float32, device=device or "cuda")
    ctx = ctx or default_context(out.device.index)
    gs = global_shape or shape
    check(lib().zt_synth_step_noise_f32(ctx.handle, _ptr(out), i64_array(shape), len(shape),
                                        i64_array(gs), int(z0), int(seed)))
    return out


def synth_u16(shape, seed: int = 0x5EED2025, global_shape=None, z0: int = 0, device=None,
              ctx: Optional[Context] = None):
    torch = _torch()
    out = torch.empty(tuple(shape), dtype=torch.uint16, device=device or "cuda")
    ctx = ctx or default_context(out.device.index)
    gs = global_shape or shape
    check(lib().zt_synth_u16(ctx.handle, _ptr(out), i64_array(shape), len(shape), i64_array(gs),
                             int(z0), int(seed)))
    return out


def synth_box(start, shape, global_shape, kind: str = "uint16", seed: int = 0x5EED2025,
              device=None, ctx: Optional[Context] = None):
    """The box [start, start+shape) of the global synthetic volume, generated on the device
    (kind "uint16" noise or "float32" step+noise): a rank's own octant or slab."""
    torch = _torch()
    dt = torch.uint16 if kind == "uint16" else torch.float32
    out = torch.empty(tuple(shape), dtype=dt, device=device or "cuda")
    ctx = ctx or default_context(out.device.index)
    check(lib().zt_synth_box(ctx.handle, 1 if kind == "uint16" else 0, _ptr(out),
                             i64_array(start), i64_array(shape), i64_array(global_shape),
                             len(shape), int(seed)))
    return out
