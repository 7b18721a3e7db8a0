"""``zarrs_filter`` for the on-path filters over Zarr V3 stores. What the tool knows about a kind
of step is one record of STEP_KINDS (below): the sub-parser, the run-config keys, the output
array's type, the call into `store` and how the step may run are all read from it.

Mirrors src/bin/zarrs_filter.rs (LDeakin/zarrs_tools 0.7.2) for the filters this framework
accelerates:

    python -m zarrs_tools_amd.zarrs_filter [--exists erase|exit] [--tmp DIR] [--chunk-limit N]
        [--device D] [RUN_CONFIG.json] [SUBCOMMAND IN OUT ARGS... [--data-type T]]

with one SUBCOMMAND per record, its name with hyphens (`--help` lists them, `SUBCOMMAND --help`
its arguments).

* subcommand arguments as GuidedFilterArguments (guided_filter.rs:25-33),
  DownsampleArguments (downsample.rs:20-33, STRIDE comma delimited) and GaussianArguments
  (gaussian.rs:22-30, SIGMA and KERNEL_HALF_SIZE comma delimited, one entry per axis);
  summed-area-table takes none of its own (SummedAreaTableArguments, summed_area_table.rs:22-23);
  median, minimum and maximum (extensions: the reference has no rank filter)
  take KERNEL_HALF_SIZE, comma delimited, one non-negative entry per axis, the median's window
  holding at most 4096 elements; the per-element filters as ReencodeArguments (reencode.rs:20), CropArguments (crop.rs:20-27,
  OFFSET and SHAPE comma delimited), RescaleArguments (rescale.rs:20-31), ClampArguments
  (clamp.rs:20-25), EqualArguments (equal.rs:23-34) and ReplaceValueArguments
  (replace_value.rs:23-44); VALUE and REPLACE follow parse_fill_value (a JSON number, true /
  false, NaN, Infinity, -Infinity) and negative numbers parse as values;
  arithmetic (an extension: the reference has no two-array filter) writes
  OUT = IN OPERATOR OTHER element by element, OPERATOR one of add, subtract, multiply, divide,
  minimum, maximum, absolute-difference (hyphens on the command line, snake_case in a run
  config), OTHER a second array of IN's shape and of any type, chunk grid and codecs;
  connected-components (an extension: the reference has no labelling) gives
  every connected set of non-zero elements its own integer 1 .. K in the C order of the sets'
  first elements, background 0; two elements are neighbours when their coordinates differ by at
  most 1 on every axis and on at most C axes (--connectivity, default 1: faces); OUT is uint32
  with fill value 0 unless --data-type names another integer type, and the step fails, writing
  nothing, when K does not fit it; the step logs K;
  distance-transform (an extension: the reference has none) gives every element
  its exact Euclidean distance to the nearest zero element (0 on the background, +inf, or the
  type's maximum, everywhere when there is none); --spacing is the length of a step along each
  axis, comma delimited integers >= 1, one per axis (default all 1); --squared stores the squared
  distance, an exact integer; OUT is float32 (uint32 with --squared) with fill value 0 unless
  --data-type names another numeric type;
  label-size-filter (an extension: the reference has none) keeps the labels of
  an integer label array (0 = background) whose element count lies in [--min-size, --max-size]
  (default 1 and no bound) and sets every other label to 0; the kept labels are renumbered
  1 .. K' in increasing order of their old value unless --no-relabel; OUT has IN's type and fill
  value 0 unless --data-type names another integer type, and the step fails, writing nothing,
  when the largest output label does not fit it or an element is negative; the step logs K';
  reconstruction (an extension: the reference has none) reconstructs a marker
  under the mask IN: by dilation the least J >= min(marker, mask) with J[p] = min(max(J over p and
  its neighbours), mask[p]), by erosion the same with the order reversed (--method, with --marker
  only; default dilation), neighbours as connected-components' (--connectivity, default 1);
  --marker PATH is a second array of IN's shape and data type, of any chunk grid and codecs;
  --fill-holes (by erosion, the marker is the mask on the array's border and the type's greatest
  value elsewhere: on a mask of background it fills the holes), --h-maxima H (by dilation, the
  marker is IN - H) and --h-minima H (by erosion, IN + H), H a finite number > 0, make the marker
  from the mask on the device; exactly one of the four is given; OUT has IN's data type and fill
  value; the step logs its rounds;
* a JSON run config is a list of {"filter": a record's name, "input", "output", ...args
  (kernel_half_size; offset, shape, multiply, add, add_first, min, max, value, replace for the
  per-element filters; connectivity for connected_components; spacing, squared for
  distance_transform; min_size, max_size, relabel for label_size_filter; marker, mode, h, method,
  connectivity for reconstruction ("mode" one of marker, fill_holes, h_maxima, h_minima: marker
  when a "marker" is given); operator, other for arithmetic; "other" and "marker" are a path or
  the "$name" of a temporary that an earlier step wrote), "data_type"}, with "$name" meaning a named
  temporary array under --tmp and an omitted input meaning the previous filter's output (zarrs_filter.rs:106-138,
  :338-381);
* a chain of steps linked only through temporaries (a "$name" or implicit output read by the
  next step alone) runs device-resident when its arrays fit 80 % of the free device memory: the
  chain input is read once, every step runs on the arrays in HBM, the last output is written
  once; the temporaries' zarr.json are created as the store path would create them, but their
  chunks never go through the store (`--no-device-chain` forces the store path); inside such a
  chain a run of consecutive per-element steps is one kernel launch that reads each element once
  and writes it once (up to 8 steps per launch; crops compose by adding their offsets;
  `--no-pointwise-fusion` launches them one by one); an arithmetic step is never part of such
  a chain (it runs store -> store and ends the chain before it), and a temporary that a later
  arithmetic step reads as its "other" is written to the store by the step that produces it;
  a connected_components step may be part of such a chain (equal -> connected_components labels
  a mask that never touches the store), and the chain's budget then counts its two index arrays;
  so may a distance_transform step (equal -> distance_transform -> clamp erodes a mask by a ball),
  whose work arrays and stacks the budget counts in the same way; so may a reconstruction step
  that makes its marker from the mask (equal -> reconstruction(fill_holes) ->
  connected_components -> label_size_filter is one chain); one with a marker array is never part
  of a chain, and a temporary that a later step reads as its "marker" is written to the store;
* every filter takes the reencoding arguments (ZarrReencodingArgs, lib.rs:274-377: -d/--data-type,
  -f/--fill-value, --separator, -c/--chunk-shape, -s/--shard-shape, --array-to-array-codecs,
  --array-to-bytes-codec, --bytes-to-bytes-codecs, --dimension-names, --attributes,
  --attributes-append; the same snake_case keys in a run config), applied to the output array as
  get_array_builder_reencode does (lib.rs:408-650; host/zt_store.cpp build_output);
* `--exists erase` (default) overwrites an existing output, `exit` refuses it (:228-235);
* the output metadata is erased before a filter runs and written when it finishes (:297-313);
* per-chunk progress (Progress, progress.rs:15-119) is shown on a terminal as
  `step/steps rw:READ/WRITE p:PROCESS` (thread-seconds, device seconds), like zarrs_filter.rs:
  149-172.

gradient_magnitude is rejected with FilterError::Other: it runs from the library only
(DESIGN.md §1). A summed-area table's chunk rows each need the previous row's last plane, so with
--gpus > 1 that step runs in one process on the first device (`rows_splittable`); so do
connected_components, distance_transform, label_size_filter and reconstruction, whose unit of work is the whole array: it is read
into device memory, processed and written once, and fails with the out-of-memory error when it
does not fit (there is no store -> store path for them). The other
filters' rows, the per-element ones included, are split over the processes. `--chunk-limit N`
bounds the chunks in flight (decoded input rows + output rows being computed or encoded, and the
host worker threads) at N, down to the pipeline's unit of one slab and one output row
(guided_filter.rs:251-258); independently the rows held in memory are bounded by 80 % of the
available host and device memory, failing like calculate_chunk_limit (filter.rs:52-66) when not
even one row fits.
"""
from __future__ import annotations

import argparse
import dataclasses
import functools
import json
import os
import re
import shutil
import sys
import tempfile
import time

import numpy as np

from . import _abi
from . import filter as F
from . import store as S
from .device_io import _read_pieces, _row_spans, read_to_device, write_from_device  # noqa: F401


def _parse_stride(s: str):
    return [int(x) for x in s.split(",") if x.strip()]


def _parse_floats(s: str):
    return [float(x) for x in s.split(",") if x.strip()]


# ZarrReencodingArgs (lib.rs:274-377), flattened into every filter's arguments
# (filter_common_arguments.rs:7-16) and into the JSON run config (serde flatten).
REENCODE_KEYS = ("data_type", "fill_value", "separator", "chunk_shape", "shard_shape",
                 "array_to_array_codecs", "array_to_bytes_codec", "bytes_to_bytes_codecs",
                 "dimension_names", "attributes", "attributes_append")


def _parse_fill_value(s: str):
    """parse_fill_value: JSON (0, 100, -1.5, "NaN", "[0, 255]"), else the bare string."""
    if s in ("NaN", "Infinity", "-Infinity"):
        return s  # the Zarr V3 fill-value strings, kept as strings
    try:
        return json.loads(s)
    except ValueError:
        return s


SKIP_EMPTY_HELP = ("do not store chunks (or inner chunks of shards) that hold nothing but the "
                   "fill value, and remove such chunks of an output being overwritten (zarrs' "
                   "store_empty_chunks = false)")


def _add_reencode_args(p: argparse.ArgumentParser) -> None:
    p.add_argument("-d", "--data-type", default=None)
    p.add_argument("-f", "--fill-value", type=_parse_fill_value, default=None)
    p.add_argument("--separator", default=None, choices=["/", "."])
    p.add_argument("-c", "--chunk-shape", type=_parse_stride, default=None)
    p.add_argument("-s", "--shard-shape", type=_parse_stride, default=None)
    p.add_argument("--array-to-array-codecs", default=None)
    p.add_argument("--array-to-bytes-codec", default=None)
    p.add_argument("--bytes-to-bytes-codecs", default=None)
    p.add_argument("--dimension-names", type=lambda s: s.split(","), default=None)
    p.add_argument("--attributes", default=None)
    p.add_argument("--attributes-append", default=None)
    p.add_argument("--chunk-limit", dest="filter_chunk_limit", type=int, default=None)
    p.add_argument("--skip-empty-chunks", dest="filter_skip_empty_chunks", action="store_true",
                   help=SKIP_EMPTY_HELP)


def _reencode_of(a) -> dict:
    return {k: getattr(a, k) for k in REENCODE_KEYS if getattr(a, k, None) is not None}


def encoding_of(step: dict) -> dict | None:
    """The reencoding arguments of a run-config step (JSON strings of the codec / attribute
    arguments parsed), or None when it has none."""
    enc = {}
    for k in REENCODE_KEYS:
        v = step.get(k)
        if v is None:
            continue
        if k in ("array_to_array_codecs", "array_to_bytes_codec", "bytes_to_bytes_codecs",
                 "attributes", "attributes_append") and isinstance(v, str):
            v = json.loads(v)
        if k in ("chunk_shape", "shard_shape") and isinstance(v, str):
            v = _parse_stride(v)
        enc[k] = v
    return enc or None


def _invalid(message: str):
    return _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS, message)


def _need(step: dict, *keys):
    missing = [k for k in keys if step.get(k) is None]
    if missing:
        raise _invalid(f"{step.get('filter')} needs {', '.join(missing)}")
    return [step[k] for k in keys]


def _ints(v):
    return _parse_stride(v) if isinstance(v, str) else [int(x) for x in v]


def _integer(step: dict, key: str, default, message: str):
    """The integer step[key], `default` when it is absent; InvalidParameters(message) else."""
    try:
        return default if step.get(key) is None else int(step[key])
    except (TypeError, ValueError):
        raise _invalid(message) from None


# ---- what the records of STEP_KINDS (below) are made of, where it takes more than a line: the
# sub-parser's own arguments, the filter object of a run-config step, the checks that need the
# output type

def _args_guided_filter(p):
    p.add_argument("epsilon", type=float)
    p.add_argument("radius", type=int)


def _args_downsample(p):
    p.add_argument("stride", type=_parse_stride)
    p.add_argument("--discrete", action="store_true")


def _args_gaussian(p):
    p.add_argument("sigma", type=_parse_floats)
    p.add_argument("kernel_half_size", type=_parse_stride)


def _args_rank(p):
    p.add_argument("kernel_half_size", type=_parse_stride)


def _args_crop(p):
    p.add_argument("offset", type=_parse_stride)
    p.add_argument("shape", type=_parse_stride)


def _args_rescale(p):
    p.add_argument("multiply", type=float)
    p.add_argument("add", type=float)
    p.add_argument("--add-first", action="store_true",
                   help="perform the addition before the multiplication")


def _args_clamp(p):
    p.add_argument("min", type=float)
    p.add_argument("max", type=float)


def _args_equal(p):
    p.add_argument("value", type=_parse_fill_value)


def _args_replace_value(p):
    p.add_argument("value", type=_parse_fill_value)
    p.add_argument("replace", type=_parse_fill_value)


def _args_arithmetic(p):
    p.add_argument("operator", choices=[o.replace("_", "-") for o in _abi.AR_OPERATORS])
    p.add_argument("other")


def _args_connectivity(p):
    p.add_argument("--connectivity", type=int, default=1,
                   help="neighbours differ on at most this many axes (1: faces, the default; "
                        "the rank: the full neighbourhood)")


def _args_distance_transform(p):
    p.add_argument("--spacing", type=_parse_stride, default=None,
                   help="the length of a step along each axis: comma delimited integers >= 1, "
                        "one per axis (default: all 1)")
    p.add_argument("--squared", action="store_true",
                   help="store the squared distance (an exact integer; uint32 by default)")


def _args_label_size_filter(p):
    p.add_argument("--min-size", type=int, default=1,
                   help="the fewest elements of a label that is kept (default 1)")
    p.add_argument("--max-size", type=int, default=None,
                   help="the most elements of a label that is kept (default: no bound)")
    p.add_argument("--no-relabel", action="store_true",
                   help="kept labels keep their values (default: renumbered 1 .. K' in "
                        "increasing order)")


def _args_reconstruction(p):
    how = p.add_mutually_exclusive_group(required=True)
    how.add_argument("--marker", default=None,
                     help="the marker: a second array of IN's shape and data type")
    how.add_argument("--fill-holes", action="store_true",
                     help="by erosion from the array's border: fills the holes of a mask of "
                          "background")
    how.add_argument("--h-maxima", type=float, default=None, metavar="H",
                     help="by dilation of IN - H: suppresses maxima lower than H")
    how.add_argument("--h-minima", type=float, default=None, metavar="H",
                     help="by erosion of IN + H: suppresses minima shallower than H")
    p.add_argument("--method", choices=["dilation", "erosion"], default=None,
                   help="with --marker only (default dilation)")
    _args_connectivity(p)


def _own_reconstruction(a):
    """The step's own keys: (those before "data_type", those after the reencoding keys)."""
    if a.method is not None and a.marker is None:
        raise _invalid("reconstruction: --method is only valid with --marker")
    mode, last = "marker", {}
    if a.marker is not None:
        last = {"marker": a.marker, "method": a.method or "dilation"}
    elif a.fill_holes:
        mode = "fill_holes"
    elif a.h_maxima is not None:
        mode, last = "h_maxima", {"h": a.h_maxima}
    elif a.h_minima is not None:
        mode, last = "h_minima", {"h": a.h_minima}
    return {"mode": mode, "connectivity": a.connectivity}, last


def _make_guided_filter(step, info):
    if "epsilon" not in step or "radius" not in step:
        raise _invalid("guided_filter needs epsilon and radius")
    return F.GuidedFilter(float(step["epsilon"]), int(step["radius"]))


def _make_downsample(step, info):
    stride = step.get("stride")
    stride = _parse_stride(stride) if isinstance(stride, str) else stride
    if not stride or len(stride) != info.ndim:
        raise _invalid("downsample stride must match the array rank")
    return F.Downsample(stride, discrete=bool(step.get("discrete", False)))


def _make_gaussian(step, info):
    sigma, half = step.get("sigma"), step.get("kernel_half_size")
    sigma = _parse_floats(sigma) if isinstance(sigma, str) else sigma
    half = _parse_stride(half) if isinstance(half, str) else half
    if not sigma or not half or len(sigma) != info.ndim or len(half) != info.ndim:
        raise _invalid("gaussian sigma and kernel_half_size need one entry per axis")
    return F.Gaussian(sigma, half)


def _make_rank(step, info):
    name, half = step["filter"], step.get("kernel_half_size")
    if half is None:
        raise _invalid(f"{name} needs kernel_half_size")
    half = _ints(half)
    F.check_rank_half(name, half, info.ndim)
    return F.RankFilter(name, half)


def pointwise_filter(step: dict):
    """The per-element filter object of a run-config step (keys as the reference's *Arguments
    structs: offset, shape; multiply, add, add_first; min, max; value; value, replace)."""
    kind = STEP_KINDS.get(step.get("filter"))
    if kind is None or kind.family != "pointwise":
        raise _invalid(f"{step.get('filter')} is not a per-element filter")
    return kind.make(step, None)


def arithmetic_args(step: dict):
    """(operator, other) of an arithmetic run-config step."""
    missing = [k for k in ("operator", "other") if step.get(k) is None]
    if missing:
        raise _invalid(f"arithmetic needs {', '.join(missing)}")
    F.arithmetic_operator(step["operator"])  # InvalidParameters for an unknown name
    return str(step["operator"]).replace("-", "_"), step["other"]


def connectivity_of(step: dict, name: str = "connected_components") -> int:
    """The connectivity of a run-config step of the filter `name` (default 1: faces)."""
    return _integer(step, "connectivity", 1,
                    f"{name}: connectivity {step.get('connectivity')!r} is not an integer")


def distance_transform_of(step: dict, info=None):
    """The DistanceTransform of a run-config step: "spacing" a list (or a comma delimited string)
    of integers >= 1, default all 1; "squared" a boolean, default false."""
    sp = step.get("spacing")
    if isinstance(sp, str):
        sp = [x.strip() for x in sp.split(",") if x.strip()]
        try:
            sp = [int(x) for x in sp]
        except ValueError:
            raise _invalid(f"distance_transform: spacing {step['spacing']!r} is not a list of "
                           "integers") from None
    elif sp is not None and not isinstance(sp, (list, tuple)):
        sp = [sp]
    return F.DistanceTransform(sp, bool(step.get("squared", False)))


def label_size_filter_of(step: dict, info=None):
    """The size filter of a run-config step: "min_size" (default 1) and "max_size" (default
    none) integers, "relabel" a boolean (default true)."""
    message = "label_size_filter: min_size and max_size are integers"
    mn, mx = _integer(step, "min_size", 1, message), _integer(step, "max_size", None, message)
    relabel = step.get("relabel")
    return S.SizeFilterStep(F.LabelSizeFilter(mn, mx, True if relabel is None else bool(relabel)))


def reconstruction_of(step: dict):
    """(Reconstruction, marker) of a run-config step: "marker" a path or the "$name" of an earlier
    step's output (then "mode" is marker, or omitted), or "mode" one of fill_holes, h_maxima,
    h_minima with "h" for the last two; "method" dilation (default) or erosion, with a marker
    only; "connectivity" an integer (default 1)."""
    marker = step.get("marker")
    mode = step.get("mode") or ("marker" if marker is not None else None)
    if mode is None:
        raise _invalid("reconstruction needs a marker or a mode (fill_holes, h_maxima, "
                       "h_minima)")
    mode = str(mode).replace("-", "_")
    if (mode == "marker") != (marker is not None):
        raise _invalid(
            "reconstruction: mode marker needs a marker" if marker is None else
            f"reconstruction: {mode} makes its marker from the mask; no marker is given")
    if step.get("method") is not None and marker is None:
        raise _invalid("reconstruction: a method is only valid with a marker")
    c = connectivity_of(step, "reconstruction")
    return F.Reconstruction(step.get("method") or "dilation", c, mode, step.get("h")), marker


def _check_pointwise(f, info, dt):
    f.is_compatible(info.data_type, dt)
    f.op(info.data_type, dt)  # value / replace must fit the types


def _check_connected_components(f, info, dt):
    f.is_compatible(info.data_type, dt)
    f.check_connectivity(info.ndim)


def _check_distance_transform(f, info, dt):
    f.is_compatible(info.data_type, dt)
    f.check_spacing(info.ndim)
    f.memory(info.data_type, dt, info.shape)  # the bound on the squared distance


def _check_reconstruction(f, info, dt):
    if dt != info.data_type:
        raise _abi.UnsupportedDataType(
            _abi.ERR_UNSUPPORTED_DATA_TYPE,
            f"reconstruction: the output has the input's data type {info.data_type}, not {dt}")
    f.is_compatible(info.data_type)
    f.check_connectivity(info.ndim)


def _output_as_given(step, in_data_type, enc):
    """The default rule: an explicit data type, else the input's; the encoding as given."""
    return step.get("data_type") or (enc or {}).get("data_type") or in_data_type, enc


def _text_key_values(p):
    """The default fragment: the step's own parameters as key=value."""
    return " ".join(f"{k}={v}" for k, v in p.items())


def _store_pointwise(name: str, src: str, dst: str, p: dict, **kw) -> dict:
    """A per-element step store -> store: p["args"] holds the filter's own run-config keys."""
    f = pointwise_filter({"filter": name, **p["args"]})
    dt, enc = S.pointwise_output(f, S.open_array(src).data_type, kw.pop("data_type", None),
                                 kw.pop("encoding", None))
    return S.pointwise(src, dst, [f], [dt], encoding=enc, **kw)


@dataclasses.dataclass(frozen=True)
class StepKind:
    """Everything zarrs_filter knows about one kind of step. The functions are the module's own
    and capture nothing (a spawned worker finds the record by its name); the `store` of each
    looks its function up in `S` when it is called. A kind without `make` is only a store call
    (for run_rows_parallel) and is outside the accelerated path."""
    name: str  # in a run config; the subcommand is the same with hyphens
    help: str = ""  # of the sub-parser
    arguments: object = None  # (sub-parser): adds its own arguments, after IN and OUT
    negative_numbers: object = None  # a pattern of arguments that begin with "-" and are values
    # the step's own keys: names in the argparse namespace, or (namespace) -> (keys, last keys)
    own: object = ()
    make: object = None  # (step, info) -> the filter object of a run-config step, validated
    output: object = _output_as_given  # (step, input type, encoding) -> (data type, encoding)
    check: object = None  # (filter, info, output type): the checks that need the output type
    shape: object = None  # (filter, info) -> the output's shape; None: the input's
    params: object = None  # (filter, step) -> the picklable dict that `store` reads; None: {}
    text: object = _text_key_values  # (params) -> the step's part of its log line
    after: object = None  # (params) -> what the log line adds behind the input array
    store: object = None  # (src, dst, params, **kw) -> stats: the one call into store.*
    family: str = ""  # "rank", "pointwise", "binary" or "whole_array": the name tuples below
    rows: bool = True  # chunk rows are independent: --gpus > 1 may split them over processes
    chain: bool = True  # may be part of a device-resident chain
    second: object = None  # (key, (step) -> value) of a second input array, "$name" allowed
    reports: str = None  # the count the filter returns, in the stats and the log


# per-element values may be negative (-1e-3 included) and VALUE may be -Infinity; a rank filter's
# negative KERNEL_HALF_SIZE parses as a value and is rejected as InvalidParameters when the step
# runs (build_parser says how the patterns take effect)
_NUMBER = re.compile(r"^-(\d+\.?\d*|\d*\.\d+)([eE][-+]?\d+)?$|^-Infinity$")
_RANK_NUMBER = re.compile(r"^-\d+(,-?\d+)*$")
POINTWISE_KEYS = ("offset", "shape", "multiply", "add", "add_first", "min", "max", "value",
                  "replace")


def _rank_kind(name: str, what: str) -> StepKind:
    return StepKind(
        name, f"Apply a {what} filter over a box neighbourhood.", _args_rank, _RANK_NUMBER,
        ("kernel_half_size",), _make_rank,
        params=lambda f, step: {"kernel_half_size": list(f.kernel_half_size())},
        store=functools.partial(_store_rank, name), family="rank")


def _store_rank(name, src, dst, p, **kw):
    return S.rank_filter(src, dst, name, p["kernel_half_size"], **kw)


def _pointwise_kind(name: str, help: str, arguments, own: tuple, make) -> StepKind:
    return StepKind(
        name, help, arguments, _NUMBER, own, make,
        output=lambda step, in_dt, enc: S.pointwise_output(  # equal: bool, fill value false
            pointwise_filter(step), in_dt, step.get("data_type"), enc),
        check=_check_pointwise, shape=lambda f, info: f.output_shape(info.shape),
        params=lambda f, step: {"args": {k: step[k] for k in POINTWISE_KEYS
                                         if step.get(k) is not None}},
        text=lambda p: f"{p['args']}", store=functools.partial(_store_pointwise, name),
        family="pointwise")


# In the order of the subcommands. A summed-area table's chunk rows are not independent: each
# row's axis-0 sum starts from the previous row's last plane (summed_area_table.rs:69, :94-97).
# Nor are the whole-array filters': a connected component may span every chunk, and the nearest
# background element may lie in any; they have no chunks in flight either, so their store
# functions take no chunk_limit.
STEP_KINDS = {k.name: k for k in (
    StepKind(
        "guided_filter", "Apply a guided filter (edge preserving noise filter).",
        _args_guided_filter, own=("epsilon", "radius"), make=_make_guided_filter,
        params=lambda f, step: {"epsilon": float(step["epsilon"]), "radius": int(step["radius"])},
        store=lambda src, dst, p, **kw: S.guided_filter(src, dst, p["epsilon"], p["radius"],
                                                        **kw)),
    StepKind(
        "downsample", "Downsample an image given a stride.", _args_downsample,
        own=("stride", "discrete"), make=_make_downsample,
        shape=lambda f, info: f.output_shape(info.shape),
        params=lambda f, step: {"stride": list(f.stride),
                                "discrete": bool(step.get("discrete", False))},
        store=lambda src, dst, p, **kw: S.downsample(src, dst, p["stride"],
                                                     discrete=p["discrete"], **kw)),
    StepKind(
        "gaussian", "Apply a Gaussian kernel.", _args_gaussian,
        own=("sigma", "kernel_half_size"), make=_make_gaussian,
        params=lambda f, step: {"sigma": list(f.sigma),
                                "kernel_half_size": list(f.kernel_half_size())},
        store=lambda src, dst, p, **kw: S.gaussian(src, dst, p["sigma"], p["kernel_half_size"],
                                                   **kw)),
    StepKind(
        "summed_area_table", "Compute a summed area table (integral image).",
        make=lambda step, info: F.SummedAreaTable(),
        store=lambda src, dst, p, **kw: S.summed_area_table(src, dst, **kw), rows=False),
    _rank_kind("median", "median"),
    _rank_kind("minimum", "minimum (grey-scale erosion)"),
    _rank_kind("maximum", "maximum (grey-scale dilation)"),
    _pointwise_kind("reencode", "Reencode an array.", None, (), lambda step, info: F.Reencode()),
    _pointwise_kind(
        "crop", "Crop an array given an offset and shape.", _args_crop, ("offset", "shape"),
        lambda step, info: F.Crop(*map(_ints, _need(step, "offset", "shape")))),
    _pointwise_kind(
        "rescale", "Rescale array values given a multiplier and offset.", _args_rescale,
        ("multiply", "add", "add_first"),
        lambda step, info: F.Rescale(*map(float, _need(step, "multiply", "add")),
                                     bool(step.get("add_first", False)))),
    _pointwise_kind(
        "clamp", "Clamp values between a minimum and maximum.", _args_clamp, ("min", "max"),
        lambda step, info: F.Clamp(*map(float, _need(step, "min", "max")))),
    _pointwise_kind(
        "equal", "Return a binary image where the input is equal to some value.", _args_equal,
        ("value",), lambda step, info: F.Equal(*_need(step, "value"))),
    _pointwise_kind(
        "replace_value", "Replace a value with another value.", _args_replace_value,
        ("value", "replace"), lambda step, info: F.ReplaceValue(*_need(step, "value", "replace"))),
    StepKind(
        "arithmetic", "Combine two arrays of one shape element by element.", _args_arithmetic,
        own=lambda a: ({"operator": a.operator.replace("-", "_"), "other": a.other}, {}),
        make=lambda step, info: F.Arithmetic(arithmetic_args(step)[0]),
        params=lambda f, step: {"operator": f.operator, "other": str(step["other"])},
        text=lambda p: p["operator"], after=lambda p: f" with {p['other']}",
        store=lambda src, dst, p, **kw: S.arithmetic(src, p["other"], dst, p["operator"], **kw),
        family="binary", chain=False, second=("other", lambda step: arithmetic_args(step)[1])),
    StepKind(
        "connected_components", "Label the connected sets of non-zero elements.",
        _args_connectivity, own=("connectivity",),
        make=lambda step, info: F.ConnectedComponents(connectivity_of(step)),
        output=lambda step, in_dt, enc: S.connected_components_output(  # uint32, fill value 0
            step.get("data_type"), enc),
        check=_check_connected_components,
        params=lambda f, step: {"connectivity": f.connectivity},
        store=lambda src, dst, p, chunk_limit=0, **kw: S.connected_components(
            src, dst, p["connectivity"], **kw),
        family="whole_array", rows=False, reports="components"),
    StepKind(
        "distance_transform", "Exact Euclidean distance to the nearest zero element.",
        _args_distance_transform, own=("spacing", "squared"), make=distance_transform_of,
        output=lambda step, in_dt, enc: S.distance_transform_output(  # float32, uint32 squared
            bool(step.get("squared", False)), step.get("data_type"), enc),
        check=_check_distance_transform,
        params=lambda f, step: {"spacing": None if f.spacing is None else list(f.spacing),
                                "squared": f.squared},
        text=lambda p: f"spacing={p['spacing'] or 'ones'} squared={p['squared']}",
        store=lambda src, dst, p, chunk_limit=0, **kw: S.distance_transform(
            src, dst, p["spacing"], p["squared"], **kw),
        family="whole_array", rows=False),
    StepKind(
        "label_size_filter", "Keep the labels of a label array whose element count is in range.",
        _args_label_size_filter,
        own=lambda a: ({"min_size": a.min_size, "max_size": a.max_size,
                        "relabel": not a.no_relabel}, {}),
        make=label_size_filter_of,
        output=lambda step, in_dt, enc: S.label_size_filter_output(  # the input's, fill value 0
            in_dt, step.get("data_type"), enc),
        check=lambda f, info, dt: f.is_compatible(info.data_type, dt),
        params=lambda f, step: {"min_size": f.min_size, "max_size": f.max_size,
                                "relabel": f.relabel},
        store=lambda src, dst, p, chunk_limit=0, **kw: S.label_size_filter(
            src, dst, p["min_size"], p["max_size"], p["relabel"], **kw),
        family="whole_array", rows=False, reports="components"),
    StepKind(
        "reconstruction", "Morphological reconstruction of a marker under the mask IN.",
        _args_reconstruction, own=_own_reconstruction,
        make=lambda step, info: reconstruction_of(step)[0], check=_check_reconstruction,
        params=lambda f, step: {
            "marker": None if step.get("marker") is None else str(step["marker"]),
            "mode": f.mode, "method": f.method, "connectivity": f.connectivity,
            "h": f.h if f.mode in ("h_maxima", "h_minima") else None},
        text=lambda p: (f"mode={p['mode']} method={p['method']} connectivity={p['connectivity']}"
                        + (f" h={p['h']}" if p["h"] is not None else "")),
        after=lambda p: f" marker {p['marker']}" if p["marker"] is not None else "",
        store=lambda src, dst, p, chunk_limit=0, **kw: S.reconstruction(
            src, dst, p["marker"], p["method"] if p["marker"] else "dilation", p["connectivity"],
            p["mode"], p["h"], **kw),
        family="whole_array", rows=False,
        second=("marker", lambda step: reconstruction_of(step)[1]), reports="rounds"),
    StepKind(  # a zarrs_ome level with --gaussian-sigma
        "downsample_gaussian",
        store=lambda src, dst, p, **kw: S.downsample_gaussian(
            src, dst, p["stride"], p["sigma"], p["kernel_half_size"], **kw)),
)}


def _family(family: str) -> tuple:
    return tuple(k.name for k in STEP_KINDS.values() if k.family == family)


POINTWISE, RANK = _family("pointwise"), _family("rank")
BINARY = _family("binary")  # two arrays in: "input" and "other"
WHOLE_ARRAY = _family("whole_array")  # no chunk rows at all: the array is the unit of work
ON_PATH = tuple(k.name for k in STEP_KINDS.values() if k.make is not None)


def rows_splittable(name: str) -> bool:
    """Whether a store step's output chunk rows are independent, so that --gpus > 1 may split
    them over processes (StepKind.rows)."""
    return name not in STEP_KINDS or STEP_KINDS[name].rows


def step_encoding(step: dict, in_data_type: str):
    """The reencoding a step's output array is created with: encoding_of(step), and for a filter
    that sets its own output type (equal: bool, fill value false) that type when the step gives
    none (output_array_builder, filter_traits.rs:47-82)."""
    kind, enc = STEP_KINDS.get(step.get("filter")), encoding_of(step)
    return enc if kind is None else kind.output(step, in_data_type, enc)[1]


def _step_params(step, info):
    """(filter object, output shape, output data type) of a run-config step on an input array."""
    kind = STEP_KINDS[step.get("filter")]
    f = kind.make(step, info)
    dt, _enc = kind.output(step, info.data_type, encoding_of(step))
    if kind.check is not None:
        kind.check(f, info, dt)
    return f, (tuple(info.shape) if kind.shape is None else kind.shape(f, info)), dt


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="zarrs_filter",
                                 description="Apply filters to a Zarr V3 array on an MI355X.")
    ap.add_argument("--exists", choices=["erase", "exit"], default="erase")
    ap.add_argument("--tmp", default=None, help="directory for temporary ($name) arrays")
    ap.add_argument("--chunk-limit", type=int, default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--skip-empty-chunks", action="store_true", help=SKIP_EMPTY_HELP)
    ap.add_argument("--stats", action="store_true", help="print per-filter stats as JSON")
    ap.add_argument("--gpus", type=int, default=1,
                    help="split every store step over this many GPUs (one process each) by "
                         "output chunk rows")
    ap.add_argument("--no-device-chain", action="store_true",
                    help="run every step store -> store, also chains of temporaries")
    ap.add_argument("--no-pointwise-fusion", action="store_true",
                    help="in a device-resident chain, launch consecutive per-element steps one "
                         "by one")
    sub = ap.add_subparsers(dest="filter")
    for kind in STEP_KINDS.values():
        if kind.make is None:
            continue
        p = sub.add_parser(kind.name.replace("_", "-"), help=kind.help)
        if kind.negative_numbers is not None:
            # argparse would take such arguments for options. This sets argparse's
            # `_negative_number_matcher`, an undocumented attribute of ArgumentParser (CPython
            # 3.2 to 3.13 consult it in `_parse_optional`): an argument that matches it is a
            # positional as long as the parser has no option that looks like a negative number.
            # tests/test_pointwise.py (test_subcommand_grammar_of_the_six) fails if a Python
            # version stops honouring it.
            p._negative_number_matcher = kind.negative_numbers
        p.add_argument("input")
        p.add_argument("output")
        if kind.arguments is not None:
            kind.arguments(p)
        _add_reencode_args(p)
    return ap


def _steps_from_cli(a) -> list:
    if a.filter is None:
        return []
    kind = STEP_KINDS[a.filter.replace("-", "_")]
    own, last = kind.own(a) if callable(kind.own) else ({k: getattr(a, k) for k in kind.own}, {})
    return [{"filter": kind.name, "input": a.input, "output": a.output, **own,
             "data_type": a.data_type, "chunk_limit": a.filter_chunk_limit, **_reencode_of(a),
             **last}]


def _is_named_temp(p) -> bool:
    return isinstance(p, str) and p.startswith("$")


def _is_temp(p) -> bool:
    return p is None or _is_named_temp(p)


def plan_chains(steps: list) -> list:
    """Maximal runs [i, j] of steps (j > i) where every step before j hands its output to the next
    step only: the output is a temporary (a "$name", or omitted) and the next step reads it (its
    input is that "$name", or omitted = the previous output), and no other step names it, as
    its input, output, (arithmetic) "other" or (reconstruction) "marker". An arithmetic step and
    a reconstruction step with a marker array are never part of a chain."""
    refs: dict = {}
    for st in steps:
        for key in ("input", "output", "other", "marker"):
            v = st.get(key)
            if _is_named_temp(v):
                refs[v] = refs.get(v, 0) + 1

    def may_chain(st):
        kind = STEP_KINDS.get(st.get("filter"))
        return (kind is None or kind.chain) and st.get("marker") is None

    def linked(k):
        if not (may_chain(steps[k]) and may_chain(steps[k + 1])):
            return False
        out, nxt = steps[k].get("output"), steps[k + 1].get("input")
        if not _is_temp(out):
            return False
        if out is None:
            return nxt is None
        return nxt in (out, None) and refs.get(out, 0) == (2 if nxt == out else 1)

    chains, i = [], 0
    while i < len(steps):
        j = i
        while j + 1 < len(steps) and linked(j):
            j += 1
        if j > i:
            chains.append((i, j))
        i = j + 1
    return chains


def _nbytes(shape, data_type) -> int:
    n = 1
    for s in shape:
        n *= int(s)
    return n * S.NUMPY[data_type]().itemsize


def allocation_refused(e: BaseException) -> bool:
    """True for a refused device or pinned-host allocation (the callers then fall back to the
    store -> store path); False for everything else, FilterError (storage, codecs) included."""
    import torch
    if isinstance(e, _abi.FilterError):
        return False
    if isinstance(e, torch.cuda.OutOfMemoryError):
        return True
    msg = str(e).lower()
    return isinstance(e, RuntimeError) and ("out of memory" in msg or "pinned" in msg or
                                            "hiphostmalloc" in msg or "cudahostalloc" in msg)


def plan_pointwise_fusion(names: list, fuse: bool = True, max_ops: int = 8) -> list:
    """The launches of a device-resident chain: [(i, j)] covering every step in order, (i, j)
    with j > i a maximal run of consecutive per-element steps (at most `max_ops`, a longer run is
    split) that becomes one kernel launch; every other step, and every step with fuse=False, is
    its own (i, i)."""
    groups, i = [], 0
    while i < len(names):
        j = i
        if fuse and names[i] in POINTWISE:
            while j + 1 < len(names) and names[j + 1] in POINTWISE and j + 1 - i < max_ops:
                j += 1
        groups.append((i, j))
        i = j + 1
    return groups


def run_device_chain(steps: list, paths: list, device: int = 0, nthreads: int = 0,
                     log=print, budget_frac: float = 0.8, fuse_pointwise: bool = True):
    """Run steps[0..] device-resident: paths[k] is step k's input path (paths[k+1] its output).
    Creates every output array as the store path would (S.create_output), reads paths[0] once,
    applies the filters on HBM arrays, writes the last output once. A run of consecutive
    per-element steps (plan_pointwise_fusion) is one launch whose intermediates are never
    materialised; their zarr.json are created all the same. Returns per-step stats (a
    fused-away step reports kernel_s 0 and `fused_into`, the step that carries the launch), or
    None (nothing done) when the chain's arrays do not fit `budget_frac` of the free device
    memory, in which case the caller runs it store -> store."""
    import torch
    # shapes / types of every array of the chain (metadata only)
    plan, info = [], S.open_array(paths[0])
    for k, step in enumerate(steps):
        f, oshape, odt = _step_params(step, info)
        plan.append((f, info, oshape, odt))
        info = S.ArrayInfo(paths[k + 1], odt, tuple(oshape), info.chunk_shape,
                           info.inner_chunk_shape)
    groups = plan_pointwise_fusion([st.get("filter") for st in steps], fuse_pointwise,
                                   _abi.PW_MAX_OPS)
    # only the arrays that are materialised count: each launch's input and output
    peak = max(_nbytes(plan[i][1].shape, plan[i][1].data_type) + _nbytes(plan[j][2], plan[j][3])
               for i, j in groups)
    # a whole-array step's scratch (the labelling's two index arrays, the distance transform's
    # work arrays and stacks) is larger than its input + output: count it
    whole = max([plan[k][0].memory(plan[k][1].data_type, plan[k][3], plan[k][2])
                 for k, st in enumerate(steps) if st.get("filter") in WHOLE_ARRAY], default=0)
    free, _total = torch.cuda.mem_get_info(device)
    # in + out of a step, plus filter scratch of the same order
    if max(2 * peak, whole) > budget_frac * free:
        return None
    # the chain input and the last output each pass through one pinned host buffer
    src0 = S.open_array(paths[0])
    host_need = max(_nbytes(src0.shape, src0.data_type), _nbytes(plan[-1][2], plan[-1][3]))
    if host_need > budget_frac * S.host_available_bytes():
        return None
    results = []
    t0 = time.perf_counter()
    src_info = S.open_array(paths[0])
    try:
        x = read_to_device(paths[0], device, nthreads)
    except RuntimeError as e:
        if not allocation_refused(e):
            raise  # storage / codec errors (FilterError) are real failures
        return None  # pinned host or device allocation refused: the store path instead
    t_read = time.perf_counter() - t0
    for k, step in enumerate(steps):
        f, src_info_k, oshape, odt = plan[k]
        S.create_output(paths[k], paths[k + 1], odt, oshape,
                        step_encoding(step, src_info_k.data_type))
    # The last output is "not finished" (no zarr.json, zarrs_filter.rs:297-313) until its chunks
    # are written; a failing step leaves no output that looks complete. Held only once the input
    # is on the device, so a fallback to the store path never leaves a stale pending file.
    S.hold_metadata(paths[-1])
    dev = torch.device("cuda", device)
    x_dt, x_chunk = src_info.data_type, src_info.chunk_shape
    ctx = F.default_context(device)
    for i, j in groups:
        out_info = S.open_array(paths[j + 1])
        y = torch.empty(tuple(out_info.shape), dtype=F.torch_dtype(out_info.data_type), device=dev)
        names = "+".join(str(steps[k].get("filter")) for k in range(i, j + 1))
        t1 = time.perf_counter()
        ret = None
        if j > i:
            prog = F.PointwiseProgram([plan[k][0] for k in range(i, j + 1)], x_dt,
                                      [plan[k][3] for k in range(i, j + 1)], x.shape)
            prog.run(x, y, ctx)
        else:
            ret = plan[i][0].apply(F.DeviceArray(x, x_chunk, x_dt),
                                   F.DeviceArray(y, out_info.chunk_shape, out_info.data_type),
                                   ctx=ctx)
        ctx.synchronize()
        t_k = time.perf_counter() - t1
        log(f"{i if j == i else f'{i}-{j}'}: {names} device-resident {list(x.shape)} {x_dt} -> "
            f"{list(y.shape)} {out_info.data_type} in {t_k:.3f}s")
        reports = STEP_KINDS[names].reports if j == i else None  # the steps with a count
        if reports:
            log(f"   {int(ret)} {reports}")
        if names in WHOLE_ARRAY:
            ctx.release_scratch()  # whole-array scratch: not held through the rest of the chain
        for k in range(i, j + 1):
            carrier = k == j
            st = {"wall_s": t_k if carrier else 0.0, "decode_s": t_read if k == 0 else 0.0,
                  "encode_s": 0.0, "h2d_s": 0.0, "kernel_s": t_k if carrier else 0.0,
                  "d2h_s": 0.0, "bytes_read": 0, "bytes_written": 0,
                  "voxels": int(y.numel()) if carrier else 0, "rows": 0, "threads": nthreads,
                  "device_resident": True}
            if j > i:
                st["fused_into" if not carrier else "fused_steps"] = (
                    j if not carrier else list(range(i, j + 1)))
            if reports:
                st[reports] = int(ret)
            results.append(st)
        x, x_dt, x_chunk = y, out_info.data_type, out_info.chunk_shape
    t2 = time.perf_counter()
    results[-1]["chunks_elided"] = write_from_device(paths[-1], x, nthreads)
    S.publish_metadata(paths[-1])  # finished
    results[-1]["encode_s"] = time.perf_counter() - t2
    return results


def _rows_worker(name: str, src: str, dst: str, params: dict, device: int, rows, nthreads: int,
                 env=None):
    """One process of a multi-GPU store step: output chunk rows [rows[0], rows[1]) on `device`,
    no metadata writes (the parent writes zarr.json once every row is done). `env`: the memory
    budget of this process (ZT_STORE_HOST_MEMORY / ZT_STORE_DEVICE_MEMORY, its share)."""
    os.environ.update(env or {})
    S.set_store_empty_chunks(params.get("store_empty_chunks", True))
    kind = STEP_KINDS.get(name)
    if kind is None or not kind.rows:
        raise _abi.FilterError(_abi.ERR_OTHER, f"no store step for filter {name!r}")
    kw = {}
    if isinstance(rows, tuple) and len(rows) == 2 and isinstance(rows[0], tuple):
        rows, kw["cols"] = rows  # ((row range), (column range)): a (t, z) block
    return kind.store(src, dst, params, device=device, rows=rows, nthreads=nthreads, erase=False,
                      finish=False, encoding=params.get("encoding"),
                      data_type=params.get("data_type"),
                      chunk_limit=params.get("chunk_limit") or 0, **kw)


def run_rows_parallel(name: str, src: str, dst: str, params: dict, out_shape, gpus: int,
                      nthreads: int = 0, devices=None) -> dict:
    """A store step split over `gpus` processes (one per GPU, guided_filter.rs:260-316's chunk
    loop partitioned into contiguous output chunk rows along axis 0; no data exchange: each
    process reads its rows' inputs with their halo). The output's zarr.json is written once, by
    the parent, after every process finished (zarrs_filter.rs:297-313). `devices` maps process
    g to a device (default g; a 1-GPU rehearsal passes [0] * gpus)."""
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    info = S.open_array(src)
    S.create_output(src, dst, params.get("data_type"), out_shape, params.get("encoding"))
    out = S.open_array(dst)
    os.remove(os.path.join(dst, "zarr.json"))  # "not finished" until every row is written
    nrows = -(-out.shape[0] // out.chunk_shape[0])
    bounds = [(g * nrows // gpus, (g + 1) * nrows // gpus) for g in range(gpus)]
    if name == "guided_filter" and len(out.shape) >= 4 and gpus > 1:
        # 4-D series (config T): (t, z) blocks of whole chunks that minimise the input the
        # processes decode and filter in all, halo included (shard.block_split): rows along t
        # alone would make each process decode 3x its output timepoints
        from . import shard
        halo = (2 * int(params["radius"])) & 0xFF
        groups = shard.block_split(gpus, out.shape, out.chunk_shape, halo)
        if groups[1] > 1:
            ncol = -(-out.shape[1] // out.chunk_shape[1])
            bounds = []
            for g in range(gpus):
                k0, k1 = g // groups[1], g % groups[1]
                bounds.append(((k0 * nrows // groups[0], (k0 + 1) * nrows // groups[0]),
                               (k1 * ncol // groups[1], (k1 + 1) * ncol // groups[1])))
    devices = devices or list(range(gpus))
    per = max(1, (nthreads or min(16, os.cpu_count() or 1)) // gpus)
    params = dict(params)
    params["store_empty_chunks"] = S.store_empty_chunks()  # the processes inherit the setting
    if params.get("chunk_limit"):  # the reference's limit is per process: split it N ways
        params["chunk_limit"] = max(1, int(params["chunk_limit"]) // gpus)
    # each process budgets its share of host memory, and of device memory where processes share
    # a device (a one-GPU rehearsal), so N processes never reserve N x 80 % together
    host_share = S.host_available_bytes() // gpus
    sharing = {d: devices[:gpus].count(d) for d in set(devices[:gpus])}
    envs = []
    for g in range(gpus):
        env = {"ZT_STORE_HOST_MEMORY": str(host_share)}
        if sharing[devices[g]] > 1 and "ZT_STORE_DEVICE_MEMORY" not in os.environ:
            import torch
            free, _ = torch.cuda.mem_get_info(devices[g])
            env["ZT_STORE_DEVICE_MEMORY"] = str(free // sharing[devices[g]])
        envs.append(env)
    t0 = time.perf_counter()
    with ProcessPoolExecutor(gpus, mp_context=mp.get_context("spawn")) as ex:
        def nonempty(b):
            if isinstance(b[0], tuple):
                return b[0][1] > b[0][0] and b[1][1] > b[1][0]
            return b[1] > b[0]
        futs = [ex.submit(_rows_worker, name, src, dst, params, devices[g], bounds[g], per,
                          envs[g])
                for g in range(gpus) if nonempty(bounds[g])]
        parts = [f.result() for f in futs]
    S.create_output(src, dst, params.get("data_type"), out_shape, params.get("encoding"))
    st = {k: sum(p[k] for p in parts) for k in parts[0] if isinstance(parts[0][k], (int, float))}
    st["wall_s"] = time.perf_counter() - t0
    st["processes"] = len(parts)
    del info
    return st


def _device_ok(device: int) -> bool:
    try:
        import torch
        return torch.cuda.is_available() and device < torch.cuda.device_count()
    except Exception:
        return False


def run(steps: list, exists: str = "erase", tmp: str | None = None,
        chunk_limit: int | None = None, device: int = 0, stats: bool = False,
        log=print, device_chain: bool = True, gpus: int = 1, gpu_devices=None,
        fuse_pointwise: bool = True, skip_empty_chunks: bool = False) -> list:
    """Run a list of filter steps (the run-config form); returns the per-step stats. gpus > 1:
    every store step is split over that many processes by output chunk rows (one per GPU;
    `gpu_devices` maps process g to a device, default g); device-resident chains are then off.
    fuse_pointwise=False launches the per-element steps of a device-resident chain one by one
    (the same results, more passes over HBM). skip_empty_chunks: every output is written without
    the chunks that hold nothing but the fill value (store.set_store_empty_chunks(False) for the
    run; the setting of the calling thread is put back afterwards)."""
    store_all_before = S.store_empty_chunks()
    if skip_empty_chunks:
        S.set_store_empty_chunks(False)
    if gpus > 1:
        device_chain = False
    tmp_root = tmp or tempfile.gettempdir()
    temps: dict[str, str] = {}
    made: list[str] = []
    last_output = None
    results = []

    def resolve(p, what):
        if p is None:
            if what == "input" and last_output is not None:
                return last_output
            if what == "output":
                d = tempfile.mkdtemp(prefix="zt_", dir=tmp_root)
                made.append(d)
                return d
            raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                         "the first filter needs an input")
        if _is_named_temp(p):
            if p not in temps:
                temps[p] = tempfile.mkdtemp(prefix=p[1:] + "_", dir=tmp_root)
                made.append(temps[p])
            return temps[p]
        return p

    def prepare(dst):
        if exists == "exit" and os.path.exists(os.path.join(dst, "zarr.json")):
            raise _abi.FilterError(_abi.ERR_OTHER, f"output {dst} already exists")
        if os.path.isdir(dst) and dst not in made:
            # create_array erases the output prefix (zarrs_filter.rs:76); only the
            # temporaries this run just made (empty) are kept
            shutil.rmtree(dst)

    def store_step(i, step, src, dst):
        name = step.get("filter")
        kind = STEP_KINDS[name]
        limit = step.get("chunk_limit") or chunk_limit or 0  # chunks in flight, not threads
        info = S.open_array(src)
        if kind.second is not None and _is_named_temp(step.get(kind.second[0])):
            # written by an earlier step (checked before the run)
            step = {**step, kind.second[0]: temps[step[kind.second[0]]]}
        f, out_shape, _dt = _step_params(step, info)
        params = kind.params(f, step) if kind.params else {}
        text = kind.text(params)
        log(f"{i}: {name}{' ' + text if text else ''} {src} ({info.data_type} "
            f"{list(info.shape)}){kind.after(params) if kind.after else ''} -> {dst}")
        params.update(data_type=step.get("data_type"), encoding=encoding_of(step),
                      chunk_limit=limit)
        if gpus > 1 and kind.rows:
            # the parent creates the output: with the type and fill value of the filter's rule
            # (equal: bool, fill value false)
            params["encoding"] = step_encoding(step, info.data_type)
            st = run_rows_parallel(name, src, dst, params, out_shape, gpus, 0,
                                   devices=gpu_devices)
        else:
            dev = device
            if gpus > 1:
                dev = (gpu_devices or [0])[0]
                log(f"   {name}: chunk rows depend on each other in order; one process on device "
                    f"{dev}, not {gpus}")
            st = kind.store(src, dst, params, data_type=params["data_type"], device=dev,
                            encoding=params["encoding"], chunk_limit=limit)
        if kind.reports in st:
            log(f"   {st[kind.reports]} {kind.reports}")
        out = S.open_array(dst)
        log(f"   -> {out.data_type} {list(out.shape)} in {st['wall_s']:.2f}s "
            f"(rw:{st['decode_s']:.2f}/{st['encode_s']:.2f} p:{st['kernel_s']:.3f})")
        if stats:
            log(json.dumps({"step": i, "filter": name, **st}))
        return st


    for step in steps:
        name = step.get("filter")
        if name not in ON_PATH:
            raise _abi.FilterError(_abi.ERR_OTHER,
                                   f"filter {name!r} is outside the accelerated path "
                                   f"(supported: {', '.join(ON_PATH)})")
    written = set()  # the temporaries that the steps so far write
    for step in steps:
        kind = STEP_KINDS[step["filter"]]
        if kind.second is not None:
            key, value_of = kind.second
            ref = value_of(step)
            if _is_named_temp(ref) and ref not in written:
                raise _invalid(f"{kind.name}: {key} {ref} is not the output of an earlier step")
        if _is_named_temp(step.get("output")):
            written.add(step["output"])
    chains = dict(plan_chains(steps)) if device_chain and _device_ok(device) else {}
    t_all = time.perf_counter()
    if sys.stderr.isatty():
        def _show(p):
            sys.stderr.write(f"\r  {p['step']}/{p['num_steps']} rw:{p['read_s']:.2f}/"
                             f"{p['write_s']:.2f} p:{p['process_s']:.3f}")
            if p["step"] == p["num_steps"]:
                sys.stderr.write("\n")
            sys.stderr.flush()
        S.set_progress_callback(_show)
    try:
        i = 0
        while i < len(steps):
            j = chains.get(i, i)
            paths = [resolve(steps[i].get("input"), "input")]
            for k in range(i, j + 1):
                d = resolve(steps[k].get("output"), "output")
                prepare(d)
                paths.append(d)
                last_output = d
            res = None
            if j > i:
                threads = chunk_limit or 0
                res = run_device_chain(steps[i:j + 1], paths, device, threads, log,
                                       fuse_pointwise=fuse_pointwise)
                if res is not None and stats:
                    for k, st in enumerate(res):
                        log(json.dumps({"step": i + k, "filter": steps[i + k].get("filter"), **st}))
            if res is None:  # one step, or a chain too large for the device: store -> store
                res = [store_step(k, steps[k], paths[k - i], paths[k - i + 1])
                       for k in range(i, j + 1)]
            results.extend(res)
            i = j + 1
    finally:
        S.set_store_empty_chunks(store_all_before)
        if sys.stderr.isatty():
            S.set_progress_callback(None)
        for d in made:
            shutil.rmtree(d, ignore_errors=True)
    log(f"Completed in {time.perf_counter() - t_all:.2f}s")
    return results


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    config = None
    # a leading positional JSON run config (Cli::run_config), before any subcommand
    if argv and argv[0].endswith(".json") and os.path.exists(argv[0]):
        config = argv.pop(0)
    a = build_parser().parse_args(argv)
    if config:
        with open(config) as f:
            steps = json.load(f)
        if isinstance(steps, dict):
            steps = [steps]
    else:
        try:
            steps = _steps_from_cli(a)
        except _abi.FilterError as e:  # an option conflict that argparse cannot express
            print(f"Error: {e}", file=sys.stderr)
            return 1
    if not steps:
        build_parser().print_help()
        return 2
    try:
        run(steps, a.exists, a.tmp, a.chunk_limit, a.device, a.stats,
            device_chain=not a.no_device_chain, gpus=a.gpus,
            fuse_pointwise=not a.no_pointwise_fusion,
            skip_empty_chunks=a.skip_empty_chunks or getattr(a, "filter_skip_empty_chunks", False))
    except _abi.FilterError as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
