"""``zarrs_filter`` for the on-path filters (guided_filter, downsample, gaussian,
summed_area_table, the rank filters median, minimum, maximum, the per-element reencode, crop,
rescale, clamp, equal, replace_value, the two-array arithmetic and the whole-array
connected_components, distance_transform, label_size_filter and reconstruction) over Zarr V3
stores.

Mirrors src/bin/zarrs_filter.rs (LDeakin/zarrs_tools 0.7.2) for the filters this framework
accelerates:

    python -m zarrs_tools_amd.zarrs_filter [--exists erase|exit] [--tmp DIR] [--chunk-limit N]
        [--device D] [RUN_CONFIG.json] [guided-filter IN OUT EPSILON RADIUS [--data-type T]
                                        | downsample IN OUT STRIDE [--discrete] [--data-type T]
                                        | gaussian IN OUT SIGMA KERNEL_HALF_SIZE [--data-type T]
                                        | summed-area-table IN OUT [--data-type T]
                                        | median IN OUT KERNEL_HALF_SIZE [--data-type T]
                                        | minimum IN OUT KERNEL_HALF_SIZE [--data-type T]
                                        | maximum IN OUT KERNEL_HALF_SIZE [--data-type T]
                                        | reencode IN OUT | crop IN OUT OFFSET SHAPE
                                        | rescale IN OUT MULTIPLY ADD [--add-first]
                                        | clamp IN OUT MIN MAX | equal IN OUT VALUE
                                        | replace-value IN OUT VALUE REPLACE
                                        | arithmetic IN OUT OPERATOR OTHER [--data-type T]
                                        | connected-components IN OUT [--connectivity C]
                                              [--data-type T]
                                        | distance-transform IN OUT [--spacing S[,S...]]
                                              [--squared] [--data-type T]
                                        | label-size-filter IN OUT [--min-size N] [--max-size N]
                                              [--no-relabel] [--data-type T]
                                        | reconstruction IN OUT (--marker PATH | --fill-holes
                                              | --h-maxima H | --h-minima H)
                                              [--method dilation|erosion] [--connectivity C]]

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
* a JSON run config is a list of {"filter": "guided_filter" | "downsample" | "gaussian" |
  "summed_area_table" | "median" | "minimum" | "maximum" | "reencode" | "crop" | "rescale" |
  "clamp" | "equal" | "replace_value" | "arithmetic" | "connected_components" |
  "distance_transform" | "label_size_filter" | "reconstruction", "input", "output", ...args (kernel_half_size; offset, shape, multiply, add, add_first, min, max, value, replace
  for the per-element filters; connectivity for connected_components; spacing, squared for
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
import json
import os
import re
import shutil
import sys
import tempfile
import time

import numpy as np

from . import _abi
from . import store as S
from .device_io import _read_pieces, _row_spans, read_to_device, write_from_device  # noqa: F401

POINTWISE = ("reencode", "crop", "rescale", "clamp", "equal", "replace_value")
RANK = ("median", "minimum", "maximum")
BINARY = ("arithmetic",)  # two arrays in: "input" and "other"
# no chunk rows at all: the array is the unit of work
WHOLE_ARRAY = ("connected_components", "distance_transform", "label_size_filter",
               "reconstruction")
ON_PATH = ("guided_filter", "downsample", "gaussian", "summed_area_table") + RANK + POINTWISE + \
    BINARY + WHOLE_ARRAY


def rows_splittable(name: str) -> bool:
    """Whether a store step's output chunk rows are independent, so that --gpus > 1 may split
    them over processes. A summed-area table's rows are not: each row's axis-0 sum starts from
    the previous row's last plane (summed_area_table.rs:69, :94-97). Nor are a labelling's or a
    distance transform's: a connected component may span every chunk, and the nearest background
    element may lie in any."""
    return name != "summed_area_table" and name not in WHOLE_ARRAY


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
    g = sub.add_parser("guided-filter", help="Apply a guided filter (edge preserving noise filter).")
    g.add_argument("input")
    g.add_argument("output")
    g.add_argument("epsilon", type=float)
    g.add_argument("radius", type=int)
    _add_reencode_args(g)
    d = sub.add_parser("downsample", help="Downsample an image given a stride.")
    d.add_argument("input")
    d.add_argument("output")
    d.add_argument("stride", type=_parse_stride)
    d.add_argument("--discrete", action="store_true")
    _add_reencode_args(d)
    gs = sub.add_parser("gaussian", help="Apply a Gaussian kernel.")
    gs.add_argument("input")
    gs.add_argument("output")
    gs.add_argument("sigma", type=_parse_floats)
    gs.add_argument("kernel_half_size", type=_parse_stride)
    _add_reencode_args(gs)
    sa = sub.add_parser("summed-area-table", help="Compute a summed area table (integral image).")
    sa.add_argument("input")
    sa.add_argument("output")
    _add_reencode_args(sa)
    # the per-element filters; their numbers may be negative (-1e-3 included) and VALUE may be
    # -Infinity, which argparse would otherwise take for options. This sets argparse's
    # `_negative_number_matcher`, an undocumented attribute of ArgumentParser (CPython 3.2 to
    # 3.13 consult it in `_parse_optional`): an argument that matches it is a positional as long
    # as the parser has no option that looks like a negative number. tests/test_pointwise.py
    # (test_subcommand_grammar_of_the_six) fails if a Python version stops honouring it.
    number = re.compile(r"^-(\d+\.?\d*|\d*\.\d+)([eE][-+]?\d+)?$|^-Infinity$")

    def pointwise(name, help):
        p = sub.add_parser(name, help=help)
        p._negative_number_matcher = number
        p.add_argument("input")
        p.add_argument("output")
        return p

    # the rank filters (an extension); a negative KERNEL_HALF_SIZE parses as a value and is
    # rejected as InvalidParameters when the step runs
    rank_number = re.compile(r"^-\d+(,-?\d+)*$")
    for name, what in (("median", "median"), ("minimum", "minimum (grey-scale erosion)"),
                       ("maximum", "maximum (grey-scale dilation)")):
        rk = sub.add_parser(name, help=f"Apply a {what} filter over a box neighbourhood.")
        rk._negative_number_matcher = rank_number
        rk.add_argument("input")
        rk.add_argument("output")
        rk.add_argument("kernel_half_size", type=_parse_stride)
        _add_reencode_args(rk)

    re_ = pointwise("reencode", "Reencode an array.")
    _add_reencode_args(re_)
    cr = pointwise("crop", "Crop an array given an offset and shape.")
    cr.add_argument("offset", type=_parse_stride)
    cr.add_argument("shape", type=_parse_stride)
    _add_reencode_args(cr)
    rs = pointwise("rescale", "Rescale array values given a multiplier and offset.")
    rs.add_argument("multiply", type=float)
    rs.add_argument("add", type=float)
    rs.add_argument("--add-first", action="store_true",
                    help="perform the addition before the multiplication")
    _add_reencode_args(rs)
    cl = pointwise("clamp", "Clamp values between a minimum and maximum.")
    cl.add_argument("min", type=float)
    cl.add_argument("max", type=float)
    _add_reencode_args(cl)
    eq = pointwise("equal", "Return a binary image where the input is equal to some value.")
    eq.add_argument("value", type=_parse_fill_value)
    _add_reencode_args(eq)
    rv = pointwise("replace-value", "Replace a value with another value.")
    rv.add_argument("value", type=_parse_fill_value)
    rv.add_argument("replace", type=_parse_fill_value)
    _add_reencode_args(rv)
    ar = sub.add_parser("arithmetic", help="Combine two arrays of one shape element by element.")
    ar.add_argument("input")
    ar.add_argument("output")
    ar.add_argument("operator", choices=[o.replace("_", "-") for o in _abi.AR_OPERATORS])
    ar.add_argument("other")
    _add_reencode_args(ar)
    cc = sub.add_parser("connected-components",
                        help="Label the connected sets of non-zero elements.")
    cc.add_argument("input")
    cc.add_argument("output")
    cc.add_argument("--connectivity", type=int, default=1,
                    help="neighbours differ on at most this many axes (1: faces, the default; "
                         "the rank: the full neighbourhood)")
    _add_reencode_args(cc)
    dtr = sub.add_parser("distance-transform",
                         help="Exact Euclidean distance to the nearest zero element.")
    dtr.add_argument("input")
    dtr.add_argument("output")
    dtr.add_argument("--spacing", type=_parse_stride, default=None,
                     help="the length of a step along each axis: comma delimited integers >= 1, "
                          "one per axis (default: all 1)")
    dtr.add_argument("--squared", action="store_true",
                     help="store the squared distance (an exact integer; uint32 by default)")
    _add_reencode_args(dtr)
    lsf = sub.add_parser("label-size-filter",
                         help="Keep the labels of a label array whose element count is in range.")
    lsf.add_argument("input")
    lsf.add_argument("output")
    lsf.add_argument("--min-size", type=int, default=1,
                     help="the fewest elements of a label that is kept (default 1)")
    lsf.add_argument("--max-size", type=int, default=None,
                     help="the most elements of a label that is kept (default: no bound)")
    lsf.add_argument("--no-relabel", action="store_true",
                     help="kept labels keep their values (default: renumbered 1 .. K' in "
                          "increasing order)")
    _add_reencode_args(lsf)
    rc = sub.add_parser("reconstruction",
                        help="Morphological reconstruction of a marker under the mask IN.")
    rc.add_argument("input")
    rc.add_argument("output")
    how = rc.add_mutually_exclusive_group(required=True)
    how.add_argument("--marker", default=None,
                     help="the marker: a second array of IN's shape and data type")
    how.add_argument("--fill-holes", action="store_true",
                     help="by erosion from the array's border: fills the holes of a mask of "
                          "background")
    how.add_argument("--h-maxima", type=float, default=None, metavar="H",
                     help="by dilation of IN - H: suppresses maxima lower than H")
    how.add_argument("--h-minima", type=float, default=None, metavar="H",
                     help="by erosion of IN + H: suppresses minima shallower than H")
    rc.add_argument("--method", choices=["dilation", "erosion"], default=None,
                    help="with --marker only (default dilation)")
    rc.add_argument("--connectivity", type=int, default=1,
                    help="neighbours differ on at most this many axes (1: faces, the default; "
                         "the rank: the full neighbourhood)")
    _add_reencode_args(rc)
    return ap


def _steps_from_cli(a) -> list:
    if a.filter == "guided-filter":
        return [{"filter": "guided_filter", "input": a.input, "output": a.output,
                 "epsilon": a.epsilon, "radius": a.radius, "data_type": a.data_type,
                 "chunk_limit": a.filter_chunk_limit, **_reencode_of(a)}]
    if a.filter == "downsample":
        return [{"filter": "downsample", "input": a.input, "output": a.output,
                 "stride": a.stride, "discrete": a.discrete, "data_type": a.data_type,
                 "chunk_limit": a.filter_chunk_limit, **_reencode_of(a)}]
    if a.filter == "gaussian":
        return [{"filter": "gaussian", "input": a.input, "output": a.output, "sigma": a.sigma,
                 "kernel_half_size": a.kernel_half_size, "data_type": a.data_type,
                 "chunk_limit": a.filter_chunk_limit, **_reencode_of(a)}]
    if a.filter == "summed-area-table":
        return [{"filter": "summed_area_table", "input": a.input, "output": a.output,
                 "data_type": a.data_type, "chunk_limit": a.filter_chunk_limit,
                 **_reencode_of(a)}]
    if a.filter in RANK:
        return [{"filter": a.filter, "input": a.input, "output": a.output,
                 "kernel_half_size": a.kernel_half_size, "data_type": a.data_type,
                 "chunk_limit": a.filter_chunk_limit, **_reencode_of(a)}]
    own = {"reencode": (), "crop": ("offset", "shape"),
           "rescale": ("multiply", "add", "add_first"), "clamp": ("min", "max"),
           "equal": ("value",), "replace-value": ("value", "replace")}
    if a.filter in own:
        return [{"filter": a.filter.replace("-", "_"), "input": a.input, "output": a.output,
                 **{k: getattr(a, k) for k in own[a.filter]}, "data_type": a.data_type,
                 "chunk_limit": a.filter_chunk_limit, **_reencode_of(a)}]
    if a.filter == "arithmetic":
        return [{"filter": "arithmetic", "input": a.input, "output": a.output,
                 "operator": a.operator.replace("-", "_"), "other": a.other,
                 "data_type": a.data_type, "chunk_limit": a.filter_chunk_limit,
                 **_reencode_of(a)}]
    if a.filter == "connected-components":
        return [{"filter": "connected_components", "input": a.input, "output": a.output,
                 "connectivity": a.connectivity, "data_type": a.data_type,
                 "chunk_limit": a.filter_chunk_limit, **_reencode_of(a)}]
    if a.filter == "distance-transform":
        return [{"filter": "distance_transform", "input": a.input, "output": a.output,
                 "spacing": a.spacing, "squared": a.squared, "data_type": a.data_type,
                 "chunk_limit": a.filter_chunk_limit, **_reencode_of(a)}]
    if a.filter == "label-size-filter":
        return [{"filter": "label_size_filter", "input": a.input, "output": a.output,
                 "min_size": a.min_size, "max_size": a.max_size, "relabel": not a.no_relabel,
                 "data_type": a.data_type, "chunk_limit": a.filter_chunk_limit,
                 **_reencode_of(a)}]
    if a.filter == "reconstruction":
        if a.method is not None and a.marker is None:
            raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                         "reconstruction: --method is only valid with --marker")
        mode, h = "marker", None
        if a.fill_holes:
            mode = "fill_holes"
        elif a.h_maxima is not None:
            mode, h = "h_maxima", a.h_maxima
        elif a.h_minima is not None:
            mode, h = "h_minima", a.h_minima
        step = {"filter": "reconstruction", "input": a.input, "output": a.output, "mode": mode,
                "connectivity": a.connectivity, "data_type": a.data_type,
                "chunk_limit": a.filter_chunk_limit, **_reencode_of(a)}
        if a.marker is not None:
            step.update(marker=a.marker, method=a.method or "dilation")
        if h is not None:
            step["h"] = h
        return [step]
    return []


def _is_temp(p) -> bool:
    return p is None or (isinstance(p, str) and p.startswith("$"))


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
            if isinstance(v, str) and v.startswith("$"):
                refs[v] = refs.get(v, 0) + 1

    def linked(k):
        if steps[k].get("filter") in BINARY or steps[k + 1].get("filter") in BINARY:
            return False
        if steps[k].get("marker") is not None or steps[k + 1].get("marker") is not None:
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


def pointwise_filter(step: dict):
    """The per-element filter object of a run-config step (keys as the reference's *Arguments
    structs: offset, shape; multiply, add, add_first; min, max; value; value, replace)."""
    from . import filter as F
    name = step.get("filter")

    def need(*keys):
        missing = [k for k in keys if step.get(k) is None]
        if missing:
            raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                         f"{name} needs {', '.join(missing)}")
        return [step[k] for k in keys]

    def ints(v):
        return _parse_stride(v) if isinstance(v, str) else [int(x) for x in v]

    if name == "reencode":
        return F.Reencode()
    if name == "crop":
        offset, shape = need("offset", "shape")
        return F.Crop(ints(offset), ints(shape))
    if name == "rescale":
        multiply, add = need("multiply", "add")
        return F.Rescale(float(multiply), float(add), bool(step.get("add_first", False)))
    if name == "clamp":
        lo, hi = need("min", "max")
        return F.Clamp(float(lo), float(hi))
    if name == "equal":
        return F.Equal(need("value")[0])
    if name == "replace_value":
        value, replace = need("value", "replace")
        return F.ReplaceValue(value, replace)
    raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS, f"{name} is not a per-element filter")


def arithmetic_args(step: dict):
    """(operator, other) of an arithmetic run-config step."""
    from .filter import arithmetic_operator
    missing = [k for k in ("operator", "other") if step.get(k) is None]
    if missing:
        raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                     f"arithmetic needs {', '.join(missing)}")
    arithmetic_operator(step["operator"])  # InvalidParameters for an unknown name
    return str(step["operator"]).replace("-", "_"), step["other"]


def step_encoding(step: dict, in_data_type: str):
    """The reencoding a step's output array is created with: encoding_of(step), and for a
    per-element filter that sets its own output type (equal: bool, fill value false) that type
    when the step gives none (output_array_builder, filter_traits.rs:47-82)."""
    enc = encoding_of(step)
    if step.get("filter") in POINTWISE:
        _dt, enc = S.pointwise_output(pointwise_filter(step), in_data_type,
                                      step.get("data_type"), enc)
    if step.get("filter") == "connected_components":  # labels: uint32, fill value 0
        _dt, enc = S.connected_components_output(step.get("data_type"), enc)
    if step.get("filter") == "distance_transform":  # float32, or uint32 squared; fill value 0
        _dt, enc = S.distance_transform_output(bool(step.get("squared", False)),
                                               step.get("data_type"), enc)
    if step.get("filter") == "label_size_filter":  # the input's type; fill value 0
        _dt, enc = S.label_size_filter_output(in_data_type, step.get("data_type"), enc)
    return enc


def label_size_filter_of(step: dict):
    """The size filter of a run-config step: "min_size" (default 1) and "max_size" (default
    none) integers, "relabel" a boolean (default true)."""
    from . import filter as F
    try:
        mn = 1 if step.get("min_size") is None else int(step["min_size"])
        mx = None if step.get("max_size") is None else int(step["max_size"])
    except (TypeError, ValueError):
        raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                     "label_size_filter: min_size and max_size are "
                                     "integers") from None
    relabel = step.get("relabel")
    return S.SizeFilterStep(F.LabelSizeFilter(mn, mx, True if relabel is None else bool(relabel)))


def connectivity_of(step: dict) -> int:
    """The connectivity of a connected_components run-config step (default 1: faces)."""
    c = step.get("connectivity")
    try:
        return 1 if c is None else int(c)
    except (TypeError, ValueError):
        raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                     f"connected_components: connectivity {c!r} is not an "
                                     "integer") from None


def reconstruction_of(step: dict):
    """(Reconstruction, marker) of a run-config step: "marker" a path or the "$name" of an earlier
    step's output (then "mode" is marker, or omitted), or "mode" one of fill_holes, h_maxima,
    h_minima with "h" for the last two; "method" dilation (default) or erosion, with a marker
    only; "connectivity" an integer (default 1)."""
    from . import filter as F
    marker = step.get("marker")
    mode = step.get("mode") or ("marker" if marker is not None else None)
    if mode is None:
        raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                     "reconstruction needs a marker or a mode (fill_holes, "
                                     "h_maxima, h_minima)")
    mode = str(mode).replace("-", "_")
    if (mode == "marker") != (marker is not None):
        raise _abi.InvalidParameters(
            _abi.ERR_INVALID_PARAMETERS,
            "reconstruction: mode marker needs a marker" if marker is None else
            f"reconstruction: {mode} makes its marker from the mask; no marker is given")
    if step.get("method") is not None and marker is None:
        raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                     "reconstruction: a method is only valid with a marker")
    c = step.get("connectivity")
    try:
        c = 1 if c is None else int(c)
    except (TypeError, ValueError):
        raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                     f"reconstruction: connectivity {c!r} is not an "
                                     "integer") from None
    return F.Reconstruction(step.get("method") or "dilation", c, mode, step.get("h")), marker


def distance_transform_of(step: dict):
    """The DistanceTransform of a run-config step: "spacing" a list (or a comma delimited string)
    of integers >= 1, default all 1; "squared" a boolean, default false."""
    from . import filter as F
    sp = step.get("spacing")
    if isinstance(sp, str):
        sp = [x.strip() for x in sp.split(",") if x.strip()]
        try:
            sp = [int(x) for x in sp]
        except ValueError:
            raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                         f"distance_transform: spacing {step['spacing']!r} is "
                                         "not a list of integers") from None
    elif sp is not None and not isinstance(sp, (list, tuple)):
        sp = [sp]
    return F.DistanceTransform(sp, bool(step.get("squared", False)))


def _step_params(step, info):
    """(filter object, output shape, output data type) of a run-config step on an input array."""
    from . import filter as F
    name = step.get("filter")
    if name in POINTWISE:
        f = pointwise_filter(step)
        dt, _enc = S.pointwise_output(f, info.data_type, step.get("data_type"),
                                      encoding_of(step))
        f.is_compatible(info.data_type, dt)
        f.op(info.data_type, dt)  # value / replace must fit the types
        return f, f.output_shape(info.shape), dt
    if name == "connected_components":
        f = F.ConnectedComponents(connectivity_of(step))
        dt, _enc = S.connected_components_output(step.get("data_type"), encoding_of(step))
        f.is_compatible(info.data_type, dt)
        f.check_connectivity(info.ndim)
        return f, tuple(info.shape), dt
    if name == "distance_transform":
        f = distance_transform_of(step)
        dt, _enc = S.distance_transform_output(f.squared, step.get("data_type"),
                                               encoding_of(step))
        f.is_compatible(info.data_type, dt)
        f.check_spacing(info.ndim)
        f.memory(info.data_type, dt, info.shape)  # the bound on the squared distance
        return f, tuple(info.shape), dt
    if name == "label_size_filter":
        f = label_size_filter_of(step)
        dt, _enc = S.label_size_filter_output(info.data_type, step.get("data_type"),
                                              encoding_of(step))
        f.is_compatible(info.data_type, dt)
        return f, tuple(info.shape), dt
    dt = step.get("data_type") or (encoding_of(step) or {}).get("data_type") or info.data_type
    if name == "reconstruction":
        f, _marker = reconstruction_of(step)
        if dt != info.data_type:
            raise _abi.UnsupportedDataType(
                _abi.ERR_UNSUPPORTED_DATA_TYPE,
                f"reconstruction: the output has the input's data type {info.data_type}, not {dt}")
        f.is_compatible(info.data_type)
        f.check_connectivity(info.ndim)
        return f, tuple(info.shape), dt
    if name == "guided_filter":
        if "epsilon" not in step or "radius" not in step:
            raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                         "guided_filter needs epsilon and radius")
        return F.GuidedFilter(float(step["epsilon"]), int(step["radius"])), tuple(info.shape), dt
    if name == "gaussian":
        sigma, half = step.get("sigma"), step.get("kernel_half_size")
        sigma = _parse_floats(sigma) if isinstance(sigma, str) else sigma
        half = _parse_stride(half) if isinstance(half, str) else half
        if not sigma or not half or len(sigma) != info.ndim or len(half) != info.ndim:
            raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                         "gaussian sigma and kernel_half_size need one entry "
                                         "per axis")
        return F.Gaussian(sigma, half), tuple(info.shape), dt
    if name == "summed_area_table":
        return F.SummedAreaTable(), tuple(info.shape), dt
    if name == "arithmetic":
        return F.Arithmetic(arithmetic_args(step)[0]), tuple(info.shape), dt
    if name in RANK:
        half = step.get("kernel_half_size")
        half = _parse_stride(half) if isinstance(half, str) else half
        if half is None:
            raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                         f"{name} needs kernel_half_size")
        half = [int(h) for h in half]
        F.check_rank_half(name, half, info.ndim)
        return F.RankFilter(name, half), tuple(info.shape), dt
    stride = step.get("stride")
    stride = _parse_stride(stride) if isinstance(stride, str) else stride
    if not stride or len(stride) != info.ndim:
        raise _abi.InvalidParameters(_abi.ERR_INVALID_PARAMETERS,
                                     "downsample stride must match the array rank")
    f = F.Downsample(stride, discrete=bool(step.get("discrete", False)))
    return f, f.output_shape(info.shape), dt


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
    from . import filter as F
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
        components = None
        if names in ("connected_components", "label_size_filter"):  # the steps with a count
            components = int(ret)
            log(f"   {components} components")
        if names == "reconstruction":
            log(f"   {int(ret)} rounds")
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
            if components is not None:
                st["components"] = components
            if names == "reconstruction":
                st["rounds"] = int(ret)
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
    cols = None
    if isinstance(rows, tuple) and len(rows) == 2 and isinstance(rows[0], tuple):
        rows, cols = rows  # ((row range), (column range)): a (t, z) block
    kw = dict(device=device, rows=rows, nthreads=nthreads, erase=False, finish=False,
              encoding=params.get("encoding"), data_type=params.get("data_type"),
              chunk_limit=params.get("chunk_limit") or 0)
    if name == "guided_filter":
        return S.guided_filter(src, dst, params["epsilon"], params["radius"], cols=cols, **kw)
    if name == "gaussian":
        return S.gaussian(src, dst, params["sigma"], params["kernel_half_size"], **kw)
    if name in RANK:
        return S.rank_filter(src, dst, name, params["kernel_half_size"], **kw)
    if name in POINTWISE:
        return _store_pointwise(name, src, dst, params["args"], **kw)
    if name == "arithmetic":
        return S.arithmetic(src, params["other"], dst, params["operator"], **kw)
    if name == "downsample_gaussian":  # a zarrs_ome level with --gaussian-sigma
        return S.downsample_gaussian(src, dst, params["stride"], params["sigma"],
                                     params["kernel_half_size"], **kw)
    if name != "downsample":
        raise _abi.FilterError(_abi.ERR_OTHER, f"no store step for filter {name!r}")
    return S.downsample(src, dst, params["stride"], discrete=params["discrete"], **kw)


def _store_pointwise(name: str, src: str, dst: str, args: dict, **kw) -> dict:
    """A per-element step store -> store: `args` holds the filter's own run-config keys."""
    f = pointwise_filter({"filter": name, **args})
    dt, enc = S.pointwise_output(f, S.open_array(src).data_type, kw.pop("data_type", None),
                                 kw.pop("encoding", None))
    return S.pointwise(src, dst, [f], [dt], encoding=enc, **kw)


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
        if isinstance(p, str) and p.startswith("$"):
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
        limit = step.get("chunk_limit") or chunk_limit or 0  # chunks in flight, not threads
        info = S.open_array(src)
        f, out_shape, _dt = _step_params(step, info)
        enc = encoding_of(step)
        if name == "guided_filter":
            params = {"epsilon": float(step["epsilon"]), "radius": int(step["radius"])}
            log(f"{i}: guided_filter epsilon={params['epsilon']} radius={params['radius']} "
                f"{src} ({info.data_type} {list(info.shape)}) -> {dst}")
        elif name == "gaussian":
            params = {"sigma": list(f.sigma), "kernel_half_size": list(f.kernel_half_size())}
            log(f"{i}: gaussian sigma={params['sigma']} "
                f"kernel_half_size={params['kernel_half_size']} "
                f"{src} ({info.data_type} {list(info.shape)}) -> {dst}")
        elif name == "summed_area_table":
            params = {}
            log(f"{i}: summed_area_table {src} ({info.data_type} {list(info.shape)}) -> {dst}")
        elif name in RANK:
            params = {"kernel_half_size": list(f.kernel_half_size())}
            log(f"{i}: {name} kernel_half_size={params['kernel_half_size']} "
                f"{src} ({info.data_type} {list(info.shape)}) -> {dst}")
        elif name in POINTWISE:
            own = ("offset", "shape", "multiply", "add", "add_first", "min", "max", "value",
                   "replace")
            params = {"args": {k: step[k] for k in own if step.get(k) is not None}}
            log(f"{i}: {name} {params['args']} {src} ({info.data_type} {list(info.shape)}) "
                f"-> {dst}")
            enc = step_encoding(step, info.data_type)  # equal: bool, fill value false
        elif name == "arithmetic":
            other = step["other"]
            if isinstance(other, str) and other.startswith("$"):
                other = temps[other]  # written by an earlier step (checked before the run)
            params = {"operator": f.operator, "other": str(other)}
            log(f"{i}: arithmetic {f.operator} {src} ({info.data_type} {list(info.shape)}) "
                f"with {other} -> {dst}")
        elif name == "connected_components":
            params = {"connectivity": f.connectivity}
            log(f"{i}: connected_components connectivity={f.connectivity} "
                f"{src} ({info.data_type} {list(info.shape)}) -> {dst}")
        elif name == "distance_transform":
            params = {"spacing": None if f.spacing is None else list(f.spacing),
                      "squared": f.squared}
            log(f"{i}: distance_transform spacing={params['spacing'] or 'ones'} "
                f"squared={f.squared} {src} ({info.data_type} {list(info.shape)}) -> {dst}")
        elif name == "label_size_filter":
            params = {"min_size": f.min_size, "max_size": f.max_size, "relabel": f.relabel}
            log(f"{i}: label_size_filter min_size={f.min_size} max_size={f.max_size} "
                f"relabel={f.relabel} {src} ({info.data_type} {list(info.shape)}) -> {dst}")
        elif name == "reconstruction":
            marker = reconstruction_of(step)[1]
            if isinstance(marker, str) and marker.startswith("$"):
                marker = temps[marker]  # written by an earlier step (checked before the run)
            params = {"marker": None if marker is None else str(marker), "mode": f.mode,
                      "method": f.method, "connectivity": f.connectivity,
                      "h": f.h if f.mode in ("h_maxima", "h_minima") else None}
            log(f"{i}: reconstruction mode={f.mode} method={f.method} "
                f"connectivity={f.connectivity}"
                + (f" h={f.h}" if params["h"] is not None else "")
                + f" {src} ({info.data_type} {list(info.shape)})"
                + (f" marker {marker}" if marker is not None else "") + f" -> {dst}")
        else:
            params = {"stride": list(f.stride), "discrete": bool(step.get("discrete", False))}
            log(f"{i}: downsample stride={params['stride']} discrete={params['discrete']} "
                f"{src} ({info.data_type} {list(info.shape)}) -> {dst}")
        params.update(data_type=step.get("data_type"), encoding=enc, chunk_limit=limit)

        def whole_step(dev):  # the filters whose rows cannot be split: their own store function
            if name == "connected_components":
                return S.connected_components(src, dst, params["connectivity"],
                                              data_type=params["data_type"], device=dev,
                                              encoding=enc)
            if name == "distance_transform":
                return S.distance_transform(src, dst, params["spacing"], params["squared"],
                                            data_type=params["data_type"], device=dev,
                                            encoding=enc)
            if name == "label_size_filter":
                return S.label_size_filter(src, dst, params["min_size"], params["max_size"],
                                           params["relabel"], data_type=params["data_type"],
                                           device=dev, encoding=enc)
            if name == "reconstruction":
                return S.reconstruction(src, dst, params["marker"],
                                        params["method"] if params["marker"] else "dilation",
                                        params["connectivity"], params["mode"], params["h"],
                                        data_type=params["data_type"], device=dev, encoding=enc)
            return S.summed_area_table(src, dst, data_type=params["data_type"], device=dev,
                                       encoding=enc, chunk_limit=limit)

        if gpus > 1 and not rows_splittable(name):
            dev0 = (gpu_devices or [0])[0]
            log(f"   {name}: chunk rows depend on each other in order; one process on device "
                f"{dev0}, not {gpus}")
            st = whole_step(dev0)
        elif gpus > 1:
            st = run_rows_parallel(name, src, dst, params, out_shape, gpus, 0,
                                   devices=gpu_devices)
        elif name == "guided_filter":
            st = S.guided_filter(src, dst, params["epsilon"], params["radius"],
                                 data_type=params["data_type"], device=device,
                                 encoding=enc, chunk_limit=limit)
        elif name == "gaussian":
            st = S.gaussian(src, dst, params["sigma"], params["kernel_half_size"],
                            data_type=params["data_type"], device=device, encoding=enc,
                            chunk_limit=limit)
        elif not rows_splittable(name):
            st = whole_step(device)
        elif name in RANK:
            st = S.rank_filter(src, dst, name, params["kernel_half_size"],
                               data_type=params["data_type"], device=device, encoding=enc,
                               chunk_limit=limit)
        elif name in POINTWISE:
            st = _store_pointwise(name, src, dst, params["args"], data_type=params["data_type"],
                                  device=device, encoding=enc, chunk_limit=limit)
        elif name == "arithmetic":
            st = S.arithmetic(src, params["other"], dst, params["operator"],
                              data_type=params["data_type"], device=device, encoding=enc,
                              chunk_limit=limit)
        else:
            st = S.downsample(src, dst, params["stride"], discrete=params["discrete"],
                              data_type=params["data_type"], device=device, encoding=enc,
                              chunk_limit=limit)
        if "components" in st:
            log(f"   {st['components']} components")
        if "rounds" in st:
            log(f"   {st['rounds']} rounds")
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
        if step.get("filter") in BINARY:
            other = arithmetic_args(step)[1]
            if isinstance(other, str) and other.startswith("$") and other not in written:
                raise _abi.InvalidParameters(
                    _abi.ERR_INVALID_PARAMETERS,
                    f"arithmetic: other {other} is not the output of an earlier step")
        if step.get("filter") == "reconstruction":
            marker = reconstruction_of(step)[1]
            if isinstance(marker, str) and marker.startswith("$") and marker not in written:
                raise _abi.InvalidParameters(
                    _abi.ERR_INVALID_PARAMETERS,
                    f"reconstruction: marker {marker} is not the output of an earlier step")
        out = step.get("output")
        if isinstance(out, str) and out.startswith("$"):
            written.add(out)
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
