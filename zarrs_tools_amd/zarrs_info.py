"""zarrs_info — information about a Zarr V3 array or group, JSON encoded (src/bin/zarrs_info.rs).

    zarrs_info [--chunk-limit N] [--device D] PATH COMMAND

COMMAND (zarrs_info.rs:42-62): metadata, metadata-v3, attributes, shape, data-type, fill-value,
dimension-names, range, histogram N_BINS MIN MAX, and the extension label-statistics [--intensity
PATH] [--n-labels K] [--max-labels N]. The first seven read zarr.json and need no GPU;
metadata, metadata-v3 and attributes also work on a group (:92-109). `range` and `histogram` run
the store path's reductions on the GPU (store.range / store.histogram; src/info/range.rs,
src/info/histogram.rs). The store is V3 only, so metadata-v3 prints the document of metadata
without a `_zarrs` attribute (:79-84). Errors print their message and give a non-zero status
(:64-71).

Where this differs from the reference, deliberately: `range` gives the smallest
and largest element, as the reference documents it; both reductions count only the elements
inside the array's shape; a `bool` array, `n_bins == 0` and a non-finite MIN or MAX are errors
where the reference panics.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

from . import _abi

GROUP_COMMANDS = ("metadata", "metadata-v3", "attributes")
# `{:?}` of the InfoCommand variants (zarrs_info.rs:106-108)
_DEBUG_NAMES = {"shape": "Shape", "data-type": "DataType", "fill-value": "FillValue",
                "dimension-names": "DimensionNames", "range": "Range",
                "label-statistics": "LabelStatistics"}
DEFAULT_MAX_LABELS = 1_000_000


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(
        prog="zarrs_info", description="Get information about a Zarr array or group. Outputs "
        "are JSON encoded.")
    ap.add_argument("--chunk-limit", type=int, default=0,
                    help="The maximum number of chunks concurrently processed (0: bounded by "
                    "memory only).")
    ap.add_argument("--device", type=int, default=0, help="The GPU range and histogram run on.")
    ap.add_argument("path", help="Path to the Zarr input array or group.")
    sub = ap.add_subparsers(dest="command", required=True, metavar="COMMAND")
    for name, text in (("metadata", "Get the array/group metadata."),
                       ("metadata-v3", "Get the array/group metadata (interpreted as V3)."),
                       ("attributes", "Get the array/group attributes."),
                       ("shape", "Get the array shape."),
                       ("data-type", "Get the array data type."),
                       ("fill-value", "Get the array fill value."),
                       ("dimension-names", "Get the array dimension names."),
                       ("range", "Get the array data range.")):
        sub.add_parser(name, help=text)
    h = sub.add_parser("histogram", help="Get the array data histogram.")
    h.add_argument("n_bins", type=int)
    h.add_argument("min", type=float)
    h.add_argument("max", type=float)
    ls = sub.add_parser("label-statistics",
                        help="Get the per-label statistics of an integer label array.")
    ls.add_argument("--intensity", default=None, metavar="PATH",
                    help="An array of the same shape whose values are reduced per label.")
    ls.add_argument("--n-labels", type=int, default=None, metavar="K",
                    help="The number of labels (default: the largest label present).")
    ls.add_argument("--max-labels", type=int, default=DEFAULT_MAX_LABELS, metavar="N",
                    help="Refuse to print more than N labels.")
    return ap


def _pretty(value) -> str:
    """serde_json::to_string_pretty: two-space indent, an empty list or object on one line."""
    return json.dumps(value, indent=2, allow_nan=False, ensure_ascii=False)


def json_number(x):
    """A range value for JSON: integers as they are, floats shortest round-trip, the infinities
    as the Zarr V3 fill-value strings, none as null."""
    if isinstance(x, float) and math.isinf(x):
        return "Infinity" if x > 0 else "-Infinity"
    return x


def _json_column(values):
    """A column for JSON: integers as integers, floats through json_number, NaN as null."""
    out = []
    for v in values.tolist():
        if isinstance(v, list):
            out.append([None if isinstance(x, float) and math.isnan(x) else json_number(x)
                        for x in v])
        else:
            out.append(None if isinstance(v, float) and math.isnan(v) else json_number(v))
    return out


def label_statistics_json(res: dict) -> dict:
    """The result of store.label_statistics as a JSON document: the columns indexed by label - 1;
    an absent label has null bounds and centroid, a label with no non-NaN intensity null minimum
    and maximum, the types without sums a null column."""
    present = (res["count"] != 0).tolist()
    doc = {"n_labels": res["n_labels"], "background": res["background"],
           "count": [int(c) for c in res["count"]]}
    for key in ("bbox_min", "bbox_max"):
        doc[key] = [row if p else None for row, p in zip(res[key].tolist(), present)]
    doc["coord_sum"] = [[int(x) for x in row] for row in res["coord_sum"].tolist()]
    doc["centroid"] = [row if p else None
                       for row, p in zip(_json_column(res["centroid"]), present)]
    if "intensity_min" in res:
        valid = res["intensity_valid"].tolist()
        for key in ("intensity_min", "intensity_max"):
            col = _json_column(res[key].astype(float) if res[key].dtype.kind == "f" else res[key])
            doc[key] = [v if ok else None for v, ok in zip(col, valid)]
        doc["intensity_sum"] = None if res["intensity_sum"] is None else \
            [int(v) for v in res["intensity_sum"]]
        doc["intensity_mean"] = None if res["intensity_mean"] is None else \
            _json_column(res["intensity_mean"])
    return doc


def _debug_command(a) -> str:
    if a.command == "histogram":
        return (f"Histogram(HistogramParams {{ n_bins: {a.n_bins}, min: {a.min!r}, "
                f"max: {a.max!r} }})")
    return _DEBUG_NAMES[a.command]


def load_metadata(path) -> dict:
    """Node::open on a filesystem store (zarrs_info.rs:89-91): the node's zarr.json."""
    p = os.path.join(os.fspath(path), "zarr.json")
    try:
        with open(p) as f:
            meta = json.load(f)
    except OSError as e:
        raise _abi.FilterError(_abi.ERR_STORAGE, f"cannot open {p}: {e.strerror}")
    except ValueError as e:
        raise _abi.FilterError(_abi.ERR_JSON, f"{p}: {e}")
    if not isinstance(meta, dict) or meta.get("zarr_format") != 3 or meta.get("node_type") not in (
            "array", "group"):
        raise _abi.FilterError(_abi.ERR_ARRAY, f"{p} is not Zarr V3 array or group metadata")
    return meta


def metadata_v3(meta: dict) -> dict:
    """The V3 document without the `_zarrs` attribute (set_include_zarrs_metadata(false), :82)."""
    out = dict(meta)
    if isinstance(out.get("attributes"), dict) and "_zarrs" in out["attributes"]:
        out["attributes"] = {k: v for k, v in out["attributes"].items() if k != "_zarrs"}
    return out


def run(a) -> str:
    meta = load_metadata(a.path)
    if a.command == "metadata":
        return _pretty(meta)
    if a.command == "metadata-v3":
        return _pretty(metadata_v3(meta))
    if a.command == "attributes":
        return _pretty(meta.get("attributes", {}))
    if meta["node_type"] == "group":
        return f"The {_debug_command(a)} command is not supported for a group"
    if a.command == "shape":
        return _pretty({"shape": meta["shape"]})
    if a.command == "data-type":
        return _pretty({"data_type": meta["data_type"]})
    if a.command == "fill-value":
        return _pretty({"fill_value": meta["fill_value"]})
    if a.command == "dimension-names":
        return _pretty({"dimension_names": meta.get("dimension_names")})
    from . import store
    if a.command == "range":
        lo, hi = store.range(a.path, device=a.device, chunk_limit=a.chunk_limit)
        return _pretty({"min": json_number(lo), "max": json_number(hi)})
    if a.command == "label-statistics":
        if a.n_labels is not None and a.n_labels > a.max_labels:
            raise _abi.InvalidParameters(
                _abi.ERR_INVALID_PARAMETERS,
                f"label-statistics: {a.n_labels} labels are more than --max-labels "
                f"{a.max_labels}; raise it, or use zarrs_tools_amd.store.label_statistics, which "
                "returns the columns as numpy arrays")
        res = store.label_statistics(a.path, a.intensity, a.n_labels, device=a.device)
        if res["n_labels"] > a.max_labels:
            raise _abi.InvalidParameters(
                _abi.ERR_INVALID_PARAMETERS,
                f"label-statistics: {res['n_labels']} labels are more than --max-labels "
                f"{a.max_labels}; raise it, or use zarrs_tools_amd.store.label_statistics, which "
                "returns the columns as numpy arrays")
        return _pretty(label_statistics_json(res))
    edges, hist = store.histogram(a.path, a.n_bins, a.min, a.max, device=a.device,
                                  chunk_limit=a.chunk_limit)
    return _pretty({"bin_edges": [float(e) for e in edges], "hist": [int(h) for h in hist]})


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    try:
        print(run(a))
    except _abi.FilterError as e:
        print(e)  # zarrs_info.rs:64-71: the message on stdout, a failure status
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
