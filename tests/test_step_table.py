"""CPU: zarrs_filter's dispatch, pinned. What every filter name turns into (its sub-parser, the
store function a step reaches and the arguments it is called with, on one GPU and in a worker of
a multi-GPU split, and the lines it logs), with the expectations written out as literals, so that
a change to how the steps are described cannot change what a step does. No device is needed: the
store functions are replaced by recorders."""
import argparse
import inspect
import json

import pytest

from zarrs_tools_amd import _abi
from zarrs_tools_amd import device_io
from zarrs_tools_amd import store as S
from zarrs_tools_amd import zarrs_filter as ZF

ON_PATH = ("guided_filter", "downsample", "gaussian", "summed_area_table", "median", "minimum",
           "maximum", "reencode", "crop", "rescale", "clamp", "equal", "replace_value",
           "arithmetic", "connected_components", "distance_transform", "label_size_filter",
           "reconstruction")


def test_the_name_tuples_keep_their_values_and_order():
    assert ZF.POINTWISE == ("reencode", "crop", "rescale", "clamp", "equal", "replace_value")
    assert ZF.RANK == ("median", "minimum", "maximum")
    assert ZF.BINARY == ("arithmetic",)
    assert ZF.WHOLE_ARRAY == ("connected_components", "distance_transform", "label_size_filter",
                              "reconstruction")
    assert ZF.ON_PATH == ON_PATH
    assert [n for n in ON_PATH if not ZF.rows_splittable(n)] == [
        "summed_area_table", "connected_components", "distance_transform", "label_size_filter",
        "reconstruction"]
    assert ZF.rows_splittable("downsample_gaussian")


# ---------------------------------------------------------------------------------------------
# the parser

SKIP_EMPTY = ("do not store chunks (or inner chunks of shards) that hold nothing but the fill "
              "value, and remove such chunks of an output being overwritten (zarrs' "
              "store_empty_chunks = false)")
CONNECTIVITY_HELP = ("neighbours differ on at most this many axes (1: faces, the default; the "
                     "rank: the full neighbourhood)")
# (option_strings, dest, nargs, default, choices, required, help, type's name)
HEAD = [
    (("-h", "--help"), "help", 0, "==SUPPRESS==", None, False, "show this help message and exit",
     None),
    ((), "input", None, None, None, True, None, None),
    ((), "output", None, None, None, True, None, None),
]
REENCODE = [
    (("-d", "--data-type"), "data_type", None, None, None, False, None, None),
    (("-f", "--fill-value"), "fill_value", None, None, None, False, None, "_parse_fill_value"),
    (("--separator",), "separator", None, None, ["/", "."], False, None, None),
    (("-c", "--chunk-shape"), "chunk_shape", None, None, None, False, None, "_parse_stride"),
    (("-s", "--shard-shape"), "shard_shape", None, None, None, False, None, "_parse_stride"),
    (("--array-to-array-codecs",), "array_to_array_codecs", None, None, None, False, None, None),
    (("--array-to-bytes-codec",), "array_to_bytes_codec", None, None, None, False, None, None),
    (("--bytes-to-bytes-codecs",), "bytes_to_bytes_codecs", None, None, None, False, None, None),
    (("--dimension-names",), "dimension_names", None, None, None, False, None, "<lambda>"),
    (("--attributes",), "attributes", None, None, None, False, None, None),
    (("--attributes-append",), "attributes_append", None, None, None, False, None, None),
    (("--chunk-limit",), "filter_chunk_limit", None, None, None, False, None, "int"),
    (("--skip-empty-chunks",), "filter_skip_empty_chunks", 0, False, None, False, SKIP_EMPTY,
     None),
]
HALF = [((), "kernel_half_size", None, None, None, True, None, "_parse_stride")]
VALUE = [((), "value", None, None, None, True, None, "_parse_fill_value")]
# the sub-parser's help, its own actions (between HEAD and REENCODE) and the pattern of its
# negative-number matcher when it is not argparse's own
NUMBER = r"^-(\d+\.?\d*|\d*\.\d+)([eE][-+]?\d+)?$|^-Infinity$"
RANK_NUMBER = r"^-\d+(,-?\d+)*$"
PARSERS = {
    "guided-filter": ("Apply a guided filter (edge preserving noise filter).", [
        ((), "epsilon", None, None, None, True, None, "float"),
        ((), "radius", None, None, None, True, None, "int")], None),
    "downsample": ("Downsample an image given a stride.", [
        ((), "stride", None, None, None, True, None, "_parse_stride"),
        (("--discrete",), "discrete", 0, False, None, False, None, None)], None),
    "gaussian": ("Apply a Gaussian kernel.", [
        ((), "sigma", None, None, None, True, None, "_parse_floats")] + HALF, None),
    "summed-area-table": ("Compute a summed area table (integral image).", [], None),
    "median": ("Apply a median filter over a box neighbourhood.", HALF, RANK_NUMBER),
    "minimum": ("Apply a minimum (grey-scale erosion) filter over a box neighbourhood.", HALF,
                RANK_NUMBER),
    "maximum": ("Apply a maximum (grey-scale dilation) filter over a box neighbourhood.", HALF,
                RANK_NUMBER),
    "reencode": ("Reencode an array.", [], NUMBER),
    "crop": ("Crop an array given an offset and shape.", [
        ((), "offset", None, None, None, True, None, "_parse_stride"),
        ((), "shape", None, None, None, True, None, "_parse_stride")], NUMBER),
    "rescale": ("Rescale array values given a multiplier and offset.", [
        ((), "multiply", None, None, None, True, None, "float"),
        ((), "add", None, None, None, True, None, "float"),
        (("--add-first",), "add_first", 0, False, None, False,
         "perform the addition before the multiplication", None)], NUMBER),
    "clamp": ("Clamp values between a minimum and maximum.", [
        ((), "min", None, None, None, True, None, "float"),
        ((), "max", None, None, None, True, None, "float")], NUMBER),
    "equal": ("Return a binary image where the input is equal to some value.", VALUE, NUMBER),
    "replace-value": ("Replace a value with another value.", VALUE + [
        ((), "replace", None, None, None, True, None, "_parse_fill_value")], NUMBER),
    "arithmetic": ("Combine two arrays of one shape element by element.", [
        ((), "operator", None, None,
         ["add", "subtract", "multiply", "divide", "minimum", "maximum", "absolute-difference"],
         True, None, None),
        ((), "other", None, None, None, True, None, None)], None),
    "connected-components": ("Label the connected sets of non-zero elements.", [
        (("--connectivity",), "connectivity", None, 1, None, False, CONNECTIVITY_HELP, "int")],
        None),
    "distance-transform": ("Exact Euclidean distance to the nearest zero element.", [
        (("--spacing",), "spacing", None, None, None, False,
         "the length of a step along each axis: comma delimited integers >= 1, one per axis "
         "(default: all 1)", "_parse_stride"),
        (("--squared",), "squared", 0, False, None, False,
         "store the squared distance (an exact integer; uint32 by default)", None)], None),
    "label-size-filter": ("Keep the labels of a label array whose element count is in range.", [
        (("--min-size",), "min_size", None, 1, None, False,
         "the fewest elements of a label that is kept (default 1)", "int"),
        (("--max-size",), "max_size", None, None, None, False,
         "the most elements of a label that is kept (default: no bound)", "int"),
        (("--no-relabel",), "no_relabel", 0, False, None, False,
         "kept labels keep their values (default: renumbered 1 .. K' in increasing order)",
         None)], None),
    "reconstruction": ("Morphological reconstruction of a marker under the mask IN.", [
        (("--marker",), "marker", None, None, None, False,
         "the marker: a second array of IN's shape and data type", None),
        (("--fill-holes",), "fill_holes", 0, False, None, False,
         "by erosion from the array's border: fills the holes of a mask of background", None),
        (("--h-maxima",), "h_maxima", None, None, None, False,
         "by dilation of IN - H: suppresses maxima lower than H", "float"),
        (("--h-minima",), "h_minima", None, None, None, False,
         "by erosion of IN + H: suppresses minima shallower than H", "float"),
        (("--method",), "method", None, None, ["dilation", "erosion"], False,
         "with --marker only (default dilation)", None),
        (("--connectivity",), "connectivity", None, 1, None, False, CONNECTIVITY_HELP, "int")],
        None),
}


def _action(a):
    return (tuple(a.option_strings), a.dest, a.nargs, a.default,
            None if a.choices is None else list(a.choices), a.required, a.help,
            a.type.__name__ if a.type is not None else None)


def _subparsers():
    ap = ZF.build_parser()
    return ap, next(a for a in ap._actions if isinstance(a, argparse._SubParsersAction))


def test_the_sub_parsers_and_their_order():
    _ap, sub = _subparsers()
    assert list(sub.choices) == list(PARSERS)
    assert [(c.dest, c.help) for c in sub._choices_actions] == [
        (name, PARSERS[name][0]) for name in PARSERS]
    assert sub.dest == "filter"


@pytest.mark.parametrize("name", list(PARSERS))
def test_a_sub_parsers_actions(name):
    _ap, sub = _subparsers()
    p = sub.choices[name]
    assert [_action(a) for a in p._actions] == HEAD + PARSERS[name][1] + REENCODE
    default = argparse.ArgumentParser()._negative_number_matcher.pattern
    assert p._negative_number_matcher.pattern == (PARSERS[name][2] or default)
    groups = [(g.required, [a.dest for a in g._group_actions])
              for g in p._mutually_exclusive_groups]
    assert groups == ([(True, ["marker", "fill_holes", "h_maxima", "h_minima"])]
                      if name == "reconstruction" else [])
    metavars = {a.dest: a.metavar for a in p._actions if a.metavar is not None}
    assert metavars == ({"h_maxima": "H", "h_minima": "H"} if name == "reconstruction" else {})


def test_the_top_level_options():
    ap, _sub = _subparsers()
    assert [_action(a)[:6] + _action(a)[7:] for a in ap._actions[:-1]] == [
        (("-h", "--help"), "help", 0, "==SUPPRESS==", None, False, None),
        (("--exists",), "exists", None, "erase", ["erase", "exit"], False, None),
        (("--tmp",), "tmp", None, None, None, False, None),
        (("--chunk-limit",), "chunk_limit", None, None, None, False, "int"),
        (("--device",), "device", None, 0, None, False, "int"),
        (("--skip-empty-chunks",), "skip_empty_chunks", 0, False, None, False, None),
        (("--stats",), "stats", 0, False, None, False, None),
        (("--gpus",), "gpus", None, 1, None, False, "int"),
        (("--no-device-chain",), "no_device_chain", 0, False, None, False, None),
        (("--no-pointwise-fusion",), "no_pointwise_fusion", 0, False, None, False, None)]


# the step dict of every subcommand, key order included
CLI_STEPS = [
    (["guided-filter", "i", "o", "0.5", "2", "--chunk-limit", "3"],
     [("filter", "guided_filter"), ("input", "i"), ("output", "o"), ("epsilon", 0.5),
      ("radius", 2), ("data_type", None), ("chunk_limit", 3)]),
    (["downsample", "i", "o", "2,2", "--discrete", "-d", "uint8", "-c", "4,4"],
     [("filter", "downsample"), ("input", "i"), ("output", "o"), ("stride", [2, 2]),
      ("discrete", True), ("data_type", "uint8"), ("chunk_limit", None),
      ("chunk_shape", [4, 4])]),
    (["gaussian", "i", "o", "1,1.5", "2,3"],
     [("filter", "gaussian"), ("input", "i"), ("output", "o"), ("sigma", [1.0, 1.5]),
      ("kernel_half_size", [2, 3]), ("data_type", None), ("chunk_limit", None)]),
    (["summed-area-table", "i", "o", "-f", "1"],
     [("filter", "summed_area_table"), ("input", "i"), ("output", "o"), ("data_type", None),
      ("chunk_limit", None), ("fill_value", 1)]),
    (["median", "i", "o", "1,0"],
     [("filter", "median"), ("input", "i"), ("output", "o"), ("kernel_half_size", [1, 0]),
      ("data_type", None), ("chunk_limit", None)]),
    (["minimum", "i", "o", "-1,0"],
     [("filter", "minimum"), ("input", "i"), ("output", "o"), ("kernel_half_size", [-1, 0]),
      ("data_type", None), ("chunk_limit", None)]),
    (["maximum", "i", "o", "2"],
     [("filter", "maximum"), ("input", "i"), ("output", "o"), ("kernel_half_size", [2]),
      ("data_type", None), ("chunk_limit", None)]),
    (["reencode", "i", "o", "-d", "int8"],
     [("filter", "reencode"), ("input", "i"), ("output", "o"), ("data_type", "int8"),
      ("chunk_limit", None)]),
    (["crop", "i", "o", "1,0", "2,3"],
     [("filter", "crop"), ("input", "i"), ("output", "o"), ("offset", [1, 0]),
      ("shape", [2, 3]), ("data_type", None), ("chunk_limit", None)]),
    (["rescale", "i", "o", "2", "-1e-3", "--add-first"],
     [("filter", "rescale"), ("input", "i"), ("output", "o"), ("multiply", 2.0),
      ("add", -0.001), ("add_first", True), ("data_type", None), ("chunk_limit", None)]),
    (["clamp", "i", "o", "-1", "1"],
     [("filter", "clamp"), ("input", "i"), ("output", "o"), ("min", -1.0), ("max", 1.0),
      ("data_type", None), ("chunk_limit", None)]),
    (["equal", "i", "o", "-Infinity"],
     [("filter", "equal"), ("input", "i"), ("output", "o"), ("value", "-Infinity"),
      ("data_type", None), ("chunk_limit", None)]),
    (["replace-value", "i", "o", "0", "7"],
     [("filter", "replace_value"), ("input", "i"), ("output", "o"), ("value", 0),
      ("replace", 7), ("data_type", None), ("chunk_limit", None)]),
    (["arithmetic", "i", "o", "absolute-difference", "b"],
     [("filter", "arithmetic"), ("input", "i"), ("output", "o"),
      ("operator", "absolute_difference"), ("other", "b"), ("data_type", None),
      ("chunk_limit", None)]),
    (["connected-components", "i", "o", "--connectivity", "2"],
     [("filter", "connected_components"), ("input", "i"), ("output", "o"), ("connectivity", 2),
      ("data_type", None), ("chunk_limit", None)]),
    (["distance-transform", "i", "o", "--spacing", "2,1", "--squared"],
     [("filter", "distance_transform"), ("input", "i"), ("output", "o"), ("spacing", [2, 1]),
      ("squared", True), ("data_type", None), ("chunk_limit", None)]),
    (["label-size-filter", "i", "o", "--min-size", "2", "--max-size", "5", "--no-relabel"],
     [("filter", "label_size_filter"), ("input", "i"), ("output", "o"), ("min_size", 2),
      ("max_size", 5), ("relabel", False), ("data_type", None), ("chunk_limit", None)]),
    (["reconstruction", "i", "o", "--h-maxima", "1.5", "-d", "uint8"],
     [("filter", "reconstruction"), ("input", "i"), ("output", "o"), ("mode", "h_maxima"),
      ("connectivity", 1), ("data_type", "uint8"), ("chunk_limit", None), ("h", 1.5)]),
    (["reconstruction", "i", "o", "--marker", "m", "--connectivity", "2"],
     [("filter", "reconstruction"), ("input", "i"), ("output", "o"), ("mode", "marker"),
      ("connectivity", 2), ("data_type", None), ("chunk_limit", None), ("marker", "m"),
      ("method", "dilation")]),
    (["reconstruction", "i", "o", "--fill-holes"],
     [("filter", "reconstruction"), ("input", "i"), ("output", "o"), ("mode", "fill_holes"),
      ("connectivity", 1), ("data_type", None), ("chunk_limit", None)]),
]


@pytest.mark.parametrize("argv, items", CLI_STEPS, ids=[" ".join(c[0][:1] + c[0][3:])
                                                        for c in CLI_STEPS])
def test_the_step_dict_of_a_subcommand(argv, items):
    steps = ZF._steps_from_cli(ZF.build_parser().parse_args(argv))
    assert [list(st.items()) for st in steps] == [items]


def test_no_subcommand_and_a_method_without_a_marker():
    assert ZF._steps_from_cli(ZF.build_parser().parse_args([])) == []
    a = ZF.build_parser().parse_args(["reconstruction", "i", "o", "--fill-holes", "--method",
                                      "erosion"])
    with pytest.raises(_abi.InvalidParameters, match="--method is only valid with --marker"):
        ZF._steps_from_cli(a)


# ---------------------------------------------------------------------------------------------
# dispatch: the store functions are recorders

STORE_FUNCTIONS = ("guided_filter", "downsample", "gaussian", "summed_area_table", "rank_filter",
                   "pointwise", "arithmetic", "connected_components", "distance_transform",
                   "label_size_filter", "reconstruction", "downsample_gaussian")
CANNED = {"wall_s": 1.0, "decode_s": 0.25, "encode_s": 0.5, "kernel_s": 0.125, "rows": 2}
EXTRA = {"connected_components": {"components": 7}, "label_size_filter": {"components": 4},
         "reconstruction": {"rounds": 3}}
TAIL = "   -> {dt} {shape} in 1.00s (rw:0.25/0.50 p:0.125)"


REAL = {fn: getattr(S, fn) for fn in STORE_FUNCTIONS}


def call_of(fn, *a, **k):
    """(function, the arguments it sees): `a` and `k` bound to the store function's signature,
    its defaults filled in, so that two calls are equal when the function cannot tell them
    apart."""
    bound = inspect.signature(REAL[fn]).bind(*a, **k)
    bound.apply_defaults()
    return fn, dict(bound.arguments)


@pytest.fixture
def recorded(monkeypatch, tmp_path):
    """Every store function a step can reach replaced by a recorder that creates the output
    array and returns canned stats; the list of the calls (call_of), with the temporary
    directory written as {tmp} and the per-element filter objects as (class, own attributes)."""
    calls = []
    tmp = str(tmp_path)

    def norm(v):
        if isinstance(v, str):
            return v.replace(tmp, "{tmp}")
        if isinstance(v, (list, tuple)):
            return type(v)(norm(x) for x in v)
        if isinstance(v, dict):
            return {k: norm(x) for k, x in v.items()}
        if hasattr(v, "output_data_type"):  # a per-element filter object
            own = {k: x for k, x in vars(v).items() if k != "chunk_limit"}  # the base class's
            return type(v).__name__, norm(own)
        return v

    def recorder(fn):
        def call(*a, **k):
            calls.append(call_of(fn, *norm(a), **norm(k)))
            src, dst = (a[0], a[2]) if fn == "arithmetic" else (a[0], a[1])
            dt = a[3][-1] if fn == "pointwise" else k.get("data_type")
            S.create_output(src, dst, dt, None, k.get("encoding"))
            return dict(CANNED, **EXTRA.get(fn, {}))
        return call

    for fn in STORE_FUNCTIONS:
        monkeypatch.setattr(S, fn, recorder(fn))
    store_all = S.store_empty_chunks()
    yield calls
    S.set_store_empty_chunks(store_all)


def _arrays(tmp_path):
    S.create_array(tmp_path / "in", "float32", (4, 4), (2, 2))
    S.create_array(tmp_path / "lab", "uint16", (4, 4), (2, 2))


def _log(lines, tmp_path):
    assert lines[-1].startswith("Completed in ")
    return [ln.replace(str(tmp_path), "{tmp}") for ln in lines[:-1]]


IN = "{tmp}/in (float32 [4, 4]) -> {tmp}/out"
LAB = "{tmp}/lab (uint16 [4, 4]) -> {tmp}/out"
# name -> (the step's own keys, the store function, its positional arguments, its keyword
# arguments beyond device=1, the first log line after "0: ", the output's type). The run's
# chunk_limit is 5; a step with its own says 3.
ONE_GPU = {
    "guided_filter": (
        {"epsilon": 0.5, "radius": 2, "data_type": "float64", "chunk_limit": 3},
        "guided_filter", ("{tmp}/in", "{tmp}/out", 0.5, 2),
        {"data_type": "float64", "encoding": {"data_type": "float64"}, "chunk_limit": 3},
        "guided_filter epsilon=0.5 radius=2 " + IN, "float64"),
    "downsample": (
        {"stride": "2,2", "discrete": True, "chunk_shape": "4,4"},
        "downsample", ("{tmp}/in", "{tmp}/out", [2, 2]),
        {"discrete": True, "data_type": None, "encoding": {"chunk_shape": [4, 4]},
         "chunk_limit": 5},
        "downsample stride=[2, 2] discrete=True " + IN, "float32"),
    "gaussian": (
        {"sigma": "1,1.5", "kernel_half_size": [2, 3], "chunk_limit": 3},
        "gaussian", ("{tmp}/in", "{tmp}/out", [1.0, 1.5], [2, 3]),
        {"data_type": None, "encoding": None, "chunk_limit": 3},
        "gaussian sigma=[1.0, 1.5] kernel_half_size=[2, 3] " + IN, "float32"),
    "summed_area_table": (
        {"data_type": "float64", "chunk_limit": 3},
        "summed_area_table", ("{tmp}/in", "{tmp}/out"),
        {"data_type": "float64", "encoding": {"data_type": "float64"}, "chunk_limit": 3},
        "summed_area_table " + IN, "float64"),
    "median": (
        {"kernel_half_size": [1, 0]},
        "rank_filter", ("{tmp}/in", "{tmp}/out", "median", [1, 0]),
        {"data_type": None, "encoding": None, "chunk_limit": 5},
        "median kernel_half_size=[1, 0] " + IN, "float32"),
    "minimum": (
        {"kernel_half_size": "1,1", "chunk_limit": 3},
        "rank_filter", ("{tmp}/in", "{tmp}/out", "minimum", [1, 1]),
        {"data_type": None, "encoding": None, "chunk_limit": 3},
        "minimum kernel_half_size=[1, 1] " + IN, "float32"),
    "maximum": (
        {"kernel_half_size": [0, 1], "fill_value": 2},
        "rank_filter", ("{tmp}/in", "{tmp}/out", "maximum", [0, 1]),
        {"data_type": None, "encoding": {"fill_value": 2}, "chunk_limit": 5},
        "maximum kernel_half_size=[0, 1] " + IN, "float32"),
    "reencode": (
        {"data_type": "int16"},
        "pointwise", ("{tmp}/in", "{tmp}/out", [("Reencode", {})], ["int16"]),
        {"encoding": {"data_type": "int16"}, "chunk_limit": 5},
        "reencode {} " + IN, "int16"),
    "crop": (
        {"offset": "1,0", "shape": [2, 3], "chunk_limit": 3},
        "pointwise", ("{tmp}/in", "{tmp}/out",
                      [("Crop", {"offset": (1, 0), "shape": (2, 3)})], ["float32"]),
        {"encoding": None, "chunk_limit": 3},
        "crop {'offset': '1,0', 'shape': [2, 3]} " + IN, "float32"),
    "rescale": (
        {"multiply": 2, "add": -1.0, "add_first": True},
        "pointwise", ("{tmp}/in", "{tmp}/out",
                      [("Rescale", {"multiply": 2.0, "add": -1.0, "add_first": True})],
                      ["float32"]),
        {"encoding": None, "chunk_limit": 5},
        "rescale {'multiply': 2, 'add': -1.0, 'add_first': True} " + IN, "float32"),
    "clamp": (
        {"min": -1, "max": 1.5},
        "pointwise", ("{tmp}/in", "{tmp}/out", [("Clamp", {"min": -1.0, "max": 1.5})],
                      ["float32"]),
        {"encoding": None, "chunk_limit": 5},
        "clamp {'min': -1, 'max': 1.5} " + IN, "float32"),
    "equal": (
        {"value": 3},
        "pointwise", ("{tmp}/in", "{tmp}/out", [("Equal", {"value": 3})], ["bool"]),
        {"encoding": {"fill_value": False, "data_type": "bool"}, "chunk_limit": 5},
        "equal {'value': 3} " + IN, "bool"),
    "replace_value": (
        {"value": 0, "replace": 7, "data_type": "uint8"},
        "pointwise", ("{tmp}/in", "{tmp}/out", [("ReplaceValue", {"value": 0, "replace": 7})],
                      ["uint8"]),
        {"encoding": {"data_type": "uint8"}, "chunk_limit": 5},
        "replace_value {'value': 0, 'replace': 7} " + IN, "uint8"),
    "arithmetic": (
        {"operator": "absolute-difference", "other": "{tmp}/lab", "chunk_limit": 3},
        "arithmetic", ("{tmp}/in", "{tmp}/lab", "{tmp}/out", "absolute_difference"),
        {"data_type": None, "encoding": None, "chunk_limit": 3},
        "arithmetic absolute_difference {tmp}/in (float32 [4, 4]) with {tmp}/lab -> {tmp}/out",
        "float32"),
    "connected_components": (
        {"connectivity": 2, "chunk_limit": 3},
        "connected_components", ("{tmp}/in", "{tmp}/out", 2),
        {"data_type": None, "encoding": None},
        "connected_components connectivity=2 " + IN, "float32"),
    "distance_transform": (
        {"spacing": [2, 1], "squared": True, "data_type": "uint16"},
        "distance_transform", ("{tmp}/in", "{tmp}/out", [2, 1], True),
        {"data_type": "uint16", "encoding": {"data_type": "uint16"}},
        "distance_transform spacing=[2, 1] squared=True " + IN, "uint16"),
    "label_size_filter": (
        {"input": "{tmp}/lab", "min_size": 2, "max_size": 5, "relabel": False},
        "label_size_filter", ("{tmp}/lab", "{tmp}/out", 2, 5, False),
        {"data_type": None, "encoding": None},
        "label_size_filter min_size=2 max_size=5 relabel=False " + LAB, "uint16"),
    "reconstruction": (
        {"input": "{tmp}/lab", "mode": "h_maxima", "h": 1.5, "connectivity": 2},
        "reconstruction", ("{tmp}/lab", "{tmp}/out", None, "dilation", 2, "h_maxima", 1.5),
        {"data_type": None, "encoding": None},
        "reconstruction mode=h_maxima method=dilation connectivity=2 h=1.5 " + LAB, "uint16"),
}


def _subst(v, tmp):
    if isinstance(v, str):
        return v.replace("{tmp}", tmp)
    if isinstance(v, dict):
        return {k: _subst(x, tmp) for k, x in v.items()}
    return v


@pytest.mark.parametrize("name", ON_PATH)
def test_a_step_on_one_gpu(name, recorded, tmp_path):
    own, fn, args, kwargs, first, out_dt = ONE_GPU[name]
    _arrays(tmp_path)
    step = {"filter": name, "input": str(tmp_path / "in"), "output": str(tmp_path / "out"),
            **_subst(own, str(tmp_path))}
    lines = []
    res = ZF.run([step], chunk_limit=5, device=1, stats=True, log=lines.append,
                 device_chain=False)
    assert recorded == [call_of(fn, *args, **kwargs, device=1)]
    stats = dict(CANNED, **EXTRA.get(fn, {}))
    assert res == [stats]
    extra = [f"   {v} {k}" for k, v in EXTRA.get(fn, {}).items()]
    assert _log(lines, tmp_path) == ["0: " + first] + extra + [
        TAIL.format(dt=out_dt, shape="[4, 4]"),
        json.dumps({"step": 0, "filter": name, **stats})]


def test_a_reconstruction_with_a_marker_and_two_steps_through_a_temporary(recorded, tmp_path):
    _arrays(tmp_path)
    tmp = str(tmp_path)
    lines = []
    ZF.run([{"filter": "clamp", "input": tmp + "/lab", "output": "$m", "min": 0, "max": 9},
            {"filter": "reconstruction", "input": tmp + "/lab", "output": tmp + "/out",
             "marker": "$m", "method": "erosion", "data_type": "uint16"},
            {"filter": "arithmetic", "input": tmp + "/lab", "output": tmp + "/sum",
             "operator": "add", "other": "$m"}],
           tmp=tmp, log=lines.append, device_chain=False)
    m = recorded[0][1]["output_path"]  # the temporary's directory
    assert m.startswith("{tmp}/m_")
    assert recorded[1:] == [
        call_of("reconstruction", "{tmp}/lab", "{tmp}/out", m, "erosion", 1, "marker", None,
                data_type="uint16", encoding={"data_type": "uint16"}),
        call_of("arithmetic", "{tmp}/lab", m, "{tmp}/sum", "add")]
    assert _log(lines, tmp_path) == [
        "0: clamp {'min': 0, 'max': 9} {tmp}/lab (uint16 [4, 4]) -> " + m,
        TAIL.format(dt="uint16", shape="[4, 4]"),
        "1: reconstruction mode=marker method=erosion connectivity=1 {tmp}/lab (uint16 [4, 4]) "
        f"marker {m} -> {{tmp}}/out",
        "   3 rounds",
        TAIL.format(dt="uint16", shape="[4, 4]"),
        f"2: arithmetic add {{tmp}}/lab (uint16 [4, 4]) with {m} -> {{tmp}}/sum",
        TAIL.format(dt="uint16", shape="[4, 4]")]


def test_validation_comes_before_the_store_function(recorded, tmp_path):
    _arrays(tmp_path)
    base = {"input": str(tmp_path / "in"), "output": str(tmp_path / "out")}
    for step, error, text in (
            ({"filter": "guided_filter"}, _abi.InvalidParameters, "needs epsilon and radius"),
            ({"filter": "downsample", "stride": [2]}, _abi.InvalidParameters,
             "stride must match the array rank"),
            ({"filter": "median"}, _abi.InvalidParameters, "median needs kernel_half_size"),
            ({"filter": "crop", "offset": [0, 0]}, _abi.InvalidParameters, "crop needs shape"),
            ({"filter": "arithmetic", "operator": "add"}, _abi.InvalidParameters,
             "arithmetic needs other"),
            ({"filter": "arithmetic", "operator": "add", "other": "$x"}, _abi.InvalidParameters,
             "other \\$x is not the output of an earlier step"),
            ({"filter": "reconstruction", "marker": "$x"}, _abi.InvalidParameters,
             "marker \\$x is not the output of an earlier step"),
            ({"filter": "reconstruction", "mode": "fill_holes", "data_type": "uint8"},
             _abi.UnsupportedDataType, "the input's data type float32, not uint8"),
            ({"filter": "connected_components", "connectivity": "x"}, _abi.InvalidParameters,
             "connected_components: connectivity 'x' is not an integer"),
            ({"filter": "reconstruction", "mode": "fill_holes", "connectivity": "x"},
             _abi.InvalidParameters, "reconstruction: connectivity 'x' is not an integer"),
            ({"filter": "label_size_filter", "min_size": "x"}, _abi.InvalidParameters,
             "min_size and max_size are integers"),
            ({"filter": "gradient_magnitude"}, _abi.FilterError,
             "outside the accelerated path \\(supported: " + ", ".join(ON_PATH) + "\\)")):
        with pytest.raises(error, match=text):
            ZF.run([{**step, **base}], log=lambda *a: None, device_chain=False)
    assert recorded == []


# a worker of a multi-GPU split: (name, params, rows) -> (store function, args, kwargs beyond
# the common ones)
COMMON = {"device": 2, "nthreads": 4, "erase": False, "finish": False}
WORKER = [
    ("guided_filter", {"epsilon": 0.5, "radius": 2, "data_type": "float64",
                       "encoding": {"data_type": "float64"}, "chunk_limit": 3},
     ((0, 1), (1, 2)),
     "guided_filter", ("{tmp}/in", "{tmp}/out", 0.5, 2),
     {"rows": (0, 1), "cols": (1, 2), "data_type": "float64",
      "encoding": {"data_type": "float64"}, "chunk_limit": 3}),
    ("guided_filter", {"epsilon": 0.5, "radius": 2}, (1, 2),
     "guided_filter", ("{tmp}/in", "{tmp}/out", 0.5, 2),
     {"rows": (1, 2), "cols": None, "data_type": None, "encoding": None, "chunk_limit": 0}),
    ("downsample", {"stride": [2, 2], "discrete": True, "chunk_limit": None}, (0, 1),
     "downsample", ("{tmp}/in", "{tmp}/out", [2, 2]),
     {"discrete": True, "rows": (0, 1), "data_type": None, "encoding": None, "chunk_limit": 0}),
    ("gaussian", {"sigma": [1.0, 1.5], "kernel_half_size": [2, 3], "chunk_limit": 3}, (0, 2),
     "gaussian", ("{tmp}/in", "{tmp}/out", [1.0, 1.5], [2, 3]),
     {"rows": (0, 2), "data_type": None, "encoding": None, "chunk_limit": 3}),
    ("median", {"kernel_half_size": [1, 0]}, (0, 1),
     "rank_filter", ("{tmp}/in", "{tmp}/out", "median", [1, 0]),
     {"rows": (0, 1), "data_type": None, "encoding": None, "chunk_limit": 0}),
    ("minimum", {"kernel_half_size": [1, 1]}, (0, 1),
     "rank_filter", ("{tmp}/in", "{tmp}/out", "minimum", [1, 1]),
     {"rows": (0, 1), "data_type": None, "encoding": None, "chunk_limit": 0}),
    ("maximum", {"kernel_half_size": [0, 1], "encoding": {"fill_value": 2}}, (0, 1),
     "rank_filter", ("{tmp}/in", "{tmp}/out", "maximum", [0, 1]),
     {"rows": (0, 1), "data_type": None, "encoding": {"fill_value": 2}, "chunk_limit": 0}),
    ("reencode", {"args": {}, "data_type": "int16", "encoding": {"data_type": "int16"}}, (0, 1),
     "pointwise", ("{tmp}/in", "{tmp}/out", [("Reencode", {})], ["int16"]),
     {"rows": (0, 1), "encoding": {"data_type": "int16"}, "chunk_limit": 0}),
    ("crop", {"args": {"offset": "1,0", "shape": [2, 3]}, "chunk_limit": 3}, (0, 1),
     "pointwise", ("{tmp}/in", "{tmp}/out", [("Crop", {"offset": (1, 0), "shape": (2, 3)})],
                   ["float32"]),
     {"rows": (0, 1), "encoding": None, "chunk_limit": 3}),
    ("rescale", {"args": {"multiply": 2, "add": -1.0, "add_first": True}}, (0, 1),
     "pointwise", ("{tmp}/in", "{tmp}/out",
                   [("Rescale", {"multiply": 2.0, "add": -1.0, "add_first": True})],
                   ["float32"]),
     {"rows": (0, 1), "encoding": None, "chunk_limit": 0}),
    ("clamp", {"args": {"min": -1, "max": 1.5}}, (0, 1),
     "pointwise", ("{tmp}/in", "{tmp}/out", [("Clamp", {"min": -1.0, "max": 1.5})],
                   ["float32"]),
     {"rows": (0, 1), "encoding": None, "chunk_limit": 0}),
    ("equal", {"args": {"value": 3}, "encoding": {"fill_value": False, "data_type": "bool"}},
     (0, 1),
     "pointwise", ("{tmp}/in", "{tmp}/out", [("Equal", {"value": 3})], ["bool"]),
     {"rows": (0, 1), "encoding": {"fill_value": False, "data_type": "bool"},
      "chunk_limit": 0}),
    ("replace_value", {"args": {"value": 0, "replace": 7}, "data_type": "uint8"}, (0, 1),
     "pointwise", ("{tmp}/in", "{tmp}/out", [("ReplaceValue", {"value": 0, "replace": 7})],
                   ["uint8"]),
     {"rows": (0, 1), "encoding": {"data_type": "uint8"}, "chunk_limit": 0}),
    ("arithmetic", {"operator": "absolute_difference", "other": "{tmp}/lab"}, (0, 1),
     "arithmetic", ("{tmp}/in", "{tmp}/lab", "{tmp}/out", "absolute_difference"),
     {"rows": (0, 1), "data_type": None, "encoding": None, "chunk_limit": 0}),
    ("downsample_gaussian", {"stride": [2, 2], "sigma": [1.0, 1.0], "kernel_half_size": [2, 2],
                             "data_type": "float32"}, (0, 1),
     "downsample_gaussian", ("{tmp}/in", "{tmp}/out", [2, 2], [1.0, 1.0], [2, 2]),
     {"rows": (0, 1), "data_type": "float32", "encoding": None, "chunk_limit": 0}),
]


@pytest.mark.parametrize("name, params, rows, fn, args, kwargs", WORKER,
                         ids=[f"{w[0]}-{k}" for k, w in enumerate(WORKER)])
def test_a_worker_of_a_multi_gpu_split(name, params, rows, fn, args, kwargs, recorded, tmp_path):
    _arrays(tmp_path)
    tmp = str(tmp_path)
    st = ZF._rows_worker(name, tmp + "/in", tmp + "/out", _subst(params, tmp), 2, rows, 4)
    assert recorded == [call_of(fn, *args, **COMMON, **kwargs)]
    assert st == dict(CANNED, **EXTRA.get(fn, {}))


def test_every_splittable_name_has_a_worker_case():
    assert {w[0] for w in WORKER} == {n for n in ON_PATH if ZF.rows_splittable(n)} | {
        "downsample_gaussian"}


@pytest.mark.parametrize("name", ["summed_area_table", "connected_components", "reconstruction",
                                  "gradient_magnitude", "nothing"])
def test_a_worker_has_no_step_for_the_other_names(name, recorded, tmp_path):
    with pytest.raises(_abi.FilterError, match=f"no store step for filter '{name}'") as e:
        ZF._rows_worker(name, "in", "out", {}, 0, (0, 1), 1)
    assert type(e.value) is _abi.FilterError and e.value.status == _abi.ERR_OTHER
    assert recorded == []


def test_a_worker_takes_the_parents_empty_chunk_setting(recorded, tmp_path):
    _arrays(tmp_path)
    tmp = str(tmp_path)
    for store_all in (False, True):
        ZF._rows_worker("gaussian", tmp + "/in", tmp + "/out",
                        {"sigma": [1, 1], "kernel_half_size": [1, 1],
                         "store_empty_chunks": store_all}, 0, (0, 1), 1)
        assert S.store_empty_chunks() is store_all


# what run() hands to run_rows_parallel for the step ONE_GPU[name][0] under gpus=2: the dict
# that crosses into the workers beside the common data_type, encoding and chunk_limit, and the
# output's shape
SPLIT = {
    "guided_filter": ({"epsilon": 0.5, "radius": 2, "data_type": "float64",
                       "encoding": {"data_type": "float64"}, "chunk_limit": 3}, (4, 4)),
    "downsample": ({"stride": [2, 2], "discrete": True, "data_type": None,
                    "encoding": {"chunk_shape": [4, 4]}, "chunk_limit": 5}, (2, 2)),
    "gaussian": ({"sigma": [1.0, 1.5], "kernel_half_size": [2, 3], "data_type": None,
                  "encoding": None, "chunk_limit": 3}, (4, 4)),
    "median": ({"kernel_half_size": [1, 0], "data_type": None, "encoding": None,
                "chunk_limit": 5}, (4, 4)),
    "minimum": ({"kernel_half_size": [1, 1], "data_type": None, "encoding": None,
                 "chunk_limit": 3}, (4, 4)),
    "maximum": ({"kernel_half_size": [0, 1], "data_type": None, "encoding": {"fill_value": 2},
                 "chunk_limit": 5}, (4, 4)),
    "reencode": ({"args": {}, "data_type": "int16", "encoding": {"data_type": "int16"},
                  "chunk_limit": 5}, (4, 4)),
    "crop": ({"args": {"offset": "1,0", "shape": [2, 3]}, "data_type": None, "encoding": None,
              "chunk_limit": 3}, (2, 3)),
    "rescale": ({"args": {"multiply": 2, "add": -1.0, "add_first": True}, "data_type": None,
                 "encoding": None, "chunk_limit": 5}, (4, 4)),
    "clamp": ({"args": {"min": -1, "max": 1.5}, "data_type": None, "encoding": None,
               "chunk_limit": 5}, (4, 4)),
    "equal": ({"args": {"value": 3}, "data_type": None,
               "encoding": {"fill_value": False, "data_type": "bool"}, "chunk_limit": 5}, (4, 4)),
    "replace_value": ({"args": {"value": 0, "replace": 7}, "data_type": "uint8",
                       "encoding": {"data_type": "uint8"}, "chunk_limit": 5}, (4, 4)),
    "arithmetic": ({"operator": "absolute_difference", "other": "{tmp}/lab", "data_type": None,
                    "encoding": None, "chunk_limit": 3}, (4, 4)),
}


@pytest.mark.parametrize("name", [n for n in ON_PATH if n in SPLIT])
def test_what_a_splittable_step_hands_to_the_split(name, monkeypatch, tmp_path):
    _arrays(tmp_path)
    tmp = str(tmp_path)
    got = []

    def split(name, src, dst, params, out_shape, gpus, nthreads=0, devices=None):
        got.append((name, src, dst, params, tuple(out_shape), gpus, nthreads, devices))
        S.create_output(src, dst, params.get("data_type"), out_shape, params.get("encoding"))
        return dict(CANNED)

    monkeypatch.setattr(ZF, "run_rows_parallel", split)
    step = {"filter": name, "input": tmp + "/in", "output": tmp + "/out",
            **_subst(ONE_GPU[name][0], tmp)}
    res = ZF.run([step], chunk_limit=5, gpus=2, gpu_devices=[1, 1], log=lambda *a: None)
    params, shape = SPLIT[name]
    assert got == [(name, tmp + "/in", tmp + "/out", _subst(params, tmp), shape, 2, 0, [1, 1])]
    assert res == [CANNED]


def test_every_splittable_name_has_a_split_case():
    assert set(SPLIT) == {n for n in ON_PATH if ZF.rows_splittable(n)}


def test_row_dependent_steps_under_two_gpus_run_in_one_process(recorded, tmp_path):
    _arrays(tmp_path)
    tmp = str(tmp_path)
    lines = []
    ZF.run([{"filter": "summed_area_table", "input": tmp + "/in", "output": tmp + "/sat",
             "chunk_limit": 3},
            {"filter": "connected_components", "input": tmp + "/in", "output": tmp + "/cc",
             "connectivity": 2, "data_type": "uint8"}],
           gpus=2, gpu_devices=[3, 3], log=lines.append)
    assert recorded == [
        call_of("summed_area_table", "{tmp}/in", "{tmp}/sat", device=3, chunk_limit=3),
        call_of("connected_components", "{tmp}/in", "{tmp}/cc", 2, data_type="uint8", device=3,
                encoding={"data_type": "uint8"})]
    assert _log(lines, tmp_path) == [
        "0: summed_area_table {tmp}/in (float32 [4, 4]) -> {tmp}/sat",
        "   summed_area_table: chunk rows depend on each other in order; one process on device "
        "3, not 2",
        TAIL.format(dt="float32", shape="[4, 4]"),
        "1: connected_components connectivity=2 {tmp}/in (float32 [4, 4]) -> {tmp}/cc",
        "   connected_components: chunk rows depend on each other in order; one process on "
        "device 3, not 2",
        "   7 components",
        TAIL.format(dt="uint8", shape="[4, 4]")]


def test_step_params_and_step_encoding_of_every_name(tmp_path):
    _arrays(tmp_path)
    info, lab = S.open_array(tmp_path / "in"), S.open_array(tmp_path / "lab")
    classes = {"guided_filter": "GuidedFilter", "downsample": "Downsample",
               "gaussian": "Gaussian", "summed_area_table": "SummedAreaTable",
               "median": "RankFilter", "minimum": "RankFilter", "maximum": "RankFilter",
               "reencode": "Reencode", "crop": "Crop", "rescale": "Rescale", "clamp": "Clamp",
               "equal": "Equal", "replace_value": "ReplaceValue", "arithmetic": "Arithmetic",
               "connected_components": "ConnectedComponents",
               "distance_transform": "DistanceTransform", "label_size_filter": "SizeFilterStep",
               "reconstruction": "Reconstruction"}
    shapes = {"downsample": (2, 2), "crop": (2, 3)}
    # the output type and encoding when the step names no type: the filter's own rule
    own_rule = {"equal": ("bool", {"fill_value": False, "data_type": "bool"}),
                "connected_components": ("uint32", {"data_type": "uint32", "fill_value": 0}),
                "distance_transform": ("uint32", {"data_type": "uint32", "fill_value": 0}),
                "label_size_filter": ("uint16", {"data_type": "uint16", "fill_value": 0})}
    for name in ON_PATH:
        own = {k: v for k, v in ONE_GPU[name][0].items()
               if k not in ("input", "data_type", "chunk_shape", "fill_value")}
        step = {"filter": name, **own}
        src = lab if name in ("label_size_filter", "reconstruction") else info
        f, shape, dt = ZF._step_params(step, src)
        assert type(f).__name__ == classes[name]
        assert shape == shapes.get(name, (4, 4)) and isinstance(shape, tuple)
        assert (dt, ZF.step_encoding(step, src.data_type)) == own_rule.get(
            name, (src.data_type, None))
        # an explicit type, as the step's data_type and as its encoding's, wins
        given = "uint16" if name == "reconstruction" else "uint8"
        enc = {"data_type": given, "fill_value": 1}
        assert ZF._step_params({**step, **enc}, src)[2] == given
        assert ZF.step_encoding({**step, **enc}, src.data_type) == enc


# ---------------------------------------------------------------------------------------------
# the helpers that the whole-array steps share

def test_the_output_rules_of_the_whole_array_filters(tmp_path):
    S.create_array(tmp_path / "in", "int16", (4, 4), (2, 2), fill_value=-1)
    rules = {"connected_components": (S.connected_components_output, (), "uint32"),
             "distance_transform": (S.distance_transform_output, (False,), "float32"),
             "distance_transform squared": (S.distance_transform_output, (True,), "uint32"),
             "label_size_filter": (S.label_size_filter_output, ("int16",), "int16")}
    for fn, first, default in rules.values():
        assert fn(*first) == (default, {"data_type": default, "fill_value": 0})
        assert fn(*first, "uint8") == ("uint8", {"data_type": "uint8", "fill_value": 0})
        assert fn(*first, "uint8", {"data_type": "int64", "chunk_shape": [2, 2]}) == (
            "int64", {"data_type": "int64", "chunk_shape": [2, 2], "fill_value": 0})
        assert fn(*first, None, {"fill_value": 9}) == (
            default, {"fill_value": 9, "data_type": default})
        assert fn(*first, None, '{"fill_value": 9}') == (
            default, {"fill_value": 9, "data_type": default})
        given = {"fill_value": 9}
        fn(*first, "uint8", given)
        assert given == {"fill_value": 9}  # the caller's dict is left alone
    src = tmp_path / "in"
    assert S.reconstruction_output(src) == ("int16", {"data_type": "int16"})
    assert S.reconstruction_output(src, "int16", {"fill_value": 9}) == (
        "int16", {"fill_value": 9, "data_type": "int16"})
    assert S.reconstruction_output(src, None, '{"data_type": "int16"}') == (
        "int16", {"data_type": "int16"})
    for args in (("uint8",), (None, {"data_type": "float32"}), ("int16", {"data_type": "int8"})):
        with pytest.raises(_abi.UnsupportedDataType,
                           match="reconstruction: the output has the input's data type int16, "
                                 "not ") as e:
            S.reconstruction_output(src, *args)
        assert e.value.status == _abi.ERR_UNSUPPORTED_DATA_TYPE


@pytest.fixture
def nothing_is_read(monkeypatch):
    def no_read(*a, **k):
        raise AssertionError("an array was read")

    monkeypatch.setattr(device_io, "read_to_device", no_read)
    monkeypatch.delenv("ZT_STORE_DEVICE_MEMORY", raising=False)
    monkeypatch.delenv("ZT_STORE_HOST_MEMORY", raising=False)
    return monkeypatch


CC_NO_FALLBACK = ("connected_components labels the whole array in device memory (a component "
                  "may span every chunk): there is no store -> store path to fall back to")
OOM_STATUS = f" (status {_abi.ERR_OUT_OF_MEMORY})"
RECON_NO_FALLBACK = ("reconstruction works on the whole array in device memory (the result at "
                     "an element may depend on every chunk): there is no store -> store path to "
                     "fall back to")


def test_the_out_of_memory_message_of_the_device(nothing_is_read, tmp_path):
    S.create_array(tmp_path / "in", "uint8", (4, 4), (2, 2))
    from zarrs_tools_amd import filter as F
    need = F.ConnectedComponents(2).memory("uint8", "uint32", (4, 4))  # the kernels' own figure
    assert need > 80
    nothing_is_read.setattr(S, "device_available_bytes", lambda device=0: 109)
    nothing_is_read.setattr(S, "host_available_bytes", lambda: 1 << 40)
    with pytest.raises(_abi.FilterError) as e:
        S.connected_components(tmp_path / "in", tmp_path / "out", 2)
    assert e.value.status == _abi.ERR_OUT_OF_MEMORY
    assert str(e.value) == (
        f"There is not enough available memory to process the array: it needs {need} bytes of "
        "device memory (input, labels and two index arrays) and 80 % of the available memory is "
        "80; " + CC_NO_FALLBACK + OOM_STATUS)
    assert not (tmp_path / "out").exists()


def test_the_out_of_memory_message_of_the_host(nothing_is_read, tmp_path):
    # (6, 4) uint16 in (4, 2) chunks: the read's pieces are whole chunk rows, the largest 4 x 4
    # elements, two of them in flight: 2 * 16 * 2 = 64 bytes; the write's rows are smaller
    S.create_array(tmp_path / "in", "uint16", (6, 4), (4, 2))
    nothing_is_read.setattr(S, "device_available_bytes", lambda device=0: 1 << 40)
    nothing_is_read.setattr(S, "host_available_bytes", lambda: 79)
    with pytest.raises(_abi.FilterError) as e:
        S.connected_components(tmp_path / "in", tmp_path / "out", 1, data_type="uint8")
    assert e.value.status == _abi.ERR_OUT_OF_MEMORY
    assert str(e.value) == (
        "There is not enough available memory to process the array: its pinned host buffers "
        "need 64 bytes and 80 % of the available memory is 56; " + CC_NO_FALLBACK + OOM_STATUS)
    assert not (tmp_path / "out" / "zarr.json").exists()
    # a reconstruction's marker is read in pieces too: of its own chunk grid
    S.create_array(tmp_path / "marker", "uint16", (6, 4), (3, 4))
    nothing_is_read.setattr(S, "host_available_bytes", lambda: 59)
    with pytest.raises(_abi.FilterError) as e:
        S.reconstruction(tmp_path / "in", tmp_path / "out", tmp_path / "marker")
    assert e.value.status == _abi.ERR_OUT_OF_MEMORY
    assert str(e.value) == (
        "There is not enough available memory to process the array: its pinned host buffers "
        "need 48 bytes and 80 % of the available memory is 40; " + RECON_NO_FALLBACK + OOM_STATUS)
    assert not (tmp_path / "out" / "zarr.json").exists()
