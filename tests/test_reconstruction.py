"""CPU half of morphological reconstruction: the numpy restatement
tests/recon_ref.py against hand-written answers and, where scipy is installed, against
scipy.ndimage.binary_propagation and binary_fill_holes (greyscale by threshold decomposition); and
everything of the feature that needs no GPU: the command and run-config grammar, the chain planner,
the option conflicts, the limits on h, connectivity and rank, the type table, the memory formula
and the exported symbols."""
import numpy as np
import pytest

from tests import recon_ref as R
from tests.rank_ref import from_key, to_key

import zarrs_tools_amd as zt
from zarrs_tools_amd import _abi
from zarrs_tools_amd import zarrs_filter as ZF

ALL = list(_abi.DTYPES)
SIZE = {"bool": 1, "int8": 1, "uint8": 1, "int16": 2, "uint16": 2, "bfloat16": 2, "float16": 2,
        "int32": 4, "uint32": 4, "float32": 4, "int64": 8, "uint64": 8, "float64": 8}

RING = np.array([[0, 0, 0, 0, 0, 0],
                 [0, 1, 1, 1, 0, 0],   # the corner (1, 4) is missing: the hole's element (2, 3)
                 [0, 1, 0, 0, 1, 0],   # touches it by a diagonal only
                 [0, 1, 0, 0, 1, 0],
                 [0, 1, 1, 1, 1, 0],
                 [0, 0, 0, 0, 0, 0]], dtype=np.uint8)


# ---- the checker itself ------------------------------------------------------------------------

def test_ramp_under_a_plateau():
    mask = np.array([0, 5, 5, 5, 5, 0, 5, 5], dtype=np.uint8)
    marker = np.array([0, 1, 2, 3, 0, 0, 0, 0], dtype=np.uint8)
    out, sweeps = R.reconstruct(mask, marker, "uint8", "dilation", 1, with_sweeps=True)
    # the ramp's top floods the plateau it stands on, and nothing crosses the gap at index 5
    assert out.tolist() == [0, 3, 3, 3, 3, 0, 0, 0]
    assert sweeps == 3  # index 1 is two steps from the top; the third sweep changes nothing
    # nothing wraps: the last element of a row and the first of the next are no neighbours
    mask2 = np.full((2, 3), 9, dtype=np.uint8)
    mask2[:, 1] = 0
    marker2 = np.zeros((2, 3), dtype=np.uint8)
    marker2[0, 2] = 7
    assert R.reconstruct(mask2, marker2, "uint8").tolist() == [[0, 0, 7], [0, 0, 7]]
    # connectivity limits and a zero extent
    for c in (0, 3):
        with pytest.raises(ValueError):
            R.reconstruct(mask2, marker2, "uint8", "dilation", c)
    empty = np.zeros((3, 0, 4), dtype=np.uint8)
    assert R.reconstruct(empty, empty, "uint8", "erosion", 2).shape == (3, 0, 4)


def test_ring_fills_by_faces_and_leaks_through_the_diagonal():
    filled = RING.copy()
    filled[2:4, 2:4] = 1
    assert np.array_equal(R.apply(RING, "uint8", "fill_holes", connectivity=1), filled)
    assert np.array_equal(R.apply(RING, "uint8", "fill_holes", connectivity=2), RING)
    assert np.array_equal(R.apply(RING, "bool", "fill_holes", connectivity=1), filled)
    # the marker: the mask on the border, the type's greatest key elsewhere
    m = R.fill_holes_marker(RING, "uint8")
    assert m[0].tolist() == [0] * 6 and m[1].tolist() == [0, 255, 255, 255, 255, 0]
    assert R.fill_holes_marker(np.zeros((3, 3), np.int8), "int8")[1, 1] == 127
    # an axis of extent 1 or 2 makes every element border: nothing is filled
    thin = np.array([[1, 0, 1]], dtype=np.uint8)
    assert np.array_equal(R.apply(thin, "uint8", "fill_holes"), thin)


def test_h_maxima_and_minima_of_known_height():
    mask = np.array([1, 2, 1, 4, 1, 1, 7, 1], dtype=np.uint8)
    # the peak of height 1 goes, the peaks of height 3 and 6 lose h = 2; 1 - 2 saturates at 0
    assert R.h_marker(mask, "uint8", 2.0, -1).tolist() == [0, 0, 0, 2, 0, 0, 5, 0]
    assert R.apply(mask, "uint8", "h_maxima", h=2.0).tolist() == [1, 1, 1, 2, 1, 1, 5, 1]
    inv = (10 - mask.astype(np.int8)).astype(np.int8)
    assert R.apply(inv, "int8", "h_minima", h=2.0).tolist() == [9, 9, 9, 8, 9, 9, 5, 9]
    # saturation at the type's limits: 250 + 10 is 255, and the result is the mask again
    high = np.array([250, 255, 250], dtype=np.uint8)
    assert R.h_marker(high, "uint8", 10.0, +1).tolist() == [255, 255, 255]
    low = np.array([-128, -120, -128], dtype=np.int8)
    assert R.h_marker(low, "int8", 10.0, -1).tolist() == [-128, -128, -128]
    assert R.apply(low, "int8", "h_maxima", h=10.0).tolist() == [-128, -128, -128]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            R.h_marker(mask, "uint8", bad, -1)
    with pytest.raises(ValueError):
        R.h_marker(mask, "bool", 1.0, -1)


def test_a_marker_above_the_mask_is_clipped():
    mask = np.array([3, 3, 0, 3], dtype=np.uint8)
    marker = np.array([9, 0, 9, 0], dtype=np.uint8)
    assert R.reconstruct(mask, marker, "uint8").tolist() == [3, 3, 0, 0]
    # by erosion a marker below the mask is raised to it
    assert R.reconstruct(mask, np.zeros(4, np.uint8), "uint8", "erosion").tolist() == [3, 3, 0, 3]


@pytest.mark.parametrize("dt,np_type,top", [("uint8", np.uint8, 255), ("int8", np.int8, -1),
                                            ("uint16", np.uint16, 65535)])
def test_erosion_is_the_dilation_of_the_complement(dt, np_type, top):
    rng = np.random.default_rng(5)
    info = np.iinfo(np_type)
    for shape in ((23,), (6, 11), (3, 5, 7)):
        mask = rng.integers(info.min, info.max, shape, endpoint=True).astype(np_type)
        marker = rng.integers(info.min, info.max, shape, endpoint=True).astype(np_type)
        for c in range(1, len(shape) + 1):
            # top - x reverses the order of the type without leaving it
            want = (top - R.reconstruct((top - mask).astype(np_type),
                                        (top - marker).astype(np_type), dt, "dilation", c))
            got = R.reconstruct(mask, marker, dt, "erosion", c)
            assert np.array_equal(got, want.astype(np_type))


def test_float_order_on_zeros_infinities_and_nans():
    neg_nan, pos_nan = 0xFFC00001, 0x7FC00001  # payloads pass through
    order = np.array([neg_nan, 0xFF800000, 0xBF800000, 0x80000001, 0x80000000, 0x00000000,
                      0x00000001, 0x3F800000, 0x7F800000, pos_nan], dtype=np.uint32)
    assert np.all(np.diff(to_key(order.view(np.float32), "float32").astype(np.int64)) > 0)
    mask = order.view(np.float32)
    # a seed of the greatest key at the right end: every element rises to its own mask value
    marker = np.full(order.shape, neg_nan, dtype=np.uint32)
    marker[-1] = pos_nan
    out = R.reconstruct(mask, marker.view(np.float32), "float32")
    assert out.view(np.uint32).tolist() == order.tolist()
    # from the left end nothing rises: the first mask value is the least and caps the flow
    marker = np.full(order.shape, neg_nan, dtype=np.uint32)
    marker[0] = pos_nan
    out = R.reconstruct(mask, marker.view(np.float32), "float32")
    assert out.view(np.uint32).tolist() == [neg_nan] * len(order)
    # -0.0 < +0.0: the marker's -0.0 rises to +0.0 under a mask of +0.0, and not the reverse
    z = np.array([0x80000000, 0x00000000], dtype=np.uint32).view(np.float32)
    pz = np.zeros(2, dtype=np.float32)
    assert R.reconstruct(pz, z, "float32").view(np.uint32).tolist() == [0, 0]
    nz = np.array([0x80000000, 0x80000000], dtype=np.uint32).view(np.float32)
    assert R.reconstruct(nz, z, "float32").view(np.uint32).tolist() == [0x80000000] * 2
    # the 16-bit floats are storage bits
    h = np.array([0xFE00, 0xFC00, 0x8000, 0x0000, 0x7C00, 0x7E00], dtype=np.uint16)
    seed = np.full(6, 0xFE00, dtype=np.uint16)
    seed[-1] = 0x7E00
    assert R.reconstruct(h, seed, "float16").tolist() == h.tolist()
    assert np.array_equal(from_key(to_key(h, "bfloat16"), "bfloat16"), h)


SCIPY_SHAPES = [(37,), (9, 70), (5, 33, 67)]


@pytest.mark.parametrize("shape", SCIPY_SHAPES)
def test_restatement_agrees_with_scipy_on_masks(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(len(shape))
    for c in range(1, len(shape) + 1):
        structure = ndi.generate_binary_structure(len(shape), c)
        for density in (0.3, 0.6, 0.9):
            mask = rng.random(shape) < density
            marker = mask & (rng.random(shape) < 0.03)
            want = ndi.binary_propagation(marker, structure=structure, mask=mask)
            got = R.reconstruct(mask.astype(np.uint8), marker.astype(np.uint8), "bool",
                                "dilation", c)
            assert np.array_equal(got.astype(bool), want)
            want = ndi.binary_fill_holes(mask, structure=structure)
            got = R.apply(mask.astype(np.uint8), "bool", "fill_holes", connectivity=c)
            assert np.array_equal(got.astype(bool), want)


@pytest.mark.parametrize("shape", SCIPY_SHAPES)
def test_greyscale_by_threshold_decomposition(shape):
    """out >= t is the binary reconstruction of marker >= t under mask >= t, for every level t."""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(10 + len(shape))
    mask = rng.integers(0, 6, shape).astype(np.uint8)
    marker = np.where(rng.random(shape) < 0.03, mask, 0).astype(np.uint8)
    for c in range(1, len(shape) + 1):
        structure = ndi.generate_binary_structure(len(shape), c)
        out, sweeps = R.reconstruct(mask, marker, "uint8", "dilation", c, with_sweeps=True)
        assert 1 <= sweeps <= mask.size + 1
        for t in range(1, 6):
            want = ndi.binary_propagation(marker >= t, structure=structure, mask=mask >= t)
            assert np.array_equal(out >= t, want), (c, t)


# ---- the feature ---------------------------------------------------------------------------------

def test_subcommand_grammar_and_option_conflicts():
    p = ZF.build_parser()
    a = p.parse_args(["reconstruction", "in", "out", "--fill-holes"])
    assert ZF._steps_from_cli(a) == [{"filter": "reconstruction", "input": "in", "output": "out",
                                      "mode": "fill_holes", "connectivity": 1, "data_type": None,
                                      "chunk_limit": None}]
    a = p.parse_args(["reconstruction", "in", "out", "--marker", "seeds", "--method", "erosion",
                      "--connectivity", "3", "-c", "16,16,16", "--skip-empty-chunks"])
    step = ZF._steps_from_cli(a)[0]
    assert step["marker"] == "seeds" and step["method"] == "erosion" and step["mode"] == "marker"
    assert step["connectivity"] == 3 and step["chunk_shape"] == [16, 16, 16]
    assert a.filter_skip_empty_chunks
    step = ZF._steps_from_cli(p.parse_args(["reconstruction", "in", "out", "--marker", "m"]))[0]
    assert step["method"] == "dilation"
    step = ZF._steps_from_cli(p.parse_args(["reconstruction", "in", "out", "--h-maxima", "2.5"]))[0]
    assert step["mode"] == "h_maxima" and step["h"] == 2.5 and "marker" not in step
    step = ZF._steps_from_cli(p.parse_args(["reconstruction", "in", "out", "--h-minima", "3"]))[0]
    assert step["mode"] == "h_minima" and step["h"] == 3.0
    # exactly one of the four
    for argv in (["reconstruction", "in", "out"],
                 ["reconstruction", "in", "out", "--fill-holes", "--marker", "m"],
                 ["reconstruction", "in", "out", "--h-maxima", "1", "--h-minima", "1"],
                 ["reconstruction", "in", "--fill-holes"],
                 ["reconstruction", "in", "out", "--fill-holes", "--method", "opening"],
                 ["reconstruction", "in", "out", "--fill-holes", "--connectivity", "faces"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    # --method is only valid with --marker
    for how in (["--fill-holes"], ["--h-maxima", "1"], ["--h-minima", "1"]):
        a = p.parse_args(["reconstruction", "in", "out", "--method", "erosion"] + how)
        with pytest.raises(zt.InvalidParameters, match="only valid with --marker"):
            ZF._steps_from_cli(a)
    assert ZF.main(["reconstruction", "in", "out", "--fill-holes", "--method", "dilation"]) == 1


def test_on_path_whole_array_and_rows():
    assert "reconstruction" in ZF.ON_PATH and "reconstruction" in ZF.WHOLE_ARRAY
    assert ZF.BINARY == ("arithmetic",)
    assert ZF.rows_splittable("reconstruction") is False
    assert ZF.rows_splittable("gaussian") is True


def test_run_config_step():
    f, marker = ZF.reconstruction_of({"filter": "reconstruction", "marker": "$seeds"})
    assert isinstance(f, zt.Reconstruction) and marker == "$seeds"
    assert (f.mode, f.method, f.connectivity) == ("marker", "dilation", 1)
    f, marker = ZF.reconstruction_of({"filter": "reconstruction", "marker": "m", "mode": "marker",
                                      "method": "erosion", "connectivity": "2"})
    assert (f.mode, f.method, f.connectivity, marker) == ("marker", "erosion", 2, "m")
    f, marker = ZF.reconstruction_of({"filter": "reconstruction", "mode": "fill_holes"})
    assert (f.mode, f.method, marker) == ("fill_holes", "erosion", None)
    f, _ = ZF.reconstruction_of({"filter": "reconstruction", "mode": "h_maxima", "h": 2})
    assert (f.mode, f.method, f.h) == ("h_maxima", "dilation", 2.0)
    f, _ = ZF.reconstruction_of({"filter": "reconstruction", "mode": "h-minima", "h": "0.5"})
    assert (f.mode, f.method, f.h) == ("h_minima", "erosion", 0.5)
    bad = [({}, "needs a marker or a mode"),
           ({"mode": "marker"}, "mode marker needs a marker"),
           ({"mode": "fill_holes", "marker": "m"}, "no marker is given"),
           ({"mode": "fill_holes", "method": "erosion"}, "only valid with a marker"),
           ({"mode": "opening"}, "unknown mode"),
           ({"marker": "m", "method": "opening"}, "unknown method"),
           ({"mode": "h_maxima"}, "needs a number h"),
           ({"mode": "h_maxima", "h": 0}, "finite number > 0"),
           ({"mode": "h_minima", "h": -1}, "finite number > 0"),
           ({"mode": "h_minima", "h": "NaN"}, "finite number > 0"),
           ({"mode": "h_maxima", "h": float("inf")}, "finite number > 0"),
           ({"mode": "fill_holes", "h": 1}, "only given with h_maxima or h_minima"),
           ({"marker": "m", "h": 1}, "only given with h_maxima or h_minima"),
           ({"mode": "fill_holes", "connectivity": "faces"}, "not an integer"),
           ({"mode": "fill_holes", "connectivity": 0}, "connectivity 0")]
    for extra, message in bad:
        with pytest.raises(zt.InvalidParameters, match=message):
            ZF.reconstruction_of({"filter": "reconstruction", **extra})


def test_chain_planning_with_markers():
    # the generated-marker modes sit in a device-resident chain
    steps = [{"filter": "equal", "input": "in", "value": 0},
             {"filter": "reconstruction", "mode": "fill_holes"},
             {"filter": "connected_components"},
             {"filter": "label_size_filter", "min_size": 4, "output": "out"}]
    assert ZF.plan_chains(steps) == [(0, 3)]
    # a temporary that a step names as its marker is written to the store, and a step with a
    # marker array is never part of a chain
    steps = [{"filter": "clamp", "input": "in", "min": 0, "max": 9, "output": "$seeds"},
             {"filter": "reconstruction", "input": "in", "marker": "$seeds", "output": "$rec"},
             {"filter": "equal", "input": "$rec", "value": 0, "output": "out"}]
    assert ZF.plan_chains(steps) == []
    steps = [{"filter": "equal", "input": "in", "value": 0, "output": "$mask"},
             {"filter": "reconstruction", "input": "$mask", "mode": "fill_holes",
              "output": "$filled"},
             {"filter": "reconstruction", "input": "in", "marker": "$filled", "output": "out"}]
    assert ZF.plan_chains(steps) == [(0, 1)]
    # the marker also counts as a reader of the temporary: $mask has two, so no chain
    steps = [{"filter": "equal", "input": "in", "value": 0, "output": "$mask"},
             {"filter": "reconstruction", "input": "$mask", "mode": "fill_holes",
              "output": "$filled"},
             {"filter": "reconstruction", "input": "$filled", "marker": "$mask", "output": "out"}]
    assert ZF.plan_chains(steps) == []
    # a $name marker must be written by an earlier step
    with pytest.raises(zt.InvalidParameters, match="not the output of an earlier step"):
        ZF.run([{"filter": "reconstruction", "input": "in", "marker": "$nowhere",
                 "output": "out"}], log=lambda *_: None)


def test_step_params_and_output_encoding():
    from zarrs_tools_amd import store as S
    info = S.ArrayInfo("in", "int16", (20, 30, 40), (8, 8, 8), (8, 8, 8))
    f, shape, dt = ZF._step_params({"filter": "reconstruction", "mode": "h_maxima", "h": 3,
                                    "connectivity": 3}, info)
    assert isinstance(f, zt.Reconstruction) and (f.mode, f.connectivity) == ("h_maxima", 3)
    assert shape == (20, 30, 40) and dt == "int16"
    for c in (0, 4, -1):
        with pytest.raises(zt.InvalidParameters, match="connectivity"):
            ZF._step_params({"filter": "reconstruction", "mode": "fill_holes",
                             "connectivity": c}, info)
    with pytest.raises(zt.UnsupportedDataType, match="the input's data type int16"):
        ZF._step_params({"filter": "reconstruction", "mode": "fill_holes",
                         "data_type": "uint8"}, info)
    boolean = S.ArrayInfo("in", "bool", (20, 30), (8, 8), (8, 8))
    ZF._step_params({"filter": "reconstruction", "mode": "fill_holes"}, boolean)
    with pytest.raises(zt.UnsupportedDataType, match="not bool"):
        ZF._step_params({"filter": "reconstruction", "mode": "h_minima", "h": 1}, boolean)
    # the output keeps the input's type and fill value: nothing is added to the encoding
    assert ZF.step_encoding({"filter": "reconstruction", "mode": "fill_holes"}, "int16") is None


def test_type_table():
    f = zt.Reconstruction()
    assert f.name() == "reconstruction" and (f.method, f.mode, f.connectivity) == (
        "dilation", "marker", 1)
    for dt in ALL:
        f.is_compatible(dt)
        f.is_compatible(dt, dt)
        zt.Reconstruction(mode="fill_holes").is_compatible(dt)
        for other in ALL:
            if other != dt:
                with pytest.raises(zt.UnsupportedDataType, match="one data type"):
                    f.is_compatible(dt, other)
        for mode in ("h_maxima", "h_minima"):
            g = zt.Reconstruction(mode=mode, h=1.5)
            if dt == "bool":
                with pytest.raises(zt.UnsupportedDataType, match="not bool"):
                    g.is_compatible(dt)
            else:
                g.is_compatible(dt)
    with pytest.raises(zt.UnsupportedDataType):
        f.is_compatible("complex64")
    # the generated modes fix the method
    assert zt.Reconstruction(mode="fill_holes").method == "erosion"
    assert zt.Reconstruction(mode="h_maxima", h=1).method == "dilation"
    assert zt.Reconstruction(mode="h_minima", h=1).method == "erosion"
    with pytest.raises(zt.InvalidParameters, match="h_maxima is by dilation"):
        zt.Reconstruction("erosion", 1, "h_maxima", 1.0)


def test_connectivity_and_rank_limits():
    with pytest.raises(zt.InvalidParameters, match=r"connectivity 0 not in \[1, rank\]"):
        zt.Reconstruction(connectivity=0)
    for shape in ((3,), (3, 3), (3, 3, 3), (1, 1, 3, 3, 3)):
        rank = len(shape)
        zt.Reconstruction(connectivity=rank).memory("uint8", "uint8", shape)
        with pytest.raises(zt.InvalidParameters,
                           match=rf"connectivity {rank + 1} not in \[1, {rank}\]"):
            zt.Reconstruction(connectivity=rank + 1).memory("uint8", "uint8", shape)
        with pytest.raises(zt.InvalidParameters):
            zt.Reconstruction(connectivity=rank + 1).check_connectivity(rank)
    # ranks above 3: only with unit axes in front of the innermost three
    f = zt.Reconstruction(mode="fill_holes")
    for shape in ((2, 3, 3, 3), (1, 2, 3, 3, 3), (2, 1, 3, 3, 3)):
        with pytest.raises(zt.InvalidParameters, match="in front of the innermost three"):
            f.memory("uint8", "uint8", shape)
    f.memory("uint8", "uint8", (1, 1, 1, 1, 1, 3, 3, 3))
    assert f.memory("uint8", "uint8", (2, 0, 3, 3, 3)) == 0  # a zero extent is a no-op


def test_memory_formula():
    """input(s) + scratch + output; the scratch is one working array of the element type, rounded
    up to 16 bytes, and 64 bytes of flag words."""
    cases = [("uint8", (70, 45, 67)), ("float64", (9, 70)), ("bool", (1001,)),
             ("uint16", (1, 4, 9, 17)), ("uint8", (1024, 1024, 1024)),
             ("int64", (2048, 2048, 2048)), ("bfloat16", (3, 5, 7))]
    for dt, shape in cases:
        n = int(np.prod([int(s) for s in shape], dtype=object))
        scratch = (n * SIZE[dt] + 15) // 16 * 16 + 64
        if dt != "bool":
            for mode in ("h_maxima", "h_minima"):
                got = zt.Reconstruction(mode=mode, h=1).memory(dt, dt, shape)
                assert got == 2 * n * SIZE[dt] + scratch
        assert zt.Reconstruction(mode="fill_holes").memory(dt, dt, shape) == \
            2 * n * SIZE[dt] + scratch, (dt, shape)
        assert zt.Reconstruction().memory(dt, dt, shape) == 3 * n * SIZE[dt] + scratch, (dt, shape)
    assert zt.Reconstruction().memory("uint8", "uint8", (5, 0, 7)) == 0
    with pytest.raises(zt.UnsupportedDataType):
        zt.Reconstruction().memory("uint8", "uint16", (5, 7))


def test_symbols_tile_and_export():
    syms = _abi.header_symbols()
    for name in ("zt_reconstruction_is_compatible", "zt_reconstruction_memory",
                 "zt_reconstruction_apply_array"):
        assert name in syms
        assert hasattr(_abi.lib(), name)
    text = open(_abi.HEADER_PATH).read()
    for axis, extent in zip("ZYX", _abi.REC_TILE):
        assert f"#define ZT_REC_TILE_{axis} {extent}\n" in text
    assert f"#define ZT_REC_BATCH {_abi.REC_BATCH}\n" in text
    assert "Reconstruction" in zt.__all__
    assert _abi.lib().zt_abi_version() == 4
    assert _abi.REC_MODES == {"marker": 0, "fill_holes": 1, "h_maxima": 2, "h_minima": 3}
    assert _abi.REC_METHODS == {"dilation": 0, "erosion": 1}
