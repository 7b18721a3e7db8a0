"""Inputs and the case table of the guided filter's value-range tests, shared by the CPU check of
the inputs (tests/test_guided_values.py) and the GPU parity test (tests/test_guided_values_gpu.py).
Needs numpy and the oracle only.

Every GPU test of the guided filter before these fed values in [0, 300) (or +-200) with
eps in {0.5 ... 2500}. The groups here move the values to where the five arithmetic paths
 can go wrong:

  A  the [0, 300) data times 2^k, eps times 4^k: (v - u)^2 + eps up to 2^126 and beyond (the
     reciprocal of a = s / (s + eps) is subnormal there) and down into the subnormals
  B  a normalised image, values in [0, 2^-10)
  C  eps = 0, and a constant region with a tiny eps (s = 0 exactly)
  D  full-range 32- and 64-bit integers and wide float64 values through the input conversions
  E  results that saturate, overflow or truncate in each of the 13 output types
  F  one NaN, +inf or -inf in otherwise tame data

Each builder returns fresh arrays; `cached` variants are read-only and computed once.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from oracle import oracle as O
from tests import fused_cases as FC
from tests.gpu_util import type_extremes, value_scale


@dataclass(frozen=True)
class Path:
    id: str
    shape: tuple
    chunk: tuple
    r: int
    din: str = "float32"  # the type the f32 values are handed over in


def _fc(case_id: str) -> FC.Case:
    (c,) = [c for c in FC.CASES if c.id == case_id]
    return c


def _from_fc(pid: str, case_id: str) -> Path:
    """A row of the fused case table (tests/test_gf_plan.py pins its launch modes)."""
    c = _fc(case_id)
    assert c.kind == "array" and c.din == "float32"
    return Path(pid, tuple(c.shape), tuple(c.chunk), c.r)


M2, M2C = (11, 37, 91), (5, 13, 30)  # fused 3-D, edge tiles only (mode 2)

PATHS = {p.id: p for p in [
    Path("m2-r1", M2, M2C, 1), Path("m2-r2", M2, M2C, 2), Path("m2-r3", M2, M2C, 3),
    Path("m2-r4", M2, M2C, 4), Path("m2-r8", M2, M2C, 8),
    _from_fc("m02-r2", "A-r2-eps0.5"),     # interior tiles: modes 0 + 2
    _from_fc("m02-r4", "A-r4-eps0.5"),
    _from_fc("m1-r2", "G-m1-d3"),          # quad-aligned: one mode-1 grid
    Path("stage-f64", M2, M2C, 2, "float64"),  # launch_cast_to_f32_3d staging, then the march
    Path("sep-r9", (12, 25, 40), (6, 8, 16), 9),
    Path("sep-5d", (3, 4, 5, 6, 18), (2, 2, 4, 4, 8), 1),
    Path("tm-r1", (10, 24, 20, 72), (5, 8, 10, 24), 1),
    Path("tm-r2", (10, 24, 20, 72), (5, 8, 10, 24), 2),
    Path("tab-r3", (32, 6, 7, 20), (8, 3, 7, 10), 3),
    Path("g4f-quad", (3, 20, 21, 136), (3, 8, 8, 64), 2),
    Path("g4f-r1", (2, 45, 26, 71), (1, 16, 13, 40), 1),
]}

A_PATHS = list(PATHS)
A_KS = (-64, -60, -20, 0, 40, 56)
A_EPS0 = (0.5, 50.0)
A_EQUIVARIANT_KS = (-60, -20, 40)     # gpu(v0 * 2^k) / 2^k against gpu(v0)
B_PATHS = ("m2-r2", "m2-r4", "tm-r2", "g4f-quad", "sep-r9")
B_EPS = (2.0 ** -20 * 0.5, 2.0 ** -20 * 50.0)
C_PATHS = ("m2-r2", "m2-r4", "tm-r2")
D_PATHS = ("m2-r2", "g4f-quad", "sep-r9")
D_TYPES = ("int32", "uint32", "int64", "uint64", "float64")
E_PATH = "m2-r2"
E_SCALES = (40, 0)
F_PATHS = ("m2-r2", "m2-r4", "tm-r2", "sep-r9")


def _seed(path: Path, salt: int) -> int:
    return 1000 * salt + sum(path.shape) + path.r


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def oracle(v32: np.ndarray, path: Path, eps: float) -> np.ndarray:
    return O.guided_filter_apply(v32, path.chunk, float(eps), path.r, nthreads=8)


def box_mean(v: np.ndarray, r: int) -> np.ndarray:
    """The f32 mean over the clamped (2r + 1)^d window, by exact f64 prefix sums: the u of
    guided_filter.rs:127 up to the rounding of its summed-area table."""
    s = v.astype(np.float64)
    cnt = np.ones((), np.float64)
    for ax in range(v.ndim):
        n = v.shape[ax]
        i = np.arange(n)
        lo, hi = np.maximum(i - r, 0), np.minimum(i + r, n - 1) + 1
        c = np.concatenate([np.zeros_like(np.take(s, [0], ax)), np.cumsum(s, ax)], ax)
        s = np.take(c, hi, ax) - np.take(c, lo, ax)
        shp = [1] * v.ndim
        shp[ax] = n
        cnt = cnt * (hi - lo).reshape(shp)
    return (s / cnt).astype(np.float32)


def variance_term(v32: np.ndarray, r: int) -> np.ndarray:
    """s = (v - u)^2 in f32, as guided_filter.rs:130-132."""
    with np.errstate(over="ignore"):
        d = v32 - box_mean(v32, r)
        return d * d


# ---- A: power-of-two scale sweep ----

@functools.lru_cache(maxsize=None)
def a_base(pid: str) -> np.ndarray:
    p = PATHS[pid]
    rng = np.random.default_rng(_seed(p, 1))
    return _ro((rng.random(p.shape, dtype=np.float32) * np.float32(300)).astype(np.float32))


def a_input(pid: str, k: int, eps0: float):
    """(v0 * 2^k, f32(eps0) * 2^k * 2^k), both in f32 (a power-of-two factor is exact unless the
    product is subnormal)."""
    f = np.float32(2.0 ** k)
    return a_base(pid) * f, np.float32(np.float32(eps0) * f * f)


# ---- B: a normalised image ----

@functools.lru_cache(maxsize=None)
def b_input(pid: str) -> np.ndarray:
    p = PATHS[pid]
    rng = np.random.default_rng(_seed(p, 2))
    return _ro((rng.random(p.shape, dtype=np.float32) * np.float32(2.0 ** -10)).astype(np.float32))


# ---- C: eps = 0; a constant region with a tiny eps ----

C_CONST_EPS = 1e-30
C_CONST_ROWS = 20


@functools.lru_cache(maxsize=None)
def c_random(pid: str) -> np.ndarray:
    """[0, 300) data in which no element equals its window mean, so s > 0 and a = 1 at eps = 0."""
    p = PATHS[pid]
    for salt in range(3, 40):
        rng = np.random.default_rng(_seed(p, salt))
        v = (rng.random(p.shape, dtype=np.float32) * np.float32(300)).astype(np.float32)
        if np.all(variance_term(v, p.r) > 0):
            return _ro(v)
    raise AssertionError("no seed without an element equal to its mean")


@functools.lru_cache(maxsize=None)
def c_constant(pid: str) -> np.ndarray:
    """The first 20 indices of axis 1 hold 7.0: s is exactly 0 where the window is inside."""
    p = PATHS[pid]
    v = np.array(a_base(pid))
    v[:, :C_CONST_ROWS] = np.float32(7.0)
    return _ro(v)


# ---- D: wide input types ----

def d_float64(shape, seed: int) -> np.ndarray:
    """Half normal draws times 10^U(-6 .. 6), half 1e18 * U(-1, 1); planted: 2^24 + 1 + 2^-28
    (the last f64 bit above the f32 tie 2^24 + 1; 2^-30 does not fit in an f64 there), which one
    rounding takes to 2^24 + 2 and a rounding through any shorter intermediate to 2^24, and
    1e-50, which becomes 0. No value overflows f32: inf - inf would be NaN."""
    rng = np.random.default_rng(seed)
    small = rng.standard_normal(shape) * 10.0 ** rng.uniform(-6, 6, shape)
    big = 1e18 * rng.uniform(-1, 1, shape)
    v = np.where(rng.random(shape) < 0.5, small, big)
    flat = v.reshape(-1)
    flat[5] = 2.0 ** 24 + 1 + 2.0 ** -28
    flat[7] = 1e-50
    return v


# 64-bit integers just above an f32 tie by less than half an f64 ulp: one rounding takes them up
# (to 2^62 + 2^39, 2^63 + 2^40), a rounding through f64 first loses the 1, lands on the tie and
# goes to even (2^62, 2^63). Full-range random draws hold such a value once in 2^29.
D_DOUBLE_ROUNDING = {"int64": (2 ** 62 + 2 ** 38 + 1, -(2 ** 62 + 2 ** 38 + 1)),
                     "uint64": (2 ** 63 + 2 ** 39 + 1,)}


@functools.lru_cache(maxsize=None)
def d_input(pid: str, din: str):
    """(stored values, their f32 images, eps). Behind type_extremes' four planted values sit
    the double-rounding witnesses. eps is 50 in the units in which the data spans [256, 512):
    the middle of the suite's smoothing strengths on its [0, 300) data."""
    p = PATHS[pid]
    seed = _seed(p, 5)
    v = d_float64(p.shape, seed) if din == "float64" else type_extremes(p.shape, din, seed)
    for i, w in enumerate(D_DOUBLE_ROUNDING.get(din, ())):
        v.reshape(-1)[4 + i] = w
    v32 = O.cast_to_f32(v, din).reshape(p.shape)
    s = np.float32(value_scale(v32))
    return _ro(v, v32) + (float(np.float32(50) * s * s),)


# ---- E: output casts at range ----

@functools.lru_cache(maxsize=None)
def e_input(k: int):
    p = PATHS[E_PATH]
    rng = np.random.default_rng(_seed(p, 6) + k)
    f = np.float32(2.0 ** k)
    v = ((rng.random(p.shape, dtype=np.float32) - np.float32(0.5)) * np.float32(600) * f)
    return _ro(v.astype(np.float32)), float(np.float32(50) * f * f)


# ---- F: one non-finite element ----
#
# What the filter promises for one NaN / +inf / -inf: every output within
# Chebyshev distance 2r of it is NaN (a is inf / inf or NaN wherever the u window holds it), and
# every output at least F_BOUND away from it along one of the last two axes is bitwise what the
# same array with 0 in its place gives. Between the two, and anywhere along the leading axes,
# nothing: stage 1 keeps add-entering / subtract-leaving sums, which a non-finite value never
# leaves again. F_BOUND per path, from the code:
#   fused 3-D: a workgroup's 64-wide (and at most 32-high) tile reads its 2r apron and nothing
#     else, and every running x / y sum stays inside it: 64 + 2r;
#   t-march: stage 1 works on 16 x 16 tiles with an r apron (kMX, kMY) and writes TAB on its
#     tile, box3_final on 64 x 16 tiles (kTX) with an r apron: (16 + r) + (64 + r);
#   separable, r > 8: a running sum of kSepSeg = 32 outputs carries the value from r before it
#     to the end of the segment, r + kSepSeg - 1 past it, in each of the two stages.
F_VALUES = {"nan": np.float32("nan"), "pinf": np.float32("inf"), "ninf": np.float32("-inf")}
F_TILE_X, F_TM_TILE, F_SEP_SEG = 64, 16, 32
F_BOUND = {"m2-r2": F_TILE_X + 2 * 2, "m2-r4": F_TILE_X + 2 * 4,
           "tm-r2": (F_TM_TILE + 2) + (F_TILE_X + 2), "sep-r9": 2 * (9 + F_SEP_SEG - 1)}
# the paths' shapes with the last axis long enough that over half of the array is F_BOUND away
F_SHAPE = {"m2-r2": (11, 37, 195), "m2-r4": (11, 37, 203), "tm-r2": (10, 24, 20, 235),
           "sep-r9": (12, 25, 227)}


def f_position(shape) -> tuple:
    """Inside the first quarter of every axis."""
    return tuple(n // 8 for n in shape)


def f_inputs(pid: str, kind: str):
    """(the array with the element, the same array with 0 there, the position)."""
    shape = F_SHAPE[pid]
    rng = np.random.default_rng(_seed(PATHS[pid], 7))
    clean = (rng.random(shape, dtype=np.float32) * np.float32(300)).astype(np.float32)
    pos = f_position(shape)
    clean[pos] = 0
    bad = clean.copy()
    bad[pos] = F_VALUES[kind]
    return bad, clean, pos


def f_masks(pid: str):
    """(near, far): within Chebyshev distance 2r of the element on every axis; at least F_BOUND
    from it along one of the last two axes."""
    shape, r, b = F_SHAPE[pid], PATHS[pid].r, F_BOUND[pid]
    pos = f_position(shape)
    d = [np.abs(np.arange(n) - q).reshape([-1 if i == ax else 1 for i in range(len(shape))])
         for ax, (n, q) in enumerate(zip(shape, pos))]
    near = np.ones(shape, bool)
    for a in d:
        near = near & (a <= 2 * r)
    far = np.broadcast_to((d[-1] >= b) | (d[-2] >= b), shape)
    return near, far
