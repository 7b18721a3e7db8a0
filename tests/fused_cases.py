"""The case table of the fused 3-D guided filter's launch modes, shared by the CPU plan test
(tests/test_gf_plan.py) and the GPU parity test (tests/test_guided_fused_modes_gpu.py).

launch_fused_cfg (zarrs_tools_amd/csrc/gf_fused.hpp) follows plan_fused (gf_plan.hpp): a
quad-aligned geometry runs one mode-1 grid, anything else mode 0 on the interior tiles plus mode 2
on the border tiles. Every case here states the modes it must launch and how many interior tiles
it must have; the plan test checks that claim against the real plan code on the CPU, so a GPU
case cannot silently move to another mode when shapes or the plan change.

A case describes a call of the host API (`kind`); `launches()` lists the fused launches that call
makes, in elements, as the C ABI derives them (zt_api.hip: apply_array, apply_ndarray, apply_slab;
filter.py: apply_chunk). Base offsets are relative to a device allocation, which the GPU test
asserts is 16-byte aligned.
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass, field
from typing import NamedTuple, Optional

ESIZE = {"float32": 4, "uint16": 2, "uint8": 1}
TX = 64  # kFusedTileX


def tile_y(r: int) -> int:
    """The radius -> tile height rule as the issue states it; the plan test compares it with
    fused_tile_y (gf_plan.hpp)."""
    return 32 if r <= 4 else 16


class Launch(NamedTuple):
    ny: int
    nx: int
    oy0: int
    ox0: int
    onz: int
    ony: int
    onx: int
    in_sz: int
    in_sy: int
    out_sz: int
    out_sy: int
    in_off: int   # elements from the input allocation's start
    out_off: int  # elements from the output allocation's start
    r: int
    din: str
    dout: str
    chunk_depth: int


@dataclass(frozen=True)
class Case:
    id: str
    group: str            # A .. G of the coverage list
    kind: str             # "array" | "ndarray" | "chunked" | "slab"
    shape: tuple          # the array (kind ndarray: the view handed to apply_ndarray)
    chunk: tuple
    r: int
    eps: float
    modes: frozenset      # the kernel modes every launch of the case must run, exactly
    min_interior: int     # interior (mode 0) tiles every launch must have at least
    din: str = "float32"
    dout: str = "float32"
    top: float = 300.0    # inputs are uniform in [0, top]
    # kind ndarray: the view is parent[:, 1:1+ny, xoff:xoff+nx] of a contiguous parent tensor
    parent: Optional[tuple] = None
    xoff: int = 0
    subset: Optional[tuple] = None  # (start, shape) of the output box in the view
    ranks: int = 0                  # kind slab
    tile0_interior: bool = False    # some launch must have tile (0, 0) interior
    walk: bool = False              # every launch grid must take all three super-tile branches
    nwg_mod8_zero: Optional[bool] = None  # every launch grid's size is (not) a multiple of 8
    seed: int = field(default=0, compare=False)

    def launches(self) -> list:
        nd = len(self.shape)
        dom = (1,) * (3 - nd) + tuple(self.shape)
        if self.kind == "array":
            sz = dom[1] * dom[2] if nd == 3 else 0
            depth = self.chunk[0] if nd == 3 else 1
            return [Launch(dom[1], dom[2], 0, 0, dom[0], dom[1], dom[2], sz, dom[2], sz, dom[2],
                           0, 0, self.r, self.din, self.dout, depth)]
        if self.kind == "ndarray":
            pz, py, px = self.parent
            (z0, y0, x0), (onz, ony, onx) = self.subset
            return [Launch(dom[1], dom[2], y0, x0, onz, ony, onx, py * px, px, ony * onx, onx,
                           px + self.xoff, 0, self.r, self.din, self.dout, 0)]
        if self.kind == "chunked":
            out = []
            grid = [-(-n // c) for n, c in zip(self.shape, self.chunk)]
            for idx in itertools.product(*[range(g) for g in grid]):
                s = [i * c for i, c in zip(idx, self.chunk)]
                n = [min(a + c, m) - a for a, c, m in zip(s, self.chunk, self.shape)]
                i0 = [max(a - 2 * self.r, 0) for a in s]
                i1 = [min(a + b + 2 * self.r, m) for a, b, m in zip(s, n, self.shape)]
                sy, sz = self.shape[2], self.shape[1] * self.shape[2]
                out.append(Launch(i1[1] - i0[1], i1[2] - i0[2], s[1] - i0[1], s[2] - i0[2],
                                  n[0], n[1], n[2], sz, sy, n[1] * n[2], n[2],
                                  i0[0] * sz + i0[1] * sy + i0[2], 0, self.r, self.din, self.dout,
                                  0))
            return out
        if self.kind == "slab":
            sz = dom[1] * dom[2]
            out = []
            for z0, nz in self.slab_rows():
                out.append(Launch(dom[1], dom[2], 0, 0, nz, dom[1], dom[2], sz, dom[2], sz, dom[2],
                                  0, 0, self.r, self.din, self.dout, self.chunk[0]))
            return out
        raise ValueError(self.kind)

    def slab_rows(self) -> list:
        """(out_z0, out_nz) per rank: the contiguous split of chunk rows (shard.slab_assignment)."""
        rows = -(-self.shape[0] // self.chunk[0])
        out = []
        for k in range(self.ranks):
            c0, c1 = k * rows // self.ranks, (k + 1) * rows // self.ranks
            z0 = min(c0 * self.chunk[0], self.shape[0])
            z1 = min(c1 * self.chunk[0], self.shape[0])
            out.append((z0, z1 - z0))
        return out


M02 = frozenset({0, 2})
M1 = frozenset({1})


def shape_a(r: int) -> tuple:
    """The smallest whole-array shape with interior tiles: 4 x 3 or 4 x 4 tiles, the x tiles
    [1, 3) and the y tile 1 interior; nx is odd, so even radii are not quad-aligned either."""
    w = 2 * r + 1
    return (2 * w + 5, 2 * tile_y(r) + 2 * r + 5, 195 + 2 * r)


def chunk_a(r: int) -> tuple:
    """Chunk depth W + 1 over nz = 2W + 5: three z-segments, the last 3 planes deep."""
    s = shape_a(r)
    return (2 * r + 2, s[1], s[2])


def _cases() -> list:
    cs = []
    # A: every radius, f32 -> f32, both eps
    for r in range(1, 9):
        for eps in (0.5, 2500.0):
            cs.append(Case(f"A-r{r}-eps{eps:g}", "A", "array", shape_a(r), chunk_a(r), r, eps, M02,
                           2, seed=10 + r))
    # B: element types in modes 0 + 2. Integer inputs full range into float outputs (eps 0.5,
    # where a 1-ulp error of the stage-1 mean shows); into integer outputs the inputs are scaled
    # so that every result stays below the output type's maximum (the pre-launch fill).
    full = {"float32": 300.0, "uint16": 65535.0, "uint8": 255.0}
    room = {"float32": None, "uint16": 30000.0, "uint8": 120.0}
    short = {"float32": "f32", "uint16": "u16", "uint8": "u8"}
    for r in (1, 2, 4, 5, 8):
        for din in ("float32", "uint16", "uint8"):
            for dout in ("float32", "uint16", "uint8"):
                top = full[din] if room[dout] is None else min(full[din], room[dout])
                eps = 0.5 if dout == "float32" else 2500.0
                cs.append(Case(f"B-r{r}-{short[din]}-{short[dout]}", "B", "array", shape_a(r),
                               chunk_a(r), r, eps, M02, 2, din=din, dout=dout, top=top,
                               seed=30 + r))
    # C: in-place views through apply_ndarray: base pointer moved by 1 row + 1..3 elements, row
    # stride 1 mod 4, output box starting at an odd x
    for r in (1, 4):
        nzv, ony, onx = 20, 70, 140
        view = (nzv, 3 + ony + 2 * r + 1, 2 * r + 1 + onx + 2 * r + 2)
        parent = (nzv, view[1] + 2, view[2] + 6)
        sub = ((1, 3, 2 * r + 1), (nzv - 2, ony, onx))
        for din in ("uint8", "uint16", "float32"):
            for xoff in (1, 2, 3):
                cs.append(Case(f"C-r{r}-{short[din]}-x{xoff}", "C", "ndarray", view, view, r, 0.5,
                               M02, 2, din=din, top=full[din], parent=parent, xoff=xoff,
                               subset=sub, seed=50 + r))
    # D: halo'd per-chunk blocks: ox0 = oy0 = 2R in the inner chunks, tile 0 itself interior
    for r in (1, 3):
        cs.append(Case(f"D-r{r}", "D", "chunked", (20, 150, 300), (10, 75, 150), r, 0.5, M02, 1,
                       tile0_interior=True, seed=60 + r))
    # E: slab form over case A's r = 3 shape, 48 planes deep, 3 ranks
    sa = shape_a(3)
    cs.append(Case("E-slab-r3", "E", "slab", (48, sa[1], sa[2]), (16, 32, 64), 3, 2500.0, M02, 2,
                   ranks=3, seed=70))
    # F: a 2-D image (nz = 1 through mode 0)
    cs.append(Case("F-2d-r3", "F", "array", (90, 210), (32, 64), 3, 0.5, M02, 2, seed=80))
    # G: the super-tile walk, all three branches in every launch grid, with and without the
    # nwg % 8 == 0 remap (chunk depth 3: four z-segments; 12: one)
    for depth, mod8 in ((3, True), (12, False)):
        cs.append(Case(f"G-m02-d{depth}", "G", "array", (12, 620, 419), (depth, 620, 419), 1, 0.5,
                       M02, 90, walk=True, nwg_mod8_zero=mod8, seed=90))
        cs.append(Case(f"G-m1-d{depth}", "G", "array", (12, 584, 324), (depth, 584, 324), 2, 0.5,
                       M1, 0, walk=True, nwg_mod8_zero=mod8, seed=91))
    return cs


CASES = _cases()


def group(g: str) -> list:
    return [c for c in CASES if c.group == g]
