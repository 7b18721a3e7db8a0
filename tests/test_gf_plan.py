"""CPU: the fused guided filter's launch decision (zarrs_tools_amd/csrc/gf_plan.hpp: plan_fused
and its parts), compiled with g++ alone (the header has no HIP dependency).

The first test is what keeps tests/test_guided_fused_modes_gpu.py on the kernel modes it is meant
to cover: every case of tests/fused_cases.py must plan exactly the modes it claims, with at least
the interior tiles it claims (mode 0 lost all coverage once, silently, when the one-grid mode 1
arrived). The others check interior_tiles against brute force, each condition of the quad-aligned
predicate, and choose_zseg's invariants and the values the code comments state."""
import os
import re
import shutil
import subprocess

import pytest

from tests import fused_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zarrs_tools_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "gf_plan.hpp"
int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "plan") || !std::strcmp(cmd, "quad")) {
            long long v[11], in, out; int R, ei, eo, depth;
            for (auto& x : v) if (std::scanf("%lld", &x) != 1) return 2;
            if (std::scanf("%d %d %d %lld %lld %d", &R, &ei, &eo, &in, &out, &depth) != 6) return 2;
            const zt::FusedGeom g{(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5],
                                  (int)v[6], v[7], v[8], v[9], v[10]};
            if (cmd[0] == 'q') {
                std::printf("%d\n", zt::fused_quad_ok(g, R, ei, eo, (uintptr_t)in, (uintptr_t)out));
                continue;
            }
            const zt::FusedPlan p = zt::plan_fused(g, R, ei, eo, (uintptr_t)in, (uintptr_t)out, depth);
            std::printf("%d %d %d %d %d %d %d %d %d\n", (int)p.mode1, p.tiles_x, p.tiles_y, p.itx0,
                        p.itx1, p.ity0, p.ity1, p.zseg, p.nseg);
        } else if (!std::strcmp(cmd, "int")) {
            long long o0, oe, n; int T, R, nt, lo, hi;
            if (std::scanf("%lld %lld %lld %d %d %d", &o0, &oe, &n, &T, &R, &nt) != 6) return 2;
            zt::interior_tiles(o0, oe, n, T, R, 0, nt, lo, hi);
            std::printf("%d %d\n", lo, hi);
        } else if (!std::strcmp(cmd, "zseg")) {
            int onz, tiles, R, depth;
            if (std::scanf("%d %d %d %d", &onz, &tiles, &R, &depth) != 4) return 2;
            std::printf("%d\n", zt::choose_zseg(onz, tiles, R, depth));
        } else if (!std::strcmp(cmd, "ty")) {
            int R;
            if (std::scanf("%d", &R) != 1) return 2;
            std::printf("%d %d\n", zt::kFusedTileX, zt::fused_tile_y(R));
        } else {
            return 3;
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("gfplan")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o",
                    str(exe)], check=True)

    def run(lines):
        """One answer (a list of ints) per request line."""
        out = subprocess.run([str(exe)], input="".join(l + "\n" for l in lines),
                             capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [[int(t) for t in o.split()] for o in out]
    return run


def geom_line(cmd, L: FC.Launch, in_addr=None, out_addr=None):
    ei, eo = FC.ESIZE[L.din], FC.ESIZE[L.dout]
    in_addr = L.in_off * ei if in_addr is None else in_addr
    out_addr = L.out_off * eo if out_addr is None else out_addr
    return (f"{cmd} {L.ny} {L.nx} {L.oy0} {L.ox0} {L.onz} {L.ony} {L.onx} {L.in_sz} {L.in_sy} "
            f"{L.out_sz} {L.out_sy} {L.r} {ei} {eo} {in_addr} {out_addr} {L.chunk_depth}")


def super_tile():
    """GF_STX x GF_STY of the block -> tile walk, from the kernel header."""
    src = open(os.path.join(CSRC, "gf_fused.hpp")).read()
    return tuple(int(re.search(rf"#define {n} (\d+)", src).group(1)) for n in ("GF_STX", "GF_STY"))


def walk_branches(gtx, gty, stx, sty):
    """Which of the walk's three branches (gf3d_fused_kernel: full super-tiles, the x remainder
    of a full super-tile row, the y remainder rows) a gtx x gty tile grid reaches."""
    full_x, full_y = gtx // stx * stx, gty // sty * sty
    return {"super": full_y > 0 and full_x > 0, "x_rem": full_y > 0 and gtx > full_x,
            "y_rem": gty > full_y}


def test_case_table_takes_its_stated_modes(plan_lib):
    launches = [(c, L) for c in FC.CASES for L in c.launches()]
    plans = plan_lib([geom_line("plan", L) for _, L in launches])
    stx, sty = super_tile()
    tile0 = {}
    for (c, L), (mode1, tx, ty, x0, x1, y0, y1, zseg, nseg) in zip(launches, plans):
        n_int = (x1 - x0) * (y1 - y0)
        grids = {}  # mode -> (gtx, gty)
        if mode1:
            grids[1] = (tx, ty)
        else:
            if n_int > 0:
                grids[0] = (x1 - x0, y1 - y0)
            if tx * ty > n_int:
                grids[2] = (tx, ty)
        assert set(grids) == set(c.modes), (c.id, L, grids)
        assert n_int >= c.min_interior, (c.id, L, n_int)
        tile0[c.id] = tile0.get(c.id, False) or (n_int > 0 and x0 == 0 and y0 == 0)
        for mode, (gtx, gty) in grids.items():
            if c.walk:
                assert all(walk_branches(gtx, gty, stx, sty).values()), (c.id, mode, gtx, gty)
            if c.nwg_mod8_zero is not None:
                assert (gtx * gty * nseg % 8 == 0) == c.nwg_mod8_zero, (c.id, mode, gtx * gty, nseg)
    for c in FC.CASES:
        if c.tile0_interior:
            assert tile0[c.id], c.id


def test_case_table_is_the_coverage_it_claims(plan_lib):
    """The table itself: every group present, every radius in A, the stated geometry of A (interior
    x tiles [1, 3), y tile 1, >= 3 z-segments with a short last one) and of G (5 x 18 interior
    tiles, 6 x 19 tiles), both nwg parities in G, the tile rule the shapes were built on."""
    assert {c.group for c in FC.CASES} == set("ABCDEFG")
    assert len({c.id for c in FC.CASES}) == len(FC.CASES)
    for r, (tx, ty) in zip(range(9), plan_lib([f"ty {r}" for r in range(9)])):
        assert (tx, ty) == (FC.TX, FC.tile_y(r))
    a = FC.group("A")
    assert {(c.r, c.eps) for c in a} == {(r, e) for r in range(1, 9) for e in (0.5, 2500.0)}
    for c, (mode1, tx, ty, x0, x1, y0, y1, zseg, nseg) in zip(
            a, plan_lib([geom_line("plan", c.launches()[0]) for c in a])):
        assert (tx, x0, x1, y0, y1) == (4, 1, 3, 1, 2) and ty in (3, 4), c.id
        assert nseg >= 3 and 0 < c.shape[0] - (nseg - 1) * zseg < zseg, c.id
    b = FC.group("B")
    assert {(c.r, c.din, c.dout) for c in b} == {
        (r, i, o) for r in (1, 2, 4, 5, 8) for i in FC.ESIZE for o in FC.ESIZE}
    g = {c.id: plan_lib([geom_line("plan", c.launches()[0])])[0] for c in FC.group("G")}
    assert g["G-m02-d3"][3:7] == [1, 6, 1, 19] and g["G-m1-d3"][:3] == [1, 6, 19]
    assert {c.nwg_mod8_zero for c in FC.group("G") if 0 in c.modes} == {True, False}
    assert {c.nwg_mod8_zero for c in FC.group("G")} == {True, False}


def test_interior_tiles_against_brute_force(plan_lib):
    reqs, want = [], []
    for T in (16, 32, 64):
        for R in range(9):
            for n in range(1, 4 * T + 41):
                for o0, onx in ((0, n), (2 * R, n - 4 * R), (1, n - 2), (2 * R + 3, n - 2 * R - 3),
                                (T, n - T - 1), (5, T)):
                    if o0 < 0 or onx <= 0 or o0 + onx > n:
                        continue
                    nt = -(-onx // T)
                    reqs.append(f"int {o0} {o0 + onx} {n} {T} {R} {nt}")
                    want.append([t for t in range(nt) if o0 + t * T - 2 * R >= 0 and
                                 o0 + t * T + T + 2 * R <= n and o0 + t * T + T <= o0 + onx])
    got = plan_lib(reqs)
    some = 0
    for q, (lo, hi), w in zip(reqs, got, want):
        assert 0 <= lo <= hi, q
        assert list(range(lo, hi)) == w, (q, lo, hi, w)
        some += bool(w)
    assert 0 < some < len(reqs)  # empty and non-empty ranges both occur


def test_quad_ok_needs_each_of_its_ten_conditions(plan_lib):
    good = FC.Launch(ny=70, nx=200, oy0=3, ox0=8, onz=5, ony=40, onx=128, in_sz=70 * 208,
                     in_sy=208, out_sz=40 * 128, out_sy=128, in_off=0, out_off=0, r=2,
                     din="uint16", dout="float32", chunk_depth=4)
    broken = {
        "ox0": good._replace(ox0=6), "R": good._replace(r=3), "nx": good._replace(nx=202),
        "onx": good._replace(onx=126), "in_sy": good._replace(in_sy=210),
        "in_sz": good._replace(in_sz=70 * 208 + 2), "out_sy": good._replace(out_sy=130),
        "out_sz": good._replace(out_sz=40 * 128 + 1),
    }
    reqs = [geom_line("quad", good, 4096, 8192)]
    reqs += [geom_line("quad", b, 4096, 8192) for b in broken.values()]
    # base pointers: a quad is 8 bytes of u16 and 16 bytes of f32
    reqs += [geom_line("quad", good, 4096 + 4, 8192), geom_line("quad", good, 4096, 8192 + 8),
             geom_line("quad", good, 4096 + 8, 8192 + 16)]
    got = [g[0] for g in plan_lib(reqs)]
    assert got == [1] + [0] * (len(broken) + 2) + [1], list(zip(["good", *broken, "in", "out",
                                                                  "moved by a quad"], got))
    # the plan follows the predicate: one grid and no interior range, or the split
    p = plan_lib([geom_line("plan", good, 4096, 8192), geom_line("plan", good, 4096 + 4, 8192)])
    assert p[0][0] == 1 and p[0][3:7] == [0, 0, 0, 0] and p[1][0] == 0


def test_choose_zseg_invariants_and_stated_values(plan_lib):
    reqs = []
    for onz in (1, 2, 7, 8, 11, 48, 255, 256, 1000, 2048):
        for tiles in (1, 3, 12, 140, 511, 512, 1024, 2048, 4096):
            for r in (0, 1, 2, 3, 4, 8):
                for depth in (0, 1, 3, 16, 128, 256, 5000):
                    reqs.append((onz, tiles, r, depth))
    got = plan_lib([f"zseg {a} {b} {c} {d}" for a, b, c, d in reqs])
    for (onz, tiles, r, depth), (zseg,) in zip(reqs, got):
        nseg = -(-onz // zseg)
        assert 1 <= zseg <= max(onz, 1) and nseg * zseg >= onz, (onz, tiles, r, depth, zseg)
    # the values the comments in gf_plan.hpp state: 2048^3 r = 4, 256-deep chunks: two chunk
    # depths per march; 1024^3 r = 2: one 1024-slice segment per tile
    t2048, t1024 = (2048 // 64) * (2048 // 32), (1024 // 64) * (1024 // 32)
    assert plan_lib([f"zseg 2048 {t2048} 4 256", f"zseg 1024 {t1024} 2 256",
                     f"zseg 1024 {t1024} 2 128"]) == [[512], [1024], [512]]
