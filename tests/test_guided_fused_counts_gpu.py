"""GPU parity of the fused guided filter's quad-aligned launch (gf_fused.hpp, mode 1) where its
window counts can go wrong: the per-lane x and y counts and in-domain masks are constants of the
march, while the z count changes only in the first and last R slices of the array, so the r = 4
kernel keeps the count, its reciprocal and the masks in registers and refreshes them only in the
unrolled blocks (18 steps) that hold a clamped z.

Shapes (all quad-aligned: nx a multiple of 4, whole contiguous arrays, even r, so fused_quad_ok
holds and the launch is one mode-1 grid):
  (24, 40, 72)   one 64 x 32 tile with its apron: every lane clamped in x, y or z
  (8, 32, 64)    nz < 2r + 1: every step has a clamped z, the refresh runs every step
  (45, 96, 128)  clamped / full / clamped z inside the unrolled blocks, z-steps no multiple of 18;
                 with chunk depth 16 also three z-segments whose marches start mid-array
  slab form      zt_guided_filter_apply_slab with in_z0 > 0 and a 2r halo: zlo / zhi (the planes
                 the slab holds) differ from the array's z range, which the counts follow
plus the integer stage 1 of the r = 4 kernel (u16 -> f32, u8 -> u8), r = 2 (mode 1, the other
radii's per-step counts) and r = 3 (odd: modes 0 + 2).

Criterion: the suite's, |gpu - oracle| <= FLOAT_TOL * max(1, |oracle|), on outputs
pre-filled with NaN so an unwritten element fails.
"""
import numpy as np
import pytest

from tests import fused_cases as FC
from tests.gpu_util import from_dev, to_dev
from tests.test_guided_fused_modes_gpu import (FILL, apply_array, data_of, filled,
                                               report_and_check)

pytestmark = pytest.mark.gpu

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)


def case(cid, shape, chunk, r, eps, modes=FC.M1, din="float32", dout="float32", top=300.0,
         kind="array", ranks=0, seed=0):
    c = FC.Case(cid, "H", kind, shape, chunk, r, eps, modes, 0, din=din, dout=dout, top=top,
                ranks=ranks, seed=seed)
    if modes == FC.M1:  # fused_quad_ok for a whole contiguous array at an aligned base
        assert r % 2 == 0 and shape[2] % 4 == 0 and (shape[1] * shape[2]) % 4 == 0
    return c


ARRAY_CASES = [
    case(f"{name}-eps{eps:g}", shape, chunk, 4, eps, seed=seed)
    for name, shape, chunk, seed in (
        ("one-tile", (24, 40, 72), (24, 40, 72), 101),
        ("short-z", (8, 32, 64), (8, 32, 64), 102),
        ("z-transitions", (45, 96, 128), (45, 96, 128), 103),
        ("z-segments", (45, 96, 128), (16, 96, 128), 103),
    )
    for eps in (0.5, 2500.0)
] + [
    # the integer stage 1 of the same kernel (u16 full range, eps 0.5: a 1-ulp error of a
    # stage-1 mean shows)
    case("z-transitions-u16", (45, 96, 128), (45, 96, 128), 4, 0.5, din="uint16", top=65535.0,
         seed=104),
    # byte input and output (inputs below the u8 fill value of the unwritten check)
    case("z-transitions-u8", (45, 96, 128), (45, 96, 128), 4, 2500.0, din="uint8", dout="uint8",
         top=120.0, seed=108),
    # the other radii: r = 2 in mode 1 (counts per step), r = 3 in modes 0 + 2
    case("r2-one-tile", (24, 40, 72), (24, 40, 72), 2, 0.5, seed=105),
    case("r3-one-tile", (24, 40, 72), (24, 40, 72), 3, 0.5, modes=FC.M02, seed=106),
]

SLAB_CASES = [
    case(f"slab-eps{eps:g}", (48, 64, 128), (16, 32, 64), 4, eps, kind="slab", ranks=3, seed=107)
    for eps in (0.5, 2500.0)
]

IDS = lambda c: c.id  # noqa: E731


@pytest.mark.parametrize("c", ARRAY_CASES, ids=IDS)
def test_whole_array(c):
    v, ref = data_of(c)
    report_and_check(c, apply_array(c, v), ref)


@pytest.mark.parametrize("c", SLAB_CASES, ids=IDS)
def test_slab_with_halo(c):
    """Each rank's slab starts at in_z0 = out_z0 - 2r > 0 from the second rank on and holds only
    its own planes: the window counts must still be the array's, and the result the whole-array
    launch's bit for bit."""
    import torch
    v, ref = data_of(c)
    whole = apply_array(c, v)
    x = to_dev(v, c.din)
    res = np.full(c.shape, FILL[c.dout])
    starts = []
    for rank, (z0, nz) in enumerate(c.slab_rows()):
        a = zt.slab_assignment(rank, c.ranks, c.shape[0], c.chunk[0], 2 * c.r)
        assert (a.out_z0, a.out_nz) == (z0, nz)
        starts.append(a.in_z0)
        y = filled((a.out_nz,) + c.shape[1:], c.dout)
        slab = x[a.in_z0:a.in_z0 + a.in_nz].clone()
        assert slab.data_ptr() % 16 == 0
        zt._abi.check(zt._abi.lib().zt_guided_filter_apply_slab(
            zt.default_context().handle, zt.DTYPES[c.din], zt.filter._ptr(slab),
            zt.DTYPES[c.dout], zt.filter._ptr(y), zt._abi.i64_array(c.shape), a.in_z0, a.in_nz,
            a.out_z0, a.out_nz, zt._abi.i64_array(c.chunk), c.eps, c.r))
        torch.cuda.synchronize()
        res[a.out_z0:a.out_z0 + a.out_nz] = from_dev(y, c.dout)
    assert max(starts) > 0 and max(starts) == c.slab_rows()[-1][0] - 2 * c.r
    report_and_check(c, whole, ref)
    report_and_check(c, res, ref)
    assert np.array_equal(res, whole)
