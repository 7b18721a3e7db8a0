"""GPU parity of the fused 3-D guided filter in each launch mode (gf_fused.hpp: mode 0 interior,
mode 1 quad-aligned, mode 2 masked edge) against the oracle, over the case table of
tests/fused_cases.py. tests/test_gf_plan.py (CPU) proves that every case launches the modes it
is listed under; here each case runs on the HIP path.

Criteria are the suite's own: float outputs |gpu - oracle| <= 1e-5 * max(1,
|oracle|), integer outputs through check_against. Every output buffer is filled before the launch
with a value no correct result can equal (NaN; the type's maximum for integer outputs, whose
inputs are scaled to stay below it), so a tile the block -> tile map never visits fails even
when the allocator hands back memory that holds an earlier result.
"""
import functools
import itertools

import numpy as np
import pytest

from oracle import oracle as O
from tests import fused_cases as FC
from tests.gpu_util import FLOAT_TOL, from_dev, rel_err, to_dev
from tests.test_guided_filter_gpu import check_against

pytestmark = pytest.mark.gpu

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)

FILL = {"float32": np.float32("nan"), "uint16": np.uint16(65535), "uint8": np.uint8(255)}


def make_input(shape, din, top, seed):
    rng = np.random.default_rng(seed)
    if din == "float32":
        return (rng.random(shape, dtype=np.float32) * np.float32(top)).astype(np.float32)
    return rng.integers(0, int(top) + 1, size=shape).astype(din)


@functools.lru_cache(maxsize=None)
def case_data(shape, din, top, seed, chunk, eps, r):
    """(input, oracle result), computed once per distinct input / filter and left unchanged."""
    v = make_input(shape, din, top, seed)
    ref = O.guided_filter_apply(O.cast_to_f32(v, din), chunk, eps, r, nthreads=8)
    v.setflags(write=False)
    ref.setflags(write=False)
    return v, ref


def data_of(c: FC.Case):
    return case_data(c.shape, c.din, c.top, c.seed, c.chunk, c.eps, c.r)


def filled(shape, dout):
    """A device tensor of the fill value, at the start of its own allocation."""
    t = to_dev(np.full(shape, FILL[dout]), dout)
    assert t.data_ptr() % 16 == 0
    return t


def report_and_check(c: FC.Case, out, ref):
    """Print the case's figures, then assert: nothing unwritten, the suite's tolerance."""
    if c.dout == "float32":
        unwritten = int(np.isnan(out).sum())
        cmp = np.asarray(ref, dtype=np.float32)
    else:
        assert float(ref.max()) < float(FILL[c.dout]) - 1, "inputs must keep results below the fill"
        unwritten = int((out == FILL[c.dout]).sum())
        cmp = O.cast_from_f32(ref, c.dout)
    err = rel_err(np.nan_to_num(out, nan=3e38) if c.dout == "float32" else out, cmp)
    print(f"{c.id}: max rel err {err:.3e}, bit-exact fraction {float(np.mean(out == cmp)):.4f}, "
          f"unwritten {unwritten}")
    assert unwritten == 0, f"{unwritten} output elements never written"
    if c.dout == "float32":
        assert err <= FLOAT_TOL
    else:
        check_against(out, ref, c.dout)


def apply_array(c: FC.Case, v):
    """GuidedFilter.apply on the whole array into a pre-filled output."""
    import torch
    x = to_dev(v, c.din)
    assert x.data_ptr() % 16 == 0
    y = filled(c.shape, c.dout)
    zt.GuidedFilter(c.eps, c.r).apply(zt.DeviceArray(x, c.chunk, c.din),
                                      zt.DeviceArray(y, c.chunk, c.dout))
    torch.cuda.synchronize()
    return from_dev(y, c.dout)


def apply_ndarray_into(block, base_ptr, sub, L: FC.Launch, eps):
    """zt_guided_filter_apply_ndarray (what GuidedFilter.apply_ndarray calls) on the view `block`
    of an allocation starting at base_ptr, into a pre-filled output; asserts that the view is the
    geometry the case table (and so the plan test) describes."""
    esz = FC.ESIZE[L.din]
    assert base_ptr % 16 == 0 and block.data_ptr() - base_ptr == L.in_off * esz
    assert tuple(block.shape[1:]) == (L.ny, L.nx) and tuple(block.stride()) == (L.in_sz, L.in_sy, 1)
    assert tuple(sub.start[1:]) == (L.oy0, L.ox0) and tuple(sub.shape) == (L.onz, L.ony, L.onx)
    out = filled(sub.shape, L.dout)
    assert tuple(out.stride()) == (L.out_sz, L.out_sy, 1)
    zt._abi.check(zt._abi.lib().zt_guided_filter_apply_ndarray(
        zt.default_context().handle, zt.DTYPES[L.din], zt.filter._ptr(block),
        zt._abi.i64_array(block.shape), zt._abi.i64_array(block.stride()), 3,
        zt._abi.i64_array(sub.start), zt._abi.i64_array(sub.shape), zt.DTYPES[L.dout],
        zt.filter._ptr(out), zt._abi.i64_array(out.stride()), eps, L.r))
    return out


IDS = lambda c: c.id  # noqa: E731


@pytest.mark.parametrize("c", FC.group("A") + FC.group("B") + FC.group("F") + FC.group("G"), ids=IDS)
def test_whole_array(c):
    """A: every radius in modes 0 + 2; B: every direct element-type pair there (the integer
    stage 1 and its three Hx write forms with the wave-uniform count); F: nz = 1; G: the
    super-tile walk's three branches in modes 0, 2 and 1, with and without the XCD remap."""
    v, ref = data_of(c)
    report_and_check(c, apply_array(c, v), ref)


@pytest.mark.parametrize("c", FC.group("C"), ids=IDS)
def test_unaligned_views(c):
    """C: mode 0's unmasked quad loads (one b32 / b64 / b128 buffer load per quad) at byte
    offsets that are no multiple of the quad, with a row stride of 1 mod 4."""
    import torch
    v, ref = data_of(c)
    (L,) = c.launches()
    # the parent's elements around the view hold the type's top value: an access that strays
    # outside the view (which must read as outside the domain) shows in the result
    host = np.full(c.parent, c.top, dtype=v.dtype)
    host[:, 1:1 + c.shape[1], c.xoff:c.xoff + c.shape[2]] = v
    parent = to_dev(host, c.din)
    view = parent[:, 1:1 + c.shape[1], c.xoff:c.xoff + c.shape[2]]
    assert not view.is_contiguous()
    sub = zt.ArraySubset(*c.subset)
    out = apply_ndarray_into(view, parent.data_ptr(), sub, L, c.eps)
    torch.cuda.synchronize()
    want = ref[tuple(slice(s, s + n) for s, n in zip(sub.start, sub.shape))]
    report_and_check(c, from_dev(out, c.dout), want)


@pytest.mark.parametrize("c", FC.group("D"), ids=IDS)
def test_halo_blocks_per_chunk(c):
    """D: GuidedFilter.apply_chunk's steps (halo'd block, apply_ndarray, interior write) for
    every chunk: the inner chunks' output box starts at 2R, so tile 0 itself is interior."""
    import torch
    v, ref = data_of(c)
    x = to_dev(v, c.din)
    y = filled(c.shape, c.dout)
    a_out = zt.DeviceArray(y, c.chunk, c.dout)
    grid = a_out.chunk_grid_shape()
    for idx, L in zip(itertools.product(*[range(n) for n in grid]), c.launches()):
        so = a_out.chunk_subset_bounded(idx)
        ov = zt.ArraySubsetOverlap(c.shape, so, [2 * c.r] * 3)
        si = ov.subset_input()
        block = x[tuple(slice(s, s + n) for s, n in zip(si.start, si.shape))]
        res = apply_ndarray_into(block, x.data_ptr(), ov.subset_dst_in_src(), L, c.eps)
        y[tuple(slice(s, s + n) for s, n in zip(so.start, so.shape))] = res
    torch.cuda.synchronize()
    report_and_check(c, from_dev(y, c.dout), ref)


@pytest.mark.parametrize("c", FC.group("E"), ids=IDS)
def test_slab_form(c):
    """E: zt_guided_filter_apply_slab per rank (zlo > 0 from the second rank on) in modes 0 + 2:
    bit-equal to the whole-array launch, and both within tolerance of the oracle."""
    import torch
    v, ref = data_of(c)
    whole = apply_array(c, v)
    x = to_dev(v, c.din)
    res = np.full(c.shape, FILL[c.dout])
    rows = []
    for rank, (z0, nz) in enumerate(c.slab_rows()):
        a = zt.slab_assignment(rank, c.ranks, c.shape[0], c.chunk[0], 2 * c.r)
        assert (a.out_z0, a.out_nz) == (z0, nz)
        rows.append(a.in_z0)
        y = filled((a.out_nz,) + c.shape[1:], c.dout)
        slab = x[a.in_z0:a.in_z0 + a.in_nz].clone()
        assert slab.data_ptr() % 16 == 0
        zt._abi.check(zt._abi.lib().zt_guided_filter_apply_slab(
            zt.default_context().handle, zt.DTYPES[c.din], zt.filter._ptr(slab),
            zt.DTYPES[c.dout], zt.filter._ptr(y), zt._abi.i64_array(c.shape), a.in_z0, a.in_nz,
            a.out_z0, a.out_nz, zt._abi.i64_array(c.chunk), c.eps, c.r))
        torch.cuda.synchronize()
        res[a.out_z0:a.out_z0 + a.out_nz] = from_dev(y, c.dout)
    assert max(rows) > 0
    report_and_check(c, whole, ref)
    report_and_check(c, res, ref)
    assert np.array_equal(res, whole)
