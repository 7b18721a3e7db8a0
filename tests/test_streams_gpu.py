"""The operators on streams other than torch's default stream ("Streams").

Every other GPU test runs on torch's default stream, the legacy null stream, where all work is
serialised: a launch, memset or copy issued on stream 0 or on the context's own stream when the
context's current stream was meant, a host readback taken before its producer finished, and a
helper that picks its stream on its own all pass there and corrupt silently anywhere else.

The delayed-producer harness (`run_delayed`) makes them fail. Per case:
  1. the call runs twice on the default stream into poisoned outputs: the bytes of the first are
     `want`, the second is timed on the host and must give the same bytes (run-to-run identical);
     then it runs once more on other data, so that neither the context's scratch nor a cached
     allocation still holds this case's intermediates;
  2. inputs x and outputs y are allocated on the default stream, all poison, beside a staging copy
     of the real input;
  3. on a fresh non-blocking stream s, in this order: a delay (a spinning kernel), x <- staging,
     y <- poison, the call as a user writes it (no ctx: default_context() follows s);
  4. after s.synchronize() the bytes of y (and what the call returned to the host) equal `want`.
A stray launch on another stream runs during the delay: it reads poison input, or its output is
overwritten by the poison copy. The delay's length is not load-bearing: an event recorded right
after it must still be pending when a call without host readback returns (else the case repeats
once with four times the delay and then fails as inconclusive, never passes). Calls that read a
count or a flag back block on s; for them the harness covers every launch up to the first
readback, and the pending-event check is skipped (`blocking=True` in the table).

A correct library can never fail this harness; only a wrong one can pass it by luck.
"""
import ctypes
import itertools
import time
from dataclasses import dataclass
from typing import Callable

import numpy as np
import pytest

from oracle import oracle as O
from tests.gpu_util import poisoned, to_dev

pytestmark = pytest.mark.gpu

import zarrs_tools_amd as zt  # noqa: E402  (no skip: the HIP library must load)
from zarrs_tools_amd import _abi  # noqa: E402

DELAY_FLOOR_MS = 20.0   # dominates launch latencies
DELAY_FACTOR = 10.0     # times the host time of the call under test


# ---- the delay ---------------------------------------------------------------------------------------

class Delay:
    """A spinning kernel on torch's current stream: torch.cuda._sleep(cycles), a single thread, or
    where this torch has none a loop of elementwise passes over a tensor large enough that a pass
    takes the device longer than its launch takes the host. Calibrated once per session by timing
    a fixed count with two events."""

    _spin = None          # units -> None, enqueues that many units
    _units_per_ms = None

    @classmethod
    def _pick(cls):
        import torch
        if hasattr(torch.cuda, "_sleep"):
            return torch.cuda._sleep, 4_000_000, "torch.cuda._sleep cycles"
        buf = torch.zeros(1 << 24, dtype=torch.float32, device="cuda")

        def passes(n):
            for _ in range(n):
                buf.add_(1.0)
        return passes, 400, "elementwise passes over a 64 MiB tensor"

    @classmethod
    def units_per_ms(cls) -> float:
        if cls._units_per_ms is None:
            import torch
            cls._spin, n, what = cls._pick()
            cls._spin(max(1, n // 40))  # loads the kernel
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cls._spin(n)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            assert ms > 0.05, f"the delay took {ms} ms for {n} {what}: cannot calibrate"
            cls._units_per_ms = n / ms
            print(f"\n[streams] delay: {n} {what} in {ms:.3f} ms = "
                  f"{cls._units_per_ms:.0f} per ms")
        return cls._units_per_ms

    @classmethod
    def enqueue(cls, ms: float) -> None:
        """The delay on torch's current stream."""
        n = max(1, int(ms * cls.units_per_ms()))
        cls._spin(n)


def delay_for(host_ms: float) -> float:
    return max(DELAY_FLOOR_MS, DELAY_FACTOR * host_ms)


# ---- bytes ------------------------------------------------------------------------------------------

def raw(t) -> bytes:
    import torch
    if t.numel() == 0:
        return b""
    return t.contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()


def canon(h):
    """What a call returned to the host, in a form that compares by value and by bits."""
    if isinstance(h, dict):
        return tuple((k, canon(h[k])) for k in sorted(h))
    if isinstance(h, (tuple, list)):
        return tuple(canon(v) for v in h)
    if isinstance(h, np.ndarray):
        if h.dtype == object:
            return ("obj", h.shape, tuple(int(v) for v in h.reshape(-1)))
        return (str(h.dtype), h.shape, np.ascontiguousarray(h).tobytes())
    if isinstance(h, float):
        return ("f", np.float64(h).tobytes())
    return h


def first_difference(got: bytes, want: bytes) -> str:
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    if a.size != b.size:
        return f"{a.size} bytes, want {b.size}"
    d = np.flatnonzero(a != b)
    return f"{d.size} of {a.size} bytes differ, first at byte {int(d[0])}"


# ---- the case table ----------------------------------------------------------------------------------

@dataclass
class Case:
    id: str
    inputs: Callable      # seed -> [(storage array, data type name), ...]
    outs: object          # [(shape, data type name), ...], or a function that returns the list
    call: Callable        # (xs, ys) -> what the call returns to the host, or None
    blocking: bool = False  # reads a count or flag back: the call waits for the stream

    @property
    def outputs(self) -> list:
        return self.outs() if callable(self.outs) else self.outs


def quiet(fn):
    """fn(xs, ys) for its effect on ys: what it returns is a device tensor, not a host value."""
    def call(xs, ys):
        fn(xs, ys)
    return call


def f32(shape, scale=300.0):
    return lambda seed: [((np.random.default_rng(seed).random(shape, dtype=np.float32)
                           * scale).astype(np.float32), "float32")]


def ints(shape, dtype, lo, hi):
    return lambda seed: [(np.random.default_rng(seed).integers(lo, hi, shape).astype(
        O.NP_STORAGE[dtype]), dtype)]


def both(*makers):
    return lambda seed: [p for k, m in enumerate(makers) for p in m(seed * 10 + k)]


def grid(shape, chunk):
    return itertools.product(*[range(-(-n // c)) for n, c in zip(shape, chunk)])


def guided(shape, chunk, r, din="float32", dout="float32", eps=0.5, src=None):
    def call(xs, ys):
        zt.GuidedFilter(eps, r).apply(zt.DeviceArray(xs[0], chunk, din),
                                      zt.DeviceArray(ys[0], chunk, dout))
    return Case(f"guided-{'x'.join(map(str, shape))}-r{r}-{din}-{dout}", src or f32(shape),
                [(shape, dout)], call)


def guided_chunk_loop(shape, chunk, r):
    def call(xs, ys):
        a, b = zt.DeviceArray(xs[0], chunk), zt.DeviceArray(ys[0], chunk)
        g = zt.GuidedFilter(0.5, r)
        for idx in grid(shape, chunk):
            g.apply_chunk(a, b, idx)
    return Case("guided-apply_chunk-loop", f32(shape), [(shape, "float32")], call)


def guided_subset(shape, sub, r):
    def call(xs, ys):
        ys[0].copy_(zt.GuidedFilter(0.5, r).apply_ndarray(xs[0], zt.ArraySubset(*sub)))
    return Case("guided-4d-tmarch-interior-subset", f32(shape), [(sub[1], "float32")], call)


def into(y, res):
    """An operator that allocates its result: copied into the harness's output on the current
    stream. A stray launch that reads is then caught through the poisoned input and the scrubbed
    scratch; a stray memset or other write-only launch on the fresh result is not, so this form is
    kept for the paths that have no form with an output argument, and for one or two allocating
    forms as a user writes them."""
    y.copy_(res)


def ndarray_case(id, maker, out, fn, blocking=False):
    def call(xs, ys):
        into(ys[0], fn(*xs))
    return Case(id, maker, [out], call, blocking)


# Where the Python surface only has the allocating form, the entry point is called as that form
# calls it, on the default context, with the harness's poisoned output: a stray memset or kernel on
# another stream is then overwritten by the poison copy, whatever it read.

def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def abi_downsample(x, y, discrete):
    dt = _abi.DTYPES[zt.dtype_of(x)]
    _abi.check(_abi.lib().zt_downsample_apply_ndarray(
        zt.default_context().handle, dt, _p(x), _abi.i64_array(x.shape), x.dim(),
        _abi.i64_array((2,) * x.dim()), int(discrete), dt, _p(y)))


def abi_pyramid(x, ys, discrete):
    ptrs = (ctypes.c_void_p * len(ys))(*[y.data_ptr() for y in ys])
    written = ctypes.c_int()
    _abi.check(_abi.lib().zt_pyramid_downsample(
        zt.default_context().handle, _abi.DTYPES[zt.dtype_of(x)], _p(x), _abi.i64_array(x.shape),
        x.dim(), _abi.i64_array((2,) * x.dim()), len(ys), int(discrete), ptrs,
        ctypes.byref(written)))
    assert written.value == len(ys)


def abi_occupancy(x, y, cells):
    _abi.check(_abi.lib().zt_chunk_occupancy(
        zt.default_context().handle, _abi.DTYPES[zt.dtype_of(x)], _p(x), _abi.i64_array(x.shape),
        x.dim(), _abi.i64_array(cells), 0, _p(y)))


def rank_case(id, kind, half, maker, dout="float32"):
    def call(xs, ys):
        zt.RankFilter(kind, half).apply(zt.DeviceArray(xs[0], (4, 16, 32)),
                                        zt.DeviceArray(ys[0], (4, 16, 32), dout))
    return Case(id, maker, [(S3, dout)], call)


S3 = (7, 33, 67)
BIG = (9, 9, 65)       # the labelling / reconstruction / watershed tests' BIG: > 1 tile per axis
EDT = (9, 9, 129)


def noise_u8(shape, density):
    return lambda seed: [((np.random.default_rng(seed).random(shape) < density).astype(np.uint8),
                          "uint8")]


def labels_u32(shape, k):
    return ints(shape, "uint32", 0, k + 1)


def seeds_u8(shape):
    def make(seed):
        rng = np.random.default_rng(seed)
        s = np.where(rng.random(shape) < 0.04, rng.choice(np.array([1, 2, 3, 255], np.uint8), shape),
                     0).astype(np.uint8)
        s.reshape(-1)[int(rng.integers(0, s.size))] = 7
        return [(s, "uint8")]
    return make


def sparse_u16(shape, cells):
    """Some cells all zero (the fill value), the others holding one non-zero element."""
    def make(seed):
        rng = np.random.default_rng(seed)
        v = np.zeros(shape, np.uint16)
        for k, idx in enumerate(grid(shape, cells)):
            if (k + seed) % 3:
                lo = [i * c for i, c in zip(idx, cells)]
                hi = [min(a + c, n) for a, c, n in zip(lo, cells, shape)]
                v[tuple(int(rng.integers(a, b)) for a, b in zip(lo, hi))] = 1 + k
        return [(v, "uint16")]
    return make


def cc_case(id, shape, connectivity):
    def call(xs, ys):
        return zt.ConnectedComponents(connectivity).apply_ndarray(xs[0], "uint32", out=ys[0])[1]
    return Case(id, noise_u8(shape, 0.45), [(shape, "uint32")], call, blocking=True)


def recon_case(id, mode, maker, **kw):
    def call(xs, ys):
        named = [zt.DeviceArray(x, (4,) * x.dim(), "uint8") for x in xs]
        return zt.Reconstruction(mode=mode, **kw).apply_ndarray(*named, out=ys[0])[1]
    return Case(id, maker, [(BIG, "uint8")], call, blocking=True)


def mask_and_marker(seed):
    """uint8 values 0 to 5, 3 % of the marker set to the mask."""
    rng = np.random.default_rng(seed)
    mask = rng.integers(0, 6, BIG).astype(np.uint8)
    return [(mask, "uint8"), (np.where(rng.random(BIG) < 0.03, mask, 0).astype(np.uint8), "uint8")]


def watershed_call(xs, ys):
    return zt.Watershed(1).apply_ndarray(xs[0], xs[1], out=ys[0])[1]


K_LABELS = 5
LBL = (3, 5, 65)


# The state-keeping operators: new_state() allocates the state it initialises, so the init entry
# point is called as new_state() calls it, on the harness's poisoned state (a stray init on
# another stream is then overwritten by the poison copy), and accumulate folds into that tensor.

def lbl_accumulate(xs, ys):
    _abi.check(_abi.lib().zt_label_statistics_init(
        zt.default_context().handle, 3, K_LABELS, 1, _p(ys[0])))
    zt.LabelStatistics(K_LABELS).accumulate(xs[0], ys[0], K_LABELS, xs[1])


def lbl_words():
    return zt.LabelStatistics(K_LABELS).state_bytes(3, K_LABELS, True) // 8


def range_accumulate(xs, ys):
    _abi.check(_abi.lib().zt_range_init(zt.default_context().handle, _p(ys[0])))
    zt.Range().accumulate(xs[0], ys[0])


def hist_accumulate(xs, ys):
    ys[0].zero_()  # Histogram.new_state's zeroing, on the harness's poisoned state
    zt.Histogram(16, 0.0, 300.0).accumulate(xs[0], ys[0])


def compare_accumulate(xs, ys):
    _abi.check(_abi.lib().zt_compare_init(zt.default_context().handle, _p(ys[0])))
    zt.Compare().accumulate(xs[0], xs[1], ys[0], base=7)


def compare_pair(shape):
    def make(seed):
        a = (np.random.default_rng(seed).random(shape, dtype=np.float32) * 300).astype(np.float32)
        b = a.copy()
        b.reshape(-1)[5 + seed % 3::97] += 1.0
        return [(a, "float32"), (b, "float32")]
    return make


def synth_f32(xs, ys):
    shape = tuple(ys[0].shape)
    _abi.check(_abi.lib().zt_synth_step_noise_f32(
        zt.default_context().handle, ctypes.c_void_p(ys[0].data_ptr()), _abi.i64_array(shape), 3,
        _abi.i64_array((9,) + shape[1:]), 3, 0x5EED2025))


def synth_u16(xs, ys):
    shape = tuple(ys[0].shape)
    _abi.check(_abi.lib().zt_synth_u16(
        zt.default_context().handle, ctypes.c_void_p(ys[0].data_ptr()), _abi.i64_array(shape), 3,
        _abi.i64_array((8,) + shape[1:]), 2, 0x5EED2025))


def halvings(shape, levels=3):
    out = []
    for _ in range(levels):
        shape = tuple(n // 2 for n in shape)
        out.append(shape)
    return out


def pyramid_case(id, shape, dtype, maker, discrete):
    return Case(id, maker, [(s, dtype) for s in halvings(shape)],
                lambda xs, ys: abi_pyramid(xs[0], ys, discrete))


EIGHT = [zt.Reencode(), zt.Rescale(0.37, -11.5), zt.Clamp(-3.0, 200.0), zt.Reencode(),
         zt.ReplaceValue(7, -2), zt.Crop([5], [900]), zt.Rescale(3.0, 1.0, add_first=True),
         zt.ReplaceValue(-3, 65535)]
EIGHT_TYPES = ["float16", "float32", "float32", "int16", "int32", "bfloat16", "int64", "uint16"]

SUB4 = ((3, 5, 4, 9), (4, 11, 9, 50))
OCC, OCC_CELLS = (3, 4, 9, 11), (2, 3, 4, 5)
G3 = (12, 40, 136)

CASES = [
    # guided filter: fused 3-D (one kernel), integer stage 1, staging casts through the scratch,
    # the separable passes, the three 4-D kernel chains, the per-chunk loop
    guided(G3, (6, 16, 64), 2),
    guided(G3, (6, 16, 64), 4),
    guided(G3, (6, 16, 64), 2, "uint16", src=ints(G3, "uint16", 0, 65536)),
    guided((6, 13, 70), (4, 8, 32), 2, "float64", "float16", eps=100.0,
           src=lambda seed: [(np.random.default_rng(seed).random((6, 13, 70)) * 120.0, "float64")]),
    guided((20, 24, 40), (8, 8, 16), 9),
    guided_subset((10, 24, 20, 72), SUB4, 2),
    guided((32, 6, 7, 20), (8, 3, 7, 10), 3),
    guided((3, 20, 21, 136), (3, 8, 8, 64), 2),
    guided_chunk_loop((14, 30, 50), (5, 16, 20), 2),
    Case("gaussian-f32", f32((9, 20, 70)), [((9, 20, 70), "float32")],
         lambda xs, ys: zt.Gaussian((1.0,) * 3, (3,) * 3).apply(
             zt.DeviceArray(xs[0], (4, 8, 32)), zt.DeviceArray(ys[0], (4, 8, 32)))),
    Case("gaussian-u16-f32", ints((9, 20, 70), "uint16", 0, 65536), [((9, 20, 70), "float32")],
         lambda xs, ys: zt.Gaussian((1.0,) * 3, (3,) * 3).apply(
             zt.DeviceArray(xs[0], (5, 8, 40)), zt.DeviceArray(ys[0], (5, 8, 40)))),
    ndarray_case("gaussian-apply_ndarray", f32((9, 20, 70)), ((9, 20, 70), "float32"),
                 lambda x: zt.Gaussian((1.0,) * 3, (3,) * 3).apply_ndarray(x)),
    Case("gradient-sobel", f32(S3), [(S3, "float32")],
         lambda xs, ys: zt.GradientMagnitude("sobel").apply(
             zt.DeviceArray(xs[0], (4, 16, 32)), zt.DeviceArray(ys[0], (4, 16, 32)))),
    Case("gradient-central-u16-f64", ints(S3, "uint16", 0, 65536), [(S3, "float64")],
         lambda xs, ys: zt.GradientMagnitude("central_difference").apply(
             zt.DeviceArray(xs[0], (4, 16, 32)), zt.DeviceArray(ys[0], (4, 16, 32)))),
    rank_case("median-1-1-1", "median", (1, 1, 1), f32(S3)),
    rank_case("minimum-1-0-2", "minimum", (1, 0, 2), f32(S3)),
    rank_case("median-2-1-1-u16-f32", "median", (2, 1, 1), ints(S3, "uint16", 0, 65536)),
    ndarray_case("maximum-apply_ndarray", f32(S3), (S3, "float32"),
                 lambda x: zt.Maximum((1, 1, 1)).apply_ndarray(x)),
    Case("summed-area-table-f32", f32((9, 7, 40)), [((9, 7, 40), "float32")],
         lambda xs, ys: zt.SummedAreaTable().apply(
             zt.DeviceArray(xs[0], (4, 4, 16)), zt.DeviceArray(ys[0], (4, 4, 16)))),
    Case("summed-area-table-u16-i64", ints((6, 7, 8, 9), "uint16", 0, 65536),
         [((6, 7, 8, 9), "int64")],
         lambda xs, ys: zt.SummedAreaTable().apply(
             zt.DeviceArray(xs[0], (3, 4, 4, 5)), zt.DeviceArray(ys[0], (3, 4, 4, 5)))),
    Case("downsample-mean", ints((37, 30, 41), "uint16", 0, 65536), [((18, 15, 20), "uint16")],
         lambda xs, ys: abi_downsample(xs[0], ys[0], False)),
    Case("downsample-mode", ints((33, 34, 35), "uint8", 0, 4), [((16, 17, 17), "uint8")],
         lambda xs, ys: abi_downsample(xs[0], ys[0], True)),
    ndarray_case("downsample-mean-apply_ndarray", ints((37, 30, 41), "uint16", 0, 65536),
                 ((18, 15, 20), "uint16"),
                 lambda x: zt.Downsample((2, 2, 2)).apply_ndarray_continuous(x)),
    pyramid_case("pyramid-mean-3-levels", (37, 50, 71), "uint16",
                 ints((37, 50, 71), "uint16", 0, 65536), False),
    pyramid_case("pyramid-mode-3-levels", (33, 34, 35), "uint8",
                 ints((33, 34, 35), "uint8", 0, 4), True),
    Case("pointwise-eight-ops", ints((1000,), "uint16", 0, 1000), [((900,), "uint16")],
         lambda xs, ys: zt.PointwiseProgram(EIGHT, "uint16", EIGHT_TYPES, (1000,)).run(
             xs[0], ys[0])),
    Case("reencode-f32-i16", f32(S3), [(S3, "int16")],
         lambda xs, ys: zt.Reencode().apply(zt.DeviceArray(xs[0], S3), zt.DeviceArray(ys[0], S3))),
    ndarray_case("reencode_cast-f32-f16", f32(S3), (S3, "float16"),
                 lambda x: zt.filter.reencode_cast(x, "float16")),
    Case("arithmetic-add-f32-u16", both(f32(S3), ints(S3, "uint16", 0, 65536)), [(S3, "float32")],
         quiet(lambda xs, ys: zt.Arithmetic("add").apply_ndarray(xs[0], xs[1], out=ys[0]))),
    cc_case("connected-3d", EDT, 1),
    cc_case("connected-4d-offset-table", (3, 4, 9, 17), 2),
    Case("distance-transform", noise_u8(EDT, 0.9), [(EDT, "float32")],
         quiet(lambda xs, ys: zt.DistanceTransform().apply_ndarray(xs[0], out=ys[0]))),
    Case("label-statistics-init-accumulate", both(labels_u32(LBL, K_LABELS),
                                                  ints(LBL, "uint16", 0, 65536)),
         lambda: [((lbl_words(),), "int64")], lbl_accumulate),
    Case("label-statistics-finish", both(labels_u32(LBL, K_LABELS), ints(LBL, "uint16", 0, 65536)),
         [], lambda xs, ys: zt.LabelStatistics().apply_ndarray(xs[0], xs[1]), blocking=True),
    Case("label-size-filter", labels_u32(LBL, 40), [(LBL, "uint32")],
         lambda xs, ys: zt.LabelSizeFilter(20).apply_ndarray(xs[0], out=ys[0])[1], blocking=True),
    recon_case("reconstruction-fill-holes", "fill_holes", noise_u8(BIG, 0.6)),
    recon_case("reconstruction-h-maxima", "h_maxima", ints(BIG, "uint8", 0, 6), h=2.0),
    recon_case("reconstruction-marker", "marker", mask_and_marker),
    Case("watershed", both(ints(BIG, "uint8", 0, 4), seeds_u8(BIG)), [(BIG, "uint8")],
         watershed_call, blocking=True),
    Case("range-init-accumulate", f32(S3), [((2,), "int64")], range_accumulate),
    Case("range-finish", f32(S3), [], lambda xs, ys: zt.Range().apply_ndarray(xs[0]),
         blocking=True),
    Case("histogram-accumulate", f32(S3), [((16,), "int64")], hist_accumulate),
    Case("histogram-finish", f32(S3), [],
         lambda xs, ys: zt.Histogram(16, 0.0, 300.0).apply_ndarray(xs[0]), blocking=True),
    Case("compare-init-accumulate", compare_pair(S3), [((2,), "int64")], compare_accumulate),
    Case("compare-finish", compare_pair(S3), [],
         lambda xs, ys: zt.Compare().apply_ndarray(xs[0], xs[1]), blocking=True),
    Case("chunk-occupancy", sparse_u16(OCC, OCC_CELLS), [((2, 2, 3, 3), "uint8")],
         lambda xs, ys: abi_occupancy(xs[0], ys[0], OCC_CELLS)),
    Case("chunk-occupancy-cpu", sparse_u16(OCC, OCC_CELLS), [],
         lambda xs, ys: zt.chunk_occupancy(xs[0], OCC_CELLS).cpu().numpy(), blocking=True),
    Case("synth_step_noise_f32", lambda seed: [], [((5, 33, 70), "float32")], synth_f32),
    Case("synth_u16", lambda seed: [], [((4, 5, 6), "uint16")], synth_u16),
]


# ---- the harness -------------------------------------------------------------------------------------

def default_stream_runs(case, staging):
    """Step 1: (want bytes, what the call returned, host ms of the second of two unsynchronised
    calls); the two runs must agree, byte for byte."""
    import torch

    def fresh():
        return [s.clone() for s in staging], [poisoned(sh, dt) for sh, dt in case.outputs]

    (xs1, ys1), (xs2, ys2) = fresh(), fresh()
    torch.cuda.synchronize()
    h1 = case.call(xs1, ys1)
    t0 = time.perf_counter()
    h2 = case.call(xs2, ys2)
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    want, again = [raw(y) for y in ys1], [raw(y) for y in ys2]
    assert want == again and canon(h1) == canon(h2), \
        f"{case.id}: two runs on the default stream differ"
    return want, h1, host_ms


def scrub(case):
    """The same call on other data on the default stream: afterwards neither the context's scratch
    nor a cached allocation holds the intermediates or the result of the case's own data."""
    import torch
    xs = [to_dev(a, dt) for a, dt in case.inputs(1)]
    case.call(xs, [poisoned(sh, dt) for sh, dt in case.outputs])
    torch.cuda.synchronize()


def run_delayed(case):
    import torch
    ins = case.inputs(0)
    staging = [to_dev(a, dt) for a, dt in ins]
    want, host_want, host_ms = default_stream_runs(case, staging)
    for y, (sh, dt) in zip(want, case.outputs):
        assert y != raw(poisoned(sh, dt)), f"{case.id}: the call leaves its output untouched"
    delay = delay_for(host_ms)
    for factor in (1, 4):
        scrub(case)
        xs = [poisoned(tuple(a.shape), dt) for a, dt in ins]
        ys = [poisoned(sh, dt) for sh, dt in case.outputs]
        poison = [y.clone() for y in ys]
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        after_delay = torch.cuda.Event()
        with torch.cuda.stream(s):
            Delay.enqueue(delay * factor)
            after_delay.record()
            for x, st in zip(xs, staging):
                x.copy_(st)
            for y, p in zip(ys, poison):
                y.copy_(p)
            host_got = case.call(xs, ys)  # no ctx: default_context() follows s
            held = not after_delay.query()
        s.synchronize()
        print(f"[streams] {case.id}: host {host_ms:.3f} ms, delay {delay * factor:.1f} ms, "
              f"{'blocking' if case.blocking else 'held' if held else 'NOT held'}")
        for k, (y, w) in enumerate(zip(ys, want)):
            got = raw(y)
            assert got == w, f"{case.id}: output {k} on a side stream: {first_difference(got, w)}"
        assert canon(host_got) == canon(host_want), \
            f"{case.id}: returned {host_got!r} on a side stream, {host_want!r} on the default one"
        if case.blocking or held:
            return
    pytest.fail(f"{case.id}: inconclusive: the delay of {delay * 4:.1f} ms had passed when the "
                "call returned, twice")


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_delayed_producer_on_a_side_stream(case):
    run_delayed(case)


def test_the_case_ids_are_unique():
    assert len({c.id for c in CASES}) == len(CASES)


# ---- a context's own stream --------------------------------------------------------------------------

def ctx_stream(ctx) -> int:
    p = ctypes.c_void_p()
    _abi.check(_abi.lib().zt_ctx_get_stream(ctx.handle, ctypes.byref(p)))
    return p.value or 0


OWN = {
    "guided-fused": (f32(G3), [(G3, "float32")],
                     lambda xs, ys, ctx: zt.GuidedFilter(0.5, 4).apply(
                         zt.DeviceArray(xs[0], (6, 16, 64)), zt.DeviceArray(ys[0], (6, 16, 64)),
                         ctx=ctx)),
    "gaussian": (ints((9, 20, 70), "uint16", 0, 65536), [((9, 20, 70), "float32")],
                 lambda xs, ys, ctx: zt.Gaussian((1.0,) * 3, (3,) * 3).apply(
                     zt.DeviceArray(xs[0], (4, 8, 32)), zt.DeviceArray(ys[0], (4, 8, 32)),
                     ctx=ctx)),
    "pyramid": (ints((37, 50, 71), "uint16", 0, 65536),
                [(s, "uint16") for s in halvings((37, 50, 71))],
                lambda xs, ys, ctx: zt.pyramid(xs[0], (2, 2, 2), max_levels=3, ctx=ctx)),
    "connected": (noise_u8(EDT, 0.45), [(EDT, "uint32")],
                  lambda xs, ys, ctx: zt.ConnectedComponents(1).apply_ndarray(
                      xs[0], "uint32", ctx=ctx, out=ys[0])[1]),
}


def own_run(call, xs, outputs, ctx, finish):
    """(bytes of every output, host value) of one call on `ctx` (None: the default context),
    waited for with `finish`. The outputs are the poisoned tensors handed in, or the tensors the
    call returns (pyramid)."""
    import torch
    ys = [poisoned(sh, dt) for sh, dt in outputs]
    torch.cuda.synchronize()  # the poison is in place before another stream writes over it
    res = call(xs, ys, ctx)
    finish()
    if isinstance(res, list):
        assert [tuple(t.shape) for t in res] == [tuple(sh) for sh, _ in outputs]
        return [raw(t) for t in res], None
    return [raw(y) for y in ys], res


@pytest.mark.parametrize("name", list(OWN))
def test_a_context_on_its_own_stream(name):
    """Context(0) with no stream runs on its own non-blocking stream, and ctx.synchronize() waits
    for it: the same bytes as on the default stream, also after the round trip
    set_stream(torch's stream) -> zt_ctx_use_own_stream, which zt_ctx_get_stream reports."""
    import torch
    maker, outputs, call = OWN[name]
    xs = [to_dev(a, dt) for a, dt in maker(0)]
    want = own_run(call, xs, outputs, None, torch.cuda.synchronize)
    ctx = zt.Context(0)
    try:
        own = ctx_stream(ctx)
        assert own != 0 and own != torch.cuda.current_stream().cuda_stream
        assert own_run(call, xs, outputs, ctx, ctx.synchronize) == want, \
            f"{name} on the context's own stream"
        ctx.set_stream(torch.cuda.current_stream())
        assert ctx_stream(ctx) == torch.cuda.current_stream().cuda_stream
        _abi.check(_abi.lib().zt_ctx_use_own_stream(ctx.handle))
        assert ctx_stream(ctx) == own
        assert own_run(call, xs, outputs, ctx, ctx.synchronize) == want, \
            f"{name} after the round trip"
    finally:
        torch.cuda.synchronize()
        ctx.close()


# ---- a switch of the context's stream orders the two streams -------------------------------------------

SWITCH_SHAPE, SWITCH_CHUNK, SWITCH_R = (20, 24, 40), (8, 8, 16), 9


def switch_op(x, y, ctx=None):
    """The separable guided filter: several passes through the context's scratch."""
    zt.GuidedFilter(0.5, SWITCH_R).apply(zt.DeviceArray(x, SWITCH_CHUNK),
                                         zt.DeviceArray(y, SWITCH_CHUNK), ctx=ctx)


def switch_data():
    """(x1, x2, their default-stream bytes, two poisoned outputs)."""
    import torch
    xs = [to_dev(f32(SWITCH_SHAPE)(seed)[0][0], "float32") for seed in (0, 1)]
    want = []
    for x in xs:
        y = poisoned(SWITCH_SHAPE, "float32")
        switch_op(x, y)
        torch.cuda.synchronize()
        want.append(raw(y))
    assert want[0] != want[1]
    ys = [poisoned(SWITCH_SHAPE, "float32") for _ in xs]
    torch.cuda.synchronize()
    return xs, want, ys


def check_switch(what, ys, want, eA, eB, held):
    ms = eA.elapsed_time(eB)
    print(f"[streams] {what}: the delay {'held' if held else 'had NOT held'} while both calls "
          f"were issued, eA -> eB {ms:.3f} ms")
    assert raw(ys[0]) == want[0], "op1 on stream A: " + first_difference(raw(ys[0]), want[0])
    assert raw(ys[1]) == want[1], "op2 after the switch: " + first_difference(raw(ys[1]), want[1])
    assert ms >= 0, (f"{what}: op2 finished {-ms:.3f} ms before op1 on the stream the context "
                     "left: the switch did not order them")
    if not held:  # op2 was issued after A's delay: the order above proves nothing; never a pass
        pytest.fail(f"{what}: inconclusive: A's delay had passed before both calls were issued")


def test_a_stream_switch_orders_the_new_stream_after_the_old():
    """The default context under torch.cuda.stream(A): a delay, then op1. Then, at once, under
    torch.cuda.stream(B), op2 on other data: the context switches from A to B, and its one scratch
    buffer is only safe when B's work runs after A's. Both results equal their default-stream
    bytes, and B's call finishes after A's. Without the ordering op2 runs inside A's delay."""
    import torch
    (x1, x2), want, ys = switch_data()
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    eA, eB = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    after_delay = torch.cuda.Event()
    with torch.cuda.stream(A):
        Delay.enqueue(delay_for(0.0))
        after_delay.record()
        switch_op(x1, ys[0])
        eA.record()
    with torch.cuda.stream(B):
        switch_op(x2, ys[1])
        eB.record()
    held = not after_delay.query()
    A.synchronize()
    B.synchronize()
    check_switch("set_stream A -> B", ys, want, eA, eB, held)


def test_two_switches_in_a_row_keep_the_order():
    """op1 on A behind the delay, then set_stream(B) and set_stream(C) with no call between them,
    then op2 on C: no entry point ran on B, yet C's work is ordered after A's (the order is carried
    through the switch that had nothing to record)."""
    import torch
    (x1, x2), want, ys = switch_data()
    A, B, C = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    eA, eC = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    after_delay = torch.cuda.Event()
    ctx = zt.Context(0)
    try:
        switch_op(x2, poisoned(SWITCH_SHAPE, "float32"), ctx)  # the scratch is allocated now
        ctx.synchronize()
        ctx.set_stream(A)
        with torch.cuda.stream(A):
            Delay.enqueue(delay_for(0.0))
            after_delay.record()
            switch_op(x1, ys[0], ctx)
            eA.record()
        ctx.set_stream(B)
        ctx.set_stream(C)
        assert ctx_stream(ctx) == C.cuda_stream
        switch_op(x2, ys[1], ctx)
        eC.record(C)
        held = not after_delay.query()
        A.synchronize()
        C.synchronize()
        check_switch("set_stream A -> B -> C", ys, want, eA, eC, held)
    finally:
        torch.cuda.synchronize()
        ctx.close()


def test_the_return_to_the_own_stream_is_ordered_too():
    """The same with an explicit context that leaves stream A for its own stream
    (zt_ctx_use_own_stream): op2 on the own stream finishes after op1 on A."""
    import torch
    (x1, x2), want, ys = switch_data()
    A = torch.cuda.Stream()
    eA, eB = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    after_delay = torch.cuda.Event()
    ctx = zt.Context(0)
    try:
        own = torch.cuda.ExternalStream(ctx_stream(ctx))
        switch_op(x2, poisoned(SWITCH_SHAPE, "float32"), ctx)  # the scratch is allocated now
        ctx.synchronize()
        ctx.set_stream(A)
        with torch.cuda.stream(A):
            Delay.enqueue(delay_for(0.0))
            after_delay.record()
            switch_op(x1, ys[0], ctx)
            eA.record()
        _abi.check(_abi.lib().zt_ctx_use_own_stream(ctx.handle))
        switch_op(x2, ys[1], ctx)
        eB.record(own)
        held = not after_delay.query()
        A.synchronize()
        ctx.synchronize()
        check_switch("stream A -> use_own_stream", ys, want, eA, eB, held)
    finally:
        torch.cuda.synchronize()
        ctx.close()


# ---- two chains on two streams, one context each -----------------------------------------------------

def test_two_chains_on_two_streams_with_a_context_each():
    """gaussian -> median -> clamp on stream A and the same chain on other data on stream B, each
    with its own Context, issued interleaved step by step with no synchronisation until the end
    (A starts with a delay, so B's whole chain runs while A's is pending): both equal their
    default-stream results. The header's "one context per (host thread, device)" in use."""
    import torch
    shape = (9, 20, 70)
    steps = [
        lambda x, ctx: zt.Gaussian((1.0,) * 3, (3,) * 3).apply_ndarray(x, ctx=ctx),
        lambda x, ctx: zt.Median((1, 1, 1)).apply_ndarray(x, ctx=ctx),
        lambda x, ctx: zt.Clamp(40.0, 250.0).apply_ndarray(x, ctx=ctx),
    ]
    data = [to_dev(f32(shape)(seed)[0][0], "float32") for seed in (0, 1)]
    want = []
    for x in data:
        for step in steps:
            x = step(x, None)
        torch.cuda.synchronize()
        want.append(raw(x))
    assert want[0] != want[1]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    ctxs = [zt.Context(0, s) for s in streams]
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(streams[0]):
            Delay.enqueue(delay_for(0.0))
        cur, keep = list(data), []
        for step in steps:
            for k in (0, 1):
                with torch.cuda.stream(streams[k]):  # the results are allocated on their stream
                    cur[k] = step(cur[k], ctxs[k])
                    keep.append(cur[k])
        for s in streams:
            s.synchronize()
        for k in (0, 1):
            got = raw(cur[k])
            assert got == want[k], f"chain {k}: " + first_difference(got, want[k])
    finally:
        torch.cuda.synchronize()
        for c in ctxs:
            c.close()
