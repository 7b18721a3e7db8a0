"""A store array into HBM and back, overlapped chunk row by chunk row: the read and write of
everything that runs device-resident (zarrs_filter's chains, zarrs_ome's levels, the
whole-array connected-component labelling of store.py)."""
from __future__ import annotations

import os

import numpy as np

from . import store as S


def _row_spans(start0: int, n0: int, chunk0: int) -> list:
    """[a, b) pieces of the axis-0 range [start0, start0 + n0) cut at the chunk grid, so that
    every chunk (or shard) is decoded / encoded by one piece only."""
    spans, a, end = [], start0, start0 + n0
    while a < end:
        b = min((a // chunk0 + 1) * chunk0, end)
        spans.append((a, b))
        a = b
    return spans


def _read_pieces(start, shape, chunk_shape, esz: int) -> list:
    """The pieces a box read is pipelined in: chunk rows of axis 0, cut along axis 1 at the chunk
    grid into pieces of about ZT_READ_PIECE_KB (default 512 MiB; 0: whole rows). Each chunk is
    still decoded once, but a pinned buffer holds a piece instead of a whole chunk row: pinning
    three 2 GB rows per process made 2048^3 u16 box reads 2x slower
    (profiles/r04_octant_workers*.json). [(a, b, ya, yb)]; ya, yb = 0, 1 for 1-D arrays."""
    nd = len(shape)
    spans = _row_spans(start[0], shape[0], int(chunk_shape[0])) if shape[0] > 0 else []
    if nd < 2:
        return [(a, b, 0, 1) for a, b in spans]
    target = int(os.environ.get("ZT_READ_PIECE_KB", "524288")) << 10
    plane2 = int(np.prod(shape[2:])) if nd > 2 else 1
    cy = int(chunk_shape[1])
    out = []
    for a, b in spans:
        if target > 0:
            m = max(1, target // max(1, (b - a) * cy * plane2 * esz))
            out += [(a, b, ya, yb) for ya, yb in _row_spans(start[1], shape[1], cy * m)]
        else:
            out.append((a, b, start[1], start[1] + shape[1]))
    return out


def read_to_device(path, device: int, nthreads: int = 0, start=None, shape=None):
    """The box [start, start + shape) of a store array (the whole array by default) decoded into
    HBM, overlapped chunk row by chunk row: a host thread decodes row k+1
    into one of three pinned row buffers while row k is copied host-to-device on a side stream
    (the reference copies level 0 then streams it chunk by chunk, zarrs_ome.rs:341-366,
    631-714). Each chunk is decoded once. bfloat16 arrays come back as torch.bfloat16."""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from . import filter as F
    info = S.open_array(path)
    nd = info.ndim
    start = [0] * nd if start is None else [int(v) for v in start]
    shape = list(info.shape) if shape is None else [int(v) for v in shape]
    store_dt = "uint16" if info.data_type == "bfloat16" else info.data_type
    tdt = F.torch_dtype(store_dt)
    dev = torch.device("cuda", device)
    x = torch.empty(tuple(shape), dtype=tdt, device=dev)
    if all(v > 0 for v in shape):
        pieces = _read_pieces(start, shape, info.chunk_shape, x.element_size())

        def pshape(p):
            a, b, ya, yb = p
            return [b - a, yb - ya] + shape[2:] if nd >= 2 else [b - a]

        n_max = max(int(np.prod(pshape(p))) for p in pieces)
        nbuf = min(3, len(pieces))
        bufs = [torch.empty((n_max,), dtype=tdt, pin_memory=True) for _ in range(nbuf)]
        evs = [None] * nbuf
        stream = torch.cuda.Stream(device=dev)
        # x was allocated on the caller's current stream: order the copies after any work that
        # stream still has queued on the block the caching allocator handed back
        stream.wait_stream(torch.cuda.current_stream(dev))

        def decode(k):
            a, b, ya, yb = pieces[k]
            ps = pshape(pieces[k])
            h = bufs[k % nbuf][:int(np.prod(ps))].view(ps)
            out = h.numpy()
            if info.data_type == "bool":  # a bool array travels as uint8 on the device
                out = out.view(np.bool_)
            S.read_array(path, [a, ya] + start[2:] if nd >= 2 else [a], ps, nthreads=nthreads,
                         out=out)
            return h

        with ThreadPoolExecutor(1) as ex:
            fut = ex.submit(decode, 0)
            for k, (a, b, ya, yb) in enumerate(pieces):
                h = fut.result()
                if k + 1 < len(pieces):
                    ev = evs[(k + 1) % nbuf]
                    if ev is not None:
                        ev.synchronize()  # the H2D that last read this buffer has finished
                    fut = ex.submit(decode, k + 1)
                with torch.cuda.stream(stream):
                    if nd >= 2:
                        x[a - start[0]:b - start[0], ya - start[1]:yb - start[1]].copy_(
                            h, non_blocking=True)
                    else:
                        x[a - start[0]:b - start[0]].copy_(h, non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(stream)
                evs[k % nbuf] = ev
        stream.synchronize()
    return x.view(torch.bfloat16) if info.data_type == "bfloat16" else x


def write_from_device(path, x, nthreads: int = 0, start=None) -> int:
    """A device tensor (the box at `start`, default the whole array at `path`) into the store,
    overlapped chunk row by chunk row: row k+1 is copied device-to-host into one of two pinned
    buffers while a host thread encodes row k. When the calling thread elides empty chunks
    (store.set_store_empty_chunks(False)) the row's inner chunks are tested on the device first
    (filter.chunk_occupancy): a row of nothing but the fill value is not copied, and the encoder
    gets the map. Returns the number of chunks elided."""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    if x.dtype == torch.bfloat16:
        x = x.view(torch.uint16)
    info = S.open_array(path)
    nd = x.dim()
    start = [0] * nd if start is None else [int(v) for v in start]
    shape = list(x.shape)
    if not shape or any(v == 0 for v in shape):
        return
    spans = _row_spans(start[0], shape[0], int(info.chunk_shape[0]))
    plane = int(np.prod(shape[1:])) if nd > 1 else 1
    rows = max(b - a for a, b in spans)
    nbuf = min(2, len(spans))
    bufs = [torch.empty((rows * plane,), dtype=x.dtype, pin_memory=True) for _ in range(nbuf)]
    futs = [None] * nbuf
    store_all = S.store_empty_chunks()
    fill = None
    if not store_all:  # the fill value's bits, as the tensor's type (bfloat16 travels as uint16)
        from . import filter as F
        fill = hex(F.fill_value_bits(S.fill_value_of(path), info.data_type))
    elided = 0

    def write(h, origin, occ):  # on the encoder thread, with the caller's setting
        S.set_store_empty_chunks(store_all)
        S.write_array(path, h, origin, nthreads, occupied=occ)
        return S.last_elided()[0]

    def skip(origin, row_shape):  # a row of fill: no copy; its files, if any, are removed
        S.set_store_empty_chunks(store_all)
        S.write_empty(path, origin, row_shape, nthreads)
        return S.last_elided()[0]

    with ThreadPoolExecutor(1) as ex:
        for k, (a, b) in enumerate(spans):
            if futs[k % nbuf] is not None:
                elided += futs[k % nbuf].result()  # this buffer's previous row is encoded
                futs[k % nbuf] = None
            row = x[a - start[0]:b - start[0]]
            occ = None
            if not store_all:
                occ = F.chunk_occupancy(row, info.inner_chunk_shape, fill).cpu().numpy()
                if not occ.any():
                    futs[k % nbuf] = ex.submit(skip, [a] + start[1:], [b - a] + shape[1:])
                    continue
            h = bufs[k % nbuf][:(b - a) * plane].view([b - a] + shape[1:])
            h.copy_(row)
            futs[k % nbuf] = ex.submit(write, h.numpy(), [a] + start[1:], occ)
        for f in futs:
            if f is not None:
                elided += f.result()
    return elided
