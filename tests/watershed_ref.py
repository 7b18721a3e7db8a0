"""numpy restatement of the seeded watershed, the semantics the GPU path is held
to bit for bit.

watershed(relief, seeds, connectivity=1, descending=False, foreground_only=False) -> labels

The relief is compared only through the rank filters' total order (tests/rank_ref.py: to_key), the
keys complemented when `descending`: the flood key. Every non-zero element of `seeds` (an integer
type) is a label, carried as storage bits; `labels` has the seeds' type. The domain D is every
element, or with `foreground_only` every element whose relief is non-zero by the labelling's rule
(tests/ccl_ref.py: foreground). Elements outside D get 0 and are never crossed; a seed outside D is
ignored. Neighbours are the labelling's.

  1. pass value   c[p] = the least, over paths in D from a seed to p, of the greatest key on the
                  path, both ends included: the reconstruction by erosion of J0 (the key at seeds,
                  the greatest key elsewhere) under the key (the greatest key outside D)
  2. distance     d[p] = 0 at seeds and where a D-neighbour has a smaller c, else 1 + the least d
                  over D-neighbours of equal c; NONE where no such chain exists: exactly the
                  elements of D that no seed is connected to in D
  3. parent       a seed is its own; d = 0: the D-neighbour of least (c, linear C index) among
                  those of smaller c; d > 0: the neighbour of least linear index with equal c and
                  d one less
  4. labels       labels[p] = seeds[root(p)], 0 where d is NONE or p is outside D

Arrays are storage arrays as the oracle holds them: bool as uint8, bfloat16 and float16 as uint16.
"""
import numpy as np

from tests import ccl_ref, recon_ref
from tests.rank_ref import to_key

NONE = np.int64(-1)  # "no distance" / "no parent" in this file's int64 arrays


def flood_key(relief, dt: str, descending: bool = False) -> np.ndarray:
    k = to_key(relief, dt).reshape(np.shape(relief))
    return ~k if descending else k


def domain(relief, dt: str, foreground_only: bool) -> np.ndarray:
    if foreground_only:
        return ccl_ref.foreground(np.asarray(relief), dt)
    return np.ones(np.shape(relief), dtype=bool)


def pass_values(key: np.ndarray, seeded: np.ndarray, dom: np.ndarray, connectivity: int):
    """(c, sweeps): the least over paths in D from a seed of the greatest key on the path; the
    greatest key of the type where no seed reaches and outside D."""
    # reconstruct_keys dilates: on complemented keys that is the erosion
    under = np.where(dom, ~key, key.dtype.type(0))
    j0 = np.where(seeded, under, key.dtype.type(0))
    out, sweeps = recon_ref.reconstruct_keys(j0, under, connectivity)
    return ~out, sweeps


def _pairs(shape, connectivity):
    """(offset, destination slices, source slices) in the order of the neighbours' linear
    indices."""
    return [(d,) + recon_ref._shifted(shape, d)
            for d in recon_ref.neighbour_offsets(len(shape), connectivity)]


def plateau_distance(c: np.ndarray, seeded: np.ndarray, dom: np.ndarray, connectivity: int):
    """(d as int64 with NONE, sweeps)."""
    big = np.int64(c.size + 1)
    pairs = _pairs(c.shape, connectivity)
    lower = np.zeros(c.shape, dtype=bool)
    for _, dst, src in pairs:
        lower[dst] |= dom[dst] & dom[src] & (c[src] < c[dst])
    fixed = seeded | lower
    d = np.where(fixed, np.int64(0), big)
    sweeps = 0
    while d.size:
        sweeps += 1
        new = d.copy()
        for _, dst, src in pairs:
            ok = dom[dst] & dom[src] & (c[src] == c[dst]) & ~fixed[dst]
            np.minimum(new[dst], np.where(ok, d[src] + 1, big), out=new[dst])
        new = np.minimum(new, big)
        if np.array_equal(new, d):
            break
        d = new
    return np.where(dom & (d < big), d, NONE), sweeps


def parents(c: np.ndarray, d: np.ndarray, seeded: np.ndarray, dom: np.ndarray,
            connectivity: int) -> np.ndarray:
    """Linear indices as int64, NONE outside the forest."""
    index = np.arange(c.size, dtype=np.int64).reshape(c.shape)
    parent = np.full(c.shape, NONE, dtype=np.int64)
    best = c.copy()  # d = 0: the smallest c seen so far; a neighbour has to be below it
    reached = dom & (d != NONE)
    for _, dst, src in _pairs(c.shape, connectivity):
        here = reached[dst] & ~seeded[dst] & dom[src]
        down = here & (d[dst] == 0) & (c[src] < best[dst])
        level = here & (d[dst] > 0) & (parent[dst] == NONE) & (c[src] == c[dst]) & \
            (d[src] == d[dst] - 1)
        best[dst] = np.where(down, c[src], best[dst])
        parent[dst] = np.where(down | level, index[src], parent[dst])
    parent[seeded] = index[seeded]
    return parent


def roots(parent: np.ndarray):
    """(root of every element or NONE, jumps): P' = P[P] until a jump changes nothing; the jumps
    count that last one."""
    p = parent.ravel().copy()
    jumps = 0
    while p.size:
        jumps += 1
        nxt = np.where(p == NONE, NONE, p[np.maximum(p, 0)])
        if np.array_equal(nxt, p):
            break
        p = nxt
    return p.reshape(parent.shape), jumps


def watershed(relief, dt: str, seeds, connectivity: int = 1, descending: bool = False,
              foreground_only: bool = False, with_steps: bool = False):
    """Labels in the seeds' storage type; with_steps: (labels, {"c", "d", "parent", "root",
    "rounds": (pass sweeps, distance sweeps, jumps)})."""
    relief, seeds = np.asarray(relief), np.asarray(seeds)
    assert relief.shape == seeds.shape, (relief.shape, seeds.shape)
    assert seeds.dtype.kind in "iu", seeds.dtype
    nd = relief.ndim
    if nd < 1 or not 1 <= int(connectivity) <= nd:
        raise ValueError(f"connectivity {connectivity} not in [1, {nd}]")
    dom = domain(relief, dt, foreground_only)
    seeded = dom & (seeds != 0)
    key = flood_key(relief, dt, descending)
    c, s0 = pass_values(key, seeded, dom, int(connectivity))
    d, s1 = plateau_distance(c, seeded, dom, int(connectivity))
    parent = parents(c, d, seeded, dom, int(connectivity))
    root, jumps = roots(parent)
    flat = seeds.ravel()
    labels = np.where(root.ravel() == NONE, flat.dtype.type(0),
                      flat[np.maximum(root.ravel(), 0)]).astype(seeds.dtype).reshape(seeds.shape)
    if with_steps:
        return labels, {"c": c, "d": d, "parent": parent, "root": root,
                        "rounds": (s0, s1, jumps)}
    return labels
